"""rf_attention against the exact integer-operand cases of tests/attn_exact_refs.py: every launch plan of attention.hip has cases that name it and
assert it through rf_attention_plan BEFORE launching (a dispatch retune that moves a case to another kernel fails here by name), every output
element of every (batch, head, query, column) is compared with the fp64 reference under the derived tolerance (one store rounding of a 16-bit
result plus 2^-18 of the softmax-weighted |v|; 2^-16 of it for fp32 and x3), and q / k / v / out are slices of NaN-filled allocations -- NaN pad
columns beside every operand, NaN rows behind the last query and the last key, ldo > C -- that must be bit-identical afterwards outside the
output region.  One launch per case; each case prints its ledger line (DESIGN.md carries the table)."""
import pytest
import torch

import attn_exact_refs as R
from reface_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                   # (cell, dtype) -> worst err / limit of this run


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_attention_exact(c):
    B, heads, d, Nq = c["B"], c["heads"], c["d"], c["Nq"]
    q, k, v, out, alloc, (q64, k64, v64) = R.buffers(c, DEV)
    x3 = c["dt"] == "x3"
    pl = ops.attention_plan(q, k, v, out, heads=heads, x3=x3)
    lost = R.plan_matches(pl, c["expect"])
    assert not lost, f"the cell {c['cell']} lost its case {c['id']}: {lost}"
    assert R.representable(q64) and R.representable(k64) and R.representable(v64)
    before = {n: R.bits(t).clone() for n, t in alloc.items()}
    ops.attention(q, k, v, out, heads=heads, scale=ops.LN2, x3=x3)()
    torch.cuda.synchronize()
    # ---- guards: the operands and everything around them untouched, the output allocation untouched outside [B, Nq, C]
    for n, t in alloc.items():
        now = R.bits(t).clone()
        if n == "out":
            now[:, :Nq, R.PAD:R.PAD + heads * d] = 0
            before[n][:, :Nq, R.PAD:R.PAD + heads * d] = 0
        assert torch.equal(now, before[n]), f"{c['id']}: {int((now != before[n]).sum())} guard elements of the {n} allocation changed"
    assert bool(torch.isfinite(out.float()).all()), f"{c['id']}: {int((~torch.isfinite(out.float())).sum())} outputs are not finite"
    got = out.to(R.F64).view(B, Nq, heads, d).permute(0, 2, 1, 3).reshape(B * heads, Nq, d)
    # ---- every element against the fp64 reference (on the device, 64 heads at a time; the operand conditions are asserted inside)
    worst, bad = 0.0, 0
    for g0 in range(0, B * heads, 64):
        s = slice(g0, g0 + 64)
        ref, A, _, _ = R.reference(q64[s], k64[s], v64[s], check=True)
        lim = R.limit_of(c, ref, A)
        err = (got[s] - ref).abs()
        bad += int((err > lim).sum())
        worst = max(worst, (err / lim.clamp(min=1e-300)).max().item())
    key = (c["cell"], c["dt"])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"[attn_exact] {c['id']} | {' '.join(f'{w}={pl[w]}' for w in ops.ATTN_PLAN_KEYS)} | {got.numel()} outputs | worst err/limit {worst:.4f}")
    assert bad == 0, f"{c['id']}: {bad} of {got.numel()} outputs beyond the tolerance, worst err/limit {worst:.3f}"


def test_ledger():
    """the worst err / limit per plan cell and dtype of this run (a figure for DESIGN.md; the bound is asserted per case above)"""
    for (cell, dt), w in sorted(WORST.items()):
        print(f"[attn_exact] ledger {cell} {dt}: worst err/limit {w:.4f}")
