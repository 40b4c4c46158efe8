"""ops.fold_ups_weight: a 3x3 convolution behind a nearest-2x upsampling equals four 2x2 phase convolutions of the stored image on folded weights.
The identity is exact; in float64 the summation order is the only difference, hence the 1e-12 bound (relative to the output's maximum)."""
import pytest
import torch
import torch.nn.functional as F

from reface_amd import ops


def phase_conv(x, wf, b):
    """The folded form in plain torch: x [B, C, H, W], wf [4, N, 2, 2, C] (fold_ups_weight's layout) -> [B, N, 2H, 2W].
    Phase (py, px) is a 2x2 window with top / left padding (1 - py, 1 - px) over the zero-extended source; the phases interleave."""
    B, C, H, W = x.shape
    out = x.new_zeros((B, wf.shape[1], 2 * H, 2 * W))
    for py in range(2):
        for px in range(2):
            w = wf[2 * py + px].permute(0, 3, 1, 2)                     # [N, C, 2, 2]
            xp = F.pad(x, (1 - px, px, 1 - py, py))                     # (left, right, top, bottom) -> (H + 1) x (W + 1)
            out[:, :, py::2, px::2] = F.conv2d(xp, w, b)
    return out


# (non-square and odd: H / W swaps and border mistakes; 1x1: all border)
@pytest.mark.parametrize("B,C,N,H,W", [(2, 8, 5, 4, 4), (1, 3, 4, 3, 5), (1, 2, 2, 1, 1)])
def test_fold_matches_upsampled_conv_float64(B, C, N, H, W):
    g = torch.Generator().manual_seed(1234 + 10 * H + W)
    x = torch.randn((B, C, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn((N,), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    wf = ops.fold_ups_weight(w)
    assert wf.shape == (4, N, 2, 2, C) and wf.dtype == torch.float64
    got = phase_conv(x, wf, b)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_fold_fp32_masters_and_packing():
    """fp32 in -> fp32 out, the float64 fold rounded once per sum; pack_ups_weight: [4, N, 4 C], k = (ty * 2 + tx) * C + c, rounded once more."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn((3, 64, 3, 3), generator=g)
    f = ops.fold_ups_weight(w)
    assert f.dtype == torch.float32 and f.shape == (4, 3, 2, 2, 64)
    f64 = ops.fold_ups_weight(w.double())
    # fp32 sums of at most four terms: at most three roundings of 2^-24 relative to the running sum (<= 4 max|w|)
    assert (f.double() - f64).abs().max().item() <= 3 * 2.0 ** -24 * 4 * w.abs().max().item()
    p = ops.pack_ups_weight(w, torch.bfloat16)
    assert p.shape == (4, 3, 256) and p.dtype == torch.bfloat16 and p.is_contiguous()
    assert torch.equal(p[3, 1, 64:128], f[3, 1, 0, 1, :].to(torch.bfloat16))
    assert torch.equal(p[1, 2, 128:192], f[1, 2, 1, 0, :].to(torch.bfloat16))
