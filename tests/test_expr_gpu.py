"""The expression score on the GPU (reface_amd/csrc/expr.hip, the ReLU-after-residual epilogue of rf_conv_gemm, reface_amd/exprscore.py,
eval_tool/Expression/expression_compare_face_recon.py) against the reference's own outputs (tests/golden/expr.npz) and the host restatements
that tests/test_expr_cpu.py pins to them.

The yardstick of the end-to-end gates is the reference itself: e_ref = max |exp_f32 - exp_f64| of the fixture is what ONE fp32 evaluation
order of the 54 layers is away from float64 (e_ref_all: the same over all 257 coefficients).  The GPU's order is another draw of the same
rounding noise and gets 4 x e_ref; a distance is a norm of the difference of two 64-vectors, each within 4 x e_ref per component, and gets
2 x sqrt(64) x 4 x e_ref = 64 x e_ref.  Every test prints its figure before it asserts (DESIGN.md section 8 keeps the record)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expr_inputs as I  # noqa: E402

from reface_amd import exprscore as ES  # noqa: E402
from reface_amd import ops  # noqa: E402
from reface_amd.align import resample_taps  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "expr.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


@pytest.fixture(scope="module")
def scorer():
    return ES.ExprScorer(ES.load_recon_state("none"), batch=3, device=DEV)          # 10 targets = 3 full batches + a tail of 1; 8 results: a tail of 2


def _edge_image(rng, H, W):
    """Noise whose first / last two rows and columns are a 0 / 255 checkerboard: the clipped edge windows and the bicubic overshoot."""
    c = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    edge = (yy < 2) | (yy >= H - 2) | (xx < 2) | (xx >= W - 2)
    c[edge] = board[edge]
    return c


@pytest.mark.parametrize("hw", [(512, 512), (1024, 1024), (300, 260), (57, 40), (1, 1)])
def test_expr_prep_is_pil_bit_for_bit(hw):
    """rf_expr_prep_u8 into a NaN-filled buffer against float32(PIL_resize_bytes / 255.): integer arithmetic and one correctly rounded
    division on both sides, so no tolerance."""
    from PIL import Image
    H, W = hw
    rng = np.random.default_rng(900 + H + W)
    imgs = np.stack([_edge_image(rng, H, W) for _ in range(2)])
    taps = [tuple(torch.from_numpy(t).to(DEV) for t in resample_taps(n, 512, "bicubic")) for n in (W, H)]
    out = torch.full((2, 512, 512, 8), float("nan"), dtype=torch.float32, device=DEV)
    ops.expr_prep_u8(torch.from_numpy(imgs).to(DEV), taps[0], taps[1], out)()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[..., 3:], np.zeros_like(got[..., 3:]))          # exactly 0 (the buffer was NaN)
    bad = 0
    for b in range(2):
        pil = np.array(Image.fromarray(imgs[b]).resize((512, 512), Image.BICUBIC))
        want = (pil / 255.).astype(np.float32)
        bad += int((got[b, :, :, :3].view(np.uint32) != want.view(np.uint32)).sum())
        if hw == (512, 512):
            assert np.array_equal(pil, imgs[b])          # PIL's resize of a 512 x 512 image is the identity
    print(f"expr prep {hw}: {bad} of {2 * 512 * 512 * 3} values differ from float32(PIL bytes / 255.) in any bit")
    assert bad == 0


def test_expr_prep_strided_batch_and_scorer_grouping(data):
    """A batch that is a strided view (every second image of a stack) and the scorer's grouping of mixed sizes equal prep_host."""
    rng = np.random.default_rng(77)
    stack = torch.from_numpy(np.stack([_edge_image(rng, 40, 24) for _ in range(4)])).to(DEV)
    view = stack[::2]
    taps = [tuple(torch.from_numpy(t).to(DEV) for t in resample_taps(n, 512, "bicubic")) for n in (24, 40)]
    out = torch.empty((2, 512, 512, 8), dtype=torch.float32, device=DEV)
    ops.expr_prep_u8(view, taps[0], taps[1], out)()
    for b in range(2):
        assert np.array_equal(out[b, :, :, :3].cpu().numpy().transpose(2, 0, 1), ES.prep_host(stack[2 * b].cpu().numpy()))
    sc = ES.ExprScorer.__new__(ES.ExprScorer)
    sc.dev, sc._taps = torch.device(DEV, torch.cuda.current_device()), {}
    imgs = [data["tgt_images"][k] for k in (3, 4, 5)]          # 512 x 512, 600 x 540, 57 x 40
    got = sc.prep_u8([torch.from_numpy(im) for im in imgs]).cpu().numpy()
    for b, im in enumerate(imgs):
        assert np.array_equal(got[b, :, :, :3].transpose(2, 0, 1), ES.prep_host(im)), im.shape


def _head(feat, w, bias):
    coef = torch.full((feat.shape[0], 257), float("nan"), dtype=torch.float32, device=DEV)
    ops.expr_head(feat.to(DEV), w.to(DEV), bias.to(DEV), coef)()
    torch.cuda.synchronize()
    return coef.cpu().numpy()


@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_expr_head_vs_float64(scale):
    """Mean over P pixels + 257 dot products against float64: 2048- and 256-term fp32 sums (the project's figure for rf_pose_head: 1e-4 of
    the largest coefficient).  Image 0 alone and image 0 of three are the same bits; P is an argument (P = 49)."""
    g = torch.Generator().manual_seed(int(scale) + 11)
    w = (torch.rand((257, 2048), generator=g) * 2 - 1) * (3.0 / 2048) ** 0.5 * scale
    bias = (torch.rand((257,), generator=g) * 2 - 1) * 0.1
    for P, B in ((256, 3), (49, 2)):
        feat = torch.relu(torch.randn((B, P, 2048), generator=g)) * scale
        got = _head(feat, w, bias)
        want = (feat.double().sum(1) / P) @ w.double().T + bias.double()
        err = float((torch.from_numpy(got).double() - want).abs().max() / want.abs().max())
        print(f"expr head scale {scale} P={P}: max|coef - fp64| / max|coef| = {err:.3e} (gate 1e-4)")
        assert np.isfinite(got).all() and err <= 1e-4
        if P == 256:
            alone = _head(feat[:1].contiguous(), w, bias)
            assert np.array_equal(alone[0].view(np.uint32), got[0].view(np.uint32))


@pytest.mark.parametrize("mn", [(1, 1), (257, 40)])
def test_expr_distance_vs_host(mn):
    """rf_expr_distance on columns 80..143 of 257-wide rows against score_host: 1e-12 relative, two runs bit-equal, NaN outside the column
    range ignored, labels N and -1 refused."""
    M, N = mn
    g = torch.Generator().manual_seed(M * 100 + N)
    tgt, res = torch.randn((N, 257), generator=g), torch.randn((M, 257), generator=g)
    labels = np.concatenate([[0, N - 1], torch.randint(0, N, (M,), generator=g).numpy()])[:M].astype(np.int64)          # both ends, repeats, permuted
    if M == 1:
        labels[:] = 0
    want = ES.score_host(tgt.numpy(), res.numpy(), labels)
    tgt[:, :80] = tgt[:, 144:] = res[:, :80] = res[:, 144:] = float("nan")
    sc = ES.ExprScorer.__new__(ES.ExprScorer)
    sc.dev = torch.device(DEV, torch.cuda.current_device())
    a = sc.score(tgt.to(DEV), res.to(DEV), labels)
    b = sc.score(tgt.to(DEV), res.to(DEV), labels)
    assert a["n"] == M and a["distances"].dtype == np.float64
    rel = float((np.abs(a["distances"] - want["distances"]) / want["distances"]).max())
    rel_v = abs(a["expression_value"] - want["expression_value"]) / want["expression_value"]
    print(f"expr distance M={M} N={N}: max rel |dist - host| = {rel:.3e}, Expression_value rel {rel_v:.3e}")
    assert rel <= 1e-12 and rel_v <= 1e-12
    assert np.array_equal(a["distances"].view(np.uint64), b["distances"].view(np.uint64)) and a["expression_value"] == b["expression_value"]
    for wrong in (N, -1):
        bad = labels.copy()
        bad[-1] = wrong
        with pytest.raises(IndexError):
            sc.score(tgt.to(DEV), res.to(DEV), bad)
        with pytest.raises(IndexError):          # the ops wrapper itself refuses them before the launch
            ops.expr_distance(res.to(DEV), tgt.to(DEV), torch.from_numpy(bad.astype(np.int32)).to(DEV), torch.empty(M, dtype=torch.float64, device=DEV),
                              torch.empty(2, dtype=torch.float64, device=DEV))


# (input shape, Cout, the epilogue rf_conv_gemm_plan2 reports for an fp32 launch without split-K scratch: 1 = direct register, 0 = staged)
EPILOGUE_CASES = [
    ((2, 9, 7, 64), 256, 0),          # aligned rows, 126 x 256: the 4-wave 64 x 64-per-wave tile, whose epilogue is the staged one
    ((2, 9, 7, 64), 160, 1),          # aligned rows on the 128 x 160 tile: the direct epilogue at the smallest size that reaches it
    ((2, 9, 7, 64), 40, 0),           # N % 16 != 0: staged, whole 4-column vectors
    ((2, 9, 7, 64), 42, 0),           # N % 4 != 0: staged, the per-element tail
    ((1, 16, 16, 512), 2048, 0),      # the bottleneck shape of layer4
    ((1, 224, 224, 64), 256, 1),      # 196 tiles of 256 x 256 on 8 waves: the direct epilogue of the engine's layer1 at batch >= 3
]


@pytest.mark.parametrize("shape,cout,direct", EPILOGUE_CASES)
def test_relu_after_residual_epilogue(shape, cout, direct):
    """A 1x1 convolution with bias and residual, fp32 operands, no split-K scratch: ACT_ADD_RELU is bit-equal to ACT_NONE followed by
    rf_add_relu with the residual (and to ACT_NONE + residual followed by rf_add_relu with zeros), on inputs where relu(conv) + residual,
    the order of every other activation code, differs from it in more than 10 % of the elements."""
    B, H, W, cin = shape
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(shape, generator=g).to(DEV)
    w = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).to(DEV)
    bias = (torch.randn((cout,), generator=g) * 0.1).to(DEV)
    res = torch.randn((B, H, W, cout), generator=g).to(DEV)
    wp = ops.pack_conv_weight(w, torch.float32)
    ws = ops.new_workspace(torch.device(DEV), nbytes=0)
    outs = {}
    with ops.workspace_scope(ws):
        for tag, act, r in (("fused", ops.ACT_ADD_RELU, res), ("plain", ops.ACT_NONE, None), ("plain_res", ops.ACT_NONE, res), ("relu_then_res", ops.ACT_RELU, res)):
            y = torch.full((B, H, W, cout), float("nan"), dtype=torch.float32, device=DEV)
            l = ops.conv2d(x, wp, y, bias, ksize=1, stride=1, pad=(0, 0), act=act, residual=r, name=tag)
            if tag == "fused":
                plan = ops.gemm_plan2(l)
            l()
            outs[tag] = y
    two = torch.empty_like(res)
    ops.add_relu(outs["plain"], res, two)()
    two0 = torch.empty_like(res)
    ops.add_relu(outs["plain_res"], torch.zeros_like(res), two0)()
    torch.cuda.synchronize()
    fused, two, two0, other = (t.cpu().numpy() for t in (outs["fused"], two, two0, outs["relu_then_res"]))
    frac = float((other != fused).mean())
    ref = torch.relu(torch.nn.functional.conv2d(x.cpu().permute(0, 3, 1, 2).double(), w.cpu().double(), bias.cpu().double()).permute(0, 2, 3, 1) + res.cpu().double())
    err = float((torch.from_numpy(fused).double() - ref).abs().max())
    print(f"relu-after-residual {shape} -> {cout}: plan {plan['bm']} x {plan['bn']} direct {plan['direct']} splitk {plan['splitk']}; "
          f"{int((fused.view(np.uint32) != two.view(np.uint32)).sum())} values differ from conv + rf_add_relu; relu(conv) + residual differs in {frac:.1%}; "
          f"max|fused - fp64| = {err:.2e}")
    assert plan["splitk"] == 1 and plan["direct"] == direct
    assert np.isfinite(fused).all() and err <= 1e-4
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    assert np.array_equal(fused.view(np.uint32), two0.view(np.uint32))
    assert frac > 0.10


def test_relu_after_residual_never_splits_k():
    """With split-K scratch available a long-K launch of few tiles splits K for ACT_NONE; the same launch with ACT_ADD_RELU does not (the
    reduce passes act before the residual) and stays bit-equal to the two-launch tail without scratch."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 8, 8, 2048), generator=g).to(DEV)
    w = (torch.randn((256, 2048, 1, 1), generator=g) / 2048 ** 0.5).to(DEV)
    res = torch.randn((1, 8, 8, 256), generator=g).to(DEV)
    wp = ops.pack_conv_weight(w, torch.float32)
    y, y0, two = (torch.empty_like(res) for _ in range(3))
    fused = ops.conv2d(x, wp, y, None, ksize=1, stride=1, pad=(0, 0), act=ops.ACT_ADD_RELU, residual=res)
    plain = ops.conv2d(x, wp, torch.empty_like(res), None, ksize=1, stride=1, pad=(0, 0), act=ops.ACT_NONE, residual=res)
    print(f"split-K with scratch: ACT_NONE {ops.gemm_plan2(plain)['splitk']}, ACT_ADD_RELU {ops.gemm_plan2(fused)['splitk']}")
    assert ops.gemm_plan2(plain)["splitk"] > 1 and ops.gemm_plan2(fused)["splitk"] == 1
    fused()
    with ops.workspace_scope(ops.new_workspace(torch.device(DEV), nbytes=0)):
        ops.conv2d(x, wp, y0, None, ksize=1, stride=1, pad=(0, 0), act=ops.ACT_NONE)()
    ops.add_relu(y0, res, two)()
    torch.cuda.synchronize()
    assert torch.equal(y, two)


def test_engine_coefficients_vs_reference(scorer, golden, data):
    """prep + ResNet-50 + head on the fixture's 18 images (mixed sizes; batch 3: full batches and tails of 1 and 2) against the reference
    module in float64.  Gates: 4 x e_ref on the 64 expression coefficients, 4 x e_ref_all on all 257, both read from the fixture."""
    e_ref, e_all = float(golden["e_ref"]), float(golden["e_ref_all"])
    worst = worst_all = 0.0
    for key, imgs in (("tgt", data["tgt_images"]), ("res", data["res_images"])):
        coef = scorer.coeffs_u8([torch.from_numpy(im) for im in imgs]).cpu().numpy()
        assert coef.shape == (len(imgs), 257) and np.isfinite(coef).all()
        d = np.abs(coef - golden[f"coef_f64_{key}"])
        worst, worst_all = max(worst, float(d[:, 80:144].max())), max(worst_all, float(d.max()))
        print(f"expr coefficients {key}: max|GPU - reference fp64| = {float(d.max()):.3e}, max|GPU - reference fp32| = "
              f"{float(np.abs(coef - golden[f'coef_f32_{key}']).max()):.3e}")
    print(f"expr coefficients: e_ref = {e_ref:.3e}, gate 4 x e_ref = {4 * e_ref:.3e}, GPU max over the 64 = {worst:.3e}; "
          f"e_ref_all = {e_all:.3e}, gate {4 * e_all:.3e}, GPU max over the 257 = {worst_all:.3e}")
    assert worst <= 4 * e_ref and worst_all <= 4 * e_all


def test_fused_tail_equals_unfused_tail(scorer, data):
    """The engine (conv3 with ACT_ADD_RELU) and the add_relu=True engine (conv3, then rf_add_relu) give the same bits on three images."""
    imgs = [torch.from_numpy(im) for im in data["tgt_images"][3:6]]          # 512 x 512, 600 x 540, 57 x 40
    fused = scorer.coeffs_u8(imgs).cpu().numpy()
    two = ES.ExprScorer(scorer.sd, batch=3, device=DEV, add_relu=True)
    n_fused, n_two = len(scorer.engine(3).launches), len(two.engine(3).launches)
    unfused = two.coeffs_u8(imgs).cpu().numpy()
    print(f"expr tail: {n_fused} launches fused, {n_two} unfused; {int((fused.view(np.uint32) != unfused.view(np.uint32)).sum())} of {fused.size} coefficients differ")
    assert n_two == n_fused + 16
    assert np.array_equal(fused.view(np.uint32), unfused.view(np.uint32))


def test_engine_is_batch_invariant(scorer, data):
    """No GEMM of the engine splits K, and the head is one workgroup per image: an image's coefficients are the same bits alone and among five."""
    imgs = [torch.from_numpy(im) for im in data["tgt_images"][:5]]
    e5 = scorer.engine(5)
    scorer.prep_u8(imgs, out=e5.x)
    c5 = e5.run().cpu().numpy()
    e1 = scorer.engine(1)
    for k in (0, 2, 4):
        scorer.prep_u8(imgs[k:k + 1], out=e1.x)
        c1 = e1.run().cpu().numpy()
        assert np.array_equal(c1[0].view(np.uint32), c5[k].view(np.uint32)), (k, np.abs(c1[0] - c5[k]).max())


def test_engine_batches_are_capped():
    sc = ES.ExprScorer.__new__(ES.ExprScorer)
    sc.batch = 50
    assert ES.ENGINE_B * 256 * 256 * 64 * 4 < 2 ** 31
    assert sc._engine_sizes(120) == {25, 20}          # 50 + 50 + 20: engine batches of 25 and 20
    assert sc._engine_sizes(18) == {18}
    sc.batch = 4
    assert sc._engine_sizes(10) == {4, 2}


def test_cli_end_to_end(tmp_path, golden, data):
    """PNG folders -> the reference's printed lines, in a fresh process.  Labels equal the reference's; every distance and Expression_value
    within 64 x e_ref of the reference's float64 ones (a wrong labelling or pairing would move Expression_value by more than 10 gates)."""
    paths = I.write_folders(str(tmp_path / "folders"), data)
    out_json = str(tmp_path / "expr.json")
    cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "Expression", "expression_compare_face_recon.py"), "--device", "cuda"] + paths + [
        "--recon_ckpt", "none", "--batch-size", "4", "--num-workers", "2", "--json", out_json, "--print_sim", "True"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert "loading the model from none" in lines
    r = json.load(open(out_json))
    assert "Expression_value:  {}".format(r["expression_value"]) in lines          # print('Expression_value: ', v): two spaces
    assert r["labels"] == golden["labels"].tolist() and r["images"] == 18 and r["images_per_s"] > 0
    at = lines.index("Similarities: ")
    sims = lines[at + 2:at + 10]
    assert lines[at + 1] == " " and len(lines) == at + 10 and [s.split(" : ")[0] for s in sims] == [str(i) for i in range(8)]
    assert [float(s.split(" : ")[1]) for s in sims] == r["distances"]
    gate = 64 * float(golden["e_ref"])
    d = float(np.abs(np.array(r["distances"]) - golden["dist_f64"]).max())
    dv = abs(r["expression_value"] - float(golden["expression_value_f64"]))
    print(f"expr CLI: max|distance - reference| = {d:.3e}, |Expression_value - reference| = {dv:.3e} (gate 64 x e_ref = {gate:.3e}); {r['images_per_s']:.1f} images/s")
    assert d <= gate and dv <= gate
