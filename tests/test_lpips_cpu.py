"""The perceptual distance, host side (reface_amd/lpips.py, eval_tool/lpips/): the host restatements against the reference's own outputs
(tests/golden/lpips.npz, tools/gen_golden.py:gen_lpips), the key layout and the loaders, the layer arithmetic (batch cap, minimum size),
nine wrong readings of the reference that the fixture must tell from the right one, and the numerics of the direct form that rf_lpips_layer
uses against the expanded one it avoids."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_inputs as I  # noqa: E402

from reface_amd import idscore as S  # noqa: E402
from reface_amd import lpips as LP  # noqa: E402
from reface_amd import params as P  # noqa: E402
from reface_amd import posescore as PS  # noqa: E402

F64 = torch.float64
GPU_GATE = 2e-5          # the relative gate of tests/test_lpips_gpu.py: a wrong reading must move a stored value by more than this


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lpips.npz"))


@pytest.fixture(scope="module")
def keys(golden_dir):
    return json.load(open(os.path.join(golden_dir, "lpips_keys.json")))


@pytest.fixture(scope="module")
def states():
    return {net: LP.load_lpips_state("none", net) for net in ("alex", "vgg")}


def _tensors(images):
    return torch.from_numpy(np.stack([LP.prep_host(im) for im in images]))


@pytest.fixture(scope="module")
def cases():
    """(net, x, y) per case: fp32 [4, 3, H, W] in [-1, 1]."""
    out = []
    for c, (net, _, _) in enumerate(I.CASES):
        xs, ys = I.build_case(c)
        out.append((net, _tensors(xs), _tensors(ys)))
    return out


def _rel(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))).max())


def test_fixture_is_not_degenerate(golden):
    e_ref, e_near = float(golden["e_ref"]), float(golden["e_ref_near"])
    assert 0.0 < e_ref < e_near < 1e-2
    assert 4 * e_ref <= GPU_GATE          # the GPU gate is never tighter than the reference's own fp32 noise
    worst, worst_near = 0.0, 0.0
    for c in range(len(I.CASES)):
        n = I.case_name(c)
        v32, v64 = golden[f"v_f32_{n}"], golden[f"v_f64_{n}"]
        assert v64.shape == (I.PAIRS, 5) and (v64 > 0).all()
        rel = np.abs(v32 - v64) / v64
        ordinary = [k for k in range(I.PAIRS) if k != I.NEAR]
        worst, worst_near = max(worst, float(rel[ordinary].max())), max(worst_near, float(rel[I.NEAR].max()))
        assert golden[f"d_f64_{n}"][I.NEAR] < 0.1 * golden[f"d_f64_{n}"][ordinary].min()
    worst = max(worst, _rel(golden["folder_v_f32"], golden["folder_v_f64"]))
    assert worst == e_ref and worst_near == e_near
    assert int(golden["seed"]) == LP.SEED


def test_host_matches_reference(golden, states, cases):
    """lpips_host / prep_host / score_host on the fixture's inputs against the reference module in float64: every v[b, l], d[b] and the
    scalar within 1e-12 relative."""
    for c, (net, x, y) in enumerate(cases):
        n = I.case_name(c)
        v = LP.distances_host(states[net], x, y, net)
        r = LP.score_host(v)
        e = (_rel(v, golden[f"v_f64_{n}"]), _rel(r["distances"], golden[f"d_f64_{n}"]), abs(r["lpips_value"] / float(golden[f"scalar_f64_{n}"]) - 1.0))
        print(f"lpips host {n}: rel |host - reference fp64|: v {e[0]:.2e}, d {e[1]:.2e}, scalar {e[2]:.2e}")
        assert v.shape == (I.PAIRS, 5) and v.dtype == np.float64 and r["n"] == I.PAIRS
        assert max(e) <= 1e-12
        s32 = LP.score_host(golden[f"v_f32_{n}"])
        assert _rel(s32["distances"], golden[f"d_f32_{n}"]) <= 1e-12
        assert abs(s32["lpips_value"] / float(golden[f"scalar_f32_{n}"]) - 1.0) <= 1e-6          # the module sums its fp32 rows in fp32


def test_normalised_features_match_reference(golden, states, cases):
    """normalize_activation of the five taps of one 'alex' pair: the stored tensors of BaseNet.forward in float64."""
    net, x, y = cases[I.FEATURE_CASE]
    k = I.FEATURE_PAIR
    for name, t in (("x", x), ("y", y)):
        feats = LP.features_host(states[net], t[k:k + 1], net)
        assert [f.shape[1] for f in feats] == list(P.LPIPS_CHANNELS[net])
        for l, f in enumerate(feats):
            want = golden[f"nfeat_{name}_{l}"]
            got = LP.normalize_host(f)[0].numpy()
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
            assert (f >= 0).all()          # taps are taken after the ReLU
    assert golden["nfeat_x_4"].shape == (256, 1, 1) and golden["nfeat_x_0"].shape == (64, 8, 7)


def test_folder_pairing_matches_reference(golden, states, tmp_path):
    """The folder layout: natural order, last-number labels, a result against the target at the position its label names."""
    data = I.build_folders()
    paths = I.write_folders(str(tmp_path), data)
    tgt, res = S.list_images(paths[0]), S.list_images(paths[1])
    assert [os.path.basename(f) for f in tgt] == data["tgt_names"] and [os.path.basename(f) for f in res] == data["res_names"]
    assert sorted(data["res_names"]) != data["res_names"]                    # lexicographic order would start with "10_"
    labels = PS.parse_labels_last(res)
    assert labels == golden["labels"].tolist() == I.RES_LABELS and len(set(labels)) < len(labels) and labels != sorted(labels)
    sd = states[I.FOLDER_NET]
    v = np.concatenate([LP.distances_host(sd, _tensors([data["tgt_images"][l]]), _tensors([data["res_images"][i]]), I.FOLDER_NET)
                        for i, l in enumerate(labels)])
    r = LP.score_host(v)
    assert _rel(v, golden["folder_v_f64"]) <= 1e-12 and _rel(r["distances"], golden["folder_d_f64"]) <= 1e-12
    assert abs(r["lpips_value"] / float(golden["folder_value_f64"]) - 1.0) <= 1e-12
    # WRONG: results paired with targets by position
    w = np.concatenate([LP.distances_host(sd, _tensors([data["tgt_images"][i]]), _tensors([data["res_images"][i]]), I.FOLDER_NET)
                        for i in range(len(labels))])
    assert abs(LP.score_host(w)["lpips_value"] / float(golden["folder_value_f64"]) - 1.0) > GPU_GATE


def test_keys_and_shapes(keys):
    """The module's and lpips_param_specs' keys, order and shapes equal the reference module's state_dict() for both nets."""
    from eval_tool.lpips.lpips import LPIPS
    assert len(keys["alex"]) == 17 and len(keys["vgg"]) == 33
    for net in ("alex", "vgg"):
        ref = [(k, tuple(s)) for k, s in keys[net]]
        assert [(k, tuple(s)) for k, s in P.lpips_param_specs(net).items()] == ref
        m = LPIPS(net_type=net)
        sd = m.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == ref
        assert all(float(v.abs().max()) == 0.0 for v in sd.values())          # zero until load_state_dict: nothing is downloaded
        assert not any(p.requires_grad for p in m.parameters())
        m.load_state_dict(LP.load_lpips_state("none", net), strict=True)
        assert float(m.state_dict()["lin.0.1.weight"].min()) >= 0.0 and m.net.n_channels_list == list(P.LPIPS_CHANNELS[net])
        assert torch.equal(m.state_dict()["net.mean"].reshape(-1), torch.tensor(LP.MEAN)) and torch.equal(m.net.std.reshape(-1), torch.tensor(LP.STD))
    assert LPIPS(net_type="alex", ckpt="none").state_dict()["net.layers.0.weight"].abs().max() > 0


def test_reference_surface():
    from eval_tool.lpips import networks, utils
    from eval_tool.lpips.lpips import LPIPS
    with pytest.raises(NotImplementedError, match="squeeze"):
        LPIPS(net_type="squeeze")
    with pytest.raises(NotImplementedError, match="is unknown"):
        LPIPS(net_type="resnet")
    with pytest.raises(AssertionError, match="v0.1"):
        LPIPS(version="0.0")
    with pytest.raises(RuntimeError, match="lpips_ckpt"):
        utils.get_state_dict("alex")
    g = torch.Generator().manual_seed(3)
    f = torch.rand((2, 5, 3, 3), generator=g, dtype=F64)
    f[0, :, 1, 1] = 0
    n = utils.normalize_activation(f)
    assert torch.isfinite(n).all() and float(n[0, :, 1, 1].abs().max()) == 0.0          # an all-zero pixel normalises to zeros
    assert torch.allclose((n ** 2).sum(1)[1], torch.ones(3, 3, dtype=F64), atol=1e-8)
    assert torch.equal(n, LP.normalize_host(f))
    assert len(networks.LinLayers([4, 8])) == 2 and networks.get_network("vgg").target_layers == [4, 9, 16, 23, 30]
    with pytest.raises(Exception, match="no CPU fallback"):          # host tensors raise, as every op here rejects them
        LPIPS(ckpt="none")(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


def test_loaders(tmp_path):
    sd = LP.load_lpips_state("none", "alex")
    assert list(sd) == list(P.lpips_param_specs("alex")) and LP.check_lpips_state(sd, "alex") is sd
    plain = str(tmp_path / "lpips.pth")
    torch.save(dict(sd), plain)
    assert set(LP.load_lpips_state(plain, "alex")) == set(sd)
    assert set(LP.load_lpips_state(dict(sd), "alex")) == set(sd)
    # a REFace Lightning checkpoint: the module sits at LatentDiffusion.lpips_loss
    full = {"model.diffusion_model.out.2.bias": torch.zeros(4), "learnable_vector": torch.zeros(1, 1, 768)}
    full.update({LP.PREFIX + k: v for k, v in sd.items()})
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"state_dict": full, "global_step": 7}, ckpt)
    got = LP.load_lpips_state(ckpt, "alex")
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="vgg"):          # the same checkpoint does not fit the other net
        LP.load_lpips_state(ckpt, "vgg")
    del full[LP.PREFIX + "lin.3.1.weight"]
    torch.save({"state_dict": full}, ckpt)
    with pytest.raises(RuntimeError, match=r"missing \['lin.3.1.weight'\]"):
        LP.load_lpips_state(ckpt, "alex")
    torch.save({"state_dict": {k: v for k, v in full.items() if not k.startswith(LP.PREFIX)}}, ckpt)
    with pytest.raises(RuntimeError, match="no 'lpips_loss"):
        LP.load_lpips_state(ckpt, "alex")
    extra = dict(sd)
    extra["lin.5.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(RuntimeError, match="unexpected .'lin.5.1.weight'"):
        LP.load_lpips_state(extra, "alex")
    bad = dict(sd)
    bad["lin.0.1.weight"] = torch.zeros(1, 64)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        LP.load_lpips_state(bad, "alex")


def test_layer_arithmetic_cap_and_minimum(states):
    """The plans against the reference's target layers; no tensor of an engine reaches 2^31 bytes; sizes below the minimum are refused."""
    assert [p[1] for p in P.lpips_plan("alex") if p[0] == "conv"] == [0, 3, 6, 8, 10]
    assert [p[1] for p in P.lpips_plan("vgg") if p[0] == "conv"] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [p[0] for p in P.lpips_plan("alex")].count("pool") == 2 and [p[0] for p in P.lpips_plan("vgg")].count("pool") == 4          # the last pool never runs
    assert P.lpips_plan("alex")[-1] == ("tap", 4) and P.lpips_plan("vgg")[-1] == ("tap", 4)
    assert [(h, w, c) for k, h, w, c in LP.layer_shapes("alex", 64, 64) if k == "tap"] == [(15, 15, 64), (7, 7, 192), (3, 3, 384), (3, 3, 256), (3, 3, 256)]
    assert [(h, w, c) for k, h, w, c in LP.layer_shapes("vgg", 70, 61) if k == "tap"] == [(70, 61, 64), (35, 30, 128), (17, 15, 256), (8, 7, 512), (4, 3, 512)]
    assert LP.min_size("alex") == 31 and LP.min_size("vgg") == 16
    assert LP.bytes_per_image("vgg", 512, 512) == 512 * 512 * 64 * 4 == 67108864
    assert LP.bytes_per_image("alex", 512, 512) == 512 * 512 * 8 * 4          # the padded input is AlexNet's largest tensor
    for net, h, w in (("vgg", 512, 512), ("alex", 512, 512), ("vgg", 1024, 1024), ("alex", 64, 64), ("vgg", 70, 61)):
        cap = LP.engine_batch_cap(net, h, w)
        assert cap >= 1 and 2 * cap * LP.bytes_per_image(net, h, w) < 2 ** 31 <= 2 * (cap + 1) * LP.bytes_per_image(net, h, w), (net, h, w, cap)
    assert LP.engine_batch_cap("vgg", 512, 512) == 15 and LP.engine_batch_cap("alex", 512, 512) == 127
    assert LP._runs([(1, 1)] * 5 + [(2, 2)] + [(1, 1)] * 2, lambda s: 2) == [(0, 2), (2, 4), (4, 5), (5, 6), (6, 8)]
    # refused before any launch (no device is touched: this runs without a GPU)
    for net, h, w in (("alex", 30, 64), ("alex", 64, 30), ("vgg", 15, 15)):
        with pytest.raises(ValueError, match=f"at least {LP.min_size(net)} x {LP.min_size(net)}"):
            LP._LPIPSEngine(states[net], net, 1, h, w, "cpu")
    LP.check_size("alex", 31, 31)
    LP.check_size("vgg", 16, 16)
    with pytest.raises(ValueError, match="at most 15"):
        LP._LPIPSEngine(states["vgg"], "vgg", 16, 512, 512, "cpu")


# ---- wrong readings of the reference -------------------------------------------------------------------------------------------------
def _variant(sd, x, y, net, pre_relu=False, zero_based=False, norm_pixels=False, w_first=False, mean_hwc=False, last_pool=False, ceil=False,
             div_then_sub=False):
    """v float64 [B, L] of the reference with one line read wrongly (all flags off: the reference)."""
    Fn = torch.nn.functional
    n_mod = {"alex": 13, "vgg": 31}[net]
    convs = {p[1]: p for p in P.lpips_plan(net) if p[0] == "conv"}
    pools = {"alex": {2: 3, 5: 3, 12: 3}, "vgg": {4: 2, 9: 2, 16: 2, 23: 2, 30: 2}}[net]
    targets = {"alex": [2, 5, 8, 10, 12], "vgg": [4, 9, 16, 23, 30]}[net]

    def feats(t):
        mean, std = sd["net.mean"].to(F64), sd["net.std"].to(F64)
        h = (t.to(F64) / std - mean) if div_then_sub else (t.to(F64) - mean) / std
        out = []
        for i in range(n_mod):
            pos = i if zero_based else i + 1
            if i in convs:
                _, _, _, _, _, s, pad = convs[i]
                h = Fn.conv2d(h, sd[f"net.layers.{i}.weight"].to(F64), sd[f"net.layers.{i}.bias"].to(F64), stride=s, padding=pad)
                if pre_relu and (pos + 1) in targets:
                    out.append(h)
            elif i in pools:
                h = Fn.max_pool2d(h, pools[i], 2, ceil_mode=ceil)
            else:
                h = Fn.relu(h)
            if pos in targets and not pre_relu:
                out.append(h)
            if len(out) == 5 and not (last_pool and i < n_mod - 1):
                break
        if last_pool:
            out[4] = h
        return out

    def norm(f):
        dims = (2, 3) if norm_pixels else (1,)
        return f / (torch.sqrt(torch.sum(f ** 2, dim=dims, keepdim=True) + 1e-16) + 1e-10)

    cols = []
    for l, (fx, fy) in enumerate(zip(feats(x), feats(y))):
        w = sd[f"lin.{l}.1.weight"].to(F64).reshape(1, -1, 1, 1)
        d = (w * (norm(fx) - norm(fy))) ** 2 if w_first else w * (norm(fx) - norm(fy)) ** 2
        cols.append(d.mean(dim=(1, 2, 3)) if mean_hwc else d.sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(cols, dim=1).numpy()


WRONG = [("pre_relu", 0), ("zero_based", 3), ("norm_pixels", 0), ("w_first", 0), ("mean_hwc", 0), ("last_pool", 0), ("ceil", 1), ("div_then_sub", 0)]


def test_variant_harness_reproduces_the_reference(golden, states, cases):
    for c in (0, 1, 3):
        net, x, y = cases[c]
        assert _rel(_variant(states[net], x, y, net), golden[f"v_f64_{I.case_name(c)}"]) <= 1e-12


@pytest.mark.parametrize("flag,case", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_readings_are_told_apart(flag, case, golden, states, cases):
    """Taps before the ReLU, tap indices read 0-based (VGG16: the taps land behind the pools), normalisation over pixels, the weight inside
    the square, a mean over HW * C, the last MaxPool run, ceil-mode pools (70 x 61), z-score divided before it is shifted: each moves an
    ordinary stored value by more than the GPU gate.  (Pairing by position: test_folder_pairing_matches_reference.)"""
    net, x, y = cases[case]
    want = golden[f"v_f64_{I.case_name(case)}"]
    v = _variant(states[net], x, y, net, **{flag: True})
    ordinary = [k for k in range(I.PAIRS) if k != I.NEAR]
    moved = float((np.abs(v - want) / want)[ordinary].max())
    print(f"wrong reading {flag} on {I.case_name(case)}: largest relative change of an ordinary v[b, l] = {moved:.3e}")
    assert moved > GPU_GATE


# ---- the direct form against the expanded one -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 192, 512])
def test_direct_form_holds_where_the_expanded_form_cancels(C):
    """y = x + 1e-3 noise on post-ReLU-like features (about half zeros), fixed seed.  In fp32 the direct form -- normalise, subtract, square,
    weight, what rf_lpips_layer does -- stays within the 2e-5 gate of float64; the expanded five-sum form
    sum w a^2 / na^2 - 2 sum w a b / (na nb) + sum w b^2 / nb^2 (one pass too) does not."""
    g = torch.Generator().manual_seed(900 + C)
    a = torch.relu(torch.randn((1, C, 12, 12), generator=g, dtype=torch.float32))
    b = torch.relu(a + 1e-3 * torch.randn((1, C, 12, 12), generator=g, dtype=torch.float32))
    w = torch.rand((C,), generator=g, dtype=torch.float32)
    want = float(LP.lpips_host([a], [b], [w])[0, 0])

    def direct(a, b, w):
        na = a / (torch.sqrt((a * a).sum(1, keepdim=True) + 1e-16) + 1e-10)
        nb = b / (torch.sqrt((b * b).sum(1, keepdim=True) + 1e-16) + 1e-10)
        return (w.view(1, -1, 1, 1) * (na - nb) ** 2).sum(1)

    def expanded(a, b, w):
        wv = w.view(1, -1, 1, 1)
        na = torch.sqrt((a * a).sum(1) + 1e-16) + 1e-10
        nb = torch.sqrt((b * b).sum(1) + 1e-16) + 1e-10
        return (wv * a * a).sum(1) / (na * na) - 2 * (wv * a * b).sum(1) / (na * nb) + (wv * b * b).sum(1) / (nb * nb)

    e_direct = abs(float(direct(a, b, w).double().mean()) / want - 1.0)
    e_expanded = abs(float(expanded(a, b, w).double().mean()) / want - 1.0)
    assert abs(float(expanded(a.double(), b.double(), w.double()).mean()) / want - 1.0) <= 1e-6          # the same quantity, in float64
    print(f"C = {C}: v = {want:.3e}; fp32 direct form {e_direct:.2e} from float64, fp32 expanded form {e_expanded:.2e} (gate {GPU_GATE:.0e})")
    assert e_direct <= GPU_GATE < e_expanded


# ---- the C-ABI entries and the CLI's argument surface ---------------------------------------------------------------------------------
def test_ops_are_exported_and_refuse_host_tensors():
    from reface_amd import _lib, ops
    assert {"rf_lpips_prep_u8", "rf_lpips_prep_f32", "rf_maxpool2d", "rf_lpips_layer", "rf_lpips_total"} <= set(_lib.EXPORTS)
    assert _lib.load().rf_version() >= 103
    f64 = torch.float64
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.lpips_prep_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 8))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.lpips_prep_f32(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, 8))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.maxpool2d(torch.zeros(1, 8, 8, 4), torch.zeros(1, 3, 3, 4), k=3)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.lpips_layer(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(4), torch.zeros(4, dtype=f64), torch.zeros(1, 5, dtype=f64), 0)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.lpips_total(torch.zeros(1, 5, dtype=f64), torch.zeros(1, dtype=f64), torch.zeros(2, dtype=f64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LP.LPIPSScorer(LP.load_lpips_state("none"), device="cpu")
    header = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert f"#define RF_LPIPS_MAX_BLOCKS {ops.LPIPS_MAX_BLOCKS}\n" in header


def test_cli_argument_surface(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "eval_tool", "lpips"))
    import lpips_compare as cli
    p = cli.build_parser()
    a = p.parse_args(["--device", "cuda", "targets", "results"])
    assert a.path == ["targets", "results"] and a.device == "cuda" and a.net == "alex" and a.batch_size == 16 and a.num_workers is None
    assert a.json is None and a.print_sim is False
    b = p.parse_args(["t", "r", "--batch-size", "4", "--num-workers", "2", "--net", "vgg", "--lpips_ckpt", "none", "--print_sim", "True", "--json", "o.json"])
    assert b.batch_size == 4 and b.num_workers == 2 and b.net == "vgg" and b.lpips_ckpt == "none" and b.print_sim is True and b.json == "o.json"
    with pytest.raises(SystemExit):
        p.parse_args(["only_one_path"])
    with pytest.raises(SystemExit):
        p.parse_args(["t", "r", "--net", "squeeze"])
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["t", "r", "--device", "cpu"])
    stats = tmp_path / "stats.npz"
    np.savez(str(stats), mu=np.zeros(3))
    (tmp_path / "results").mkdir()
    with pytest.raises(SystemExit, match="npz"):
        cli.main([str(stats), str(tmp_path / "results"), "--lpips_ckpt", "none"])
