"""The identity score on the GPU (reface_amd/csrc/idscore.hip, reface_amd/idscore.py, eval_tool/ID_retrieval/ID_retrieval.py) against the
reference's own outputs (tests/golden/idscore.npz) and the host restatements that tests/test_idscore_cpu.py pins to them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import idscore_inputs as I  # noqa: E402

from reface_amd import idscore as S  # noqa: E402
from reface_amd import params as P  # noqa: E402
from reface_amd.data import resize_u8_linear  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP1 = 2.0 ** -23          # one fp32 ulp of 1.0


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "idscore.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


@pytest.fixture(scope="module")
def scorer():
    return S.IDScorer(S.load_arcface_state("none"), precision="full", batch=5, device=DEV)          # 16 images = 3 full batches + a tail of 1


def _lut(keep):
    t = torch.zeros(256, dtype=torch.uint8)
    t[torch.tensor(list(keep), dtype=torch.long)] = 1
    return t.to(DEV)


def _prep(img, lab, lut):
    from reface_amd import ops
    img, lab = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (img, lab))
    if img.dim() == 3:
        img, lab = img[None], lab[None]
    out = torch.full((img.shape[0], 3, 112, 112), float("nan"), dtype=torch.float32, device=DEV)
    ops.id_prep_u8(img, lab, lut, out)()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("hw", [(160, 144), (128, 128), (224, 224), (112, 112), (1024, 1024), (301, 517), (57, 40)])
def test_id_prep_image_resize_is_cv2_exact(hw):
    """With every label preserved the mask is 1 and the output is the normalised cv2 INTER_LINEAR resize: integer arithmetic, so the bytes
    recovered from it must EQUAL resize_u8_linear's (224 -> 112 is OpenCV's 2:1 area case, 112 -> 112 the identity, 57 x 40 an upscale)."""
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    img = torch.randint(0, 256, (2,) + hw + (3,), dtype=torch.uint8, generator=g).numpy()
    lab = torch.randint(0, 256, (2, hw[0] // 2 + 1, hw[1] // 3 + 1), dtype=torch.uint8, generator=g).numpy()
    got = _prep(img, lab, _lut(range(256)))
    for b in range(2):
        want_u8 = resize_u8_linear(img[b], 112, 112).transpose(2, 0, 1)
        want = (torch.from_numpy(want_u8.copy()).float() / 255.0 - 0.5) / 0.5
        assert np.array_equal(got[b], want.numpy())
        assert np.array_equal(np.rint((got[b] * 0.5 + 0.5) * 255.0).astype(np.uint8), want_u8)


def test_id_prep_unmasked_equals_reference(golden, data):
    got = _prep(np.stack([data["src_images"][i] for i in I.PREP_SAMPLES["src"]]), np.stack([data["src_labels"][i] for i in I.PREP_SAMPLES["src"]]),
                _lut(S.preserve_labels("other")))
    assert np.array_equal(got, golden["prep_src_nomask"])


def test_id_prep_masked_vs_reference(golden, data, scorer):
    """The masked, normalised tensor against the reference's.  Legitimate differences: FMA contraction and the order of the two bilinear
    lerps of the mask.  Gate = (reference vs prep_host, measured here) + 4 fp32 ulp of 1.0 (values are in [-1, 1]).  Measured on an
    MI355X: reference vs prep_host 0, kernel vs reference 1.3e-7."""
    keep = S.preserve_labels(I.DATASET)
    worst_host = worst_dev = 0.0
    for key, imgs, labs, idx in (("prep_src", data["src_images"], data["src_labels"], I.PREP_SAMPLES["src"]),
                                 ("prep_res", data["res_images"], data["res_labels"], I.PREP_SAMPLES["res"])):
        got = _prep(np.stack([imgs[i] for i in idx]), np.stack([labs[i] for i in idx]), _lut(keep))          # one stacked launch
        for k, i in enumerate(idx):
            d_host = float(np.abs(S.prep_host(imgs[i], labs[i], keep) - golden[key][k]).max())
            d_dev = float(np.abs(got[k] - golden[key][k]).max())
            print(f"{key}[{i}]: reference vs prep_host {d_host:.3e}, kernel vs reference {d_dev:.3e}")
            worst_host, worst_dev = max(worst_host, d_host), max(worst_dev, d_dev)
            assert d_dev <= d_host + 4 * ULP1, (key, i, d_dev, d_host)
    print(f"id_prep worst: reference vs prep_host {worst_host:.3e}, kernel vs reference {worst_dev:.3e}, gate + {4 * ULP1:.3e}")
    # images of different sizes as lists: the same numbers as the stacked launches
    # (runs of equal sizes are stacked into one launch: here [source 0, source 7 | result 0])
    imgs = [torch.from_numpy(data["src_images"][0]), torch.from_numpy(data["src_images"][7]), torch.from_numpy(data["res_images"][0])]
    labs = [torch.from_numpy(data["src_labels"][0]), torch.from_numpy(data["src_labels"][7]), torch.from_numpy(data["res_labels"][0])]
    x = scorer.prep_u8(imgs, labs, keep).cpu().numpy()
    for got, want in zip(x, (golden["prep_src"][0], golden["prep_src"][1], golden["prep_res"][0])):
        assert np.abs(got - want).max() <= 4 * ULP1


def test_features_vs_reference(golden, data, scorer):
    """All 32 fixture images from bytes to features: the project's ArcFace gate (1e-5 max abs, tests/test_e2e_gpu.py)."""
    keep = S.preserve_labels(I.DATASET)
    f_src = scorer.embed_u8(torch.from_numpy(np.stack(data["src_images"])), torch.from_numpy(np.stack(data["src_labels"])), keep).cpu().numpy()
    f_res = scorer.embed_u8(torch.from_numpy(np.stack(data["res_images"])), torch.from_numpy(np.stack(data["res_labels"])), keep).cpu().numpy()
    e_src, e_res = float(np.abs(f_src - golden["f_src"]).max()), float(np.abs(f_res - golden["f_res"]).max())
    print(f"features max|d| vs reference: sources {e_src:.3e}, results {e_res:.3e}")
    assert e_src < 1e-5 and e_res < 1e-5, (e_src, e_res)
    assert np.allclose(np.linalg.norm(f_src, axis=1), 1.0, atol=1e-6)


def test_forward_id112_matches_extract_feats_chain(golden, scorer):
    """The engine entry alone, from the reference's prepared tensors (a copy-in call, not the in-place buffer)."""
    x = torch.from_numpy(golden["prep_res"]).to(DEV)
    f = scorer.net.forward_id112(x)[0].cpu().numpy()
    e = float(np.abs(f - golden["f_res"][I.PREP_SAMPLES["res"]]).max())
    assert e < 1e-5, e


def _check_retrieve(scorer, f_src, f_res, labels):
    h = S.score_host(f_src, f_res, labels)
    r = scorer.score(torch.from_numpy(f_src).to(DEV), torch.from_numpy(f_res).to(DEV), labels)
    k = min(5, f_src.shape[0])
    assert np.array_equal(r["pred"], h["pred"])                                      # every row
    assert np.array_equal(r["rank"], h["rank"])
    assert np.array_equal(r["top5_idx"][:, :k], h["top5_idx"][:, :k]) and (r["top5_idx"][:, k:] == -1).all()
    assert np.array_equal(r["rank"] == 0, h["rank"] == 0) and np.array_equal(r["rank"] < 5, h["rank"] < 5)
    assert r["top1"] == h["top1"] and r["top5"] == h["top5"] and r["n"] == h["n"]
    assert np.abs(r["similarities"] - h["similarities"]).max() <= 1e-12
    assert abs(r["mean"] - h["mean"]) <= 1e-12
    return h, r


def test_retrieve_golden_features(golden, scorer):
    h, r = _check_retrieve(scorer, golden["f_src"], golden["f_res"], golden["labels"])
    assert np.array_equal(r["rank"], golden["rank"]) and np.array_equal(r["pred"], golden["pred"])
    assert r["top1"] == float(golden["top1"]) and r["top5"] == float(golden["top5"])
    assert np.abs(r["similarities"] - golden["similarities"]).max() <= 1e-12


@pytest.mark.parametrize("N,M", [(1000, 1000), (997, 1003), (65, 6), (3, 7), (1, 5)])
def test_retrieve_synthetic(scorer, N, M):
    """Unit-norm features, labels planted at known ranks: row i's label is the source at position PLANT[i % len] of the host's order.  The
    preconditions (no score within 1e-9 of the label's, none among the first six within 1e-9 of each other) are checked here on the CPU;
    fp64 summation-order noise is ~1e-15."""
    f_src = torch.nn.functional.normalize(P.seeded_randn((N, 512), 900 + N), dim=1)
    mix = f_src[torch.arange(M) % N] * 0.5 + torch.nn.functional.normalize(P.seeded_randn((M, 512), 901 + M), dim=1)
    f_res = torch.nn.functional.normalize(mix, dim=1)
    f_src, f_res = f_src.numpy(), f_res.numpy()
    dot = f_res.astype(np.float64) @ f_src.astype(np.float64).T
    order = np.argsort(-dot, axis=1, kind="stable")
    plant = np.array([0, 1, 2, 4, 5, 9, N - 1])[np.arange(M) % 7] % N
    labels = order[np.arange(M), plant]
    srt = np.take_along_axis(dot, order, axis=1)
    lab_gap = np.abs(srt - dot[np.arange(M), labels][:, None])
    lab_gap[np.arange(M), plant] = np.inf
    assert lab_gap.min() > 1e-9 and (N < 2 or np.abs(np.diff(srt[:, :7], axis=1)).min() > 1e-9), "tied scores: choose another seed"
    h, r = _check_retrieve(scorer, f_src, f_res, labels)
    assert np.array_equal(r["rank"], plant)


def test_retrieve_ties_go_to_the_lower_index(scorer):
    f_src = np.zeros((70, 512), dtype=np.float32)
    f_src[:, 0] = 1.0                                   # 70 identical sources (more than one tile of 64): every score ties
    f_res = np.zeros((3, 512), dtype=np.float32)
    f_res[:, 0] = 1.0
    r = scorer.score(torch.from_numpy(f_src).to(DEV), torch.from_numpy(f_res).to(DEV), [0, 3, 69])
    assert r["top5_idx"].tolist() == [[0, 1, 2, 3, 4]] * 3 and r["rank"].tolist() == [0, 3, 69]
    with pytest.raises(IndexError):
        scorer.score(torch.from_numpy(f_src).to(DEV), torch.from_numpy(f_res).to(DEV), [0, 3, 70])


def test_cli_end_to_end(tmp_path, golden, data):
    """PNG folders -> the reference's three printed lines.  Top-1 / top-5 equal the reference's exactly; every similarity and the mean
    within 5e-4: two unit vectors each within 1e-5 per component move their dot product by at most 2 * 1e-5 * sqrt(512) = 4.5e-4, far
    below the fixture's smallest boundary gap (>= 1e-2), so the hit flags cannot move."""
    paths = I.write_folders(str(tmp_path / "folders"), data)
    out_json = str(tmp_path / "id.json")
    cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "ID_retrieval", "ID_retrieval.py"), "--device", "cuda"] + paths + [
        "--dataset", I.DATASET, "--print_sim", "True", "--arcface", "True", "--arcface_ckpt", "none", "--batch-size", "5", "--num-workers", "2",
        "--json", out_json]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert "Top-1 accuracy: {:.2f}%".format(float(golden["top1"]) * 100) in lines
    assert "Top-5 accuracy: {:.2f}%".format(float(golden["top5"]) * 100) in lines
    assert "Mean ID feat:  {:.2f}".format(float(golden["mean"])) in lines
    at = lines.index("Similarities: ")
    printed = [float(l.split(":")[1]) for l in lines[at + 1:] if ":" in l]
    assert len(printed) == 16
    r = json.load(open(out_json))
    assert r["top1"] == float(golden["top1"]) and r["top5"] == float(golden["top5"]) and r["images"] == 32
    assert r["labels"] == golden["labels"].tolist() and r["rank"] == golden["rank"].tolist() and r["pred"] == golden["pred"].tolist()
    d = float(np.abs(np.array(r["similarities"]) - golden["similarities"]).max())
    print(f"CLI similarities max|d| vs reference {d:.3e}, mean |d| {abs(r['mean'] - float(golden['mean'])):.3e}, {r['images_per_s']:.1f} images/s")
    assert d <= 5e-4 and abs(r["mean"] - float(golden["mean"])) <= 5e-4
    assert np.abs(np.array(printed) - golden["similarities"]).max() <= 5e-4
