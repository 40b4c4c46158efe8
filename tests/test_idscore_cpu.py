"""The identity score, host side (reface_amd/idscore.py, eval_tool/ID_retrieval/ID_retrieval.py): the host restatements of the reference's
item preparation and scoring against the reference's own outputs (tests/golden/idscore.npz, tools/gen_golden.py:gen_idscore), file
ordering and label parsing, the C-ABI entries and the CLI's argument surface."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import idscore_inputs as I  # noqa: E402

from reface_amd import idscore as S  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "idscore.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


def test_fixture_is_not_trivial(golden):
    """Neither accuracy is 0 or 1, and every hit flag is at least 1e-2 of score away from flipping (the generator's condition)."""
    assert 0.0 < float(golden["top1"]) < float(golden["top5"]) < 1.0
    assert golden["gaps"].min() >= 1e-2
    assert golden["f_src"].shape == (16, 512) and golden["f_res"].shape == (16, 512)


def test_prep_host_matches_reference(golden, data):
    """MaskedImagePathDataset.__getitem__ of the reference (with cv2's resize restated: see the fixture's docstring) == prep_host."""
    keep = S.preserve_labels(I.DATASET)
    for key, imgs, labs, idx in (("prep_src", data["src_images"], data["src_labels"], I.PREP_SAMPLES["src"]),
                                 ("prep_res", data["res_images"], data["res_labels"], I.PREP_SAMPLES["res"])):
        for g, i in zip(golden[key], idx):
            x = S.prep_host(imgs[i], labs[i], keep)
            assert x.shape == (3, 112, 112) and x.dtype == np.float32
            d = float(np.abs(x - g).max())
            print(f"{key}[{i}]: max|prep_host - reference| = {d:.3e}")
            assert np.array_equal(x, g), d          # the same fp32 operations in the same order
    for g, i in zip(golden["prep_src_nomask"], I.PREP_SAMPLES["src"]):          # `--dataset <other>`: every label kept, mask == 1
        x = S.prep_host(data["src_images"][i], data["src_labels"][i], S.preserve_labels("other"))
        assert np.array_equal(x, g)
    m = S.prep_host(data["src_images"][0], data["src_labels"][0], keep)
    assert (m == 0).mean() > 0.2 and (m != 0).mean() > 0.2          # the mask cuts a real part of the image away and keeps a real part


def test_score_host_matches_reference(golden):
    r = S.score_host(golden["f_src"], golden["f_res"], golden["labels"])
    assert r["top1"] == float(golden["top1"]) and r["top5"] == float(golden["top5"])
    assert np.abs(r["similarities"] - golden["similarities"]).max() <= 1e-12
    assert abs(r["mean"] - float(golden["mean"])) <= 1e-12
    assert np.array_equal(r["rank"], golden["rank"]) and np.array_equal(r["pred"], golden["pred"])
    assert np.allclose(S.boundary_gaps(golden["f_src"], golden["f_res"], golden["labels"]), golden["gaps"], rtol=0, atol=1e-12)


def test_score_host_ties_go_to_the_lower_index():
    f_src = np.zeros((4, 512), dtype=np.float32)
    f_src[0, 0] = f_src[1, 1] = f_src[2, 1] = f_src[3, 2] = 1.0          # sources 1 and 2 are the same vector
    f_res = np.zeros((2, 512), dtype=np.float32)
    f_res[:, 1] = 1.0
    r = S.score_host(f_src, f_res, [1, 2])
    assert r["pred"].tolist() == [1, 1] and r["rank"].tolist() == [0, 1] and r["top1"] == 0.5 and r["top5"] == 1.0
    with pytest.raises(IndexError):
        S.score_host(f_src, f_res, [1, 4])


def test_file_order_and_labels(tmp_path):
    names = ["10.png", "2.png", "000003_x.jpg", "1_b.png", "notes.txt", "7.PNG", "12-5.jpeg"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    files = S.list_images(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["1_b.png", "2.png", "000003_x.jpg", "10.png", "12-5.jpeg"]
    assert S.parse_labels(files) == [0, 1, 2, 9, 11]          # first number of each name minus the smallest (1)
    assert S.parse_labels(["a/28000.jpg", "a/28002_swap.png", "a/face.png", "a/x_28001.png"]) == [0, 2, 1]          # no number: no label
    with pytest.raises(ValueError):
        S.parse_labels(["a/face.png"])
    assert sorted(["a10b2", "a10b10", "a9", "b1", "10"], key=S.natural_key) == ["10", "a9", "a10b2", "a10b10", "b1"]


def test_fixture_folders_sort_into_fixture_order(tmp_path, data):
    paths = I.write_folders(str(tmp_path), data)
    assert [os.path.basename(f) for f in S.list_images(paths[0])] == data["src_names"]
    res = S.list_images(paths[1])
    assert [os.path.basename(f) for f in res] == data["res_names"]
    assert S.parse_labels(res) == data["labels"].tolist()
    assert S.parse_labels(S.list_images(paths[0])) == list(range(16))
    img, lab = S.read_pair(os.path.join(paths[0], data["src_names"][3]), os.path.join(paths[2], data["src_names"][3]))
    assert np.array_equal(img, data["src_images"][3]) and np.array_equal(lab, data["src_labels"][3])          # PNG: lossless


def test_preserve_lists():
    assert S.preserve_labels("celeba") == [1, 2, 4, 5, 8, 9, 6, 7, 10, 11, 12]
    assert S.preserve_labels("ffhq") == [1, 2, 3, 5, 6, 7, 9]
    assert S.preserve_labels("ff++") == [1, 2, 4, 5, 8, 9]
    assert S.preserve_labels("anything") == list(range(21))


def test_cli_parses_the_reference_command_lines():
    """The two invocations of the reference's evaluate_all.sh, and the defaults of its parser."""
    sys.path.insert(0, os.path.join(ROOT, "eval_tool", "ID_retrieval"))
    import ID_retrieval as cli
    p = cli.build_parser()
    a = p.parse_args(["--device", "cuda", "dataset/FaceData/FFHQ/Val", "results/REFace/FFHQ/results", "dataset/FaceData/FFHQ/src_mask",
                      "dataset/FaceData/FFHQ/target_mask", "--dataset", "ffhq", "--print_sim", "True", "--arcface", "True"])
    assert a.path == ["dataset/FaceData/FFHQ/Val", "results/REFace/FFHQ/results", "dataset/FaceData/FFHQ/src_mask", "dataset/FaceData/FFHQ/target_mask"]
    assert a.device == "cuda" and a.dataset == "ffhq" and a.print_sim is True and a.arcface is True
    assert a.batch_size == 1 and a.num_workers is None and a.mask is True
    assert a.arcface_ckpt == "Other_dependencies/arcface/model_ir_se50.pth" and a.json is None and a.precision == "full"
    b = p.parse_args(["s", "r", "sm", "tm", "--batch-size", "50", "--num-workers", "4", "--arcface_ckpt", "none", "--json", "o.json", "--precision", "bf16"])
    assert b.batch_size == 50 and b.num_workers == 4 and b.dataset == "celeba" and b.print_sim is False and b.arcface is False
    assert b.arcface_ckpt == "none" and b.json == "o.json" and b.precision == "bf16"
    with pytest.raises(SystemExit):
        p.parse_args(["only", "three", "paths"])
    with pytest.raises(SystemExit, match="--arcface"):
        cli.main(["s", "r", "sm", "tm"])
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["s", "r", "sm", "tm", "--arcface", "True", "--device", "cpu"])


def test_ops_are_exported_and_refuse_host_tensors():
    from reface_amd import _lib, ops
    assert {"rf_id_prep_u8", "rf_id_retrieve"} <= set(_lib.EXPORTS)
    u8 = torch.uint8
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.id_prep_u8(torch.zeros(1, 8, 8, 3, dtype=u8), torch.zeros(1, 4, 4, dtype=u8), torch.zeros(256, dtype=u8), torch.zeros(1, 3, 112, 112))
    i32 = torch.int32
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.id_retrieve(torch.zeros(2, 512), torch.zeros(3, 512), torch.zeros(2, dtype=i32), torch.zeros(2, 5, dtype=i32), torch.zeros(2, dtype=i32),
                        torch.zeros(2, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.IDScorer({}, device="cpu")


def test_backbone_id_entry_refuses_the_cpu():
    from reface_amd.encoders import Backbone
    net = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_id112(torch.zeros(1, 3, 112, 112))
