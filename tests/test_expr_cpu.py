"""The host side of the expression score (reface_amd/exprscore.py, eval_tool/Expression/expression_compare_face_recon.py) against the
reference's own outputs on the seeded folders of tests/expr_inputs.py (tests/golden/expr.npz, written by tools/gen_golden.py::gen_expr from
the reference's ReconNetWrapper, split_coeff, ImagePathDataset, compute_features and calculate_id_given_paths).  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expr_inputs as I  # noqa: E402

from reface_amd import exprscore as ES  # noqa: E402
from reface_amd import idscore as S  # noqa: E402
from reface_amd import posescore as PS  # noqa: E402
from reface_amd.params import recon_param_specs  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "expr.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


def test_prep_host_is_pil_resize_over_255(data):
    """prep_host against the reference's three lines (:125-129) written out, once per size of the fixture; a 512 x 512 image is its own bytes."""
    from PIL import Image
    seen = {}
    for im in data["tgt_images"] + data["res_images"]:
        seen.setdefault(im.shape[:2], im)
    assert set(seen) == {(512, 512), (1024, 1024), (600, 540), (57, 40)}
    for hw, im in seen.items():
        pil = Image.fromarray(im).convert("RGB").resize((512, 512), Image.BICUBIC)
        want = torch.tensor(np.array(pil) / 255., dtype=torch.float32).permute(2, 0, 1).numpy()
        got = ES.prep_host(im)
        assert got.shape == (3, 512, 512) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), hw
        if hw == (512, 512):
            assert np.array_equal(got, (im.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_byte_over_255_in_float32_equals_the_float64_division():
    b = np.arange(256)
    assert np.array_equal((b / 255.).astype(np.float32), b.astype(np.float32) / np.float32(255))


def test_file_order_and_first_number_labels(tmp_path, golden, data):
    paths = I.write_folders(str(tmp_path), data)
    tgt, res = ES.list_images_sorted(paths[0]), ES.list_images_sorted(paths[1])
    assert [os.path.basename(f) for f in tgt] == data["tgt_names"] and [os.path.basename(f) for f in res] == data["res_names"]
    assert [os.path.basename(f) for f in S.list_images(paths[1])] != data["res_names"]          # natural order would start with "8_"
    assert ES.parse_labels_first(res) == golden["labels"].tolist() == data["labels"].tolist() == I.RES_LABELS
    assert ES.parse_labels_first(res) == S.parse_labels(res)                                    # the identity metric's rule
    assert PS.parse_labels_last(res) == I.last_number_labels() != I.RES_LABELS                  # the pose metric's labelling disagrees
    assert I.RES_LABELS != list(range(8)) and min(I.RES_LABELS) == 0 and max(I.RES_LABELS) == 9
    assert ES.parse_labels_first(["a/28000_7.jpg", "a/swap_28002.png", "a/face.png", "a/x_28001-3.png"]) == [0, 2, 1]      # no number: no label
    with pytest.raises(ValueError):
        ES.parse_labels_first(["a/face.png"])


def test_score_host_vs_reference(golden):
    """calculate_id_given_paths' value and distances (:366-375) from the reference's own fp32 coefficients, and the float64 ones."""
    for tag in ("f32", "f64"):
        r = ES.score_host(golden[f"coef_{tag}_tgt"], golden[f"coef_{tag}_res"], golden["labels"])
        assert r["distances"].dtype == np.float64 and r["n"] == 8
        assert (np.abs(r["distances"] - golden[f"dist_{tag}"]) / golden[f"dist_{tag}"]).max() <= 1e-12
        assert abs(r["expression_value"] - float(golden[f"expression_value_{tag}"])) <= 1e-12 * float(golden[f"expression_value_{tag}"])
        only_exp = ES.score_host(golden[f"coef_{tag}_tgt"][:, 80:144], golden[f"coef_{tag}_res"][:, 80:144], golden["labels"])
        assert only_exp["expression_value"] == r["expression_value"]
    assert golden["coef_f32_tgt"].dtype == np.float32 and golden["coef_f64_tgt"].dtype == np.float64
    assert golden["coef_f32_tgt"].shape == (10, 257) and golden["coef_f32_res"].shape == (8, 257)
    e = max(float(np.abs(golden[f"coef_f32_{k}"][:, 80:144] - golden[f"coef_f64_{k}"][:, 80:144]).max()) for k in ("tgt", "res"))
    e_all = max(float(np.abs(golden[f"coef_f32_{k}"] - golden[f"coef_f64_{k}"]).max()) for k in ("tgt", "res"))
    assert e == float(golden["e_ref"]) and e_all == float(golden["e_ref_all"]) and 0 < e <= e_all
    with pytest.raises(IndexError):
        ES.score_host(golden["coef_f64_tgt"], golden["coef_f64_res"], [0, 1, 2, 3, 4, 5, 6, 10])
    with pytest.raises(IndexError):
        ES.score_host(golden["coef_f64_tgt"], golden["coef_f64_res"], [0, 1, 2])


def test_recon_param_specs_equal_the_reference_layout(golden):
    specs = recon_param_specs()
    assert list(specs) == golden["keys"].tolist()
    assert [",".join(str(d) for d in v) for v in specs.values()] == golden["shapes"].tolist()
    assert sum(v[0] for k, v in specs.items() if k.startswith("final_layers.") and k.endswith(".bias")) == 257
    assert not any(".fc." in k or k.startswith("backbone.fc") for k in specs)


def test_check_recon_state_is_strict(golden):
    sd = ES.load_recon_state("none")
    assert ES.check_recon_state(sd) is sd and int(golden["seed"]) == ES.SEED
    missing = dict(sd)
    del missing["final_layers.1.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        ES.check_recon_state(missing)
    extra = dict(sd)
    extra["backbone.fc.weight"] = torch.zeros(1000, 2048)
    with pytest.raises(RuntimeError, match="unexpected"):
        ES.check_recon_state(extra)
    wrong = dict(sd)
    wrong["final_layers.1.weight"] = torch.zeros(64, 2048)          # a Linear's shape, not the 1x1 convolution's
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ES.check_recon_state(wrong)
    old = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}          # checkpoints older than the counter load
    assert ES.check_recon_state(old) is old


def test_load_recon_state_reads_the_net_recon_entry(tmp_path):
    sd = ES.load_recon_state("none")
    torch.save({"net_recon": sd, "opt": 1}, str(tmp_path / "epoch_latest.pth"))
    torch.save(sd, str(tmp_path / "bare.pth"))
    for name in ("epoch_latest.pth", "bare.pth"):
        got = ES.load_recon_state(str(tmp_path / name))
        assert list(got) == list(sd) and torch.equal(got["final_layers.1.bias"], sd["final_layers.1.bias"])


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "eval_tool", "Expression"))
    import expression_compare_face_recon as cli
    return cli


def test_cli_parses_the_reference_command_line():
    cli = _cli()
    p = cli.build_parser()
    a = p.parse_args(["--device", "cuda", "dataset/FaceData/CelebAMask-HQ/Val_target", "results/REFace/results"])
    assert a.path == ["dataset/FaceData/CelebAMask-HQ/Val_target", "results/REFace/results"] and a.device == "cuda"
    assert a.batch_size == 50 and a.num_workers is None and a.print_sim is False
    assert a.recon_ckpt == "Other_dependencies/face_recon/epoch_latest.pth" and a.json is None
    b = p.parse_args(["t", "r", "--batch-size", "4", "--num-workers", "2", "--recon_ckpt", "none", "--json", "o.json", "--print_sim", "False"])
    assert b.batch_size == 4 and b.num_workers == 2 and b.recon_ckpt == "none" and b.json == "o.json" and b.print_sim is True      # type=bool
    with pytest.raises(SystemExit):
        p.parse_args(["only_one_path"])
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["t", "r", "--device", "cpu"])


def test_cli_refuses_npz(tmp_path):
    cli = _cli()
    stats = tmp_path / "stats.npz"
    np.savez(str(stats), mu=np.zeros(3), sigma=np.eye(3))
    (tmp_path / "results").mkdir()
    with pytest.raises(SystemExit, match="npz statistics are not supported"):
        cli.main([str(stats), str(tmp_path / "results"), "--recon_ckpt", "none"])


def test_cli_refuses_a_folder_without_numbered_names(tmp_path, data):
    """The labels are read before any weights are loaded: a folder whose names carry no number cannot be scored."""
    from PIL import Image
    cli = _cli()
    (tmp_path / "targets").mkdir()
    (tmp_path / "results").mkdir()
    Image.fromarray(data["tgt_images"][5]).save(str(tmp_path / "targets" / "3_100.png"))
    Image.fromarray(data["res_images"][4]).save(str(tmp_path / "results" / "face.png"))
    assert [os.path.basename(f) for f in ES.list_images_sorted(str(tmp_path / "results"))] == ["face.png"]
    with pytest.raises(SystemExit, match="no file name carries a number"):
        cli.main([str(tmp_path / "targets"), str(tmp_path / "results"), "--recon_ckpt", "none"])
    with pytest.raises(SystemExit, match="no file name carries a number"):
        cli.main([str(tmp_path / "results"), str(tmp_path / "targets"), "--recon_ckpt", "none"])


def test_ops_are_exported_and_refuse_host_tensors():
    from reface_amd import _lib, ops
    assert {"rf_expr_prep_u8", "rf_expr_head", "rf_expr_distance"} <= set(_lib.EXPORTS)
    assert ops.ACT_ADD_RELU == 8 and ops.ACT_RELU == 5
    t = (torch.zeros(512, 2, dtype=torch.int32), torch.zeros(512, 1, dtype=torch.int32))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.expr_prep_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), t, t, torch.zeros(1, 512, 512, 8))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.expr_head(torch.zeros(1, 256, 2048), torch.zeros(257, 2048), torch.zeros(257), torch.zeros(1, 257))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.expr_distance(torch.zeros(2, 257), torch.zeros(3, 257), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64),
                          torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ES.ExprScorer(ES.load_recon_state("none"), device="cpu")
