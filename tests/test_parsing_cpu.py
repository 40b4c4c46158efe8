"""Face parser (BiSeNet, pretrained/face_parsing/ of the reference) -- the host side: checkpoint key layout, the seg12 table, the
GPU-only contract and the front-end's flags.  No GPU needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bisenet_param_specs_match_reference_keys(golden_dir):
    from reface_amd.params import bisenet_param_specs
    ref = json.load(open(os.path.join(golden_dir, "bisenet_keys.json")))
    spec = bisenet_param_specs()
    assert [k for k, _ in ref] == list(spec)
    assert all(tuple(shape) == spec[k] for k, shape in ref)


def test_seg12_lut_matches_reference(golden_dir):
    from reface_amd.parsing import identity_lut, seg12_lut
    g = np.load(os.path.join(golden_dir, "bisenet.npz"))
    lut = seg12_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    assert np.array_equal(lut[:19], g["lut_seg12"])
    assert np.array_equal(lut[g["labels"]], g["labels_seg12"])
    assert np.array_equal(identity_lut(), np.arange(256))


def test_face_parser_needs_a_gpu(monkeypatch):
    from reface_amd.parsing import FaceParser
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU only"):
        FaceParser("none")
    sys.path.insert(0, ROOT)
    from pretrained.face_parsing.face_parsing_demo import init_faceParsing_pretrained_model
    with pytest.raises(RuntimeError, match="GPU only"):
        init_faceParsing_pretrained_model("default", "none")
    with pytest.raises(NotImplementedError, match="segnext"):
        init_faceParsing_pretrained_model("segnext", "x.pth", "cfg.py")


def test_checkpoint_loading_is_strict(tmp_path):
    from reface_amd.params import bisenet_param_specs, seeded_state_dict
    from reface_amd.parsing import SEED, load_bisenet_state
    sd = seeded_state_dict(bisenet_param_specs(), SEED)
    none = load_bisenet_state("none")
    assert list(none) == list(sd) and all(torch.equal(none[k], sd[k]) for k in sd)
    old = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}      # checkpoints older than the counter load
    torch.save(old, tmp_path / "old.pth")
    assert set(load_bisenet_state(str(tmp_path / "old.pth"))) == set(old)
    torch.save({k: v for k, v in old.items() if "conv_out32" not in k}, tmp_path / "noaux.pth")
    with pytest.raises(RuntimeError, match="missing"):
        load_bisenet_state(str(tmp_path / "noaux.pth"))                                 # aux heads are part of the strict key set
    torch.save(dict(old, extra=torch.zeros(1)), tmp_path / "extra.pth")
    with pytest.raises(RuntimeError, match="unexpected"):
        load_bisenet_state(str(tmp_path / "extra.pth"))
    bad = dict(old)
    bad["conv_out.conv_out.weight"] = torch.zeros(12, 256, 1, 1)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="shape"):
        load_bisenet_state(str(tmp_path / "bad.pth"))


def test_estimate_ffhq_mask_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "esitmate_FFHQ_mask.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--faceParser_name", "--faceParsing_ckpt", "--segnext_config", "--FFHQ_root", "--save_vis", "--seg12"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "esitmate_FFHQ_mask.py"), "--save_vis", "--FFHQ_root", "/nonexistent"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--save_vis" in r.stderr


@pytest.mark.parametrize("script", ["inference_swap_selected.py", "inference_swap_video.py"])
def test_swap_clis_take_parse_masks(script):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    mod = __import__(script[:-3])
    opt = mod.build_parser().parse_args([])
    assert opt.parse_masks is False
    assert mod.build_parser().parse_args(["--parse_masks"]).parse_masks is True
