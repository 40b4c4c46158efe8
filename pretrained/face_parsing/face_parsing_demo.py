"""Drop-in for the reference's pretrained/face_parsing/face_parsing_demo.py: the same two entry points, with the same signatures and
return types, on the HIP BiSeNet engine (reface_amd/parsing.py).

  init_faceParsing_pretrained_model("default", ckpt)  -> FaceParser(ckpt)     (ckpt "none": seeded weights)
  faceParsing_demo(parser, pil_1024, convert_to_seg12) -> uint8 numpy [512, 512] label map (19 classes, or 12 with convert_to_seg12)

The SegNeXt parser ("segnext", an mmsegmentation model) is not built.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reface_amd.parsing import FaceParser, seg12_lut  # noqa: E402,F401

_SEGNEXT = "face parser 'segnext' (mmsegmentation SegNeXt) is not supported by this build; use faceParser_name='default' (BiSeNet)"


def init_faceParsing_pretrained_model(faceParser_name, ckpt_path, config_path=""):
    if faceParser_name == "default":
        return FaceParser(seg_ckpt=ckpt_path)
    if faceParser_name == "segnext":
        raise NotImplementedError(_SEGNEXT)
    raise ValueError(f"unknown face parser {faceParser_name!r} (supported: 'default')")


def faceParsing_demo(model, img, convert_to_seg12=True, model_name="default"):
    """model: a FaceParser; img: PIL image (RGB, 1024^2 in every caller) -> uint8 numpy label map [H/2, W/2]."""
    if model_name == "segnext":
        raise NotImplementedError(_SEGNEXT)
    if model_name != "default":
        raise ValueError(f"unknown face parser {model_name!r} (supported: 'default')")
    return model.parse(np.asarray(img.convert("RGB")), seg12=convert_to_seg12)[0].cpu().numpy()
