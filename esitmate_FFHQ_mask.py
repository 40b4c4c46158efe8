#!/usr/bin/env python3
"""FFHQ face-parsing masks on the GPU: the reference's esitmate_FFHQ_mask.py (same file name, same flags) on the HIP BiSeNet engine.

Reads ``<FFHQ_root>/images512/*.png``, resizes each to 1024^2 (PIL bilinear, as the reference does before parsing) and writes the 512^2
label map to ``<FFHQ_root>/BiSeNet_mask/<name>.png`` -- what the FFHQ reader (reface_amd/data.py) loads.  Images are parsed in device
batches of ``--batch_size``.  ``--save_vis`` (an OpenCV colour blend) and the SegNeXt parser are not built and are refused.
"""
import glob
import os
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = ArgumentParser()
    p.add_argument("--faceParser_name", default="default", type=str, help="face parser name; only 'default' (BiSeNet) is built")
    p.add_argument("--faceParsing_ckpt", type=str, default="Other_dependencies/face_parsing/79999_iter.pth",
                   help="BiSeNet checkpoint (79999_iter.pth); 'none' = seeded weights")
    p.add_argument("--segnext_config", default="", type=str, help="SegNeXt configuration (not supported)")
    p.add_argument("--FFHQ_root", type=str, default="dataset/FaceData/FFHQ")
    p.add_argument("--save_vis", action="store_true", help="colour visualisations (not supported: needs OpenCV)")
    p.add_argument("--seg12", action="store_true", help="write the 12-class maps instead of the 19-class ones")
    # additions (not in the reference)
    p.add_argument("--batch_size", type=int, default=16, help="images per device batch")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.save_vis:
        raise SystemExit("esitmate_FFHQ_mask: --save_vis (the OpenCV colour blend) is not supported by this build")
    if args.faceParser_name != "default":
        raise SystemExit(f"esitmate_FFHQ_mask: face parser {args.faceParser_name!r} is not supported by this build (only 'default', BiSeNet)")
    from reface_amd.parsing import parse_label_maps
    mask_dir = os.path.join(args.FFHQ_root, "BiSeNet_mask")
    os.makedirs(mask_dir, exist_ok=True)
    imgs = sorted(glob.glob(os.path.join(args.FFHQ_root, "images512", "*.png")), reverse=True)
    parse_label_maps([(f, os.path.join(mask_dir, os.path.basename(f))) for f in imgs], args.faceParsing_ckpt, seg12=args.seg12,
                     batch=args.batch_size)
    print(f"[esitmate_FFHQ_mask] {len(imgs)} label maps written to {mask_dir}")
    return len(imgs)


if __name__ == "__main__":
    main()
