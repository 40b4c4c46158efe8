#!/usr/bin/env python3
"""A Motion-JPEG AVI from an existing folder of frames (the ``results/`` of inference_swap_video.py --paste_back / --stream): PIL reads the
PNGs, they are uploaded, and the GPU encodes them (reface_amd/mjpeg.py) -- the file ``--write_video`` would have written during the run.

Frames are taken in the callers' numeric frame order (``int(stem)``: 000000000002.png before 10.png); all must have one size.  No audio
track.

Usage: python tools/frames_to_video.py FRAMES_DIR OUT.avi [--fps 25] [--quality 90] [--subsampling 420] [--batch 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_files(frames_dir):
    """The .png files of `frames_dir` whose stem is a number, in numeric order."""
    names = [f for f in os.listdir(frames_dir) if f.lower().endswith(".png") and os.path.splitext(f)[0].isdigit()]
    return [os.path.join(frames_dir, f) for f in sorted(names, key=lambda f: (int(os.path.splitext(f)[0]), f))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("frames_dir")
    ap.add_argument("out")
    ap.add_argument("--fps", type=float, default=25.0, help="frames per second of the file (the frames carry no rate; default 25)")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", type=str, default="420", choices=["420", "444"])
    ap.add_argument("--batch", type=int, default=8, help="frames per encode call")
    a = ap.parse_args(argv)
    if not 1 <= a.quality <= 100:
        raise SystemExit(f"frames_to_video: --quality is libjpeg's 1 .. 100, got {a.quality}")
    if not a.fps > 0 or a.batch < 1:
        raise SystemExit("frames_to_video: --fps and --batch must be positive")
    files = frame_files(a.frames_dir) if os.path.isdir(a.frames_dir) else []
    if not files:
        raise SystemExit(f"frames_to_video: no <number>.png frames in {a.frames_dir}")
    import torch
    from PIL import Image
    from reface_amd.mjpeg import VideoOutput
    video = VideoOutput(a.out, a.fps, a.quality, a.subsampling, "cuda")
    size = None
    for k in range(0, len(files), a.batch):
        frames = []
        for path in files[k:k + a.batch]:
            im = Image.open(path)
            arr = np.asarray(im if im.mode in ("RGB", "RGBA") else im.convert("RGB"))
            size = size or arr.shape[:2]
            if arr.shape[:2] != size:
                raise SystemExit(f"frames_to_video: {path} is {arr.shape[1]} x {arr.shape[0]}, the frames before it {size[1]} x {size[0]}: a video has one size")
            frames.append(torch.from_numpy(arr[..., :3].copy()))
        video.push(torch.stack(frames).cuda())
    written = video.close()
    print(f"frames_to_video: {sum(n for _, n in written)} frames of {a.frames_dir} written to " + ", ".join(f"{p} ({n} frames)" for p, n in written)
          + f": Motion-JPEG AVI, {a.fps:g} fps, quality {a.quality}, {':'.join(a.subsampling)}, no audio track.")
    return written


if __name__ == "__main__":
    main()
