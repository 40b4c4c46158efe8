#!/usr/bin/env python3
"""The streamed video route's device work per batch (reface_amd/stream.py), timed with HIP events around whole batches, data already on the
device (no PNG decode / encode, no copies):
  prep    rf_video_prep_u8: B crops 1024^2 + label maps 512^2 -> target, keep-mask, masked target (one launch)
  chain   the four launches it replaces on the device: rf_resample_u8 (bicubic taps, through a [B, 1024, 512, 3] u8 intermediate and a
          512^2 u8 image) + rf_u8_to_norm + rf_label_mask + rf_mul_mask
  stream  the whole device chain of one batch of 1080p frames without the model: align -> parse -> prep, then paste crop -> paste back
          (VideoStream.prepare + VideoStream.paste on frames that are on the device; seeded parser weights)
One JSON line.

Usage: python tools/stream_rate.py [--batch 10] [--iters 200] [--warmup 5] [--chain-iters 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reface_amd import ops  # noqa: E402
from reface_amd.align import resample_taps  # noqa: E402
from reface_amd.stream import VideoStream, keep_lut  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def face_landmarks(cx, cy, eye):
    lm = np.zeros((68, 2))
    lm[:] = [cx, cy]
    lm[36:42] = [cx - 0.5 * eye, cy]
    lm[42:48] = [cx + 0.5 * eye, cy + 0.05 * eye]
    lm[48], lm[54] = [cx - 0.35 * eye, cy + 0.9 * eye], [cx + 0.35 * eye, cy + 0.9 * eye]
    return lm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chain-iters", type=int, default=10)
    a = ap.parse_args()
    B, S, h = a.batch, 1024, 512
    g = torch.Generator().manual_seed(0)
    crops = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).cuda()
    labels = torch.randint(0, 19, (B, h, h), dtype=torch.uint8, generator=g).cuda()
    lut = torch.from_numpy(keep_lut([1, 2, 3, 5, 6, 7, 9])).cuda()
    taps = tuple(torch.from_numpy(t).cuda() for t in resample_taps(S, h, "bicubic"))
    target, inpaint = (torch.empty((B, 3, h, h), dtype=torch.float32, device="cuda") for _ in range(2))
    mask = torch.empty((B, 1, h, h), dtype=torch.float32, device="cuda")
    prep = [ops.video_prep_u8(crops, labels, lut, taps, taps, target, mask, inpaint)]
    t_prep = timed(lambda: ops.run(prep), a.iters, a.warmup)
    tmp = torch.empty((B, S, h, 3), dtype=torch.uint8, device="cuda")
    small = torch.empty((B, h, h, 3), dtype=torch.uint8, device="cuda")
    half = torch.full((3,), 0.5, dtype=torch.float32, device="cuda")
    t2, i2, m2 = torch.empty_like(target), torch.empty_like(inpaint), torch.empty_like(mask)
    four = [ops.resample_u8(crops, taps, taps, tmp, small), ops.u8_to_norm(small, half, half, t2), ops.label_mask(labels, lut, m2, invert=True),
            ops.mul_mask(t2, m2, i2)]
    t_four = timed(lambda: ops.run(four), a.iters, a.warmup)
    each = [timed(lambda l=l: l(), a.iters, a.warmup) for l in four]
    assert torch.equal(t2, target) and torch.equal(m2, mask) and torch.equal(i2, inpaint)
    # the whole device chain of a batch of 1080p frames (no model between prepare and paste: the swapped crops are a fixed tensor)
    H, W = 1080, 1920
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    lm = np.stack([face_landmarks(960.0 + 3 * i, 480.0, 170.0) for i in range(B)])
    vs = VideoStream(lm, [1, 2, 3, 5, 6, 7, 9], seg_ckpt="none")
    ids = [str(i).zfill(12) for i in range(B)]
    x_img = torch.rand((B, 3, h, h), device="cuda")
    state = {}

    def prepare():
        state["s"] = vs.prepare(frames, ids)[2]

    t_prepare = timed(prepare, a.chain_iters, 2)
    t_paste = timed(lambda: vs.paste(x_img, state["s"]), a.chain_iters, 2)
    mb = lambda *ts: sum(t.numel() * t.element_size() for t in ts) / 1e6          # noqa: E731
    print(json.dumps({"metric": "stream_ms_per_batch", "batch": B, "crop": S, "image": h, "video_prep_ms": round(t_prep, 4),
                      "four_launch_chain_ms": round(t_four, 4), "chain_parts_ms": {"resample_u8": round(each[0], 4), "u8_to_norm": round(each[1], 4),
                                                                                  "label_mask": round(each[2], 4), "mul_mask": round(each[3], 4)},
                      "video_prep_compulsory_MB": round(mb(crops, labels, target, mask, inpaint), 1),
                      "video_prep_GBps": round(mb(crops, labels, target, mask, inpaint) / t_prep, 1),
                      "frame": f"{W}x{H}", "prepare_ms": round(t_prepare, 3), "paste_ms": round(t_paste, 3),
                      "device_chain_ms": round(t_prepare + t_paste, 3)}))


if __name__ == "__main__":
    main()
