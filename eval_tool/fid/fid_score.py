#!/usr/bin/env python3
"""FID of a swap run on the MI355X-native engines: the Frechet distance between the Gaussians fitted to the ``clip`` ViT-B/32 image features
of two image folders -- the reference's eval_tool/fid/fid_score.py (whose "inception" returns ``clip_model.encode_image``), same positionals,
options and printed line:

    python eval_tool/fid/fid_score.py --device cuda <dataset images | stats.npz> <results>

Each folder is listed as the reference lists it (``glob('*.ext')`` per image extension, sorted).  Everything between the decode and the
mean / covariance runs on the GPU (reface_amd/fidscore.py: rf_fid_prep_u8, the vision tower, rf_fid_stats); the Frechet step is the
reference's ``scipy.linalg.sqrtm`` on the host.  ``--dims`` is accepted and unused, as in the reference.  A path ending in ``.npz`` is read
for its ``mu`` and ``sigma``.

Additions (not in the reference): ``--clip_ckpt`` (the file ``clip.load`` caches; ``none`` = the seeded tower of the tests), ``--precision``,
``--json FILE``, ``--save-stats FILE.npz`` (``mu`` and ``sigma`` of the first path: a large dataset folder is featurised once).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from reface_amd.fidscore import DEFAULT_CLIP_CKPT
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=50, help="Batch size to use")
    p.add_argument("--num-workers", type=int, help="decode workers of the loader (default: the CPUs this process may run on, 8 at the most)")
    p.add_argument("--device", type=str, default=None, help="cuda or cuda:<i>; the HIP kernels have no CPU path")
    p.add_argument("--dims", type=int, default=2048, choices=[64, 192, 768, 2048], help="accepted and unused, as in the reference: the features are CLIP's 512")
    p.add_argument("path", type=str, nargs=2, default=["dataset/FaceData/CelebAMask-HQ/CelebA-HQ-img", "results/test_bench/results"],
                   help="Paths to the images or to .npz statistic files")
    # ---- additions
    p.add_argument("--clip_ckpt", type=str, default=DEFAULT_CLIP_CKPT,
                   help="(addition) the ViT-B/32 file clip.load caches (TorchScript archive or state dict); 'none' = the seeded tower the tests use")
    p.add_argument("--precision", type=str, default="full", choices=["full", "bf16"], help="(addition) tower arithmetic: fp32, or bf16 operands")
    p.add_argument("--gpu_png_decode", action="store_true",
                   help="(addition) decode PNG files on the GPU (reface_amd/pngdec.py): the loader's workers only read bytes; the values are the same")
    p.add_argument("--gpu_jpeg_decode", action="store_true",
                   help="(addition) decode baseline JPEG files on the GPU (reface_amd/jpegdec.py): the loader's workers only read bytes; the values are "
                        "the same.  Independent of --gpu_png_decode; both may be given")
    p.add_argument("--gpu_jpeg_parallel", action="store_true",
                   help="(addition) with --gpu_jpeg_decode: files without restart markers are decoded by one lane per sub-sequence of the scan "
                        "(the self-synchronising plan of reface_amd/jpegdec.py) instead of one lane per file; the values are the same")
    p.add_argument("--gpu_png_parallel", action="store_true",
                   help="(addition) with --gpu_png_decode: PNG files that --gpu_png did not write are inflated by one wave per dynamic Huffman block "
                        "(the blocks plan of reface_amd/pngdec.py) instead of one wave per file; the values are the same")
    p.add_argument("--json", type=str, default=None,
                   help="(addition) write the value, its four terms, image counts, images/s (decode to value; engine construction excluded) and the "
                        "number of images prepared on the host to this file")
    p.add_argument("--save-stats", type=str, default=None, help="(addition) write mu and sigma of the first path to this .npz file")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gpu_jpeg_parallel and not args.gpu_jpeg_decode:
        raise SystemExit("fid_score: --gpu_jpeg_parallel chooses a plan of the GPU JPEG decoder and needs --gpu_jpeg_decode; without it no file "
                         "is decoded on the GPU")
    if args.gpu_png_parallel and not args.gpu_png_decode:
        raise SystemExit("fid_score: --gpu_png_parallel chooses a plan of the GPU PNG decoder and needs --gpu_png_decode; without it no file "
                         "is decoded on the GPU")
    import numpy as np
    import torch
    from reface_amd.fidscore import FidScorer, load_fid_clip_state
    device = torch.device(args.device if args.device is not None else "cuda")
    if device.type != "cuda":
        raise SystemExit(f"fid_score: --device {args.device}: the HIP kernels run on the GPU only (there is no CPU fallback)")
    num_workers = min(len(os.sched_getaffinity(0)), 8) if args.num_workers is None else args.num_workers
    for p in args.path:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    state, _ = load_fid_clip_state(args.clip_ckpt)
    scorer = FidScorer(state, precision=args.precision, batch=args.batch_size, device=device)
    if args.gpu_jpeg_decode:          # one decoder behind both flags: every file goes by its signature
        from reface_amd.jpegdec import FileDecoder
        scorer.png_decoder = FileDecoder(device, png=args.gpu_png_decode, jpeg=True, jpeg_parallel=args.gpu_jpeg_parallel, png_parallel=args.gpu_png_parallel)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import PngDecoder
        scorer.png_decoder = PngDecoder(device, parallel=args.gpu_png_parallel)
    r = scorer.score_folders(args.path, num_workers=num_workers)
    fid_value = r["fid"]
    print("FID: ", fid_value)
    if args.save_stats:
        np.savez(args.save_stats, mu=r["mu1"], sigma=r["sigma1"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump({k: r[k] for k in ("fid", "mean_term", "trace1", "trace2", "trace_covmean", "images1", "images2", "images", "host_prepared",
                                         "images_per_s", "seconds")} | {"precision": args.precision}, f)
    if args.gpu_jpeg_decode:          # (stderr: the printed lines stay what they are without the flags)
        for line in scorer.png_decoder.lines():
            print(line, file=sys.stderr)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import counts_line
        print(counts_line(scorer.png_decoder), file=sys.stderr)
    return r


if __name__ == "__main__":
    main()
