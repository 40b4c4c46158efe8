#!/usr/bin/env python3
"""Identity score of a swap run on the MI355X-native engines: ArcFace ID retrieval (top-1, top-5) and mean ID similarity of the swapped
results against their sources -- the reference's eval_tool/ID_retrieval/ID_retrieval.py, same positionals, options and printed lines:

    python eval_tool/ID_retrieval/ID_retrieval.py --device cuda <source images> <results> <source masks> <target masks> \\
        --dataset ffhq --print_sim True --arcface True

The four folders are listed in natural order of the file names; images and label maps are paired by position, the identity label of a
file is the first number in its name minus the smallest one of its folder, and the labels of the results index the sorted sources.
Everything after the decode runs on the GPU (reface_amd/idscore.py: rf_id_prep_u8, the ArcFace engine, rf_id_retrieve).

As in the reference, ``--mask``, ``--print_sim`` and ``--arcface`` are ``type=bool``: any non-empty value (``False`` included) switches
them on; ``--mask`` is read and not used (the mask is always applied: ``--dataset <other>`` keeps every label), and without
``--arcface`` there is no model to score with.

Additions (not in the reference): ``--arcface_ckpt`` (``none`` = the seeded weights of the tests), ``--json FILE``, ``--precision``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from reface_amd.idscore import DEFAULT_ARCFACE_CKPT
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=1, help="images per ArcFace engine run")
    p.add_argument("--num-workers", type=int, help="decode workers of the loader (default: the CPUs this process may run on, 8 at the most)")
    p.add_argument("--device", type=str, default=None, help="cuda or cuda:<i>; the HIP kernels have no CPU path")
    p.add_argument("--dataset", type=str, default="celeba", help="selects the preserved face-parsing labels: celeba | ffhq | ff++ | any other name keeps every label")
    p.add_argument("--mask", type=bool, default=True, help="accepted and ignored, as in the reference: the mask is always applied")
    p.add_argument("path", type=str, nargs=4,
                   default=["dataset/FaceData/CelebAMask-HQ/CelebA-HQ-img", "results/test_bench/results", "dataset/FaceData/CelebAMask-HQ/src_mask",
                            "dataset/FaceData/CelebAMask-HQ/target_mask"],
                   help="source images, results, source label maps, result (target) label maps")
    p.add_argument("--print_sim", type=bool, default=False)
    p.add_argument("--arcface", type=bool, default=False)
    # ---- additions
    p.add_argument("--arcface_ckpt", type=str, default=DEFAULT_ARCFACE_CKPT,
                   help="(addition) ArcFace IR-SE50 weights; 'none' = the seeded weights the tests use")
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
                   help="(addition) write top1, top5, mean, similarities, labels, image count and images/s (decode to scores; engine construction excluded) to this file")
    p.add_argument("--precision", type=str, choices=["full", "bf16"], default="full", help="(addition) precision of the ArcFace engine")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gpu_jpeg_parallel and not args.gpu_jpeg_decode:
        raise SystemExit("ID_retrieval: --gpu_jpeg_parallel chooses a plan of the GPU JPEG decoder and needs --gpu_jpeg_decode; without it no file "
                         "is decoded on the GPU")
    if args.gpu_png_parallel and not args.gpu_png_decode:
        raise SystemExit("ID_retrieval: --gpu_png_parallel chooses a plan of the GPU PNG decoder and needs --gpu_png_decode; without it no file "
                         "is decoded on the GPU")
    if not args.arcface:
        raise SystemExit("ID_retrieval: --arcface True is required (the reference defines no other identity model)")
    import torch
    from reface_amd.idscore import IDScorer, load_arcface_state
    device = torch.device(args.device if args.device is not None else "cuda")
    if device.type != "cuda":
        raise SystemExit(f"ID_retrieval: --device {args.device}: the HIP kernels run on the GPU only (there is no CPU fallback)")
    num_workers = min(len(os.sched_getaffinity(0)), 8) if args.num_workers is None else args.num_workers
    for p in args.path:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    print("Loading ResNet ArcFace")
    scorer = IDScorer(load_arcface_state(args.arcface_ckpt), precision=args.precision, batch=args.batch_size, device=device)
    if args.gpu_jpeg_decode:          # one decoder behind both flags: every file goes by its signature
        from reface_amd.jpegdec import FileDecoder
        scorer.png_decoder = FileDecoder(device, png=args.gpu_png_decode, jpeg=True, jpeg_parallel=args.gpu_jpeg_parallel, png_parallel=args.gpu_png_parallel)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import PngDecoder
        scorer.png_decoder = PngDecoder(device, parallel=args.gpu_png_parallel)
    r = scorer.score_folders(args.path, dataset=args.dataset, num_workers=num_workers)
    print("Top-1 accuracy: {:.2f}%".format(r["top1"] * 100))
    print("Top-5 accuracy: {:.2f}%".format(r["top5"] * 100))
    print("Mean ID feat:  {:.2f}".format(r["mean"]))
    if args.print_sim:
        print("Similarities: \n ")
        for i, s in enumerate(r["similarities"]):
            print(i, ":", s)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"top1": r["top1"], "top5": r["top5"], "mean": r["mean"], "similarities": [float(s) for s in r["similarities"]],
                       "labels": r["labels"], "rank": [int(k) for k in r["rank"]], "pred": [int(k) for k in r["pred"]], "images": r["images"],
                       "images_per_s": r["images_per_s"], "seconds": r["seconds"], "precision": args.precision, "dataset": args.dataset}, f)
    if args.gpu_jpeg_decode:          # (stderr: the printed lines stay what they are without the flags)
        for line in scorer.png_decoder.lines():
            print(line, file=sys.stderr)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import counts_line
        print(counts_line(scorer.png_decoder), file=sys.stderr)
    return r


if __name__ == "__main__":
    main()
