#!/usr/bin/env python3
"""Perceptual distance of a swap run on the MI355X-native engines: the mean LPIPS distance (eval_tool/lpips/lpips.py of the reference,
AlexNet by default) between every swapped result and its target.  The reference ships the metric as a module only; this command is modelled
on its sibling tools:

    python eval_tool/lpips/lpips_compare.py --device cuda <target images> <results>

Both folders are listed in natural order.  The label of a result is the LAST number in its file name minus the smallest one of its folder,
and it is a position in the sorted target list, exactly as the pose metric pairs them: that target is the image the result is compared with.
A result and its target must have the same size (nothing is resized).  Everything after the decode runs on the GPU (reface_amd/lpips.py:
rf_lpips_prep_u8, the feature stack on rf_conv_gemm and rf_maxpool2d, rf_lpips_layer, rf_lpips_total), in fp32.  ``.npz`` paths are refused.
``--print_sim`` is ``type=bool`` as in the siblings: any non-empty string is true.

The weights are not downloaded: ``--lpips_ckpt`` names a state dict of the LPIPS module or a REFace checkpoint that holds ``lpips_loss.*``
keys; ``none`` selects the seeded weights of the tests.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=16, help="pairs per engine run (capped per image size so that no tensor reaches 2^31 bytes)")
    p.add_argument("--num-workers", type=int, help="decode workers of the loader (default: the CPUs this process may run on, 8 at the most)")
    p.add_argument("--device", type=str, default=None, help="cuda or cuda:<i>; the HIP kernels have no CPU path")
    p.add_argument("path", type=str, nargs=2, help="target images, results")
    p.add_argument("--net", type=str, default="alex", choices=["alex", "vgg"], help="the backbone whose features are compared")
    p.add_argument("--lpips_ckpt", type=str, default="models/REFace/checkpoints/last.ckpt",
                   help="LPIPS weights: a state dict of the module or a REFace checkpoint with lpips_loss.* keys; 'none' = the seeded weights the tests use")
    p.add_argument("--print_sim", type=bool, default=False, help="also print one distance per result (any non-empty string is true)")
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
                   help="write LPIPS_value, distances, labels, image count and images/s (decode to score; engine construction excluded) to this file")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gpu_jpeg_parallel and not args.gpu_jpeg_decode:
        raise SystemExit("lpips_compare: --gpu_jpeg_parallel chooses a plan of the GPU JPEG decoder and needs --gpu_jpeg_decode; without it no file "
                         "is decoded on the GPU")
    if args.gpu_png_parallel and not args.gpu_png_decode:
        raise SystemExit("lpips_compare: --gpu_png_parallel chooses a plan of the GPU PNG decoder and needs --gpu_png_decode; without it no file "
                         "is decoded on the GPU")
    import torch
    from reface_amd.idscore import list_images
    from reface_amd.lpips import NPZ_REFUSED, LPIPSScorer, load_lpips_state
    from reface_amd.posescore import parse_labels_last
    device = torch.device(args.device if args.device is not None else "cuda")
    if device.type != "cuda":
        raise SystemExit(f"lpips_compare: --device {args.device}: the HIP kernels run on the GPU only (there is no CPU fallback)")
    num_workers = min(len(os.sched_getaffinity(0)), 8) if args.num_workers is None else args.num_workers
    for p in args.path:
        if p.endswith(".npz"):
            raise SystemExit(f"lpips_compare: {p}: {NPZ_REFUSED}")
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    try:          # refuse names without numbers before any weights are loaded
        parse_labels_last(list_images(args.path[1]))
    except ValueError as e:
        raise SystemExit(f"lpips_compare: {args.path[1]}: {e}")
    state = load_lpips_state(args.lpips_ckpt, args.net)
    print("Loading LPIPS(%s) from %s" % (args.net, args.lpips_ckpt))
    scorer = LPIPSScorer(state, net=args.net, batch=args.batch_size, device=device)
    if args.gpu_jpeg_decode:          # one decoder behind both flags: every file goes by its signature
        from reface_amd.jpegdec import FileDecoder
        scorer.png_decoder = FileDecoder(device, png=args.gpu_png_decode, jpeg=True, jpeg_parallel=args.gpu_jpeg_parallel, png_parallel=args.gpu_png_parallel)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import PngDecoder
        scorer.png_decoder = PngDecoder(device, parallel=args.gpu_png_parallel)
    try:
        r = scorer.score_folders(args.path, num_workers=num_workers)
    except ValueError as e:          # a result whose size differs from its target's, an image too small for the net
        raise SystemExit(f"lpips_compare: {e}")
    print("LPIPS_value: ", r["lpips_value"])
    if args.print_sim:
        print("Similarities: \n ")
        for i in range(len(r["distances"])):
            print(i, ":", r["distances"][i])
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"lpips_value": r["lpips_value"], "distances": [float(d) for d in r["distances"]],
                       "labels": r["labels"], "net": args.net, "images": r["images"], "images_per_s": r["images_per_s"], "seconds": r["seconds"]}, f)
    if args.gpu_jpeg_decode:          # (stderr: the printed lines stay what they are without the flags)
        for line in scorer.png_decoder.lines():
            print(line, file=sys.stderr)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import counts_line
        print(counts_line(scorer.png_decoder), file=sys.stderr)
    return r


if __name__ == "__main__":
    main()
