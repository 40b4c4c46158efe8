#!/usr/bin/env python3
"""Expression score of a swap run on the MI355X-native engines: the mean L2 distance between the 64 expression coefficients that
Deep3DFaceRecon's net_recon predicts for the swapped results and for their targets -- the reference's
eval_tool/Expression/expression_compare_face_recon.py, same positionals, options and printed lines:

    python eval_tool/Expression/expression_compare_face_recon.py --device cuda <target images> <results>

Both folders are listed in plain ``sorted()`` order of the file names.  The label of a result is the FIRST number in its file name minus
the smallest one of its folder, and it is a position in the sorted target list: that target's coefficients are the ones the result is
compared with.  Everything after the decode runs on the GPU (reface_amd/exprscore.py: rf_expr_prep_u8, the ResNet-50 engine, rf_expr_head,
rf_expr_distance), in fp32.  ``.npz`` paths are refused: the reference's branch for them cannot run.  ``--print_sim`` is ``type=bool`` as in
the reference: any non-empty string is true.

Additions (not in the reference): ``--recon_ckpt`` (``none`` = the seeded weights of the tests), ``--json FILE``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from reface_amd.exprscore import DEFAULT_RECON_CKPT
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=50, help="images per loader batch (run as engine batches of exprscore.ENGINE_B at the most)")
    p.add_argument("--num-workers", type=int, help="decode workers of the loader (default: the CPUs this process may run on, 8 at the most)")
    p.add_argument("--device", type=str, default=None, help="cuda or cuda:<i>; the HIP kernels have no CPU path")
    p.add_argument("path", type=str, nargs=2,
                   default=["dataset/FaceData/CelebAMask-HQ/Val_target", "results_grad/v4_reconstruct_img_train_2_step_multi_false_with_LPIPS_ep16/results"],
                   help="target images, results")
    p.add_argument("--print_sim", type=bool, default=False, help="also print one distance per result (any non-empty string is true)")
    # ---- additions
    p.add_argument("--recon_ckpt", type=str, default=DEFAULT_RECON_CKPT, help="(addition) net_recon weights (epoch_latest.pth); 'none' = the seeded weights the tests use")
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
                   help="(addition) write Expression_value, distances, labels, expression coefficients, image count and images/s (decode to score; engine "
                        "construction excluded) to this file")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gpu_jpeg_parallel and not args.gpu_jpeg_decode:
        raise SystemExit("expression_compare_face_recon: --gpu_jpeg_parallel chooses a plan of the GPU JPEG decoder and needs --gpu_jpeg_decode; without it no file "
                         "is decoded on the GPU")
    if args.gpu_png_parallel and not args.gpu_png_decode:
        raise SystemExit("expression_compare_face_recon: --gpu_png_parallel chooses a plan of the GPU PNG decoder and needs --gpu_png_decode; without it no file "
                         "is decoded on the GPU")
    import torch
    from reface_amd.exprscore import NPZ_REFUSED, ExprScorer, list_images_sorted, load_recon_state, parse_labels_first
    device = torch.device(args.device if args.device is not None else "cuda")
    if device.type != "cuda":
        raise SystemExit(f"expression_compare_face_recon: --device {args.device}: the HIP kernels run on the GPU only (there is no CPU fallback)")
    num_workers = min(len(os.sched_getaffinity(0)), 8) if args.num_workers is None else args.num_workers
    for p in args.path:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
        if p.endswith(".npz"):
            raise SystemExit(f"expression_compare_face_recon: {p}: {NPZ_REFUSED}")
    for p in args.path:          # both folders are labelled (:311-324): refuse names without numbers before any weights are loaded
        try:
            parse_labels_first(list_images_sorted(p))
        except ValueError as e:
            raise SystemExit(f"expression_compare_face_recon: {p}: {e}")
    state = load_recon_state(args.recon_ckpt)
    print("loading the model from %s" % args.recon_ckpt)
    scorer = ExprScorer(state, batch=args.batch_size, device=device)
    if args.gpu_jpeg_decode:          # one decoder behind both flags: every file goes by its signature
        from reface_amd.jpegdec import FileDecoder
        scorer.png_decoder = FileDecoder(device, png=args.gpu_png_decode, jpeg=True, jpeg_parallel=args.gpu_jpeg_parallel, png_parallel=args.gpu_png_parallel)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import PngDecoder
        scorer.png_decoder = PngDecoder(device, parallel=args.gpu_png_parallel)
    r = scorer.score_folders(args.path, num_workers=num_workers)
    print("Expression_value: ", r["expression_value"])
    if args.print_sim:
        print("Similarities: \n ")
        for i in range(len(r["distances"])):
            print(i, ":", r["distances"][i])
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"expression_value": r["expression_value"], "distances": [float(d) for d in r["distances"]], "labels": r["labels"],
                       "target_labels": r["target_labels"], "exp_target": r["exp_target"].tolist(), "exp_result": r["exp_result"].tolist(),
                       "images": r["images"], "images_per_s": r["images_per_s"], "seconds": r["seconds"]}, f)
    if args.gpu_jpeg_decode:          # (stderr: the printed lines stay what they are without the flags)
        for line in scorer.png_decoder.lines():
            print(line, file=sys.stderr)
    elif args.gpu_png_decode:
        from reface_amd.pngdec import counts_line
        print(counts_line(scorer.png_decoder), file=sys.stderr)
    return r


if __name__ == "__main__":
    main()
