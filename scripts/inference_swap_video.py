#!/usr/bin/env python3
"""Video face-swap CLI on the MI355X-native engines: ONE source face onto every frame crop of a target video -- the sampling stage
of the reference's scripts/inference_swap_video.py:504-700.

The reference script has three stages.  Stage 1 (:430-500) decodes ``--target_video`` with OpenCV, aligns / crops every frame and the
``--src_image`` (dlib / FFHQ alignment, keeping the inverse transforms) and writes face-parsing label maps (BiSeNet); stage 3
(:690-760) warps every swapped crop back into its frame and encodes the mp4 with the original audio (moviepy).  Both are host-side
I/O around models that are outside this build, so this CLI takes stage 1's on-disk product, in the reference's
own layout (``--parse_masks`` writes the label maps below from the crops with the GPU face parser, reface_amd/parsing.py, when they are
missing):

  <Base_dir>/<video>cropped_face/<i>.png      aligned 1024^2 crops, one per frame           (:416, written at :489)
  <Base_dir>/<video>mask_frames/<i>.png       their face-parsing label maps                 (:417, :497)
  <outdir>/temp_results/<src>.png             the aligned source crop                       (:456-457)
  <outdir>/temp_results/<basename(src_image)> its label map                                 (:463)

Stage 2 is the test bench's batch body (reface_amd/pipeline.py) with the source repeated over the batch (:619-620) and
``drop_last=True`` (:541: a trailing partial batch of frames is NOT swapped -- kept, it is the reference's behaviour); every
swapped crop is written as the reference does before pasting, resized to 1024^2 (bilinear), to
``<outdir>/model_outputs/<frame id>.png`` (:690-691).

Stage 3's paste-back runs with ``--paste_back`` (reface_amd/pasteback.py, :705-724): every swapped crop is enlarged to 1024^2 and warped into
its full frame on the GPU with the reference's PIL arithmetic, byte for byte, and written as ``<outdir>/results/<frame id>.png`` (RGBA) by
an encoder pool.  It reads two more products of stage 1, checked before anything is loaded:

  <Base_dir>/<video>/<int(frame id)>.png      the full frames                               (:413, written at :475)
  <Base_dir>/<video>_inv_transforms.npy       per frame, the 8 PERSPECTIVE coefficients     (:496)

Stage 1's alignment runs with ``--align`` (reface_amd/align.py, src/utils/alignmengt.py of the reference): from 68 landmarks per frame, the
FFHQ quad, PIL's LANCZOS shrink and QUAD / BILINEAR resampling on the GPU, byte for byte, before any model loads.  It reads the full frames
``<Base_dir>/<video>/<i>.png`` (i = 0 .. N-1; there is no video decoder in this build, so the frames arrive as PNGs) and ``--src_image``,
and writes ``<Base_dir>/<video>cropped_face/<i>.png``, ``<Base_dir>/<video>_inv_transforms.npy`` and ``<outdir>/temp_results/<src>.png``.
Landmarks come from ``--landmarks FILE.npy`` ([N, 68, 2]) and ``--src_landmarks FILE.npy`` ([68, 2]), or from dlib where it is installed
(landmark detection is not built).  A frame whose landmarks are not finite ("no face") repeats the previous frame's crop and transform, as
the reference's ``except`` branch does.  ``--align --parse_masks --paste_back`` together run raw frames to pasted frames in one command.

``--stream`` does the work of ``--align --parse_masks --paste_back`` as one device-resident chain (reface_amd/stream.py): every frame is decoded
once (by the loader's workers), uploaded once, aligned, parsed, turned into the model's input tensors (rf_video_prep_u8: the dataset's
``__getitem__`` on the GPU, bit for bit), swapped and pasted without leaving the device, and encoded once (``results/<id>.png``) off the launch
thread.  It reads what the three flags read and writes ``results/``, ``<video>_inv_transforms.npy`` and the source's two files under
``temp_results/`` -- the same bytes as the staged route -- but not ``<video>cropped_face/``, ``<video>mask_frames/`` or ``model_outputs/``;
``--stream_keep`` writes those three too, from the device bytes, for the frames that are swapped (the staged route also aligns and parses the
trailing frames that ``drop_last`` never swaps; the stream does not decode them).

``--write_video [PATH]`` (with ``--paste_back`` or ``--stream``) ends stage 3 in a playable file: every pasted frame is JPEG-encoded on the
GPU (reface_amd/mjpeg.py: libjpeg's baseline arithmetic, byte for byte) and appended in frame order to a Motion-JPEG AVI, by default
``<outdir>/<video>_swapped.avi`` at ``--video_fps`` 25.  There is no audio track: the frames arrive as PNGs, so there is nothing to demux.
The reference's H.264 mp4 + audio mux of stage 3 is not built (no video encoder in this build).

``--video_in FILE.avi`` (with ``--paste_back`` or ``--stream``) takes the full frames from a Motion-JPEG AVI file -- the kind ``--write_video``
writes -- instead of ``<Base_dir>/<video>/<i>.png``: frame i is the file's i-th frame, decoded on the GPU (reface_amd/jpegdec.py: exactly
PIL's array) as RGB; ``--landmarks`` index its frames (and are required: dlib reads image files), ``drop_last`` and the ids are unchanged,
and ``--write_video`` without ``--video_fps`` takes the input's rate.

``--paste_mask`` (with ``--paste_back`` or ``--stream``; not in the reference) pastes every swapped crop through a feathered mask instead of
replacing the whole oriented square around the face: alpha is 255 where the crop's face-parsing label map (``<video>mask_frames/<i>.png``,
or the stream's label maps on the device) has a label the model repaints (``remove_mask_tar_FFHQ``, or [2, 3, 5, 6, 7]), grown by
``--paste_dilate`` pixels of the 512^2 label map (default 8), softened by two box blurs of radius ``--paste_feather`` (default 8) that fall
to 0 towards the crop's border, and enlarged to 1024^2; the crop with that alpha is warped and ``alpha_composite``-d over the frame with
PIL's arithmetic, byte for byte (rf_paste_alpha_u8, rf_paste_back_alpha_u8).  Where the mask has no support the written frame is the input
frame bit for bit.  Only ``results/<id>.png`` and the video change; ``model_outputs/`` and every other file are what they are without the
flag.  The defaults are a design choice: no trained checkpoint was available, so the effect on image quality is not measured.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from reface_amd import config as rcfg  # noqa: E402
from reface_amd import output as O  # noqa: E402
from inference_test_bench import load_model_from_config  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--prompt", type=str, nargs="?", default="a photograph of an astronaut riding a horse")
    p.add_argument("--outdir", type=str, nargs="?", default="results_video/debug")
    p.add_argument("--Base_dir", type=str, nargs="?", default="results_video")
    p.add_argument("--skip_grid", action="store_true")
    p.add_argument("--skip_save", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50)
    step_rule = p.add_mutually_exclusive_group()          # one step rule per run: DDIM (default), --plms or --dpm_solver
    step_rule.add_argument("--plms", action="store_true")
    step_rule.add_argument("--dpm_solver", action="store_true", help="DPM-Solver++ multistep sampler (not in the reference): made for few steps, "
                           "e.g. --ddim_steps 20; --ddim_eta must be 0")
    p.add_argument("--laion400m", action="store_true")
    p.add_argument("--fixed_code", action="store_true", default=True)        # (sic: on by default in the video caller, :231-235)
    p.add_argument("--Start_from_target", action="store_true")
    p.add_argument("--only_target_crop", action="store_true", default=True)
    p.add_argument("--target_start_noise_t", type=int, default=1000)
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--n_iter", type=int, default=2)
    p.add_argument("--H", type=int, default=512)
    p.add_argument("--W", type=int, default=512)
    p.add_argument("--C", type=int, default=4)
    p.add_argument("--f", type=int, default=8)
    p.add_argument("--n_samples", type=int, default=10)
    p.add_argument("--n_rows", type=int, default=0)
    p.add_argument("--scale", type=float, default=5)
    p.add_argument("--target_video", type=str, default="examples/faceswap/Andy2.mp4")
    p.add_argument("--src_image", type=str, default="examples/faceswap/source.jpg")
    p.add_argument("--src_image_mask", type=str, default=None)
    p.add_argument("--from-file", type=str, default=None)
    p.add_argument("--config", type=str, default="configs/debug.yaml")
    p.add_argument("--ckpt", type=str, default="models/REFace/checkpoints/last.ckpt")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--rank", type=int, default=0)
    p.add_argument("--precision", type=str, choices=["full", "fullx3", "autocast", "bf16", "fp16", "fp8"], default="autocast")
    p.add_argument("--faceParser_name", default="default", type=str)
    p.add_argument("--faceParsing_ckpt", type=str, default="Other_dependencies/face_parsing/79999_iter.pth")
    p.add_argument("--segnext_config", default="", type=str)
    p.add_argument("--save_vis", action="store_true")
    p.add_argument("--seg12", default=True, action="store_true")
    # additions (not in the reference)
    p.add_argument("--dpm_order", type=int, choices=[1, 2, 3], default=2, help="--dpm_solver: order of the multistep rule")
    p.add_argument("--dpm_spacing", type=str, choices=["logsnr", "quad", "uniform"], default="logsnr", help="--dpm_solver: the timestep grid "
                   "(uniform in log-SNR, quadratic in t, or DDIM's own)")
    p.add_argument("--dump_tensors", type=str, default=None, help="directory for per-batch .npz dumps of the tensors fed to / produced by the engines (tests)")
    p.add_argument("--clip_vision_config", type=str, default=None, help="JSON dict overriding the CLIP ViT dims (tests)")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--parse_masks", action="store_true", help="write missing face-parsing label maps from the existing crops with the GPU "
                   "face parser (--faceParsing_ckpt, 'none' = seeded weights; --seg12) before sampling")
    p.add_argument("--paste_back", action="store_true", help="stage 3: paste every swapped crop back into its full frame on the GPU "
                   "(<Base_dir>/<video>/<i>.png, <Base_dir>/<video>_inv_transforms.npy) and write <outdir>/results/<id>.png (RGBA)")
    p.add_argument("--align", action="store_true", help="stage 1: align the full frames <Base_dir>/<video>/<i>.png and --src_image on the GPU from "
                   "their 68 landmarks; writes <video>cropped_face/, <video>_inv_transforms.npy and temp_results/<src>.png")
    p.add_argument("--landmarks", type=str, default=None, help="--align: .npy of the frames' landmarks [N, 68, 2] (non-finite row = no face); "
                   "without it they come from dlib")
    p.add_argument("--src_landmarks", type=str, default=None, help="--align: .npy of --src_image's landmarks [68, 2]; without it they come from dlib")
    p.add_argument("--align_padding", action="store_true", help="--align / --stream: crop_image's enable_padding for --src_image and the frames: "
                   "a face whose crop reaches over the frame's edge is reflect-padded, blurred towards the border and filled towards the median "
                   "on the GPU (the FFHQ recipe) instead of showing a black wedge; other crops keep their bytes.  Its effect on swap "
                   "quality is unmeasured")
    p.add_argument("--stream", action="store_true", help="raw frames to pasted frames as one device-resident chain: the work of --align --parse_masks "
                   "--paste_back with one PNG decode and one encode per frame and no intermediate files (reads what they read; writes results/, "
                   "<video>_inv_transforms.npy and temp_results/)")
    p.add_argument("--gpu_png_decode", action="store_true", help="--paste_back / --stream: decode the video's frames on the GPU "
                   "(reface_amd/pngdec.py) and hand them to the device chain as device tensors; the files written are the same")
    p.add_argument("--gpu_png_parallel", action="store_true", help="--gpu_png_decode: frames that --gpu_png did not write (extracted video frames) "
                   "are inflated by one wave per dynamic Huffman block (the blocks plan of reface_amd/pngdec.py) instead of one wave per frame; "
                   "the frames are the same")
    p.add_argument("--gpu_png", action="store_true", help="--paste_back / --stream: encode the pasted RGBA frames of results/ on the GPU "
                   "(reface_amd/pngenc.py): the same pixels, other file bytes (about zlib level 1 in size); crops, label maps and model_outputs "
                   "stay on the host writer")
    p.add_argument("--stream_keep", action="store_true", help="--stream: also write <video>cropped_face/, <video>mask_frames/ and model_outputs/ "
                   "of the swapped frames, from the device bytes, off the launch thread")
    p.add_argument("--write_video", type=str, nargs="?", const="", default=None, metavar="PATH", help="--paste_back / --stream: also JPEG-encode every "
                   "pasted frame on the GPU (reface_amd/mjpeg.py) and write them in frame order as a Motion-JPEG AVI (default PATH: "
                   "<outdir>/<video>_swapped.avi); no audio track")
    p.add_argument("--video_fps", type=float, default=25.0, help="--write_video: frames per second of the file.  The reference reads the rate from "
                   "the mp4 through cv2; here the frames arrive as PNGs and there is no container to read it from, so it is given (default 25)")
    p.add_argument("--video_in", type=str, default=None, metavar="FILE.avi", help="--paste_back / --stream: frame i is the i-th frame of this "
                   "Motion-JPEG AVI file (as --write_video writes them), decoded on the GPU (reface_amd/jpegdec.py) and used where "
                   "<Base_dir>/<video>/<i>.png is used otherwise; --landmarks index its frames.  With --write_video and no --video_fps the output "
                   "takes this file's rate")
    p.add_argument("--gpu_jpeg_parallel", action="store_true", help="--video_in: frames without restart markers (an MJPG file of another writer) "
                   "are decoded by one lane per sub-sequence of the scan (the self-synchronising plan of reface_amd/jpegdec.py) instead of one lane "
                   "per frame; the frames are the same")
    p.add_argument("--paste_mask", action="store_true", help="--paste_back / --stream: composite every swapped crop through a feathered alpha plane "
                   "made of its face-parsing label map (the labels the model repaints, remove_mask_tar_FFHQ) instead of replacing the whole "
                   "square around the face; where the mask has no support the frame's pixels stay bit for bit")
    p.add_argument("--paste_dilate", type=int, default=8, metavar="N", help="--paste_mask: grow the repainted region by N pixels of the 512^2 "
                   "label map before feathering, 0 .. 64 (default 8)")
    p.add_argument("--paste_feather", type=int, default=8, metavar="N", help="--paste_mask: radius of the two box blurs that soften the mask's "
                   "edge, in pixels of the label map, 0 .. 64 (default 8; 0 = a hard edge)")
    p.add_argument("--video_quality", type=int, default=90, help="--write_video: libjpeg quality, 1 .. 100 (default 90)")
    p.add_argument("--video_subsampling", type=str, choices=["420", "444"], default="420", help="--write_video: chroma subsampling (default 420)")
    return p


VIDEO_OPTIONS = ("write_video", "video_fps", "video_quality", "video_subsampling", "video_in", "gpu_jpeg_parallel", "gpu_png_parallel")
_READERS = {}


def video_reader(opt):
    """--video_in: the AviReader of the file, opened once per run (None without the flag).  Exits naming what is wrong with the file."""
    if not opt.video_in:
        return None
    if opt.video_in not in _READERS:
        from reface_amd.mjpeg import AviReader
        try:
            _READERS[opt.video_in] = AviReader(opt.video_in)
        except (OSError, ValueError) as e:
            raise SystemExit(f"inference_swap_video: --video_in: {e}")
    return _READERS[opt.video_in]


def video_source(opt, device):
    """--video_in: the file's frames as device tensors (reface_amd.stream.VideoFrames: AviReader + the device JPEG decoder), else None."""
    if not opt.video_in:
        return None
    from reface_amd.jpegdec import JpegDecoder
    from reface_amd.stream import VideoFrames
    return VideoFrames(video_reader(opt), JpegDecoder(device, parallel=opt.gpu_jpeg_parallel))


def prepared_paths(opt):
    """The reference's names for what its stage 1 leaves on disk (:408-418, :456-463)."""
    video = os.path.basename(opt.target_video).split(".")[0]
    src = os.path.basename(opt.src_image).split(".")[0]
    tmp = os.path.join(opt.outdir, "temp_results")
    return {"frames": os.path.join(opt.Base_dir, video + "cropped_face"), "masks": os.path.join(opt.Base_dir, video + "mask_frames"),
            "src": os.path.join(tmp, src + ".png"), "src_mask": os.path.join(tmp, os.path.basename(opt.src_image))}


def pasteback_paths(opt):
    """The reference's names for what stage 3 reads besides the crops: the full frames and their inverse transforms (:413, :496)."""
    from reface_amd.pasteback import stage3_paths
    return stage3_paths(opt.Base_dir, opt.target_video)


def check_pasteback_inputs(opt, pp):
    """Paths stage 3 needs that are missing: the frames directory and the .npy, then (when both exist) the frame of every crop that a
    drop_last run swaps and its row of inverse transforms."""
    sp = pasteback_paths(opt)
    reader = video_reader(opt)          # --video_in: the frames come from the file, not from <Base_dir>/<video>/
    missing = [sp["video_frames"]] if reader is None and not os.path.isdir(sp["video_frames"]) else []
    missing += [sp["inv_transforms"]] if not os.path.isfile(sp["inv_transforms"]) else []
    if missing or not os.path.isdir(pp["frames"]):
        return missing
    n = len(os.listdir(pp["frames"])) // max(1, opt.n_samples) * max(1, opt.n_samples)
    if reader is None:
        missing += [p for p in (os.path.join(sp["video_frames"], f"{i}.png") for i in range(n)) if not os.path.isfile(p)]
    elif len(reader) < n:
        missing.append(f"{opt.video_in} (frames 0..{n - 1}: the file holds {len(reader)})")
    from reface_amd.pasteback import load_inv_transforms
    if len(load_inv_transforms(sp["inv_transforms"])) < n:
        missing.append(f"{sp['inv_transforms']} (rows for frames 0..{n - 1})")
    return missing


def check_align_inputs(opt):
    """What --align reads, checked without touching the GPU: (frame paths, their landmarks [N, 68, 2], the source's landmarks [1, 68, 2]).
    Exits naming what is missing or malformed."""
    from reface_amd import align as A
    frames_dir = pasteback_paths(opt)["video_frames"]
    problems = []
    reader = video_reader(opt)
    if reader is not None:          # --video_in: frame i of the file stands where <frames_dir>/<i>.png stands
        n = len(reader)
        if n == 0:
            problems.append(f"{opt.video_in} (it holds no frame)")
        paths = [f"{opt.video_in}#{i}" for i in range(n)]
        if not opt.landmarks:
            problems.append("--landmarks (dlib reads image files; the frames of --video_in are not files)")
    else:
        n = len([f for f in os.listdir(frames_dir) if f.endswith(".png")]) if os.path.isdir(frames_dir) else 0
        if n == 0:
            problems.append(f"{frames_dir} (the full frames <i>.png, i = 0 .. N-1)")
        paths = [os.path.join(frames_dir, f"{i}.png") for i in range(n)]
        problems += [p for p in paths if not os.path.isfile(p)]
    if not os.path.isfile(opt.src_image):
        problems.append(f"{opt.src_image} (--src_image)")
    lm = src_lm = None
    if not problems:
        for what, files, arg in (("the frames (--landmarks)", paths, opt.landmarks), ("--src_image (--src_landmarks)", [opt.src_image], opt.src_landmarks)):
            try:
                got = A.landmarks_for(files, arg, what)
                A.fill_missing(got)
            except ValueError as e:
                problems.append(f"{what}: {e}")
                continue
            lm, src_lm = (got, src_lm) if files is paths else (lm, got)
    if problems:
        raise SystemExit(f"inference_swap_video: {'--stream' if getattr(opt, 'stream', False) else '--align'} needs the full frames, the source image and 68 landmarks for each; problems:\n  " +
                         "\n  ".join(problems[:8]) + (f"\n  ... and {len(problems) - 8} more" if len(problems) > 8 else ""))
    return paths, lm, src_lm


def run_align(opt, paths, lm, src_lm):
    """Stage 1's alignment on the GPU: the crops of every frame, their inverse transforms and the aligned source."""
    from reface_amd.align import align_to_disk
    pp = prepared_paths(opt)
    os.makedirs(pp["frames"], exist_ok=True)
    os.makedirs(os.path.dirname(pp["src"]), exist_ok=True)
    padded, src_padded = [], []
    pad = dict(pad_edges=True) if opt.align_padding else {}
    align_to_disk([opt.src_image], src_lm, [pp["src"]], **pad, **(dict(padded=src_padded) if pad else {}))
    if opt.video_in:          # the frames as device tensors, decoded when the aligner asks for them
        paths = video_source(opt, torch.device("cuda"))
    inv = align_to_disk(paths, lm, [os.path.join(pp["frames"], f"{i}.png") for i in range(len(paths))], batch=max(1, opt.n_samples), **pad,
                        **(dict(padded=padded) if pad else {}))
    np.save(pasteback_paths(opt)["inv_transforms"], inv)
    print(f"inference_swap_video: {len(paths)} frames aligned into {pp['frames']} ({int((~np.isfinite(lm).all(axis=(1, 2))).sum())} without a face "
          f"repeat the previous one); inverse transforms in {pasteback_paths(opt)['inv_transforms']}" + padding_clause(opt, len(padded), len(src_padded)))


def padding_clause(opt, n_frames, n_src):
    """--align_padding: how many crops went through crop_image's padding (nothing without the flag)."""
    if not opt.align_padding:
        return ""
    return f"; --align_padding padded the crops of {n_frames} frames at the frame's edge" + (" and the source crop" if n_src else "")


def load_model_and_sampler(opt, config):
    """The model of --config / --ckpt on the GPU in --precision, and its DDIM / PLMS sampler."""
    if opt.clip_vision_config:
        import json
        config.model.params.cond_stage_config["params"] = {"vision_config": json.loads(opt.clip_vision_config)}
    model = load_model_from_config(config, opt.ckpt)
    device = torch.device("cuda")
    if opt.precision in ("autocast", "bf16"):
        model.set_compute_dtype(torch.bfloat16, encoders=True)
    elif opt.precision == "fp16":                   # the bf16 mode's UNet kernels on fp16 storage / MFMA (same speed, ~17 dB closer to the exact-fp32 image);
        model.set_compute_dtype(torch.float16)      # the towers and the VAE encoder stay fp32: this mode is chosen for its distance to "full"
    elif opt.precision == "fp8":
        model.set_compute_dtype("fp8", encoders=True)
    elif opt.precision == "fullx3":                 # the fast form of "full": fp32 storage, split-bf16 GEMM operands (3 bf16 MFMA passes)
        model.set_compute_dtype("f32x3")
    if opt.plms:
        from ldm.models.diffusion.plms import PLMSSampler
        sampler = PLMSSampler(model)
    elif opt.dpm_solver:
        from ldm.models.diffusion.dpm_solver import DPMSolverSampler
        sampler = DPMSolverSampler(model, order=opt.dpm_order, spacing=opt.dpm_spacing)
    else:
        sampler = DDIMSampler(model)
    return model, sampler, device


def run_stream(opt):
    """--stream: frames -> pasted frames with every intermediate on the device (reface_amd/stream.py)."""
    from reface_amd.data import load_source_reference, raw_collate
    from reface_amd.stream import FrameDataset, VideoStream, frame_items_collate, stream_paths
    paths, lm, src_lm = check_align_inputs(opt)
    config = rcfg.load(opt.config)
    test_args = dict(config.data.params.test.params)
    remove = test_args["remove_mask_tar_FFHQ"] if test_args["gray_outer_mask"] else [2, 3, 5, 6, 7]
    vs = VideoStream(lm, remove, seg_ckpt=opt.faceParsing_ckpt, seg12=opt.seg12, paste_mask=make_paste_mask(opt, test_args),
                     **(dict(pad_edges=True) if opt.align_padding else {}))          # host fp64 only: quads and inverse transforms of EVERY frame
    pp, sp = prepared_paths(opt), pasteback_paths(opt)
    np.save(sp["inv_transforms"], vs.inv_transforms)
    torch.manual_seed(opt.seed)
    np.random.seed(opt.seed)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    # the ONE source image stays on the staged code: its crop and label map as files, read back by load_source_reference
    from reface_amd.align import align_to_disk
    from reface_amd.parsing import FaceParser, parse_label_maps
    os.makedirs(os.path.dirname(pp["src"]), exist_ok=True)
    src_padded = []
    align_to_disk([opt.src_image], src_lm, [pp["src"]], **(dict(pad_edges=True, padded=src_padded) if opt.align_padding else {}))
    vs.parser = FaceParser(opt.faceParsing_ckpt)
    parse_label_maps([(pp["src"], pp["src_mask"])], opt.faceParsing_ckpt, seg12=opt.seg12, parser=vs.parser)
    model, sampler, device = load_model_and_sampler(opt, config)
    from reface_amd.pasteback import PngWriter
    from reface_amd.pipeline import SwapRunner
    runner = SwapRunner(model, sampler, opt)
    results = os.path.join(opt.outdir, "results")
    os.makedirs(results, exist_ok=True)
    keep = stream_paths(opt.Base_dir, opt.target_video, opt.outdir) if opt.stream_keep and not opt.skip_save else None
    for d in (keep or {}).values():
        os.makedirs(d, exist_ok=True)
    ref1 = load_source_reference(pp["src"], pp["src_mask"], test_args["preserve_mask_src_FFHQ"]).to(device)
    ns = max(1, opt.n_samples)
    source = video_source(opt, device)
    if source is not None:          # --video_in: the workers read the frames' JPEG bytes out of the AVI file
        from reface_amd.stream import AviFrameDataset
        ds = AviFrameDataset(opt.video_in, len(paths) // ns * ns)
    else:
        ds = FrameDataset(sp["video_frames"], len(paths) // ns * ns, raw=opt.gpu_png_decode)          # drop_last: the trailing partial batch is never swapped, so never decoded
    loader = torch.utils.data.DataLoader(ds, batch_size=ns, num_workers=opt.num_workers, pin_memory=True, shuffle=False, drop_last=True,
                                         collate_fn=frame_items_collate if opt.gpu_png_decode or source is not None else raw_collate)
    decoder = source.decoder if source is not None else make_png_decoder(opt, device)
    start_code = None
    if opt.fixed_code:
        start_code = torch.randn([opt.C, opt.H // opt.f, opt.W // opt.f], device=device).unsqueeze(0).repeat(opt.n_samples, 1, 1, 1)
    writer = None if opt.skip_save else PngWriter(png_encoder=make_png_encoder(opt, device))
    video = make_video(opt, device)
    n_done = 0
    held = []          # --gpu_png: the previous batch's enqueued encodes, handed to the writer only after this batch has been enqueued
    with torch.no_grad(), model.ema_scope():
        for frames, ids in loader:          # (the iterator draws its base seed from the CPU generator, as the staged loader's does)
            if decoder is not None:          # the workers read bytes: the frames are decoded here, on the device
                job = decoder.decode_async(*((source.items(ids, frames), "RGB") if source is not None else (frames,)))
                frames = job.result()
                frames = job.batch if job.batch is not None else frames
            test_batch, kw, state = vs.prepare(frames, ids)
            if opt.Start_from_target:
                start_code = runner.start_from_target(test_batch)
            B = test_batch.shape[0]
            x_img, _ = runner.run_batch(test_batch, kw, ref1.repeat(B, 1, 1, 1), start_code=start_code)
            pasted, swapped = vs.paste(x_img, state)
            n_done += B
            if writer is None:
                continue
            if video is not None:          # (holds one batch back itself, as hand_over does for the PNG encodes)
                video.push(pasted)
            if opt.gpu_png:
                held = hand_over(writer, held, [([os.path.join(results, ids[i] + ".png") for i in idx], job) for idx, job in writer.encode_device(pasted)])
            else:
                for sid, frame in zip(ids, pasted):
                    writer.submit(os.path.join(results, sid + ".png"), frame.cpu().numpy())
            if keep:
                for sid, i, crop, lab, mo in zip(ids, state["index"], state["crops"].cpu().numpy(), state["labels"].cpu().numpy(), swapped.cpu().numpy()):
                    writer.submit(os.path.join(keep["crops"], f"{i}.png"), crop)
                    writer.submit(os.path.join(keep["masks"], f"{i}.png"), lab)
                    writer.submit(os.path.join(keep["model_outputs"], sid + ".png"), mo)
    if writer is not None:
        hand_over(writer, held, [])
    torch.cuda.synchronize()
    n_files = writer.close() if writer is not None else 0
    video_files = video.close() if video is not None else None
    n_pasted = n_files // 4 if keep else n_files
    if decoder is not None:
        print("inference_swap_video --" + decoder_line(opt, decoder))
    left = len(paths) - n_done
    print(f"inference_swap_video --stream: {n_done} of {len(paths)} frames swapped and pasted on the device"
          + (f" ({left} trailing frames are not swapped: drop_last)" if left else "") + f"; {n_pasted} pasted frames written to {results}, inverse "
          f"transforms of all {len(paths)} frames to {sp['inv_transforms']}; "
          + (f"crops, label maps and swapped crops of the swapped frames kept in {', '.join(keep.values())}" if keep else
             "no crops, label maps or model_outputs files were written (--stream_keep writes them)")
          + padding_clause(opt, len(vs.padded), len(src_padded)) + mask_clause(opt) + (video_clause(opt, video_files) if video is not None else " (the mp4 + audio mux of the reference's stage 3 is not built)."))
    return n_done


def make_paste_mask(opt, test_args):
    """--paste_mask: the PasteMask of the labels the dataset's keep-mask cuts out of the target (None without the flag)."""
    if not opt.paste_mask:
        return None
    from reface_amd.pasteback import PasteMask
    remove = test_args["remove_mask_tar_FFHQ"] if test_args["gray_outer_mask"] else [2, 3, 5, 6, 7]
    return PasteMask(remove, dilate=opt.paste_dilate, feather=opt.paste_feather)


def mask_clause(opt):
    """The closing line's account of --paste_mask."""
    return (f"; pasted through the feathered mask of the repainted labels (--paste_mask: dilate {opt.paste_dilate}, feather {opt.paste_feather}, "
            "2 passes, at the label map's size)") if opt.paste_mask else ""


def make_png_decoder(opt, device):
    """--gpu_png_decode: the device PNG decoder the video's frames come through (None: PIL in the loader)."""
    if not opt.gpu_png_decode:
        return None
    from reface_amd.pngdec import PngDecoder
    return PngDecoder(device, parallel=opt.gpu_png_parallel)


def decoder_line(opt, decoder):
    """The line that says where the frames were decoded (--gpu_png_decode's, or --video_in's)."""
    if opt.video_in:
        from reface_amd.jpegdec import counts_line
    else:
        from reface_amd.pngdec import counts_line
    return counts_line(decoder, "frames")


def make_png_encoder(opt, device):
    """--gpu_png: the device PNG encoder the pasted frames go through (None: the host writer)."""
    if not opt.gpu_png:
        return None
    from reface_amd.pngenc import PngEncoder
    return PngEncoder(device)


def make_video(opt, device):
    """--write_video: the device JPEG encoder, ordered sink and AVI writer the pasted frames also go through (None: no video)."""
    if opt.write_video is None or opt.skip_save:
        return None
    from reface_amd.mjpeg import VideoOutput
    path = opt.write_video or os.path.join(opt.outdir, os.path.basename(opt.target_video).split(".")[0] + "_swapped.avi")
    return VideoOutput(path, opt.video_fps, opt.video_quality, opt.video_subsampling, device)


def video_clause(opt, files):
    """The closing line's account of the video: the files, their frame counts and what kind of file they are."""
    names = ", ".join(f"{p} ({n} frames)" for p, n in files) or "no file (no frame was pasted)"
    return (f"; video of {sum(n for _, n in files)} frames written to {names}: Motion-JPEG AVI, {opt.video_fps:g} fps, quality {opt.video_quality}, "
            f"{opt.video_subsampling[0]}:{opt.video_subsampling[1]}:{opt.video_subsampling[2]}, no audio track.")


def hand_over(writer, held, jobs):
    """The encodes enqueued one batch ago go to the writer threads now that the next batch is behind them in the stream; returns what to hold."""
    for paths, job in held:
        writer.submit_device(paths, job)
    return jobs


def main(argv=None):
    opt = build_parser().parse_args(argv)
    print(argparse.Namespace(**{k: v for k, v in vars(opt).items() if k not in VIDEO_OPTIONS and (k != "align_padding" or v)}))          # (the closing line states the video's settings)
    if opt.align_padding and not (opt.align or opt.stream or opt.stream_keep):
        raise SystemExit("inference_swap_video: --align_padding pads the crops that --align or --stream make at the frame's edge; without either no "
                         "frame is aligned (the crops of target_frames/ are read as they are)")
    if opt.gpu_png and not (opt.paste_back or opt.stream or opt.stream_keep):
        raise SystemExit("inference_swap_video: --gpu_png encodes the pasted frames of results/ and needs --paste_back or --stream "
                         "(model_outputs/ stays on the host writer)")
    if opt.gpu_png_decode and not (opt.paste_back or opt.stream or opt.stream_keep):
        raise SystemExit("inference_swap_video: --gpu_png_decode decodes the video's frames for --paste_back or --stream; without either no frame "
                         "is read (the crops of target_frames/ go through the dataset's host transforms)")
    if opt.gpu_png_parallel and not opt.gpu_png_decode:
        raise SystemExit("inference_swap_video: --gpu_png_parallel chooses a plan of the GPU PNG decoder and needs --gpu_png_decode; without it no PNG "
                         "frame is decoded on the GPU")
    if opt.gpu_png and opt.skip_save:
        print("inference_swap_video: --skip_save writes no files, so --gpu_png has nothing to encode")
    if opt.paste_mask and not (opt.paste_back or opt.stream or opt.stream_keep):
        raise SystemExit("inference_swap_video: --paste_mask composites the pasted frames of results/ through the crops' label maps and needs "
                         "--paste_back or --stream (model_outputs/ holds crops, not frames)")
    for flag, value in (("--paste_dilate", opt.paste_dilate), ("--paste_feather", opt.paste_feather)):
        if not opt.paste_mask and any(a == flag or a.startswith(flag + "=") for a in (sys.argv[1:] if argv is None else argv)):
            raise SystemExit(f"inference_swap_video: {flag} shapes the mask of --paste_mask and needs it; without it every pixel of the quad is replaced")
        if not 0 <= value <= 64:
            raise SystemExit(f"inference_swap_video: {flag} is 0 .. 64 pixels of the label map, got {value}")
    if opt.gpu_jpeg_parallel and not opt.video_in:
        raise SystemExit("inference_swap_video: --gpu_jpeg_parallel chooses a plan of the GPU JPEG decoder and needs --video_in; without it no JPEG "
                         "frame is decoded")
    if opt.video_in:
        if not (opt.paste_back or opt.stream or opt.stream_keep):
            raise SystemExit("inference_swap_video: --video_in supplies the video's full frames for --paste_back or --stream; without either no frame "
                             "is read (the crops of target_frames/ go through the dataset's host transforms)")
        if opt.gpu_png_decode:
            raise SystemExit("inference_swap_video: the frames of --video_in are JPEG and are decoded on the GPU already; --gpu_png_decode has no PNG "
                             "frame to decode")
        reader = video_reader(opt)
        if opt.write_video is not None and not any(a == "--video_fps" or a.startswith("--video_fps=") for a in (sys.argv[1:] if argv is None else argv)):
            opt.video_fps = reader.fps          # the output takes the input's rate
    if opt.write_video is not None:
        if not (opt.paste_back or opt.stream or opt.stream_keep):
            raise SystemExit("inference_swap_video: --write_video encodes the pasted frames of results/ into a video and needs --paste_back or --stream "
                             "(model_outputs/ holds crops, not frames)")
        if not 1 <= opt.video_quality <= 100:
            raise SystemExit(f"inference_swap_video: --video_quality is libjpeg's 1 .. 100, got {opt.video_quality}")
        if not opt.video_fps > 0:
            raise SystemExit(f"inference_swap_video: --video_fps must be positive, got {opt.video_fps}")
        if opt.skip_save:
            print("inference_swap_video: --skip_save writes no files, so --write_video has nothing to encode")
    if opt.stream or opt.stream_keep:
        opt.stream = True
        return run_stream(opt)
    aligned = check_align_inputs(opt) if opt.align else None
    if aligned is not None:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        run_align(opt, *aligned)
    if opt.paste_back:
        missing = check_pasteback_inputs(opt, prepared_paths(opt))
        if missing:
            raise SystemExit("inference_swap_video: --paste_back needs the full frames and the inverse alignment transforms that stage 1 of the "
                             "reference writes (inference_swap_video.py:475, :496); missing:\n  " + "\n  ".join(missing[:8]) +
                             (f"\n  ... and {len(missing) - 8} more" if len(missing) > 8 else ""))
    torch.manual_seed(opt.seed)
    np.random.seed(opt.seed)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    pp = prepared_paths(opt)
    if opt.parse_masks:             # stage 1's parsing half on the GPU: label maps of the frame crops / source crop that lack them
        from reface_amd.parsing import parse_label_maps
        jobs = []
        if os.path.isdir(pp["frames"]) and os.listdir(pp["frames"]) and not (os.path.isdir(pp["masks"]) and os.listdir(pp["masks"])):
            jobs += [(os.path.join(pp["frames"], f), os.path.join(pp["masks"], f)) for f in sorted(os.listdir(pp["frames"]))]
        if os.path.isfile(pp["src"]) and not os.path.isfile(pp["src_mask"]):
            jobs.append((pp["src"], pp["src_mask"]))
        print(f"inference_swap_video: {parse_label_maps(jobs, opt.faceParsing_ckpt, seg12=opt.seg12)} label maps written by the face parser")
    missing = [pp[k] for k in ("frames", "masks") if not os.path.isdir(pp[k]) or not os.listdir(pp[k])]
    missing += [pp[k] for k in ("src", "src_mask") if not os.path.isfile(pp[k])]
    if missing:
        raise SystemExit("inference_swap_video: stage 1 of the reference (frame extraction, face alignment and BiSeNet parsing of --target_video / "
                         "--src_image, inference_swap_video.py:430-500) is outside this build's scope; prepare\n  " + "\n  ".join(missing) +
                         "\n(the reference's stage 1 writes exactly these paths).")
    config = rcfg.load(opt.config)
    model, sampler, device = load_model_and_sampler(opt, config)
    from PIL import Image
    from reface_amd.data import VideoDataset, load_source_reference
    from reface_amd.pipeline import SwapRunner
    runner = SwapRunner(model, sampler, opt)
    model_out = os.path.join(opt.outdir, "model_outputs")
    os.makedirs(model_out, exist_ok=True)
    os.makedirs(os.path.join(opt.outdir, "results"), exist_ok=True)      # stage 3 fills it (pasted frames: --paste_back)
    test_args = dict(config.data.params.test.params)
    ref1 = load_source_reference(pp["src"], pp["src_mask"], test_args["preserve_mask_src_FFHQ"]).to(device)
    ds = VideoDataset(data_path=pp["frames"], mask_path=pp["masks"], **test_args)
    loader = torch.utils.data.DataLoader(ds, batch_size=opt.n_samples, num_workers=opt.num_workers, pin_memory=True, shuffle=False, drop_last=True)
    start_code = None
    if opt.fixed_code:      # ONE latent, repeated over the batch (:549-552) -- not one per sample as in the selected-swap caller
        start_code = torch.randn([opt.C, opt.H // opt.f, opt.W // opt.f], device=device).unsqueeze(0).repeat(opt.n_samples, 1, 1, 1)
    n_done = 0
    paster = writer = None
    if opt.paste_back and not opt.skip_save:
        from reface_amd.pasteback import PasteBack, PngWriter
        sp = pasteback_paths(opt)
        paster = PasteBack(sp["video_frames"], sp["inv_transforms"], mask=make_paste_mask(opt, test_args), masks_dir=pp["masks"])
        writer = PngWriter(png_encoder=make_png_encoder(opt, device))
    video = make_video(opt, device) if paster is not None else None
    source = video_source(opt, device) if paster is not None else None
    decoder = (source.decoder if source is not None else make_png_decoder(opt, device)) if paster is not None else None

    def device_frames(ids):
        if source is not None:
            return source.batch(ids)
        from reface_amd.pasteback import load_frames_device
        return load_frames_device(decoder, sp["video_frames"], ids)
    held = []
    with torch.no_grad(), model.ema_scope():
        for test_batch, prior, kw, ids in loader:
            frames = paster.prefetch(ids) if paster is not None and decoder is None else None          # decoded on the pool while the batch samples
            if opt.Start_from_target:
                start_code = runner.start_from_target(test_batch)        # `use_prior = False` (:555)
            kw = {n: kw[n].to(device, non_blocking=True) for n in kw}
            B = test_batch.shape[0]
            x_img, _ = runner.run_batch(test_batch, kw, ref1.repeat(B, 1, 1, 1), start_code=start_code)
            n_done += B
            if opt.skip_save:
                continue
            res = x_img.cpu().numpy()
            for i, sid in enumerate(ids):
                Image.fromarray(O.to_u8_hwc(res[i])).resize((1024, 1024), Image.BILINEAR).save(os.path.join(model_out, sid + ".png"))
            if paster is not None and decoder is not None and not opt.gpu_png:          # frames decoded and pasted on the device, encoded on the host
                pasted = paster.paste_device(x_img, ids, device_frames(ids))
                for sid, frame in zip(ids, pasted):
                    writer.submit(os.path.join(opt.outdir, "results", sid + ".png"), frame.cpu().numpy())
                if video is not None:
                    video.push(pasted)
            elif paster is not None and opt.gpu_png:          # the pasted frames stay on the device and are encoded there
                if decoder is not None:
                    dev_frames = device_frames(ids)
                else:
                    dev_frames = [torch.from_numpy(np.array(f.result(), copy=True)).to(device) for f in frames]
                pasted = paster.paste_device(x_img, ids, dev_frames)
                held = hand_over(writer, held, [([os.path.join(opt.outdir, "results", ids[i] + ".png") for i in idx], job)
                                                for idx, job in writer.encode_device(pasted)])
                if video is not None:
                    video.push(pasted)
            elif paster is not None:          # stage 3 (:705-724): the crops enlarged and warped into their frames on the device, PNGs encoded off this thread
                pasted = paster.paste(x_img, ids, frames)
                for sid, frame in zip(ids, pasted):
                    writer.submit(os.path.join(opt.outdir, "results", sid + ".png"), frame)
                if video is not None:          # the host-pasted frames go up once more, for the encoder
                    video.push([torch.from_numpy(f).to(device) for f in pasted])
    if writer is not None:
        hand_over(writer, held, [])
    torch.cuda.synchronize()
    if paster is not None:
        paster.close()
        n_pasted = writer.close()
        video_files = video.close() if video is not None else None
        if decoder is not None:
            print("inference_swap_video --" + decoder_line(opt, decoder))
        print(f"Swapped crops of {n_done} frames are in {model_out}; {n_pasted} pasted frames are in {os.path.join(opt.outdir, 'results')}"
              + mask_clause(opt) + (video_clause(opt, video_files) if video is not None else " (the mp4 + audio mux of the reference's stage 3 is not built)."))
    else:
        print(f"Swapped crops of {n_done} frames are in {model_out}; the reference's stage 3 (paste back with the inverse alignment of every frame, "
              f"mp4 + audio) takes them from there (--paste_back pastes them back on the GPU).")
    return n_done


if __name__ == "__main__":
    main()
