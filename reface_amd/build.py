"""Build the gfx950 shared library  reface_amd/lib/libreface_hip.so  with hipcc (in-tree).

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so
travels to the GPU box with the repo snapshot.
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libreface_hip.so")
SOURCES = ["gemm.hip", "gemm_f16.hip", "norm.hip", "attention.hip", "elementwise.hip", "encoder.hip", "ffn.hip", "smallconv.hip", "attnin.hip", "parsing.hip", "pasteback.hip", "align.hip", "align_pad.hip", "video_prep.hip", "idscore.hip", "pose.hip", "expr.hip", "fid.hip", "lpips.hip", "pngenc.hip", "pngdec.hip", "jpegenc.hip", "jpegdec.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
# per-file extras.  attention: keep MFMA accumulators in VGPRs -- the online softmax reads every score and rescales O each
# tile, and with AGPR accumulators hipcc emitted ~160 v_accvgpr_read/write per KV tile (40 % of the loop's VALU work).
# -fno-honor-nans (round 6): the online-softmax max chains are fmaxf over MFMA results; under IEEE NaN semantics hipcc quiets every input first (v_max x, x) --
# 10 of the ~86 VALU instructions per 64 x 32 unit of the VALU-bound d = 40 kernel.  Scores are finite (masked keys are -inf, never NaN): -0.35 % per batch at 512x512,
# -0.6 % at 768x768, every attention test unchanged (profiles/r06e_attention_no_nan_quieting.txt).
EXTRA_FLAGS = {"attention.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"]}
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "check.h"), os.path.join(os.path.dirname(HERE), "include", "reface_hip.h")]
# further files a unit includes (part of its content key): gemm_f16.hip is gemm.hip's templates instantiated for fp16 operands
# gemm_plan.h: rf_conv_gemm's planner, host-only C++ that gemm.hip launches from and a host compiler builds into tests/gemm_plan_host_main.cpp
# pil_u8.h: PIL's sampler / clip / packed store shared by the units that reproduce PIL's bytes; cv_u8.h: cv2's u8 INTER_LINEAR taps likewise
UNIT_DEPS = {"gemm.hip": [os.path.join(CSRC, "gemm_plan.h")], "gemm_f16.hip": [os.path.join(CSRC, "gemm.hip"), os.path.join(CSRC, "gemm_plan.h")],
             "pasteback.hip": [os.path.join(CSRC, "pil_u8.h")], "align.hip": [os.path.join(CSRC, "pil_u8.h")],
             "video_prep.hip": [os.path.join(CSRC, "pil_u8.h")], "elementwise.hip": [os.path.join(CSRC, "cv_u8.h")],
             "idscore.hip": [os.path.join(CSRC, "cv_u8.h")], "expr.hip": [os.path.join(CSRC, "pil_u8.h")],
             "fid.hip": [os.path.join(CSRC, "pil_u8.h")],
             # png_inflate.h: the zlib decoder core, compiled by hipcc here and by a host compiler into tests/pngdec_host_main.cpp
             "pngdec.hip": [os.path.join(CSRC, "png_inflate.h"), os.path.join(CSRC, "png_blocks.h")],
             # jpeg_decode.h: the JPEG entropy-decoder core, compiled by hipcc here and by a host compiler into tests/jpegdec_host_main.cpp
             "jpegdec.hip": [os.path.join(CSRC, "jpeg_decode.h"), os.path.join(CSRC, "jpeg_sync.h")]}



def _digest(paths, extra):
    """sha256 over the bytes of `paths` (in order) and the strings in `extra`."""
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    for e in extra:
        h.update(e.encode())
        h.update(b"\0")
    return h.hexdigest()


_HIPCC_ID = {}


def _hipcc_id(hipcc):
    """Compiler version string (one `hipcc --version` per process), or None when there is no hipcc on this box."""
    if hipcc not in _HIPCC_ID:
        try:
            out = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
            _HIPCC_ID[hipcc] = " ".join(l.strip() for l in out.splitlines() if "version" in l.lower())          # (no install paths: the key must not depend on them)
        except OSError:
            _HIPCC_ID[hipcc] = None
    return _HIPCC_ID[hipcc]


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def unit_key(unit, hipcc=None):
    """Content key of one compile unit: sha256 of (source, headers, compile flags, compiler version).  Stored next to the object as
    `<unit>.o.key`; an object whose key file does not match is rebuilt -- file times play no part (a checkout or a snapshot copy
    sets them arbitrarily)."""
    hipcc = hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return _digest([], [source_key(unit), _hipcc_id(hipcc) or "unknown"])


def source_key(unit):
    """The compiler-independent part of a unit's key: sha256 of (source, headers, compile flags)."""
    return _digest([os.path.join(CSRC, unit)] + UNIT_DEPS.get(unit, []) + HEADERS, FLAGS + EXTRA_FLAGS.get(unit, []))


def build(force=False, verbose=True):
    """Compile what is out of date BY CONTENT and link.  Returns the library path; `build.last_report` lists, per unit, the key and whether
    it was compiled in this call (the round's "does it build" evidence)."""
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    force = force or os.environ.get("REFACE_BUILD_FORCE", "0") == "1"
    objs, procs, report = [], [], {}
    if _hipcc_id(hipcc) is None:
        # a box that received the prebuilt objects and library but has no compiler: accept them when every unit's SOURCE part (source, headers,
        # flags) still matches what the stored key was made from -- nothing can be rebuilt here anyway
        ok = os.path.exists(LIB) and all(_read(os.path.join(LIBDIR, s.replace(".hip", ".o.src"))) == source_key(s) for s in SOURCES)
        if not ok:
            raise RuntimeError(f"reface_amd.build: no hipcc at {hipcc} and the prebuilt library is missing or stale (sources changed since it was built)")
        if verbose:
            print("[build] no hipcc on this box: prebuilt library accepted (source keys match)", flush=True)
        build.last_report = {s: {"key": (_read(os.path.join(LIBDIR, s.replace(".hip", ".o.key"))) or "")[:16], "compiled": False} for s in SOURCES}
        return LIB
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        objs.append(obj)
        key = unit_key(s, hipcc)
        fresh = (not force) and os.path.exists(obj) and _read(obj + ".key") == key
        report[s] = {"key": key[:16], "compiled": not fresh}
        if not fresh:
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(s, []) + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            if os.path.exists(obj + ".key"):
                os.remove(obj + ".key")
            procs.append((s, obj, key, subprocess.Popen(cmd)))
        elif verbose:
            print(f"[build] {s}: up to date (content key {key[:16]})", flush=True)
    for s, obj, key, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
        with open(obj + ".key", "w") as f:
            f.write(key + "\n")
    for s in SOURCES:          # the compiler-independent part, kept beside every object (boxes without hipcc check it)
        srcf = os.path.join(LIBDIR, s.replace(".hip", ".o.src"))
        if _read(srcf) != source_key(s):
            with open(srcf, "w") as f:
                f.write(source_key(s) + "\n")
    # the library's key = the keys of its objects: relinked whenever one of them changed
    lib_key = _digest([], [report[s]["key"] for s in SOURCES])
    if force or procs or not os.path.exists(LIB) or _read(LIB + ".key") != lib_key:
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(LIB + ".key", "w") as f:
            f.write(lib_key + "\n")
        # hipcc's host pass can drop a kernel stub without a diagnostic (seen with a call expression inside a builtin's argument
        # list): the library then links but fails to load.  Catch it here.
        und = subprocess.run(["nm", "-u", "-C", LIB], capture_output=True, text=True).stdout
        bad = [l.strip() for l in und.splitlines() if "rf::" in l]
        if bad:
            os.remove(LIB)
            raise RuntimeError("libreface_hip.so has undefined rf:: symbols (host stubs missing): " + "; ".join(bad[:4]))
    build.last_report = report
    return LIB


if __name__ == "__main__":
    if "--print-flags" in sys.argv:          # tools/build_a16_variants.sh: the ONE source of the per-unit compile flags
        unit = sys.argv[sys.argv.index("--print-flags") + 1]
        print(" ".join(FLAGS + EXTRA_FLAGS.get(unit + ".hip", [])))
        sys.exit(0)
    build(force="--force" in sys.argv)
    print(LIB)
