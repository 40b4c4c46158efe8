"""The descriptor sweep behind tests/golden/gemm_plans.json: what rf_conv_gemm's planner (reface_amd/csrc/gemm_plan.h) answers -- return code, the 24 words
of rf_conv_gemm_plan3, the message of a rejection -- for the descriptor of every case of gemm_exact_refs.CASES and for a deterministic sample of a grid
over operand families, sizes, windows, activations and optional operands.

A plan query reads sizes and alignments only, so the grid's descriptors carry fake, suitably aligned pointer values; the cases' descriptors are the real
ones with every pointer replaced by such a value of the same alignment.  A descriptor travels as one text line `field=value ...` (zero fields left
out, floats as their bit patterns): that line is what tests/gemm_plan_host_main.cpp reads.

The table is a recording of the library BEFORE the planner moved into its header (tools/gen_golden.py gemm_plans, run against that build); a planner
that answers differently for one of these descriptors has changed a dispatch rule."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import struct

import torch

import gemm_exact_refs as R
from reface_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")
FIELDS = [(n, t) for n, t in _lib.ConvGemmDesc._fields_]
PTR_FIELDS = [n for n, t in FIELDS if t is C.c_void_p]
F32, BF16, FP8, X3, F16 = _lib.RF_F32, _lib.RF_BF16, _lib.RF_FP8_E4M3, _lib.RF_BF16X3, _lib.RF_F16
NONE, GEGLU, PRELU, ADD_RELU = _lib.ACT_NONE, _lib.ACT_GEGLU, _lib.ACT_PRELU, _lib.ACT_ADD_RELU
FAMILIES = ("bf16", "f16", "f32", "x3", "w8", "a8")
TILES = ((256, 320), (256, 256), (128, 320), (128, 256), (128, 160), (128, 128), (128, 64))
GRID_ROWS = 2400


def fake_ptr(field, low=0):
    """a non-null pointer value for `field`: 4 GiB apart per field, 64-byte aligned + `low`"""
    return ((PTR_FIELDS.index(field) + 1) << 32) | low


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def desc_values(d):
    """ConvGemmDesc -> {field: int} of its non-zero fields (floats as bit patterns)"""
    out = {}
    for n, t in FIELDS:
        v = getattr(d, n)
        v = _bits(v) if t is C.c_float else int(v or 0)
        if v:
            out[n] = v
    return out


def to_desc(vals):
    d = _lib.ConvGemmDesc()
    for n, t in FIELDS:
        v = vals.get(n, 0)
        setattr(d, n, struct.unpack("<f", struct.pack("<I", v))[0] if t is C.c_float else (v or None if t is C.c_void_p else v))
    return d


def line_of(vals):
    return " ".join(f"{n}={vals[n]}" for n, _ in FIELDS if n in vals)


# ------------------------------------------------------------------------------------------------ the cases' descriptors
@contextlib.contextmanager
def _sizes_only():
    """gemm_exact_refs.prepare without a GPU and without drawing operand values: a plan query reads neither"""
    saved = (ops._require_gpu, R._ints, R._x3_values, R._keep)
    ops._require_gpu = lambda *a: None
    R._ints = lambda g, shape, lo, hi, nonzero=True: torch.zeros(shape, dtype=torch.float64)
    R._x3_values = lambda g, shape, every: torch.zeros(shape, dtype=torch.float64)
    R._keep = lambda g, t, n, cover=False, **kw: t
    try:
        yield
    finally:
        ops._require_gpu, R._ints, R._x3_values, R._keep = saved


def _anonymous(d):
    vals = desc_values(d)
    for f in PTR_FIELDS:
        if f in vals:
            vals[f] = fake_ptr(f, vals[f] & 63)
    return vals


def case_descriptors():
    """[(name, values)]: every case as gemm_exact_refs.prepare builds it and, where it carries statistics, again as wire_stats leaves it (the slots
    are sized by the plan the loaded library reports, exactly as the GPU tests do)"""
    out = []
    with _sizes_only():
        for c in R.CASES:
            i = R.make_inputs(c)
            P = R.prepare(c, i, "cpu")
            out.append((c["id"], _anonymous(P["launch"].keep[0])))
            if c["gn"] or c["ln"]:
                R.wire_stats(c, P, ops.gemm_plan3(P["launch"]), "cpu", i)
                out.append((c["id"] + "+stats", _anonymous(P["launch"].keep[0])))
    return out


# ------------------------------------------------------------------------------------------------ the grid
class _Lcg:
    """a 64-bit linear congruential generator (Knuth's MMIX constants): the same draws on every Python"""

    def __init__(self, seed):
        self.s = seed & (2 ** 64 - 1)

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.s >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def chance(self, num, den):
        return self.below(den) < num


OUTS = {"bf16": (BF16, F32), "f16": (F16, F32), "f32": (F32, BF16), "x3": (F32,), "w8": (BF16, F32), "a8": (BF16, BF16, FP8)}
IMAGES = {64: (1, 8, 8), 256: (1, 16, 16), 1000: (1, 25, 40), 1024: (1, 32, 32), 4096: (1, 64, 64), 16384: (1, 128, 128), 65536: (1, 256, 256),
          73728: (2, 192, 192)}          # M -> (samples, H, W); 1000 is the ragged one
NS = (32, 64, 160, 200, 256, 320, 640, 1024, 1280, 2048, 2560, 3840, 5120, 10240)          # (200: no multiple of 16)
KS_LINEAR = (64, 320, 640, 1280, 2560, 5120, 11520)
CS_CONV = (64, 128, 320, 640, 1280)          # 3x3: K = 576 ... 11520
WS_BYTES = 256 << 20


def grid_descriptor(g):
    """one draw: (name, values).  The core axes are drawn freely; each optional operand joins with a small probability, so that most descriptors are
    launchable and the rejections stay a minority."""
    fam = g.pick(FAMILIES)
    out = g.pick(OUTS[fam])
    M = g.pick(tuple(IMAGES))
    N = g.pick(NS)
    shape = g.pick(("linear", "linear", "conv0", "conv1", "conv2"))
    act = g.pick((NONE, NONE, NONE, GEGLU, GEGLU, ADD_RELU, PRELU))
    if out == FP8:
        act = GEGLU
    # five draws of six keep to what the family takes (the dispatcher's answers); the sixth keeps whatever was drawn (the descriptor checks' answers)
    strict = g.chance(5, 6)
    b16 = fam in ("bf16", "f16")
    if strict:
        if shape == "conv2" and not (b16 and out != F32):
            shape = "conv1"
        if shape == "conv1" and fam in ("x3", "w8", "a8"):
            shape = "conv0"
        if act == GEGLU and N % 64:
            N = {32: 64, 160: 320, 200: 256}[N]
    eo = 4 if out == F32 else (1 if out == FP8 else 2)
    B, H, W = IMAGES[M]
    v = dict(dtype={"bf16": BF16, "f16": F16, "f32": F32, "x3": X3, "w8": BF16, "a8": FP8}[fam], out_dtype=out, M=M, N=N, act=act, batch=1, alpha=_bits(1.0),
             src0=fake_ptr("src0"), W=fake_ptr("W"), out=fake_ptr("out"), KH=1, KW=1, stride=1)
    tags = [fam, {F32: "f32", BF16: "bf16", F16: "f16", FP8: "fp8"}[out], f"M{M}", f"N{N}", shape, f"act{act}"]
    ups2 = shape != "linear" and g.chance(1, 12) and (b16 or not strict)
    two = shape != "linear" and not ups2 and g.chance(1, 12) and (fam in ("bf16", "f16", "f32", "w8") or not strict)          # a second source
    a8k = strict and fam == "a8"          # (fp8 activations: channel runs in multiples of 128)
    if shape == "linear":
        K = C0 = g.pick(KS_LINEAR[2:] if a8k else KS_LINEAR)
        v.update(Hin=1, Win=M, Hout=1, Wout=M)
    elif ups2:
        C0 = g.pick(CS_CONV)
        K = 4 * C0
        v.update(M=4 * M, Hin=H, Win=W, Hout=2 * H, Wout=2 * W, KH=2, KW=2, pad_t=1, pad_l=1, ups=2, korder=g.below(2))
        tags.append("ups2")
    else:
        C0 = g.pick((128, 640, 1280) if a8k else CS_CONV)
        K = 9 * C0 * (2 if two else 1)
        v.update(Hin=H, Win=W, Hout=H, Wout=W, KH=3, KW=3, pad_t=1, pad_l=1, korder=int(shape[-1]))
        if two:
            v.update(src1=fake_ptr("src1"), C1=C0, ld1=C0)
            tags.append("two")
    v.update(K=K, C0=C0, ld0=2 * C0 if fam == "x3" else C0)
    nout = N // 2 if act == GEGLU else N
    v["ldo"] = nout
    if fam in ("w8", "a8"):
        v.update(w_dtype=FP8, wscale=fake_ptr("wscale"), ldw=(K + 127) // 128 * 128)
    if fam == "a8":
        v.update(ascale=fake_ptr("ascale"), as_ld=(C0 // 32 + 3) // 4 * 4)
    if out == FP8:
        v.update(oscale=fake_ptr("oscale"), os_ld=N // 64)
    if act == PRELU:
        v["act_vec"] = fake_ptr("act_vec")
    if g.chance(3, 4):
        v["bias"] = fake_ptr("bias")
    if g.chance(1, 2):
        v.update(workspace=fake_ptr("workspace"), workspace_bytes=WS_BYTES)
        tags.append("ws")
    plain = not (strict and ups2)          # (the folded upsampling takes none of the optional operands)
    if (act == ADD_RELU or g.chance(1, 4)) and plain and not (strict and out == FP8):
        v.update(residual=fake_ptr("residual"), ldr=nout)
        tags.append("res")
    if g.chance(1, 8) and plain and not (strict and act == GEGLU):
        v.update(rowvec=fake_ptr("rowvec"), ldv=N, rows_per_sample=g.pick((M // B, max(M // 4, 1), 4096)))
        tags.append("rowvec")
    ln_able = b16 and shape == "linear" and out != F32 and act != ADD_RELU
    if g.chance(1, 2 if ln_able else 10) and (ln_able or not strict):
        role = g.pick(("prod128", "prod160", "cons"))
        if role == "cons":
            v.update(ln_stats_in=fake_ptr("ln_stats_in"), ln_in_parts=max(K // 64, 1), ln_in_cols=64, ln_eps=_bits(1e-5), ln_u=fake_ptr("ln_u"))
            if strict and g.chance(7, 8):
                v.pop("residual", None), v.pop("ldr", None)
        else:
            v.update(ln_stats_out=fake_ptr("ln_stats_out"), ln_out_parts=max(N // int(role[4:]), 1))
        tags.append(role)
    lone = "ln_stats_in" not in v and "ln_stats_out" not in v
    if g.chance(1, 12) and ((shape == "linear" and fam in ("bf16", "f16", "f32")) or not strict):
        v.update(w_sample_stride=N * K, rows_per_sample=g.pick((M // 2, 4096, 32)))
        tags.append("wps")
    if shape != "linear" and not ups2 and not two and g.chance(1, 8) and (b16 or not strict):
        Cx = g.pick((64, 320, 640))
        v.update(srcx=fake_ptr("srcx"), Cx=Cx, ldx=Cx, K=K + Cx)
        if "ldw" in v:
            v["ldw"] = (K + Cx + 127) // 128 * 128
        tags.append(f"srcx{Cx}")
    if shape == "linear" and g.chance(1, 10) and ((fam in ("bf16", "f16", "f32") and lone and "w_sample_stride" not in v) or not strict):
        nb = g.pick((2, 8))
        v.update(batch=nb, sA=M * K, sW=N * K, sO=M * nout, sR=M * nout)
        tags.append(f"batch{nb}")
    if g.chance(1, 40):          # a misaligned output: no vector epilogue
        v["out"] = fake_ptr("out", eo * 2)
        tags.append("out+2")
    return "-".join(tags), {k: x for k, x in v.items() if x}


def grid_descriptors():
    g = _Lcg(20240607)
    rows, seen = [], set()
    while len(rows) < GRID_ROWS:
        name, vals = grid_descriptor(g)
        line = line_of(vals)
        if line not in seen:
            seen.add(line)
            rows.append((f"grid{len(rows)}-{name}", vals))
    return rows


def descriptors():
    return case_descriptors() + grid_descriptors()


# ------------------------------------------------------------------------------------------------ asking a library, recording, reading the table
def ask(lib, vals):
    """(return code, the 24 words, message of a rejection) of rf_conv_gemm_plan3"""
    info = (C.c_int32 * 24)()
    d = to_desc(vals)
    rc = lib.rf_conv_gemm_plan3(C.byref(d), info)
    return rc, [int(x) for x in info], (lib.rf_last_error().decode() if rc else "")


def sweep_digest(rows):
    return hashlib.sha256("\n".join(line_of(v) for _, v in rows).encode()).hexdigest()


def record(recorded_from):
    """write tests/golden/gemm_plans.json from the LOADED library (REFACE_HIP_LIB selects the build): the digest of the descriptor lines, the distinct
    answers [rc, message index or -1, then the 24 words unless all are zero] and, per descriptor in sweep order, the index of its answer."""
    lib = _lib.load()
    rows = descriptors()
    msgs, answers, out = [], [], []
    for _, vals in rows:
        rc, words, msg = ask(lib, vals)
        if msg and msg not in msgs:
            msgs.append(msg)
        a = [rc, msgs.index(msg) if msg else -1] + (words if any(words) else [])
        if a not in answers:
            answers.append(a)
        out.append(answers.index(a))
    with open(GOLDEN, "w") as f:
        json.dump(dict(recorded_from=recorded_from, sweep_sha256=sweep_digest(rows), messages=msgs, answers=answers, rows=out), f, separators=(",", ":"))
        f.write("\n")
    return len(rows), len(msgs), os.path.getsize(GOLDEN)


def golden():
    """[(rc, words, message)] of the recorded table, one per descriptor, plus its header"""
    with open(GOLDEN) as f:
        t = json.load(f)
    rows = [(r[0], r[2:] or [0] * 24, t["messages"][r[1]] if r[1] >= 0 else "") for r in (t["answers"][k] for k in t["rows"])]
    return t, rows
