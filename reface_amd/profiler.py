"""Per-launch timing with HIP events (on the stream the kernels are launched on) and the
algorithmic FLOP / byte accounting used for the roofline numbers of bench.py."""
import collections

import torch

from ._lib import ConvGemmDesc


GAP_CAP_MS = 0.0025


def launch_family(l):
    n = l.fn.__name__
    if n == "rf_conv_gemm":
        d = l.keep[0]
        if d.dtype == 2:
            return "rf_conv_gemm[fp8]"           # fp8 activations (E8M0 block scales) x fp8 weights on the MX-scaled fp8 MFMA
        if d.w_dtype == 2:
            return "rf_conv_gemm[fp8w]"          # fp8 (e4m3fn) weights x bf16 activations on the bf16 MFMA
        if d.dtype == 3:
            return "rf_conv_gemm[bf16x3]"        # split-bf16 operand pairs, three bf16 MFMA passes per product, fp32 accumulate / output
        if d.dtype == 4:
            return "rf_conv_gemm[f16]"           # fp16 operands on v_mfma_f32_32x32x16_f16 (the bf16 kernels' geometry and rate)
        return f"rf_conv_gemm[{'bf16' if d.dtype == 1 else 'f32'}]"
    if n == "rf_ffn_block":
        return "rf_ffn_geglu"          # (one family with the plain fused feed-forward: the same kernel)
    return n


def gemm_flops(l):
    """Algorithmic FLOPs of one rf_conv_gemm launch: 2*M*N*K_real (padding excluded); GEGLU N counts both halves."""
    if l.fn.__name__ != "rf_conv_gemm":
        return 0.0
    d = l.keep[0]
    k_real = d.KH * d.KW * (d.C0 + d.C1) + (d.Cx if d.srcx else 0)          # (+ the centre-tap tail source's channels)
    if d.dtype == 2:            # fp8 activations: C0 / K count the channel run PADDED to 128; the algorithmic count uses the real channels
        k_real = d.KH * d.KW * next((k.C for k in l.keep if type(k).__name__ == "Fp8Act"), d.C0)
    return 2.0 * d.M * d.N * min(k_real, d.K) * d.batch


def ffn_flops(l):
    """rf_ffn_geglu: 2*M*C*8C (GEGLU projection) + 2*M*4C*C (ff.net.2)."""
    if l.fn.__name__ == "rf_ffn_block":          # + proj_out (2*M*C*C) when fused behind the feed-forward
        d = l.keep[0]
        return 2.0 * d.M * d.C * 8 * d.C + 2.0 * d.M * 4 * d.C * d.C + (2.0 * d.M * d.C * d.C if d.wpo else 0.0) + (2.0 * d.M * d.C * d.C if d.wo else 0.0)
    if l.fn.__name__ != "rf_ffn_geglu":
        return 0.0
    M, C_ = l.args[10], l.args[11]
    return 2.0 * M * C_ * 8 * C_ + 2.0 * M * 4 * C_ * C_


def attn_in_flops(l):
    """rf_attn_in: proj_in (2*M*C*C) + the fused q / k / v projection (2*M*3C*C)."""
    if l.fn.__name__ != "rf_attn_in":
        return 0.0
    d = l.keep[0]
    return 2.0 * d.M * d.C * d.C + 2.0 * d.M * 3 * d.C * d.C


def attention_flops(l):
    if l.fn.__name__ != "rf_attention":
        return 0.0
    a = l.args          # (dtype, q, k, v, out, B, heads, d, Nq, Nk, ...)
    B, heads, d, Nq, Nk = a[5], a[6], a[7], a[8], a[9]
    return 4.0 * B * heads * Nq * Nk * d


def launch_bytes(l):
    """Compulsory bytes of one launch: every distinct operand / output tensor it points at, counted once (a view counts its own elements -- a column slice
    of a concat buffer, a batch half).  Not counted: the split-K scratch, the fp64 GroupNorm slots and LayerNorm records (tiny), anything a kernel re-reads
    (filter taps, K slices): this is the floor a perfect kernel of the same operation would move through HBM."""
    import torch
    keep = list(l.keep)
    if l.fn.__name__ == "rf_conv_gemm" and len(keep) > 9:
        keep = keep[:9] + keep[10:]          # (index 9 = the engine's split-K workspace)
    seen, total = set(), 0
    for k in keep:
        parts = [k]
        if type(k).__name__ in ("Fp8Weight", "Fp8Act"):
            parts = [k.q, k.scale]
        for t in parts:
            if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype != torch.float64:
                key = (t.data_ptr(), t.numel(), t.element_size())
                if key not in seen:
                    seen.add(key)
                    total += t.numel() * t.element_size()
    return total


def time_launches(launches, reps=5, warmup=1):
    """Time every launch of a launch list (HIP events on the current torch stream, which is the stream the launches run on).

    The list is run as a whole, in order, `warmup` + `reps` times -- every launch follows its real predecessor, so caches are in
    the state they have inside the step -- with ONE event between consecutive launches: a launch's time is the interval between the
    event before it and the event after it minus the cost of an empty interval (two events with nothing between, measured in
    the same passes), and the MEDIAN over the passes is reported
    (a mean over three back-to-back repetitions of one launch moved by 13 % between two runs on one box when clocks dipped, and
    ran 4-8 % ahead of the in-graph durations rocprofv3 shows because the operands of a repeated launch stay cached).
    Returns a list of (launch, ms)."""
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for _ in range(warmup):
        for l in launches:
            l(sp)
    n = len(launches)
    med = lambda ts: sorted(ts)[len(ts) // 2] if len(ts) % 2 else 0.5 * (sorted(ts)[len(ts) // 2 - 1] + sorted(ts)[len(ts) // 2])
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)] for _ in range(reps)]
    null = [[torch.cuda.Event(enable_timing=True) for _ in range(9)] for _ in range(reps)]
    for r in range(reps):
        for e in null[r]:                 # empty intervals: what one event record costs on the stream (subtracted below)
            e.record(stream)
        ev[r][0].record(stream)
        for i, l in enumerate(launches):
            l(sp)
            ev[r][i + 1].record(stream)
    torch.cuda.synchronize()
    gap = med([null[r][j].elapsed_time(null[r][j + 1]) for r in range(reps) for j in range(8)])
    # What is subtracted per launch is CAPPED: an empty event interval costs 4.6 us on this chip, but only part of that is in a kernel's
    # interval -- against rocprofv3's in-graph kernel durations of the same build the r03 bench read 2.9 us per launch too much with no
    # correction (GEMM family raw 10.94 ms, rocprofv3 10.49 ms) and 1.6 us too LITTLE with the whole gap subtracted (10.24 ms): the family
    # then looked faster than its own kernel-time sum.  2.5 us keeps every family at or above its rocprofv3 kernel time.
    sub = min(gap, GAP_CAP_MS)
    out, raw, floored = [], {}, 0
    for i, l in enumerate(launches):
        t = med([ev[r][i].elapsed_time(ev[r][i + 1]) for r in range(reps)])
        floored += int(t - sub < 0.5 * t)
        out.append((l, max(t - sub, 0.5 * t)))
        f = launch_family(l)
        raw[f] = raw.get(f, 0.0) + t
    # audit trail of the correction (bench.py reports it beside the corrected numbers)
    time_launches.last_gap_ms = gap
    time_launches.last_sub_ms = sub               # what was actually subtracted per launch (capped)
    time_launches.last_raw_ms = raw               # per family: sum of the UNcorrected event intervals
    time_launches.last_floored = floored          # launches whose correction hit the 0.5 * t floor
    return out


def summarize(timed):
    """Aggregate per kernel family: calls, total ms, algorithmic TFLOP, TFLOP/s."""
    fam = collections.OrderedDict()
    for l, ms in timed:
        f = fam.setdefault(launch_family(l), dict(calls=0, ms=0.0, flops=0.0))
        f["calls"] += 1
        f["ms"] += ms
        f["flops"] += gemm_flops(l) + attention_flops(l) + ffn_flops(l) + attn_in_flops(l)
    for f in fam.values():
        f["tflops_per_s"] = (f["flops"] / (f["ms"] * 1e-3) / 1e12) if f["ms"] > 0 else 0.0
    return fam
