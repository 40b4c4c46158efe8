"""rf_conv_gemm's planner (reface_amd/csrc/gemm_plan.h) against a recorded table, without a GPU.

tests/golden/gemm_plans.json holds what the library answered -- return code, the 24 words of rf_conv_gemm_plan3, the message of a rejection -- for
the descriptors of tests/gemm_plan_sweep.py BEFORE the planner moved out of the kernels' compile unit.  The planner must answer the same, twice: as
built into the library, and alone, compiled by a host compiler under AddressSanitizer and UndefinedBehaviorSanitizer (tests/gemm_plan_host_main.cpp,
run as a child process).  The table's own coverage is asserted too, so that a thin sweep cannot pass."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_plan_sweep as S  # noqa: E402
from reface_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = {k: i for i, k in enumerate(("stat_rows", "stat_cols", "splitk", "bm", "bn", "wave_cols", "direct", "flags", "waves", "stages", "hx", "glds", "conv", "ln_role", "pm",
                                 "pn", "reduce", "tail_bm", "tail_bn", "tail_waves", "tiles_m", "tiles_n", "split_n", "tail_direct"))}


@pytest.fixture(scope="module")
def sweep():
    """(names, descriptor values, recorded rows, the table's header) -- the descriptors are built once per module"""
    rows = S.descriptors()
    head, gold = S.golden()
    return [n for n, _ in rows], [v for _, v in rows], gold, head


def _diff(names, got, gold):
    bad = [f"{n}: got {g}, recorded {r}" for n, g, r in zip(names, got, gold) if (g[0], list(g[1]), g[2]) != (r[0], list(r[1]), r[2])]
    return bad[:5] + ([f"... and {len(bad) - 5} more"] if len(bad) > 5 else [])


def test_sweep_is_the_recorded_one(sweep):
    names, vals, gold, head = sweep
    assert len(gold) == len(names) == len(set(names))
    assert S.sweep_digest(list(zip(names, vals))) == head["sweep_sha256"], "the sweep's descriptors changed: record the table again AT THE COMMIT IT WAS RECORDED FROM"
    assert head["recorded_from"] == "f0becd4"          # the commit before gemm_plan.h existed


def test_library_answers_as_recorded(sweep):
    names, vals, gold, _ = sweep
    lib = _lib.load()
    assert not _diff(names, [S.ask(lib, v) for v in vals], gold)


def test_plan_and_plan2_report_the_first_words_of_plan3(sweep):
    import ctypes as C
    names, vals, gold, _ = sweep
    lib = _lib.load()
    for n, v, (rc, w, _) in zip(names, vals, gold):
        d, i8, a, b, c = S.to_desc(v), (C.c_int32 * 8)(), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        assert (lib.rf_conv_gemm_plan2(C.byref(d), i8), list(i8)) == (rc, w[:8]), n
        assert (lib.rf_conv_gemm_plan(C.byref(d), C.byref(a), C.byref(b), C.byref(c)), [a.value, b.value, c.value]) == (rc, w[:3]), n


def _compiler():
    """(compiler, the flags that link the sanitizer runtimes statically into the program)"""
    for cxx, static in (("/opt/rocm/llvm/bin/clang++", ["-static-libsan"]), ("clang++", ["-static-libsan"]), ("g++", ["-static-libasan", "-static-libubsan"])):
        p = shutil.which(cxx) or (cxx if os.path.exists(cxx) else None)
        if p:
            return p, static
    raise RuntimeError("no host C++ compiler")


def test_planner_alone_under_sanitizers_answers_as_recorded(sweep, tmp_path):
    names, vals, gold, _ = sweep
    exe = str(tmp_path / "gemm_plan_host_main")
    cxx, static = _compiler()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    os.path.join(ROOT, "tests", "gemm_plan_host_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    lines = tmp_path / "descriptors.txt"
    lines.write_text("".join(S.line_of(v) + "\n" for v in vals))
    r = subprocess.run([exe, str(lines)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = []
    for l in r.stdout.splitlines():
        nums, msg = l.split("|", 1)
        nums = [int(x) for x in nums.split()]
        got.append((nums[0], nums[1:], msg))
    assert len(got) == len(gold)
    assert not _diff(names, got, gold)


def test_table_covers_the_planner(sweep):
    names, vals, gold, _ = sweep
    fam_tiles = {f: set() for f in S.FAMILIES}
    reduce, seen = set(), set()
    for n, (rc, w, _) in zip(names, gold):
        if rc:
            continue
        if n.startswith("grid"):
            fam = n.split("-")[1]
            fam_tiles[fam].add((w[W["bm"]], w[W["bn"]]))
            if w[W["flags"]] & 2:
                fam_tiles[fam].add((w[W["tail_bm"]], w[W["tail_bn"]]))
        reduce.add(w[W["reduce"]])
        seen |= {k for k, on in (("stages 4", w[W["stages"]] == 4), ("hx", w[W["hx"]] == 1), ("two kernels", w[W["flags"]] & 2), ("pm > 1", w[W["pm"]] > 1),
                                 ("direct 0", w[W["direct"]] == 0), ("direct 1", w[W["direct"]] == 1)) if on}
    for fam in S.FAMILIES:          # (fp8 x fp8 has no 256x320 instantiation: its fragments leave no room for the 64-row wave tiles)
        want = set(S.TILES) - ({(256, 320)} if fam == "a8" else set())
        assert fam_tiles[fam] == want, (fam, sorted(want - fam_tiles[fam]))
    assert reduce == {0, 1, 2, 3}
    assert seen == {"stages 4", "hx", "two kernels", "pm > 1", "direct 0", "direct 1"}
    # every rejection that depends on the tile
    msgs = {re.sub(r"\d+", "#", m) for rc, _, m in gold if rc}
    for part in ("per-sample weights need rows_per_sample", "fp# operands need the direct-to-LDS main loop", "fp# output needs the direct epilogue (even TN",
                 "korder # (row-extended A tiles) needs a bf# #x# stride-# pad-# convolution", "LayerNorm folding needs a bf# linear layer on a direct-epilogue tile",
                 "a LayerNorm consumer takes no residual", "ln_stats_out needs the direct epilogue", "ln_stats_in needs the direct epilogue",
                 "ups # needs Hin * Win = # to be a multiple of the #-row tile"):
        assert any(part in m for m in msgs), part
    rejected = sum(1 for rc, _, _ in gold if rc)
    assert 0.10 * len(gold) <= rejected <= 0.50 * len(gold), (rejected, len(gold))
