// rf_conv_gemm's planner (reface_amd/csrc/gemm_plan.h) alone, built by a host compiler under AddressSanitizer / UndefinedBehaviorSanitizer by
// tests/test_gemm_plan_cpu.py.  Reads descriptors as the text lines of tests/gemm_plan_sweep.py (`field=value ...`, zero fields left out, floats as
// their bit patterns) and prints, per line, what rf_conv_gemm_plan3 answers:  <return code> <24 words>|<message of a rejection>.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../reface_amd/csrc/gemm_plan.h"

static char g_err[1024];
namespace rf {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace rf

#define DESC_INTS(X)                                                                                                                              \
    X(dtype) X(out_dtype) X(M) X(N) X(K) X(C0) X(C1) X(ld0) X(ld1) X(Hin) X(Win) X(Hout) X(Wout) X(KH) X(KW) X(stride) X(pad_t) X(pad_l) X(ups)  \
    X(ldw) X(rows_per_sample) X(ldv) X(ldr) X(act) X(ldo) X(batch) X(sA) X(sW) X(sO) X(sR) X(korder) X(workspace_bytes) X(gn_rows) X(gn_cpg0)   \
    X(gn_coff0) X(gn_slot0) X(gn_nchunks0) X(gn_cpg1) X(gn_coff1) X(gn_slot1) X(gn_nchunks1) X(w_dtype) X(as_ld) X(os_ld) X(ln_out_parts)        \
    X(ln_in_parts) X(ln_in_cols) X(w_sample_stride) X(Cx) X(ldx)
#define DESC_PTRS(X)                                                                                                                             \
    X(src0) X(src1) X(W) X(bias) X(rowvec) X(residual) X(out) X(act_vec) X(workspace) X(gn_part0) X(gn_part1) X(wscale) X(ascale) X(oscale)    \
    X(ln_stats_out) X(ln_stats_in) X(ln_u) X(srcx)
#define DESC_FLOATS(X) X(alpha) X(ln_eps)

static bool set_field(rf_conv_gemm_desc& d, const std::string& key, long long v) {
#define X(f) if (key == #f) { d.f = (decltype(d.f))v; return true; }
    DESC_INTS(X)
#undef X
#define X(f) if (key == #f) { d.f = (decltype(d.f))(uintptr_t)v; return true; }
    DESC_PTRS(X)
#undef X
#define X(f) if (key == #f) { const uint32_t b = (uint32_t)v; memcpy(&d.f, &b, 4); return true; }
    DESC_FLOATS(X)
#undef X
    return false;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <descriptor lines>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        rf_conv_gemm_desc d;
        memset(&d, 0, sizeof(d));
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set_field(d, tok.substr(0, eq), strtoll(tok.c_str() + eq + 1, nullptr, 10))) {
                fprintf(stderr, "bad token '%s'\n", tok.c_str());
                return 2;
            }
        }
        rf::GemmParams p{};
        rf::GemmPlan plan;
        int32_t w[rf::RF_PLAN_WORDS];
        g_err[0] = 0;
        const int rc = rf::plan_conv_gemm(&d, p, plan);
        rf::plan_words(plan, p, w);
        printf("%d", rc);
        for (int i = 0; i < rf::RF_PLAN_WORDS; ++i) printf(" %d", w[i]);
        printf("|%s\n", rc ? g_err : "");
    }
    return 0;
}
