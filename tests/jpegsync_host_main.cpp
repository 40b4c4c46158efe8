// The self-synchronising plan of the JPEG entropy decoder (reface_amd/csrc/jpeg_sync.h) on the host, for tests/test_jpegsync_cpu.py: built
// with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program.  It does what rf_jpeg_selfsync_decode enqueues: `launches`
// launches in which every workgroup of 64 lanes iterates to its fixed point (Jacobi passes, 64 at the most) from the boundary states the
// launch began with, returns at once when its incoming state is the one it last ran with, and publishes its outgoing state; the prefix sum
// of the block counts; the write pass; the DC prefix sums; and the serial core for a file whose last launch still moved a boundary.  The
// serial core also runs on every file, for its error code.  Scan, tables and coefficients live in heap blocks of exactly their sizes.
//   usage: jpegsync_host_main <dir> <subseq_bytes> <launches>     <dir> as tests/jpegdec_host_main.cpp reads it.  Writes
//   <dir>/<name>.coef and prints "<name> code=<c> serial_code=<c> plan=<p> fallback=<0|1> subseqs=<n> wgs=<n> launches_used=<n>
//   ff_cut=<cuts between FF and 00> straddle=<true states behind their cut> blocks=<n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../reface_amd/csrc/jpeg_sync.h"

using namespace rf::jpgdec;

static std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Sync {
    std::vector<uint64_t> state, seen;
    std::vector<int> cnt, chg;
    std::vector<long long> first;
};

// one workgroup of one launch, as jpeg_sync_kernel; `begin` = the states the launch began with
static void workgroup(const SsFile& file, const long long* d, Sync& w, const std::vector<uint64_t>& begin, long long x, int launch) {
    const long long n = d[D_SS_COUNT], g0 = x * SS_LANES;
    const uint64_t L = (uint64_t)d[D_SS_BYTES];
    const uint32_t len = file.len;
    uint64_t incoming = x == 0 ? 0ull : begin[g0];
    if (incoming == SS_NEVER) incoming = ss_guess(file.scan, len, (uint64_t)g0 * L);
    const bool first_run = w.seen[x] == SS_NEVER;
    if (!first_run && incoming == w.seen[x]) return;
    uint64_t sh[SS_LANES + 1];
    int mycnt[SS_LANES];
    bool dirty[SS_LANES];
    for (int lane = 0; lane < SS_LANES; ++lane) {
        const long long gi = g0 + lane;
        const bool live = gi < n;
        sh[lane] = !live ? 0 : lane == 0 ? incoming : first_run ? ss_guess(file.scan, len, (uint64_t)gi * L) : w.state[gi];
        mycnt[lane] = live && !first_run ? w.cnt[gi] : 0;
        dirty[lane] = live && (first_run || lane == 0);
    }
    uint64_t old_out = 0;
    if (g0 + SS_LANES < n) {
        old_out = begin[g0 + SS_LANES];
        if (old_out == SS_NEVER) old_out = ss_guess(file.scan, len, (uint64_t)(g0 + SS_LANES) * L);
    }
    sh[SS_LANES] = old_out;
    for (int pass = 0; pass < SS_LANES; ++pass) {
        uint64_t in[SS_LANES], out[SS_LANES];
        bool moved[SS_LANES], any = false;
        for (int lane = 0; lane < SS_LANES; ++lane) {
            const long long gi = g0 + lane;
            in[lane] = sh[lane];
            moved[lane] = false;
            if (dirty[lane]) {
                const uint64_t bound = 8ull * (((uint64_t)gi + 1) * L < len ? ((uint64_t)gi + 1) * L : len);
                out[lane] = ss_eval(file, in[lane], bound, &mycnt[lane]);
                moved[lane] = out[lane] != sh[lane + 1];
            }
        }
        for (int lane = 0; lane < SS_LANES; ++lane)
            if (moved[lane]) {
                sh[lane + 1] = out[lane];
                any = true;
            }
        for (int lane = 0; lane < SS_LANES; ++lane) dirty[lane] = g0 + lane < n && lane > 0 && sh[lane] != in[lane];
        if (!any) break;
    }
    for (int lane = 0; lane < SS_LANES; ++lane) {
        const long long gi = g0 + lane;
        if (gi >= n) break;
        w.cnt[gi] = mycnt[lane];
        if (gi + 1 < n) {
            w.state[gi + 1] = sh[lane + 1];
            if (lane == SS_LANES - 1 && sh[SS_LANES] != old_out) w.chg[launch] = 1;
        }
    }
    w.seen[x] = incoming;
}

static int serial(const uint8_t* scan, const int32_t* starts, int nivl, const long long* d, const uint8_t* tables, const Geometry& g, int16_t* coef) {
    int code = OK;
    const long long expected = g.intervals(d[D_RI]);
    for (long long k = 0; k < nivl; ++k) {
        int rc = check_interval(scan, starts, k, nivl, expected);
        if (rc == OK) {
            const uint32_t begin = (uint32_t)starts[k];
            const uint32_t end = k + 1 < nivl ? (uint32_t)starts[k + 1] - 2u : (uint32_t)d[D_SCAN_LEN];
            rc = decode_interval(scan, begin, end, d, tables, k, coef);
        }
        if (rc != OK && code == OK) code = rc;
    }
    return code;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::string dir = argv[1];
    const long long L = atoll(argv[2]);
    const int launches = atoi(argv[3]);
    if (L < SS_MIN_BYTES || L > SS_MAX_BYTES || launches < 1 || launches > SS_MAX_LAUNCHES) return 2;
    std::ifstream manifest(dir + "/manifest.txt");
    std::string name;
    while (manifest >> name) {
        const std::vector<uint8_t> job = read_file(dir + "/" + name + ".job");
        long long d[DESC];
        int32_t nivl = 0;
        size_t at = 0;
        if (job.size() < sizeof(d) + 4) return 2;
        memcpy(d, job.data(), sizeof(d));
        at += sizeof(d);
        memcpy(&nivl, job.data() + at, 4);
        at += 4;
        if (nivl < 1 || job.size() < at + 4ull * nivl + TABLE_BYTES + (size_t)d[D_SCAN_LEN]) return 2;
        int32_t* starts = (int32_t*)malloc(4ull * nivl);
        memcpy(starts, job.data() + at, 4ull * nivl);
        at += 4ull * nivl;
        uint8_t* tables = (uint8_t*)aligned_alloc(16, TABLE_BYTES);
        memcpy(tables, job.data() + at, TABLE_BYTES);
        at += TABLE_BYTES;
        const size_t scan_len = (size_t)d[D_SCAN_LEN];
        uint8_t* scan = (uint8_t*)malloc(scan_len ? scan_len : 1);
        memcpy(scan, job.data() + at, scan_len);
        const Geometry g = geometry((int)d[D_H], (int)d[D_W], (int)d[D_NCOMP], (int)d[D_HS], (int)d[D_VS]);
        const long long blocks = g.blocks();
        bool ok = starts[0] == 0 && d[D_IVL_COUNT] == nivl;
        for (int k = 1; k < nivl && ok; ++k) ok = starts[k] >= 2 && starts[k] >= starts[k - 1] + 2 && starts[k] <= (long long)scan_len;
        if (!ok) return 2;
        // the serial plan's code, on coefficients of its own
        int16_t* ref = (int16_t*)calloc((size_t)blocks * 64, 2);
        const int serial_code = serial(scan, starts, nivl, d, tables, g, ref);
        int16_t* coef = (int16_t*)calloc((size_t)blocks * 64, 2);
        int code = OK, plan = d[D_RI] > 0 ? 1 : 0, fallback = 0, used = 0, ff_cut = 0, straddle = 0;
        long long n = 0, wgs = 0;
        if (d[D_RI] == 0 && (long long)scan_len >= 2 * L) {
            n = ((long long)scan_len + L - 1) / L;
            wgs = (n + SS_LANES - 1) / SS_LANES;
            d[D_SS_BEGIN] = 0;
            d[D_SS_COUNT] = n;
            d[D_SS_BYTES] = L;
            d[D_SS_WG_BEGIN] = 0;
            plan = PLAN_SELFSYNC;
            if (nivl != 1) {
                code = E_RST_COUNT;
            } else {
                const SsFile file = ss_file(scan, d, (const HuffTab*)(tables + QUANT_BYTES));
                Sync w;
                w.state.assign((size_t)n, SS_NEVER);
                w.seen.assign((size_t)wgs, SS_NEVER);
                w.cnt.assign((size_t)n, -1);
                w.first.assign((size_t)n, 0);
                w.chg.assign((size_t)launches, 0);
                for (int k = 0; k < launches; ++k) {
                    const std::vector<uint64_t> begin = w.state;
                    for (long long x = 0; x < wgs; ++x) workgroup(file, d, w, begin, x, k);
                }
                int last = -1;
                for (int k = 0; k < launches; ++k) last = w.chg[k] ? k : last;
                fallback = last == launches - 1;
                used = last + 2 < launches ? last + 2 : launches;
                if (fallback) {
                    plan = 0;
                    code = serial(scan, starts, nivl, d, tables, g, coef);
                } else {
                    long long run = 0;
                    for (long long i = 0; i < n; ++i) {
                        w.first[i] = run;
                        run += w.cnt[i];
                    }
                    unsigned long long err = ~0ull;
                    for (long long i = 0; i < n; ++i) {
                        const uint64_t bound = 8ull * ((uint64_t)(i + 1) * L < scan_len ? (uint64_t)(i + 1) * L : scan_len);
                        const uint64_t s = i == 0 ? 0ull : w.state[i];
                        if (i > 0 && scan[i * L - 1] == 0xFF && scan[i * L] == 0) ++ff_cut;
                        if (i > 0 && w.first[i] < blocks && ss_pos(s) > ss_pos(ss_guess(scan, (uint32_t)scan_len, (uint64_t)i * L))) ++straddle;
                        const int rc = ss_write(file, s, bound, i == n - 1, w.first[i], blocks, coef);
                        const unsigned long long e = ((unsigned long long)i << 8) | (unsigned long long)rc;
                        if (rc != OK && e < err) err = e;
                    }
                    if (err != ~0ull) {
                        code = (int)(err & 255);
                    } else {
                        const int ny = file.ny;
                        for (int c = 0; c < (int)d[D_NCOMP]; ++c) {
                            uint32_t pred = 0;
                            const long long nb = g.mcus() * (c == 0 ? ny : 1);
                            for (long long i = 0; i < nb; ++i) {
                                int16_t* o = coef + ss_block_of(i, c, ny, g.bpm) * 64;
                                pred += (uint32_t)(int32_t)*o;
                                *o = (int16_t)pred;
                            }
                        }
                    }
                }
            }
        } else {
            code = serial(scan, starts, nivl, d, tables, g, coef);
        }
        FILE* o = fopen((dir + "/" + name + ".coef").c_str(), "wb");
        fwrite(coef, 2, (size_t)blocks * 64, o);
        fclose(o);
        printf("%s code=%d serial_code=%d plan=%d fallback=%d subseqs=%lld wgs=%lld launches_used=%d ff_cut=%d straddle=%d blocks=%lld\n", name.c_str(), code, serial_code,
               plan, fallback, n, wgs, used, ff_cut, straddle, blocks);
        free(coef);
        free(ref);
        free(scan);
        free(tables);
        free(starts);
    }
    return 0;
}
