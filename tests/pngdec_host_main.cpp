// Stand-alone host program around reface_amd/csrc/png_inflate.h, the decoder core of the device PNG decoder: the same code, compiled by
// a host compiler with -fsanitize=address,undefined by tests/test_pngdec_cpu.py and run as a child process on a corpus of good and damaged
// zlib streams.  Usage:  pngdec_host_main <dir>   where <dir>/manifest.txt has one line per stream,
//     <name> <expected length> [<H> <W> <bpp>] [c <candidate offset> ...]
// and <dir>/<name> holds the stream.  One line is printed per stream:
//     <name> code=<error code> sha=<SHA-256 of the output> pix=<SHA-256 of the unfiltered pixels or -> plan=<segments|serial> pieces=<n>
//     stored=<n> fixed=<n> dynamic=<n> empty=<n> maxlen=<n> maxdist=<n> maxcode=<n> run1=<longest total of consecutive distance-1 matches>
// The serial decode sizes its output buffer to exactly the expected length and the compressed bytes to exactly the file, so an access
// beyond either is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../reface_amd/csrc/png_inflate.h"

using namespace rf::pnginf;

struct Stats {
    int blocks[4], empty, maxlen, maxdist, maxcode, run1, cur1;
};
static Stats g_stats;

struct HostW {
    static bool leader() { return true; }
    static void sync() {}
    static void note_block(int t) {
        g_stats.blocks[t & 3]++;
        g_stats.cur1 = 0;
    }
    static void note_match(int len, int dist) {
        if (len > g_stats.maxlen) g_stats.maxlen = len;
        if (dist > g_stats.maxdist) g_stats.maxdist = dist;
        g_stats.cur1 = dist == 1 ? g_stats.cur1 + len : 0;
        if (g_stats.cur1 > g_stats.run1) g_stats.run1 = g_stats.cur1;
    }
    static void note_empty_stored() { g_stats.empty++; }
    static void note_code_length(int l) {
        if (l > g_stats.maxcode) g_stats.maxcode = l;
    }
};

struct HostSrc {
    const uint8_t* p;
    uint32_t n;
    uint32_t size() const { return n; }
    uint32_t byte(uint32_t i) const { return p[i]; }
    uint32_t word(uint32_t i) const { return (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24); }
};

// a0 / b0: the Adler-32 state the sink starts from (1, 0 for a whole stream; 0, 0 for a piece's partial)
struct HostSink {
    uint8_t* out;
    uint32_t capv, pos, a0, b0;
    uint32_t cap() const { return capv; }
    uint32_t produced() const { return pos; }
    bool literal(uint8_t v) {
        if (pos >= capv) return false;
        out[pos++] = v;
        g_stats.cur1 = 0;
        return true;
    }
    int match(int len, int dist) {
        if ((uint32_t)dist > pos) return E_DISTANCE;
        if ((uint32_t)len > capv - pos) return E_TOO_LONG;
        for (int i = 0; i < len; ++i, ++pos) out[pos] = out[pos - (uint32_t)dist];
        return OK;
    }
    void copy(const HostSrc& src, uint32_t p, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) out[pos++] = (uint8_t)src.byte(p + i);
    }
    uint32_t finish() {
        uint64_t a = a0, b = b0;
        if (a0 == 0) {          // a piece's partial: A = sum, B = sum of (count - i) * byte_i
            for (uint32_t i = 0; i < pos; ++i) {
                a = (a + out[i]) % ADLER_MOD;
                b = (b + (uint64_t)(pos - i) * out[i]) % ADLER_MOD;
            }
        } else {
            for (uint32_t i = 0; i < pos; ++i) {
                a = (a + out[i]) % ADLER_MOD;
                b = (b + a) % ADLER_MOD;
            }
        }
        return (uint32_t)((b << 16) | a);
    }
};

// ---- SHA-256 (FIPS 180-4)
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static std::string sha256(const uint8_t* data, size_t n) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<uint8_t> m(data, data + n);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const uint64_t bits = (uint64_t)n * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
    for (size_t o = 0; o < m.size(); o += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = ((uint32_t)m[o + 4 * i] << 24) | ((uint32_t)m[o + 4 * i + 1] << 16) | ((uint32_t)m[o + 4 * i + 2] << 8) | (uint32_t)m[o + 4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
        }
        h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
    }
    char buf[65];
    for (int i = 0; i < 8; ++i) snprintf(buf + 8 * i, 9, "%08x", h[i]);
    return std::string(buf, 64);
}

// plain serial reconstruction of the filtered rows; false on a filter byte above 4
static bool unfilter(const uint8_t* s, int H, int W, int bpp, std::vector<uint8_t>& out) {
    const size_t n = (size_t)W * bpp;
    out.assign((size_t)H * n, 0);
    for (int y = 0; y < H; ++y) {
        const uint8_t* r = s + (size_t)y * (1 + n);
        const int t = r[0];
        if (t > 4) return false;
        uint8_t* cur = out.data() + (size_t)y * n;
        const uint8_t* up = y ? cur - n : nullptr;
        for (size_t i = 0; i < n; ++i) {
            const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= (size_t)bpp) ? up[i - bpp] : 0;
            cur[i] = (uint8_t)((r[1 + i] + png_predict(t, a, b, c)) & 255);
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <corpus directory>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream man(dir + "/manifest.txt");
    if (!man) {
        fprintf(stderr, "no manifest in %s\n", dir.c_str());
        return 2;
    }
    std::string line;
    Tables* tables = new Tables;
    while (std::getline(man, line)) {
        std::istringstream ls(line);
        std::string name, tok;
        long long expect = -1;
        int H = 0, W = 0, bpp = 0;
        std::vector<int32_t> cand;
        if (!(ls >> name >> expect)) continue;
        bool in_c = false;
        std::vector<long long> nums;
        while (ls >> tok) {
            if (tok == "c") in_c = true;
            else if (in_c) cand.push_back((int32_t)atoll(tok.c_str()));
            else nums.push_back(atoll(tok.c_str()));
        }
        if (nums.size() == 3) H = (int)nums[0], W = (int)nums[1], bpp = (int)nums[2];
        std::ifstream f(dir + "/" + name, std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        // exact-size heap copies: an overrun of either buffer lands in a sanitizer redzone
        uint8_t* comp = (uint8_t*)malloc(raw.size() ? raw.size() : 1);
        if (!raw.empty()) memcpy(comp, raw.data(), raw.size());
        uint8_t* out = (uint8_t*)malloc(expect > 0 ? (size_t)expect : 1);
        memset(&g_stats, 0, sizeof g_stats);
        const HostSrc src{comp, (uint32_t)raw.size()};
        HostSink sink{out, (uint32_t)expect, 0, 1, 0};
        const int code = inflate_zlib<HostSrc, HostSink, HostW>(src, sink, tables);
        const Stats st = g_stats;
        const std::string sha = code == OK ? sha256(out, (size_t)expect) : "-";
        std::string pix = "-";
        if (code == OK && H > 0) {
            std::vector<uint8_t> px;
            pix = unfilter(out, H, W, bpp, px) ? sha256(px.data(), px.size()) : "badfilter";
        }
        // the segmented plan as the device runs it: a piece per candidate into a slot of WINDOW bytes, then the chain
        int npieces = 0;
        bool same = true;
        if (cand.size() >= 2) {
            std::vector<Piece> pieces(cand.size());
            std::vector<uint8_t*> slots(cand.size());
            for (size_t c = 0; c < cand.size(); ++c) {
                slots[c] = (uint8_t*)malloc(WINDOW);
                HostSink ps{slots[c], (uint32_t)WINDOW, 0, 0, 0};
                inflate_piece<HostSrc, HostSink, HostW>(src, (uint32_t)cand[c], ps, tables, &pieces[c]);
            }
            npieces = chain_accept(src, cand.data(), pieces.data(), (int)cand.size(), (uint32_t)expect);
            if (npieces > 0) {          // what the gather kernel assembles must be what the serial plan decoded
                same = code == OK;
                for (size_t c = 0; c < cand.size() && same; ++c)
                    if (pieces[c].k >= 0) same = memcmp(out + (size_t)pieces[c].k * WINDOW, slots[c], (size_t)pieces[c].count) == 0;
            }
            for (uint8_t* s : slots) free(s);
        }
        printf("%s code=%d sha=%s pix=%s plan=%s pieces=%d stored=%d fixed=%d dynamic=%d empty=%d maxlen=%d maxdist=%d maxcode=%d run1=%d\n", name.c_str(), code,
               sha.c_str(), pix.c_str(), npieces > 0 ? (same ? "segments" : "MISMATCH") : "serial", npieces, st.blocks[0], st.blocks[1], st.blocks[2], st.empty,
               st.maxlen, st.maxdist, st.maxcode, st.run1);
        free(comp);
        free(out);
    }
    delete tables;
    return 0;
}
