// Stand-alone host program around reface_amd/csrc/png_blocks.h, the block-parallel inflate plan of the device PNG decoder: the same code,
// compiled by a host compiler with -fsanitize=address,undefined by tests/test_pngblocks_cpu.py and run as a child process.  It emulates the
// five stages (search, count, chain, decode, resolve) as the device orders them, then the serial plan for whatever was not accepted.
// Usage:  pngblocks_host_main <dir> <min_bytes> <block_bytes> [<block_bytes> ...]   where <dir>/manifest.txt has one line per stream,
//     <name> <expected length>
// and <dir>/<name> holds the stream.  One line is printed per stream and block_bytes:
//     <name> bb=<block_bytes> code=<the serial core's code> sha=<SHA-256 of the serial output or -> plan=<blocks|serial> eligible=<0|1>
//     chunks=<chain length> candidates=<found> fallback=<0|1> out=<SHA-256 of what the plan leaves, or -> same=<0|1: equal to the serial output>
//     blocks=<all block starts the serial walker met> dyn=<the dynamic ones> dynfound=<of those, candidates> chaintrue=<chain chunks that
//     start at candidate 0 or at a dynamic block start> fixed=<the fixed blocks among the block starts> maxdist=<n>
// The buffers are sized exactly (compressed bytes, output, symbols), so an access beyond any of them is the sanitizer's to report.
#define main pngdec_host_main_unused          // HostSrc, HostSink, HostW and sha256 are that program's
#include "pngdec_host_main.cpp"
#undef main

#include <algorithm>
#include <set>

#include "../reface_amd/csrc/png_blocks.h"

// the W policy that records where the serial walker's blocks start: note_block runs behind the 3 header bits
struct Start {
    uint32_t bit;
    int type;
};
static std::vector<Start> g_starts;
static const BitReader<HostSrc>* g_br;
struct RecW : HostW {
    static void note_block(int t) {
        g_starts.push_back({g_br->bitpos() - 3u, t});
        HostW::note_block(t);
    }
};

struct BitmapStop {
    const std::vector<uint32_t>* bm;
    bool operator()(uint32_t bit) const { return (bit >> 5) < bm->size() && (((*bm)[bit >> 5] >> (bit & 31)) & 1u); }
};
struct StopAt {
    uint32_t bit;
    bool operator()(uint32_t b) const { return b == bit; }
};

struct Result {
    bool eligible = false, accepted = false;
    int chunks = 0, candidates = 0, chaintrue = 0;
    std::vector<uint8_t> out;
};

static Result run_blocks(const HostSrc& src, uint32_t expect, const std::vector<uint32_t>& hits, bool header_ok, uint32_t block_bytes, uint32_t min_bytes,
                         const std::set<uint32_t>& dyn_starts, Tables* tables) {
    Result r;
    r.eligible = src.size() < BLK_MAX_STREAM && expect >= min_bytes;
    if (!r.eligible) return r;
    const uint32_t cap = 16 + src.size() / block_bytes, tsize = 2 * cap;
    // search: slot 0 is candidate 0; a hit beyond the capacity is counted and dropped
    std::vector<Chunk> ch(cap);
    memset(ch.data(), 0, cap * sizeof(Chunk));
    std::vector<int32_t> hash(tsize, 0), order(cap, 0);
    std::vector<uint32_t> bitmap((src.size() + 3) / 4, 0);
    if (header_ok) ch[0].start = FIRST_BIT;
    uint32_t found = 1;
    for (uint32_t bit : hits) {
        bitmap[bit >> 5] |= 1u << (bit & 31);
        const uint32_t slot = found++;
        if (slot >= cap) continue;
        ch[slot].start = bit;
        uint32_t h = blk_hash(bit, tsize);
        while (hash[h] != 0) h = h + 1 == tsize ? 0 : h + 1;          // the table is twice the slots: a free word exists
        hash[h] = (int32_t)slot + 1;
    }
    r.candidates = (int)found;
    if (found > cap) return r;          // overflow: not accepted
    // count
    for (uint32_t s = 0; s < found; ++s) {
        if (ch[s].start < FIRST_BIT) continue;
        CountSink sink{expect, 0};
        WalkResult w;
        walk_blocks<HostSrc, CountSink, HostW, BitmapStop>(src, ch[s].start, sink, tables, BitmapStop{&bitmap}, &w);
        ch[s].end = w.end;
        ch[s].count = w.count;
        ch[s].flags = (w.status == OK ? 1 : 0) | (w.final ? 2 : 0);
    }
    // chain
    uint32_t want = 0;
    const int n = blocks_chain_accept(src, ch.data(), (int)found, hash.data(), tsize, order.data(), expect, &want);
    if (n == 0) return r;
    // decode: exactly `expect` symbols
    uint16_t* sym = (uint16_t*)malloc((size_t)expect * 2);
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        Chunk& c = ch[order[k]];
        MarkerSink sink{sym + c.off, c.count, 0};
        WalkResult w;
        walk_blocks<HostSrc, MarkerSink, HostW, StopAt>(src, c.start, sink, tables, StopAt{c.end}, &w);
        if (w.status == OK && w.end == c.end && w.count == c.count) c.flags |= 4;
    }
    // resolve
    r.out.assign(expect, 0);
    uint64_t s1 = 1, s2 = 0;
    for (int k = 0; k < n && ok; ++k) {
        const Chunk& c = ch[order[k]];
        if (!(c.flags & 4)) ok = false;
        uint64_t a = 0, b = 0;
        for (uint32_t i = 0; i < c.count && ok; ++i) {
            uint8_t v = 0;
            ok = resolve_sym(sym[c.off + i], c.off, r.out.data(), &v);
            r.out[c.off + i] = v;
            a += v;
            b += (uint64_t)(c.count - i) * v;
        }
        adler_push(&s1, &s2, c.count, (uint32_t)(a % ADLER_MOD), (uint32_t)(b % ADLER_MOD));
        if (c.start == FIRST_BIT || dyn_starts.count(c.start)) r.chaintrue++;
    }
    free(sym);
    if (ok && want == (uint32_t)((s2 << 16) | s1)) {
        r.accepted = true;
        r.chunks = n;
    } else {
        r.out.clear();
    }
    return r;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <corpus directory> <min_bytes> <block_bytes> ...\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const uint32_t min_bytes = (uint32_t)atoll(argv[2]);
    std::ifstream man(dir + "/manifest.txt");
    if (!man) {
        fprintf(stderr, "no manifest in %s\n", dir.c_str());
        return 2;
    }
    Tables* tables = new Tables;
    std::string name;
    long long expect;
    while (man >> name >> expect) {
        std::ifstream f(dir + "/" + name, std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        uint8_t* comp = (uint8_t*)malloc(raw.size() ? raw.size() : 1);
        if (!raw.empty()) memcpy(comp, raw.data(), raw.size());
        uint8_t* out = (uint8_t*)malloc(expect > 0 ? (size_t)expect : 1);
        const HostSrc src{comp, (uint32_t)raw.size()};
        // the serial core: the code and the bytes every setting must end on
        memset(&g_stats, 0, sizeof g_stats);
        HostSink sink{out, (uint32_t)expect, 0, 1, 0};
        const int code = inflate_zlib<HostSrc, HostSink, HostW>(src, sink, tables);
        const int maxdist = g_stats.maxdist;
        const std::string sha = code == OK ? sha256(out, (size_t)expect) : "-";
        // the block starts of the serial walker, through its W policy
        g_starts.clear();
        const bool header_ok = zlib_header(src) == OK;
        if (header_ok) {
            uint8_t* out2 = (uint8_t*)malloc(expect > 0 ? (size_t)expect : 1);
            HostSink s2{out2, (uint32_t)expect, 0, 1, 0};
            BitReader<HostSrc> br(src, 2);
            g_br = &br;
            int ended;
            inflate_blocks<HostSrc, HostSink, RecW>(br, s2, tables, true, &ended);
            free(out2);
        }
        std::set<uint32_t> dyn;
        int nfixed = 0;
        for (const Start& s : g_starts) {
            if (s.type == 2) dyn.insert(s.bit);
            nfixed += s.type == 1;
        }
        // search, once for every setting: it does not depend on block_bytes
        std::vector<uint32_t> hits;
        const bool searched = src.size() < BLK_MAX_STREAM && (uint32_t)expect >= min_bytes;
        if (searched)
            for (uint32_t bit = FIRST_BIT + 1; bit < 8 * src.size(); ++bit)
                if (dyn_header_at(src, bit)) hits.push_back(bit);
        int dynfound = 0;
        for (uint32_t b : dyn)
            if (b == FIRST_BIT || std::binary_search(hits.begin(), hits.end(), b)) ++dynfound;
        for (int a = 3; a < argc; ++a) {
            const uint32_t bb = (uint32_t)atoll(argv[a]);
            const Result r = run_blocks(src, (uint32_t)expect, hits, header_ok, bb, min_bytes, dyn, tables);
            const bool same = r.accepted ? (code == OK && memcmp(out, r.out.data(), (size_t)expect) == 0) : true;
            const std::string osha = r.accepted ? sha256(r.out.data(), r.out.size()) : sha;
            printf("%s bb=%u code=%d sha=%s plan=%s eligible=%d chunks=%d candidates=%d fallback=%d out=%s same=%d blocks=%d dyn=%d dynfound=%d chaintrue=%d fixed=%d maxdist=%d\n",
                   name.c_str(), bb, code, sha.c_str(), r.accepted ? "blocks" : "serial", r.eligible ? 1 : 0, r.chunks, r.candidates,
                   r.eligible && !r.accepted ? 1 : 0, osha.c_str(), same ? 1 : 0, (int)g_starts.size(), (int)dyn.size(), dynfound, r.accepted ? r.chaintrue : 0,
                   nfixed, maxdist);
        }
        free(comp);
        free(out);
    }
    delete tables;
    return 0;
}
