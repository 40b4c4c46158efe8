// The JPEG entropy-decoder core (reface_amd/csrc/jpeg_decode.h) on the host, for tests/test_jpegdec_cpu.py: built with AddressSanitizer and
// UndefinedBehaviorSanitizer and run once over a corpus of good and damaged scans.  It does what rf_jpeg_entropy_decode does: the entry
// point's range checks of the interval starts, then, for every interval the scan holds, check_interval + decode_interval, the first error
// code of a file kept.  Scan, tables and coefficients live in heap blocks of exactly their sizes, so a read or write past an end is a report.
//   usage: jpegdec_host_main <dir>      <dir>/manifest.txt lists the case names; <dir>/<name>.job = int64 desc[24], int32 nivl, int32
//   starts[nivl], the table block, the scan.  Writes <dir>/<name>.coef (int16 [blocks, 64]) and prints "<name> code=<c> plan=<p> blocks=<n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../reface_amd/csrc/jpeg_decode.h"

using namespace rf::jpgdec;

static std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
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
        int16_t* coef = (int16_t*)calloc((size_t)blocks * 64, 2);
        // the entry point's checks of the starts
        bool ok = starts[0] == 0 && d[D_IVL_COUNT] == nivl;
        for (int k = 1; k < nivl && ok; ++k) ok = starts[k] >= 2 && starts[k] >= starts[k - 1] + 2 && starts[k] <= (long long)scan_len;
        int code = ok ? OK : -1;
        if (ok) {
            const long long expected = g.intervals(d[D_RI]);
            for (long long k = 0; k < nivl; ++k) {          // one lane each on the device
                int rc = check_interval(scan, starts, k, nivl, expected);
                if (rc == OK) {
                    const uint32_t begin = (uint32_t)starts[k];
                    const uint32_t end = k + 1 < nivl ? (uint32_t)starts[k + 1] - 2u : (uint32_t)scan_len;
                    rc = decode_interval(scan, begin, end, d, tables, k, coef);
                }
                if (rc != OK && code == OK) code = rc;
            }
        }
        FILE* o = fopen((dir + "/" + name + ".coef").c_str(), "wb");
        fwrite(coef, 2, (size_t)blocks * 64, o);
        fclose(o);
        printf("%s code=%d plan=%d blocks=%lld\n", name.c_str(), code, d[D_RI] > 0 ? 1 : 0, blocks);
        free(coef);
        free(scan);
        free(tables);
        free(starts);
    }
    return 0;
}
