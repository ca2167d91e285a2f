// TEST INFRASTRUCTURE: the host rateConverter under the sanitizers, as a stand-alone program
// (tests/cpp/Makefile.rate builds it with -fsanitize=address,undefined; tests/test_rate_cpu.py
// runs it).  Input: records of int32 rate, int32 format, int32 n_samples, int32 n_chunks,
// int32 chunk[n_chunks] (the chunk sizes, used in turn until the samples are through), then the
// samples as the format holds them.  Every chunk goes through convert as a heap block of exactly
// its length.  Output: per record int64 n_out, then the n_out cf32 samples.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rate_converter.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t hdr[4];
    while (fread(hdr, sizeof hdr, 1, in) == 1) {
        if (hdr[2] < 0 || hdr[3] < 1 || hdr[3] > 64) return 3;
        std::vector<int32_t> chunk((size_t)hdr[3]);
        if (fread(chunk.data(), sizeof(int32_t), chunk.size(), in) != chunk.size()) return 3;
        const size_t bps = (size_t)dabgpu::rate_format_bytes(hdr[1]);
        std::vector<char> x(bps * (size_t)hdr[2] + 1);
        if (hdr[2] && fread(x.data(), bps, (size_t)hdr[2], in) != (size_t)hdr[2]) return 3;
        dabgpu::rateConverter c(hdr[0], hdr[1]);
        std::vector<dabgpu::rateConverter::DSPCOMPLEX> got;
        size_t idle = 0;                                  // empty chunks in a row
        for (int64_t at = 0, turn = 0; at < hdr[2] && idle < chunk.size(); turn++) {
            int64_t m = chunk[(size_t)turn % chunk.size()];
            if (m < 0) return 3;
            idle = m ? 0 : idle + 1;
            if (m > hdr[2] - at) m = hdr[2] - at;
            char *piece = (char *)malloc(bps * (size_t)m + (m ? 0 : 1));
            memcpy(piece, x.data() + bps * (size_t)at, bps * (size_t)m);
            c.convert(piece, m, got);
            free(piece);
            at += m;
        }
        const int64_t n = (int64_t)got.size();
        fwrite(&n, sizeof n, 1, out);
        if (n) fwrite(got.data(), sizeof(got[0]), got.size(), out);
    }
    fclose(out);
    return 0;
}
