// TEST INFRASTRUCTURE: a stand-alone program over the host audioResampler, built with
// -fsanitize=address,undefined (Makefile.audio) and run by tests/test_sink_cpu.py: every call's PCM
// is a heap block of exactly its length, so that a read past it is seen.
//   input : per sink  int32 n_calls, then per call int32 rate, int32 amount, int16 pcm[2 * amount]
//   output: per call int32 n_pairs (-1: refused), float samples[2 * n_pairs]
#include <cstdio>
#include <vector>

#include "msc_consumers.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_calls;
    while (fread(&n_calls, sizeof n_calls, 1, in) == 1) {
        dabgpu::audioResampler sink;
        for (int32_t c = 0; c < n_calls; c++) {
            int32_t hdr[2];
            if (fread(hdr, sizeof hdr, 1, in) != 1 || hdr[1] < 0) return 3;
            int16_t *pcm = new int16_t[2 * (size_t)hdr[1]];
            if (hdr[1] && fread(pcm, 2 * sizeof(int16_t), (size_t)hdr[1], in) != (size_t)hdr[1]) return 3;
            std::vector<float> got;
            const bool ok = sink.audioOut(pcm, hdr[1], hdr[0], got);
            delete[] pcm;
            if (!ok && !got.empty()) return 4;
            const int32_t n = ok ? (int32_t)(got.size() / 2) : -1;
            fwrite(&n, sizeof n, 1, out);
            if (n > 0) fwrite(got.data(), 2 * sizeof(float), (size_t)n, out);
        }
    }
    fclose(out);
    fclose(in);
    return 0;
}
