// ensembleDecoder::on_pcm driven from a file of cf32 samples (one stream), for
// tests/test_gpu_mp2.py: every delivered frame is written out as
//   int64 cif, int32 subch, int32 rate, int32 n_samples, int16 pcm[2 * n_samples]
// usage: test_mp2_dropin IQ.f32 OUT.bin N_FRAMES STEPS  startAddr length bitRate protLevel uepFlag flags ...
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dabgpu_dropin.h"

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 5) % 6) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    std::vector<dabgpu::DSPCOMPLEX> iq((size_t)bytes / sizeof(dabgpu::DSPCOMPLEX));
    if (std::fread(iq.data(), sizeof(dabgpu::DSPCOMPLEX), iq.size(), in) != iq.size()) return 3;
    std::fclose(in);
    try {
        dabgpu::ensembleDecoder::config cfg;
        cfg.n_streams = 1;
        cfg.n_frames = std::atoi(argv[3]);
        for (int a = 5; a < argc; a += 6) {
            dabgpu_subch sc;
            int16_t *f = &sc.startAddr;
            for (int k = 0; k < 6; k++) f[k] = (int16_t)std::strtol(argv[a + k], nullptr, 0);
            cfg.subch.push_back(sc);
        }
        dabgpu::ensembleDecoder dec(cfg);
        long n = 0;
        dec.on_pcm([&](int stream, int64_t cif, int subch, const int16_t *pcm, int n_samples, int rate) {
            const int32_t h[3] = {subch, rate, n_samples};
            if (stream != 0) std::abort();
            std::fwrite(&cif, sizeof cif, 1, out);
            std::fwrite(h, sizeof h, 1, out);
            std::fwrite(pcm, sizeof(int16_t), 2 * (size_t)n_samples, out);
            n++;
        });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        for (int s = 0; s < std::atoi(argv[4]); s++) dec.step();
        std::fclose(out);
        std::printf("MP2 DROPIN OK %ld frames\n", n);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
