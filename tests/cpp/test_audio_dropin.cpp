// ensembleDecoder::on_audio (and on_pcm) driven from a file of cf32 samples (one stream), for
// tests/test_gpu_audio_pipeline.py: every callback is written out in the order it came, as
//   int32 kind (0 on_pcm, 1 on_audio), int64 cif, int32 subch, int32 n_pairs,
//   kind 0: int32 rate, int16 pcm[2 * n_pairs]; kind 1: float samples[2 * n_pairs]
// and a record of kind 2 (no payload) ends each step.
// usage: test_audio_dropin IQ.f32 OUT.bin N_FRAMES STEPS WITH_AUDIO  startAddr length bitRate protLevel uepFlag flags ...
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dabgpu_dropin.h"

int main(int argc, char **argv) {
    if (argc < 6 || (argc - 6) % 6) return 2;
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
        for (int a = 6; a < argc; a += 6) {
            dabgpu_subch sc;
            int16_t *f = &sc.startAddr;
            for (int k = 0; k < 6; k++) f[k] = (int16_t)std::strtol(argv[a + k], nullptr, 0);
            cfg.subch.push_back(sc);
        }
        dabgpu::ensembleDecoder dec(cfg);
        long n_pcm = 0, n_audio = 0;
        const auto head = [&](int32_t kind, int64_t cif, int32_t subch, int32_t n_pairs) {
            std::fwrite(&kind, sizeof kind, 1, out);
            std::fwrite(&cif, sizeof cif, 1, out);
            std::fwrite(&subch, sizeof subch, 1, out);
            std::fwrite(&n_pairs, sizeof n_pairs, 1, out);
        };
        dec.on_pcm([&](int stream, int64_t cif, int subch, const int16_t *pcm, int n_samples, int rate) {
            if (stream != 0) std::abort();
            const int32_t r = rate;
            head(0, cif, subch, n_samples);
            std::fwrite(&r, sizeof r, 1, out);
            std::fwrite(pcm, sizeof(int16_t), 2 * (size_t)n_samples, out);
            n_pcm++;
        });
        if (std::atoi(argv[5]))
            dec.on_audio([&](int stream, int64_t cif, int subch, const float *samples, int n_pairs) {
                if (stream != 0) std::abort();
                head(1, cif, subch, n_pairs);
                std::fwrite(samples, sizeof(float), 2 * (size_t)n_pairs, out);
                n_audio++;
            });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        for (int s = 0; s < std::atoi(argv[4]); s++) {
            dec.step();
            head(2, 0, 0, 0);
        }
        std::fclose(out);
        std::printf("AUDIO DROPIN OK %ld frames %ld audio\n", n_pcm, n_audio);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
