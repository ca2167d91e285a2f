// ensembleDecoder::load_rate against rateConverter followed by load, for
// tests/test_gpu_rate_pipeline.py: one file of int16 I/Q pairs per stream, each at its own rate.  A
// decoder takes streams of one rate, so every stream gets two one-stream decoders: one loads the
// int16 samples through load_rate (converted on the device), the other the host rateConverter's
// output through load.  Both run STEPS steps of N_FRAMES frames and must deliver the same on_fib
// sequence (frame, ficno, the 256 bits, the CRC flag).
// Prints "FIB stream frame ficno crc_ok" per FIB and "RATE DROPIN OK <fibs> fibs <good> good" at the end.
// usage: test_rate_dropin N_FRAMES STEPS  RATE IN.s16 [RATE IN.s16 ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dabgpu_dropin.h"
#include "rate_converter.h"

struct fib {
    int64_t frame;
    int ficno;
    bool ok;
    std::string bits;
    bool operator==(const fib &o) const { return frame == o.frame && ficno == o.ficno && ok == o.ok && bits == o.bits; }
};

static std::vector<fib> run(int n_frames, int steps, const std::function<void(dabgpu::ensembleDecoder &)> &load) {
    dabgpu::ensembleDecoder::config cfg;
    cfg.n_streams = 1;
    cfg.n_frames = n_frames;
    dabgpu::ensembleDecoder dec(cfg);
    std::vector<fib> got;
    dec.on_fib([&](int stream, int64_t frame, int ficno, const uint8_t *bits256, bool crc_ok) {
        if (stream != 0) std::abort();
        got.push_back({frame, ficno, crc_ok, std::string((const char *)bits256, 256)});
    });
    load(dec);
    for (int s = 0; s < steps; s++) dec.step();
    return got;
}

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 3) % 2) return 2;
    const int n_frames = std::atoi(argv[1]), steps = std::atoi(argv[2]);
    long total = 0, good = 0;
    int fails = 0;
    try {
        for (int a = 3, stream = 0; a < argc; a += 2, stream++) {
            const int rate = std::atoi(argv[a]);
            std::FILE *in = std::fopen(argv[a + 1], "rb");
            if (!in) return 2;
            std::fseek(in, 0, SEEK_END);
            std::vector<int16_t> x((size_t)std::ftell(in) / sizeof(int16_t));
            std::fseek(in, 0, SEEK_SET);
            if (std::fread(x.data(), sizeof(int16_t), x.size(), in) != x.size()) return 3;
            std::fclose(in);
            const int64_t n = (int64_t)(x.size() / 2);
            const std::vector<fib> dev = run(n_frames, steps, [&](dabgpu::ensembleDecoder &d) {
                d.load_rate(rate, DABGPU_IQ_S12, {x.data()}, {n});
            });
            const std::vector<fib> host = run(n_frames, steps, [&](dabgpu::ensembleDecoder &d) {
                dabgpu::rateConverter c(rate, dabgpu::RATE_IQ_S12);
                std::vector<dabgpu::DSPCOMPLEX> iq;
                c.convert(x.data(), n, iq);
                d.load({iq.data()}, {(int64_t)iq.size()});
            });
            if (!(dev == host)) {
                std::printf("MISMATCH: stream %d at %d Hz: %zu FIBs through load_rate, %zu through rateConverter and load\n", stream, rate,
                            dev.size(), host.size());
                fails++;
            }
            for (const fib &f : dev) {
                std::printf("FIB %d %lld %d %d\n", stream, (long long)f.frame, f.ficno, (int)f.ok);
                total++;
                good += f.ok;
            }
        }
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    if (fails) {
        std::printf("FAILED: %d mismatches\n", fails);
        return 1;
    }
    std::printf("RATE DROPIN OK %ld fibs %ld good\n", total, good);
    return 0;
}
