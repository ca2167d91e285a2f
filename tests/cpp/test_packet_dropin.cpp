// ensembleDecoder::on_datagroup / on_packet_quality driven from a file of cf32 samples (one
// stream) with auto_layout, for tests/test_gpu_packet.py.  Records written, each headed by
//   int32 kind, int32 subch, int64 cif, int32 value, int32 nbytes
// kind 0: a data group, followed by its dabgpu_datagroup and its nbytes bytes;
// kind 1: a show_mscErrors value;
// kind 2: the stream's table was applied at the end of step `value`: nbytes entries of six
//         int16 follow.
// usage: test_packet_dropin IQ.f32 OUT.bin N_FRAMES STEPS
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dabgpu_dropin.h"

struct head {
    int32_t kind, subch;
    int64_t cif;
    int32_t value, nbytes;
};

int main(int argc, char **argv) {
    if (argc != 5) return 2;
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
        cfg.auto_layout = true;
        cfg.max_subch = 5;
        cfg.max_bitrate = 128;
        cfg.max_dabplus = 1;
        cfg.max_packet = 3;
        dabgpu::ensembleDecoder dec(cfg);
        long n = 0;
        dec.on_datagroup([&](int stream, int64_t cif, int subch, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
            const head h = {0, subch, cif, 0, nbytes};
            if (stream != 0) std::abort();
            std::fwrite(&h, sizeof h, 1, out);
            std::fwrite(&g, sizeof g, 1, out);
            std::fwrite(b, 1, (size_t)nbytes, out);
            n++;
        });
        dec.on_packet_quality([&](int stream, int64_t cif, int subch, int value) {
            const head h = {1, subch, cif, value, 0};
            if (stream != 0) std::abort();
            std::fwrite(&h, sizeof h, 1, out);
        });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        bool applied = false;
        for (int s = 0; s < std::atoi(argv[4]); s++) {
            dec.step();
            const std::vector<dabgpu_subch> t = dec.get_subch(0);
            if (!applied && !t.empty()) {
                const head h = {2, 0, 0, s, (int32_t)t.size()};
                std::fwrite(&h, sizeof h, 1, out);
                std::fwrite(t.data(), sizeof(dabgpu_subch), t.size(), out);
                applied = true;
            }
        }
        std::fclose(out);
        std::printf("PACKET DROPIN OK %ld groups\n", n);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
