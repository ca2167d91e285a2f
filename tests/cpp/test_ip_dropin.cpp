// ensembleDecoder::on_datagram and on_ip_quality driven from a file of cf32 samples (one stream)
// with auto_layout, for tests/test_gpu_ip_dropin.py: every datagram and show_ipErrors value the
// GPU's IP layer delivers against the host ipAssembler (msc_consumers) fed, per table entry, the
// groups on_datagroup delivered in the same step -- the bytes, the order, the group's CIF.
// Prints, for the Python side,
//   TABLE step n  a:n:br:pl:uep:flags ...     the table the decoder applied, after which step
//   DGRAM subch cif nbytes bytes-in-hex
//   QUALITY subch value
// and "IP DROPIN OK <datagrams> datagrams <groups> groups" when everything was equal.
// usage: test_ip_dropin IQ.f32 N_FRAMES STEPS [gpu]     gpu: the FIBs are parsed on the GPU (config::fic_on_gpu)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>
#include "dabgpu_dropin.h"

struct event {
    int64_t cif;            // -1: a show_ipErrors value
    int value;
    std::vector<uint8_t> bytes;
};

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("MISMATCH: " __VA_ARGS__); std::printf("\n"); fails++; } } while (0)

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    std::vector<dabgpu::DSPCOMPLEX> iq((size_t)bytes / sizeof(dabgpu::DSPCOMPLEX));
    if (std::fread(iq.data(), sizeof(dabgpu::DSPCOMPLEX), iq.size(), in) != iq.size()) return 3;
    std::fclose(in);
    try {
        dabgpu::ensembleDecoder::config cfg;
        cfg.n_streams = 1;
        cfg.n_frames = std::atoi(argv[2]);
        cfg.auto_layout = true;
        cfg.fic_on_gpu = argc == 5 && !std::strcmp(argv[4], "gpu");
        cfg.max_subch = 5;
        cfg.max_bitrate = 128;
        cfg.max_dabplus = 1;
        cfg.max_packet = 3;
        dabgpu::ensembleDecoder dec(cfg);
        std::map<int, std::unique_ptr<dabgpu::ipAssembler>> host;       // [table entry]
        std::map<int, std::vector<event>> want, got;
        int64_t cif_now = 0;
        long ngroups = 0, ndatagrams = 0;
        dec.on_datagroup([&](int stream, int64_t cif, int subch, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
            if (stream != 0) std::abort();
            ngroups++;
            if (g.flags & DABGPU_DG_TRUNCATED) return;               // not what the transmitter sent: never accepted
            if (!host.count(subch))
                host[subch].reset(new dabgpu::ipAssembler(
                    [&want, &cif_now, subch](const uint8_t *p, int32_t n) { want[subch].push_back({cif_now, n, std::vector<uint8_t>(p, p + n)}); },
                    [&want, subch](int v) { want[subch].push_back({-1, v, {}}); }));
            cif_now = cif;
            host[subch]->add_group(b, nbytes);
        });
        dec.on_datagram([&](int stream, int subch, int64_t cif, const uint8_t *p, int n) {
            if (stream != 0) std::abort();
            got[subch].push_back({cif, n, std::vector<uint8_t>(p, p + n)});
        });
        dec.on_ip_quality([&](int stream, int subch, int v) {
            if (stream != 0) std::abort();
            got[subch].push_back({-1, v, {}});
        });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        bool applied = false;
        for (int s = 0; s < std::atoi(argv[3]); s++) {
            dec.step();
            const std::vector<dabgpu_subch> t = dec.get_subch(0);
            // the step's events, per entry flagged for the layer, in order
            for (auto &kv : want) {
                const int k = kv.first;
                if (k >= (int)t.size() || !(t[(size_t)k].flags & DABGPU_SUBCH_IP)) {
                    kv.second.clear();                               // (a DSCTy 60 entry: the host handler above is not the reference's)
                    continue;
                }
                std::vector<event> &g = got[k];
                CHECK(g.size() == kv.second.size(), "step %d entry %d: %zu events, the host assembler %zu", s, k, g.size(), kv.second.size());
                for (size_t i = 0; i < g.size() && i < kv.second.size(); i++) {
                    const event &w = kv.second[i];
                    CHECK(g[i].cif == w.cif && g[i].value == w.value && g[i].bytes == w.bytes, "step %d entry %d event %zu: cif %lld value %d for %lld %d",
                          s, k, i, (long long)g[i].cif, g[i].value, (long long)w.cif, w.value);
                    if (g[i].cif < 0) {
                        std::printf("QUALITY %d %d\n", k, g[i].value);
                        continue;
                    }
                    std::printf("DGRAM %d %lld %d ", k, (long long)g[i].cif, g[i].value);
                    for (uint8_t c : g[i].bytes) std::printf("%02x", c);
                    std::printf("\n");
                    ndatagrams++;
                }
                kv.second.clear();
                g.clear();
            }
            for (auto &kv : got)
                CHECK(kv.second.empty(), "step %d entry %d: %zu events the host assembler did not deliver", s, kv.first, kv.second.size());
            if (!applied && !t.empty()) {
                std::printf("TABLE %d %zu", s, t.size());
                for (const dabgpu_subch &e : t)
                    std::printf(" %d:%d:%d:%d:%d:%d", e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags);
                std::printf("\n");
                applied = true;
            }
        }
        if (fails) {
            std::printf("FAILED: %d mismatches\n", fails);
            return 1;
        }
        std::printf("IP DROPIN OK %ld datagrams %ld groups\n", ndatagrams, ngroups);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
