// ensembleDecoder with config::fic_on_gpu (the FIC layer: dabgpu_pipe_fic, a database per stream on
// the device) against the same decoder with the host's fib_processors, for
// tests/test_gpu_fic_dropin.py: two streams with different layouts from files of cf32 samples,
// auto_layout on the transmitter's FIGs.  Step by step both decoders must hold the same applied
// tables (so they made the same set_subch calls at the same steps) and must have delivered the
// same ensemble and service names for the same frames; at the end database(stream) of the one
// answers serviceLabels and the three lookups as that of the other.
// Prints, for the Python side,
//   TABLE step stream  a:n:br:pl:uep:flags ...    a table the decoders applied, after which step
//   NAME stream frame E|S eid text-in-hex
//   LOOKUP stream label-in-hex kind audio-subch data-subch
// and "FIC DROPIN OK <names> names <tables> tables <lookups> lookups" when everything was equal.
// usage: test_fic_dropin A.f32 B.f32 N_FRAMES STEPS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "dabgpu_dropin.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("MISMATCH: " __VA_ARGS__); std::printf("\n"); fails++; } } while (0)

static std::vector<dabgpu::DSPCOMPLEX> read_iq(const char *path) {
    std::FILE *in = std::fopen(path, "rb");
    if (!in) std::exit(2);
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    std::vector<dabgpu::DSPCOMPLEX> iq((size_t)bytes / sizeof(dabgpu::DSPCOMPLEX));
    if (std::fread(iq.data(), sizeof(dabgpu::DSPCOMPLEX), iq.size(), in) != iq.size()) std::exit(3);
    std::fclose(in);
    return iq;
}

static std::string hex(const std::string &s) {
    std::string h;
    char b[3];
    for (unsigned char c : s) {
        std::snprintf(b, sizeof b, "%02x", c);
        h += b;
    }
    return h;
}

struct side {
    std::unique_ptr<dabgpu::ensembleDecoder> dec;
    std::vector<std::string> names;            // "stream frame E|S eid text-in-hex"
    long msc = 0;
};

static void make(side &x, int n_frames, bool on_gpu) {
    dabgpu::ensembleDecoder::config cfg;
    cfg.n_streams = 2;
    cfg.n_frames = n_frames;
    cfg.auto_layout = true;
    cfg.fic_on_gpu = on_gpu;
    cfg.max_subch = 4;
    cfg.max_bitrate = 96;
    cfg.max_dabplus = 3;
    x.dec.reset(new dabgpu::ensembleDecoder(cfg));
    side *p = &x;
    x.dec->on_ensemble_name([p](int s, int64_t frame, uint32_t eid, const std::string &name) {
        p->names.push_back(std::to_string(s) + " " + std::to_string(frame) + " E " + std::to_string(eid) + " " + hex(name));
    });
    x.dec->on_service_name([p](int s, int64_t frame, const std::string &label) {
        p->names.push_back(std::to_string(s) + " " + std::to_string(frame) + " S 0 " + hex(label));
    });
    x.dec->on_msc([p](int, int64_t, int, const uint8_t *, int) { p->msc++; });
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const std::vector<dabgpu::DSPCOMPLEX> a = read_iq(argv[1]), b = read_iq(argv[2]);
    try {
        side host, gpu;
        make(host, std::atoi(argv[3]), false);
        make(gpu, std::atoi(argv[3]), true);
        for (side *x : {&host, &gpu}) x->dec->load({a.data(), b.data()}, {(int64_t)a.size(), (int64_t)b.size()});
        long ntables = 0, nlookups = 0;
        std::vector<std::vector<dabgpu_subch>> last(2);
        size_t printed = 0;
        for (int step = 0; step < std::atoi(argv[4]); step++) {
            const bool oh = host.dec->step(), og = gpu.dec->step();
            CHECK(oh == og, "step %d: step() returned %d, with the host's parse %d", step, (int)og, (int)oh);
            for (int s = 0; s < 2; s++) {
                const std::vector<dabgpu_subch> th = host.dec->get_subch(s), tg = gpu.dec->get_subch(s);
                CHECK(th.size() == tg.size() && (th.empty() || !std::memcmp(th.data(), tg.data(), th.size() * sizeof(dabgpu_subch))),
                      "step %d stream %d: the applied tables differ (%zu entries, the host's parse %zu)", step, s, tg.size(), th.size());
                if (tg.size() != last[s].size() || (!tg.empty() && std::memcmp(tg.data(), last[s].data(), tg.size() * sizeof(dabgpu_subch)))) {
                    std::printf("TABLE %d %d", step, s);
                    for (const dabgpu_subch &e : tg)
                        std::printf(" %d:%d:%d:%d:%d:%d", e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags);
                    std::printf("\n");
                    last[s] = tg;
                    ntables++;
                }
            }
            CHECK(host.names == gpu.names, "step %d: %zu names, the host's parse %zu", step, gpu.names.size(), host.names.size());
            for (; printed < gpu.names.size(); printed++) std::printf("NAME %s\n", gpu.names[printed].c_str());
        }
        CHECK(host.msc == gpu.msc, "%ld MSC deliveries, with the host's parse %ld", gpu.msc, host.msc);
        for (int s = 0; s < 2; s++) {
            dabgpu::fib_processor dh = host.dec->database(s), dg = gpu.dec->database(s);
            std::vector<std::string> labels = dh.serviceLabels();
            CHECK(labels == dg.serviceLabels(), "stream %d: the service labels differ", s);
            CHECK(dh.ensembleName() == dg.ensembleName(), "stream %d: the ensemble names differ", s);
            labels.push_back("nothing");
            for (const std::string &l : labels) {
                dabgpu::audiodata ah = {}, ag = {};
                dabgpu::packetdata ph = {}, pg = {};
                const int kh = dh.kindofService(l), kg = dg.kindofService(l);
                const bool rah = kh == dabgpu::AUDIO_SERVICE && dh.dataforAudioService(l, &ah);
                const bool rag = kg == dabgpu::AUDIO_SERVICE && dg.dataforAudioService(l, &ag);
                const bool rph = kh == dabgpu::PACKET_SERVICE && dh.dataforDataService(l, &ph);
                const bool rpg = kg == dabgpu::PACKET_SERVICE && dg.dataforDataService(l, &pg);
                CHECK(kh == kg && rah == rag && rph == rpg, "stream %d label %s: kind %d / %d", s, hex(l).c_str(), kg, kh);
                CHECK(ah.subchId == ag.subchId && ah.startAddr == ag.startAddr && ah.uepFlag == ag.uepFlag && ah.protLevel == ag.protLevel &&
                          ah.length == ag.length && ah.bitRate == ag.bitRate && ah.ASCTy == ag.ASCTy && ah.language == ag.language &&
                          ah.programType == ag.programType,
                      "stream %d label %s: dataforAudioService", s, hex(l).c_str());
                CHECK(ph.subchId == pg.subchId && ph.startAddr == pg.startAddr && ph.uepFlag == pg.uepFlag && ph.protLevel == pg.protLevel &&
                          ph.DSCTy == pg.DSCTy && ph.length == pg.length && ph.bitRate == pg.bitRate && ph.FEC_scheme == pg.FEC_scheme &&
                          ph.DGflag == pg.DGflag && ph.packetAddress == pg.packetAddress,
                      "stream %d label %s: dataforDataService", s, hex(l).c_str());
                std::printf("LOOKUP %d %s %d %d %d\n", s, hex(l).c_str(), kg, rag ? ag.subchId : -1, rpg ? pg.subchId : -1);
                nlookups++;
            }
        }
        if (fails) {
            std::printf("FAILED: %d mismatches\n", fails);
            return 1;
        }
        std::printf("FIC DROPIN OK %zu names %ld tables %ld lookups\n", gpu.names.size(), ntables, nlookups);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
