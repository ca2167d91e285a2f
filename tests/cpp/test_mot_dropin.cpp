// ensembleDecoder::on_mot_object driven from a file of cf32 samples (one stream) with
// auto_layout, for tests/test_gpu_mot_dropin.py: every object the GPU's MOT layer delivers
// against the host motAssembler (msc_consumers) fed, per table entry, the groups on_datagroup
// delivered in the same step -- record fields, name, body and the completing group's CIF.
// Prints, for the Python side,
//   TABLE step n  a:n:br:pl:uep:flags ...     the table the decoder applied, after which step
//   OBJ subch cif transportId kind nbytes name-in-hex
// and "MOT DROPIN OK <objects> objects <groups> groups" when everything was equal.
// usage: test_mot_dropin IQ.f32 N_FRAMES STEPS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>
#include "dabgpu_dropin.h"

struct host_object {
    int64_t cif;
    dabgpu::motAssembler::object o;
};

struct gpu_object {
    int64_t cif;
    dabgpu_mot_object rec;
    std::vector<uint8_t> body;
};

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("MISMATCH: " __VA_ARGS__); std::printf("\n"); fails++; } } while (0)

int main(int argc, char **argv) {
    if (argc != 4) return 2;
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
        cfg.max_subch = 5;
        cfg.max_bitrate = 128;
        cfg.max_dabplus = 1;
        cfg.max_packet = 3;
        cfg.max_mot = 3;
        dabgpu::ensembleDecoder dec(cfg);
        std::map<int, std::unique_ptr<dabgpu::motAssembler>> host;      // [table entry]
        std::map<int, std::vector<host_object>> want;
        std::map<int, std::vector<gpu_object>> got;
        int64_t cif_now = 0;
        long ngroups = 0, nobjects = 0;
        dec.on_datagroup([&](int stream, int64_t cif, int subch, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
            if (stream != 0) std::abort();
            ngroups++;
            if (g.flags & DABGPU_DG_TRUNCATED) return;               // not what the transmitter sent: never accepted
            if (!host.count(subch))
                host[subch].reset(new dabgpu::motAssembler([&want, &cif_now, subch](const dabgpu::motAssembler::object &o) {
                    want[subch].push_back({cif_now, o});
                }));
            std::vector<uint8_t> bits((size_t)nbytes * 8);           // as packetAssembler delivers it
            for (size_t i = 0; i < bits.size(); i++) bits[i] = (uint8_t)((b[i >> 3] >> (7 - (i & 7))) & 1);
            cif_now = cif;
            host[subch]->add_mscDatagroup(bits);
        });
        dec.on_mot_object([&](int stream, int64_t cif, int subch, const dabgpu_mot_object &o, const uint8_t *body) {
            if (stream != 0) std::abort();
            got[subch].push_back({cif, o, std::vector<uint8_t>(body, body + o.nbytes)});
        });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        bool applied = false;
        for (int s = 0; s < std::atoi(argv[3]); s++) {
            dec.step();
            // the step's objects, per entry in completion order
            for (auto &kv : want) {
                const int k = kv.first;
                std::vector<gpu_object> &g = got[k];
                CHECK(g.size() == kv.second.size(), "step %d entry %d: %zu objects, the host assembler %zu", s, k, g.size(),
                      kv.second.size());
                for (size_t i = 0; i < g.size() && i < kv.second.size(); i++) {
                    const dabgpu::motAssembler::object &w = kv.second[i].o;
                    const dabgpu_mot_object &r = g[i].rec;
                    const size_t nl = std::min<size_t>(w.name.size(), DABGPU_MOT_NAME_BYTES);
                    CHECK(g[i].cif == kv.second[i].cif, "step %d entry %d object %zu: cif %lld for %lld", s, k, i,
                          (long long)g[i].cif, (long long)kv.second[i].cif);
                    CHECK(r.kind == w.kind && r.transportId == w.transportId && r.contentType == w.contentType &&
                              r.contentsubType == w.contentsubType && r.flags == 0,
                          "step %d entry %d object %zu: record (kind %d tid %d flags %d)", s, k, i, r.kind, r.transportId, r.flags);
                    CHECK(r.name_len == (int32_t)w.name.size() && !std::memcmp(r.name, w.name.data(), nl),
                          "step %d entry %d object %zu: name", s, k, i);
                    CHECK(g[i].body.size() == w.body.size() && (w.body.empty() || !std::memcmp(g[i].body.data(), w.body.data(), w.body.size())),
                          "step %d entry %d object %zu: body (%zu bytes for %zu)", s, k, i, g[i].body.size(), w.body.size());
                    std::printf("OBJ %d %lld %d %d %d ", k, (long long)g[i].cif, r.transportId, r.kind, r.nbytes);
                    for (size_t c = 0; c < nl; c++) std::printf("%02x", r.name[c]);
                    std::printf("\n");
                    nobjects++;
                }
                kv.second.clear();
                g.clear();
            }
            for (auto &kv : got)
                CHECK(kv.second.empty(), "step %d entry %d: %zu objects the host assembler did not deliver", s, kv.first, kv.second.size());
            const std::vector<dabgpu_subch> t = dec.get_subch(0);
            if (!applied && !t.empty()) {
                std::printf("TABLE %d %zu", s, t.size());
                for (const dabgpu_subch &e : t)
                    std::printf(" %d:%d:%d:%d:%d:%d", e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags);
                std::printf("\n");
                applied = true;
            }
        }
        for (auto &kv : host)
            std::printf("HOST %d objects %d malformed %d bad %d other %d\n", kv.first, kv.second->objects(), kv.second->malformed(),
                        kv.second->badSegments(), kv.second->otherTypes());
        if (fails) {
            std::printf("FAILED: %d mismatches\n", fails);
            return 1;
        }
        std::printf("MOT DROPIN OK %ld objects %ld groups\n", nobjects, ngroups);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
