// ensembleDecoder::on_dynamic_label / on_pad_datagroup / on_pad_object driven from a file of cf32
// samples (one stream) with auto_layout, for tests/test_gpu_pad_dropin.py: every label, X-PAD
// data group and slide the GPU's PAD layer (and dabgpu_mot_groups behind it) delivers against
// the host padAssembler + motAssembler (msc_consumers) fed, per table entry, the AUs of the
// superframes on_superframe delivered in the same step, as mp4Processor hands them on.
// Prints, for the Python side,
//   TABLE step n  a:n:br:pl:uep:flags ...     the table the decoder applied, after which step
//   LABEL subch cif charset text-in-hex
//   OBJ subch cif transportId kind nbytes name-in-hex
// Then the one-stream mp4Processor drop-in with its optional PAD hook over the MSC bits on_msc
// delivered for the first DAB+ entry: the labels a padAssembler behind the hook shows are those
// of the decoder ("HOOK n labels").
// and "PAD DROPIN OK <labels> labels <groups> groups <objects> objects" when everything was equal.
// usage: test_pad_dropin IQ.f32 N_FRAMES STEPS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>
#include "dabgpu_dropin.h"

using dabgpu::motAssembler;
using dabgpu::padAssembler;

struct host_side {
    std::unique_ptr<padAssembler> pad;
    std::unique_ptr<motAssembler> mot;
    std::vector<std::pair<int64_t, padAssembler::label>> labels;
    std::vector<std::pair<int64_t, padAssembler::datagroup>> groups;
    std::vector<std::pair<int64_t, motAssembler::object>> objects;
    int64_t cif = 0;
};
struct gpu_side {
    std::vector<std::pair<int64_t, dabgpu_pad_label>> labels;
    std::vector<std::pair<dabgpu_datagroup, std::vector<uint8_t>>> groups;
    std::vector<int64_t> group_cif;
    std::vector<std::pair<int64_t, dabgpu_mot_object>> objects;
    std::vector<std::vector<uint8_t>> bodies;
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
        cfg.max_subch = 4;
        cfg.max_bitrate = 64;
        cfg.max_dabplus = 2;
        cfg.max_pad = 2;
        dabgpu::ensembleDecoder dec(cfg);
        std::map<int, host_side> host;      // [table entry]
        std::map<int, gpu_side> gpu;
        long nlabels = 0, ngroups = 0, nobjects = 0;
        std::vector<std::vector<uint8_t>> cifs0;                     // entry 0's CIFs, one bit per byte
        std::vector<std::vector<uint8_t>> texts0;                    // the labels the decoder delivered for it
        dec.on_msc([&](int, int64_t, int subch, const uint8_t *bits, int nbits) {
            if (subch == 0) cifs0.push_back(std::vector<uint8_t>(bits, bits + nbits));
        });
        auto host_of = [&](int subch) -> host_side & {
            host_side &h = host[subch];
            if (!h.pad) {
                host_side *hp = &h;         // (map nodes stay where they are)
                h.mot.reset(new motAssembler([hp](const motAssembler::object &o) { hp->objects.push_back({hp->cif, o}); }));
                h.pad.reset(new padAssembler([hp](const padAssembler::label &l) { hp->labels.push_back({hp->cif, l}); },
                                             [hp](const padAssembler::datagroup &g) {
                                                 hp->groups.push_back({hp->cif, g});
                                                 // build_MSC_segment's call (pad-handler.cpp:352-356)
                                                 if (g.accepted)
                                                     hp->mot->process_mscGroup(g.data.data(), (int32_t)g.data.size(), g.groupType, g.last,
                                                                               g.segmentNumber, g.transportId);
                                             }));
            }
            return h;
        };
        dec.on_superframe([&](int stream, int64_t cif, int subch, const dabgpu_superframe &i, const uint8_t *b, int nbytes) {
            if (stream != 0) std::abort();
            if (i.status != 3) return;
            host_side &h = host_of(subch);
            h.cif = cif;
            for (int a = 0; a < i.num_aus; a++) {
                const int a0 = i.au_start[a], len = i.au_start[a + 1] - a0 - 2;
                if (!((i.au_crc_ok >> a) & 1) || len < 0 || a0 + len > nbytes) continue;
                h.pad->processAU(b + a0, len, len);
            }
        });
        dec.on_dynamic_label([&](int stream, int64_t cif, int subch, const dabgpu_pad_label &l) {
            if (stream != 0) std::abort();
            gpu[subch].labels.push_back({cif, l});
        });
        dec.on_pad_datagroup([&](int stream, int64_t cif, int subch, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
            if (stream != 0) std::abort();
            gpu[subch].groups.push_back({g, std::vector<uint8_t>(b, b + nbytes)});
            gpu[subch].group_cif.push_back(cif);
        });
        dec.on_pad_object([&](int stream, int64_t cif, int subch, const dabgpu_mot_object &o, const uint8_t *body) {
            if (stream != 0) std::abort();
            gpu[subch].objects.push_back({cif, o});
            gpu[subch].bodies.push_back(std::vector<uint8_t>(body, body + o.nbytes));
        });
        dec.load({iq.data()}, {(int64_t)iq.size()});
        bool applied = false;
        for (int s = 0; s < std::atoi(argv[3]); s++) {
            dec.step();
            for (auto &kv : host) {
                const int k = kv.first;
                host_side &h = kv.second;
                gpu_side &g = gpu[k];
                CHECK(g.labels.size() == h.labels.size(), "step %d entry %d: %zu labels, the host %zu", s, k, g.labels.size(), h.labels.size());
                for (size_t i = 0; i < g.labels.size() && i < h.labels.size(); i++) {
                    const dabgpu_pad_label &r = g.labels[i].second;
                    const padAssembler::label &w = h.labels[i].second;
                    CHECK(g.labels[i].first == h.labels[i].first, "step %d entry %d label %zu: cif %lld for %lld", s, k, i,
                          (long long)g.labels[i].first, (long long)h.labels[i].first);
                    CHECK(r.charset == w.charset && r.nbytes == w.nbytes && r.n_pieces == w.n_pieces &&
                              (r.flags & DABGPU_PAD_LABEL_TRUNCATED ? 1 : 0) == (int)w.truncated,
                          "step %d entry %d label %zu: record", s, k, i);
                    CHECK(!std::memcmp(r.text, w.text.data(), w.text.size()) && !std::memcmp(r.piece_len, w.piece_len.data(), w.piece_len.size()),
                          "step %d entry %d label %zu: text or pieces", s, k, i);
                    if (k == 0) texts0.push_back(std::vector<uint8_t>(r.text, r.text + std::min(r.nbytes, DABGPU_PAD_LABEL_BYTES)));
                    std::printf("LABEL %d %lld %d ", k, (long long)g.labels[i].first, r.charset);
                    for (int c = 0; c < std::min(r.nbytes, DABGPU_PAD_LABEL_BYTES); c++) std::printf("%02x", r.text[c]);
                    std::printf("\n");
                    nlabels++;
                }
                CHECK(g.groups.size() == h.groups.size(), "step %d entry %d: %zu groups, the host %zu", s, k, g.groups.size(), h.groups.size());
                for (size_t i = 0; i < g.groups.size() && i < h.groups.size(); i++) {
                    const dabgpu_datagroup &r = g.groups[i].first;
                    const padAssembler::datagroup &w = h.groups[i].second;
                    CHECK(g.group_cif[i] == h.groups[i].first, "step %d entry %d group %zu: cif", s, k, i);
                    CHECK(((r.flags & DABGPU_DG_ACCEPTED) != 0) == w.accepted && r.nbytes == (int32_t)w.bytes.size() &&
                              r.data_offset == w.data_offset && r.data_nbytes == w.data_nbytes && r.groupType == w.groupType &&
                              r.segmentNumber == w.segmentNumber && r.transportId == w.transportId,
                          "step %d entry %d group %zu: record", s, k, i);
                    CHECK(g.groups[i].second == w.bytes, "step %d entry %d group %zu: bytes", s, k, i);
                    ngroups++;
                }
                CHECK(g.objects.size() == h.objects.size(), "step %d entry %d: %zu objects, the host %zu", s, k, g.objects.size(),
                      h.objects.size());
                for (size_t i = 0; i < g.objects.size() && i < h.objects.size(); i++) {
                    const dabgpu_mot_object &r = g.objects[i].second;
                    const motAssembler::object &w = h.objects[i].second;
                    const size_t nl = std::min<size_t>(w.name.size(), DABGPU_MOT_NAME_BYTES);
                    CHECK(g.objects[i].first == h.objects[i].first, "step %d entry %d object %zu: cif", s, k, i);
                    CHECK(r.kind == w.kind && r.transportId == w.transportId && r.contentType == w.contentType && r.flags == 0 &&
                              r.name_len == (int32_t)w.name.size() && !std::memcmp(r.name, w.name.data(), nl),
                          "step %d entry %d object %zu: record", s, k, i);
                    CHECK(g.bodies[i] == w.body, "step %d entry %d object %zu: body", s, k, i);
                    std::printf("OBJ %d %lld %d %d %d ", k, (long long)g.objects[i].first, r.transportId, r.kind, r.nbytes);
                    for (size_t c = 0; c < nl; c++) std::printf("%02x", r.name[c]);
                    std::printf("\n");
                    nobjects++;
                }
                h.labels.clear();
                h.groups.clear();
                h.objects.clear();
                g = gpu_side();
            }
            for (auto &kv : gpu)
                CHECK(kv.second.labels.empty() && kv.second.groups.empty() && kv.second.objects.empty(),
                      "step %d entry %d: deliveries the host side did not make", s, kv.first);
            const std::vector<dabgpu_subch> t = dec.get_subch(0);
            if (!applied && !t.empty()) {
                std::printf("TABLE %d %zu", s, t.size());
                for (const dabgpu_subch &e : t)
                    std::printf(" %d:%d:%d:%d:%d:%d", e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags);
                std::printf("\n");
                applied = true;
            }
        }
        {
            std::vector<std::vector<uint8_t>> hooked;
            padAssembler pa([&](const padAssembler::label &l) { hooked.push_back(l.text); }, nullptr);
            int calls = 0;
            dabgpu::mp4Processor plain(32, nullptr), proc(32, nullptr);
            proc.set_pad_hook([&](const uint8_t *theAU, int16_t len) {
                calls++;
                pa.processAU(theAU, 2 * 960, len);
            });
            for (auto &c : cifs0) {
                proc.addtoFrame(c.data(), (int16_t)c.size());
                plain.addtoFrame(c.data(), (int16_t)c.size());       // without a hook: as before
            }
            CHECK(hooked == texts0 && !texts0.empty(), "the PAD hook: %zu labels for the decoder's %zu", hooked.size(), texts0.size());
            CHECK(calls > 0 && plain.superframes() == proc.superframes() && plain.frameErrors() == proc.frameErrors(),
                  "the PAD hook: %d calls, %d superframes for %d", calls, proc.superframes(), plain.superframes());
            std::printf("HOOK %zu labels %d calls\n", hooked.size(), calls);
        }
        if (fails) {
            std::printf("FAILED: %d mismatches\n", fails);
            return 1;
        }
        std::printf("PAD DROPIN OK %ld labels %ld groups %ld objects\n", nlabels, ngroups, nobjects);
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
