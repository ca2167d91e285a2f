// ensembleDecoder with two streams of different layouts and every callback set, for
// tests/test_gpu_streams_dropin.py: the element index (stream * slots + slot) of the packet, MOT,
// IP, PAD, layer II and audio layers at stream index 1.  Signal A carries a MOT, an IP and a layer II
// entry, signal B two DAB+ entries (one with PAD) and a layer II entry.  Four decoders of one config
// (auto_layout, every callback): A alone, B alone, the pair (A, B) and the pair (B, A).  Every
// callback appends one line to its stream's log: its name, the CIF or frame, the entry, the record's
// fields and a hash of the bytes it was handed (no step index).  What holds:
//   - in both pairs each stream's log is the log of that signal decoded alone, line for line;
//   - within a step and stream on_audio comes after the on_pcm calls, on_mot_object and on_datagram
//     after the on_datagroup calls, and the on_ip_quality / on_datagram sequence is the one a host
//     ipAssembler gives for the step's groups (a group's quality before its datagram);
//   - every kind of callback occurs on the stream that carries it.
// Prints "COUNT signal kind n" per kind, "STEP i ms applied" for each step of the (A, B) decoder
// (wall time of step(); applied: both tables were in force when it began), "MEDIAN_MS x" over the
// applied steps, and "STREAMS DROPIN OK" when everything held.
// usage: test_streams_dropin A.f32 B.f32 N_FRAMES STEPS [gpu]     gpu: config::fic_on_gpu
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "dabgpu_dropin.h"

typedef std::vector<dabgpu::DSPCOMPLEX> signal;
typedef std::vector<std::string> log_t;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 40) { std::printf("MISMATCH: " __VA_ARGS__); std::printf("\n"); } fails++; } } while (0)

static unsigned long long fnv(const void *p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
    return h;
}

static std::string line(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

static bool read_signal(const char *path, signal &iq) {
    std::FILE *in = std::fopen(path, "rb");
    if (!in) return false;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    iq.resize((size_t)bytes / sizeof(dabgpu::DSPCOMPLEX));
    const bool ok = std::fread(iq.data(), sizeof(dabgpu::DSPCOMPLEX), iq.size(), in) == iq.size();
    std::fclose(in);
    return ok;
}

struct ip_event {
    int64_t cif;            // -1: a show_ipErrors value
    int value;
    unsigned long long hash;
    bool operator==(const ip_event &o) const { return cif == o.cif && value == o.value && hash == o.hash; }
};

// the state the order checks keep per stream, cleared after every step
struct step_order {
    bool audio = false, after_groups = false;
    std::map<int, std::unique_ptr<dabgpu::ipAssembler>> host;   // [table entry], fed the entry's groups (kept over the steps)
    std::map<int, std::vector<ip_event>> want, got;
    int64_t cif_now = 0;
};

// one decoder over the given signals: the per-stream logs; step_ms (optional): wall time per step and
// whether every stream's table was in force when it began
static std::vector<log_t> decode(const std::vector<const signal *> &sig, int n_frames, int steps, bool fic_on_gpu, const char *what,
                                 std::vector<std::pair<double, bool>> *step_ms) {
    const int S = (int)sig.size();
    dabgpu::ensembleDecoder::config cfg;
    cfg.n_streams = S;
    cfg.n_frames = n_frames;
    cfg.auto_layout = true;
    cfg.fic_on_gpu = fic_on_gpu;
    cfg.max_subch = 4;
    cfg.max_bitrate = 128;
    cfg.max_dabplus = 2;
    cfg.max_mp2 = 1;
    cfg.max_audio = 1;
    cfg.max_packet = 2;
    cfg.max_mot = 2;
    cfg.max_pad = 2;
    dabgpu::ensembleDecoder dec(cfg);
    std::vector<log_t> log((size_t)S);
    std::vector<step_order> ord((size_t)S);
    auto bad = [&](int s) { return s < 0 || s >= S; };
    dec.on_fib([&](int s, int64_t frame, int ficno, const uint8_t *bits, bool ok) {
        if (bad(s)) std::abort();
        log[s].push_back(line("fib %lld %d %d %016llx", (long long)frame, ficno, (int)ok, fnv(bits, 256)));
    });
    dec.on_msc([&](int s, int64_t cif, int k, const uint8_t *bits, int nbits) {
        if (bad(s)) std::abort();
        log[s].push_back(line("msc %lld %d %d %016llx", (long long)cif, k, nbits, fnv(bits, (size_t)nbits)));
    });
    dec.on_superframe([&](int s, int64_t cif, int k, const dabgpu_superframe &i, const uint8_t *b, int nbytes) {
        if (bad(s)) std::abort();
        log[s].push_back(line("superframe %lld %d %d %d %d %d %d %016llx %016llx", (long long)cif, k, i.status, i.num_aus, i.n_corrected, i.au_crc_ok,
                              nbytes, fnv(i.au_start, sizeof i.au_start), fnv(b, (size_t)nbytes)));
    });
    dec.on_ensemble_name([&](int s, int64_t frame, uint32_t EId, const std::string &name) {
        if (bad(s)) std::abort();
        log[s].push_back(line("ensemble_name %lld %u %016llx", (long long)frame, EId, fnv(name.data(), name.size())));
    });
    dec.on_service_name([&](int s, int64_t frame, const std::string &label) {
        if (bad(s)) std::abort();
        log[s].push_back(line("service_name %lld %016llx", (long long)frame, fnv(label.data(), label.size())));
    });
    dec.on_pcm([&](int s, int64_t cif, int k, const int16_t *pcm, int n, int rate) {
        if (bad(s)) std::abort();
        CHECK(!ord[s].audio, "%s stream %d: on_pcm (cif %lld) after an on_audio of the step", what, s, (long long)cif);
        log[s].push_back(line("pcm %lld %d %d %d %016llx", (long long)cif, k, n, rate, fnv(pcm, (size_t)n * 2 * sizeof(int16_t))));
    });
    dec.on_audio([&](int s, int64_t cif, int k, const float *samples, int n_pairs) {
        if (bad(s)) std::abort();
        ord[s].audio = true;
        log[s].push_back(line("audio %lld %d %d %016llx", (long long)cif, k, n_pairs, fnv(samples, (size_t)n_pairs * 2 * sizeof(float))));
    });
    dec.on_datagroup([&](int s, int64_t cif, int k, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
        if (bad(s)) std::abort();
        step_order &o = ord[s];
        CHECK(!o.after_groups, "%s stream %d: on_datagroup (cif %lld) after an on_mot_object or on_datagram of the step", what, s, (long long)cif);
        log[s].push_back(line("datagroup %lld %d %d %d %d %d %d %u %u %u %u %u %u %016llx", (long long)cif, k, g.cif, g.offset, g.nbytes, g.data_offset,
                              g.data_nbytes, g.flags, g.segmentNumber, g.transportId, g.groupType, g.CI, g.lengthInd, fnv(b, (size_t)nbytes)));
        if (g.flags & DABGPU_DG_TRUNCATED) return;                   // never accepted: not for the host assembler
        if (!o.host.count(k)) {
            step_order *op = &o;
            o.host[k].reset(new dabgpu::ipAssembler(
                [op, k](const uint8_t *p, int32_t n) { op->want[k].push_back({op->cif_now, n, fnv(p, (size_t)n)}); },
                [op, k](int v) { op->want[k].push_back({-1, v, 0}); }));
        }
        o.cif_now = cif;
        o.host[k]->add_group(b, nbytes);
    });
    dec.on_packet_quality([&](int s, int64_t cif, int k, int value) {
        if (bad(s)) std::abort();
        log[s].push_back(line("packet_quality %lld %d %d", (long long)cif, k, value));
    });
    dec.on_mot_object([&](int s, int64_t cif, int k, const dabgpu_mot_object &o, const uint8_t *body) {
        if (bad(s)) std::abort();
        ord[s].after_groups = true;
        log[s].push_back(line("mot_object %lld %d %d %d %d %d %u %u %u %u %u %d %016llx %016llx", (long long)cif, k, o.group, o.cif, o.offset, o.nbytes,
                              o.transportId, o.contentType, o.kind, o.contentsubType, o.flags, o.name_len,
                              fnv(o.name, (size_t)std::min(o.name_len, DABGPU_MOT_NAME_BYTES)), fnv(body, (size_t)o.nbytes)));
    });
    dec.on_datagram([&](int s, int k, int64_t cif, const uint8_t *p, int n) {
        if (bad(s)) std::abort();
        ord[s].after_groups = true;
        ord[s].got[k].push_back({cif, n, fnv(p, (size_t)n)});
        log[s].push_back(line("datagram %lld %d %d %016llx", (long long)cif, k, n, fnv(p, (size_t)n)));
    });
    dec.on_ip_quality([&](int s, int k, int value) {
        if (bad(s)) std::abort();
        ord[s].got[k].push_back({-1, value, 0});
        log[s].push_back(line("ip_quality %d %d", k, value));
    });
    dec.on_dynamic_label([&](int s, int64_t cif, int k, const dabgpu_pad_label &l) {
        if (bad(s)) std::abort();
        log[s].push_back(line("dynamic_label %lld %d %d %d %d %d %d %d %016llx %016llx", (long long)cif, k, l.cif, l.au, l.charset, l.nbytes, l.n_pieces,
                              l.flags, fnv(l.piece_len, (size_t)std::min(l.n_pieces, DABGPU_PAD_LABEL_PIECES)),
                              fnv(l.text, (size_t)std::min(l.nbytes, DABGPU_PAD_LABEL_BYTES))));
    });
    dec.on_pad_datagroup([&](int s, int64_t cif, int k, const dabgpu_datagroup &g, const uint8_t *b, int nbytes) {
        if (bad(s)) std::abort();
        log[s].push_back(line("pad_datagroup %lld %d %d %d %d %d %d %u %u %u %u %u %u %016llx", (long long)cif, k, g.cif, g.offset, g.nbytes, g.data_offset,
                              g.data_nbytes, g.flags, g.segmentNumber, g.transportId, g.groupType, g.CI, g.lengthInd, fnv(b, (size_t)nbytes)));
    });
    dec.on_pad_object([&](int s, int64_t cif, int k, const dabgpu_mot_object &o, const uint8_t *body) {
        if (bad(s)) std::abort();
        log[s].push_back(line("pad_object %lld %d %d %d %d %d %u %u %u %u %u %d %016llx %016llx", (long long)cif, k, o.group, o.cif, o.offset, o.nbytes,
                              o.transportId, o.contentType, o.kind, o.contentsubType, o.flags, o.name_len,
                              fnv(o.name, (size_t)std::min(o.name_len, DABGPU_MOT_NAME_BYTES)), fnv(body, (size_t)o.nbytes)));
    });
    std::vector<const dabgpu::DSPCOMPLEX *> ptr;
    std::vector<int64_t> n;
    for (const signal *v : sig) {
        ptr.push_back(v->data());
        n.push_back((int64_t)v->size());
    }
    dec.load(ptr, n);
    for (int i = 0; i < steps; i++) {
        bool applied = true;
        for (int s = 0; s < S; s++) applied = applied && !dec.get_subch(s).empty();
        const auto t0 = std::chrono::steady_clock::now();
        dec.step();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (step_ms) step_ms->push_back({ms, applied});
        for (int s = 0; s < S; s++) {
            step_order &o = ord[s];
            const std::vector<dabgpu_subch> t = dec.get_subch(s);
            for (auto &kv : o.want) {
                const int k = kv.first;
                // (a DSCTy 60 entry's groups: the host handler above is not the reference's for them)
                if (k < (int)t.size() && (t[(size_t)k].flags & DABGPU_SUBCH_IP))
                    CHECK(o.got[k] == kv.second, "%s stream %d step %d entry %d: %zu IP events, not the host assembler's %zu in its order", what, s, i, k,
                          o.got[k].size(), kv.second.size());
                kv.second.clear();
                o.got[k].clear();
            }
            for (auto &kv : o.got) CHECK(kv.second.empty(), "%s stream %d step %d entry %d: IP events without a group", what, s, i, kv.first);
            o.audio = o.after_groups = false;
        }
    }
    return log;
}

static void same_log(const log_t &pair, const log_t &solo, const char *what) {
    CHECK(pair.size() == solo.size(), "%s: %zu lines, alone %zu", what, pair.size(), solo.size());
    for (size_t i = 0; i < pair.size() && i < solo.size(); i++)
        if (pair[i] != solo[i]) {
            CHECK(false, "%s line %zu: '%s', alone '%s'", what, i, pair[i].c_str(), solo[i].c_str());
            break;
        }
}

static void counts(const log_t &log, const char *signal_name, const std::vector<const char *> &kinds) {
    std::map<std::string, long> n;
    for (const std::string &l : log) n[l.substr(0, l.find(' '))]++;
    for (const char *k : kinds) {
        std::printf("COUNT %s %s %ld\n", signal_name, k, n[k]);
        CHECK(n[k] > 0, "signal %s: no on_%s call", signal_name, k);
    }
}

int main(int argc, char **argv) {
    if (argc != 5 && argc != 6) return 2;
    signal a, b;
    if (!read_signal(argv[1], a) || !read_signal(argv[2], b)) return 3;
    const int F = std::atoi(argv[3]), steps = std::atoi(argv[4]);
    const bool gpu = argc == 6 && !std::strcmp(argv[5], "gpu");
    try {
        const log_t alone_a = decode({&a}, F, steps, gpu, "A", nullptr)[0];
        const log_t alone_b = decode({&b}, F, steps, gpu, "B", nullptr)[0];
        std::vector<std::pair<double, bool>> ms;
        const std::vector<log_t> ab = decode({&a, &b}, F, steps, gpu, "(A, B)", &ms);
        const std::vector<log_t> ba = decode({&b, &a}, F, steps, gpu, "(B, A)", nullptr);
        same_log(ab[0], alone_a, "(A, B) stream 0");
        same_log(ab[1], alone_b, "(A, B) stream 1");
        same_log(ba[0], alone_b, "(B, A) stream 0");
        same_log(ba[1], alone_a, "(B, A) stream 1");
        counts(alone_a, "A", {"fib", "msc", "ensemble_name", "service_name", "pcm", "audio", "datagroup", "packet_quality", "mot_object", "datagram",
                              "ip_quality"});
        counts(alone_b, "B", {"fib", "msc", "superframe", "ensemble_name", "service_name", "pcm", "audio", "dynamic_label", "pad_datagroup",
                              "pad_object"});
        std::vector<double> applied;
        for (size_t i = 0; i < ms.size(); i++) {
            std::printf("STEP %zu %.3f %d\n", i, ms[i].first, (int)ms[i].second);
            if (ms[i].second) applied.push_back(ms[i].first);
        }
        std::sort(applied.begin(), applied.end());
        if (!applied.empty())
            std::printf("MEDIAN_MS %.3f\n", applied.size() % 2 ? applied[applied.size() / 2]
                                                                : 0.5 * (applied[applied.size() / 2 - 1] + applied[applied.size() / 2]));
        if (fails) {
            std::printf("FAILED: %d mismatches\n", fails);
            return 1;
        }
        std::printf("STREAMS DROPIN OK %zu lines A %zu lines B\n", alone_a.size(), alone_b.size());
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
