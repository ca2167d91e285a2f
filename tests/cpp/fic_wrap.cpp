// TEST INFRASTRUCTURE: a C surface over the host fib_processor (fib_processor.h) so that
// tests/test_fic_cpu.py and the GPU tests can drive it from Python (ctypes) and compare it with
// tests/fib_py.py and with dabgpu_fib_parse, record for record.
#include <cstring>
#include <string>
#include <vector>

#include "dabgpu.h"
#include "fib_processor.h"

static_assert(sizeof(dabgpu::fib_db) == sizeof(dabgpu_fic_db), "fib_db is dabgpu_fic_db");

struct FicCapture {
    dabgpu::fib_processor p;
    std::vector<dabgpu_fic_event> events;
    int fib = 0;
};

extern "C" {

void *fw_new(void) {
    auto *c = new FicCapture();
    c->p.on_event([c](int kind, int32_t id, const uint8_t *raw, int charset) {
        dabgpu_fic_event e = {};
        e.kind = kind;
        e.fib = c->fib;
        e.id = id;
        e.charset = charset;
        std::memcpy(e.label, raw, 16);
        c->events.push_back(e);
    });
    return c;
}
void fw_free(void *h) { delete static_cast<FicCapture *>(h); }
// one FIB of 32 bytes, msb first; index: what its events carry as `fib`.  Returns whether it overran.
int fw_fib(void *h, const uint8_t *fib, int index) {
    auto *c = static_cast<FicCapture *>(h);
    uint8_t b[256];
    for (int i = 0; i < 256; i++) b[i] = (fib[i >> 3] >> (7 - (i & 7))) & 1;
    c->fib = index;
    c->p.process_FIB(b, 0);
    return c->p.overran() ? 1 : 0;
}
void fw_clear(void *h) { static_cast<FicCapture *>(h)->p.clearEnsemble(); }
void fw_export(void *h, dabgpu_fic_db *db) { static_cast<FicCapture *>(h)->p.export_db(reinterpret_cast<dabgpu::fib_db *>(db)); }
void fw_import(void *h, const dabgpu_fic_db *db) {
    static_cast<FicCapture *>(h)->p.import_db(*reinterpret_cast<const dabgpu::fib_db *>(db));
}
// the events since the last call, at most max of them; returns how many there were
int fw_events(void *h, dabgpu_fic_event *out, int max) {
    auto *c = static_cast<FicCapture *>(h);
    const int n = (int)c->events.size();
    for (int i = 0; i < n && i < max; i++) out[i] = c->events[(size_t)i];
    c->events.clear();
    return n;
}
void fw_table(void *h, int want, dabgpu_fic_table *t) {
    auto *c = static_cast<FicCapture *>(h);
    std::vector<int> ids;
    const auto v = c->p.subchannels(&ids, want & DABGPU_SUBCH_MP2, want & DABGPU_SUBCH_PACKET, want & DABGPU_SUBCH_MOT,
                                    want & DABGPU_SUBCH_PAD);
    std::memset(t, 0, sizeof *t);
    t->n = (int32_t)v.size();
    for (size_t i = 0; i < v.size() && i < 64; i++) {
        std::memcpy(&t->sub[i], &v[i], sizeof(dabgpu_subch));
        t->ids[i] = (uint8_t)ids[i];
    }
}
// the named services' labels (UTF-8), each NUL-terminated, back to back; returns their number
int fw_labels(void *h, char *out, int max) {
    const auto v = static_cast<FicCapture *>(h)->p.serviceLabels();
    int at = 0, n = 0;
    for (const std::string &s : v) {
        if (at + (int)s.size() + 1 > max) break;
        std::memcpy(out + at, s.c_str(), s.size() + 1);
        at += (int)s.size() + 1;
        n++;
    }
    return n;
}
int fw_ensemble(void *h, char *out, int max) {
    const std::string s = static_cast<FicCapture *>(h)->p.ensembleName();
    if ((int)s.size() + 1 > max) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}
// out[0] kindofService; out[1] dataforAudioService's return, out[2..10] its fields; out[11]
// dataforDataService's return, out[12..21] its fields
void fw_lookup(void *h, const char *label, int *out) {
    auto &p = static_cast<FicCapture *>(h)->p;
    std::memset(out, 0, 22 * sizeof(int));
    out[0] = p.kindofService(label);
    dabgpu::audiodata a = {};
    dabgpu::packetdata d = {};
    if ((out[1] = p.dataforAudioService(label, &a))) {
        const int v[9] = {a.subchId, a.startAddr, a.uepFlag, a.protLevel, a.length, a.bitRate, a.ASCTy, a.language, a.programType};
        std::memcpy(out + 2, v, sizeof v);
    }
    if ((out[11] = p.dataforDataService(label, &d))) {
        const int v[10] = {d.subchId, d.startAddr, d.uepFlag, d.protLevel, d.DSCTy, d.length, d.bitRate, d.FEC_scheme, d.DGflag,
                           d.packetAddress};
        std::memcpy(out + 12, v, sizeof v);
    }
}

}
