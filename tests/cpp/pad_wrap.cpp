// TEST INFRASTRUCTURE: a C surface over the host padAssembler (msc_consumers.h) so that
// tests/test_pad_cpu.py can drive it from Python (ctypes) and compare it with tests/pad_py.py
// and the golden file.
#include <algorithm>
#include <cstring>
#include <vector>

#include "msc_consumers.h"

struct PadCapture {
    dabgpu::padAssembler *a;
    std::vector<dabgpu::padAssembler::label> labels;
    std::vector<dabgpu::padAssembler::datagroup> groups;
    std::vector<int> label_at, group_at;    // the AU during which each was delivered
    int calls = 0;
};

extern "C" {

void *pw_new(void) {
    auto *c = new PadCapture();
    c->a = new dabgpu::padAssembler(
        [c](const dabgpu::padAssembler::label &l) {
            c->labels.push_back(l);
            c->label_at.push_back(c->calls);
        },
        [c](const dabgpu::padAssembler::datagroup &g) {
            c->groups.push_back(g);
            c->group_at.push_back(c->calls);
        });
    return c;
}
void pw_free(void *h) {
    auto *c = static_cast<PadCapture *>(h);
    delete c->a;
    delete c;
}
void pw_au(void *h, const uint8_t *bytes, int n, int length) {
    auto *c = static_cast<PadCapture *>(h);
    c->a->processAU(bytes, n, length);
    c->calls++;
}
int pw_labels(void *h) { return (int)static_cast<PadCapture *>(h)->labels.size(); }
int pw_groups(void *h) { return (int)static_cast<PadCapture *>(h)->groups.size(); }
// label i: info = {au, charset, nbytes, n_pieces, truncated}, piece_len[64], text[256]
int pw_label(void *h, int i, int *info, uint8_t *piece_len, uint8_t *text) {
    auto *c = static_cast<PadCapture *>(h);
    if (i < 0 || i >= (int)c->labels.size()) return -1;
    const auto &l = c->labels[(size_t)i];
    const int v[5] = {c->label_at[(size_t)i], l.charset, l.nbytes, l.n_pieces, (int)l.truncated};
    std::memcpy(info, v, sizeof v);
    std::memset(piece_len, 0, 64);
    std::memset(text, 0, 256);
    std::memcpy(piece_len, l.piece_len.data(), std::min<size_t>(l.piece_len.size(), 64));
    std::memcpy(text, l.text.data(), std::min<size_t>(l.text.size(), 256));
    return 0;
}
// group i: info = {au, nbytes, data_offset, data_nbytes, flags (DABGPU_DG_*), segmentNumber,
// transportId, groupType, lengthInd}, its bytes (at most max_bytes)
int pw_group(void *h, int i, int *info, uint8_t *bytes, int max_bytes) {
    auto *c = static_cast<PadCapture *>(h);
    if (i < 0 || i >= (int)c->groups.size()) return -1;
    const auto &g = c->groups[(size_t)i];
    const int flags = 1 * g.extension | 2 * g.crc | 4 * g.segment | 8 * g.user_access | 16 * g.last | 32 * g.transport |
                      64 * g.accepted;
    const int v[9] = {c->group_at[(size_t)i], (int)g.bytes.size(), g.data_offset, g.data_nbytes, flags,
                      g.segmentNumber, g.transportId, g.groupType, g.lengthInd};
    std::memcpy(info, v, sizeof v);
    std::memcpy(bytes, g.bytes.data(), std::min<size_t>(g.bytes.size(), (size_t)max_bytes));
    return 0;
}
// {labels, groups, aus, pads, unhandled, undefined[4], crc_failed, guard_dropped}
void pw_counters(void *h, int *out) {
    const auto &k = static_cast<PadCapture *>(h)->a->count();
    const int v[11] = {k.labels, k.groups, k.aus, k.pads, k.unhandled, k.undefined[0], k.undefined[1],
                       k.undefined[2], k.undefined[3], k.crc_failed, k.guard_dropped};
    std::memcpy(out, v, sizeof v);
}

}
