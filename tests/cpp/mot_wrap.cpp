// TEST INFRASTRUCTURE: a C surface over the host motAssembler (msc_consumers.h) so that
// tests/test_mot_cpu.py can drive it from Python (ctypes) and compare it with tests/mot_py.py
// and the golden file.
#include <cstring>
#include <vector>

#include "msc_consumers.h"

struct MotCapture {
    dabgpu::motAssembler *a;
    std::vector<dabgpu::motAssembler::object> objects;
    std::vector<int> at;        // the call during which each object was delivered
    int calls = 0;
};

extern "C" {

void *mw_new(int max_body_bytes) {
    auto *c = new MotCapture();
    c->a = new dabgpu::motAssembler([c](const dabgpu::motAssembler::object &o) {
        c->objects.push_back(o);
        c->at.push_back(c->calls);
    }, max_body_bytes);
    return c;
}
void mw_free(void *h) {
    auto *c = static_cast<MotCapture *>(h);
    delete c->a;
    delete c;
}
// a whole data group, as bytes: expanded to bits as packetAssembler delivers them
void mw_group(void *h, const uint8_t *bytes, int n) {
    auto *c = static_cast<MotCapture *>(h);
    std::vector<uint8_t> bits((size_t)8 * n);
    for (int i = 0; i < 8 * n; i++) bits[(size_t)i] = (bytes[i >> 3] >> (7 - (i & 7))) & 1;
    c->a->add_mscDatagroup(bits);
    c->calls++;
}
int mw_count(void *h) { return (int)static_cast<MotCapture *>(h)->objects.size(); }
// object i: info = {call, kind, transportId, contentType, contentsubType, name length, body length}
int mw_object(void *h, int i, int *info, uint8_t *name, int max_name, uint8_t *body, int max_body) {
    auto *c = static_cast<MotCapture *>(h);
    if (i < 0 || i >= (int)c->objects.size()) return -1;
    const auto &o = c->objects[(size_t)i];
    const int v[7] = {c->at[(size_t)i], o.kind, o.transportId, o.contentType, o.contentsubType, (int)o.name.size(), (int)o.body.size()};
    std::memcpy(info, v, sizeof v);
    std::memcpy(name, o.name.data(), std::min<size_t>(o.name.size(), (size_t)max_name));
    std::memcpy(body, o.body.data(), std::min<size_t>(o.body.size(), (size_t)max_body));
    return 0;
}
// {malformed, bad segment numbers, other types, entries in use}
void mw_counters(void *h, int *out) {
    auto *a = static_cast<MotCapture *>(h)->a;
    out[0] = a->malformed();
    out[1] = a->badSegments();
    out[2] = a->otherTypes();
    out[3] = a->entries();
}

}
