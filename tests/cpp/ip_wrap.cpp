// TEST INFRASTRUCTURE: a C surface over the host ipAssembler (msc_consumers.h) so that
// tests/test_ip_cpu.py can drive it from Python (ctypes) and compare it with tests/ip_py.py
// and the golden file.
#include <cstring>
#include <vector>

#include "msc_consumers.h"

struct IpCapture {
    dabgpu::ipAssembler *a;
    std::vector<uint8_t> payload;   // of the last call
    int delivered = 0, quality = -1;
};

extern "C" {

void *iw_new(int handled, int crc_errors) {
    auto *c = new IpCapture();
    c->a = new dabgpu::ipAssembler(
        [c](const uint8_t *p, int32_t n) {
            c->payload.assign(p, p + n);
            c->delivered++;
        },
        [c](int v) { c->quality = v; });
    c->a->setCounters(handled, crc_errors);
    return c;
}
void iw_free(void *h) {
    auto *c = static_cast<IpCapture *>(h);
    delete c->a;
    delete c;
}
// a whole data group, as bytes: expanded to bits as packetAssembler delivers them.
// info = {status, quality, ip_bytes, payload length or -1, what the quality callback got or -1};
// returns the number of datagram callbacks inside the call
int iw_group(void *h, const uint8_t *bytes, int n, int *info, uint8_t *payload, int max_payload) {
    auto *c = static_cast<IpCapture *>(h);
    std::vector<uint8_t> bits((size_t)8 * n);
    for (int i = 0; i < 8 * n; i++) bits[(size_t)i] = (bytes[i >> 3] >> (7 - (i & 7))) & 1;
    c->delivered = 0;
    c->quality = -1;
    c->payload.clear();
    const dabgpu::ipAssembler::result r = c->a->add_mscDatagroup(bits);
    const int v[5] = {r.status, r.quality, r.ip_bytes, c->delivered ? (int)c->payload.size() : -1, c->quality};
    std::memcpy(info, v, sizeof v);
    std::memcpy(payload, c->payload.data(), std::min<size_t>(c->payload.size(), (size_t)max_payload));
    return c->delivered;
}
// {handledPackets, crcErrors, count of every status}
void iw_counters(void *h, int *out) {
    auto *a = static_cast<IpCapture *>(h)->a;
    out[0] = a->handledPackets();
    out[1] = a->crcErrors();
    for (int s = 0; s < dabgpu::ipAssembler::NSTATUS; s++) out[2 + s] = a->count(s);
}

}
