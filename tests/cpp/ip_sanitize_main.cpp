// TEST INFRASTRUCTURE: a stand-alone program over the host ipAssembler, built with
// -fsanitize=address,undefined (Makefile.ip) and run by tests/test_ip_cpu.py: every group goes in
// twice, as bits and as a heap block of exactly its length, so that a read past a group is seen.
//   input : int32 n_slots; per slot int32 handled, crc_errors, n_groups; per group int32 n_bytes, bytes
//   output: per group int32 status, quality, ip_bytes, payload length (-1: none), then the payload;
//           per slot, after its groups, int32 handledPackets, crcErrors
#include <cstdio>
#include <cstring>
#include <vector>

#include "msc_consumers.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_slots;
    if (fread(&n_slots, sizeof n_slots, 1, in) != 1) return 3;
    for (int32_t s = 0; s < n_slots; s++) {
        int32_t head[3];
        if (fread(head, sizeof head, 1, in) != 1) return 3;
        std::vector<uint8_t> pay[2];
        int got[2] = {0, 0};
        dabgpu::ipAssembler a([&](const uint8_t *p, int32_t n) { pay[0].assign(p, p + n); got[0]++; });
        dabgpu::ipAssembler b([&](const uint8_t *p, int32_t n) { pay[1].assign(p, p + n); got[1]++; });
        a.setCounters(head[0], head[1]);
        b.setCounters(head[0], head[1]);
        for (int32_t g = 0; g < head[2]; g++) {
            int32_t n;
            if (fread(&n, sizeof n, 1, in) != 1 || n < 0) return 3;
            uint8_t *bytes = new uint8_t[(size_t)n];
            if (n && fread(bytes, 1, (size_t)n, in) != (size_t)n) return 3;
            std::vector<uint8_t> bits((size_t)8 * n);
            for (int i = 0; i < 8 * n; i++) bits[(size_t)i] = (bytes[i >> 3] >> (7 - (i & 7))) & 1;
            got[0] = got[1] = 0;
            const dabgpu::ipAssembler::result ra = a.add_mscDatagroup(bits), rb = b.add_group(bytes, n);
            delete[] bytes;
            if (ra.status != rb.status || ra.quality != rb.quality || ra.ip_bytes != rb.ip_bytes || got[0] != got[1] ||
                (got[0] && pay[0] != pay[1]) || got[0] != (ra.status == dabgpu::ipAssembler::DELIVERED))
                return 4;
            const int32_t r[4] = {ra.status, ra.quality, ra.ip_bytes, got[0] ? (int32_t)pay[0].size() : -1};
            fwrite(r, sizeof r, 1, out);
            if (got[0] && !pay[0].empty()) fwrite(pay[0].data(), 1, pay[0].size(), out);
        }
        const int32_t tail[2] = {a.handledPackets(), a.crcErrors()};
        fwrite(tail, sizeof tail, 1, out);
    }
    fclose(out);
    fclose(in);
    return 0;
}
