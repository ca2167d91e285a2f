// msc_feed.h -- what the layers behind the MSC share (DAB+ superframes, the layer II
// synchroniser, packet mode; the PAD layer takes the wave helpers and the CRC): the run's MSC
// rows and a layer's slot map as the jobs carry them, the delivery rule, the row address, the
// bit/byte reader of the two row formats, the wave scans and the CRC-16 of a wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "crc16_poly.h"

namespace dab {

struct MscFeed {
    const uint8_t *msc;             // MSC bits of the run: [S][ncif][nsub][msc_stride]
    int32_t msc_stride, ncif, nsub, nstreams;
    int32_t packed;                 // msc holds bytes (8 bits msb first), else one bit per byte
    const int64_t *cif0s;           // [stream] CIF index of the run's first CIF slot
    const int32_t *ncifs;           // [stream] CIFs the stream delivered in the run
};
struct SlotMapView {                // a layer's slot map, [S][slots per stream]
    const int32_t *sub;             // table entry of each slot of the stream, -1: absent
    const int16_t *br;              // its bitRate
    const int64_t *since;           // its entry's since_cif (VitJob::ent_since)
};

// The delivery rule.  A slot receives the run's CIF slot c when it has an entry (sub >= 0), the
// stream delivered that CIF (c < nfed = ncifs[stream]) and the CIF lies 16 past the entry's
// since (dab-concurrent.cpp:172-175, the de-interleaver's warm-up): rel0 is rel_cif, the CIF
// index of the run's slot 0 counted from since.  A kernel that walks a run loads the three once.
// All three are read whatever sub is (an absent slot's too: the maps and the per-stream arrays
// hold every slot and stream).
__device__ __forceinline__ int64_t rel_cif(const MscFeed &F, const SlotMapView &M, int slot, int stream) {
    return F.cif0s[stream] - M.since[slot];
}
__device__ __forceinline__ bool fed(int sub, int nfed, int64_t rel0, int c) { return sub >= 0 && c < nfed && rel0 + c >= 16; }
__device__ __forceinline__ bool fed(const MscFeed &F, const SlotMapView &M, int slot, int stream, int c) {
    return fed(M.sub[slot], F.ncifs[stream], rel_cif(F, M, slot, stream), c);
}

// the row of table entry sub in CIF slot c of the stream
__device__ __forceinline__ const uint8_t *msc_row(const MscFeed &F, int stream, int c, int sub) {
    return F.msc + (((int64_t)stream * F.ncif + c) * F.nsub + sub) * F.msc_stride;
}
// Byte k of a row, 8 bits msb first (addtoFrame, mp4processor.cpp:115-121).  The unpacked
// format's 8 bytes come as one 8-byte load -- the form k_dp_layer is timed with -- so the row is
// read 8 bytes at a time at row + 8 k: global memory, where the hardware takes such a load at
// any address.  k_dp_layer, k_pkt_scan and k_pkt_copy read their rows through it; it is not for
// LDS.
__device__ __forceinline__ uint32_t row_byte(const uint8_t *__restrict__ row, int packed, int k) {
    if (packed) return row[k];
    const uint2 w = *(const uint2 *)(row + 8 * k);
    uint32_t t = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) t = (t << 1) | ((w.x >> (8 * j)) & 1u);
#pragma unroll
    for (int j = 0; j < 4; j++) t = (t << 1) | ((w.y >> (8 * j)) & 1u);
    return t;
}
__device__ __forceinline__ uint32_t row_bit(const uint8_t *__restrict__ row, int packed, int i) {
    return packed ? (row[i >> 3] >> (7 - (i & 7))) & 1u : row[i] & 1u;
}

// ---- over the 64 lanes of a wave -----------------------------------------------------------
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(v, d);
        if (lane >= d) v += n;
    }
    return v;
}
__device__ __forceinline__ int wave_scan_excl(int v, int lane) { return wave_scan_incl(v, lane) - v; }
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
// The CRC-16 register, from the all-ones preset, over bytes[0 .. n) (LDS or global memory), by
// the whole wave: each lane runs its slice from zero and shifts it past the bytes after it.
// The bytes pass check_CRC_bits when the result is crc16::CRC_GOOD.
__device__ __forceinline__ uint32_t wave_crc16(const uint8_t *bytes, int n, int lane) {
    const int m = (n + 63) / 64, a = min(n, lane * m), z = min(n, a + m);
    uint32_t part = 0;
    for (int i = a; i < z; i++) part = crc16::crc_byte(part, bytes[i]);
    return wave_xor(crc16::mulmod(part, crc16::xpow8(n - z))) ^ crc16::crc_ones(n);
}

}  // namespace dab
