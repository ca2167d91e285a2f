// k_mp2.hip -- MPEG-1/2 audio layer II on the GPU: the MSC bits of a classic DAB audio
// subchannel to PCM, bit for bit what mp2Processor does (mp2processor.cpp:365-617).
//
//   k_mp2_sync    mp2Processor::addtoFrame (:572-617), one lane-group per (stream, MP2 entry):
//                 the 12-ones search, the 12 header bits, the frame of lf bits, over the
//                 entry's delivered CIFs in order; state carried from run to run
//   k_mp2_decode  mp2Processor::mp2decodeFrame (:365-568): header, allocation, scfsi, scale
//                 factors, read_samples, the 64x32 matrixing, the 512-tap window, PCM
//
// The decoder is integer only.  Three places the reference leaves to the compiler or to the
// contents of memory are fixed here by rule (include/dabgpu.h, dabgpu_mp2_decode):
//   1. V is int16: (sum + 8192) >> 14 wraps modulo 2^16 when stored (the reference's int16_t V);
//   2. bits past the end of a frame read as 0 (the reference reads its frame buffer on);
//   3. products and sums are int32, two's complement (signed overflow is undefined in the
//      reference; every product below is taken in uint32 where it could leave int32).
//
// Matrixing is memoryless and only the window reaches back, over the 15 previous V vectors
// of the channel; Voffs only says where the reference's ring is written.  So the frames of
// a chain decode in parallel: a workgroup takes MP2_GROUP consecutive frames, and gets the
// 15 vectors before its first one from the chain's carried state or, when a decoded frame
// precedes it in the call, by decoding that frame's last five sample groups again.
//
// Work per frame: side information by one wave (every field's bit position is a prefix sum
// of widths known from the fields before it, so 64 lanes = 32 subbands x 2 channels read
// them at once); 12 groups x 64 code words over the 256 lanes; matrixing with lane = row i
// of N (its 32 coefficients in registers, the samples broadcast from LDS); window and
// output with lane = (step, j), both channels, one 32-bit store per stereo sample.
#include "dab_kernels.h"
#include <cmath>
#include <vector>

namespace dab {

// ---- tables (host) -------------------------------------------------------------------
// The upper half of the synthesis window, W[256 + k] = the ISO 11172-3 window (with the
// polyphase form's alternating block signs) times 65536.  The lower half follows from
// W[256 - k] = -W[256 + k] (equal where 256 + k is a multiple of 64), and the reference's
// table holds trunc(W + 0.5): a negative value is one closer to zero.
static const int32_t kHalfWindow[256] = {
    75038, 74992, 74856, 74630, 74313, 73908, 73415, 72835, 72169, 71420, 70590, 69679,
    68692, 67629, 66494, 65290, 64019, 62684, 61289, 59838, 58333, 56778, 55178, 53534,
    51853, 50137, 48390, 46617, 44821, 43006, 41176, 39336, 37489, 35640, 33791, 31947,
    30112, 28289, 26482, 24694, 22929, 21189, 19478, 17799, 16155, 14548, 12980, 11455,
    9975, 8540, 7154, 5818, 4533, 3300, 2122, 998, -70, -1082, -2037, -2935,
    -3776, -4561, -5288, -5959, 6574, 7134, 7640, 8092, 8492, 8840, 9139, 9389,
    9592, 9750, 9863, 9935, 9966, 9959, 9916, 9838, 9727, 9585, 9416, 9219,
    8998, 8755, 8491, 8209, 7910, 7597, 7271, 6935, 6589, 6237, 5879, 5517,
    5153, 4788, 4425, 4063, 3705, 3351, 3004, 2663, 2330, 2006, 1692, 1388,
    1095, 814, 545, 288, 45, -185, -402, -605, -794, -970, -1131, -1280,
    -1414, -1535, -1644, -1739, -1822, -1893, -1952, -2000, 2037, 2063, 2080, 2087,
    2085, 2075, 2057, 2032, 2001, 1962, 1919, 1870, 1817, 1759, 1698, 1634,
    1567, 1498, 1428, 1356, 1283, 1210, 1137, 1064, 991, 919, 848, 779,
    711, 645, 581, 519, 459, 401, 347, 294, 244, 197, 153, 111,
    72, 36, 2, -29, -57, -83, -106, -127, -146, -163, -177, -189,
    -200, -208, -215, -221, -224, -227, -228, -228, -227, -225, -222, -218,
    213, 208, 202, 196, 190, 183, 176, 169, 161, 154, 147, 139,
    132, 125, 117, 111, 104, 97, 91, 85, 79, 73, 68, 63,
    58, 53, 49, 45, 41, 38, 35, 31, 29, 26, 24, 21,
    19, 17, 16, 14, 13, 11, 10, 9, 8, 7, 7, 6,
    5, 5, 4, 4, 3, 3, 2, 2, 2, 2, 1, 1,
    1, 1, 1, 1,
};

std::vector<uint8_t> mp2_host_tables() {
    std::vector<uint8_t> blob(sizeof(Mp2Tabs), 0);
    Mp2Tabs &T = *reinterpret_cast<Mp2Tabs *>(blob.data());
    for (int k = 0; k < 256; k++) {
        const int32_t h = kHalfWindow[k];
        T.D[256 + k] = h;
        if (k) T.D[256 - k] = ((256 + k) % 64 == 0) ? h : -h;
    }
    for (int i = 0; i < 512; i++)
        if (T.D[i] < 0) T.D[i] += 1;
    // N[i][j] with the reference's expression and its constant for pi / 64 (mp2processor.cpp:229-233)
    for (int i = 0; i < 64; i++)
        for (int j = 0; j < 32; j++)
            T.N[i * 32 + j] = (int16_t)(256.0 * std::cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405));
    // subband layouts as runs of (subbands, allocation bits, allocation row): the low-rate
    // tables (3-B.2c/d), the high-rate tables (3-B.2a/b), the MPEG-2 LSF table (13818-3 B.1)
    static const int runs[3][4][3] = {{{2, 4, 4}, {10, 3, 4}, {0, 0, 0}, {0, 0, 0}},
                                      {{3, 4, 3}, {8, 4, 2}, {12, 3, 1}, {7, 2, 0}},
                                      {{4, 4, 5}, {7, 3, 4}, {19, 2, 4}, {0, 0, 0}}};
    for (int t = 0; t < 3; t++)
        for (int r = 0, sb = 0; r < 4; r++)
            for (int n = 0; n < runs[t][r][0]; n++) T.band[t][sb++] = (uint8_t)(runs[t][r][1] << 4 | runs[t][r][2]);
    // allocation rows: the set of quantisers (bit q: quantiser q = 1..17) a row offers, in
    // ascending order after "nothing allocated"
    auto range = [](int a, int b) { uint32_t m = 0; for (int q = a; q <= b; q++) m |= 1u << q; return m; };
    const uint32_t rows[6] = {range(1, 2) | range(17, 17), range(1, 6) | range(17, 17), range(1, 14) | range(17, 17),
                              range(1, 1) | range(3, 3) | range(5, 17), range(1, 2) | range(4, 15) | range(17, 17),
                              range(1, 15)};
    for (int r = 0; r < 6; r++)
        for (int q = 1, a = 1; q <= 17 && a < 16; q++)
            if (rows[r] >> q & 1) T.rowq[r][a++] = (uint8_t)q;
    return blob;
}

// ---- device helpers ------------------------------------------------------------------
constexpr int MP2_GROUP = 4;        // consecutive frames of a chain per workgroup
constexpr int MP2_THREADS = 256;

// n <= 16 bits at bit position pos of a frame of `len` readable bytes, msb first; bytes
// past the end read as 0 (rule 2)
__device__ __forceinline__ uint32_t mp2_bits(const uint8_t *__restrict__ f, int len, int pos, int n) {
    const int b = pos >> 3;
    const uint32_t w = (b < len ? (uint32_t)f[b] << 16 : 0u) | (b + 1 < len ? (uint32_t)f[b + 1] << 8 : 0u) |
                       (b + 2 < len ? (uint32_t)f[b + 2] : 0u);
    return (w >> (24 - (pos & 7) - n)) & ((1u << n) - 1u);
}

// the checks of mp2decodeFrame that return 0 (mp2processor.cpp:383-402): sync word and
// layer, bit-rate index 1..14, sampling frequency not 3
__device__ __forceinline__ bool mp2_header_ok(const uint8_t *__restrict__ f, int len) {
    const uint32_t h = mp2_bits(f, len, 0, 16), b2 = mp2_bits(f, len, 16, 8);
    const uint32_t bri = b2 >> 4, fs = (b2 >> 2) & 3;
    return (h >> 8) == 0xFF && (h & 0xF6) == 0xF4 && bri >= 1 && bri <= 14 && fs != 3;
}

// quantiser q = 1..17: levels (3, 5, 9 grouped three to a code word; else 2^bits - 1)
__device__ __forceinline__ void mp2_quant(int q, int &lev, int &grouped, int &cw) {
    grouped = (q == 1 || q == 2 || q == 4);
    if (grouped) {
        lev = q == 1 ? 3 : q == 2 ? 5 : 9;
        cw = q == 1 ? 5 : q == 2 ? 7 : 10;
    } else {
        cw = q == 3 ? 3 : q - 1;
        lev = (1 << cw) - 1;
    }
}

// side information of one frame, per lane l = 2 * subband + channel
struct Mp2Side {
    int32_t sf[64][3];      // the scale factor of each part, resolved (mp2processor.cpp:311-316)
    int16_t spos[64];       // bit offset of the lane's code words within a group's bits
    uint8_t q[64];          // quantiser (0: nothing allocated)
    int32_t base, gbits;    // first sample bit; bits per group
    int32_t sblimit, bound;
    int32_t ret;            // mp2decodeFrame's return value
};

// Wave 0 reads the header and the side information of frame f.  S.ret = 0: rejected.
__device__ __forceinline__ void mp2_parse(const uint8_t *__restrict__ f, int len, const Mp2Tabs *__restrict__ T, Mp2Side &S, int lane) {
    if (!mp2_header_ok(f, len)) {
        if (lane == 0) S.ret = 0;
        return;
    }
    const uint32_t b1 = mp2_bits(f, len, 8, 8), b2 = mp2_bits(f, len, 16, 8), b3 = mp2_bits(f, len, 24, 8);
    const int bri = (int)(b2 >> 4), fs = (int)(b2 >> 2) & 3, padding = (int)(b2 >> 1) & 1;
    const int mode = (int)(b3 >> 6), ext = (int)(b3 >> 4) & 3;
    const bool lsf = (b1 & 8) == 0, mono = mode == 3;
    // kbit/s and Hz: 32 .. 384 (MPEG-1), 8 .. 160 (MPEG-2), as steps from the one before
    int kbps;
    if (!lsf) kbps = bri <= 2 ? 16 + 16 * bri : bri <= 4 ? 32 + 8 * bri : bri <= 8 ? 16 * bri : bri <= 12 ? 32 * bri - 128 : 64 * bri - 512;
    else kbps = bri <= 8 ? 8 * bri : 16 * bri - 64;
    const int rate = (fs == 0 ? 44100 : fs == 1 ? 48000 : 32000) >> (lsf ? 1 : 0);
    // the quantisation class: by the bit rate per channel for MPEG-1 (<= 48: low-rate
    // tables with 8 or 12 subbands; <= 80: 27 subbands; above: 30, or 27 at 48 kHz)
    int table, sblimit;
    if (lsf) { table = 2; sblimit = 30; }
    else {
        const int per = mono ? kbps : kbps >> 1;
        if (per <= 48) { table = 0; sblimit = fs == 2 ? 12 : 8; }
        else if (per <= 80) { table = 1; sblimit = 27; }
        else { table = 1; sblimit = fs == 1 ? 27 : 30; }
    }
    int bound = mode == 1 ? (ext + 1) << 2 : mono ? 0 : 32;
    if (bound > sblimit) bound = sblimit;
    int pos = 32 + ((b1 & 1) ? 0 : 16);
    const int sb = lane >> 1, ch = lane & 1, nch = mono ? 1 : 2;
    const bool live = sb < sblimit;
    const bool own = live && (sb < bound || ch == 0);      // reads its own allocation and code words
    // allocation
    const int bd = live ? T->band[table][sb] : 0;
    int w = own ? bd >> 4 : 0;
    int inc = wave_scan_incl(w, lane);
    int a = own ? (int)mp2_bits(f, len, pos + inc - w, w) : 0;
    const int a0 = __shfl(a, lane & ~1);
    if (live && !own) a = a0;
    const int q = a ? T->rowq[bd & 15][a] : 0;
    pos += __shfl(inc, 63);
    // scale factor selection, then the scale factors it announces
    const bool reads = live && q && ch < nch;
    w = reads ? 2 : 0;
    inc = wave_scan_incl(w, lane);
    int si = reads ? (int)mp2_bits(f, len, pos + inc - w, 2) : 0;
    pos += __shfl(inc, 63);
    const int nsf = reads ? (si == 0 ? 3 : si == 2 ? 1 : 2) : 0;
    w = 6 * nsf;
    inc = wave_scan_incl(w, lane);
    int s0 = 0, s1 = 0, s2 = 0;
    if (reads) {
        const int p0 = pos + inc - w;
        const int x = (int)mp2_bits(f, len, p0, 6), y = nsf > 1 ? (int)mp2_bits(f, len, p0 + 6, 6) : 0,
                  z = nsf > 2 ? (int)mp2_bits(f, len, p0 + 12, 6) : 0;
        s0 = x;
        s1 = si == 0 ? y : si == 3 ? y : x;
        s2 = si == 0 ? z : si == 2 ? x : y;
    }
    pos += __shfl(inc, 63);
    // the code words of one group of three steps
    int lev = 0, grouped = 0, cw = 0;
    if (q) mp2_quant(q, lev, grouped, cw);
    w = (own && q) ? (grouped ? cw : 3 * cw) : 0;
    inc = wave_scan_incl(w, lane);
    S.spos[lane] = (int16_t)(inc - w);
    S.q[lane] = (uint8_t)((own && q) ? q : 0);
    const int sv[3] = {s0, s1, s2};
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const int s = sv[p], adj = s / 3;
        const int32_t base = s % 3 == 0 ? 0x02000000 : s % 3 == 1 ? 0x01965FEA : 0x01428A30;   // 2^25 * 2^(-k/3)
        S.sf[lane][p] = s == 63 ? 0 : (base + ((1 << adj) >> 1)) >> adj;
    }
    const int gbits = __shfl(inc, 63);
    if (lane == 0) {
        S.base = pos;
        S.gbits = gbits;
        S.sblimit = sblimit;
        S.bound = bound;
        S.ret = 144000 * kbps / rate + padding;
    }
}

// read_samples (mp2processor.cpp:299-342) for groups [g0, g1): smp[3 * group + idx][ch][sb]
__device__ __forceinline__ void mp2_dequant(const uint8_t *__restrict__ f, int len, const Mp2Side &S, int32_t (*smp)[2][32], int g0,
                            int g1, int tid) {
    for (int it = tid; it < (g1 - g0) * 64; it += MP2_THREADS) {
        const int g = g0 + (it >> 6), l = it & 63, sb = l >> 1, ch = l & 1;
        const bool joint = sb >= S.bound;              // one set of samples for both channels
        if (joint && ch) continue;
        int32_t v[3] = {0, 0, 0};
        const int q = S.q[l];
        if (q) {
            int lev, grouped, cw;
            mp2_quant(q, lev, grouped, cw);
            const int p = S.base + g * S.gbits + S.spos[l];
            int c[3];
            if (grouped) {
                const int x = (int)mp2_bits(f, len, p, cw);
                c[0] = x % lev;
                c[1] = (x / lev) % lev;
                c[2] = x / lev / lev;
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++) c[k] = (int)mp2_bits(f, len, p + k * cw, cw);
            }
            const int32_t scale = 65536 / (lev + 1), adj = ((lev + 1) >> 1) - 1;
            const int32_t sf = S.sf[l][g >> 2];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t val = (uint32_t)((adj - c[k]) * scale);
                const int32_t hi = (int32_t)(val * (uint32_t)(sf >> 12));
                const int32_t lo = (int32_t)(val * (uint32_t)(sf & 4095) + 2048u) >> 12;
                v[k] = (int32_t)((uint32_t)hi + (uint32_t)lo) >> 12;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            smp[3 * g + k][ch][sb] = v[k];
            if (joint) smp[3 * g + k][1][sb] = v[k];
        }
    }
}

// matrixing (mp2processor.cpp:528-535) of steps [t0, t1) into vec[ch][slot0 + t - t0][i]:
// lane i = tid & 63 holds row i of N, each wave takes every fourth (step, channel)
__device__ __forceinline__ void mp2_matrix(const int32_t (*smp)[2][32], int16_t (*vec)[51][64], const int32_t *n, int t0, int t1, int slot0,
                           int tid) {
    const int i = tid & 63;
    for (int p = tid >> 6; p < 2 * (t1 - t0); p += MP2_THREADS / 64) {
        const int t = t0 + (p >> 1), ch = p & 1;
        const int32_t *s = smp[t][ch];
        uint32_t sum = 0;
#pragma unroll
        // 24-bit multiplies: |N| <= 256, and |sample| <= 104,848 < 2^23 whatever the code words
        // (mp2_dequant: |val| <= 8 * 6553, scale factor <= 2.0), so the low 32 bits are the int32
        // product; the full-rate form measured 26 % faster for the kernel (profiles/mp2_layer.txt)
        for (int j = 0; j < 32; j++) sum += (uint32_t)__mul24(n[j], s[j]);
        vec[ch][slot0 + t - t0][i] = (int16_t)((int32_t)(sum + 8192u) >> 14);      // rule 1: V is int16
    }
}

// window and output (mp2processor.cpp:537-561) of the 36 steps in vec slots 15..50: step t
// reads the vectors t .. t - 15, even ones at [j], odd ones at [32 + j]
__device__ __forceinline__ void mp2_window(const int16_t (*vec)[51][64], const int32_t *D, uint32_t *__restrict__ pcm, int tid) {
    for (int it = tid; it < 1152; it += MP2_THREADS) {
        const int t = it >> 5, j = it & 31;
        uint32_t out = 0;
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            uint32_t acc = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int32_t u = vec[ch][15 + t - i][(i & 1) * 32 + j];
                // (u is int16 and |D| < 2^17: both fit 24 bits; the product wraps to int32, rule 3)
                const int32_t p = (int32_t)((uint32_t)__mul24(u, D[32 * i + j]) + 32u) >> 6;
                acc -= (uint32_t)p;
            }
            int32_t s = (int32_t)(acc + 8u) >> 4;
            s = s < -32768 ? -32768 : s > 32767 ? 32767 : s;
            out |= ((uint32_t)s & 0xFFFFu) << (16 * ch);
        }
        pcm[it] = out;                                   // pcm[(t * 32 + j) * 2 + ch]
    }
}

__global__ __launch_bounds__(MP2_THREADS) void k_mp2_decode(Mp2Job J) {
    __shared__ __attribute__((aligned(16))) int32_t smp[36][2][32];
    __shared__ __attribute__((aligned(16))) int16_t vec[2][51][64];
    __shared__ int32_t Dl[512];
    __shared__ Mp2Side S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ngrp = (J.chain_len + MP2_GROUP - 1) / MP2_GROUP;
    const int chain = blockIdx.x / ngrp, j0 = (blockIdx.x % ngrp) * MP2_GROUP;
    if (chain >= J.n_chains) return;
    const int64_t f0 = (int64_t)(chain / J.cdiv) * J.idx_a + (int64_t)(chain % J.cdiv) * J.idx_b;   // output index of frame 0
    const uint8_t *frames = J.frames + (int64_t)chain * J.chain_len * J.stride;
    const uint8_t *present = J.present ? J.present + (int64_t)chain * J.chain_len : nullptr;
    const int len = (int)J.stride;
    int32_t n[32];
#pragma unroll
    for (int j = 0; j < 32; j++) n[j] = J.tabs->N[lane * 32 + j];
    for (int i = tid; i < 512; i += MP2_THREADS) Dl[i] = J.tabs->D[i];
    // the 15 V vectors before frame j0: the tail of the last decoded frame before it in this
    // call, else the carried state
    int prev = j0 - 1;
    while (prev >= 0 && !((!present || present[prev]) && mp2_header_ok(frames + (int64_t)prev * J.stride, len))) prev--;
    if (prev >= 0) {
        const uint8_t *f = frames + (int64_t)prev * J.stride;
        if (tid < 64) mp2_parse(f, len, J.tabs, S, lane);
        __syncthreads();
        mp2_dequant(f, len, S, smp, 7, 12, tid);
        __syncthreads();
        mp2_matrix(smp, vec, n, 21, 36, 0, tid);
    } else {
        const int16_t *st = J.state_in + (int64_t)chain * (2 * 15 * 64);
        for (int i = tid; i < 2 * 15 * 64; i += MP2_THREADS) vec[i / 960][(i % 960) >> 6][i & 63] = st[i];
    }
    __syncthreads();
    for (int j = j0; j < j0 + MP2_GROUP && j < J.chain_len; j++) {
        const int64_t o = f0 + (int64_t)j * J.idx_c;
        const bool have = !present || present[j];
        const uint8_t *f = frames + (int64_t)j * J.stride;
        if (have && tid < 64) mp2_parse(f, len, J.tabs, S, lane);
        __syncthreads();
        const int ret = have ? S.ret : 0;
        if (tid == 0) {
            if (J.ret) J.ret[o] = ret;
            if (J.info && have) {
                J.info[o].status = ret ? 2 : 1;
                J.info[o].frame_bytes = ret;
            }
        }
        if (ret) {
            mp2_dequant(f, len, S, smp, 0, 12, tid);
            __syncthreads();
            mp2_matrix(smp, vec, n, 0, 36, 15, tid);
            __syncthreads();
            mp2_window(vec, Dl, (uint32_t *)(J.pcm + o * 2304), tid);
            // the frame's last 15 vectors become the history of the next one
            int16_t keep[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = tid + k * MP2_THREADS;
                keep[k] = i < 1920 ? vec[i / 960][36 + ((i % 960) >> 6)][i & 63] : (int16_t)0;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = tid + k * MP2_THREADS;
                if (i < 1920) vec[i / 960][(i % 960) >> 6][i & 63] = keep[k];
            }
        }
        __syncthreads();
    }
    if (j0 + MP2_GROUP >= J.chain_len) {                 // the chain's last workgroup leaves the state
        int16_t *st = J.state_out + (int64_t)chain * (2 * 15 * 64);
        for (int i = tid; i < 2 * 15 * 64; i += MP2_THREADS) st[i] = vec[i / 960][(i % 960) >> 6][i & 63];
    }
}

// ---- the frame synchroniser ----------------------------------------------------------
constexpr int MP2_MAX_FRAME = 6 * 384;      // bytes: 2 * 24 * bitRate bits at 384 kbit/s

// addbittoMP2 for m bits at once: bits [i, i + m) of the CIF's row to bits [bc, bc + m) of the
// frame being collected, each lane one byte of the frame
__device__ __forceinline__ void mp2_take(uint8_t *part, int bc, const uint8_t *__restrict__ row, int packed, int i, int m,
                                         int lane) {
    for (int k = (bc >> 3) + lane; k <= (bc + m - 1) >> 3; k += 64) {
        uint32_t byte = part[k];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const int d = 8 * k + b;
            if (d >= bc && d < bc + m) byte = (byte & ~(0x80u >> b)) | (row_bit(row, packed, i + d - bc) << (7 - b));
        }
        part[k] = (uint8_t)byte;
    }
}

// mp2Processor::addtoFrame (mp2processor.cpp:572-617) for one (stream, MP2 slot) per wave,
// over the CIFs of the run that its entry delivers, in order.  A frame that completes in
// CIF c goes to frame slot c (lf bits, zeros up to fstride: rule 2); lf is taken once per
// CIF, as the reference takes it once per call.  Every branch is wave-uniform: a stretch
// of bits is searched 48 at a time (the run of ones carried in, the twelve-ones test by
// shifts of the ballot mask) or taken in bulk.
__global__ __launch_bounds__(64) void k_mp2_sync(Mp2SyncJob J) {
    __shared__ uint8_t part[MP2_MAX_FRAME];
    const int chain = blockIdx.x, lane = threadIdx.x;
    const int s = chain / J.nmp, m = chain % J.nmp;
    const MscFeed &F = J.feed;
    const int sub = J.map.sub[chain], nfed = F.ncifs[s];
    const int64_t rel0 = rel_cif(F, J.map, chain, s);
    const int nb = 24 * J.map.br[chain];
    Mp2SyncState st = J.state[chain];
    uint8_t *carried = J.part + (int64_t)chain * J.fstride;
    if (sub >= 0)
        for (int k = lane; k < J.fstride; k += 64) part[k] = carried[k];
    __syncthreads();
    for (int c = 0; c < F.ncif; c++) {
        const int64_t o = ((int64_t)s * F.ncif + c) * J.nmp + m;
        const bool on = fed(sub, nfed, rel0, c);
        int emitted = 0, rate = 0;
        if (on) {
            const uint8_t *row = msc_row(F, s, c, sub);
            const int lf = st.half_rate ? 2 * nb : nb;
            int i = 0;
            while (i < nb) {
                if (st.ok == 2) {
                    const int mm = max(1, min(nb - i, lf - st.bc));
                    mp2_take(part, st.bc, row, F.packed, i, mm, lane);
                    __syncthreads();
                    st.bc += mm;
                    i += mm;
                    if (st.bc >= lf) {
                        uint8_t *f = J.frames + ((int64_t)chain * F.ncif + c) * J.fstride;
                        for (int k = lane; k < J.fstride; k += 64) f[k] = k < (lf >> 3) ? part[k] : (uint8_t)0;
                        __syncthreads();
                        emitted = 1;
                        rate = st.half_rate ? 24000 : 48000;
                        st.ok = st.hc = st.bc = 0;
                    }
                } else if (st.ok == 0) {
                    const int n = min(48, nb - i);
                    const uint32_t bit = lane < n ? row_bit(row, F.packed, i + lane) : 0u;
                    const uint64_t mask = __ballot(bit != 0);
                    const uint64_t ext = ((1ull << st.hc) - 1ull) | (mask << st.hc);     // the carried ones, then the bits
                    const uint64_t x2 = (ext & ext >> 1) & (ext & ext >> 1) >> 2;
                    const uint64_t r = (x2 & x2 >> 4) & x2 >> 8;                      // bit p: ones at p .. p + 11
                    if (r) {
                        i += __builtin_ctzll(r) + 12 - st.hc;
                        if (lane == 0) {
                            part[0] = 0xFF;
                            part[1] = (uint8_t)(part[1] | 0xF0);
                        }
                        __syncthreads();
                        st.bc = 12;
                        st.hc = 12;
                        st.ok = 1;
                    } else {
                        const int L = st.hc + n;
                        st.hc = __builtin_clzll(~(ext << (64 - L)));
                        i += n;
                    }
                } else {
                    const int mm = min(24 - st.bc, nb - i);
                    mp2_take(part, st.bc, row, F.packed, i, mm, lane);
                    __syncthreads();
                    st.bc += mm;
                    i += mm;
                    if (st.bc == 24) {
                        // mp2sampleRate + setSamplerate (:261-285): only 48000 and 24000 are taken
                        const int f1 = part[1], f2 = part[2];
                        if ((f1 & 0xF6) == 0xF4 && f2 - 0x10 < 0xE0 && ((f2 >> 2) & 3) == 1) st.half_rate = (f1 & 8) ? 0 : 1;
                        st.ok = 2;
                    }
                }
            }
        }
        if (lane == 0) {
            J.info[o].status = on ? emitted : -1;
            J.info[o].sample_rate = rate;
            J.info[o].frame_bytes = 0;
            J.present[(int64_t)chain * F.ncif + c] = (uint8_t)emitted;
        }
    }
    __syncthreads();
    if (sub >= 0)
        for (int k = lane; k < J.fstride; k += 64) carried[k] = part[k];
    if (lane == 0) J.state[chain] = st;
}

hipError_t launch_mp2_sync(hipStream_t st, const Mp2SyncJob &job) {
    if (job.nmp <= 0 || job.feed.nstreams <= 0 || job.feed.ncif <= 0) return hipSuccess;
    if (job.fstride <= 0 || job.fstride > MP2_MAX_FRAME) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mp2_sync, dim3(job.feed.nstreams * job.nmp), dim3(64), 0, st, job);
    return hipGetLastError();
}

hipError_t launch_mp2_decode(hipStream_t st, const Mp2Job &job) {
    if (job.n_chains <= 0 || job.chain_len <= 0) return hipSuccess;
    if (job.stride < 4 || job.cdiv <= 0) return hipErrorInvalidValue;
    const int64_t blocks = (int64_t)job.n_chains * ((job.chain_len + MP2_GROUP - 1) / MP2_GROUP);
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mp2_decode, dim3((unsigned)blocks), dim3(MP2_THREADS), 0, st, job);
    return hipGetLastError();
}

}  // namespace dab
