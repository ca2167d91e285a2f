// k_dabplus.hip -- DAB+ superframe layer for gfx950: mp4Processor::addtoFrame +
// processSuperframe (mp4processor.cpp:107-292) for every DAB+ subchannel of every
// stream, over the CIFs one pipeline run decoded.
//
// One kernel, k_dp_layer, one workgroup per (stream, DAB+ subchannel), in three phases;
// one launch per run of up to 512 frames.  Fire: every CIF of the run is a superframe candidate -- the 5 blocks ending
// at it -- and one thread per CIF checks the fire code at the oldest block.  Decode: the
// workgroup's waves take the passing candidates in turn, one wave per superframe: the
// RS(120,110) decode of the RSDims interleaved codewords, the AU table and the AU
// CRCs.  Walk: one wave runs the reference's sequential block counting
// (blocksInBuffer) over the candidates' verdicts, which decides which of them the
// reference would have evaluated, and carries the last 4 CIFs and the state to the
// next run.  The RS decoder is a restatement of the reference's Karn-style decoder
// (reed-solomon.cpp:143-399: syndromes, Berlekamp-Massey, Chien search over all 255
// positions, Forney), so its return value (errors corrected, or -1) and corrections
// match it exactly.  k_rs is that decoder on its own, one lane per codeword.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

constexpr int RS_NN = 255, RS_PAD = 135, RS_ROW = 121;   // LDS row stride (odd: spreads banks)

__device__ __forceinline__ int mod255(int x) { return x % 255; }

struct GfTabs {
    uint8_t exp[256];
    uint8_t log[256];
    uint16_t fire[256];      // fire-code syndrome table
    uint8_t mul[10][256];    // s * alpha^i: one lookup per Horner step of syndrome i
    uint16_t crc[256];       // CRC-CCITT (0x1021, msb first) byte table
    uint16_t pow8[1024];     // x^(8d) mod the CRC polynomial
};
static_assert(sizeof(GfTabs) == FIBCRC_OFF, "host table layout (the FIB CRC table follows)");

__device__ __forceinline__ int gmul(const GfTabs &g, int a, int b) {
    return (a && b) ? g.exp[mod255(g.log[a] + g.log[b])] : 0;
}
__device__ __forceinline__ int gdiv(const GfTabs &g, int a, int b) {
    return a ? g.exp[mod255(RS_NN + g.log[a] - g.log[b])] : 0;
}

// Syndrome i of the codeword src[0..119] (byte m is full-codeword position 135 + m; the
// 135 leading pad bytes are zero and leave the Horner sum at zero) (reed-solomon.cpp:231-266).
__device__ __forceinline__ int rs_syndrome(const uint8_t *src, int i, const GfTabs &g) {
    int s = 0;
    for (int m = 0; m < 120; m++) s = src[m] ^ g.mul[i][s];
    return s;
}

// decode_rs after the syndromes (reed-solomon.cpp:268-399): Berlekamp-Massey,
// Chien search over all 255 positions, error evaluator, Forney.  Returns the
// number of corrected symbols or -1, and the corrections to apply: fix_pos[k]
// (full-codeword position) ^= fix_val[k] for k < *nfix.
__device__ int rs_solve(const int (&syn)[10], const GfTabs &g, uint8_t *roots, uint8_t *locs, uint8_t *fix_pos,
                        uint8_t *fix_val, int *nfix) {
    *nfix = 0;
    int any = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) any |= syn[i];
    if (!any) return 0;
    // Berlekamp-Massey (:268-318)
    int L[11], Cr[11];
#pragma unroll
    for (int i = 0; i < 11; i++) L[i] = Cr[i] = 0;
    L[0] = 1;
    Cr[1] = 1;
    int err = syn[0], Lr = 0;
#pragma unroll
    for (int K = 1; K <= 10; K++) {
        int old[11];
#pragma unroll
        for (int i = 0; i < 11; i++) old[i] = L[i];
#pragma unroll
        for (int i = 0; i < 11; i++) L[i] ^= gmul(g, err, Cr[i]);
        if (2 * Lr < K && err != 0) {
            Lr = K - Lr;
#pragma unroll
            for (int i = 0; i < 11; i++) Cr[i] = gdiv(g, old[i], err);
        }
#pragma unroll
        for (int i = 10; i >= 1; i--) Cr[i] = Cr[i - 1];
        Cr[0] = 0;
        if (K < 10) {
            err = syn[K];
#pragma unroll
            for (int i = 1; i <= K; i++) err ^= gmul(g, syn[K - i], L[i]);
        }
    }
    int deg = 0, LL[11];
#pragma unroll
    for (int i = 0; i < 11; i++) {
        if (L[i]) deg = i;
        LL[i] = g.log[L[i]];                              // log(0) = 255
    }
    // Chien search over every position (:323-360)
    int reg[11];
#pragma unroll
    for (int j = 0; j < 11; j++) reg[j] = LL[j];
    int count = 0;
    for (int i = 1; i <= RS_NN; i++) {
        int result = 1;
#pragma unroll
        for (int j = 10; j >= 1; j--) {
            if (j <= deg && reg[j] != RS_NN) {
                reg[j] = mod255(reg[j] + j);
                result ^= g.exp[reg[j]];
            }
        }
        if (result == 0) {
            if (count < 10) { roots[count] = (uint8_t)i; locs[count] = (uint8_t)(i - 1); }
            count++;
        }
    }
    if (count != deg) return -1;
    // error evaluator (:370-399)
    int om[10], deg_omega = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        int tmp = 0;
#pragma unroll
        for (int j = i; j >= 0; j--) {
            if (j <= deg) {
                const int a = g.log[syn[i - j]];
                if (a != RS_NN && LL[j] != RS_NN) tmp ^= g.exp[mod255(a + LL[j])];
            }
        }
        if (tmp) deg_omega = i;
        om[i] = g.log[tmp];
    }
    // Forney (:183-227)
    const int dmax = (deg < 9 ? deg : 9) & ~1;
    int nf = 0;
    for (int jj = count - 1; jj >= 0; jj--) {
        const int r = roots[jj], loc = locs[jj];
        int num1 = 0;
#pragma unroll
        for (int i = 0; i < 10; i++)
            if (i <= deg_omega && om[i] != RS_NN) num1 ^= g.exp[mod255(om[i] + (i ? (i * r) % RS_NN : 0))];
        const int num2 = g.exp[(r * 254) % RS_NN];
        int den = 0;
#pragma unroll
        for (int i = 0; i <= 8; i += 2)
            if (i <= dmax && LL[i + 1] != RS_NN) den ^= g.exp[mod255(LL[i + 1] + (i ? (i * r) % RS_NN : 0))];
        if (den == 0) {
            *nfix = nf;                                  // corrections made before the failure stay
            return -1;
        }
        if (num1 != 0) {
            if (loc >= RS_NN - 10) {
                count--;
            } else {
                int c = mod255(g.log[num1] + g.log[num2]);
                c = mod255(c + RS_NN - g.log[den]);
                fix_pos[nf] = (uint8_t)loc;
                fix_val[nf] = g.exp[c];
                nf++;
            }
        }
    }
    *nfix = nf;
    return count;
}

// firecode_checker::check (firecode-checker.cpp:76-94) on 11 bytes
__device__ __forceinline__ bool fire_ok(const uint32_t (&x)[11], const uint16_t *fire) {
    uint32_t st = (x[2] << 8) | x[3];
#pragma unroll
    for (int i = 4; i < 13; i++) {
        const uint32_t b = i < 11 ? x[i] : x[i - 11];     // bytes 4..10 then 0..1
        const uint32_t is = fire[st >> 8];
        st = ((is & 0xffu) ^ b) | ((is ^ (st << 8)) & 0xff00u);
    }
    return st == 0;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Byte p of the superframe candidate ending at CIF cl of this run: the 5 blocks
// cl-4..cl in delivery order, i.e. the reference's ring read from its oldest block
// (mp4processor.cpp:128-140).  Blocks before the run come from the carry (the
// previous run's last 4 CIFs, oldest first).
__device__ __forceinline__ uint32_t window_byte(const DpJob &J, const uint8_t *carry, int stream, int sub,
                                                int nbytes, int cl, int p) {
    const int b = p / nbytes, w = p - b * nbytes, q = cl - 4 + b;
    if (q < 0) return carry[(q + 4) * nbytes + w];
    return row_byte(msc_row(J.feed, stream, q, sub), J.feed.packed, w);
}

// Bytes 4d .. 4d+3 of the same window as one little-endian word (packed MSC with 4-byte
// aligned rows: a CIF block is 3 * bitRate bytes, a multiple of 24, so no word straddles two)
__device__ __forceinline__ uint32_t window_word(const DpJob &J, const uint8_t *carry, int stream, int sub,
                                                int nbytes, int cl, int d) {
    const int p = 4 * d, b = p / nbytes, w = p - b * nbytes, q = cl - 4 + b;
    if (q < 0) return *(const uint32_t *)(carry + (q + 4) * nbytes + w);
    return *(const uint32_t *)(msc_row(J.feed, stream, q, sub) + w);
}
__device__ __forceinline__ bool words_ok(const DpJob &J) {
    return J.feed.packed && (((uintptr_t)J.feed.msc | (uintptr_t)J.feed.msc_stride | (uintptr_t)J.ring) & 3) == 0;
}
// the window's fsz bytes into LDS: every load of a lane in flight before its first store
// (a load-store pair per byte would wait out one memory round trip per byte)
__device__ __forceinline__ void window_to_lds(const DpJob &J, const uint8_t *carry, int stream, int sub, int nbytes,
                                              int cl, int fsz, uint8_t *dst, int lane) {
    if (words_ok(J)) {
        const int nw = fsz >> 2;                         // fsz = 120 RS: a multiple of 4
        uint32_t *d32 = (uint32_t *)dst;
        for (int d0 = 0; d0 < nw; d0 += 8 * 64) {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int d = d0 + 64 * k + lane;
                v[k] = d < nw ? window_word(J, carry, stream, sub, nbytes, cl, d) : 0u;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int d = d0 + 64 * k + lane;
                if (d < nw) d32[d] = v[k];
            }
        }
        return;
    }
    for (int p0 = 0; p0 < fsz; p0 += 8 * 64) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int p = p0 + 64 * k + lane;
            v[k] = p < fsz ? window_byte(J, carry, stream, sub, nbytes, cl, p) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int p = p0 + 64 * k + lane;
            if (p < fsz) dst[p] = (uint8_t)v[k];
        }
    }
}

// processSuperframe (mp4processor.cpp:146-292) of the candidate window ending at CIF cl of
// (stream, DAB+ subchannel) sd, by one wave: RS(120,110) over the RSDims columns, the AU
// table and AU CRCs.  The verdict (2 rejected, 3 decoded) goes to J.code, the record and,
// for a decoded one, the corrected bytes to their slots.  The work is spread over the
// wave: syndromes as direct sums (lane = column x a slice of its rows), Berlekamp-Massey/
// Chien/Forney one column per lane, each AU CRC in 64 slices joined by x^(8d) shifts (the
// CRC is linear).
// LDS: sfb [120 * DP_MAX_RS], syn_s [10 * DP_MAX_RS], rl [64 * 40], red [64] of the wave.
__device__ void sf_decode(const DpJob &J, const GfTabs &g, int sd, int cl, uint8_t *sfb, uint32_t *syn_s,
                          uint8_t *rl, int32_t *red, int lane) {
    const int stream = sd / J.ndp, dp = sd - stream * J.ndp;
    const int br = J.map.br[sd], sub = J.map.sub[sd];
    const int RS = br / 8, nbytes = 3 * br, fsz = 120 * RS, end = 110 * RS;
    uint8_t *code = J.code + (int64_t)sd * J.feed.ncif + cl;
    const uint8_t *carry = J.ring + (int64_t)sd * (120 * DP_MAX_RS);
    window_to_lds(J, carry, stream, sub, nbytes, cl, fsz, sfb, lane);
    for (int p = lane; p < 10 * RS; p += 64) syn_s[p] = 0;
    wave_sync();
    // syndromes S_i = sum_m r_m alpha^(i (119-m)) per column: the Horner sums of
    // reed-solomon.cpp:231-266 (roots alpha^0..alpha^9, the 135 zero pad bytes
    // contribute nothing).  Lane -> column lane % RS, rows lane / RS + k * (64 / RS).
    const int per = 64 / RS;
    if (lane < per * RS) {
        const int j = lane % RS;
        uint32_t acc[10];
#pragma unroll
        for (int i = 0; i < 10; i++) acc[i] = 0;
        for (int m = lane / RS; m < 120; m += per) {
            const int r = sfb[j + m * RS];
            if (r) {
                const int t = 119 - m;
                int e = g.log[r];
                acc[0] ^= g.exp[e];
#pragma unroll
                for (int i = 1; i < 10; i++) {
                    e += t;
                    if (e >= RS_NN) e -= RS_NN;
                    acc[i] ^= g.exp[e];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 10; i++)
            if (acc[i]) atomicXor(&syn_s[10 * j + i], acc[i]);
    }
    wave_sync();
    int ler = 0;
    if (lane < RS) {                                     // one column per lane
        int sy[10];
#pragma unroll
        for (int i = 0; i < 10; i++) sy[i] = (int)syn_s[10 * lane + i];
        uint8_t *w = rl + lane * 40;
        int nf = 0;
        ler = rs_solve(sy, g, w, w + 10, w + 20, w + 30, &nf);
        for (int f = 0; f < nf; f++) {
            const int m = w[20 + f] - RS_PAD;
            if (m >= 0 && m < 110) sfb[lane + m * RS] ^= w[30 + f];
        }
    }
    red[lane] = ler;
    wave_sync();
    // the reference stops at the first failing column
    int nerr = 0, fail = 0;
    for (int j = 0; j < RS && !fail; j++) {
        const int l = red[j];
        if (l > 0) nerr += l;
        if (l < 0) fail = 1;
    }
    dabgpu_superframe info;
    info.status = 2;
    info.num_aus = 0;
    info.n_corrected = (int16_t)nerr;
    for (int i = 0; i < 7; i++) info.au_start[i] = 0;
    info.au_crc_ok = 0;
    info.reserved = 0;
    bool ok = !fail;
    if (ok) {
        // AU table (:181-233)
        const int dac = (sfb[2] >> 6) & 1, sbr = (sfb[2] >> 5) & 1;
        int n, a[7];
        switch (2 * dac + sbr) {
        default:
        case 0: n = 4; a[0] = 8; a[1] = sfb[3] * 16 + (sfb[4] >> 4);
            a[2] = (sfb[4] & 0xf) * 256 + sfb[5]; a[3] = sfb[6] * 16 + (sfb[7] >> 4); a[4] = end; break;
        case 1: n = 2; a[0] = 5; a[1] = sfb[3] * 16 + (sfb[4] >> 4); a[2] = end; break;
        case 2: n = 6; a[0] = 11; a[1] = sfb[3] * 16 + (sfb[4] >> 4);
            a[2] = (sfb[4] & 0xf) * 256 + sfb[5]; a[3] = sfb[6] * 16 + (sfb[7] >> 4);
            a[4] = (sfb[7] & 0xf) * 256 + sfb[8]; a[5] = sfb[9] * 16 + (sfb[10] >> 4); a[6] = end; break;
        case 3: n = 3; a[0] = 6; a[1] = sfb[3] * 16 + (sfb[4] >> 4);
            a[2] = (sfb[4] & 0xf) * 256 + sfb[5]; a[3] = end; break;
        }
        info.num_aus = (int8_t)n;
        for (int i = 0; i < 7; i++) info.au_start[i] = (int16_t)(i <= n ? a[i] : 0);
        int bad = n;                                     // first AU with an impossible layout
        for (int i = 0; i < n; i++) {
            const int len = a[i + 1] - a[i] - 2;
            if (a[i + 1] < a[i] || len >= 960 || len < 0) { bad = i; break; }
        }
        // dabPlus_crc (mp4processor.cpp:40-61) of AU i over [a[i], a[i+1]): lane l
        // runs the table CRC over its slice (lane 0 from the 0xFFFF preset, the others
        // from 0), shifts it past the bytes after the slice, and the slices XOR
        // together.  Bytes past the superframe read as zero.
        uint32_t mask = 0;
        for (int i = 0; i < bad; i++) {
            const int ai = a[i], len = a[i + 1] - ai - 2, limit = end - ai;
            const int cs = (len + 63) >> 6;
            const int k0 = min(len, lane * cs), k1 = min(len, k0 + cs);
            uint32_t acc = lane == 0 ? 0xFFFFu : 0u;
            for (int k = k0; k < k1; k++) {
                const uint32_t b = k < limit ? sfb[ai + k] : 0u;
                acc = ((acc << 8) ^ g.crc[((acc >> 8) ^ b) & 0xFFu]) & 0xFFFFu;
            }
            if (acc) acc = crc16::mulmod(acc, g.pow8[len - k1]);
            acc = wave_xor(acc);
            const uint32_t hi = len < limit ? sfb[ai + len] : 0u, lo = len + 1 < limit ? sfb[ai + len + 1] : 0u;
            if (((~((hi << 8) | lo) & 0xFFFFu) ^ acc) == 0) mask |= 1u << i;
        }
        info.au_crc_ok = (uint8_t)(mask & 0x3F);
        ok = bad == n;
    }
    if (ok) {
        info.status = 3;
        uint8_t *o = J.sf_out + (((int64_t)stream * J.feed.ncif + cl) * J.ndp + dp) * J.sf_stride;
        for (int i = lane; i < end; i += 64) o[i] = sfb[i];
    }
    if (lane == 0) {
        J.info[((int64_t)stream * J.feed.ncif + cl) * J.ndp + dp] = info;
        *code = (uint8_t)info.status;
    }
}

// The superframe state machine of addtoFrame (mp4processor.cpp:107-145) over the run's
// CIFs of sd, by one wave: blocksInBuffer decides which candidates the reference
// evaluates; their verdicts are in J.code.  Writes the records of the CIFs without an
// evaluated superframe, the state, and the carry (the run's last 4 CIFs as bytes) for
// the next run.  nc: LDS [4 * 3 * 384]
__device__ void dp_walk(const DpJob &J, int sd, uint8_t *nc, int lane) {
    const int stream = sd / J.ndp, dp = sd - stream * J.ndp;
    const int br = J.map.br[sd], sub = J.map.sub[sd], nbytes = 3 * br;
    if (sub < 0) {                                       // absent slot: status -1 records, no state
        for (int cl = lane; cl < J.feed.ncif; cl += 64) {
            dabgpu_superframe info;
            info.status = -1;
            info.num_aus = 0;
            info.n_corrected = 0;
            for (int i = 0; i < 7; i++) info.au_start[i] = 0;
            info.au_crc_ok = 0;
            info.reserved = J.sf_compact ? 0xFF : 0;
            J.info[((int64_t)stream * J.feed.ncif + cl) * J.ndp + dp] = info;
        }
        return;
    }
    DpState st = J.state[sd];
    const uint8_t *code = J.code + (int64_t)sd * J.feed.ncif;
    const int nd = J.feed.ncifs[stream];                // CIFs this stream delivered
    const int64_t rel0 = rel_cif(J.feed, J.map, sd, stream);
    for (int c0 = 0; c0 < J.feed.ncif; c0 += 64) {
        const int cl = c0 + lane;
        const int v = cl < J.feed.ncif ? code[cl] : 0;
        int fs = 0;
        const int nc = min(64, J.feed.ncif - c0);
        for (int i = 0; i < nc; i++) {                  // uniform
            int s;
            if (!fed(sub, nd, rel0, c0 + i)) {
                s = -1;                                  // not delivered (warm-up, or past the stream's CIFs)
            } else {
                st.blocks++;
                st.fill = (st.fill + 1) % 5;
                s = 0;
                if (st.blocks >= 5) {
                    const int cd = __builtin_amdgcn_readlane(v, i);
                    s = cd == 0 ? 1 : cd;
                    st.blocks = cd == 3 ? 0 : 4;
                }
            }
            if (lane == i) fs = s;
        }
        if (cl < J.feed.ncif && fs < 2) {
            dabgpu_superframe info;
            info.status = (int8_t)fs;
            info.num_aus = 0;
            info.n_corrected = 0;
            for (int i = 0; i < 7; i++) info.au_start[i] = 0;
            info.au_crc_ok = 0;
            info.reserved = 0;
            J.info[((int64_t)stream * J.feed.ncif + cl) * J.ndp + dp] = info;
        }
    }
    // carry = the stream's last 4 delivered CIFs (oldest first); with fewer than 4 new
    // ones the older part comes from the previous carry (staged: it is overwritten)
    uint8_t *carry = J.ring + (int64_t)sd * (120 * DP_MAX_RS);
    for (int p0 = 0; p0 < 4 * nbytes; p0 += 8 * 64) {    // a lane's loads in flight together
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int p = p0 + 64 * k + lane;
            v[k] = 0;
            if (p < 4 * nbytes) {
                const int b = p / nbytes, w = p - b * nbytes, q = nd - 4 + b;
                v[k] = q >= 0 ? row_byte(msc_row(J.feed, stream, q, sub), J.feed.packed, w) : carry[(q + 4) * nbytes + w];
            }
        }
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (p0 + 64 * k + lane < 4 * nbytes) nc[p0 + 64 * k + lane] = (uint8_t)v[k];
    }
    wave_sync();
    for (int p = lane; p < 4 * nbytes; p += 64) carry[p] = nc[p];
    if (lane == 0) J.state[sd] = st;
}

// The whole layer for one (stream, DAB+ subchannel) in one workgroup of DP_WAVES waves.
// Fire: one thread per CIF checks the fire code at the oldest block of the 5-CIF window
// ending at that CIF (firecode-checker.cpp:76-94); a window that holds an undelivered CIF
// or fails is marked 0 in J.code, a passing one (about one CIF in five once the
// superframes are aligned) is marked 1 and listed in LDS.  Decode: the waves take the
// listed candidates in turn (sf_decode).  Walk: which candidates the reference actually
// evaluates depends on the superframe state (dp_walk); the workgroup's own verdicts are all
// it reads, so the kernel has no grid-wide step and the GF tables are loaded once per
// workgroup.
// The list holds DP_LIST CIFs.  A launch runs the fire and decode phases over the CIFs
// [c0, c1) of the run, at most DP_LIST, and the launch of the run's last CIFs (`last`) then
// walks the whole run: a run of up to 512 frames is one launch, a longer one takes one per
// DP_LIST CIFs (launch_dabplus), the earlier launches' verdicts waiting in J.code.  (The same
// blocks as a loop inside one launch measured 7 % slower for the usual single block, 0.099
// against 0.092 ms for C5 alone: profiles/kernel_forms_ab.txt.)
constexpr int DP_WAVES = 8;
constexpr int DP_LIST = 4 * 512;            // CIFs per launch of the fire and decode phases
__global__ __launch_bounds__(64 * DP_WAVES) void k_dp_layer(DpJob J, int c0, int c1, int last) {
    __shared__ __attribute__((aligned(16))) GfTabs g;
    __shared__ __attribute__((aligned(16))) uint8_t sfb[DP_WAVES][120 * DP_MAX_RS];
    __shared__ uint32_t syn_s[DP_WAVES][10 * DP_MAX_RS];
    __shared__ uint8_t rl[DP_WAVES][64 * 40];
    __shared__ int32_t red[DP_WAVES][64];
    __shared__ int16_t list[DP_LIST];                    // the passing CIFs, relative to c0
    __shared__ int32_t nlist;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, sd = blockIdx.x;
    const int stream = sd / J.ndp, dp = sd - stream * J.ndp;
    const int br = J.map.br[sd], sub = J.map.sub[sd], nbytes = 3 * br;
    if (sub < 0) {                                       // absent slot (the whole workgroup): status -1 records
        if (w == 0 && last) dp_walk(J, sd, sfb[1], lane);
        return;
    }
    const int nfed = J.feed.ncifs[stream];
    const int64_t rel0 = rel_cif(J.feed, J.map, sd, stream);
    const uint32_t *tabs32 = (const uint32_t *)J.tabs;
    for (int i = t; i < (int)sizeof(GfTabs) / 4; i += 64 * DP_WAVES) ((uint32_t *)&g)[i] = tabs32[i];
    if (t == 0) nlist = 0;
    __syncthreads();
    const uint8_t *carry = J.ring + (int64_t)sd * (120 * DP_MAX_RS);
    for (int cl = c0 + t; cl < c1; cl += 64 * DP_WAVES) {
        // a window holding an undelivered CIF (de-interleaver warm-up, or a CIF slot the
        // stream did not fill in this run) is never evaluated: its CIFs are delivered when
        // its newest and its oldest are
        bool ok = fed(sub, nfed, rel0, cl) && fed(sub, nfed, rel0, cl - 4);
        if (ok) {
            uint32_t x[11];
#pragma unroll
            for (int p = 0; p < 11; p++) x[p] = window_byte(J, carry, stream, sub, nbytes, cl, p);
            ok = fire_ok(x, g.fire);
        }
        J.code[(int64_t)sd * J.feed.ncif + cl] = ok ? 1 : 0;
        if (ok) list[atomicAdd(&nlist, 1)] = (int16_t)(cl - c0);
    }
    __syncthreads();
    const int nc = nlist;
    for (int ci = w; ci < nc; ci += DP_WAVES) {
        sf_decode(J, g, sd, c0 + list[ci], sfb[w], syn_s[w], rl[w], red[w], lane);
        wave_sync();                                     // this wave's LDS reads are done
    }
    if (!last) return;
    __syncthreads();                                     // every verdict of sd written (J.code)
    if (w == 0) dp_walk(J, sd, sfb[1], lane);            // (the carry staging reuses an idle stage)
    if (!J.sf_compact) return;
    // compact output: the run's decoded superframes of sd in CIF order (after the walk,
    // status 3 marks exactly the ones the reference evaluated and decoded), slot k of the
    // k-th; the record's `reserved` byte carries k (0xFF: not stored).  The list now holds
    // their CIFs (c0 = 0: launch_dabplus refuses a compact run past DP_LIST CIFs)
    __syncthreads();                                     // the walk's records are written
    if (w == 0) {
        int k = 0;
        for (int c0 = 0; c0 < J.feed.ncif; c0 += 64) {
            const int cl = c0 + lane;
            dabgpu_superframe *r = cl < J.feed.ncif ? &J.info[((int64_t)stream * J.feed.ncif + cl) * J.ndp + dp] : nullptr;
            const bool dec = r && r->status == 3;
            const uint64_t bal = __ballot(dec);
            const int kk = k + __popcll(bal & ((1ull << lane) - 1ull));
            if (dec) {
                r->reserved = (uint8_t)(kk < J.kmax ? kk : 0xFF);
                if (kk < J.kmax) list[kk] = (int16_t)cl;
            } else if (r) {
                r->reserved = 0xFF;
            }
            k += __popcll(bal);
        }
        if (lane == 0) nlist = k < J.kmax ? k : J.kmax;
    }
    __syncthreads();
    const int nk = nlist, end = 110 * (br / 8);
    for (int q = w; q < nk; q += DP_WAVES) {             // a wave per superframe, a byte per lane
        const uint8_t *src = J.sf_out + (((int64_t)stream * J.feed.ncif + list[q]) * J.ndp + dp) * J.sf_stride;
        uint8_t *dst = J.sf_compact + ((int64_t)sd * J.kmax + q) * J.sf_stride;
        for (int i = lane; i < end; i += 64) dst[i] = src[i];
    }
}

hipError_t launch_dabplus(hipStream_t st, const DpJob &job) {
    if (job.ndp <= 0 || job.feed.nstreams <= 0) return hipSuccess;
    const int ncif = job.feed.ncif;
    if (ncif < 4) return hipErrorInvalidValue;            // the carry holds the last 4 CIFs
    if (job.sf_compact && ncif > DP_LIST) return hipErrorInvalidValue;   // the list holds the run's superframes
    for (int c0 = 0; c0 < ncif; c0 += DP_LIST) {
        const int c1 = c0 + DP_LIST < ncif ? c0 + DP_LIST : ncif;
        hipLaunchKernelGGL(k_dp_layer, dim3(job.feed.nstreams * job.ndp), dim3(64 * DP_WAVES), 0, st, job, c0, c1,
                           c1 == ncif ? 1 : 0);
    }
    return hipGetLastError();
}

// reedSolomon::dec batched: one lane per codeword (the a19 operator on its own).
__global__ __launch_bounds__(64) void k_rs(const uint8_t *__restrict__ in, int n, const uint8_t *__restrict__ tabs,
                                          uint8_t *__restrict__ out, int16_t *__restrict__ ret) {
    __shared__ GfTabs g;
    __shared__ uint8_t rows[64 * RS_ROW];
    __shared__ uint8_t rl[64 * 40];
    const int lane = threadIdx.x, cw = blockIdx.x * 64 + lane;
    for (int i = lane; i < (int)sizeof(GfTabs); i += 64) ((uint8_t *)&g)[i] = tabs[i];
    wave_sync();
    if (cw >= n) return;
    uint8_t *row = rows + lane * RS_ROW;
    for (int k = 0; k < 120; k++) row[k] = in[(int64_t)cw * 120 + k];
    int sy[10];
#pragma unroll
    for (int i = 0; i < 10; i++) sy[i] = rs_syndrome(row, i, g);
    uint8_t *w = rl + lane * 40;
    int nf = 0;
    const int r = rs_solve(sy, g, w, w + 10, w + 20, w + 30, &nf);
    for (int f = 0; f < nf; f++) {
        const int m = w[20 + f] - RS_PAD;
        if (m >= 0) row[m] ^= w[30 + f];
    }
    for (int k = 0; k < 110; k++) out[(int64_t)cw * 110 + k] = row[k];
    ret[cw] = (int16_t)r;
}

hipError_t launch_rs(hipStream_t st, const uint8_t *in, int n, const uint8_t *tabs, uint8_t *out, int16_t *ret) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rs, dim3((n + 63) / 64), dim3(64), 0, st, in, n, tabs, out, ret);
    return hipGetLastError();
}

}  // namespace dab
