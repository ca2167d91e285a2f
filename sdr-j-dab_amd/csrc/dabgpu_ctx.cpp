// dabgpu_ctx.cpp -- the C ABI (include/dabgpu.h), first half: errors, host tables, the
// context and the batched operators (the streaming pipeline is dabgpu_pipe.cpp).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <string>
#include <memory>
#include <algorithm>
#include "dabgpu_internal.h"
#include "../host/audio_fir.h"
#include "../host/rate_converter.h"
#include "stage_layout.h"
#include "dab_tables.h"

using namespace dab;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int dab::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ------------------------------------------------------------- host tables
namespace {

constexpr int M = 2048000;


// Mode-I phase reference rows (k_min, i, n), k_max = k_min + 31 (phasetable.cpp:115-166)
const int16_t kPhi[48][3] = {
    {-768,0,1},{-736,1,2},{-704,2,0},{-672,3,1},{-640,0,3},{-608,1,2},{-576,2,2},{-544,3,3},
    {-512,0,2},{-480,1,1},{-448,2,2},{-416,3,3},{-384,0,1},{-352,1,2},{-320,2,3},{-288,3,3},
    {-256,0,2},{-224,1,2},{-192,2,2},{-160,3,1},{-128,0,1},{ -96,1,3},{ -64,2,1},{ -32,3,2},
    {   1,0,3},{  33,3,1},{  65,2,1},{  97,1,1},{ 129,0,2},{ 161,3,2},{ 193,2,1},{ 225,1,0},
    { 257,0,2},{ 289,3,2},{ 321,2,3},{ 353,1,3},{ 385,0,0},{ 417,3,2},{ 449,2,1},{ 481,1,3},
    { 513,0,3},{ 545,3,3},{ 577,2,3},{ 609,1,0},{ 641,0,3},{ 673,3,0},{ 705,2,1},{ 737,1,1}};
const int8_t kHpar[4][16] = {
    {0,2,0,0,0,0,1,1,2,0,0,0,2,2,1,1},
    {0,3,2,3,0,1,3,0,2,1,2,3,2,3,3,0},
    {0,0,0,2,0,2,1,3,2,2,0,2,2,0,1,3},
    {0,1,2,1,0,3,3,2,2,3,2,1,2,1,3,2}};

float get_phi(int k) {                                   // phasetable.cpp:261-274 (float result)
    for (auto &r : kPhi)
        if (r[0] <= k && k <= r[0] + 31) return (float)(M_PI / 2 * (kHpar[r[1]][(k - r[0]) & 15] + r[2]));
    return 0.0f;
}

struct HostTables {
    std::vector<float2> osc;
    std::vector<double2> nco;               // factor tables of the NCO (dab_kernels.h)
    std::vector<uint32_t> prbs_words;
    std::vector<float2> w2048;
    std::vector<int16_t> carrier_bin;
    bool stage_ok = true;
    std::vector<float> refarg;
    std::vector<float2> ref;                // natural order refTable
    std::vector<int16_t> perm;              // carrier -> signed carrier (mapIn)
    HostTables() {
#pragma clang fp contract(off)
        osc.resize(M);
        for (int i = 0; i < M; i++)          // ofdm-processor.cpp:79-81
            osc[i] = make_float2((float)cos(2.0 * M_PI * i / M), (float)sin(2.0 * M_PI * i / M));
        nco.assign(NCO_N, make_double2(0.0, 0.0));
        for (int k = 0; k < 128; k++) nco[NCO_A + k] = make_double2(cos(2.0 * M_PI * k / 128), sin(2.0 * M_PI * k / 128));
        for (int k = 0; k < 125; k++)
            nco[NCO_B + k] = make_double2(cos(2.0 * M_PI * k / 16000), sin(2.0 * M_PI * k / 16000));
        for (int k = 0; k < 128; k++) nco[NCO_C + k] = make_double2(cos(2.0 * M_PI * k / M), sin(2.0 * M_PI * k / M));
        ref.assign(2048, make_float2(0.0f, 0.0f));
        for (int i = 1; i <= 768; i++) {      // phasereference.cpp:42-47
            float phi = get_phi(i);
            ref[i] = make_float2(cosf(phi), sinf(phi));
            phi = get_phi(-i);
            ref[2048 - i] = make_float2(cosf(phi), sinf(phi));
        }
        // mapper.cpp:33-55 (Mode I: V1 = 511, [256, 1792] \ {1024})
        int16_t seq[2048];
        seq[0] = 0;
        for (int i = 1; i < 2048; i++) seq[i] = (int16_t)((13 * seq[i - 1] + 511) % 2048);
        for (int i = 0; i < 2048; i++) {
            int v = seq[i];
            if (v == 1024 || v < 256 || v > 256 + 1536) continue;
            perm.push_back((int16_t)(v - 1024));
        }
        std::vector<int> carrier_of_bin(2048, -1);
        for (int c = 0; c < 1536; c++) { int k = perm[c]; carrier_of_bin[k < 0 ? k + 2048 : k] = c; }
        // k_demod: carrier of each FFT bin [2048], then the soft-bit stage words of the
        // bins [2048] and of the carrier pairs [768] (stage_layout.h)
        carrier_bin.assign(2048 + 2048 + 768, -1);
        for (int b = 0; b < 2048; b++) carrier_bin[b] = (int16_t)carrier_of_bin[b];
        {
            int rank[32] = {};
            std::vector<int> sig(768);
            for (int p = 0; p < 768; p++) sig[p] = 32 * rank[STAGE_COL[p]]++ + STAGE_COL[p];
            for (int r : rank) stage_ok = stage_ok && r == 24;        // a permutation of the 1536 words
            for (int p = 0; p < 768; p++) carrier_bin[4096 + p] = (int16_t)(2 * sig[p]);
            // a carrier's word: its pair's, even carrier first; the demod stores carriers only
            // (the other bins keep -1)
            for (int b = 0; b < 2048; b++) {
                const int c = carrier_of_bin[b];
                if (c >= 0) carrier_bin[2048 + b] = (int16_t)(2 * sig[c >> 1] + (c & 1));
            }
        }
        w2048.resize(2048);                    // k_demod twiddles
        for (int j = 0; j < 2048; j++) {
            const double ph = -2.0 * M_PI * j / 2048.0;
            w2048[j] = make_float2((float)cos(ph), (float)sin(ph));
        }
        refarg.resize(18);
        for (int i = 0; i < 18; i++) {        // ofdm-decoder.cpp:71-74
            float2 a = ref[(2048 + i) % 2048], b = ref[(2048 + i + 1) % 2048];
            float nb = -b.y;
            float ac = a.x * b.x, bd = a.y * nb, ad = a.x * nb, bc = a.y * b.x;
            float re = ac - bd, im = ad + bc;
            refarg[i] = atan2f(im, re);
        }
        // energy dispersal (fic-handler.cpp:100-108; dab-concurrent.cpp:183-190 runs the same
        // register for 24 * bitRate bits): PRBS_WORDS words, the longest subchannel's
        prbs_words.assign(PRBS_WORDS, 0u);
        uint8_t sr[9];
        memset(sr, 1, 9);
        for (int i = 0; i < 32 * PRBS_WORDS; i++) {
            uint8_t b = sr[8] ^ sr[4];
            for (int j = 8; j > 0; j--) sr[j] = sr[j - 1];
            sr[0] = b;
            if (b) prbs_words[i >> 5] |= 1u << (i & 31);
        }
        // DAB+ tables: GF(2^8) with poly 0435 (galois.cpp:33-63, mp4processor.cpp:74)
        // and the fire-code syndrome table (firecode-checker.cpp:31-74)
        dptab.assign(DP_TAB_BYTES, 0);
        uint8_t *gexp = dptab.data(), *glog = dptab.data() + 256;
        glog[0] = 255;
        gexp[255] = 0;
        for (int i = 0, sr = 1; i < 255; i++) {
            glog[sr] = (uint8_t)i;
            gexp[i] = (uint8_t)sr;
            sr <<= 1;
            if (sr & 256) sr ^= 0435;
            sr &= 255;
        }
        static const uint8_t fg[16] = {1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0};
        uint16_t itab[8];
        for (int i = 0; i < 8; i++) {
            uint8_t regs[16] = {};
            regs[8 + i] = 1;
            for (int r = 0; r < 8; r++) {
                const uint8_t z = regs[15];
                for (int j = 15; j > 0; j--) regs[j] = regs[j - 1] ^ (z & fg[j]);
                regs[0] = z;
            }
            uint16_t v = 0;
            for (int j = 15; j >= 0; j--) v = (uint16_t)((v << 1) | regs[j]);
            itab[i] = v;
        }
        uint16_t *fire = (uint16_t *)(dptab.data() + 512);
        for (int i = 0; i < 256; i++) {
            uint16_t v = 0;
            for (int j = 0; j < 8; j++) if (i & (1 << j)) v ^= itab[j];
            fire[i] = v;
        }
        uint8_t *mul = dptab.data() + 1024;            // mul[i][s] = s * alpha^i
        for (int i = 0; i < 10; i++)
            for (int v = 0; v < 256; v++) mul[i * 256 + v] = v ? gexp[(glog[v] + i) % 255] : 0;
        uint16_t *crc = (uint16_t *)(dptab.data() + 1024 + 2560);   // CRC-CCITT, msb first
        for (int b = 0; b < 256; b++) {
            uint32_t c = (uint32_t)b << 8;
            for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) : (c << 1);
            crc[b] = (uint16_t)(c & 0xFFFFu);
        }
        // x^(8d) mod the CRC polynomial: shifts a partial CRC past d bytes
        uint16_t *pow8 = (uint16_t *)(dptab.data() + 1024 + 2560 + 512);
        pow8[0] = 1;
        for (int d = 1; d < 1024; d++)
            pow8[d] = (uint16_t)(((uint32_t)pow8[d - 1] << 8) ^ crc[pow8[d - 1] >> 8]);
        // FIB CRC (dab-constants.h:310-340) by linearity: the register after 256 bits is
        // the XOR of each 1 bit's contribution (a lone 1 at position i, zeros after) and
        // of the all-ones initial value's (256 zero bits): k_fic_post reduces it over a wave
        uint16_t *fc = (uint16_t *)(dptab.data() + FIBCRC_OFF);
        auto run = [](uint32_t r, int one_at) {
            for (int i = 0; i < 256; i++) {
                const uint32_t top = (r >> 15) & 1u;
                r = (r << 1) & 0xFFFFu;
                if (top ^ (uint32_t)(i == one_at)) r ^= 0x1021u;
            }
            return (uint16_t)r;
        };
        for (int i = 0; i < 256; i++) fc[i] = run(0, i);
        fc[256] = run(0xFFFF, -1);
    }
    std::vector<uint8_t> dptab;             // GF exp[256], log[256], fire uint16[256]
};
const HostTables &host_tables() {
    static HostTables t;
    return t;
}

}  // namespace

// depuncturing profile of a subchannel (deconvolve.cpp:142-366)
int dab::make_profile(const dabgpu_subch &s, Profile &p) {
    memset(&p, 0, sizeof p);
    int Ls[4] = {0, 0, 0, 0}, PIs[4] = {0, 0, 0, 0}, nseg = 0;
    const int br = s.bitRate;
    if (s.uepFlag == 0) {
        int idx = -1;
        for (int i = 0; i < kNumUep; i++)
            if (kUepProfiles[i][0] == br && kUepProfiles[i][1] == s.protLevel) { idx = i; break; }
        if (idx < 0) idx = 1;               // deconvolve.cpp:150-153 fallback
        for (int j = 0; j < 4; j++) { Ls[j] = kUepProfiles[idx][2 + j]; PIs[j] = kUepProfiles[idx][6 + j]; }
        nseg = 4;
    } else {
        const int lvl = s.protLevel & 7;
        if (s.protLevel & 0100) {
            switch (lvl) {
            case 1: Ls[0] = 6 * br / 8 - 3; Ls[1] = 3; PIs[0] = 24; PIs[1] = 23; break;
            case 2: if (br == 8) { Ls[0] = 5; Ls[1] = 1; PIs[0] = 13; PIs[1] = 12; }
                    else { Ls[0] = 2 * br / 8 - 3; Ls[1] = 4 * br / 8 + 3; PIs[0] = 14; PIs[1] = 13; } break;
            case 3: Ls[0] = 6 * br / 8 - 3; Ls[1] = 3; PIs[0] = 8; PIs[1] = 7; break;
            case 4: Ls[0] = 4 * br / 8 - 3; Ls[1] = 2 * br / 8 + 3; PIs[0] = 3; PIs[1] = 2; break;
            default: return -1;
            }
        } else if (s.protLevel & 0200) {
            Ls[0] = 24 * br / 32 - 3; Ls[1] = 3;
            switch (lvl) {
            case 4: PIs[0] = 2; PIs[1] = 1; break;
            case 3: PIs[0] = 4; PIs[1] = 3; break;
            case 2: PIs[0] = 6; PIs[1] = 5; break;
            case 1: PIs[0] = 10; PIs[1] = 9; break;
            default: return -1;
            }
        } else {
            return -1;                       // protection not defined by the reference
        }
        nseg = 2;
    }
    p.nbits = 24 * br;
    // drop empty segments, keep order
    int ns = 0, blk = 0, in = 0;
    for (int j = 0; j < nseg; j++) {
        if (Ls[j] <= 0) continue;
        uint32_t m = pcode_mask(PIs[j]);
        p.mask[ns] = m;
        p.in_base[ns] = in;
        blk += Ls[j];
        in += Ls[j] * 4 * __builtin_popcount(m);
        p.blk_end[ns] = blk;
        ns++;
    }
    p.nseg = ns;
    p.in_base[ns] = in;
    p.tail_mask = kPiXMask;
    p.frag = in + 12;
    // an unknown UEP (bitRate, level) falls back to row 1 (deconvolve.cpp:150-153): its
    // blocks then cover fewer than 4*nbits mother bits and the rest stays zero
    if (blk * 128 > 4 * p.nbits) return -2;
    return 0;
}

Profile dab::fic_profile() {                      // fic-handler.cpp:254-288
    Profile p;
    memset(&p, 0, sizeof p);
    p.nbits = 768;
    p.nseg = 2;
    p.mask[0] = pcode_mask(16);
    p.mask[1] = pcode_mask(15);
    p.blk_end[0] = 21;
    p.blk_end[1] = 24;
    p.in_base[0] = 0;
    p.in_base[1] = 21 * 4 * 24;
    p.in_base[2] = p.in_base[1] + 3 * 4 * 23;
    p.tail_mask = kPiXMask;
    p.frag = 2304;
    return p;
}

// Inverse depuncturing table of a profile: the mother-code position q = 4 * step + e of
// each punctured input, in input order (the same rule as the kernels' idx4 /
// in_index: PI masks per 128-bit block, then the 24-bit PI_X tail, deconvolve.cpp:172-237),
// stored as its position within the ACS tile holding it (q mod VIT_TILE_POS < 240: one
// byte, and the tile loader scatters with no offset arithmetic)
std::vector<uint8_t> dab::make_inv(const Profile &P) {
    std::vector<uint8_t> inv;
    inv.reserve(P.frag);
    const int last_end = P.nseg ? P.blk_end[P.nseg - 1] : 0;
    for (int q = 0; q < 4 * (P.nbits + 6); q++) {
        const int blk = q >> 7;
        bool keep;
        if (blk < last_end) {
            int k = 0;
            while (blk >= P.blk_end[k]) k++;
            keep = (P.mask[k] >> (q & 31)) & 1u;
        } else {
            const int b = q - 128 * last_end;
            keep = b < 24 && ((P.tail_mask >> b) & 1u);
        }
        if (keep) inv.push_back((uint8_t)(q % VIT_TILE_POS));
    }
    return inv;
}

// audioSink's three interpolation kernels (host/audio_fir.h)
const std::vector<float> &dab::audio_host_fir() {
    static const std::vector<float> tab = [] {
        std::vector<float> k(15);
        dabgpu::audio_fir_kernels(k.data());
        return k;
    }();
    return tab;
}
int dab::audio_tables(dabgpu_ctx *c, const float **out) {
    if (!c->audiotab) HIPCHK(c->audiotab.put(audio_host_fir()));
    *out = c->audiotab.ptr;
    return 0;
}

// airspyHandler's mapTable_int / mapTable_float of a rate (host/rate_converter.h: products and
// differences that are exact, so this file's contraction cannot change them)
int dab::rate_tables(dabgpu_ctx *c, int rate, const RateEntry **out) {
    auto it = c->ratetab.find(rate);
    if (it == c->ratetab.end()) {
        std::vector<RateTab> h(1);
        dabgpu::rate_tables(rate, h[0].base, h[0].frac);
        RateEntry e;
        e.base.assign(h[0].base, h[0].base + 2048);
        HIPCHK(e.tab.put(h));
        it = c->ratetab.emplace(rate, std::move(e)).first;
    }
    *out = &it->second;
    return 0;
}

// ----------------------------------------------------------------- context
int dab::scratch(dabgpu_ctx *c, int slot, size_t bytes, void **p) {
    DevBuf<uint8_t> &b = c->scratch[slot];
    if (b.n < bytes) {
        b.reset();
        HIPCHK(b.alloc(std::max<size_t>(bytes, 4096)));
    }
    *p = b.ptr;
    return 0;
}

// The layer II tables of the context, uploaded at their first use: a context that never
// decodes layer II allocates nothing for it.
int dab::mp2_tables(dabgpu_ctx *c, const Mp2Tabs **out) {
    if (!c->mp2tab) HIPCHK(c->mp2tab.put(mp2_host_tables()));
    *out = (const Mp2Tabs *)c->mp2tab.ptr;
    return 0;
}

// read (and clear) the device error word; call after a stream synchronisation
int dab::kernel_errors(dabgpu_ctx *c) {
    HIPCHK(hipMemcpyAsync(c->h_err, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int32_t e = *c->h_err;
    if (!e) return 0;
    HIPCHK(hipMemsetAsync(c->err, 0, sizeof(int32_t), c->stream));
    return bounds_error(e);
}
int dab::bounds_error(int32_t e) {
    return fail(DABGPU_E_BOUNDS, "kernel refused out-of-bounds work:%s%s%s", (e & KERR_FRAME) ? " frame descriptor" : "",
                (e & KERR_VITERBI) ? " viterbi source" : "", (e & KERR_RATE) ? " rate conversion table" : "");
}

// symbols 1..75 of a frame are split over `chunks` workgroups of k_demod (each
// recomputes the FFT of the symbol before its first one).  Pick the split whose
// rounds of resident workgroups (kDemodWgPerCu per CU) cost least:
// rounds * (symbols per chunk + 1 warm-up symbol).
#ifndef DEMOD_CHUNK_WG_PER_CU
#define DEMOD_CHUNK_WG_PER_CU 3
#endif
static const int kDemodWgPerCu = DEMOD_CHUNK_WG_PER_CU;
static int num_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 256;
        cus = std::max(cus, 1);
    }
    return cus;
}
// extra: FFTs every chunk adds besides its warm-up symbol (2 when it runs findIndex)
int dab::demod_chunks(int n, int extra) {
    const int cus = num_cus();
    const int64_t slots = (int64_t)kDemodWgPerCu * cus;
    int best = 1;
    double best_cost = 1e30;
    for (int c : {1, 2, 3, 5, 15, 25}) {
        const int64_t items = (int64_t)n * c;
        const double cost = (double)((items + slots - 1) / slots) * ((NSYM + c - 1) / c + 1 + extra);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = c; }
    }
    return best;
}

extern "C" {

int dabgpu_abi_version(void) { return DABGPU_ABI_VERSION; }

int dabgpu_host_table(int which, void *out, size_t bytes) {
    const HostTables &t = host_tables();
    const void *src = nullptr;
    size_t n = 0;
    switch (which) {
    case DABGPU_TABLE_PRS: src = t.ref.data(); n = t.ref.size() * sizeof(float2); break;
    case DABGPU_TABLE_MAPPER: src = t.perm.data(); n = t.perm.size() * sizeof(int16_t); break;
    case DABGPU_TABLE_REFARG: src = t.refarg.data(); n = t.refarg.size() * sizeof(float); break;
    case DABGPU_TABLE_NCO: src = t.nco.data(); n = t.nco.size() * sizeof(double2); break;
    case DABGPU_TABLE_OSC: src = t.osc.data(); n = t.osc.size() * sizeof(float2); break;
    case DABGPU_TABLE_AUDIO_FIR: src = audio_host_fir().data(); n = audio_host_fir().size() * sizeof(float); break;
    default: return fail(DABGPU_E_ARG, "unknown table %d", which);
    }
    if (!out || bytes < n) return fail(DABGPU_E_ARG, "table %d needs %zu bytes", which, n);
    memcpy(out, src, n);
    return 0;
}

int dabgpu_subch_profile(const dabgpu_subch *s, int32_t *nbits, int32_t *frag, int32_t *nseg, int32_t *L, int32_t *PI) {
    if (!s || !nbits || !frag || !nseg || !L || !PI) return fail(DABGPU_E_ARG, "null arg");
    Profile p;
    if (make_profile(*s, p)) return fail(DABGPU_E_UNSUP, "protection (uep=%d, level 0%o) undefined", s->uepFlag, s->protLevel);
    bool fallback = false;
    if (s->uepFlag == 0) {
        fallback = true;
        for (int i = 0; i < kNumUep; i++)
            if (kUepProfiles[i][0] == s->bitRate && kUepProfiles[i][1] == s->protLevel) fallback = false;
    }
    *nbits = p.nbits;
    *frag = p.frag;
    *nseg = p.nseg;
    for (int k = 0; k < 4; k++) {
        L[k] = k < p.nseg ? p.blk_end[k] - (k ? p.blk_end[k - 1] : 0) : 0;
        PI[k] = k < p.nseg ? __builtin_popcount(p.mask[k]) - 8 : 0;
    }
    return fallback ? 1 : 0;
}
const char *dabgpu_last_error(void) { return g_err.c_str(); }

int dabgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dabgpu_ctx_create(int device, dabgpu_ctx **out) {
    if (!out) return fail(DABGPU_E_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DABGPU_E_NODEV, "no HIP device");
    if (device < 0 || device >= n) return fail(DABGPU_E_ARG, "device %d out of range (%d)", device, n);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DABGPU_E_NODEV, "device %d is %s, this build targets gfx950", device, prop.gcnArchName);
    HIPCHK(hipSetDevice(device));
    auto c = std::make_unique<dabgpu_ctx>();
    c->device = device;
    // the context stream carries the OFDM front end: highest priority, so a streaming
    // pipeline's next front end takes the SIMDs the Viterbi tail leaves idle
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(c->stream.create(greatest));
    for (Event &e : c->ev) HIPCHK(e.create(hipEventDefault));
    const HostTables &t = host_tables();
    if (!t.stage_ok) return fail(DABGPU_E_STATE, "stage_layout.h: STAGE_COL is not 24 pairs per colour");
    HIPCHK(c->osc.put(t.osc));
    HIPCHK(c->nco.put(t.nco));
    HIPCHK(c->ref.put(t.ref));
    HIPCHK(c->w2048.put(t.w2048));
    HIPCHK(c->carrier_bin.put(t.carrier_bin));
    HIPCHK(c->prbs.put(t.prbs_words));
    HIPCHK(c->refarg.put(t.refarg));
    HIPCHK(c->dptab.put(t.dptab));
    HIPCHK(c->fic_inv.put(make_inv(fic_profile())));
    HIPCHK(c->err.alloc(1));
    HIPCHK(hipMemset(c->err, 0, sizeof(int32_t)));
    HIPCHK(c->h_err.alloc(1));
    c->T.osc = c->osc;
    c->T.nco = c->nco;
    c->T.ref = c->ref;
    c->T.w2048 = c->w2048;
    c->T.carrier_of_bin = c->carrier_bin;
    c->T.stage_of_bin = c->carrier_bin + 2048;
    c->T.stage_pair = c->carrier_bin + 4096;
    c->T.refarg = c->refarg;
    c->T.err = c->err;
    *out = c.release();
    return 0;
}

int dabgpu_ctx_destroy(dabgpu_ctx *c) {
    delete c;
    return 0;
}

int dabgpu_sync(dabgpu_ctx *c) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int dabgpu_alloc(dabgpu_ctx *c, size_t bytes, void **p) {
    if (!c || !p) return fail(DABGPU_E_ARG, "null arg");
    HIPCHK(hipSetDevice(c->device));
    if (hipMalloc(p, bytes) != hipSuccess) return fail(DABGPU_E_NOMEM, "hipMalloc(%zu) failed", bytes);
    return 0;
}
int dabgpu_free(dabgpu_ctx *c, void *p) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    if (p) HIPCHK(hipFree(p));
    return 0;
}
int dabgpu_memcpy_h2d(dabgpu_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int dabgpu_memcpy_d2h(dabgpu_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int dabgpu_host_alloc(dabgpu_ctx *c, size_t bytes, void **h) {
    if (!c || !h) return fail(DABGPU_E_ARG, "bad args");
    *h = nullptr;
    if (!bytes) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostMalloc(h, bytes, hipHostMallocDefault));
    return 0;
}
int dabgpu_host_free(dabgpu_ctx *c, void *h) {
    if (!c) return fail(DABGPU_E_ARG, "bad args");
    if (h) HIPCHK(hipHostFree(h));
    return 0;
}
int dabgpu_memcpy_d2d(dabgpu_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
int dabgpu_iq_convert(dabgpu_ctx *c, int format, const void *src, int64_t n_pairs, float *iq) {
    if (!c || (!src && n_pairs > 0) || (!iq && n_pairs > 0) || n_pairs < 0) return fail(DABGPU_E_ARG, "bad args");
    if (format != DABGPU_IQ_U8 && format != DABGPU_IQ_S16) return fail(DABGPU_E_ARG, "unknown IQ format %d", format);
    // the vector path reads 16 B per 16 values: the source must be 16-byte aligned
    if (((uintptr_t)src & 15) || ((uintptr_t)iq & 15)) return fail(DABGPU_E_ARG, "IQ buffers must be 16-byte aligned");
    HIPCHK(launch_iq_convert(c->stream, format, src, 2 * n_pairs, iq));
    return 0;
}
int dabgpu_rate_convert(dabgpu_ctx *c, int in_rate, int format, const void *src, int64_t src_stride, int n_streams,
                        const int64_t *n_in, float *iq, int64_t iq_stride, int64_t *n_out, int64_t *n_used) {
    if (!c || !n_in || !n_out || !n_used || n_streams < 1) return fail(DABGPU_E_ARG, "bad args");
    if (!dabgpu::rate_valid(in_rate)) return fail(DABGPU_E_ARG, "in_rate %d: whole kHz in 2048000 .. 10000000", in_rate);
    if (!dabgpu::rate_format_valid(format)) return fail(DABGPU_E_ARG, "unknown IQ format %d", format);
    const int M = in_rate / 1000, bps = dabgpu::rate_format_bytes(format);
    if (((uintptr_t)src & (uintptr_t)(bps - 1)) || ((uintptr_t)iq & 7))
        return fail(DABGPU_E_ARG, "src_d and iq_d must be aligned to one I/Q pair (%d and 8 bytes)", bps);
    bool any = false;
    for (int s = 0; s < n_streams; s++) {
        const int64_t n = n_in[s], B = n < 1 ? 0 : (n - 1) / M;
        if (n < 0) return fail(DABGPU_E_ARG, "stream %d: %lld samples", s, (long long)n);
        if (src_stride < n) return fail(DABGPU_E_ARG, "stream %d: src_stride %lld < %lld samples", s, (long long)src_stride, (long long)n);
        if (B > 0x7FFFFFFF || iq_stride < 2048 * B)
            return fail(DABGPU_E_ARG, "stream %d: iq_stride %lld < %lld outputs", s, (long long)iq_stride, (long long)(2048 * B));
        any = any || B > 0;
    }
    if (any && (!src || !iq)) return fail(DABGPU_E_ARG, "null samples");
    for (int s = 0; s < n_streams; s++) {
        const int64_t B = n_in[s] < 1 ? 0 : (n_in[s] - 1) / M;
        n_out[s] = 2048 * B;
        n_used[s] = M * B;
    }
    if (!any) return 0;
    HIPCHK(hipSetDevice(c->device));
    const RateEntry *e = nullptr;
    if (int rc = rate_tables(c, in_rate, &e)) return rc;
    RateJob J;
    memset(&J, 0, sizeof J);
    J.src_stride = src_stride;
    J.out_stride = iq_stride;
    J.tab = e->tab;
    J.err = c->err;
    J.M = M;
    // the fewest pieces (of 2048 / passes outputs each) whose input spans all fit the kernel's LDS image
    for (J.passes = 1; J.passes <= 8; J.passes *= 2) {
        bool fits = true;
        for (int p = 0, S = 2048 / J.passes; p < J.passes; p++) {
            J.first[p] = e->base[p * S];
            J.last[p] = e->base[p * S + S - 1] + 1;
            fits = fits && (J.last[p] - J.first[p] + 1) * bps <= RATE_LDS_BYTES;
        }
        if (fits) break;
    }
    if (J.passes > 8) return fail(DABGPU_E_STATE, "rate %d: a piece's samples do not fit %d bytes", in_rate, RATE_LDS_BYTES);
    for (int s0 = 0; s0 < n_streams; s0 += RATE_GROUP) {
        J.n_streams = std::min(RATE_GROUP, n_streams - s0);
        J.src = (const char *)src + src_stride * s0 * bps;
        J.out = iq + 2 * iq_stride * s0;
        for (int s = 0; s < J.n_streams; s++) J.blocks[s] = (int32_t)(n_out[s0 + s] / 2048);
        HIPCHK(launch_rate_convert(c->stream, format, J));
    }
    return 0;
}
int dabgpu_memset_d(dabgpu_ctx *c, void *dst, int value, size_t bytes) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    HIPCHK(hipMemsetAsync(dst, value, bytes, c->stream));
    return 0;
}
int dabgpu_kernel_errors(dabgpu_ctx *c) {
    if (!c) return fail(DABGPU_E_ARG, "null ctx");
    return kernel_errors(c);
}

int dabgpu_event_record(dabgpu_ctx *c, int slot) {
    if (!c || slot < 0 || slot >= 16) return fail(DABGPU_E_ARG, "bad event slot");
    HIPCHK(c->ev[slot].record(c->stream));
    return 0;
}
int dabgpu_event_elapsed(dabgpu_ctx *c, int a, int b, float *ms) {
    if (!c || a < 0 || a >= 16 || b < 0 || b >= 16 || !ms) return fail(DABGPU_E_ARG, "bad event slot");
    HIPCHK(c->ev[b].sync());
    HIPCHK(hipEventElapsedTime(ms, c->ev[a].e, c->ev[b].e));
    return 0;
}

// ---- OFDM operators --------------------------------------------------------
int dabgpu_prs_sync(dabgpu_ctx *c, const float *iq, const dabgpu_frame *fr, int n, int16_t level, int32_t *si,
                    float *mx, float *sm) {
    if (!c || !iq || !fr || !si || n < 0) return fail(DABGPU_E_ARG, "bad args");
    HIPCHK(launch_prs_sync(c->stream, iq, DABGPU_IQ_F32, fr, n, c->T, level, si, mx, sm, true));
    return 0;
}
int dabgpu_block0(dabgpu_ctx *c, const float *iq, const dabgpu_frame *fr, int n, int method, int16_t *corr,
                  int16_t *snr) {
    if (!c || !iq || !fr || !corr || n < 0) return fail(DABGPU_E_ARG, "bad args");
    if (method < 0 || method > 2) return fail(DABGPU_E_UNSUP, "freqSyncMethod %d", method);
    HIPCHK(launch_block0(c->stream, iq, DABGPU_IQ_F32, fr, n, c->T, method, corr, snr, true));
    return 0;
}
static int demod_impl(dabgpu_ctx *c, const float *iq, const dabgpu_frame *fr, int n, int16_t *soft, float *softf,
                      float *fc, bool general) {
    void *part = nullptr;
    const int kChunks = demod_chunks(n);
    int rc = scratch(c, SC_FC, sizeof(float2) * (size_t)n * kChunks, &part);
    if (rc) return rc;
    DemodAux aux{};
    HIPCHK(launch_demod(c->stream, iq, fr, n, kChunks, c->T, soft, softf, (float *)part, general, aux));
    if (fc) HIPCHK(launch_fc_reduce(c->stream, (const float *)part, kChunks, n, fc));
    return 0;
}
int dabgpu_ofdm_demod(dabgpu_ctx *c, const float *iq, const dabgpu_frame *fr, int n, int16_t *soft, float *softf,
                      float *fc) {
    if (!c || !iq || !fr || !soft || n < 0) return fail(DABGPU_E_ARG, "bad args");
    return demod_impl(c, iq, fr, n, soft, softf, fc, true);
}
int dabgpu_ofdm_symbol(dabgpu_ctx *c, const float *smp, int kind, float *spec, int16_t *ibits) {
    if (!c || !smp || !spec || (kind != 0 && kind != 1) || (kind == 1 && !ibits)) return fail(DABGPU_E_ARG, "bad args");
    HIPCHK(launch_symbol(c->stream, smp, kind, c->T, spec, ibits));
    return 0;
}
int dabgpu_get_snr(dabgpu_ctx *c, const float *spectrum, int16_t *snr) {
    if (!c || !spectrum || !snr) return fail(DABGPU_E_ARG, "bad args");
    HIPCHK(launch_snr(c->stream, spectrum, snr));
    return 0;
}
int dabgpu_ofdm_demod_mix(dabgpu_ctx *c, const void *iq, int format, const dabgpu_frame *fr, int n, int chunks,
                          int16_t level, int32_t *si, float *mix, float *spec, void *soft) {
    if (!c || !iq || !fr || !mix || !spec || !soft || n < 0 || chunks < 1 || chunks > NSYM) return fail(DABGPU_E_ARG, "bad args");
    if (format != DABGPU_IQ_F32 && format != DABGPU_IQ_S16 && format != DABGPU_IQ_U8) return fail(DABGPU_E_ARG, "format %d", format);
    if (!si && format != DABGPU_IQ_F32) return fail(DABGPU_E_UNSUP, "the operator form reads cf32");
    void *part = nullptr;
    int rc = scratch(c, SC_FC, sizeof(float2) * (size_t)n * chunks, &part);
    if (rc) return rc;
    DemodAux aux{};
    aux.mix = (float2 *)mix;
    aux.spec = (float2 *)spec;
    aux.fmt = format;
    if (si) {                                          // the pipeline's instantiation: findIndex + RING8
        aux.si = si;
        aux.level = level;
        aux.ring8 = 1;
    }
    HIPCHK(launch_demod(c->stream, iq, fr, n, chunks, c->T, (int16_t *)soft, nullptr, (float *)part, true, aux));
    return 0;
}
int dabgpu_nco_eval(dabgpu_ctx *c, int32_t first, int32_t n, float *out) {
    if (!c || !out || first < 0 || n < 0 || (int64_t)first + n > M) return fail(DABGPU_E_ARG, "bad args");
    if (n) HIPCHK(launch_nco_eval(c->stream, c->T, first, n, (float2 *)out));
    return 0;
}
int dabgpu_ofdm_sync_demod(dabgpu_ctx *c, const float *iq, const dabgpu_frame *fr, int n, int16_t level, int32_t *si,
                           int16_t *snr, int16_t *soft, float *softf, float *fc) {
    if (!c || !iq || !fr || !si || !soft || n < 0) return fail(DABGPU_E_ARG, "bad args");
    void *part = nullptr;
    const int kChunks = demod_chunks(n, 2);
    int rc = scratch(c, SC_FC, sizeof(float2) * (size_t)n * kChunks, &part);
    if (rc) return rc;
    DemodAux aux{};
    aux.si = si;
    aux.snr = snr;
    aux.level = level;
    HIPCHK(launch_demod(c->stream, iq, fr, n, kChunks, c->T, soft, softf, (float *)part, true, aux));
    if (fc) HIPCHK(launch_fc_reduce(c->stream, (const float *)part, kChunks, n, fc));
    return 0;
}

// ---- Viterbi operators -------------------------------------------------------
static int run_viterbi(dabgpu_ctx *c, VitJob &J, int max_nbits) {
    void *dec = nullptr;
    int rc = scratch(c, SC_DEC, (size_t)dec_bytes(J.n_cw, max_nbits), &dec);
    if (rc) return rc;
    J.dec = (uint32_t *)dec;
    J.dec_ncw = dec_rows(J.n_cw);
    J.dec_nch = dec_chunks(max_nbits);
    J.prbs_words = c->prbs;
    J.err = c->err;
    HIPCHK(launch_viterbi(c->stream, J));
    return 0;
}

int dabgpu_viterbi(dabgpu_ctx *c, const int16_t *in, int n_cw, int nbits, uint8_t *out) {
    if (!c || !in || !out || n_cw < 0 || nbits <= 0 || nbits > 32768) return fail(DABGPU_E_ARG, "bad args");
    Profile p;
    memset(&p, 0, sizeof p);
    p.nbits = nbits;
    void *pd = nullptr;
    int rc = scratch(c, SC_PROF, sizeof p, &pd);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pd, &p, sizeof p, hipMemcpyHostToDevice, c->stream));
    VitJob J;
    memset(&J, 0, sizeof J);
    J.kind = SRC_MOTHER;
    J.n_cw = n_cw;
    J.src = in;
    J.src_stride = 4 * (int64_t)(nbits + 6);
    J.src_len = (int64_t)n_cw * J.src_stride;
    J.prof = (const Profile *)pd;
    J.out = out;
    J.out_stride = nbits;
    J.prbs = 0;
    return run_viterbi(c, J, nbits);
}

static int fic_common(dabgpu_ctx *c, VitJob &J, uint8_t *bits, uint8_t *ok) {
    Profile p = fic_profile();
    void *pd = nullptr;
    int rc = scratch(c, SC_PROF, sizeof p, &pd);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pd, &p, sizeof p, hipMemcpyHostToDevice, c->stream));
    J.prof = (const Profile *)pd;
    J.out = bits;
    J.out_stride = 768;
    J.prbs = 1;
    if ((rc = run_viterbi(c, J, 768))) return rc;
    if (ok) HIPCHK(launch_fic_post(c->stream, bits, ok, 3 * J.n_cw, c->dptab));
    return 0;
}

int dabgpu_fic_decode(dabgpu_ctx *c, const int16_t *soft, int n, uint8_t *bits, uint8_t *ok) {
    if (!c || !soft || !bits || n < 0) return fail(DABGPU_E_ARG, "bad args");
    VitJob J;
    memset(&J, 0, sizeof J);
    J.kind = SRC_FRAG;
    J.n_cw = n;
    J.src = soft;
    J.src_stride = 2304;
    J.src_len = (int64_t)n * 2304;
    return fic_common(c, J, bits, ok);
}

int dabgpu_fic_decode_frames(dabgpu_ctx *c, const int16_t *soft, const int32_t *slots_h, int nf, uint8_t *bits,
                             uint8_t *ok) {
    if (!c || !soft || !slots_h || !bits || nf < 0) return fail(DABGPU_E_ARG, "bad args");
    void *sd = nullptr;
    int rc = scratch(c, SC_I32, sizeof(int32_t) * (size_t)std::max(nf, 1), &sd);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(sd, slots_h, sizeof(int32_t) * nf, hipMemcpyHostToDevice, c->stream));
    VitJob J;
    memset(&J, 0, sizeof J);
    J.kind = SRC_FIC;
    J.n_cw = 4 * nf;
    J.src = soft;
    J.inv = c->fic_inv;
    J.slots = (const int32_t *)sd;
    {
        int32_t mx = 0;
        for (int i = 0; i < nf; i++) {
            if (slots_h[i] < 0) return fail(DABGPU_E_ARG, "negative slot");
            mx = std::max(mx, slots_h[i]);
        }
        J.src_len = (int64_t)(mx + 1) * FRAME_SOFT;
    }
    rc = fic_common(c, J, bits, ok);
    if (rc) return rc;
    return kernel_errors(c);                       // also: slots scratch may be reused by the next call
}

int dabgpu_rs_decode(dabgpu_ctx *c, const uint8_t *in, int n, uint8_t *out, int16_t *ret) {
    if (!c || !in || !out || !ret || n < 0) return fail(DABGPU_E_ARG, "bad args");
    HIPCHK(launch_rs(c->stream, in, n, c->dptab, out, ret));
    return 0;
}

int dabgpu_mp2_decode(dabgpu_ctx *c, const uint8_t *frames, int64_t frame_stride, int n_chains, int chain_len,
                      void *state, int16_t *pcm, int32_t *ret) {
    if (!c || !frames || !state || !pcm || !ret || n_chains < 0 || chain_len < 0) return fail(DABGPU_E_ARG, "bad args");
    if (frame_stride < 4 || frame_stride > 0x7FFFFFFF) return fail(DABGPU_E_ARG, "frame_stride %lld", (long long)frame_stride);
    if (!n_chains || !chain_len) return 0;
    // the chain's first workgroup reads the state its last one writes: it reads a copy
    const size_t sb = (size_t)n_chains * DABGPU_MP2_STATE_BYTES;
    void *copy = nullptr;
    if (int rc = scratch(c, SC_MP2, sb, &copy)) return rc;
    HIPCHK(hipMemcpyAsync(copy, state, sb, hipMemcpyDeviceToDevice, c->stream));
    Mp2Job J;
    memset(&J, 0, sizeof J);
    J.frames = frames;
    J.stride = frame_stride;
    J.n_chains = n_chains;
    J.chain_len = chain_len;
    J.state_in = (const int16_t *)copy;
    J.state_out = (int16_t *)state;
    J.pcm = pcm;
    J.ret = ret;
    J.cdiv = 1;
    J.idx_a = chain_len;
    J.idx_c = 1;
    if (int rc = mp2_tables(c, &J.tabs)) return rc;
    HIPCHK(launch_mp2_decode(c->stream, J));
    return 0;
}

int dabgpu_audio_out(dabgpu_ctx *c, const int16_t *pcm, int64_t pcm_stride, int n_chains, int chain_len, int max_amount,
                     const int32_t *rates, const int32_t *amounts, void *state, float *samples, int32_t *n_out) {
    if (!c || !pcm || !rates || !amounts || !state || !samples || !n_out || n_chains < 0 || chain_len < 0 || max_amount < 0)
        return fail(DABGPU_E_ARG, "bad args");
    if (pcm_stride < max_amount) return fail(DABGPU_E_ARG, "pcm_stride %lld < max_amount %d", (long long)pcm_stride, max_amount);
    if (max_amount > 0x7FFFFFFF / 3) return fail(DABGPU_E_ARG, "max_amount %d", max_amount);
    if (((uintptr_t)pcm & 3) || ((uintptr_t)state & 3) || ((uintptr_t)samples & 7))
        return fail(DABGPU_E_ARG, "pcm_d and state_d must be 4-byte aligned, samples_d 8-byte aligned");
    const int64_t ncall = (int64_t)n_chains * chain_len;
    if (ncall > 0x7FFFFFFF) return fail(DABGPU_E_ARG, "%lld calls in one batch", (long long)ncall);
    for (int64_t i = 0; i < ncall; i++) {
        if (rates[i] == 0) continue;
        if (amounts[i] < 0 || amounts[i] > max_amount)
            return fail(DABGPU_E_ARG, "call %lld: amount %d outside 0 .. %d", (long long)i, amounts[i], max_amount);
        if (rates[i] == 32000 && (amounts[i] & 1))
            return fail(DABGPU_E_ARG, "call %lld: odd amount %d at 32000 Hz", (long long)i, amounts[i]);
    }
    if (!ncall) return 0;
    void *desc = nullptr;
    if (int rc = scratch(c, SC_AUDIO, 2 * sizeof(int32_t) * (size_t)ncall, &desc)) return rc;
    HIPCHK(hipMemcpyAsync(desc, rates, sizeof(int32_t) * ncall, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync((int32_t *)desc + ncall, amounts, sizeof(int32_t) * ncall, hipMemcpyHostToDevice, c->stream));
    AudioJob J;
    memset(&J, 0, sizeof J);
    J.pcm = pcm;
    J.in_pairs = pcm_stride;
    J.in_a = chain_len;
    J.in_c = 1;
    J.n_chains = n_chains;
    J.chain_len = chain_len;
    J.cdiv = 1;
    J.rates = (const int32_t *)desc;
    J.amounts = (const int32_t *)desc + ncall;
    J.state = (AudioState *)state;
    J.samples = samples;
    J.n_out = n_out;
    J.out_pairs = 3 * (int64_t)max_amount;
    J.out_a = chain_len;
    J.out_c = 1;
    if (int rc = audio_tables(c, &J.coef)) return rc;
    HIPCHK(launch_audio(c->stream, J));
    return 0;
}

size_t dabgpu_pad_state_bytes(void) { return sizeof(PadState); }

int dabgpu_pad_aus(dabgpu_ctx *c, void *state, int n_slots, const uint8_t *aus, int64_t au_stride, const int32_t *len,
                   int n_aus, const int32_t *cif, dabgpu_pad_label *labels, int label_slots, dabgpu_datagroup *groups,
                   int group_slots, uint8_t *bytes, int64_t arena_bytes, dabgpu_pad_run *run) {
    if (!c || !state || !labels || !groups || !bytes || !run || n_slots < 0 || n_aus < 0 || au_stride < 0 || label_slots < 0 ||
        group_slots < 0 || (n_aus && (!aus || !len)))
        return fail(DABGPU_E_ARG, "bad args");
    if (arena_bytes < DABGPU_PAD_ARENA_BYTES(0) || arena_bytes > 0x7FFFFFFF)
        return fail(DABGPU_E_ARG, "arena_bytes %lld", (long long)arena_bytes);
    if ((uintptr_t)state & 15) return fail(DABGPU_E_ARG, "state_d must be 16-byte aligned");
    if (!n_slots) return 0;
    PadJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = n_slots;
    J.n_aus = n_aus;
    J.state = (uint8_t *)state;
    J.aus = aus;
    J.au_stride = au_stride;
    J.len = len;
    J.cif = cif;
    J.labels = labels;
    J.label_slots = label_slots;
    J.groups = groups;
    J.group_slots = group_slots;
    J.bytes = bytes;
    J.arena = arena_bytes;
    J.run = run;
    HIPCHK(launch_pad(c->stream, J));
    return 0;
}

size_t dabgpu_fic_db_bytes(void) { return sizeof(dabgpu_fic_db); }

int dabgpu_fib_parse(dabgpu_ctx *c, dabgpu_fic_db *db, int n_slots, const uint8_t *fibs, int64_t fib_stride, const uint8_t *ok,
                     int n_fibs, int want_flags, dabgpu_fic_event *events, int event_slots, dabgpu_fic_table *table,
                     dabgpu_fic_run *run) {
    if (!c || !db || !table || !run || n_slots < 0 || n_fibs < 0 || event_slots < 0 || (n_fibs && (!fibs || !ok)) ||
        (event_slots && !events))
        return fail(DABGPU_E_ARG, "bad args");
    if (fib_stride < (int64_t)32 * n_fibs) return fail(DABGPU_E_ARG, "fib_stride %lld below 32 * n_fibs", (long long)fib_stride);
    if ((uintptr_t)db & 15) return fail(DABGPU_E_ARG, "db_d must be 16-byte aligned");
    if (event_slots > (1 << 24)) return fail(DABGPU_E_ARG, "event_slots %d", event_slots);
    if (!n_slots) return 0;
    FibJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = n_slots;
    J.n_fibs = n_fibs;
    J.db = db;
    J.fibs = fibs;
    J.stride = fib_stride;
    J.ok = ok;
    J.want = want_flags & (DABGPU_SUBCH_MP2 | DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT | DABGPU_SUBCH_PAD | DABGPU_SUBCH_IP);
    J.events = events;
    J.event_slots = event_slots;
    J.table = table;
    J.run = run;
    HIPCHK(launch_fib(c->stream, J));
    return 0;
}

int dabgpu_fic_clear(dabgpu_ctx *c, dabgpu_fic_db *db, int n_slots, const uint8_t *which) {
    if (!c || !db || n_slots < 0) return fail(DABGPU_E_ARG, "bad args");
    for (int s = 0; s < n_slots;) {                // one launch per run of chosen slots
        if (which && !which[s]) {
            s++;
            continue;
        }
        int e = s;
        while (e < n_slots && (!which || which[e])) e++;
        HIPCHK(launch_fic_clear(c->stream, db + s, e - s));
        s = e;
    }
    return 0;
}

size_t dabgpu_mot_state_bytes(int max_body_bytes) {
    if (max_body_bytes < 0 || max_body_bytes > (1 << 24)) return 0;
    const size_t cap = ((size_t)(max_body_bytes ? max_body_bytes : DABGPU_MOT_BODY_BYTES) + 15) / 16 * 16;
    return MOT_TABLE_BYTES + DABGPU_MOT_ENTRIES * cap;
}

int dabgpu_mot_groups(dabgpu_ctx *c, void *state, int n_slots, int max_body_bytes, const dabgpu_datagroup *groups,
                      int group_slots, const uint8_t *bytes, int64_t arena_bytes, const dabgpu_packet_run *run,
                      dabgpu_mot_object *objects, uint8_t *out, int64_t out_arena_bytes, dabgpu_mot_run *mot_run) {
    if (!c || !state || !groups || !bytes || !run || !objects || !out || !mot_run || n_slots < 0 || group_slots < 0)
        return fail(DABGPU_E_ARG, "bad args");
    if (max_body_bytes < 0 || max_body_bytes > (1 << 24)) return fail(DABGPU_E_ARG, "max_body_bytes %d", max_body_bytes);
    const int body = max_body_bytes ? max_body_bytes : DABGPU_MOT_BODY_BYTES;
    if (arena_bytes < 0 || arena_bytes > 0x7FFFFFFF || out_arena_bytes > 0x7FFFFFFF || (out_arena_bytes & 15) ||
        out_arena_bytes < DABGPU_MOT_ARENA_FOR(0, body))
        return fail(DABGPU_E_ARG, "arena sizes %lld / %lld", (long long)arena_bytes, (long long)out_arena_bytes);
    if (((uintptr_t)state | (uintptr_t)out) & 15) return fail(DABGPU_E_ARG, "state_d and out_d must be 16-byte aligned");
    if (!n_slots) return 0;
    MotJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = n_slots;
    J.max_body = body;
    J.body_cap = (body + 15) / 16 * 16;
    J.state_bytes = (int64_t)dabgpu_mot_state_bytes(body);
    J.state = (uint8_t *)state;
    J.groups = groups;
    J.gslots = group_slots;
    J.bytes = bytes;
    J.arena = arena_bytes;
    J.run = run;
    J.objects = objects;
    J.out = out;
    J.out_arena = out_arena_bytes;
    J.mot_run = mot_run;
    void *w = nullptr;
    const size_t ob = ((size_t)n_slots * 2 * group_slots * sizeof(int4) + 15) / 16 * 16;
    if (int rc = scratch(c, SC_MOT, ob + sizeof(int32_t) * n_slots, &w)) return rc;
    J.ops = (int4 *)w;
    J.nops = (int32_t *)((uint8_t *)w + ob);
    HIPCHK(launch_mot(c->stream, J));
    return 0;
}

int dabgpu_ip_groups(dabgpu_ctx *c, dabgpu_ip_state *state, int n_slots, const dabgpu_datagroup *groups, int group_slots,
                     const uint8_t *bytes, int64_t arena_bytes, const dabgpu_packet_run *run, dabgpu_ip_result *results,
                     uint8_t *out, int64_t out_arena_bytes, dabgpu_ip_run *ip_run) {
    if (!c || !state || !groups || !bytes || !run || !results || !out || !ip_run || n_slots < 0 || group_slots < 0)
        return fail(DABGPU_E_ARG, "bad args");
    if (arena_bytes < 0 || arena_bytes > 0x7FFFFFFF || out_arena_bytes < 0 || out_arena_bytes > 0x7FFFFFFF)
        return fail(DABGPU_E_ARG, "arena sizes %lld / %lld", (long long)arena_bytes, (long long)out_arena_bytes);
    if (!n_slots) return 0;
    IpJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = n_slots;
    J.state = state;
    J.groups = groups;
    J.gslots = group_slots;
    J.bytes = bytes;
    J.arena = arena_bytes;
    J.run = run;
    J.results = results;
    J.out = out;
    J.out_arena = out_arena_bytes;
    J.ip_run = ip_run;
    HIPCHK(launch_ip(c->stream, J));
    return 0;
}

int dabgpu_msc_deconvolve(dabgpu_ctx *c, const int16_t *frag, int64_t frag_stride, const dabgpu_subch *sub,
                          int n_cw, uint8_t *bits, int64_t out_stride) {
    if (!c || !frag || !sub || !bits || n_cw < 0) return fail(DABGPU_E_ARG, "bad args");
    std::vector<Profile> profs;
    std::vector<int32_t> cwp(n_cw);
    int maxbits = 8;
    const int raw = n_cw ? (sub[0].flags & DABGPU_SUBCH_RAW) : 0;
    for (int i = 0; i < n_cw; i++) {
        if ((sub[i].flags & DABGPU_SUBCH_RAW) != raw)
            return fail(DABGPU_E_ARG, "DABGPU_SUBCH_RAW must be the same for every codeword of a call");
        if (sub[i].bitRate > MSC_MAX_BITRATE)          // beyond the energy-dispersal table (and any CIF)
            return fail(DABGPU_E_UNSUP, "subchannel %d: bitRate %d above %d kbit/s", i, sub[i].bitRate, MSC_MAX_BITRATE);
        Profile p;
        int rc = make_profile(sub[i], p);
        if (rc) return fail(DABGPU_E_UNSUP, "subchannel %d: protection (uep=%d, level 0%o, %d kbps) undefined",
                            i, sub[i].uepFlag, sub[i].protLevel, sub[i].bitRate);
        if (p.frag > frag_stride) return fail(DABGPU_E_ARG, "fragment stride %lld < %d", (long long)frag_stride, p.frag);
        if (p.nbits > out_stride) return fail(DABGPU_E_ARG, "out stride too small");
        int found = -1;
        for (size_t j = 0; j < profs.size(); j++)
            if (!memcmp(&profs[j], &p, sizeof p)) { found = (int)j; break; }
        if (found < 0) { found = (int)profs.size(); profs.push_back(p); }
        cwp[i] = found;
        maxbits = std::max(maxbits, p.nbits);
    }
    void *pd = nullptr, *cd = nullptr;
    int rc = scratch(c, SC_PROF, sizeof(Profile) * std::max<size_t>(profs.size(), 1), &pd);
    if (rc) return rc;
    if ((rc = scratch(c, SC_I32, sizeof(int32_t) * std::max(n_cw, 1), &cd))) return rc;
    if (!profs.empty()) HIPCHK(hipMemcpyAsync(pd, profs.data(), sizeof(Profile) * profs.size(), hipMemcpyHostToDevice, c->stream));
    if (n_cw) HIPCHK(hipMemcpyAsync(cd, cwp.data(), sizeof(int32_t) * n_cw, hipMemcpyHostToDevice, c->stream));
    VitJob J;
    memset(&J, 0, sizeof J);
    J.kind = SRC_FRAG;
    J.n_cw = n_cw;
    J.src = frag;
    J.src_stride = frag_stride;
    J.src_len = (int64_t)n_cw * frag_stride;
    J.prof = (const Profile *)pd;
    J.cw_prof = (const int32_t *)cd;
    J.out = bits;
    J.out_stride = out_stride;
    J.prbs = raw ? 0 : 1;
    if ((rc = run_viterbi(c, J, maxbits))) return rc;
    return kernel_errors(c);
}

}  // extern "C"
