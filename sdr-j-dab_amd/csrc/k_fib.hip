// FIC layer: CRC-good FIBs -> the service database, the signals and the subchannel table
// (dabgpu_fib_parse).  fib_processor::process_FIB (fib-processor.cpp), bit for bit what
// host/fib_processor.cpp does, which cites the reference line for every function; the rules
// where the reference is undefined are those of dabgpu_fib_parse (include/dabgpu.h).
//
// A database is a chain: every FIG sees what the FIGs before it left -- the service a FIG 0/2
// allocated is the one a FIG 1/1 names, a FIG 0/3 finds the component a FIG 0/2 bound.  So the
// parallelism is databases, one wave each (k_fib_walk), as k_pad_walk's is handlers.  The state,
// 5.1 KB, and the table under construction, 0.8 KB, live in LDS for the pass; the FIB is staged
// there too (32 bytes, packed from one bit per byte where the pipeline delivers that).  The FIG
// walk is wave-uniform: every field is read by all lanes from the same LDS bytes and passed
// through readfirstlane, so offsets, lengths and branches are scalar.
// What the lanes are for is the tables: all three have 64 entries, the wave's width.
// find_service, find_packet_component, bind's duplicate test and first-free search and FIG
// 0/14's sweep are one compare per lane, a ballot and a find-first; a label's 16 bytes move by
// 16 lanes; the end-of-call table is built with lane = SubChId, a ballot prefix for the output
// position and a 64-step component scan per lane (every lane reads the same component: an LDS
// broadcast).
// Every index is bounded by the width of the field it comes from (6 bits for a SubChId or a
// UEP index, a find-first over 64 lanes for a slot) or checked (the event slots): no FIB makes
// the kernel leave its slot.  Plain vector stores only; a slot's state is its own, so nothing
// is atomic.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

// Short-form sub-channel table (ETSI EN 300 401 table 8, fib-processor.cpp:30-94): size in CUs,
// protection level, bit rate per table index
static __device__ const int16_t FIB_UEP[64][3] = {
    {16, 5, 32},   {21, 4, 32},   {24, 3, 32},   {29, 2, 32},   {35, 1, 32},   {24, 5, 48},   {29, 4, 48},   {35, 3, 48},
    {42, 2, 48},   {52, 1, 48},   {29, 5, 56},   {35, 4, 56},   {42, 3, 56},   {52, 2, 56},   {32, 5, 64},   {42, 4, 64},
    {48, 3, 64},   {58, 2, 64},   {70, 1, 64},   {40, 5, 80},   {52, 4, 80},   {58, 3, 80},   {70, 2, 80},   {84, 1, 80},
    {48, 5, 96},   {58, 4, 96},   {70, 3, 96},   {84, 2, 96},   {104, 1, 96},  {58, 5, 112},  {70, 4, 112},  {84, 3, 112},
    {104, 2, 112}, {64, 5, 128},  {84, 4, 128},  {96, 3, 128},  {116, 2, 128}, {140, 1, 128}, {80, 5, 160},  {104, 4, 160},
    {116, 3, 160}, {140, 2, 160}, {168, 1, 160}, {96, 5, 192},  {116, 4, 192}, {140, 3, 192}, {168, 2, 192}, {208, 1, 192},
    {116, 5, 224}, {140, 4, 224}, {168, 3, 224}, {208, 2, 224}, {232, 1, 224}, {128, 5, 256}, {168, 4, 256}, {192, 3, 256},
    {232, 2, 256}, {280, 1, 256}, {160, 5, 320}, {208, 4, 320}, {280, 2, 320}, {192, 5, 384}, {280, 3, 384}, {416, 1, 384}};

constexpr int FIB_TABLE_WORDS = (int)(sizeof(dabgpu_fic_table) / 4);

__global__ __launch_bounds__(64) void k_fib_walk(FibJob J) {
    __shared__ __attribute__((aligned(16))) dabgpu_fic_db S;
    __shared__ __attribute__((aligned(16))) dabgpu_fic_table T;
    __shared__ uint8_t fib[32];
    __shared__ int32_t figs[8];
    const int lane = threadIdx.x, slot = blockIdx.x;
    dabgpu_fic_db *state = J.db + slot;
    {
        const uint4 *sw = (const uint4 *)state;
        uint4 *lw = (uint4 *)&S;
        for (int i = lane; i < (int)(sizeof(dabgpu_fic_db) / 16); i += 64) lw[i] = sw[i];
        if (lane < 8) figs[lane] = 0;
    }
    __syncthreads();
    // everything below is the same in every lane (wave-uniform) unless a lane index appears
    auto U = [](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    int over = 0;                                                         // this FIB met the overrun rule
    // n (1..32) bits from bit `off` of the FIB, msb first; the overrun rule past bit 255
    auto bits = [&](int off, int n) -> uint32_t {
        if (off + n > 256) over = 1;
        const int b0 = off >> 3;
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) w = (w << 8) | (b0 + k < 32 ? (uint32_t)fib[b0 + k] : 0u);
        const uint32_t v = (uint32_t)(w >> (40 - (off & 7) - n));
        return U(n == 32 ? v : v & ((1u << n) - 1u));
    };
    // byte i of the 16 label bytes at bit `off` (a multiple of 8): lanes read theirs
    auto label_byte = [&](int off, int i) -> uint8_t {
        const int b = (off >> 3) + i;
        return b < 32 ? fib[b] : (uint8_t)0;
    };
    dabgpu_fic_event *events = J.events + (int64_t)slot * J.event_slots;
    int n_events = 0, fibno = 0;
    auto raise = [&](int kind, int id, int charset, int off) {            // a signal, with the label at bit off
        if (n_events < J.event_slots) {
            dabgpu_fic_event *E = events + n_events;
            if (lane == 0) {
                E->kind = kind;
                E->fib = fibno;
                E->id = id;
                E->charset = charset;
            }
            if (lane < 16) E->label[lane] = label_byte(off, lane);
        }
        n_events++;
    };

    // find_service (:1041-1058): the in-use entry with this SId, else a new one in the first
    // free slot, else entry 0
    auto find_service = [&](int32_t sid) -> int {
        const dabgpu_fic_service &e = S.services[lane];
        const unsigned long long hit = __ballot(e.inUse && e.serviceId == sid);
        if (hit) return __ffsll(hit) - 1;
        const unsigned long long fr = __ballot(!e.inUse);
        if (!fr) return 0;
        const int k = __ffsll(fr) - 1;
        if (lane == 0) {
            S.services[k].inUse = 1;
            S.services[k].hasName = 0;
            S.services[k].serviceId = sid;
        }
        __syncthreads();
        return k;
    };
    // bind_audioService / bind_packetService (:1077-1140): once per (service, component number),
    // in the first free slot; -1: bound already, or the table is full (rule 2)
    auto bind = [&](int tmid, int32_t sid, int compnr) -> int {
        const int s = find_service(sid);
        const dabgpu_fic_component &c = S.components[lane];
        if (__ballot(c.inUse && c.service == s && c.componentNr == compnr)) return -1;
        const unsigned long long fr = __ballot(!c.inUse);
        if (!fr) return -1;
        const int k = __ffsll(fr) - 1;
        if (lane == 0) {
            S.components[k].inUse = 1;
            S.components[k].TMid = (int8_t)tmid;
            S.components[k].service = (int16_t)s;
            S.components[k].componentNr = (int16_t)compnr;
        }
        __syncthreads();
        return k;
    };

    // FIG 0/1 (:288-354); d: the FIG's first bit
    auto fig0_1 = [&](int d, int used) -> int {
        const int o = d + used * 8;
        const int id = (int)bits(o, 6);
        const int start = (int)bits(o + 6, 10);
        const bool longform = bits(o + 16, 1);
        int len = -1, level = 0, rate = 0;                                // -1: the three fields stay
        if (!longform) {                                                  // UEP table index
            const int idx = (int)bits(o + 18, 6);
            len = FIB_UEP[idx][0];
            level = FIB_UEP[idx][1];
            rate = FIB_UEP[idx][2];
        } else {                                                          // EEP
            const int option = (int)bits(o + 17, 3);
            const int lv = (int)bits(o + 20, 2) + 1;
            const int size = (int)bits(o + 22, 10);
            const int divA = lv == 1 ? 12 : lv == 2 ? 8 : lv == 3 ? 6 : 4, divB = lv == 1 ? 27 : lv == 2 ? 21 : lv == 3 ? 18 : 15;
            if (option == 0) {
                len = size;
                level = lv + 0100;
                rate = size / divA * 8;
            } else if (option == 1) {
                len = size;
                level = lv + 0200;
                rate = size / divB * 32;
            }
        }
        if (lane == 0) {
            dabgpu_fic_subch &s = S.sub[id];
            s.inUse = 1;
            s.StartAddr = (int16_t)start;
            s.uepFlag = longform ? 1 : 0;
            if (len >= 0) {
                s.Length = (int16_t)len;
                s.protLevel = (int16_t)level;
                s.BitRate = (int16_t)rate;
            }
        }
        __syncthreads();
        return used + (longform ? 4 : 3);
    };
    // FIG 0/2 (:377-422)
    auto fig0_2 = [&](int d, int used, int pd) -> int {
        int o = d + used * 8;
        int32_t sid;
        if (pd == 1) {
            sid = (int32_t)bits(o, 32);
            o += 32;
        } else {
            sid = (int32_t)bits(o, 16);
            o += 16;
        }
        const int ncomp = (int)bits(o + 4, 4);
        o += 8;
        for (int i = 0; i < ncomp; i++) {
            const int tmid = (int)bits(o, 2);
            // (the fields are read before the bind, as the reference's calls do: it matters to the
            // overrun rule alone)
            if (tmid == 0) {                                              // audio
                const int a = (int)bits(o + 2, 6), sc = (int)bits(o + 8, 6), ps = (int)bits(o + 14, 1);
                const int k = bind(tmid, sid, i);
                if (k >= 0) {
                    if (lane == 0) {
                        S.components[k].ASCTy = (int16_t)a;
                        S.components[k].subchannelId = (int16_t)sc;
                        S.components[k].PS_flag = (int16_t)ps;
                    }
                    __syncthreads();
                }
            } else if (tmid == 3) {                                       // packet data
                const int sc = (int)bits(o + 2, 12), ps = (int)bits(o + 14, 1), ca = (int)bits(o + 15, 1);
                const int k = bind(tmid, sid, i);
                if (k >= 0) {
                    if (lane == 0) {
                        S.components[k].SCId = (uint16_t)sc;
                        S.components[k].PS_flag = (int16_t)ps;
                        S.components[k].CAflag = (uint8_t)ca;
                    }
                    __syncthreads();
                }
            }
            o += 16;
        }
        return (o - d) / 8;
    };
    // FIG 0/3 (:433-453), with find_packetComponent (:1060-1075)
    auto fig0_3 = [&](int d, int used) -> int {
        const int o = d + used * 8;
        const uint32_t scid = bits(o, 12);
        const dabgpu_fic_component &c = S.components[lane];
        const unsigned long long hit = __ballot(c.inUse && c.TMid == 3 && c.SCId == scid);
        if (hit) {
            const int k = __ffsll(hit) - 1;
            const int dg = (int)bits(o + 16, 1), ty = (int)bits(o + 18, 6), sc = (int)bits(o + 24, 6), pa = (int)bits(o + 30, 10);
            if (lane == 0) {
                S.components[k].DGflag = (int8_t)dg;
                S.components[k].DSCTy = (int16_t)ty;
                S.components[k].subchannelId = (int16_t)sc;
                S.components[k].packetAddress = (int16_t)pa;
            }
            __syncthreads();
        }
        return used + 7;
    };
    // FIG 0 (:162-239)
    auto fig0 = [&](int d) {
        const int len = (int)bits(d + 3, 5);
        const int pd = (int)bits(d + 10, 1);
        switch (bits(d + 11, 5)) {
        case 1:                                                           // :278-286
            for (int used = 2; used < len - 1;) used = fig0_1(d, used);
            break;
        case 2:                                                           // :356-367
            for (int used = 2; used < len;) used = fig0_2(d, used, pd);
            break;
        case 3:                                                           // :424-431
            for (int used = 2; used < len;) used = fig0_3(d, used);
            break;
        case 14:                                                          // :688-705: the entries whose SubChId field matches
            for (int used = 2; used < len; used++) {
                const int id = (int)bits(d + used * 8, 6), fec = (int)bits(d + used * 8 + 6, 2);
                if (S.sub[lane].SubChId == id) S.sub[lane].FEC_scheme = (int16_t)fec;
            }
            __syncthreads();
            break;
        case 16:                                                          // :707-724: a service entry per SId
            for (int o = 16; o < len * 8; o += 72) find_service((int32_t)bits(d + o, 16));
            break;
        case 17:                                                          // :726-752
            for (int o = 16; o < len * 8;) {
                const int32_t sid = (int32_t)bits(d + o, 16);
                const bool lflag = bits(d + o + 18, 1), ccflag = bits(d + o + 19, 1);
                const int k = find_service(sid);
                int lang = -1;
                if (lflag) {
                    lang = (int)bits(d + o + 24, 8);
                    o += 8;
                }
                const int pty = (int)bits(d + o + 27, 5);
                if (lane == 0) {
                    if (lang >= 0) {
                        S.services[k].language = (int16_t)lang;
                        S.services[k].hasLanguage = 1;
                    }
                    S.services[k].programType = (int16_t)pty;
                }
                __syncthreads();
                o += ccflag ? 40 : 32;
            }
            break;
        default:
            break;
        }
    };
    // a service label (FIG 1/1, 1/5, 2/5): taken once per entry
    auto name_service = [&](int k, int charset, int off, bool suffix, bool signal) {
        if (U(S.services[k].hasName)) return;
        if (off + 128 > 256) over = 1;
        if (lane < 16) S.services[k].label[lane] = label_byte(off, lane);
        if (lane == 0) {
            S.services[k].charset = (uint8_t)charset;
            S.services[k].data_suffix = suffix ? 1 : 0;
            S.services[k].hasName = 1;
        }
        __syncthreads();
        if (signal) raise(DABGPU_FIC_ADD_SERVICE, k, charset, off);
    };
    // FIG 1 (:850-997): extensions 0, 1 and 5
    auto fig1 = [&](int d) {
        const int charset = (int)bits(d + 8, 4);
        const bool oe = bits(d + 12, 1);
        const int ext = (int)bits(d + 13, 3);
        if (ext == 0) {                                                   // ensemble label
            const int eid = (int)bits(d + 16, 16);
            if (d + 32 + 128 > 256) over = 1;                             // the label is read whatever OE says
            if (!oe) {
                if (!U(S.named)) {
                    if (lane < 16) S.label[lane] = label_byte(d + 32, lane);
                    if (lane == 0) {
                        S.EId = eid;
                        S.charset = (uint8_t)charset;
                        S.named = 1;
                    }
                    __syncthreads();
                    raise(DABGPU_FIC_NAME_ENSEMBLE, eid, charset, d + 32);
                }
            }
        } else if (ext == 1) {
            name_service(find_service((int32_t)bits(d + 16, 16)), charset, d + 32, false, true);
        } else if (ext == 5) {                                            // " (data)" appended, no signal
            name_service(find_service((int32_t)bits(d + 16, 32)), charset, d + 48, true, false);
        }
    };
    // FIG 2 extension 5 (:998-1037)
    auto fig2 = [&](int d) {
        const int charset = (int)bits(d + 8, 4);
        if (bits(d + 13, 3) != 5u) return;
        name_service(find_service((int32_t)bits(d + 16, 32)), charset, d + 48, false, false);
    };

    int parsed = 0, skipped = 0, overrun = 0;
    for (int i = 0; i < J.n_fibs; i++) {
        if (!U(J.ok[(int64_t)slot * J.n_fibs + i])) {
            skipped++;
            continue;
        }
        const uint8_t *src = J.fibs + (int64_t)slot * J.stride + (int64_t)i * (J.bit_src ? 256 : 32);
        __syncthreads();                                                  // the last FIB's reads, before it is replaced
        if (lane < 32) {
            uint32_t b;
            if (J.bit_src) {
                const uint2 w = *(const uint2 *)(src + 8 * lane);         // (256-byte FIBs of a 16-byte aligned buffer)
                b = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) b |= (((w.x >> (8 * k)) & 1u) << (7 - k)) | (((w.y >> (8 * k)) & 1u) << (3 - k));
            } else {
                b = src[lane];
            }
            fib[lane] = (uint8_t)b;
        }
        __syncthreads();
        parsed++;
        fibno = i;
        over = 0;
        for (int processed = 0; processed < 30;) {                        // process_FIB (:123-160)
            const int d = processed * 8;
            const int type = (int)bits(d, 3);
            if (lane == 0) figs[type]++;
            if (type == 7) break;
            if (type == 0) fig0(d);
            else if (type == 1) fig1(d);
            else if (type == 2) fig2(d);
            processed += (int)bits(d + 3, 5) + 1;
        }
        overrun += over;
    }
    __syncthreads();
    // the event slots this call did not fill are zeroed: a caller's buffer may hold an earlier call's
    if (n_events < J.event_slots) {
        uint32_t *w = (uint32_t *)(events + n_events);
        const int words = (J.event_slots - n_events) * (int)(sizeof(dabgpu_fic_event) / 4);
        for (int i = lane; i < words; i += 64) w[i] = 0u;
    }

    // fib_processor::subchannels: lane = SubChId
    {
        uint32_t *tw = (uint32_t *)&T;
        for (int i = lane; i < FIB_TABLE_WORDS; i += 64) tw[i] = 0u;
    }
    __syncthreads();
    {
        const dabgpu_fic_subch s = S.sub[lane];
        const unsigned long long mask = __ballot(s.inUse);
        if (s.inUse) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            const bool classic = J.want & DABGPU_SUBCH_MP2, packet = J.want & DABGPU_SUBCH_PACKET, mot = J.want & DABGPU_SUBCH_MOT,
                       pad = J.want & DABGPU_SUBCH_PAD, ip = J.want & DABGPU_SUBCH_IP;
            int flags = 0;
            for (int k = 0; k < 64; k++) {
                const dabgpu_fic_component c = S.components[k];
                if (!c.inUse || c.subchannelId != lane) continue;
                if (c.TMid == 0) {
                    if (c.ASCTy == 077) flags |= DABGPU_SUBCH_DABPLUS;
                    else if (c.ASCTy == 0 && classic) flags |= DABGPU_SUBCH_MP2;
                } else if (c.TMid == 3 && c.DSCTy != 0 && !(c.DSCTy == 5 && c.DGflag)) {
                    if (packet) flags |= DABGPU_SUBCH_PACKET;
                    if (mot && c.DSCTy == 60) flags |= DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT;
                    if (ip && c.DSCTy == 59) flags |= DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP;
                }
            }
            if ((flags & DABGPU_SUBCH_DABPLUS) && pad) flags |= DABGPU_SUBCH_PAD;
            if (flags & DABGPU_SUBCH_DABPLUS) flags &= ~DABGPU_SUBCH_MP2;                           // (one layer per entry,
            if (flags & (DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_MP2))
                flags &= ~(DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT | DABGPU_SUBCH_IP);                // the audio layers first,
            if (flags & DABGPU_SUBCH_MOT) flags &= ~DABGPU_SUBCH_IP;                                 // MOT before IP)
            dabgpu_subch e;
            e.startAddr = s.StartAddr;
            e.length = s.Length;
            e.bitRate = s.BitRate;
            e.protLevel = s.protLevel;
            e.uepFlag = s.uepFlag;
            e.flags = (int16_t)flags;
            T.sub[pos] = e;
            T.ids[pos] = (uint8_t)lane;
        }
        if (lane == 0) T.n = __popcll(mask);
    }
    __syncthreads();
    int changed;
    {
        const uint32_t *tw = (const uint32_t *)&T;
        uint32_t *lw = (uint32_t *)&S.table, *gw = (uint32_t *)(J.table + slot);
        bool diff = false;
        for (int i = lane; i < FIB_TABLE_WORDS; i += 64) {
            diff |= tw[i] != lw[i];
            lw[i] = tw[i];
            gw[i] = tw[i];
        }
        changed = __ballot(diff) ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) {
        dabgpu_fic_run R = {};
        R.parsed = parsed;
        R.skipped = skipped;
        for (int k = 0; k < 8; k++) R.figs[k] = figs[k];
        R.n_events = n_events;
        R.overrun = overrun;
        R.table_changed = changed;
        J.run[slot] = R;
    }
    {
        uint4 *sw = (uint4 *)state;
        const uint4 *lw = (const uint4 *)&S;
        for (int i = lane; i < (int)(sizeof(dabgpu_fic_db) / 16); i += 64) sw[i] = lw[i];
    }
}

// fib_processor::clearEnsemble (:1149-1163): lane = table entry
__global__ __launch_bounds__(64) void k_fic_clear(dabgpu_fic_db *db) {
    dabgpu_fic_db &D = db[blockIdx.x];
    const int lane = threadIdx.x;
    D.components[lane] = dabgpu_fic_component{};
    D.sub[lane] = dabgpu_fic_subch{};
    dabgpu_fic_service s = D.services[lane];                              // language, programType, hasLanguage (and hasName) stay
    s.inUse = 0;
    s.serviceId = 0;
    s.charset = 0;
    s.data_suffix = 0;
    for (int i = 0; i < 16; i++) s.label[i] = 0;
    D.services[lane] = s;
    if (lane < 16) D.label[lane] = 0;
    if (lane == 0) {
        D.EId = 0;
        D.charset = 0;
        D.named = 0;
    }
}

hipError_t launch_fib(hipStream_t st, const FibJob &J) {
    if (J.n_slots <= 0) return hipSuccess;
    if (J.n_fibs < 0 || J.event_slots < 0 || J.stride < 0 || !J.db || !J.table || !J.run || ((uintptr_t)J.db & 15) ||
        ((uintptr_t)J.table & 3) || ((uintptr_t)J.events & 3) || J.event_slots > (1 << 24) || (J.n_fibs && (!J.fibs || !J.ok)) || (J.event_slots && !J.events) ||
        (J.bit_src && (((uintptr_t)J.fibs | (uintptr_t)J.stride) & 7)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fib_walk, dim3((unsigned)J.n_slots), dim3(64), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_fic_clear(hipStream_t st, dabgpu_fic_db *db, int n_slots) {
    if (n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fic_clear, dim3((unsigned)n_slots), dim3(64), 0, st, db);
    return hipGetLastError();
}

}  // namespace dab
