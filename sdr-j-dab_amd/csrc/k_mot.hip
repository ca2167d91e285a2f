// MOT layer: checked MSC data groups -> slides and files, for every packet entry flagged
// DABGPU_SUBCH_MOT.  motHandler::process_mscGroup in header mode (mot-data.cpp:679-728), bit for
// bit what host/msc_consumers.cpp's motAssembler does; the rules where the reference is
// undefined are those of dabgpu_mot_groups (include/dabgpu.h).
//
// A motHandler is a chain: every group sees the table the groups before it left.  What a
// group does to the table is a few dozen integer operations; what it does to memory is one copy.
// So the work is split by kind, not by group:
//   k_mot_walk  one wave per slot.  The table (head and 16 entries, 2960 bytes) lives in LDS for
//               the pass; getHandle and newEntry's pick are ballots over the entries, one per
//               lane; the marks are four 32-bit masks, so isComplete is a mask compare.  It
//               walks the run's groups in order, updates the table, writes the object records
//               and an ordered list of byte operations: clear a body, copy a segment into a
//               body, snapshot a body into the output arena.  It touches no body byte.
//   k_mot_copy  one workgroup per slot executes that list in order, a barrier between
//               operations (a snapshot reads what the copies before it wrote), 16 bytes per
//               lane where source and destination allow.
// Every offset in the list was checked against its buffer by the walk: no record, however
// hostile, makes either kernel leave [0, bodySize) of a body, the group's stored bytes or the
// output arena.  Plain vector stores only; a slot's state is its own, so nothing is atomic.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

enum { MOT_OP_CLEAR = 1, MOT_OP_SEGMENT = 2, MOT_OP_SNAPSHOT = 3 };

__device__ __forceinline__ bool mot_marked(const dabgpu_mot_entry &e, int n) { return (e.marked[n >> 5] >> (n & 31)) & 1u; }
// marks 0 .. n-1 (n <= 100) as word w of the four
__device__ __forceinline__ uint32_t mot_below(int n, int w) {
    const int k = n - 32 * w;
    return k <= 0 ? 0u : k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u;
}

__global__ __launch_bounds__(64) void k_mot_walk(MotJob J) {
    __shared__ dabgpu_mot_head H;
    __shared__ dabgpu_mot_entry T[DABGPU_MOT_ENTRIES];
    const int lane = threadIdx.x, slot = blockIdx.x;
    uint8_t *state = J.state + (int64_t)slot * J.state_bytes;
    {
        const uint32_t *sw = (const uint32_t *)state;
        uint32_t *hw = (uint32_t *)&H, *tw = (uint32_t *)T;
        constexpr int NH = sizeof(dabgpu_mot_head) / 4, NT = DABGPU_MOT_ENTRIES * sizeof(dabgpu_mot_entry) / 4;
        if (lane < NH) hw[lane] = sw[lane];
        for (int i = lane; i < NT; i += 64) tw[i] = sw[NH + i];
    }
    __syncthreads();
    const int src = J.src ? J.src[slot] : slot;
    const int ng = src >= 0 ? max(0, min(J.run[src].n_groups, J.gslots)) : 0;
    const dabgpu_datagroup *groups = J.groups + (int64_t)max(src, 0) * J.gslots;
    const uint8_t *arena = J.bytes + (int64_t)max(src, 0) * J.arena;
    dabgpu_mot_object *objects = J.objects + (int64_t)slot * J.gslots;
    int4 *ops = J.ops + (int64_t)slot * 2 * J.gslots;
    int nops = 0, nobj = 0, nout = 0, malformed = 0, bad_segment = 0, other = 0;
    // everything below is the same in every lane (wave-uniform) unless a lane index appears
    auto push = [&](int kind, int from, int to, int n) {
        if (lane == 0) ops[nops] = make_int4(kind, from, to, n);
        nops++;
    };

    // processSegment (:278-312) on entry h; src_off: the segment's first byte in the arena
    auto segment = [&](int h, int src_off, int n, int size, bool last, int g, int cif) {
        const dabgpu_mot_entry &E = T[h];
        if ((E.flags & DABGPU_MOT_TOO_LARGE) || E.bodySize > J.max_body || size < 0) return;   // rules 3 and 4
        if (mot_marked(E, n)) return;
        int ss = E.segmentSize;
        if (!last && ss == -1) ss = size;                                     // (the latch outlives a failed check)
        const bool fits = ss >= 0 && (int64_t)n * ss + size <= E.bodySize;
        int nseg = E.numofSegments;
        uint32_t m[4] = {E.marked[0], E.marked[1], E.marked[2], E.marked[3]};
        bool complete = false;
        if (fits) {
            if (size > 0) push(MOT_OP_SEGMENT, src_off, h * J.body_cap + n * ss, size);
            m[n >> 5] |= 1u << (n & 31);
            if (last) nseg = n + 1;
            complete = nseg != -1;                                            // isComplete (:578-588)
            for (int w = 0; w < 4; w++) complete = complete && (m[w] & mot_below(nseg, w)) == mot_below(nseg, w);
        }
        const int ct = E.contentType, body = E.bodySize;
        const int kind = ct == 2 ? DABGPU_MOT_SLIDE : ct == 7 ? DABGPU_MOT_EPG : DABGPU_MOT_FILE;
        const bool unmark = complete && kind == DABGPU_MOT_SLIDE && H.old_slide;   // show_slide (:337-346)
        if (complete) {                                                       // handleComplete (:315-336)
            int off = 0, nb = 0, fl = 0;
            if (kind != DABGPU_MOT_EPG) {
                off = (nout + 15) & ~15;
                if ((int64_t)off + body > J.out_arena) {
                    off = 0;
                    fl = DABGPU_MOT_OVERFLOW;
                } else {
                    nb = body;
                    if (body > 0) push(MOT_OP_SNAPSHOT, h * J.body_cap, off, body);
                    nout = off + body;
                }
            }
            dabgpu_mot_object *O = objects + nobj++;
            if (lane == 0) {
                O->group = g;
                O->cif = cif;
                O->offset = off;
                O->nbytes = nb;
                O->transportId = (uint16_t)E.transportId;
                O->contentType = (uint8_t)ct;
                O->kind = (uint8_t)kind;
                O->contentsubType = (uint16_t)E.contentsubType;
                O->flags = (uint16_t)fl;
                O->name_len = E.name_len;
            }
            for (int i = lane; i < DABGPU_MOT_NAME_BYTES; i += 64) O->name[i] = E.name[i];
        }
        __syncthreads();                                                      // the reads of E above, before lane 0 writes
        if (lane == 0) {
            T[h].segmentSize = ss;
            if (fits) {
                T[h].numofSegments = nseg;
                for (int w = 0; w < 4; w++) T[h].marked[w] = unmark ? m[w] & ~mot_below(nseg, w) : m[w];
            }
            if (complete && kind == DABGPU_MOT_SLIDE) H.old_slide = 1;
        }
    };

    for (int g = 0; g < ng; g++) {
        __syncthreads();                                                      // the table as the last group left it
        const dabgpu_datagroup G = groups[g];
        if ((G.flags & (DABGPU_DG_ACCEPTED | DABGPU_DG_TRANSPORT)) != (DABGPU_DG_ACCEPTED | DABGPU_DG_TRANSPORT)) continue;
        const bool hdr = G.groupType == 3 && G.segmentNumber == 0, last = G.flags & DABGPU_DG_LAST;
        if (!hdr && G.groupType != 4) {                                       // rule 6
            other++;
            continue;
        }
        const int dn = G.data_nbytes;
        if (G.offset < 0 || G.nbytes < 0 || G.data_offset < 0 || dn < 0 || (int64_t)G.data_offset + dn > G.nbytes ||
            (int64_t)G.offset + G.nbytes > J.arena) {                         // the record points outside its arena
            malformed++;
            continue;
        }
        const int base = G.offset + G.data_offset;
        const uint8_t *d = arena + base;
        auto B = [&](int i) -> uint32_t { return i >= 0 && i < dn ? d[i] : 0u; };   // rule 1
        const int size = (int)(((B(0) & 0x1Fu) << 8) | B(1));
        if (dn < 2 || size + 2 > dn) {
            malformed++;
            continue;
        }
        const int tid = G.transportId;
        // getHandle (:590-598): the entries sit in lanes
        const uint64_t HIT = __ballot(lane < DABGPU_MOT_ENTRIES && T[lane & 15].order != 0 && T[lane & 15].transportId == tid);
        if (!hdr) {
            if (G.segmentNumber >= 100) {                                     // rule 2
                bad_segment++;
                continue;
            }
            if (HIT) segment(__builtin_ctzll(HIT), base + 2, G.segmentNumber, size, last, g, G.cif);
            continue;
        }
        if (HIT) continue;                                                    // (:113-114)
        const int hsize = (int)(((B(5) & 0x0Fu) << 9) | B(6) | (B(7) >> 7)); // (:687-689: d[6] unshifted)
        const int bsize = (int)((B(2) << 20) | (B(3) << 12) | (B(4) << 4) | (B(5) >> 4));
        // newEntry (:612-656): the first free entry, else the least ordernumber
        const int order = lane < DABGPU_MOT_ENTRIES ? T[lane & 15].order : 0x7FFFFFFF;
        const uint64_t FREE = __ballot(lane < DABGPU_MOT_ENTRIES && order == 0);
        int h;
        if (FREE) {
            h = __builtin_ctzll(FREE);
        } else {
            int lo = order;
#pragma unroll
            for (int k = 8; k; k >>= 1) lo = min(lo, __shfl_xor(lo, k));      // lanes 16.. hold INT_MAX and stay out (k < 16)
            h = __builtin_ctzll(__ballot(lane < DABGPU_MOT_ENTRIES && order == __shfl(lo, 0)));
        }
        // processHeader (:62-111) on segment = d + 2
        auto S = [&](int i) -> uint32_t { return B(i + 2); };
        const int ct = (int)((S(5) >> 1) & 0x3Fu), cst = (int)(((S(5) & 1u) << 8) | S(6));
        int p = 7, name_len = 0;
        while (p < hsize) {
            const uint32_t pli = S(p) >> 6, pid = S(p) & 0x3Fu;
            if (pli == 0) {
                p += 1;
            } else if (pli == 1) {
                p += 2;
            } else if (pli == 2) {
                p += 5;
            } else {
                int len;
                if (S(p + 1) & 0x80u) {
                    len = (int)(((S(p + 1) & 0x7Fu) << 8) | S(p + 2));
                    p += 3;
                } else {
                    len = (int)(S(p + 1) & 0x7Fu);
                    p += 2;
                }
                if (pid == 12 && len > 1) {
                    for (int i = name_len + lane; i < min(name_len + len - 1, DABGPU_MOT_NAME_BYTES); i += 64)
                        T[h].name[i] = (uint8_t)S(p + 1 + i - name_len);     // rule 5: the first 128 bytes
                    name_len += len - 1;
                }
                p += len;
            }
        }
        const bool too_large = bsize > J.max_body;                            // rule 3
        for (int i = max(name_len, 0) + lane; i < DABGPU_MOT_NAME_BYTES; i += 64) T[h].name[i] = 0;
        if (lane == 0) {
            dabgpu_mot_entry &E = T[h];
            E.order = ++H.created;
            E.transportId = tid;
            E.bodySize = bsize;
            E.segmentSize = -1;
            E.numofSegments = -1;
            E.contentType = ct;
            E.contentsubType = cst;
            E.flags = too_large ? DABGPU_MOT_TOO_LARGE : 0;
            E.name_len = name_len;
            E.reserved = 0;
        }
        if (!too_large && bsize > 0) push(MOT_OP_CLEAR, 0, h * J.body_cap, bsize);                      // rule 4
        __syncthreads();
        // a header segment that is not the last carries body bytes behind the header (:121-132)
        if (!last) segment(h, base + 2 + hsize, 0, size - hsize, false, g, G.cif);
    }
    __syncthreads();
    {
        uint32_t *sw = (uint32_t *)state;
        const uint32_t *hw = (const uint32_t *)&H, *tw = (const uint32_t *)T;
        constexpr int NH = sizeof(dabgpu_mot_head) / 4, NT = DABGPU_MOT_ENTRIES * sizeof(dabgpu_mot_entry) / 4;
        if (lane < NH) sw[lane] = hw[lane];
        for (int i = lane; i < NT; i += 64) sw[NH + i] = tw[i];
    }
    const int used = __popcll(__ballot(lane < DABGPU_MOT_ENTRIES && T[lane & 15].order != 0));
    if (lane == 0) {
        dabgpu_mot_run R = {};
        R.n_objects = nobj;
        R.n_bytes = nout;
        R.malformed = malformed;
        R.bad_segment = bad_segment;
        R.other_types = other;
        R.entries = used;
        J.mot_run[slot] = R;
        J.nops[slot] = nops;
    }
}

constexpr int MOT_COPY_THREADS = 256;

__global__ __launch_bounds__(MOT_COPY_THREADS) void k_mot_copy(MotJob J) {
    const int t = threadIdx.x, slot = blockIdx.x;
    const int src = J.src ? J.src[slot] : slot;
    const int nops = min(J.nops[slot], 2 * J.gslots);
    if (nops <= 0) return;
    uint8_t *bodies = J.state + (int64_t)slot * J.state_bytes + MOT_TABLE_BYTES;
    const uint8_t *arena = J.bytes + (int64_t)max(src, 0) * J.arena;
    uint8_t *out = J.out + (int64_t)slot * J.out_arena;
    const int4 *ops = J.ops + (int64_t)slot * 2 * J.gslots;
    for (int k = 0; k < nops; k++) {
        const int4 op = ops[k];
        const int n = op.w;
        if (op.x == MOT_OP_CLEAR) {
            uint8_t *dst = bodies + op.z;                                     // an entry's body starts at a multiple of 16
            const int nv = n >> 4;
            for (int i = t; i < nv; i += MOT_COPY_THREADS) ((uint4 *)dst)[i] = make_uint4(0, 0, 0, 0);
            for (int i = 16 * nv + t; i < n; i += MOT_COPY_THREADS) dst[i] = 0;
        } else {
            const uint8_t *s = op.x == MOT_OP_SEGMENT ? arena + op.y : bodies + op.y;
            uint8_t *dst = op.x == MOT_OP_SEGMENT ? bodies + op.z : out + op.z;
            if ((((uintptr_t)s | (uintptr_t)dst) & 15) == 0) {
                const int nv = n >> 4;
                for (int i = t; i < nv; i += MOT_COPY_THREADS) ((uint4 *)dst)[i] = ((const uint4 *)s)[i];
                for (int i = 16 * nv + t; i < n; i += MOT_COPY_THREADS) dst[i] = s[i];
            } else {
                for (int i = t; i < n; i += MOT_COPY_THREADS) dst[i] = s[i];
            }
        }
        __syncthreads();                                                      // the next operation may read these bytes
    }
}

hipError_t launch_mot(hipStream_t st, const MotJob &J) {
    if (J.n_slots <= 0) return hipSuccess;
    if (J.gslots < 0 || J.max_body <= 0 || J.max_body > (1 << 24) || J.body_cap < J.max_body || (J.body_cap & 15) ||
        J.state_bytes != MOT_TABLE_BYTES + (int64_t)DABGPU_MOT_ENTRIES * J.body_cap || J.arena < 0 || J.arena > 0x7FFFFFFF ||
        J.out_arena < 0 || J.out_arena > 0x7FFFFFFF || ((uintptr_t)J.state & 15) || ((uintptr_t)J.out & 15) || (J.out_arena & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mot_walk, dim3((unsigned)J.n_slots), dim3(64), 0, st, J);
    hipLaunchKernelGGL(k_mot_copy, dim3((unsigned)J.n_slots), dim3(MOT_COPY_THREADS), 0, st, J);
    return hipGetLastError();
}

}  // namespace dab
