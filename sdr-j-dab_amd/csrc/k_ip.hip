// IP layer: checked MSC data groups -> the UDP payloads of their IPv4 datagrams, for every packet
// entry flagged DABGPU_SUBCH_IP.  ip_dataHandler::add_mscDatagroup (ip-datahandler.cpp:40-127), bit
// for bit what host/msc_consumers.cpp's ipAssembler does; the rules where the reference is
// undefined are those of dabgpu_ip_groups (include/dabgpu.h).
//
// An ip_dataHandler keeps two counters and nothing else, so a run's groups are independent but for
// their order:
//   k_ip_walk  one wave per slot, 64 groups a batch, one group per lane.  A lane reads its group's
//              record and IPv4 header (at most 60 bytes), classifies it and sums the header.  What
//              depends on order comes from ballots: a lane's rank among the groups that reach
//              process_ipVector places it in the 100-datagram window (at most one window closes
//              per batch: they are 100 datagrams apart), and a lane-prefix sum of the payload
//              lengths, each rounded up to 16, gives the arena offsets.  handled, crc_errors and
//              the arena fill carry from batch to batch as wave-uniform scalars.
//   k_ip_copy  workgroups over (slot, part of the run's groups): one wave per delivered datagram
//              copies its payload, 16 or 4 bytes per lane and store where the destination allows.
// Every read is held against the group's stored bytes and every write against the output arena by
// the walk: no record, however hostile, makes either kernel leave them.  Plain vector loads and
// stores only; a slot's state is its own, so nothing is atomic.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

// A group's bytes as ip_dataHandler reads them: rule 1 past the stored end, and the group's own CRC
// field complemented, as check_CRC_bits (:54) has left it by then
struct IpGroup {
    const uint8_t *d;   // the group's first byte
    int nb, crc0;       // stored bytes; index of the CRC field (nb when the group has none)
    __device__ __forceinline__ uint32_t operator()(int64_t i) const {
        if (i < 0 || i >= nb) return 0u;
        const uint32_t v = d[i];
        return i >= crc0 ? v ^ 0xFFu : v;
    }
};

// the record holds a group the reference would go on with, inside its arena (rule 5)
__device__ __forceinline__ bool ip_group_ok(const dabgpu_datagroup &G, int64_t arena) {
    return (G.flags & DABGPU_DG_ACCEPTED) && G.offset >= 0 && G.nbytes > 0 && G.data_offset >= 0 &&
           (int64_t)G.offset + G.nbytes <= arena;
}

__global__ __launch_bounds__(64) void k_ip_walk(IpJob J) {
    const int lane = threadIdx.x, slot = blockIdx.x;
    if (J.on && !J.on[slot]) {                            // an entry that is not flagged: not walked
        if (lane < (int)(sizeof(dabgpu_ip_run) / 4)) ((int32_t *)(J.ip_run + slot))[lane] = 0;
        return;
    }
    const int ng = max(0, min(J.run[slot].n_groups, J.gslots));
    const dabgpu_datagroup *groups = J.groups + (int64_t)slot * J.gslots;
    const uint8_t *arena = J.bytes + (int64_t)slot * J.arena;
    dabgpu_ip_result *results = J.results + (int64_t)slot * J.gslots;
    // wave-uniform: the handler's counters, the arena's fill and the run's tallies
    int handled = J.state[slot].handled, crc_errors = J.state[slot].crc_errors;
    int64_t fill = 0;
    int n_datagrams = 0, n_bytes = 0, counts = 0;         // counts: in lane s, the groups that ended with status s
    const uint64_t below = (1ull << lane) - 1ull;

    for (int g0 = 0; g0 < ng; g0 += 64) {
        const int g = g0 + lane;
        int status = -1, ip_len = 0, plen = 0;            // status -1: no group in this lane
        bool reach = false, bad = false;
        if (g < ng) {
            const dabgpu_datagroup G = groups[g];
            status = DABGPU_IP_NOT_ACCEPTED;
            if (ip_group_ok(G, J.arena)) {
                const IpGroup B{arena + G.offset, G.nbytes, (G.flags & DABGPU_DG_CRC) ? G.nbytes - 2 : G.nbytes};
                const int64_t nx = G.data_offset;         // (:57-74) as the packet layer restates it
                auto D = [&](int i) -> uint32_t { return i < ip_len ? B(nx + i) : 0u; };   // ipVector [i]; rule 3 past ipLength
                ip_len = (int)((B(nx + 2) << 8) | B(nx + 3));                              // (:79)
                const uint32_t b0 = D(0);
                if (!(ip_len < B.nb)) {                   // (:80)
                    status = DABGPU_IP_TOO_LONG;
                } else if (ip_len == 0 || (b0 >> 4) != 4u) {   // rule 2; (:85) a signed shift leaves 4 only for 0x4?
                    status = DABGPU_IP_NOT_V4;
                } else {
                    reach = true;
                    const int hs = (int)(b0 & 15u);
                    uint32_t sum = 0;
                    for (int i = 0; i < 2 * hs; i++) sum += (D(2 * i) << 8) | D(2 * i + 1);   // (:105-106)
                    sum = (sum >> 16) + (sum & 0xFFFFu);                                      // one fold (:107)
                    bad = (~sum & 0xFFFFu) != 0;
                    plen = ip_len - 4 * hs - 8;
                    status = bad ? DABGPU_IP_CHECKSUM : D(9) != 17u ? DABGPU_IP_NOT_UDP : plen < 0 ? DABGPU_IP_MALFORMED
                                                                                                     : DABGPU_IP_DELIVERED;
                }
            }
        }
        // the window (:100-104): it steps before the datagram's own checksum test
        const uint64_t R = __ballot(reach), BAD = __ballot(bad);
        const int rank = __popcll(R & below) + 1, nreach = __popcll(R);
        const int64_t first = handled >= 99 ? 1 : 100 - (int64_t)handled;     // the rank whose ++handledPackets reaches 100
        const uint64_t E = __ballot(reach && rank == first);
        int quality = -1;
        if (E) {
            const int el = __builtin_ctzll(E);
            const uint64_t before = (1ull << el) - 1ull;
            if (lane == el) quality = (int16_t)(100u - ((uint32_t)crc_errors + (uint32_t)__popcll(BAD & before)));
            crc_errors = __popcll(BAD & ~before);
            handled = nreach - (int)first;
        } else {
            crc_errors += __popcll(BAD);
            handled += nreach;
        }
        // the arena: payloads in group order, each at a multiple of 16 (rule 6: what does not fit is malformed)
        const int room = status == DABGPU_IP_DELIVERED ? (plen + 15) & ~15 : 0;
        int incl = room;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const int up = __shfl_up(incl, k);
            if (lane >= k) incl += up;
        }
        const int64_t off = fill + incl - room;
        if (status == DABGPU_IP_DELIVERED && off + plen > J.out_arena) status = DABGPU_IP_MALFORMED;
        fill = min(fill + __shfl(incl, 63), (int64_t)1 << 40);
        const bool ok = status == DABGPU_IP_DELIVERED;
        if (status >= 0) {
            dabgpu_ip_result r;
            r.offset = ok ? (int32_t)off : 0;
            r.nbytes = ok ? plen : 0;
            r.status = (int16_t)status;
            r.quality = (int16_t)quality;
            r.ip_bytes = ip_len;
            results[g] = r;
        }
        n_datagrams += __popcll(__ballot(ok));
        int nb = ok ? plen : 0;
#pragma unroll
        for (int k = 32; k; k >>= 1) nb += __shfl_xor(nb, k);
        n_bytes += nb;
#pragma unroll
        for (int s = 0; s < 7; s++) {
            const int c = __popcll(__ballot(status == s));
            if (lane == s) counts += c;
        }
    }
    if (lane == 0) {
        J.state[slot].handled = handled;
        J.state[slot].crc_errors = crc_errors;
    }
    // dabgpu_ip_run: n_datagrams, n_bytes, counts[7], reserved[3]
    const int count = __shfl(counts, max(lane - 2, 0));
    if (lane < (int)(sizeof(dabgpu_ip_run) / 4))
        ((int32_t *)(J.ip_run + slot))[lane] = lane == 0 ? n_datagrams : lane == 1 ? n_bytes : lane < 9 ? count : 0;
}

constexpr int IP_COPY_THREADS = 256, IP_COPY_PARTS = 8;

__global__ __launch_bounds__(IP_COPY_THREADS) void k_ip_copy(IpJob J) {
    const int lane = threadIdx.x & 63, slot = blockIdx.x;
    if (J.on && !J.on[slot]) return;
    const int ng = max(0, min(J.run[slot].n_groups, J.gslots));
    const dabgpu_datagroup *groups = J.groups + (int64_t)slot * J.gslots;
    const dabgpu_ip_result *results = J.results + (int64_t)slot * J.gslots;
    const uint8_t *arena = J.bytes + (int64_t)slot * J.arena;
    uint8_t *out = J.out + (int64_t)slot * J.out_arena;
    const int nwave = IP_COPY_PARTS * (IP_COPY_THREADS / 64);
    // a wave per delivered datagram (g is wave-uniform)
    for (int g = blockIdx.y * (IP_COPY_THREADS / 64) + (threadIdx.x >> 6); g < ng; g += nwave) {
        const dabgpu_ip_result r = results[g];
        const int n = r.nbytes;
        if (r.status != DABGPU_IP_DELIVERED || n <= 0 || r.offset < 0 || (int64_t)r.offset + n > J.out_arena) continue;
        const dabgpu_datagroup G = groups[g];
        if (!ip_group_ok(G, J.arena)) continue;           // (the walk delivered it: it is)
        const IpGroup B{arena + G.offset, G.nbytes, (G.flags & DABGPU_DG_CRC) ? G.nbytes - 2 : G.nbytes};
        const int64_t p0 = (int64_t)G.data_offset + r.ip_bytes - n;           // the payload's first byte in the group
        auto P = [&](int i) -> uint32_t { return B(p0 + i); };                // i < n: inside ipLength
        auto W = [&](int i) -> uint32_t { return P(i) | (P(i + 1) << 8) | (P(i + 2) << 16) | (P(i + 3) << 24); };
        uint8_t *dst = out + r.offset;
        int done = 0;
        if (((uintptr_t)dst & 15) == 0) {
            for (int v = lane; v < (n >> 4); v += 64) ((uint4 *)dst)[v] = make_uint4(W(16 * v), W(16 * v + 4), W(16 * v + 8), W(16 * v + 12));
            done = n & ~15;
        } else if (((uintptr_t)dst & 3) == 0) {
            for (int v = lane; v < (n >> 2); v += 64) ((uint32_t *)dst)[v] = W(4 * v);
            done = n & ~3;
        }
        for (int i = done + lane; i < n; i += 64) dst[i] = (uint8_t)P(i);
    }
}

hipError_t launch_ip(hipStream_t st, const IpJob &J) {
    if (J.n_slots <= 0) return hipSuccess;
    if (J.gslots < 0 || J.arena < 0 || J.arena > 0x7FFFFFFF || J.out_arena < 0 || J.out_arena > 0x7FFFFFFF)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ip_walk, dim3((unsigned)J.n_slots), dim3(64), 0, st, J);
    hipLaunchKernelGGL(k_ip_copy, dim3((unsigned)J.n_slots, IP_COPY_PARTS), dim3(IP_COPY_THREADS), 0, st, J);
    return hipGetLastError();
}

}  // namespace dab
