// Packet-mode data layer: MSC bits -> checked MSC data groups, for every entry flagged
// DABGPU_SUBCH_PACKET.  mscDatagroup::handlePackets + handlePacket (msc-datagroup.cpp:221-319)
// and the generic data-group header and CRC of mot_databuilder::add_mscDatagroup
// (mot-databuilder.cpp:37-95), bit for bit what host/msc_consumers.cpp's packetAssembler does.
//
// Packets never span a CIF and are 24, 48, 72 or 96 bytes long, so a CIF of a <= 384 kbit/s
// entry has at most 48 cells of 24 bytes and lane l of a wave looks at cell l.  Four kernels:
//   k_pkt_scan      one wave per (stream, slot, CIF): the reference's walk resolves which cells
//                   start a packet, the CRC of every packet by linearity (each lane its cell
//                   from zero, shifted by x^(8 * bytes after), xor over the packet's cells,
//                   the all-ones term per length), one 32-bit record per cell
//   k_pkt_assemble  one wave per (stream, slot) over the records of the run's CIFs in order;
//                   per CIF the state machine is ballot arithmetic (no loop over packets).
//                   Writes the group records, the per-CIF info, one take record per cell
//                   (which series it feeds, at which byte) and the fate of every series
//   k_pkt_copy      one wave per (stream, slot, CIF) and one for the carried bytes: the bytes of
//                   completed groups to the arena, those of the series in flight to the carry
//   k_pkt_groups    a wave per completed group: its CRC (the same CRC by linearity over 64
//                   lanes, msc_feed.h's wave_crc16) and the header fields
// The delivery rule, the row address and the row reader are msc_feed.h's, the CRC arithmetic
// crc16_poly.h's.
// Only the packetState, the address latch, the 500-packet window and the bytes of the series
// in flight cross CIFs.  msc_bits_d is only read: check_CRC_bits' in-place inversion of a
// packet's CRC field is applied where a copy reads it (useful length past the data field).
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

constexpr int PK_MAX_ROW = 24 * PK_MAX_CELLS;     // bytes of a CIF at 384 kbit/s

// the all-ones start register after a packet of lc + 1 cells
__device__ __forceinline__ uint32_t pk_ones(int lc) {
    constexpr uint32_t o1 = crc16::crc_ones(24), o2 = crc16::crc_ones(48), o3 = crc16::crc_ones(72), o4 = crc16::crc_ones(96);
    return lc == 0 ? o1 : lc == 1 ? o2 : lc == 2 ? o3 : o4;
}

__device__ __forceinline__ int pk_top(uint64_t m) { return 63 - __builtin_clzll(m); }   // m != 0

// the CIF's row as nbytes bytes in LDS
__device__ __forceinline__ void pk_load_row(uint8_t *dst, const uint8_t *__restrict__ row, int packed, int nbytes, int lane) {
    for (int k = lane; k < nbytes; k += 64) dst[k] = (uint8_t)row_byte(row, packed, k);
}

// record of a cell: bit 0 a packet starts here, 1 its CRC is good, 2-3 first/last,
// 4-5 length code, 6-12 useful length, 13-22 address
__global__ __launch_bounds__(64) void k_pkt_scan(PkJob J) {
    __shared__ uint8_t row[PK_MAX_ROW];
    const int lane = threadIdx.x;
    const MscFeed &F = J.feed;
    const int c = blockIdx.x % F.ncif, e = blockIdx.x / F.ncif, s = e / J.npk;
    uint32_t *rec = J.rec + ((int64_t)e * F.ncif + c) * J.ncell;
    if (!fed(F, J.map, e, s, c)) {
        if (lane < J.ncell) rec[lane] = 0;
        return;
    }
    const int ncell = min((int)J.map.br[e] >> 3, J.ncell);
    pk_load_row(row, msc_row(F, s, c, J.map.sub[e]), F.packed, 24 * ncell, lane);
    __syncthreads();
    const bool in = lane < ncell;
    const uint8_t *cell = row + 24 * (in ? lane : 0);
    const int lc = in ? cell[0] >> 6 : 0;
    // the reference's walk (handlePackets): wave-uniform on the ballots of the length codes
    const uint64_t m1 = __ballot(in && lc == 1), m2 = __ballot(in && lc == 2), m3 = __ballot(in && lc == 3);
    uint64_t starts = 0;
    for (int pos = 0; pos < ncell;) {
        const int L = ((m1 >> pos) & 1) ? 2 : ((m2 >> pos) & 1) ? 3 : ((m3 >> pos) & 1) ? 4 : 1;
        if (pos + L > ncell) break;                      // the claimed length exceeds what is left
        starts |= 1ull << pos;
        pos += L;
    }
    uint32_t part = 0;
    if (in)
        for (int i = 0; i < 24; i++) part = crc16::crc_byte(part, cell[i]);
    // a start lane gathers its packet's cells (all lanes shuffle, the packet's own are used)
    uint32_t crc = part;
    const bool st = (starts >> lane) & 1;
    constexpr uint32_t x24 = crc16::xpow8(24);           // one cell further
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const uint32_t p = __shfl_down(part, k);
        if (st && k <= lc) crc = crc16::mulmod(crc, x24) ^ p;
    }
    const bool ok = (crc ^ pk_ones(lc)) == crc16::CRC_GOOD;
    if (lane < J.ncell) {
        uint32_t r = 0;
        if (st)
            r = 1u | (ok ? 2u : 0u) | (((cell[0] >> 2) & 3u) << 2) | ((uint32_t)lc << 4) | ((cell[2] & 0x7Fu) << 6) |
                ((((cell[0] & 3u) << 8) | cell[1]) << 13);
        rec[lane] = r;
    }
}

__global__ __launch_bounds__(64) void k_pkt_assemble(PkJob J) {
    const int lane = threadIdx.x, e = blockIdx.x, s = e / J.npk, j = e % J.npk;
    PkState st = J.state[e];
    const int nbytes_row = 3 * J.map.br[e];
    const uint64_t below = (1ull << lane) - 1ull;
    int32_t *segtab = J.segtab + (int64_t)e * (1 + J.feed.ncif * J.ncell);
    dabgpu_datagroup *groups = J.groups + (int64_t)e * J.gslots;
    st.prev_state = st.state;
    st.prev_pending = st.pending;
    if (lane == 0 && st.state == 0) segtab[0] = -1;
    int ngroups = 0, nstored = 0, serial_next = 1, open_serial = 0;
    // what decides `fed` does not change over the run, and the next CIF's records are loaded
    // while this one's are worked on: the loop is a chain of latencies, nothing else
    const int sub = J.map.sub[e], nfed = J.feed.ncifs[s];
    const int64_t rel0 = rel_cif(J.feed, J.map, e, s);
    const uint32_t *rec_e = J.rec + (int64_t)e * J.feed.ncif * J.ncell;
    uint32_t rnext = lane < J.ncell ? rec_e[lane] : 0u;
    for (int c = 0; c < J.feed.ncif; c++) {
        const bool on = fed(sub, nfed, rel0, c);
        const int64_t cell0 = ((int64_t)e * J.feed.ncif + c) * J.ncell;
        dabgpu_packet_info *info = J.info + ((int64_t)s * J.feed.ncif + c) * J.npk + j;
        const uint32_t r = rnext;                        // (k_pkt_scan wrote 0 for a CIF that is not fed)
        if (c + 1 < J.feed.ncif) rnext = lane < J.ncell ? rec_e[(int64_t)(c + 1) * J.ncell + lane] : 0u;
        const bool valid = r & 1u, ok = (r >> 1) & 1u;
        const int fl = (r >> 2) & 3, useful = (r >> 6) & 0x7F, addr = (r >> 13) & 0x3FF;
        const uint64_t V = __ballot(valid), BAD = __ballot(valid && !ok);
        const int npk = __popcll(V);
        // show_mscErrors: the packet that brings handledPackets to 500 emits before its own CRC
        int quality = -1;
        if (st.handled + npk >= 500) {
            const int rank = 500 - st.handled;           // 1-based among this CIF's packets
            const int el = __builtin_ctzll(__ballot(valid && __popcll(V & below) == rank - 1));
            const int before = __popcll(BAD & ((1ull << el) - 1ull));
            quality = 100 - (st.crc_errors + before) / 5;
            st.crc_errors = __popcll(BAD) - before;
            st.handled = npk - rank;
        } else {
            st.handled += npk;
            st.crc_errors += __popcll(BAD);
        }
        const uint64_t EFF = __ballot(valid && ok && addr != 0);
        if (st.address == -1 && EFF) st.address = __shfl(addr, __builtin_ctzll(EFF));
        const bool act = valid && ok && addr != 0 && addr == st.address;
        const uint64_t A1 = __ballot(act && fl == 1), A2 = __ballot(act && fl == 2), A3 = __ballot(act && fl == 3);
        const uint64_t NZ = A1 | A2 | A3, pnz = NZ & below;
        // packetState before this packet: the last earlier packet with first/last != 0 decides
        const int sb = pnz ? (int)((A2 >> pk_top(pnz)) & 1) : st.state;
        const bool start = act && (fl == 2 || (fl == 3 && sb == 0));
        const bool takes = act && (start || (sb == 1 && fl < 2));
        const bool complete = act && ((fl == 3 && sb == 0) || (fl == 1 && sb == 1));
        const bool abort = act && sb == 1 && fl >= 2;
        const int n = takes ? min(useful, nbytes_row - (24 * lane + 3)) : 0;       // the copy stops at the CIF's end
        const int E = wave_scan_excl(n, lane);
        const int total = __shfl(E + n, 63);
        const uint64_t STARTS = __ballot(start), psb = STARTS & below;
        // the series open before this packet, and the one it feeds
        const int slb = psb ? pk_top(psb) : 0;
        const int E_slb = __shfl(E, slb);
        const int serial_before = psb ? serial_next + __popcll(STARTS & ((1ull << slb) - 1ull)) : open_serial;
        const int serial = start ? serial_next + __popcll(psb) : serial_before;
        const int goff = start ? 0 : psb ? E - E_slb : st.pending + E;
        const int gtotal = goff + n;                                             // int32: no 4095-byte wrap
        const int gstored = complete ? min(gtotal, J.cap) : 0;
        const int aoff = nstored + wave_scan_excl(gstored, lane);
        const uint64_t COMPLETE = __ballot(complete);
        if (complete) {
            dabgpu_datagroup g = {};
            g.cif = c;
            g.offset = aoff;
            g.nbytes = gtotal;
            g.flags = gtotal > J.cap ? 128 : 0;
            groups[ngroups + __popcll(COMPLETE & below)] = g;
            segtab[serial] = aoff;
        } else if (abort) {
            segtab[serial_before] = -1;
        }
        if (lane < J.ncell) J.take[cell0 + lane] = takes ? make_int2(n | (serial << 7), goff) : make_int2(0, 0);
        if (NZ) st.state = (int)((A2 >> pk_top(NZ)) & 1);
        if (st.state == 1) {
            if (STARTS) {
                const int sl = pk_top(STARTS);
                open_serial = serial_next + __popcll(STARTS) - 1;
                st.pending = total - __shfl(E, sl);
            } else {
                st.pending += total;
            }
        } else {
            st.pending = 0;
        }
        serial_next += __popcll(STARTS);
        ngroups += __popcll(COMPLETE);
        nstored = __shfl(aoff + gstored, 63);
        if (lane == 0) {
            info->status = on ? 0 : -1;
            info->packets = (int16_t)npk;
            info->crc_errors = (int16_t)__popcll(BAD);
            info->groups = (int16_t)__popcll(COMPLETE);
            info->quality = (int16_t)quality;
            info->address = (int16_t)st.address;
        }
    }
    if (lane == 0) {
        if (st.state == 1) segtab[open_serial] = -2;     // the series in flight goes to the carry
        dabgpu_packet_run *run = J.run + e;
        run->n_groups = ngroups;
        run->n_bytes = nstored;
        run->state = st.state;
        run->pending_bytes = st.pending;
        J.state[e] = st;
    }
}

__global__ __launch_bounds__(64) void k_pkt_copy(PkJob J) {
    __shared__ uint8_t row[PK_MAX_ROW];
    const int lane = threadIdx.x;
    const int c = blockIdx.x % (J.feed.ncif + 1), e = blockIdx.x / (J.feed.ncif + 1), s = e / J.npk;
    const int32_t *segtab = J.segtab + (int64_t)e * (1 + J.feed.ncif * J.ncell);
    uint8_t *arena = J.bytes + (int64_t)e * J.arena, *carry = J.carry_out + (int64_t)e * J.cap;
    if (c == J.feed.ncif) {                                   // the bytes carried into the run
        const PkState st = J.state[e];
        const int fate = segtab[0], nn = min(st.prev_pending, J.cap);
        if (st.prev_state != 1 || fate == -1) return;
        uint8_t *dst = fate >= 0 ? arena + fate : carry;
        const uint8_t *src = J.carry_in + (int64_t)e * J.cap;
        for (int i = lane; i < nn; i += 64) dst[i] = src[i];
        return;
    }
    const int64_t cell0 = ((int64_t)e * J.feed.ncif + c) * J.ncell;
    const int2 t = lane < J.ncell ? J.take[cell0 + lane] : make_int2(0, 0);
    const int n = t.x & 0x7F, goff = t.y;
    const int fate = n ? segtab[t.x >> 7] : -1;
    const int ncopy = fate == -1 ? 0 : max(0, min(n, J.cap - goff));             // the cap keeps the first bytes
    uint64_t M = __ballot(ncopy > 0);
    if (!M) return;
    const int ncell = min((int)J.map.br[e] >> 3, J.ncell);
    pk_load_row(row, msc_row(J.feed, s, c, J.map.sub[e]), J.feed.packed, 24 * ncell, lane);
    __syncthreads();
    const int64_t dsto = fate >= 0 ? (arena - J.bytes) + fate + goff : -1 - ((carry - J.carry_out) + goff);
    const int plen = 24 * (int)(((J.rec[cell0 + min(lane, J.ncell - 1)] >> 4) & 3u) + 1);
    for (; M; M &= M - 1) {
        const int tl = __builtin_ctzll(M);
        const int64_t d = __shfl(dsto, tl);
        const int nn = __shfl(ncopy, tl), crc0 = 24 * tl + __shfl(plen, tl) - 2;
        uint8_t *dst = d >= 0 ? J.bytes + d : J.carry_out + (-1 - d);
        for (int i = lane; i < nn; i += 64) {
            const int p = 24 * tl + 3 + i;
            // its own CRC field reads complemented: check_CRC_bits has inverted it in place by then
            dst[i] = (uint8_t)(row[p] ^ ((p == crc0 || p == crc0 + 1) ? 0xFFu : 0u));
        }
    }
}

__global__ __launch_bounds__(64) void k_pkt_groups(PkJob J) {
    const int lane = threadIdx.x, e = blockIdx.x;
    const int ng = min(J.run[e].n_groups, J.gslots);
    const uint8_t *arena = J.bytes + (int64_t)e * J.arena;
    for (int g = blockIdx.y; g < ng; g += gridDim.y) {
        dabgpu_datagroup *G = J.groups + (int64_t)e * J.gslots + g;
        const int nb = G->nbytes, ns = min(nb, J.cap);
        const bool trunc = nb > J.cap;
        const uint8_t *p = arena + G->offset;
        auto B = [&](int i) -> uint32_t { return i < ns ? p[i] : 0u; };          // fields past the end read 0
        const uint32_t b0 = B(0);
        const bool ext = b0 & 0x80, crcf = b0 & 0x40, seg = b0 & 0x20, ua = b0 & 0x10;
        bool good = true;
        if (crcf) good = ns >= 2 && !trunc && wave_crc16(p, ns, lane) == crc16::CRC_GOOD;   // (wave-uniform)
        if (lane) continue;
        int next = 2 + (ext ? 2 : 0);
        uint32_t last = 0, segno = 0, tidf = 0, tid = 0, li = 0;
        if (seg) {
            last = B(next) >> 7;
            segno = ((B(next) & 0x7Fu) << 8) | B(next + 1);
            next += 2;
        }
        if (ua) {
            tidf = (B(next) >> 4) & 1u;
            li = B(next) & 0xFu;
            next += 1;
            if (tidf) tid = (B(next) << 8) | B(next + 1);
            next += li;
        }
        const bool accepted = nb > 0 && !trunc && good;
        G->flags = (uint16_t)((ext ? 1 : 0) | (crcf ? 2 : 0) | (seg ? 4 : 0) | (ua ? 8 : 0) | (last ? 16 : 0) | (tidf ? 32 : 0) |
                              (accepted ? 64 : 0) | (trunc ? 128 : 0));
        G->groupType = (uint8_t)(b0 & 0xFu);
        G->CI = (uint8_t)(B(1) >> 4);
        G->lengthInd = (uint8_t)li;
        G->segmentNumber = (uint16_t)segno;
        G->transportId = (uint16_t)tid;
        G->data_offset = next;
        G->data_nbytes = max(0, nb - next - (crcf ? 2 : 0));
    }
}

hipError_t launch_packet(hipStream_t st, const PkJob &J) {
    if (J.npk <= 0 || J.feed.nstreams <= 0 || J.feed.ncif <= 0) return hipSuccess;
    if (J.ncell <= 0 || J.ncell > PK_MAX_CELLS || J.cap <= 0 || J.gslots < J.feed.ncif * J.ncell ||
        J.arena < (int64_t)J.cap + (int64_t)J.feed.ncif * J.ncell * 127)
        return hipErrorInvalidValue;
    const int64_t ne = (int64_t)J.feed.nstreams * J.npk;
    if (ne * (J.feed.ncif + 1) > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pkt_scan, dim3((unsigned)(ne * J.feed.ncif)), dim3(64), 0, st, J);
    hipLaunchKernelGGL(k_pkt_assemble, dim3((unsigned)ne), dim3(64), 0, st, J);
    hipLaunchKernelGGL(k_pkt_copy, dim3((unsigned)(ne * (J.feed.ncif + 1))), dim3(64), 0, st, J);
    hipLaunchKernelGGL(k_pkt_groups, dim3((unsigned)ne, 32), dim3(64), 0, st, J);
    return hipGetLastError();
}

}  // namespace dab
