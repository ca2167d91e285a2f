// PAD layer: the good AUs of DAB+ subchannels -> dynamic labels and X-PAD MSC data groups
// (dabgpu_pad_aus).  padHandler::processPAD (pad-handler.cpp), bit for bit what
// host/msc_consumers.cpp's padAssembler does; the rules where the reference is undefined are
// those of dabgpu_pad_aus (include/dabgpu.h).
//
// A padHandler is a chain: every AU sees the state the AUs before it left -- last_appType, the
// group in progress with its 8 KB buffer, the label text, dynamicLabel's five statics.  So the
// parallelism is handlers, one wave each (k_pad_walk), and inside a handler the lanes do what
// is wide: they stage the PAD (up to 255 bytes) in LDS, move a sub-field's bytes (up to 48)
// into the label text or the group buffer, take a completed group's CRC-16 over 64 slices
// joined by x^(8d) shifts (the CRC is linear: msc_feed.h's wave_crc16 over crc16_poly.h's
// arithmetic), and copy the group and the label snapshot out.
// The state, 8.4 KB, lives in LDS for the pass: a workgroup of one wave, far below the CU's
// 160 KB, so every handler of a C5-shaped call (256) is resident at once.  What is stateless in
// a PAD -- the data stream element test, count, the F-PAD fields, the CI list, each sub-field's
// type, start and length -- is a few dozen integer operations on bytes the wave has just
// staged; it is done in the walk, wave-uniform, and costs no round trip through memory.
// Every index is checked against its buffer: no AU, however hostile, makes the kernel leave
// the AU's row, the PAD, the state or the output slots and arena.  Plain vector stores only; a
// slot's state is its own, so nothing is atomic.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

__device__ __forceinline__ int pad_sublen(uint32_t ci) {                         // mapLength (:86-95)
    const int k = (int)(ci >> 5);
    return k == 0 ? 4 : k == 1 ? 6 : k == 2 ? 8 : k == 3 ? 12 : k == 4 ? 16 : k == 5 ? 24 : k == 6 ? 32 : 48;
}

__global__ __launch_bounds__(64) void k_pad_walk(PadJob J) {
    __shared__ __attribute__((aligned(16))) PadState S;
    __shared__ uint8_t pad[256];
    const int lane = threadIdx.x, slot = blockIdx.x;
    uint8_t *state = J.state + (int64_t)slot * sizeof(PadState);
    {
        const uint4 *sw = (const uint4 *)state;
        uint4 *lw = (uint4 *)&S;
        for (int i = lane; i < (int)(sizeof(PadState) / 16); i += 64) lw[i] = sw[i];
    }
    __syncthreads();
    // everything below is the same in every lane (wave-uniform) unless a lane index appears.
    // The scalars of the state are kept in registers and written back once.
    int last_app = S.last_appType, last_set = S.last_set, started = S.started, index = S.index, glen = S.length;
    int hiwater = S.hiwater, charset = S.charset, cs_set = S.cs_set, remain = S.remain, is_last = S.is_last, more = S.more;
    int tbytes = S.text_nbytes, tpieces = S.text_npieces;
    // a state from elsewhere: keep every index inside its buffer whatever it holds
    index = max(0, min(index, PAD_BUFFER - 1));
    hiwater = max(0, min(hiwater, PAD_BUFFER));
    glen = max(0, min(glen, 0x3FFF));
    tbytes = max(0, tbytes);
    tpieces = max(0, tpieces);
    remain = max(0, remain);

    dabgpu_pad_label *labels = J.labels + (int64_t)slot * J.label_slots;
    dabgpu_datagroup *groups = J.groups + (int64_t)slot * J.group_slots;
    uint8_t *arena = J.bytes + (int64_t)slot * J.arena;
    int n_labels = 0, n_groups = 0, n_bytes = 0, aus = 0, pads = 0, unhandled = 0, crc_failed = 0, guard = 0;
    int undef0 = 0, undef1 = 0, undef2 = 0, undef3 = 0;
    uint32_t touched = 0;
    int count = 0, cif = 0, aui = 0;

    auto rd = [&](int i) -> uint32_t {                                    // rule 2 (i < count always)
        if (i < 0) {
            touched |= 2u;
            return 0u;
        }
        return pad[i];
    };
    // a sub-field's byte j (0 <= j < 48) is PAD byte base - j: lanes read theirs
    auto sub = [&](int base, int j) -> uint8_t { return base - j >= 0 ? pad[base - j] : (uint8_t)0; };

    auto show = [&]() {                                                   // showLabel: a snapshot of the text
        if (n_labels < J.label_slots) {
            dabgpu_pad_label *L = labels + n_labels;
            if (lane == 0) {
                L->cif = cif;
                L->au = aui;
                L->charset = charset;
                L->nbytes = tbytes;
                L->n_pieces = tpieces;
                L->flags = (tbytes > DABGPU_PAD_LABEL_BYTES || tpieces > DABGPU_PAD_LABEL_PIECES) ? DABGPU_PAD_LABEL_TRUNCATED : 0;
            }
            L->piece_len[lane] = lane < tpieces ? S.piece_len[lane] : (uint8_t)0;
            for (int i = lane; i < DABGPU_PAD_LABEL_BYTES; i += 64) L->text[i] = i < tbytes ? S.text[i] : (uint8_t)0;
        }
        n_labels++;
    };
    // append PAD bytes base-off, base-off-1, ... (n of them, 1..48) to the text as one piece
    auto append = [&](int base, int off, int n) {
        if (!cs_set) touched |= 4u;                                       // rule 3: charSet is read
        if (tbytes + n > DABGPU_PAD_LABEL_BYTES || tpieces + 1 > DABGPU_PAD_LABEL_PIECES) touched |= 8u;   // rule 4
        if (lane < n && tbytes + lane < DABGPU_PAD_LABEL_BYTES) S.text[tbytes + lane] = sub(base, off + lane);
        if (lane == 0 && tpieces < DABGPU_PAD_LABEL_PIECES) S.piece_len[tpieces] = (uint8_t)n;
        tbytes = min(tbytes + n, 0x7FFF0000);
        tpieces = min(tpieces + 1, 0x7FFF0000);
        __syncthreads();
    };
    // dynamicLabel (:177-269) on the sub-field at base, `length` bytes
    auto dynamic_label = [&](int base, int length, uint32_t ci) {
        if ((ci & 31u) == 2u) {
            if (base - 1 < 0) touched |= 2u;
            const uint32_t prefix = (rd(base) << 8) | rd(base - 1);
            const int field_1 = (int)((prefix >> 8) & 15u);
            const bool cflag = (prefix >> 12) & 1u, first = (prefix >> 14) & 1u, last = (prefix >> 13) & 1u;
            if (first) {
                charset = (int)((prefix >> 4) & 15u);
                cs_set = 1;
                tbytes = tpieces = 0;
            }
            if (cflag) {                                                  // the clear command: moreXPad stays as it was
                tbytes = tpieces = 0;
                return;
            }
            const int total = field_1 + 1;
            int dl;
            if (length - 2 < total) {
                dl = length - 2;
                more = 1;
            } else {
                dl = total;
                more = 0;
            }
            append(base, 2, dl);
            if (last) {
                if (!more)
                    show();
                else
                    is_last = 1;
            } else {
                is_last = 0;
            }
            remain = total - dl;
        } else if ((ci & 31u) == 3u && more) {
            int dl;
            if (remain > length) {
                dl = length;
                remain -= length;
            } else {
                dl = remain;
                more = 0;
            }
            if (dl > 0) append(base, 0, min(dl, 48));                     // (dl >= 1 in every state the walk itself leaves)
            if (!more && is_last) show();
        }
    };
    // build_MSC_segment (:299-357) on the buffer's first `length` bytes (length <= 8191 here)
    auto build = [&](int length) {
        auto H = [&](int i) -> uint32_t {                                 // rule 3: a byte nothing ever wrote (it reads 0)
            if (i >= hiwater) touched |= 4u;
            return S.buffer[min(i, PAD_BUFFER - 1)];
        };
        const uint32_t b0 = H(0);
        H(1);
        const bool ext = b0 & 0x80u, crcf = b0 & 0x40u, seg = b0 & 0x20u, ua = b0 & 0x10u;
        bool good = true;
        if (crcf) {
            if (length < 2) {                                             // rule 3
                touched |= 4u;
                good = false;
            } else {
                // pad_crc complements the last two bytes and compares with the register from all ones
                good = wave_crc16(S.buffer, length, lane) == crc16::CRC_GOOD;
            }
            if (!good) crc_failed++;
        }
        int idx = ext ? 4 : 2;
        uint32_t last = 0, segno = 0xFFFFu, tid = 0xFFFFu, tidf = 1, li = 0;
        if (seg) {
            last = H(idx) >> 7;
            segno = ((H(idx) & 0x7Fu) << 8) | H(idx + 1);
            idx += 2;
        }
        if (ua) {
            li = H(idx) & 15u;
            if (H(idx) & 0x10u) {
                tid = (H(idx + 1) << 8) | H(idx + 2);
                idx += 3 + (int)li - 2;
            } else {
                tidf = 0;                                                 // "sorry no transportId"
            }
        }
        const uint32_t gtype = b0 & 15u;
        bool accepted = good && (gtype == 3u || gtype == 4u) && tidf;
        const bool trunc = (int64_t)n_bytes + length > J.arena;
        if (trunc) accepted = false;
        if (n_groups < J.group_slots) {
            if (lane == 0) {
                dabgpu_datagroup G = {};
                G.cif = cif;
                G.offset = n_bytes;
                G.nbytes = length;
                G.data_offset = idx;
                G.data_nbytes = max(0, length - idx - (crcf ? 2 : 0));
                G.flags = (uint16_t)((ext ? 1 : 0) | (crcf ? 2 : 0) | (seg ? 4 : 0) | (ua ? 8 : 0) | (last ? 16 : 0) | (tidf ? 32 : 0) |
                                     (accepted ? 64 : 0) | (trunc ? 128 : 0));
                G.segmentNumber = (uint16_t)segno;
                G.transportId = (uint16_t)tid;
                G.groupType = (uint8_t)gtype;
                G.CI = 0;                                                 // (b[1] & 0xF) >> 4
                G.lengthInd = (uint8_t)li;
                G.reserved[0] = (uint8_t)aui;
                groups[n_groups] = G;
            }
        }
        if (!trunc) {
            if (n_groups < J.group_slots)
                for (int i = lane; i < length; i += 64) arena[n_bytes + i] = S.buffer[i];
            n_bytes += length;
        }
        n_groups++;
    };
    // add_MSC_element (:274-297) with the sub-field at base
    auto add_msc = [&](int base, int length) {
        if (!started) {                                                   // rule 3: no length indicator yet
            touched |= 4u;
            return;
        }
        if (index + length >= PAD_BUFFER) {
            guard++;
            return;
        }
        if (lane < length) S.buffer[index + lane] = sub(base, lane);
        index += length;
        hiwater = max(hiwater, index);
        __syncthreads();
        if (index < glen) return;
        build(glen);
        index = 0;
        __syncthreads();
    };

    // one good AU as mp4Processor hands it on (mp4processor.cpp:255-265): lim readable bytes at au,
    // the rest of theAU reads 0
    auto process_au = [&](const uint8_t *au, int lim, int au_cif, int au_no) {
        aus++;
        auto B = [&](int i) -> uint32_t { return i < lim ? au[i] : 0u; };
        if (((B(0) >> 5) & 7u) != 4u) return;                             // (mp4processor.cpp:264)
        pads++;
        count = (int)B(1);
        cif = au_cif;
        aui = au_no;
        __syncthreads();                                                  // the last PAD's reads, before it is replaced
        for (int i = lane; i < 256; i += 64) pad[i] = i < count ? (uint8_t)B(2 + i) : (uint8_t)0;
        __syncthreads();
        touched = 0;
        do {                                                              // processPAD (:47-71)
            if (count < 2) {                                              // rule 1
                touched |= 1u;
                break;
            }
            const uint32_t fp = pad[count - 2];
            if (((fp >> 6) & 3u) != 0u) break;                            // only F-PAD type 0
            const uint32_t x_ind = (fp >> 4) & 3u;
            if (x_ind == 1u) {                                            // handle_shortPAD (:73-82)
                const uint32_t ci = rd(count - 3);
                if (count - 6 < 0) touched |= 2u;
                if ((ci & 31u) == 2u || (ci & 31u) == 3u) dynamic_label(count - 4, 3, ci);
                break;
            }
            if (x_ind != 2u || !((pad[count - 1] >> 1) & 1u)) break;      // handle_variablePAD (:97-173); CI flag 0
            int base = count - 3, n_ci = 0;
            uint32_t table[4];
            while ((rd(base) & 31u) != 0u && n_ci < 4) table[n_ci++] = rd(base--);
            if (n_ci < 4) base -= 1;
            for (int i = 0; i < n_ci; i++) {
                const uint32_t ci = table[i], app = ci & 31u;
                const int length = pad_sublen(ci);
                if (app == 1u) {
                    if (base - 3 < 0) touched |= 2u;                      // (with the crc the reference reads and drops)
                    glen = (int)(((rd(base) & 63u) << 8) | rd(base - 1));
                    index = 0;
                    started = 1;
                    base -= 4;
                    last_app = 1;
                    last_set = 1;
                    continue;
                }
                if (app != 2u && app != 3u && app != 12u && app != 13u) {
                    last_app = (int)app;
                    last_set = 1;
                    unhandled++;
                    break;
                }
                if (base - (length - 1) < 0) touched |= 2u;               // the reference copies the whole sub-field
                if (app == 2u || app == 3u) {
                    dynamic_label(base, length, ci);
                } else {
                    if (!last_set) touched |= 4u;                         // rule 3: last_appType is read
                    if ((app == 12u && last_app == 1) || (app == 13u && (last_app == 12 || last_app == 13))) add_msc(base, length);
                }
                last_app = (int)app;
                last_set = 1;
                base -= length;
                if (base < 0 && i < n_ci - 1) break;
            }
        } while (false);
        undef0 += touched & 1u;
        undef1 += (touched >> 1) & 1u;
        undef2 += (touched >> 2) & 1u;
        undef3 += (touched >> 3) & 1u;
    };
    int rejected = 0;
    if (!J.info) {                                                        // the operator: rows of AUs
        const int64_t row_bytes = max(J.au_stride, (int64_t)0);
        for (int a = 0; a < J.n_aus; a++) {
            const int64_t e = (int64_t)slot * J.n_aus + a;
            const int len = J.len[e];
            if (len < 0) continue;
            process_au(J.aus + e * row_bytes, (int)min((int64_t)len, row_bytes), J.cif ? J.cif[e] : a, a);
        }
    } else if (J.src[slot] >= 0) {
        // the pipeline: the AUs of the run's status-3 superframes of DAB+ slot src, in CIF and AU
        // order, straight from dabgpu_pipe_dabplus's outputs (sparse or compact)
        const int e = J.src[slot], s = e / J.ndp, d = e % J.ndp;
        for (int c = 0; c < J.ncif; c++) {
            const int64_t r = ((int64_t)s * J.ncif + c) * J.ndp + d;
            const dabgpu_superframe I = J.info[r];
            if (I.status == 2) rejected++;
            if (I.status != 3) continue;
            const uint8_t *sf;
            if (J.kmax) {
                if (I.reserved >= J.kmax) continue;                       // (0xFF: no bytes)
                sf = J.sf + (((int64_t)s * J.ndp + d) * J.kmax + I.reserved) * J.sf_stride;
            } else {
                sf = J.sf + r * J.sf_stride;
            }
            const int na = max(0, min((int)I.num_aus, 6));
            for (int a = 0; a < na; a++) {
                const int a0 = I.au_start[a], len = I.au_start[a + 1] - a0 - 2;
                if (!((I.au_crc_ok >> a) & 1) || len < 0 || a0 < 0 || a0 >= J.sf_stride) continue;
                process_au(sf + a0, min(len, J.sf_stride - a0), c, a);
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        S.last_appType = last_app;
        S.last_set = last_set;
        S.started = started;
        S.index = index;
        S.length = glen;
        S.hiwater = hiwater;
        S.charset = charset;
        S.cs_set = cs_set;
        S.remain = remain;
        S.is_last = is_last;
        S.more = more;
        S.text_nbytes = tbytes;
        S.text_npieces = tpieces;
        dabgpu_pad_run R = {};
        R.n_labels = n_labels;
        R.n_groups = n_groups;
        R.n_bytes = n_bytes;
        R.aus = aus;
        R.pads = pads;
        R.unhandled = unhandled;
        R.undefined[0] = undef0;
        R.undefined[1] = undef1;
        R.undefined[2] = undef2;
        R.undefined[3] = undef3;
        R.crc_failed = crc_failed;
        R.guard_dropped = guard;
        R.rejected_sf = rejected;
        J.run[slot] = R;
    }
    __syncthreads();
    {
        uint4 *sw = (uint4 *)state;
        const uint4 *lw = (const uint4 *)&S;
        for (int i = lane; i < (int)(sizeof(PadState) / 16); i += 64) sw[i] = lw[i];
    }
}

hipError_t launch_pad(hipStream_t st, const PadJob &J) {
    if (J.n_slots <= 0) return hipSuccess;
    if (J.info && (!J.src || !J.sf || J.ndp <= 0 || J.ncif < 0 || J.sf_stride < 0 || J.kmax < 0)) return hipErrorInvalidValue;
    if (J.n_aus < 0 || J.au_stride < 0 || J.label_slots < 0 || J.group_slots < 0 || J.arena < 0 || J.arena > 0x7FFFFFFF ||
        ((uintptr_t)J.state & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pad_walk, dim3((unsigned)J.n_slots), dim3(64), 0, st, J);
    return hipGetLastError();
}

}  // namespace dab
