// ensemble_util.h -- the pure pieces of ensembleDecoder (ensemble_decoder.cpp): no GPU call, no
// HIP, only dabgpu.h's types and the standard library, so tests/cpp/test_ensemble_util.cpp builds
// from this header alone.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dabgpu.h"

namespace dabgpu {

// The one slot rule of the pipeline's layers, as csrc/layer_slots.h states it for the library:
// slot j of a stream is its j-th table entry whose flags hold every bit of mask.  Returns the
// table indices of those entries in order, at most max of them (a layer's slot count).
inline std::vector<int> entries_flagged(const std::vector<dabgpu_subch> &table, int mask, int max) {
    std::vector<int> v;
    for (int k = 0; k < (int)table.size() && (int)v.size() < max; k++)
        if ((table[k].flags & mask) == mask) v.push_back(k);
    return v;
}

inline int count_flagged(const std::vector<dabgpu_subch> &table, int mask) {
    int n = 0;
    for (const dabgpu_subch &e : table) n += (e.flags & mask) == mask;
    return n;
}

// the first nbits bits of a packed row (MSB first), one per byte
inline void unpack_bits(const uint8_t *packed, int nbits, uint8_t *out) {
    for (int i = 0; i < nbits; i++) out[i] = (uint8_t)((packed[i >> 3] >> (7 - (i & 7))) & 1);
}

// The DABGPU_SUBCH_* bits auto_layout asks the FIC for (dabgpu_pipe_fic's want_flags; the host parse hands
// them to fib_processor::subchannels): a layer's bit, when one of its callbacks is set and it holds slots.
struct layers_wanted {
    bool on_pcm, on_audio, on_datagroup, on_mot_object, on_datagram, on_pad;   // on_pad: one of the three PAD callbacks
    int n_mp2, n_audio, n_packet, n_mot, n_pad;                                // the layers' slot counts
};
inline int wanted_flags(const layers_wanted &w) {
    return ((w.on_pcm || (w.on_audio && w.n_audio > 0)) && w.n_mp2 > 0 ? DABGPU_SUBCH_MP2 : 0) |
           (w.on_datagroup && w.n_packet > 0 ? DABGPU_SUBCH_PACKET : 0) | (w.on_mot_object && w.n_mot > 0 ? DABGPU_SUBCH_MOT : 0) |
           (w.on_datagram && w.n_packet > 0 ? DABGPU_SUBCH_IP : 0) | (w.on_pad && w.n_pad > 0 ? DABGPU_SUBCH_PAD : 0);
}

// the data chunk of an .sdr recording: what wavFiles accepts (wavfiles.cpp:56-69 via
// libsndfile: 2 channels, 2048000 Hz, 16-bit PCM; WAVE_FORMAT_EXTENSIBLE with the PCM
// subformat too).  Returns the payload's byte offset and size; throws Error(DABGPU_E_ARG, text).
template <class Error>
std::pair<int64_t, int64_t> sdr_payload(std::FILE *f, const std::string &path) {
    auto u32 = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
    auto u16 = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8; };
    uint8_t h[12];
    if (std::fread(h, 1, 12, f) != 12 || std::memcmp(h, "RIFF", 4) || std::memcmp(h + 8, "WAVE", 4))
        throw Error(DABGPU_E_ARG, path + ": not a RIFF/WAVE file");
    int64_t off = 12;
    bool fmt_ok = false, have_fmt = false;
    for (;;) {
        uint8_t ck[8];
        if (std::fread(ck, 1, 8, f) != 8) throw Error(DABGPU_E_ARG, path + ": no data chunk");
        const int64_t n = u32(ck + 4);
        off += 8;
        if (!std::memcmp(ck, "fmt ", 4)) {
            std::vector<uint8_t> b((size_t)n);
            if (n < 16 || std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) throw Error(DABGPU_E_ARG, path + ": bad fmt chunk");
            uint32_t tag = u16(&b[0]);
            if (tag == 0xFFFE && n >= 26) tag = u16(&b[24]);       // WAVE_FORMAT_EXTENSIBLE: the subformat
            fmt_ok = tag == 1 && u16(&b[2]) == 2 && u32(&b[4]) == 2048000 && u16(&b[14]) == 16;
            have_fmt = true;
            if (n & 1) std::fseek(f, 1, SEEK_CUR);
        } else if (!std::memcmp(ck, "data", 4)) {
            if (!have_fmt || !fmt_ok)
                throw Error(DABGPU_E_ARG, path + ": not a recorded DAB file (need PCM16, 2 channels, 2048000 Hz)");
            return {off, n};
        } else {
            std::fseek(f, (long)(n + (n & 1)), SEEK_CUR);
        }
        off += n + (n & 1);
    }
}

}  // namespace dabgpu
