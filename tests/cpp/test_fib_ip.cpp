// TEST INFRASTRUCTURE: fib_processor::subchannels(ids, classic_audio, packet_data, mot, pad, ip) on
// the FIBs of the synthetic transmitter (figs = 1) with a DSCTy 59 (DABSYNTH_IP), a DSCTy 60
// (DABSYNTH_MOT) and an audio sub-channel: the DSCTy 59 one is flagged 8 | 64 with ip, with
// packet_data or without it, 8 with packet_data alone and nothing without either; the DSCTy 60
// one never gets 64; the five-argument call is what it was.  Host code only.  Prints "FIB IP OK".
#include <cstdio>
#include <cstring>
#include <vector>

#include "dabsynth.h"
#include "fib_processor.h"

using namespace dabgpu;

int main() {
    const std::vector<dabsynth_subch> tx = {{0, 96, 128, 3, 1, 0, DABSYNTH_MP2}, {96, 48, 64, 0103, 0, 0, DABSYNTH_IP},
                                            {144, 24, 32, 0103, 0, 0, DABSYNTH_MOT}, {200, 48, 64, 0103, 0, 1, 0}};
    dabsynth_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    const int NF = 8;
    cfg.n_frames = NF;
    cfg.pre_offset = 50000;
    cfg.snr_db = 300.0f;
    cfg.amplitude = 1.0f;
    cfg.n_subch = (int32_t)tx.size();
    cfg.subch = tx.data();
    cfg.figs = 1;
    std::vector<float> iq(2 * dabsynth_stream_len(&cfg));
    std::vector<uint8_t> fic((size_t)NF * 4 * 768);
    int64_t f0;
    if (dabsynth_generate(&cfg, 7, iq.data(), fic.data(), nullptr, nullptr, &f0) != 0) return 2;
    fib_processor fp;
    for (int f = 0; f < NF; f++)
        for (int b = 0; b < 12; b++) fp.process_FIB(fic.data() + ((size_t)f * 12 + b) * 256, (uint16_t)(b / 3));
    int failures = 0;
    // mode bit 0: packet_data, bit 1: mot, bit 2: ip
    const int want[8][4] = {{0, 0, 0, 1},  {0, 8, 8, 1},  {0, 0, 24, 1},  {0, 8, 24, 1},
                            {0, 72, 0, 1}, {0, 72, 8, 1}, {0, 72, 24, 1}, {0, 72, 24, 1}};
    for (int m = 0; m < 8; m++) {
        const std::vector<fib_subch> t = fp.subchannels(nullptr, false, m & 1, m & 2, false, m & 4);
        if (t.size() != tx.size()) {
            std::printf("FAIL %zu sub-channels\n", t.size());
            return 1;
        }
        for (size_t k = 0; k < t.size(); k++)
            if (t[k].flags != want[m][k] || t[k].startAddr != tx[k].startAddr || t[k].bitRate != tx[k].bitRate) {
                std::printf("FAIL mode %d entry %zu: flags %d, want %d\n", m, k, t[k].flags, want[m][k]);
                failures++;
            }
        if (!(m & 4)) {                                      // without ip: the call existing callers make
            const std::vector<fib_subch> u = fp.subchannels(nullptr, false, m & 1, m & 2, false);
            for (size_t k = 0; k < t.size(); k++)
                if (u[k].flags != t[k].flags) failures++;
        }
    }
    if (failures) return 1;
    std::printf("FIB IP OK\n");
    return 0;
}
