// TEST INFRASTRUCTURE: fib_processor::subchannels() on the FIBs of the synthetic
// transmitter (figs = 1): the FIG 0/1 sub-channel organisation as the table
// dabgpu_pipe_set_subch takes, with the DAB+ flag from FIG 0/2's ASCTy 63.  Host code only.
// Prints "FIB SUBCHANNELS OK"; exit code 0 on success.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dabsynth.h"
#include "fib_processor.h"

using namespace dabgpu;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            failures++;                                    \
        }                                                  \
    } while (0)

static bool equal(const std::vector<fib_subch> &a, const std::vector<fib_subch> &b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(fib_subch)));
}

int main() {
    // UEP short form (two table rows), EEP long form A and B, DAB+ on EEP-3A and on UEP
    const std::vector<dabsynth_subch> tx = {{0, 96, 128, 3, 1, 0, 0},    {96, 48, 64, 0103, 0, 1, 0},
                                            {144, 54, 64, 0201, 0, 0, 0}, {200, 16, 32, 0104, 0, 0, 0},
                                            {224, 84, 96, 2, 1, 0, 0},    {400, 24, 32, 0103, 0, 2, 0},
                                            {500, 18, 32, 0203, 0, 0, 0}};
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
    CHECK(dabsynth_generate(&cfg, 7, iq.data(), fic.data(), nullptr, nullptr, &f0) == 0, "synth");
    fib_processor fp;
    CHECK(fp.subchannels().empty(), "a new parser has sub-channels");
    // the FIGs cycle one item per FIB (dabsynth.cpp make_fig_fib): 1 + 2 items per sub-channel
    const int cycle = 1 + 2 * (int)tx.size();
    std::vector<fib_subch> at_second;
    int nfib = 0;
    for (int f = 0; f < NF; f++)
        for (int b = 0; b < 12; b++) {
            fp.process_FIB(fic.data() + ((size_t)f * 12 + b) * 256, (uint16_t)(b / 3));
            nfib++;
            std::vector<int> ids;
            const std::vector<fib_subch> t = fp.subchannels(&ids);
            if (nfib == 2 * cycle) at_second = t;
            if (nfib >= 2 * cycle) CHECK(equal(t, at_second), "the set changed at FIB %d", nfib);   // stable from the second cycle
            for (size_t k = 1; k < ids.size(); k++) CHECK(ids[k] > ids[k - 1], "SubChId order at FIB %d", nfib);
            if (nfib >= 2 * cycle)
                for (size_t k = 0; k < ids.size(); k++) CHECK(ids[k] == (int)k, "FIB %d entry %zu id %d", nfib, k, ids[k]);
        }
    CHECK(nfib >= 3 * cycle, "too few FIBs");
    const std::vector<fib_subch> t = fp.subchannels();
    CHECK(t.size() == tx.size(), "%zu sub-channels", t.size());
    for (size_t k = 0; k < t.size() && k < tx.size(); k++) {
        const dabsynth_subch &w = tx[k];
        CHECK(t[k].startAddr == w.startAddr && t[k].length == w.length && t[k].bitRate == w.bitRate &&
                  t[k].protLevel == w.protLevel && t[k].uepFlag == (w.uep ? 0 : 1) && t[k].flags == (w.dabplus ? 1 : 0),
              "entry %zu: %d %d %d 0%o %d %d", k, t[k].startAddr, t[k].length, t[k].bitRate, t[k].protLevel, t[k].uepFlag,
              t[k].flags);
    }
    fp.clearEnsemble();
    CHECK(fp.subchannels().empty(), "clearEnsemble keeps sub-channels");
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("FIB SUBCHANNELS OK\n");
    return 0;
}
