// TEST INFRASTRUCTURE: ensembleDecoder with auto_layout -- two synthetic ensembles that
// announce different sub-channel organisations in their FIC (figs = 1), decoded from an
// empty table: each stream's table must become what its transmitter announced, and every
// MSC callback (entries deliver from since_cif + 16) must carry the transmitter's bits.
// Prints "LAYOUTS OK" at the end; exit code 0 on success.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dabgpu_dropin.h"
#include "dabsynth.h"

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

int main() {
    try {
        // UEP short form, a DAB+ sub-channel (EEP-3A), EEP-1B | UEP-2, EEP-4A
        const std::vector<std::vector<dabsynth_subch>> tx = {
            {{0, 96, 128, 3, 1, 0, 0}, {96, 48, 64, 0103, 0, 1, 0}, {144, 54, 64, 0201, 0, 0, 0}},
            {{0, 84, 96, 2, 1, 0, 0}, {100, 16, 32, 0104, 0, 0, 0}}};
        const int S = 2, F = 3, steps = 5, NC = 4 * F * steps;
        const int maxbits[2] = {24 * 128, 24 * 96};      // the truth's row: 24 * the ensemble's largest bitRate
        std::vector<std::vector<float>> iq(S);
        std::vector<std::vector<uint8_t>> msc(S);
        std::vector<int64_t> n(S);
        for (int s = 0; s < S; s++) {
            dabsynth_cfg cfg;
            std::memset(&cfg, 0, sizeof cfg);
            cfg.n_frames = F * steps;
            cfg.pre_offset = 50000;
            cfg.snr_db = 300.0f;
            cfg.amplitude = 1.0f;
            cfg.n_subch = (int32_t)tx[s].size();
            cfg.subch = tx[s].data();
            cfg.figs = 1;
            n[s] = dabsynth_stream_len(&cfg);
            iq[s].assign(2 * n[s], 0.0f);
            msc[s].assign((size_t)NC * tx[s].size() * maxbits[s], 0);
            int64_t f0;
            CHECK(dabsynth_generate(&cfg, 900 + s, iq[s].data(), nullptr, msc[s].data(), nullptr, &f0) == 0, "synth");
        }
        dabgpu::ensembleDecoder::config ec;
        ec.n_streams = S;
        ec.n_frames = F;
        ec.max_subch = 4;
        ec.max_bitrate = 128;
        ec.max_dabplus = 1;
        ec.auto_layout = true;                          // subch stays empty: FIC first
        dabgpu::ensembleDecoder dec(ec);
        std::vector<std::vector<int64_t>> since(S);     // of the applied tables, read after each step
        std::vector<int> msc_n(S, 0), msc_bad(S, 0), early(S, 0);
        int sf_ok = 0, sf_bad = 0;
        dec.on_msc([&](int s, int64_t cif, int k, const uint8_t *bits, int nbits) {
            msc_n[s]++;
            if (k >= (int)since[s].size() || cif < since[s][k] + 16) early[s]++;
            if (k >= (int)tx[s].size() || nbits != 24 * tx[s][k].bitRate ||
                std::memcmp(bits, msc[s].data() + ((size_t)cif * tx[s].size() + k) * maxbits[s], nbits))
                msc_bad[s]++;
        });
        dec.on_superframe([&](int s, int64_t, int k, const dabgpu_superframe &info, const uint8_t *, int nb) {
            if (info.status == 3) sf_ok += (s == 0 && k == 1 && nb == 110 * 8 && (info.au_crc_ok & 0xF) == 0xF);
            else if (info.status == 2) sf_bad++;
        });
        dec.load({(const dabgpu::DSPCOMPLEX *)iq[0].data(), (const dabgpu::DSPCOMPLEX *)iq[1].data()}, {n[0], n[1]});
        for (int r = 0; r < steps; r++) {
            CHECK(dec.step(), "step %d", r);
            for (int s = 0; s < S; s++) dec.get_subch(s, &since[s]);
        }
        for (int s = 0; s < S; s++) {
            std::vector<int64_t> sc;
            const std::vector<dabgpu_subch> t = dec.get_subch(s, &sc);
            CHECK(t.size() == tx[s].size(), "stream %d: %zu entries", s, t.size());
            for (size_t k = 0; k < t.size() && k < tx[s].size(); k++) {
                const dabsynth_subch &w = tx[s][k];
                CHECK(t[k].startAddr == w.startAddr && t[k].length == w.length && t[k].bitRate == w.bitRate &&
                          t[k].protLevel == w.protLevel && t[k].uepFlag == (w.uep ? 0 : 1) &&
                          t[k].flags == (w.dabplus ? DABGPU_SUBCH_DABPLUS : 0),
                      "stream %d entry %zu: %d %d %d 0%o %d %d", s, k, t[k].startAddr, t[k].length, t[k].bitRate,
                      t[k].protLevel, t[k].uepFlag, t[k].flags);
                // applied at the end of a step, at the latest after the second whole FIG cycle
                CHECK(sc[k] % (4 * F) == 0 && sc[k] > 0 && sc[k] <= 4 * F * 3, "stream %d entry %zu since %lld", s, k,
                      (long long)sc[k]);
            }
            CHECK(dec.state(s).cif_count == NC, "stream %d cif_count %lld", s, (long long)dec.state(s).cif_count);
            // every entry delivered every CIF from since + 16 to the end, with the transmitter's bits
            int want = 0;
            for (size_t k = 0; k < sc.size(); k++) want += (int)(NC - (sc[k] + 16));
            CHECK(msc_n[s] == want && want > 0 && msc_bad[s] == 0 && early[s] == 0, "stream %d: MSC %d (want %d) bad %d early %d",
                  s, msc_n[s], want, msc_bad[s], early[s]);
            std::printf("stream %d: %zu entries, since %lld, %d MSC CIF-subchannels\n", s, t.size(),
                        sc.empty() ? -1LL : (long long)sc[0], msc_n[s]);
        }
        CHECK(sf_ok >= 1 && sf_bad == 0, "superframes ok %d bad %d", sf_ok, sf_bad);
        // a table the caps cannot hold is refused and leaves the stream's table
        bool threw = false;
        try {
            dec.set_subch(0, {{0, 96, 128, 3, 0, 0}, {96, 48, 64, 0103, 1, DABGPU_SUBCH_DABPLUS},
                              {144, 48, 64, 0103, 1, DABGPU_SUBCH_DABPLUS}});
        } catch (const dabgpu::error &) {
            threw = true;
        }
        CHECK(threw && dec.get_subch(0).size() == tx[0].size(), "caps not enforced");
    } catch (const std::exception &e) {
        std::printf("FAIL exception: %s\n", e.what());
        failures++;
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("LAYOUTS OK\n");
    return 0;
}
