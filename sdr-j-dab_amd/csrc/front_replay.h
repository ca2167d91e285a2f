// front_replay.h -- the receiver's sequential logic (ofdmProcessor::run per frame,
// ofdm-processor.cpp:344-468) as the pipeline's front end runs it: predict a batch of frames
// per stream, measure them, replay the reference's per-frame updates on the measured values,
// commit the longest correctly predicted prefix.  No HIP here: include/dabgpu.h and the standard
// library only (tests/cpp/test_front_replay.cpp checks batch == one frame at a time on the CPU).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../include/dabgpu.h"

namespace front {

constexpr int M = 2048000;                         // INPUT_RATE: the oscillator table's length
constexpr int TU = DABGPU_TU, TS = DABGPU_TS, TNULL = DABGPU_TNULL, NSYM = DABGPU_L - 1;
constexpr int64_t TDATA = (int64_t)NSYM * TS;      // symbols 1..75

struct StreamSt {
    int64_t window = 0;      // next SyncOnPhase position
    int32_t lp = 0;          // localPhase before `window`
    int32_t coarse = 0;
    int16_t fine = 0;
    bool f2 = true;
    int16_t prev1 = 1000, prev2 = 999;
    bool synced = false;
    int64_t cif_count = 0;
    int64_t frame_count = 0;
    int32_t last_si = 504;
    int32_t resyncs = 0;
    int32_t attempts = 0;        // ofdmProcessor::run's `attempts` (ofdm-processor.cpp:274-314)
    bool in_attempt = false;     // a null search cut by the end of the samples: `attempts` counts it
    int32_t no_signal = 0;       // No_Signal_Found emissions (scan mode)
    int32_t frames_run = 0;      // frames committed by the last dabgpu_pipe_run
    int32_t acquisitions = 0;    // null-symbol searches completed
};

inline int32_t modM(int64_t x) {
    int64_t r = x % M;
    return (int32_t)(r < 0 ? r + M : r);
}
// advance localPhase over n samples read with `phase` (getSamples, ofdm-processor.cpp:217-219)
inline int32_t lp_after(int32_t lp, int64_t n, int32_t phase) { return modM((int64_t)lp - n * (int64_t)phase); }

// processBlock_0's correction into the coarse corrector (ofdm-processor.cpp:395-406); the
// prediction runs it with the correction 0 a settled stream reports
inline void coarse_step(StreamSt &x, int16_t corr) {
    if (!x.f2) return;
    if (corr == 0 && x.prev1 == 0 && x.prev2 == 0) x.f2 = false;
    else if (corr != 100) {
        x.coarse += corr * 1000;
        if (std::abs(x.coarse) > 35000) x.coarse = 0;
        x.prev2 = x.prev1;
        x.prev1 = corr;
    }
}

// a null search's outcome (AcqResult) into the stream state; 1 if it found the end of a null symbol
template <class Result>
inline int acq_apply(StreamSt &x, const Result &r) {
    x.lp = r.local_phase;
    x.window = r.window;
    x.attempts = r.attempts;
    x.in_attempt = r.status != 0;
    x.no_signal += r.no_signal;
    if (r.status != 0) return 0;
    x.synced = true;
    x.acquisitions++;
    return 1;
}

struct FreqCorr { float x, y; };                   // a frame's FreqCorr sum (float2's layout)

// One pass: the pending frames of every stream, stream by stream in frame order, as predicted
// (fr: the descriptors the device reads), and what the device measured of each
struct Entry {
    int s, f;                                      // stream, frame
    int32_t si;                                    // startIndex measured (predicted: block0 - window)
    int16_t corr, snr;                             // processBlock_0's correction, get_snr
    FreqCorr fc;
    bool ok, cut;                                  // usable; the frames after this one are not
};
struct Pass {
    std::vector<dabgpu_frame> fr;
    std::vector<Entry> e;                          // the caller fills si, then corr / snr, then fc
    bool general = false;                          // some frame has a nonzero NCO phase step
    bool fast = true;                              // no frame runs the coarse AFC (f2 off everywhere)
    int n() const { return (int)fr.size(); }
    // the frames still usable, for the next measurement
    void usable(std::vector<int> &idx, std::vector<dabgpu_frame> &sel) const {
        idx.clear(), sel.clear();
        for (int i = 0; i < n(); i++)
            if (e[i].ok) { idx.push_back(i); sel.push_back(fr[i]); }
    }
};

// Predict frames done[s] .. F-1 of every synchronised stream: startIndex = the last one,
// correction 0, fine corrector unchanged, the null symbol skipped.
inline void predict(Pass &P, const std::vector<StreamSt> &cur, const std::vector<int> &done, int F, int R,
                    int64_t stride, const int64_t *n_avail) {
    P = Pass();
    for (int s = 0; s < (int)cur.size(); s++) {
        if (done[s] >= F || !cur[s].synced) continue;
        StreamSt x = cur[s];
        for (int f = done[s]; f < F; f++) {
            dabgpu_frame d = {};
            const int32_t si = x.last_si;
            d.iq_base = stride * s;
            d.n_samples = n_avail[s];
            d.window = x.window;
            d.block0 = x.window + si;
            d.lp_window = x.lp;
            d.phase_a = x.coarse + x.fine;
            // the reference reads the T_u window first (ofdm-processor.cpp:344-352); whether
            // the rest of the frame is there is known once startIndex is (place)
            if (d.window + TU > n_avail[s]) break;
            d.flags = x.f2 ? 1 : 0;
            coarse_step(x, 0);
            d.lp_data = lp_after(x.lp, (int64_t)TU + si, d.phase_a);
            d.phase_b = x.coarse + x.fine;
            d.out_slot = (int32_t)((int64_t)s * R + (x.frame_count + (f - done[s])) % R);
            P.fr.push_back(d);
            P.e.push_back(Entry{s, f, 0, 0, 0, FreqCorr{0.0f, 0.0f}, false, false});
            if (d.phase_a || d.phase_b) P.general = true;
            if (d.flags & 1) P.fast = false;
            x.lp = lp_after(lp_after(d.lp_data, TDATA, d.phase_b), TNULL, d.phase_b);
            x.window = d.block0 + TU + TDATA + TNULL;
        }
    }
}

// every stream synchronised with its coarse AFC off: the first pass of a run then commits
// exactly the frames it predicts, unless a measurement says otherwise
inline bool steady(const std::vector<StreamSt> &cur) {
    for (const StreamSt &x : cur)
        if (!x.synced || x.f2) return false;
    return true;
}
// The frames a run's first prediction (done = 0) has all the samples of: pred[s] of them for
// stream s, in ring slots pred_slot[s * F + f] (-1 beyond) -- what the speculative back end decodes.
inline void predicted_whole(const Pass &P, int S, int F, const int64_t *n_avail, std::vector<int> &pred,
                            std::vector<int32_t> &pred_slot) {
    pred.assign(S, 0);
    pred_slot.assign((size_t)S * F, -1);
    for (int i = 0; i < P.n(); i++) {
        const int s = P.e[i].s, f = P.e[i].f;
        if (f != pred[s] || P.fr[i].block0 + TU + TDATA > n_avail[s]) continue;
        pred_slot[(size_t)s * F + f] = P.fr[i].out_slot;
        pred[s] = f + 1;
    }
}

// Windows (si measured).  A frame is usable if every earlier frame of its stream had the
// predicted startIndex; its own startIndex fixes block0.
inline void place(Pass &P, const int64_t *n_avail) {
    int prev_s = -1;
    bool valid = true;
    for (int i = 0; i < P.n(); i++) {
        if (P.e[i].s != prev_s) { prev_s = P.e[i].s; valid = true; }
        if (!valid) continue;
        // sync lost (ofdm-processor.cpp:354-357), or symbols 1..75 not all there yet: wait for samples
        if (P.e[i].si < 0 || P.fr[i].window + P.e[i].si + TU + TDATA > n_avail[P.e[i].s]) { valid = false; continue; }
        // (the null symbol after the frame is skipped when the next frame is read,
        // as the reference's getSamples(T_null) does, ofdm-processor.cpp:449-453)
        P.e[i].ok = 1;
        if (P.e[i].si != P.fr[i].block0 - P.fr[i].window) { P.e[i].cut = 1; valid = false; }
        P.fr[i].block0 = P.fr[i].window + P.e[i].si;
        P.fr[i].lp_data = lp_after(P.fr[i].lp_window, (int64_t)TU + P.e[i].si, P.fr[i].phase_a);
    }
}

// The coarse corrector over the usable frames (corr measured): phase_b of a frame uses its
// own correction; later frames are cut if the corrector moved (the prediction assumed 0).
inline void replay_coarse(Pass &P, const std::vector<StreamSt> &cur) {
    int prev_s = -1;
    StreamSt x;
    bool valid = true;
    for (int i = 0; i < P.n(); i++) {
        if (!P.e[i].ok) continue;
        if (P.e[i].s != prev_s) { prev_s = P.e[i].s; x = cur[P.e[i].s]; valid = true; }
        if (!valid) { P.e[i].ok = 0; continue; }
        const int32_t coarse0 = x.coarse;
        coarse_step(x, P.e[i].corr);
        P.fr[i].phase_b = x.coarse + x.fine;
        if (P.fr[i].phase_b) P.general = true;
        if (P.e[i].corr != 0 || x.coarse != coarse0) P.e[i].cut = 1;
        if (P.e[i].cut) valid = false;
    }
}

// Commit (fc measured): the full per-frame state update (ofdm-processor.cpp:395-468) of each
// stream's usable frames up to the first whose correctors moved.  sink(s, frame, descriptor,
// record, state after the frame) takes every committed frame; true if any was.
template <class Sink>
inline bool commit(const Pass &P, std::vector<StreamSt> &cur, std::vector<int> &done, Sink &&sink) {
    int prev_s = -1;
    bool valid = true, progress = false;
    for (int i = 0; i < P.n(); i++) {
        if (!P.e[i].ok) continue;
        const int s = P.e[i].s;
        if (s != prev_s) { prev_s = s; valid = true; }
        if (!valid) continue;
        StreamSt &x = cur[s];
        const dabgpu_frame &d = P.fr[i];
        coarse_step(x, P.e[i].corr);
        const int16_t fine0 = x.fine;
        const int32_t coarse0 = x.coarse;
        // fineCorrector += 0.1 * arg(FreqCorr) / M_PI * (carrierDiff / 2)
        const float a = atan2f(P.e[i].fc.y, P.e[i].fc.x);
        x.fine = (int16_t)(x.fine + 0.1 * a / M_PI * (1000 / 2));
        x.lp = lp_after(lp_after(d.lp_data, TDATA, d.phase_b), TNULL, x.coarse + x.fine);
        if (x.fine > 500) { x.coarse += 1000; x.fine -= 1000; }
        else if (x.fine < -500) { x.coarse -= 1000; x.fine += 1000; }
        x.window = d.block0 + TU + TDATA + TNULL;
        x.last_si = (int32_t)(d.block0 - d.window);
        const dabgpu_frame_info fi = {d.window, x.last_si, coarse0, fine0, P.e[i].corr, P.e[i].snr, 1};
        x.frame_count++;
        sink(s, done[s]++, d, fi, (const StreamSt &)x);
        progress = true;
        if (x.fine != fine0 || x.coarse != coarse0 || P.e[i].cut) valid = false;
    }
    return progress;
}

// Sync loss: the first uncommitted frame's window was read exactly as the reference would
// and findIndex failed -> goto notSynced past the window (ofdm-processor.cpp:354-357)
inline bool sync_lost(const Pass &P, std::vector<StreamSt> &cur, const std::vector<int> &done) {
    bool lost = false;
    for (int i = 0; i < P.n(); i++) {
        const int s = P.e[i].s;
        StreamSt &x = cur[s];
        if (P.e[i].f == done[s] && P.e[i].si < 0 && P.fr[i].window == x.window && P.fr[i].lp_window == x.lp &&
            P.fr[i].phase_a == x.coarse + x.fine) {
            x.synced = false;
            x.lp = lp_after(x.lp, TU, x.coarse + x.fine);
            x.window += TU;
            x.resyncs++;
            lost = true;
        }
    }
    return lost;
}

}  // namespace front
