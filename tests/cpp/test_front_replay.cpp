// The pipeline's front-end replay (sdr-j-dab_amd/csrc/front_replay.h: speculate a batch of
// frames, replay, commit a prefix, repeat) against ofdmProcessor::run's loop taken one frame
// at a time (ofdm-processor.cpp:344-468), on a synthetic channel defined here.  Host code
// only: the header needs no GPU.  A measurement depends only on the frame descriptor it is
// given (window, phase_a, phase_b), so a mispredicted frame measures differently when it is
// run again -- as on the device.
#include <cmath>
#include <cstdio>
#include <vector>
#include "front_replay.h"

using front::StreamSt;
using front::TU;
using front::TDATA;
using front::TNULL;

static const int TF = DABGPU_TF, NS = 2;

// ---- the channel -----------------------------------------------------------------------
// block 0 of frame k of stream s starts at T(s, k): frames T_F apart with a slow drift, which
// moves the startIndex by +-1..3 samples for one frame in seven
static int64_t T(int s, int k) {
    int64_t drift = 0;
    for (int j = 1; 7 * j <= k; j++) drift += (j % 2 ? -1 : 1) * (1 + j % 3);
    return 5000 + 1000 * s + (int64_t)k * TF + drift;
}
static int frame_at(int s, int64_t window) {             // the frame whose block 0 lies in the T_u window
    const int k = (int)((window - 5000 - 1000 * s + TU) / TF);
    for (int q = std::max(0, k - 1); q <= k + 1; q++)
        if (T(s, q) - window >= 0 && T(s, q) - window < TU) return q;
    return -1;
}
// carrier offset in Hz while frame k is on the air: kHz steps plus a remainder
static int f_true(int s, int k) {
    if (s == 1) return k < 20 ? -13000 : -13350;         // (a whole kHz first: only the coarse corrector moves)
    return k == 0 ? 36200 : k < 14 ? 7300 : k < 30 ? 7700 : 7400;
}
static const int kDropout[NS] = {-1, 9};                 // a frame whose phase reference is not found
// processBlock_0 returns 100 (no estimate) for these frames; stream 1's first estimate then comes with a
// frame whose startIndex is as predicted and moves no fine corrector: only the coarse replay cuts after it
static bool no_corr(int s, int k) { return s == 0 ? k == 3 : k < 2; }

static int32_t find_index(int s, int64_t window) {       // phaseReference::findIndex
    const int k = frame_at(s, window);
    return (k < 0 || k == kDropout[s]) ? -1 : (int32_t)(T(s, k) - window);
}
static int16_t block0_corr(int s, int64_t window, int32_t phase_a, bool f2) {   // processBlock_0
    const int k = frame_at(s, window);
    if (!f2 || k < 0) return 0;
    if (no_corr(s, k)) return 100;
    return (int16_t)lround((f_true(s, k) - phase_a) / 1000.0);
}
// FreqCorr, the sum over the guard intervals: its argument follows the remaining offset's sub-kHz part
// (whole carriers do not show in it) -- steeply, so that the fine corrector settles within a few frames
// and whole batches commit
static front::FreqCorr freq_corr(int s, int64_t window, int32_t phase_b) {
    const int k = std::max(0, frame_at(s, window));
    const int rest = f_true(s, k) - phase_b, sub = rest - 1000 * (int)lround(rest / 1000.0);
    const double a = M_PI * std::min(0.95, std::max(-0.95, sub / 100.0));
    return front::FreqCorr{(float)(1000.0 * cos(a)), (float)(1000.0 * sin(a))};
}
static int16_t snr_of(int s, int64_t window) { return (int16_t)(10 + (frame_at(s, window) + s) % 17); }
// the null search: the next frame's SyncOnPhase position, a few samples early; cut by the end of the samples
struct Acq { int64_t window; int32_t local_phase, status, attempts, no_signal; };
static Acq acquire(int s, const StreamSt &x, int64_t n_avail) {
    int k = 0;
    while (T(s, k) - 480 < x.window) k++;
    const bool cut = T(s, k) - 480 > n_avail;
    const int64_t w = cut ? n_avail : T(s, k) - 480;
    return Acq{w, front::lp_after(x.lp, w - x.window, x.coarse + x.fine), cut ? 1 : 0, x.attempts + 1, 0};
}

struct Rec { StreamSt st; dabgpu_frame_info fi; };       // a committed frame: the state after it, its record
struct Events {
    int coarse_moved = 0, coarse_reset = 0, f2_off = 0, no_corr = 0, fine_up = 0, fine_down = 0, lp_wrap_neg = 0,
        si_changed = 0, short_of_samples = 0, sync_lost = 0;
    int mid_batch_si = 0, mid_batch_samples = 0, fast_passes = 0, slow_passes = 0, spec_hits = 0,
        whole_batches = 0;                               // batch side
};

// ---- one frame at a time, as the reference's loop reads -----------------------------------
static int32_t seq_lp(int32_t lp, int64_t n, int32_t phase, Events &ev) {
    if (phase < 0 && (int64_t)lp - n * phase >= front::M) ev.lp_wrap_neg++;     // through 0, going up
    return front::lp_after(lp, n, phase);
}
static void sequential_run(int s, StreamSt &x, int F, int64_t n_avail, std::vector<Rec> &out, Events &ev) {
    for (int frames = 0; frames < F;) {
        if (!x.synced) {                                 // notSynced .. SyncOnEndNull
            const Acq r = acquire(s, x, n_avail);
            x.lp = r.local_phase; x.window = r.window; x.attempts = r.attempts; x.in_attempt = r.status != 0;
            if (r.status != 0) return;
            x.synced = true;
            x.acquisitions++;
        }
        // SyncOnPhase: T_u samples, findIndex
        if (x.window + TU > n_avail) return;
        const int32_t phase_a = x.coarse + x.fine;
        const int32_t si = find_index(s, x.window);
        if (si < 0) {                                    // goto notSynced, the window consumed
            x.lp = seq_lp(x.lp, TU, phase_a, ev);
            x.window += TU;
            x.synced = false;
            x.resyncs++;
            ev.sync_lost++;
            continue;
        }
        if (x.window + si + TU + TDATA > n_avail) { ev.short_of_samples++; return; }
        if (si != x.last_si) ev.si_changed++;
        dabgpu_frame_info fi = {x.window, si, 0, 0, 0, snr_of(s, x.window), 1};
        // OFDM_PRS: the rest of block 0, processBlock_0, the coarse corrector
        int32_t lp = seq_lp(x.lp, (int64_t)TU + si, phase_a, ev);
        const int16_t correction = block0_corr(s, x.window, phase_a, x.f2);
        if (x.f2) {
            if (correction == 0 && x.prev1 == 0 && x.prev2 == 0) { x.f2 = false; ev.f2_off++; }
            else if (correction != 100) {
                x.coarse += correction * 1000;
                if (correction) ev.coarse_moved++;
                if (std::abs(x.coarse) > 35000) { x.coarse = 0; ev.coarse_reset++; }
                x.prev2 = x.prev1;
                x.prev1 = correction;
            } else ev.no_corr++;
        }
        fi.coarse = x.coarse; fi.fine = x.fine; fi.correction = correction;
        // OFDM_SYMBOLS: 75 symbols, FreqCorr into the fine corrector, the null symbol skipped
        const front::FreqCorr fc = freq_corr(s, x.window, x.coarse + x.fine);
        lp = seq_lp(lp, TDATA, x.coarse + x.fine, ev);
        x.fine = (int16_t)(x.fine + 0.1 * atan2f(fc.y, fc.x) / M_PI * (1000 / 2));
        x.lp = seq_lp(lp, TNULL, x.coarse + x.fine, ev);
        if (x.fine > 500) { x.coarse += 1000; x.fine -= 1000; ev.fine_up++; }
        else if (x.fine < -500) { x.coarse -= 1000; x.fine += 1000; ev.fine_down++; }
        x.window += si + TU + TDATA + TNULL;
        x.last_si = si;
        x.frame_count++;
        frames++;
        out.push_back(Rec{x, fi});
    }
}

// ---- the batch side: front_replay.h driven as pipe_front_pass / dabgpu_pipe_run drive it ----
static void batch_pass(std::vector<StreamSt> &cur, std::vector<int> &done, int F, const int64_t *n_avail,
                       std::vector<Rec> *out, std::vector<int32_t> &slot, Events &ev, front::Pass &P, bool &progress,
                       bool &lost) {
    front::predict(P, cur, done, F, 2 * F + 4, (int64_t)1 << 32, n_avail);
    progress = false;
    if (!P.n()) return;
    std::vector<int> idx;
    std::vector<dabgpu_frame> sel;
    for (int i = 0; i < P.n(); i++) P.e[i].si = find_index(P.e[i].s, P.fr[i].window);
    if (P.fast) {                    // all measurements in one go, on the predicted descriptors
        ev.fast_passes++;
        for (int i = 0; i < P.n(); i++) {
            P.e[i].snr = snr_of(P.e[i].s, P.fr[i].window);
            P.e[i].fc = freq_corr(P.e[i].s, P.fr[i].window, P.fr[i].phase_b);
        }
    } else ev.slow_passes++;
    front::place(P, n_avail);
    for (int i = 0; i < P.n(); i++) {
        if (P.e[i].ok && P.e[i].cut && P.e[i].f > done[P.e[i].s]) ev.mid_batch_si++;
        // the frame after a usable, correctly predicted one, found but with symbols past the samples
        if (P.e[i].f > done[P.e[i].s] && P.e[i - 1].ok && !P.e[i - 1].cut && P.e[i].si >= 0 &&
            P.fr[i].window + P.e[i].si + TU + TDATA > n_avail[P.e[i].s])
            ev.mid_batch_samples++;
    }
    if (!P.fast) {                   // three steps: block 0 of the placed frames, then their demod
        P.usable(idx, sel);
        for (size_t k = 0; k < idx.size(); k++) {
            P.e[idx[k]].corr = block0_corr(P.e[idx[k]].s, sel[k].window, sel[k].phase_a, sel[k].flags & 1);
            P.e[idx[k]].snr = snr_of(P.e[idx[k]].s, sel[k].window);
        }
    }
    front::replay_coarse(P, cur);
    if (!P.fast) {
        P.usable(idx, sel);
        for (size_t k = 0; k < idx.size(); k++) P.e[idx[k]].fc = freq_corr(P.e[idx[k]].s, sel[k].window, sel[k].phase_b);
    }
    progress = front::commit(P, cur, done, [&](int s, int f, const dabgpu_frame &d, const dabgpu_frame_info &fi, const StreamSt &x) {
        out[s].push_back(Rec{x, fi});
        slot[(size_t)s * F + f] = d.out_slot;
    });
    if (front::sync_lost(P, cur, done)) lost = true;
    if (F > 1 && done == std::vector<int>(NS, F) && P.n() == NS * F) ev.whole_batches++;
}
static void batch_run(std::vector<StreamSt> &st, int F, const int64_t *n_avail, std::vector<Rec> *out, Events &ev) {
    std::vector<int> done(NS, 0), pred;
    std::vector<int32_t> pred_slot, slot((size_t)NS * F, -1);
    std::vector<StreamSt> cur = st;
    const bool spec = front::steady(cur);
    bool sent = false;
    int passes = 0;
    front::Pass P;
    for (int it = 0; it < 64 * F + 64; it++) {
        int found = 0;
        for (int s = 0; s < NS; s++)
            if (!cur[s].synced && done[s] < F) found += front::acq_apply(cur[s], acquire(s, cur[s], n_avail[s]));
        bool progress = false, lost = false;
        batch_pass(cur, done, F, n_avail, out, slot, ev, P, progress, lost);
        if (spec && it == 0 && found == 0 && P.n()) {    // what the speculative back end would decode
            front::predicted_whole(P, NS, F, n_avail, pred, pred_slot);
            sent = true;
        }
        if (P.n()) passes++;
        if (!progress && !lost && !found) break;
    }
    if (sent && passes == 1 && done == pred) {
        ev.spec_hits++;
        if (slot != pred_slot) { printf("FAIL: a hit whose slots differ from the prediction\n"); exit(1); }
    }
    st = cur;
}

static bool same(const StreamSt &a, const StreamSt &b) {
    return a.window == b.window && a.lp == b.lp && a.coarse == b.coarse && a.fine == b.fine && a.f2 == b.f2 &&
           a.prev1 == b.prev1 && a.prev2 == b.prev2 && a.last_si == b.last_si && a.frame_count == b.frame_count &&
           a.resyncs == b.resyncs && a.synced == b.synced && a.acquisitions == b.acquisitions && a.attempts == b.attempts;
}
static bool same(const dabgpu_frame_info &a, const dabgpu_frame_info &b) {
    return a.window == b.window && a.start_index == b.start_index && a.coarse == b.coarse && a.fine == b.fine &&
           a.correction == b.correction && a.snr == b.snr && a.committed == b.committed;
}

static int scenario(int F, Events &total) {
    std::vector<StreamSt> seq(NS), bat(NS);
    std::vector<Rec> so[NS], bo[NS];
    Events ev;
    const int runs = 52 / F + 6;
    for (int r = 0; r < runs; r++) {
        // every fourth run ends inside a frame's symbols
        int64_t n_avail[NS];
        for (int s = 0; s < NS; s++) n_avail[s] = 5000 + 1000 * s + (int64_t)(r + 1) * F * TF + (r % 4 == 2 ? -90000 : 4000);
        for (int s = 0; s < NS; s++) sequential_run(s, seq[s], F, n_avail[s], so[s], ev);
        batch_run(bat, F, n_avail, bo, ev);
        for (int s = 0; s < NS; s++) {
            if (so[s].size() != bo[s].size()) {
                printf("FAIL F=%d run %d stream %d: %zu frames one at a time, %zu in batches\n", F, r, s, so[s].size(), bo[s].size());
                return 1;
            }
            if (!same(seq[s], bat[s])) { printf("FAIL F=%d run %d stream %d: states differ after the run\n", F, r, s); return 1; }
        }
    }
    for (int s = 0; s < NS; s++) {
        if (so[s].size() < 12) { printf("FAIL F=%d stream %d: only %zu frames\n", F, s, so[s].size()); return 1; }
        for (size_t k = 0; k < so[s].size(); k++)
            if (!same(so[s][k].st, bo[s][k].st) || !same(so[s][k].fi, bo[s][k].fi)) {
                printf("FAIL F=%d stream %d frame %zu: window %lld/%lld coarse %d/%d fine %d/%d lp %d/%d\n", F, s, k,
                       (long long)so[s][k].st.window, (long long)bo[s][k].st.window, so[s][k].st.coarse, bo[s][k].st.coarse,
                       so[s][k].st.fine, bo[s][k].st.fine, so[s][k].st.lp, bo[s][k].st.lp);
                return 1;
            }
    }
    printf("F=%d: %zu + %zu frames; coarse moved %d reset %d no-corr %d f2 off %d; fine wraps +%d -%d; lp wraps %d; "
           "si changes %d (mid-batch %d); short of samples %d (mid-batch %d); sync lost %d; passes fast %d slow %d; hits %d, whole batches %d\n",
           F, so[0].size(), so[1].size(), ev.coarse_moved, ev.coarse_reset, ev.no_corr, ev.f2_off, ev.fine_up, ev.fine_down,
           ev.lp_wrap_neg, ev.si_changed, ev.mid_batch_si, ev.short_of_samples, ev.mid_batch_samples, ev.sync_lost,
           ev.fast_passes, ev.slow_passes, ev.spec_hits, ev.whole_batches);
    // the events the scenario is there for, seen by the one-frame-at-a-time side
    if (ev.coarse_moved < 2 || ev.coarse_reset != 1 || ev.f2_off != NS || ev.no_corr != 3 || ev.fine_up < 1 || ev.fine_down < 1 ||
        ev.lp_wrap_neg < 1 || ev.si_changed < 4 || ev.short_of_samples < 1 || ev.sync_lost != 1 || ev.fast_passes < 1 ||
        ev.slow_passes < 1 || ev.spec_hits < 1 || (F > 1 && (ev.whole_batches < 1 || ev.mid_batch_si < 1))) {
        printf("FAIL F=%d: an event did not occur\n", F);
        return 1;
    }
    total.mid_batch_samples += ev.mid_batch_samples;
    return 0;
}

int main() {
    Events total;
    for (int F : {1, 2, 4})
        if (scenario(F, total)) return 1;
    if (total.mid_batch_samples < 1) {
        printf("FAIL: no frame ran out of samples in the middle of a batch\n");
        return 1;
    }
    printf("FRONT REPLAY OK\n");
    return 0;
}
