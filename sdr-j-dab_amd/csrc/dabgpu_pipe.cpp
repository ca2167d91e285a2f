// dabgpu_pipe.cpp -- the C ABI (include/dabgpu.h), second half: the streaming pipeline that replaces
// ofdmProcessor::run + ficHandler + mscHandler for many ensembles at once (its receiver logic:
// front_replay.h; its state: dabgpu_pipe.h; the layers behind its outputs: dabgpu_layers.cpp)
#include <cstdlib>
#include <cstring>
#include <memory>
#include <algorithm>
#include "dabgpu_pipe.h"

using namespace dab;
using front::StreamSt;

hipError_t dab::prof_mark(dabgpu_pipe *p, int stage, bool start) {
    if (!p->profiling) return hipSuccess;
    hipStream_t st = (stage >= DABGPU_STAGE_FIC) ? p->back[p->cur].stream : p->c->stream;
    if (p->profiling == 3) {                    // the stage alone on the device
        hipError_t r = hipDeviceSynchronize();
        if (r != hipSuccess) return r;
    }
    if (start) {
        size_t need = 2 * (p->ev_rec.size() + 1);
        while (p->ev_pool.size() < need) {
            Event e;
            hipError_t r = e.create(hipEventDefault);
            if (r != hipSuccess) return r;
            p->ev_pool.push_back(std::move(e));
        }
        int idx = (int)(2 * p->ev_rec.size());
        p->ev_rec.push_back({stage, idx});
        return p->ev_pool[idx].record(st);
    }
    hipError_t r = p->ev_pool[p->ev_rec.back().second + 1].record(st);
    if (r == hipSuccess && p->profiling == 3) r = hipDeviceSynchronize();
    return r;
}

// errors the back-end streams' kernels raised (refused out-of-bounds Viterbi sources):
// read for every back end known complete -- after a sync (wait) or by a non-blocking
// query -- and reported once
static int back_errors(dabgpu_pipe *p, bool wait) {
    for (int par = 0; par < 2; par++) {
        if (!p->back[par].ev_back.recorded()) continue;
        if (!wait) {
            const hipError_t q = p->back[par].ev_back.query();
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) return fail(DABGPU_E_HIP, "back-end stream %d: %s", par, hipGetErrorString(q));
        }
        const int32_t e = *(volatile int32_t *)&p->h_berr[par];
        if (e) {
            p->h_berr[par] = 0;
            return fail(DABGPU_E_BOUNDS, "kernel refused out-of-bounds work on back-end stream %d:%s", par,
                        (e & KERR_VITERBI) ? " viterbi source" : " (unknown)");
        }
    }
    return 0;
}

// DABGPU_CTL_INJECT_BOUNDS: the table the next run's MSC job reads its start offsets from
int dab::inject_table(dabgpu_pipe *p) {
    if (!p->substart_bad_d) {                       // (rebuild_tables drops it with the tables)
        // the start offsets in use (shared, or per entry) with the first decoded entry's
        // far past any ring (no int32 overflow in the loader)
        std::vector<int32_t> bad;
        if (p->uniform) {
            for (int i = 0; i < p->NSUB; i++) bad.push_back(p->tab[0][i].startAddr * 64);
            bad[0] = 0x40000000;
        } else {
            bad.assign((size_t)p->S * p->NSUB, 0);
            bool first = true;
            for (int s = 0; s < p->S; s++)
                for (int k = 0; k < (int)p->tab[s].size(); k++) {
                    bad[(size_t)s * p->NSUB + k] = first ? 0x40000000 : p->tab[s][k].startAddr * 64;
                    first = false;
                }
        }
        HIPCHK(p->substart_bad_d.put(bad));
    }
    return 0;
}

extern "C" {

// the background null search's stream (lowest priority), event and buffers
static int acq_async_setup(dabgpu_pipe *p) {
    if (p->acq.stream) return 0;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(p->acq.stream.create(lo));
    HIPCHK(p->acq.ev.create(hipEventDisableTiming));
    HIPCHK(p->acq.jobs_d.alloc(p->S));
    HIPCHK(p->acq.res_d.alloc(p->S));
    HIPCHK(p->acq.h_res.alloc(p->S));
    HIPCHK(p->acq.h_jobs.alloc(p->S));
    p->acq.acquiring.assign(p->S, 0);
    return 0;
}

int dabgpu_pipe_create(dabgpu_ctx *c, const dabgpu_pipe_cfg *cfg, dabgpu_pipe **out) {
    if (!c || !cfg || !out) return fail(DABGPU_E_ARG, "null arg");
    *out = nullptr;
    if (cfg->n_subch < 0 || (cfg->n_subch > 0 && !cfg->subch)) return fail(DABGPU_E_ARG, "bad sizes");
    // the caps of the table itself
    dabgpu_pipe_caps caps = {cfg->n_subch, 0, 0, 0};
    for (int i = 0; i < cfg->n_subch; i++) caps.max_bitrate = std::max<int32_t>(caps.max_bitrate, cfg->subch[i].bitRate);
    caps.max_dabplus = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_DABPLUS);
    caps.max_mp2 = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_MP2);
    return dabgpu_pipe_create_caps(c, cfg, &caps, out);
}

int dabgpu_pipe_create_caps(dabgpu_ctx *c, const dabgpu_pipe_cfg *cfg, const dabgpu_pipe_caps *caps, dabgpu_pipe **out) {
    if (!c || !cfg || !caps || !out) return fail(DABGPU_E_ARG, "null arg");
    *out = nullptr;
    if (cfg->n_streams <= 0 || cfg->n_frames <= 0 || cfg->n_subch < 0) return fail(DABGPU_E_ARG, "bad sizes");
    if (caps->max_subch < 0 || caps->max_bitrate < 0 || caps->max_dabplus < 0 || caps->max_dabplus > caps->max_subch ||
        caps->max_mp2 < 0 || caps->max_mp2 > caps->max_subch || caps->max_subch > 64 || caps->max_bitrate > 8 * DP_MAX_RS)
        return fail(DABGPU_E_ARG, "bad caps (at most 64 subchannels of at most 384 kbit/s)");
    if (cfg->freq_sync_method < 0 || cfg->freq_sync_method > 2)
        return fail(DABGPU_E_UNSUP, "freqSyncMethod %d (0, 1 or 2: ofdm-decoder.cpp:103-161)", cfg->freq_sync_method);
    // the packet-mode, MOT, PAD and audio output layers start with what the table flags (dabgpu_pipe_packet_caps)
    const int npk = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_PACKET);
    const int nmot = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_MOT);
    const int npad = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_PAD);
    const int naudio = slots::count_flag(cfg->subch, cfg->n_subch, DABGPU_SUBCH_AUDIO);
    const TableLimits lim{caps->max_subch, caps->max_bitrate, {caps->max_dabplus, caps->max_mp2, npk, nmot, npad, naudio}};
    if (int rc = check_table(cfg->subch, cfg->n_subch, lim)) return rc;
    auto p = std::make_unique<dabgpu_pipe>();
    p->c = c;
    p->S = cfg->n_streams;
    p->F = cfg->n_frames;
    p->NSUB = caps->max_subch;
    p->NDP = caps->max_dabplus;
    p->NMP = caps->max_mp2;
    p->max_bitrate = caps->max_bitrate;
    p->R = 2 * cfg->n_frames + 4;
    p->threshold = cfg->threshold;
    p->method = cfg->freq_sync_method;
    p->tab.assign(p->S, std::vector<dabgpu_subch>(cfg->subch, cfg->subch + cfg->n_subch));
    p->since.assign(p->S, std::vector<int64_t>(cfg->n_subch, 0));
    p->st.assign(p->S, StreamSt());
    p->max_nbits = std::max(768, 24 * p->max_bitrate);
    if (const char *e = getenv("DABGPU_NO_SPECULATE")) p->speculate = !(e[0] == '1');
    const size_t SF = (size_t)p->S * p->F;
    const size_t ring_bytes = (size_t)p->S * p->R * FRAME_SOFT;
    HIPCHK(p->ring.alloc(ring_bytes));
    HIPCHK(hipMemset(p->ring, RING8_BIAS, ring_bytes));
    HIPCHK(p->frames_d.alloc(SF));
    HIPCHK(p->si_d.alloc(SF));
    HIPCHK(p->corr_d.alloc(SF));
    HIPCHK(p->snr_d.alloc(SF));
    HIPCHK(p->fc_d.alloc(2 * SF));
    HIPCHK(p->fcpart_d.alloc(2 * SF * kMaxChunks));
    HIPCHK(p->h_frames.alloc(SF));
    HIPCHK(p->h_si.alloc(SF));
    HIPCHK(p->h_fc.alloc(SF));
    HIPCHK(p->h_snr.alloc(SF));
    p->desc_sz = (12 * (size_t)p->S + 4 * (size_t)SF + 15) / 16 * 16;
    HIPCHK(p->desc_d.alloc(2 * p->desc_sz));
    HIPCHK(p->h_desc.alloc(2 * p->desc_sz));
    HIPCHK(p->berr_d.alloc(2));
    HIPCHK(hipMemset(p->berr_d, 0, sizeof(int32_t) * 2));
    HIPCHK(p->h_berr.alloc(2));
    p->h_berr[0] = p->h_berr[1] = 0;
    HIPCHK(p->ficprof_d.put({fic_profile()}));
    // MSC decisions, then the FIC's (both jobs of one run decode in one launch)
    const int64_t msc_words = p->NSUB > 0 ? dec_bytes(SF * 4 * p->NSUB, p->max_nbits) / 4 : 0;
    p->dec_fic_off = msc_words;
    const size_t dec_words = (size_t)(msc_words + dec_bytes(SF * 4, 768) / 4);
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    for (BackSlot &b : p->back) {
        HIPCHK(b.dec.alloc(dec_words));
        HIPCHK(b.stream.create(prio_least));
        for (Event *e : {&b.ev_copy, &b.ev_back, &b.ev_acs}) HIPCHK(e->create(hipEventDisableTiming));
    }
    HIPCHK(p->dp.ev.create(hipEventDisableTiming));
    HIPCHK(p->ev_front.create(hipEventDisableTiming));
    if (p->NDP) {
        const size_t nd = (size_t)p->S * p->NDP;
        HIPCHK(p->dp.map.alloc(nd));
        HIPCHK(p->dp.ring_d.zalloc(nd * 120 * DP_MAX_RS));
        HIPCHK(p->dp.state_d.zalloc(nd));
        HIPCHK(p->dp.code_d.alloc(nd * 4 * p->F));
    }
    if (p->NMP) {
        Mp2Layer &m = p->mp2;
        const size_t nm = (size_t)p->S * p->NMP;
        m.fstride = 6 * std::max(p->max_bitrate, 1);
        HIPCHK(m.ev.create(hipEventDisableTiming));
        HIPCHK(m.map.alloc(nm));
        HIPCHK(m.sync_d.zalloc(nm));
        HIPCHK(m.part_d.zalloc(nm * m.fstride));
        HIPCHK(m.frames_d.alloc(nm * 4 * p->F * m.fstride));
        HIPCHK(m.present_d.alloc(nm * 4 * p->F));
        for (auto &v : m.vstate_d) HIPCHK(v.zalloc(nm * MP2_STATE_I16));
    }
    if (npk)
        if (int rc = packet_size(p.get(), npk, DABGPU_PKT_GROUP_BYTES)) return rc;
    if (nmot)
        if (int rc = mot_size(p.get(), nmot, DABGPU_MOT_BODY_BYTES)) return rc;
    if (npad)
        if (int rc = pad_size(p.get(), npad)) return rc;
    if (naudio)
        if (int rc = audio_size(p.get(), naudio)) return rc;
    if (int rc = rebuild_tables(p.get())) return rc;
    // the default re-acquisition mode: a stream that loses sync is searched in the
    // background (DABGPU_CTL_ACQ_ASYNC; DABGPU_CTL_ACQ_SYNC restores the in-run search)
    if (int rc = acq_async_setup(p.get())) return rc;
    p->acq.async = true;
    *out = p.release();
    return 0;
}

int dabgpu_pipe_destroy(dabgpu_pipe *p) {
    delete p;
    return 0;
}

}  // extern "C"

static AcqJob acq_job(const dabgpu_pipe *p, const StreamSt &x, int s, int64_t stride, const int64_t *n_avail) {
    // the kernel enters notSynced (attempts++) first; a cut attempt is repeated whole
    return AcqJob{stride * s, x.window, n_avail[s], x.lp, x.coarse + x.fine, x.attempts - (x.in_attempt ? 1 : 0),
                  p->scan ? 1 : 0};
}

// Null-symbol search (notSynced .. SyncOnEndNull, ofdm-processor.cpp:274-338) for the
// streams `who` of `cur`, each from its current position (window, localPhase) with
// its correctors: one k_acquire wave per stream.  A stream that finds the end of a
// null symbol is synchronised at SyncOnPhase; one that runs out of samples stays
// unsynchronised at the end of its samples (the next call continues from there).
static int acquire_streams(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *n_avail,
                           const std::vector<int> &who, std::vector<StreamSt> &cur, int &found) {
    dabgpu_ctx *c = p->c;
    found = 0;
    if (who.empty()) return 0;
    std::vector<AcqJob> jobs;
    for (int s : who) jobs.push_back(acq_job(p, cur[s], s, stride, n_avail));
    void *jd = nullptr, *rd = nullptr;
    if (int rc = scratch(c, SC_MISC, sizeof(AcqJob) * jobs.size(), &jd)) return rc;
    if (int rc = scratch(c, SC_ACQ, sizeof(AcqResult) * jobs.size(), &rd)) return rc;
    HIPCHK(hipMemcpyAsync(jd, jobs.data(), sizeof(AcqJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_acquire(c->stream, iq, p->iq_fmt, (const AcqJob *)jd, (int)jobs.size(), c->osc, (AcqResult *)rd));
    std::vector<AcqResult> res(jobs.size());
    HIPCHK(hipMemcpyAsync(res.data(), rd, sizeof(AcqResult) * jobs.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < jobs.size(); i++) found += front::acq_apply(cur[who[i]], res[i]);
    return 0;
}

// Background form (DABGPU_CTL_ACQ_ASYNC): the same search launched on the pipeline's
// acquisition stream without waiting; acq_collect applies the results once they are in.
static int acquire_streams_async(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *n_avail,
                                 const std::vector<int> &who, const std::vector<StreamSt> &cur) {
    for (size_t i = 0; i < who.size(); i++) p->acq.h_jobs[i] = acq_job(p, cur[who[i]], who[i], stride, n_avail);
    const size_t n = who.size();
    HIPCHK(hipMemcpyAsync(p->acq.jobs_d, p->acq.h_jobs, sizeof(AcqJob) * n, hipMemcpyHostToDevice, p->acq.stream));
    HIPCHK(launch_acquire(p->acq.stream, iq, p->iq_fmt, p->acq.jobs_d, (int)n, p->c->osc, p->acq.res_d));
    HIPCHK(hipMemcpyAsync(p->acq.h_res, p->acq.res_d, sizeof(AcqResult) * n, hipMemcpyDeviceToHost, p->acq.stream));
    HIPCHK(p->acq.ev.record(p->acq.stream));
    p->acq.who = who;
    for (int s : who) p->acq.acquiring[s] = 1;
    p->acq.inflight = true;
    return 0;
}
static int acq_collect(dabgpu_pipe *p, bool wait) {
    if (!p->acq.inflight) return 0;
    const hipError_t q = wait ? p->acq.ev.sync() : p->acq.ev.query();
    if (q == hipErrorNotReady) return 0;
    if (q != hipSuccess) return fail(DABGPU_E_HIP, "background null search: %s", hipGetErrorString(q));
    for (size_t i = 0; i < p->acq.who.size(); i++) {
        const int s = p->acq.who[i];
        (void)front::acq_apply(p->st[s], p->acq.h_res[i]);
        p->acq.acquiring[s] = 0;
    }
    p->acq.who.clear();
    p->acq.inflight = false;
    return 0;
}

extern "C" int dabgpu_pipe_acquire(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *start_h,
                                   const int64_t *n_avail_h) {
    if (!p || !iq || !start_h || !n_avail_h) return fail(DABGPU_E_ARG, "null arg");
    std::vector<int> who;
    for (int s = 0; s < p->S; s++)
        if (!p->st[s].synced) {
            who.push_back(s);
            p->st[s].window = start_h[s];
        }
    int found = 0;
    if (int rc = acquire_streams(p, iq, stride, n_avail_h, who, p->st, found)) return rc;
    if (found < (int)who.size()) return fail(DABGPU_E_STATE, "%d stream(s) found no null symbol", (int)who.size() - found);
    return 0;
}

// One speculative front-end pass over the uncommitted frames of every stream: predict
// windows (startIndex = last one) and correctors (unchanged), run the batched kernels on
// the prediction, then replay ofdmProcessor::run's sequential logic with the measured
// values and commit the longest correctly predicted prefix of each stream.  All of that
// logic is front_replay.h's; here are the staging, the launches and the error checks, in
// two halves: front_launch predicts and makes the pass's first launches, front_finish
// waits for them and does the rest.  Between the two dabgpu_pipe_run queues the speculative
// back end, which reads the prediction in P (the caller's).

// the pipeline's demod, on either path
static DemodAux pipe_demod_aux(const dabgpu_pipe *p) {
    DemodAux aux{};
    aux.disp = p->display ? p->disp_d.ptr : nullptr;
    aux.disp_token = p->disp_token;
    aux.ring8 = 1;
    aux.fmt = p->iq_fmt;
    return aux;
}

// gate: record ev_front behind the demod, for a speculative back end queued after this call
static int front_launch(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *n_avail,
                        const std::vector<int> &done, const std::vector<StreamSt> &cur, front::Pass &P, bool gate) {
    dabgpu_ctx *c = p->c;
    front::predict(P, cur, done, p->F, p->R, stride, n_avail);
    const int n = P.n();
    if (n == 0) return 0;
    // Steady state (no stream runs the coarse AFC of processBlock_0): ONE launch per
    // pass -- every predicted frame's workgroup runs findIndex on its window, places
    // the frame at the startIndex it finds, reports get_snr of block 0 and demodulates
    // the 75 symbols (k_demod_wg<.., SYNC>); one host round trip per pass.  Frames the
    // replay does not commit are re-predicted and decoded again.  While a
    // stream's coarse AFC is pending the host needs startIndex and processBlock_0's
    // correction first: findIndex, block 0 and the demod run as three launches.
    memcpy(p->h_frames, P.fr.data(), sizeof(dabgpu_frame) * n);
    HIPCHK(hipMemcpyAsync(p->frames_d, p->h_frames, sizeof(dabgpu_frame) * n, hipMemcpyHostToDevice, c->stream));
    if (P.fast) {
        DemodAux sync = pipe_demod_aux(p);
        sync.si = p->si_d;
        sync.snr = p->snr_d;
        sync.level = p->threshold;
        HIPCHK(prof_mark(p, DABGPU_STAGE_DEMOD, true));
        const int kChunks = demod_chunks(n, 2);
        HIPCHK(launch_demod(c->stream, iq, p->frames_d, n, kChunks, c->T, (int16_t *)p->ring.ptr, nullptr, p->fcpart_d, P.general, sync));
        HIPCHK(prof_mark(p, DABGPU_STAGE_DEMOD, false));
        // the speculative back end waits for the demod only:
        // the publish feeds the host, not the decoders -- one kernel and its dispatch off
        // the ACS's critical path (profiles/r05_back_gate_ab.txt).  The publish is still
        // launched first, so the ACS's waves do not take the slot it needs before the host
        // can read the pass.
        if (gate) {
            HIPCHK(p->ev_front.record(c->stream));
            p->ev_front_demod = true;
        }
        // the host's values and the error word straight into pinned memory (no copies)
        HIPCHK(launch_front_publish(c->stream, p->fcpart_d, kChunks, n, p->fc_d, (float *)p->h_fc.ptr, p->si_d,
                                    p->h_si, p->snr_d, p->h_snr, c->err, c->h_err));
    } else {
        HIPCHK(prof_mark(p, DABGPU_STAGE_PRS, true));
        HIPCHK(launch_prs_sync(c->stream, iq, p->iq_fmt, p->frames_d, n, c->T, p->threshold, p->si_d, nullptr, nullptr, P.general));
        HIPCHK(prof_mark(p, DABGPU_STAGE_PRS, false));
        HIPCHK(hipMemcpyAsync(p->h_si, p->si_d, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    }
    return 0;
}

static int front_finish(dabgpu_pipe *p, const void *iq, const int64_t *n_avail, std::vector<int> &done,
                        std::vector<StreamSt> &cur, front::Pass &P, bool &progress, bool &lost) {
    dabgpu_ctx *c = p->c;
    const int n = P.n();
    const bool fast = P.fast;
    progress = false;
    if (n == 0) return 0;
    if (fast) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (const int32_t e = *(volatile int32_t *)c->h_err.ptr) return bounds_error(e);
        for (int i = 0; i < n; i++) {                           // demodulated and measured by front_launch
            P.e[i].fc = front::FreqCorr{p->h_fc[i].x, p->h_fc[i].y};
            P.e[i].snr = p->h_snr[i];
        }
    } else if (int rc = kernel_errors(c)) {
        return rc;
    }
    for (int i = 0; i < n; i++) P.e[i].si = p->h_si[i];
    front::place(P, n_avail);
    std::vector<int> idx;
    std::vector<dabgpu_frame> sel;
    // processBlock_0 (get_snr; coarse AFC for the frames with f2 on) of the usable frames
    if (!fast) P.usable(idx, sel);
    if (const int n2 = (int)sel.size()) {
        std::vector<int16_t> corr(n2), snr(n2);
        HIPCHK(hipMemcpyAsync(p->frames_d, sel.data(), sizeof(dabgpu_frame) * n2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(prof_mark(p, DABGPU_STAGE_BLOCK0, true));
        HIPCHK(launch_block0(c->stream, iq, p->iq_fmt, p->frames_d, n2, c->T, p->method, p->corr_d, p->snr_d, P.general));
        HIPCHK(prof_mark(p, DABGPU_STAGE_BLOCK0, false));
        HIPCHK(hipMemcpyAsync(corr.data(), p->corr_d, sizeof(int16_t) * n2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(snr.data(), p->snr_d, sizeof(int16_t) * n2, hipMemcpyDeviceToHost, c->stream));
        if (int rc = kernel_errors(c)) return rc;
        for (int k = 0; k < n2; k++) { P.e[idx[k]].corr = corr[k]; P.e[idx[k]].snr = snr[k]; }
    }
    front::replay_coarse(P, cur);
    // demod of the frames still usable
    sel.clear();
    if (!fast) P.usable(idx, sel);
    if (const int n3 = (int)sel.size()) {
        std::vector<float2> fc(n3);
        HIPCHK(hipMemcpyAsync(p->frames_d, sel.data(), sizeof(dabgpu_frame) * n3, hipMemcpyHostToDevice, c->stream));
        HIPCHK(prof_mark(p, DABGPU_STAGE_DEMOD, true));
        const int kChunks = demod_chunks(n3);
        HIPCHK(launch_demod(c->stream, iq, p->frames_d, n3, kChunks, c->T, (int16_t *)p->ring.ptr, nullptr, p->fcpart_d, P.general,
                            pipe_demod_aux(p)));
        HIPCHK(prof_mark(p, DABGPU_STAGE_DEMOD, false));
        HIPCHK(launch_fc_reduce(c->stream, p->fcpart_d, kChunks, n3, p->fc_d));
        HIPCHK(hipMemcpyAsync(fc.data(), p->fc_d, sizeof(float2) * n3, hipMemcpyDeviceToHost, c->stream));
        if (int rc = kernel_errors(c)) return rc;
        for (int k = 0; k < n3; k++) P.e[idx[k]].fc = front::FreqCorr{fc[k].x, fc[k].y};
    }
    progress = front::commit(P, cur, done, [&](int s, int f, const dabgpu_frame &d, const dabgpu_frame_info &fi, const StreamSt &) {
        const size_t i = (size_t)s * p->F + f;
        p->last_frames[i] = d;
        p->last_info[i] = fi;
    });
    if (front::sync_lost(P, cur, done)) lost = true;
    return 0;
}

// the caller's output pointers of a run (dabgpu_pipe_run's arguments)
struct RunOut {
    uint8_t *fic_bits, *fic_crc, *msc_bits;
    int32_t msc_stride;
    bool do_msc;                     // MSC rows wanted and some stream has an entry to decode
};

// what the FIC's and the MSC's jobs share: n_cw codewords of up to nbits bits from the soft-bit ring
static VitJob ring_job(const dabgpu_pipe *p, int par, int32_t kind, int n_cw, int nbits, int64_t dec_off) {
    VitJob J;
    memset(&J, 0, sizeof J);
    J.kind = kind;
    J.n_cw = n_cw;
    J.src = (const int16_t *)p->ring.ptr;
    J.ring8 = 1;
    J.src_len = (int64_t)p->S * p->R * FRAME_SOFT;
    J.err = p->berr_d + par;
    J.prbs = 1;
    J.prbs_words = p->c->prbs;
    J.dec = p->back[par].dec + dec_off;
    J.dec_ncw = dec_rows(n_cw);
    J.dec_nch = dec_chunks(nbits);
    return J;
}
static VitJob make_fic_job(const dabgpu_pipe *p, int par, uint8_t *fic_bits) {
    VitJob J = ring_job(p, par, SRC_FIC, 4 * p->S * p->F, 768, p->dec_fic_off);
    J.slots = p->slots_dev(par);
    J.prof = (const Profile *)p->ficprof_d;
    J.inv = p->c->fic_inv;
    J.out = fic_bits;
    J.out_stride = p->fic_packed ? 96 : 768;     // 3 FIBs of 32 bytes, or 768 bits
    J.packed = p->fic_packed ? 1 : 0;
    return J;
}
static VitJob make_msc_job(const dabgpu_pipe *p, int par, uint8_t *msc_bits, int32_t msc_stride) {
    VitJob J = ring_job(p, par, SRC_MSC, p->S * 4 * p->F * p->NSUB, p->max_nbits, 0);
    J.prof = p->prof_d;
    J.inv = p->inv_d;
    J.nsub = p->NSUB;
    J.ncif = 4 * p->F;
    J.ring = p->R;
    J.cif0s = p->cif0_dev(par);
    J.ncifs = p->ncif_dev(par);
    J.sub_start = p->inject_bounds ? p->substart_bad_d : p->substart_d;
    if (!p->uniform) {                          // per-stream tables, the active pairs only
        J.ent_prof = p->ent_prof_d;
        J.ent_start = p->inject_bounds ? p->substart_bad_d : p->ent_start_d;
        J.ent_since = p->ent_since_d;
        J.act = p->act_d;
        J.n_acs = p->n_act * 4 * p->F;
    }
    J.out = msc_bits;
    J.out_stride = msc_stride;
    J.packed = p->packed ? 1 : 0;
    return J;
}

// Channel decoding on back-end stream `par`, after this run's front end: FIC for every
// committed frame (slots[s*F+f] = its ring slot, -1 none), MSC for all subchannels of every
// delivered CIF (dn[s] frames of stream s).  With both, one ACS and one traceback launch
// decode them together (the FIC's short waves fill the SIMDs the MSC's last waves leave
// idle); decisions in separate halves of the stream's decision buffer.
static int enqueue_back(dabgpu_pipe *p, int par, const RunOut &o, const std::vector<int> &dn,
                        const std::vector<int32_t> &slots) {
    dabgpu_ctx *c = p->c;
    BackSlot &b = p->back[par];
    hipStream_t bs = b.stream;
    const int S = p->S, F = p->F;
    const bool fic = o.fic_bits != nullptr, msc = o.do_msc;
    // per stream: CIF index of its first CIF slot and the CIFs it delivered (the
    // staging half is reused only once its previous uploads have executed)
    HIPCHK(b.ev_copy.sync());
    for (int s = 0; s < S; s++) {
        p->h_cif0(par)[s] = p->st[s].cif_count;
        p->h_ncif(par)[s] = 4 * dn[s];
    }
    if (fic) memcpy(p->h_slots(par), slots.data(), sizeof(int32_t) * S * F);
    // one upload of the block (the FIC slots only when the FIC is decoded)
    HIPCHK(hipMemcpyAsync(p->cif0_dev(par), p->h_cif0(par), 12 * (size_t)S + (fic ? 4 * (size_t)S * F : 0),
                          hipMemcpyHostToDevice, bs));
    HIPCHK(b.ev_copy.record(bs));
    // the small upload above runs on the back-end stream while the front end still
    // works; only the decoders wait for it.
    // What the back end may read of the front end's output: the soft-bit ring (p->ring,
    // written by the demod) and the host-built descriptors uploaded on bs above -- never
    // what k_front_publish writes (fc_d, si_d, snr_d, the error word): ev_front may mark
    // the demod alone (ev_front_demod), before the publish.  A back-end reader of those
    // must wait for an event recorded after the publish.  (Measured: launching run r's traceback beside
    // run r+1's ACS instead of beside run r+1's demod is 2 % slower -- the ACS loses more than the demod gains.)
    if (!p->ev_front_demod) HIPCHK(p->ev_front.record(c->stream));
    p->ev_front_demod = false;
    HIPCHK(p->ev_front.wait_on(bs));
    if (!fic && !msc) return 0;
    // ACS (joint, FIC only or MSC only) -> ev_acs -> traceback -> FIB CRCs.  Stage times:
    // the MSC's stages take the joint kernels; the FIC stage is the FIB CRCs beside an MSC,
    // the whole decode without one
    const VitJob JF = fic ? make_fic_job(p, par, o.fic_bits) : VitJob();
    const VitJob JM = msc ? make_msc_job(p, par, o.msc_bits, o.msc_stride) : VitJob();
    HIPCHK(prof_mark(p, msc ? DABGPU_STAGE_MSC_ACS : DABGPU_STAGE_FIC, true));
    HIPCHK(fic && msc ? launch_acs_msc_fic(bs, JM, JF) : launch_acs(bs, msc ? JM : JF));
    if (msc) HIPCHK(prof_mark(p, DABGPU_STAGE_MSC_ACS, false));
    HIPCHK(b.ev_acs.record(bs));
    if (msc) HIPCHK(prof_mark(p, DABGPU_STAGE_MSC_TB, true));
    HIPCHK(fic && msc ? launch_traceback_msc_fic(bs, JM, JF) : launch_traceback(bs, msc ? JM : JF));
    if (msc) HIPCHK(prof_mark(p, DABGPU_STAGE_MSC_TB, false));
    if (!fic) return 0;
    if (msc) HIPCHK(prof_mark(p, DABGPU_STAGE_FIC, true));
    if (o.fic_crc) HIPCHK(launch_fic_post(bs, o.fic_bits, o.fic_crc, 12 * S * F, c->dptab, p->slots_dev(par), p->fic_packed));
    HIPCHK(prof_mark(p, DABGPU_STAGE_FIC, false));
    return 0;
}

// Speculative back end: in steady state (every stream synchronised, no coarse AFC
// pending) the first front pass commits exactly the frames it predicts, so the
// channel decoding of those frames is queued right behind it, before the host has
// read and verified the pass -- the GPU does not idle through the host's replay.  If
// the replay commits anything else, or a second pass rewrites frames, the back end
// is queued again with the committed frames and overwrites the outputs.
struct Spec {
    bool on = false, sent = false;
    size_t rec0 = 0, rec1 = 0;                   // profiling records of the speculative enqueue
    std::vector<int> pred;                       // [S] frames it decodes (front::predicted_whole)
    std::vector<int32_t> pred_slot;              // [S][F] their ring slots
};
// an error after the speculative back end was queued: it still writes the caller's
// outputs and reads ring slots, so it is tracked like a completed run's back end
// (the next run's demod waits for it) and finished before the error returns
static int bail(dabgpu_pipe *p, int par, const Spec &sp, int rc) {
    if (sp.sent) {
        BackSlot &b = p->back[par];
        (void)launch_take_error(b.stream, p->berr_d + par, p->h_berr + par);
        (void)b.ev_back.record(b.stream);
        (void)b.stream.sync();
    }
    return rc;
}
// the back end's last step: publish (and clear) its error word, mark the run's back end done
static int finish_back(dabgpu_pipe *p, int par) {
    BackSlot &b = p->back[par];
    HIPCHK(launch_take_error(b.stream, p->berr_d + par, p->h_berr + par));
    HIPCHK(b.ev_back.record(b.stream));
    return 0;
}

// Streams that need the null search: in the background (DABGPU_CTL_ACQ_ASYNC, the
// default) those that lost sync after an acquisition -- this run goes on without
// them, one batch in flight; inside the run (the reference's order) the others: a
// stream's first search (it has no frames to decode before it) and, with
// DABGPU_CTL_ACQ_SYNC, every search.  found: streams synchronised inside the run.
static int acquire_pending(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *n_avail,
                           const std::vector<int> &done, std::vector<StreamSt> &cur, int &found) {
    std::vector<int> who, bg;
    for (int s = 0; s < p->S; s++) {
        if (cur[s].synced || done[s] >= p->F) continue;
        if (p->acq.async && cur[s].acquisitions > 0) {
            if (!p->acq.acquiring[s]) bg.push_back(s);
        } else {
            who.push_back(s);
        }
    }
    found = 0;
    if (!bg.empty() && !p->acq.inflight)
        if (int rc = acquire_streams_async(p, iq, stride, n_avail, bg, cur)) return rc;
    return acquire_streams(p, iq, stride, n_avail, who, cur, found);
}

// msc_valid (optional, [S][4F]) and the per-entry validity of the run: the CIF was delivered
// (done[s] frames of stream s) and lies past the 16-CIF warm-up -- the stream's, the entry's own
static void publish_validity(dabgpu_pipe *p, const std::vector<int> &done, bool have_rows, uint8_t *msc_valid) {
    const int S = p->S, F = p->F;
    if (msc_valid)
        for (int s = 0; s < S; s++)
            for (int q = 0; q < 4 * F; q++)
                msc_valid[(size_t)s * 4 * F + q] = (q < 4 * done[s] && p->st[s].cif_count + q >= 16) ? 1 : 0;
    p->entry_valid.assign((size_t)S * 4 * F * p->NSUB, 0);
    if (have_rows)
        for (int s = 0; s < S; s++)
            for (int q = 0; q < 4 * done[s]; q++)
                for (int k = 0; k < (int)p->tab[s].size(); k++)
                    p->entry_valid[((size_t)s * 4 * F + q) * p->NSUB + k] = p->st[s].cif_count + q - p->since[s][k] >= 16;
}

extern "C" {

int dabgpu_pipe_run(dabgpu_pipe *p, const void *iq, int64_t stride, const int64_t *n_avail, uint8_t *fic_bits,
                    uint8_t *fic_crc, uint8_t *msc_bits, int32_t msc_stride, uint8_t *msc_valid) {
    if (!p || !iq || !n_avail) return fail(DABGPU_E_ARG, "null arg");
    dabgpu_ctx *c = p->c;
    const int S = p->S, F = p->F;
    const bool have_rows = msc_bits && p->NSUB > 0;
    // (no entry in any stream's table: nothing to decode)
    const RunOut out{fic_bits, fic_crc, msc_bits, msc_stride, have_rows && p->n_act > 0};
    const int need = p->packed ? (p->max_nbits + 7) / 8 : p->max_nbits;
    if (have_rows && msc_stride < need) return fail(DABGPU_E_ARG, "msc_stride %d < %d", msc_stride, need);
    if (int rc = back_errors(p, false)) return rc;
    if (int rc = acq_collect(p, false)) return rc;        // a background null search that finished
    p->last_frames.assign((size_t)S * F, dabgpu_frame());
    p->last_info.assign((size_t)S * F, dabgpu_frame_info());
    p->feed.last_msc = nullptr;                // (a run that fails leaves no rows and no FIBs to consume)
    p->feed.fic_pending = false;
    if (p->profiling == 1) p->ev_rec.clear();   // modes 2, 3 accumulate over runs
    p->ev_front_demod = false;
    // at most one run of overlap: run r-2's ACS, the last reader of the ring slots this
    // run's demod reuses, must be done (not its traceback, FIC CRC and DAB+ layer: waiting
    // for those held the demod back from the slots the ACS's last waves leave free --
    // profiles/r04_front_gate_ab.txt)
    const int par = (int)(p->run_idx & 1);
    BackSlot &b = p->back[par];
    HIPCHK(b.ev_acs.wait_on(c->stream));
    std::vector<int> done(S, 0);
    std::vector<StreamSt> cur = p->st;
    p->cur = par;
    Spec sp;
    sp.on = (fic_bits || out.do_msc) && p->speculate && front::steady(cur);
    // ofdmProcessor::run per stream: speculative front-end passes commit frames; a
    // stream that loses sync (or was never synchronised) searches the next null
    // symbol from where it is and continues (goto notSynced, ofdm-processor.cpp:354-357).
    // Every pass either commits a frame or moves a stream past samples, so this ends.
    front::Pass P;
    int passes = 0;
    for (int it = 0; it < 64 * F + 64; it++) {
        int found = 0;
        if (int rc = acquire_pending(p, iq, stride, n_avail, done, cur, found)) return bail(p, par, sp, rc);
        bool progress = false, lost = false;
        const bool spec = sp.on && it == 0 && found == 0;
        if (int rc = front_launch(p, iq, stride, n_avail, done, cur, P, spec)) return bail(p, par, sp, rc);
        if (spec && P.n()) {                     // the frames this pass predicted whole, decoded behind it
            front::predicted_whole(P, S, F, n_avail, sp.pred, sp.pred_slot);
            sp.sent = true;
            sp.rec0 = p->ev_rec.size();
            const int rc = enqueue_back(p, par, out, sp.pred, sp.pred_slot);
            sp.rec1 = p->ev_rec.size();
            if (rc) return bail(p, par, sp, rc);
        }
        if (int rc = front_finish(p, iq, n_avail, done, cur, P, progress, lost)) return bail(p, par, sp, rc);
        if (P.n()) passes++;                     // (a pass with nothing to predict launches nothing)
        if (!progress && !lost && !found) break;
    }
    bool all = true;
    for (int s = 0; s < S; s++) {
        if (done[s] != F && !(p->acq.async && cur[s].acquisitions > 0 && (p->acq.acquiring[s] || !cur[s].synced))) all = false;
        cur[s].frames_run = done[s];
    }
    // the speculation hit if the one pass committed exactly what it predicted; else the
    // back end is queued (again) with what was committed
    std::vector<int32_t> slot((size_t)S * F, -1);
    for (int s = 0; s < S; s++)
        for (int f = 0; f < done[s]; f++) slot[(size_t)s * F + f] = p->last_frames[(size_t)s * F + f].out_slot;
    const bool hit = sp.sent && passes == 1 && done == sp.pred && slot == sp.pred_slot;
    if (!hit) {
        // the speculative decode is overwritten: its stage times are not this run's
        for (size_t i = sp.rec0; i < sp.rec1; i++) p->ev_rec[i].first = -1;
        if (int rc = enqueue_back(p, par, out, done, slot)) return bail(p, par, sp, rc);
    }
    if (int rc = finish_back(p, par)) return bail(p, par, sp, rc);
    p->run_idx++;
    p->inject_bounds = false;
    LayerFeed &f = p->feed;
    f.last_msc = have_rows ? msc_bits : nullptr;
    f.last_msc_stride = msc_stride;
    f.last_msc_packed = p->packed;
    f.last_fic = fic_bits;
    f.last_crc = fic_crc;
    f.last_fic_packed = p->fic_packed;
    f.new_run(have_rows, fic_bits && fic_crc);
    publish_validity(p, done, have_rows, msc_valid);
    for (int s = 0; s < S; s++) cur[s].cif_count = p->st[s].cif_count + 4 * (int64_t)done[s];
    p->st = cur;
    if (!all) return fail(DABGPU_E_STATE, "a stream ran out of samples (see dabgpu_pipe_state)");
    return 0;
}

int dabgpu_pipe_set_profiling(dabgpu_pipe *p, int on) {
    if (!p) return fail(DABGPU_E_ARG, "null pipe");
    if (on < 0 || on > 3) return fail(DABGPU_E_ARG, "profiling mode %d", on);
    if (int rc = sync_streams(p)) return rc;            // events of earlier runs are complete
    p->profiling = on;
    p->ev_rec.clear();
    return 0;
}
int dabgpu_pipe_timing(dabgpu_pipe *p, float *ms, int32_t *launches) {
    if (!p || !ms) return fail(DABGPU_E_ARG, "bad args");
    // stages recorded since the last dabgpu_pipe_run started (incl. dabgpu_pipe_dabplus)
    if (int rc = sync_streams(p)) return rc;
    for (int k = 0; k < DABGPU_NSTAGE; k++) { ms[k] = 0.0f; if (launches) launches[k] = 0; }
    for (auto &r : p->ev_rec) {
        if (r.first < 0) continue;              // discarded (a missed speculation)
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, p->ev_pool[r.second].e, p->ev_pool[r.second + 1].e));
        ms[r.first] += t;
        if (launches) launches[r.first] += 1;
    }
    return 0;
}

int dabgpu_pipe_acquire_wait(dabgpu_pipe *p) {
    if (!p) return fail(DABGPU_E_ARG, "null pipe");
    return acq_collect(p, true);
}

int dabgpu_pipe_sync(dabgpu_pipe *p) {
    if (!p) return fail(DABGPU_E_ARG, "null pipe");
    if (int rc = sync_streams(p)) return rc;
    if (int rc = back_errors(p, true)) return rc;
    return kernel_errors(p->c);
}

int dabgpu_pipe_state(dabgpu_pipe *p, int s, dabgpu_stream_state *o) {
    if (!p || !o || s < 0 || s >= p->S) return fail(DABGPU_E_ARG, "bad args");
    // a background null search that has finished is taken now (not at the next run), so
    // `acquiring` says whether the search still reads iq_d
    if (int rc = acq_collect(p, false)) return rc;
    const StreamSt &x = p->st[s];
    o->next_pos = x.window;
    o->local_phase = x.lp;
    o->coarse = x.coarse;
    o->fine = x.fine;
    o->f2correction = x.f2;
    o->prev1 = x.prev1;
    o->prev2 = x.prev2;
    o->synced = x.synced;
    o->cif_count = x.cif_count;
    o->last_start_index = x.last_si;
    o->resyncs = x.resyncs;
    o->acquisitions = x.acquisitions;
    o->attempts = x.attempts;
    o->no_signal = x.no_signal;
    o->frames_run = x.frames_run;
    o->acquiring = (p->acq.async && !p->acq.acquiring.empty() && p->acq.acquiring[s]) ? 1 : 0;
    return 0;
}

int dabgpu_pipe_frame_info(dabgpu_pipe *p, dabgpu_frame_info *info) {
    if (!p || !info) return fail(DABGPU_E_ARG, "bad args");
    if (p->last_info.empty()) memset(info, 0, sizeof(dabgpu_frame_info) * (size_t)p->S * p->F);
    else memcpy(info, p->last_info.data(), sizeof(dabgpu_frame_info) * p->last_info.size());
    return 0;
}

int dabgpu_pipe_control(dabgpu_pipe *p, int stream, int op) {
    if (!p || stream < -1 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (op == DABGPU_CTL_SCAN_ON || op == DABGPU_CTL_SCAN_OFF) {      // set_scanMode (one flag, like the reference's)
        p->scan = op == DABGPU_CTL_SCAN_ON;
        return 0;
    }
    if (op == DABGPU_CTL_INJECT_BOUNDS) {
        if (p->n_act == 0) return fail(DABGPU_E_STATE, "no MSC subchannel to corrupt");
        if (int rc = inject_table(p)) return rc;
        p->inject_bounds = true;
        return 0;
    }
    if (op == DABGPU_CTL_ACQ_ASYNC || op == DABGPU_CTL_ACQ_SYNC) {
        if (op == DABGPU_CTL_ACQ_SYNC) {
            if (int rc = acq_collect(p, true)) return rc;   // a search in flight completes first
            p->acq.async = false;
            return 0;
        }
        if (int rc = acq_async_setup(p)) return rc;
        p->acq.async = true;
        return 0;
    }
    // a background search in flight carries the stream's old correctors and position: it
    // completes and is applied first, so the control below is the last word (the reference
    // runs these methods between its own sequential steps)
    if (int rc = acq_collect(p, true)) return rc;
    for (auto [s, end] = stream_range(p, stream); s < end; s++) {
        StreamSt &x = p->st[s];
        switch (op) {
        case DABGPU_CTL_RESET: x.fine = 0; x.coarse = 0; x.f2 = true; break;      // ofdm-processor.cpp:476-479
        case DABGPU_CTL_COARSE_ON: x.f2 = true; x.coarse = 0; break;             // :498-501
        case DABGPU_CTL_COARSE_OFF: x.f2 = false; break;                         // :503-505
        case DABGPU_CTL_RESYNC: x.synced = false; break;
        default: return fail(DABGPU_E_ARG, "unknown control op %d", op);
        }
    }
    return 0;
}

int dabgpu_pipe_softbits(dabgpu_pipe *p, const uint8_t **soft, int32_t *ring) {
    if (!p || !soft || !ring) return fail(DABGPU_E_ARG, "bad args");
    *soft = p->ring;
    *ring = p->R;
    return 0;
}
int dabgpu_pipe_frame_slot(dabgpu_pipe *p, int frame, int32_t *slot) {
    if (!p || !slot || frame < 0 || frame >= p->F) return fail(DABGPU_E_ARG, "bad args");
    *slot = p->last_frames.empty() ? -1 : p->last_frames[frame].out_slot;
    return 0;
}
int dabgpu_pipe_msc_entry_valid(dabgpu_pipe *p, uint8_t *valid_h) {
    if (!p || !valid_h) return fail(DABGPU_E_ARG, "bad args");
    const size_t nb = (size_t)p->S * 4 * p->F * p->NSUB;
    if (p->entry_valid.size() != nb) memset(valid_h, 0, nb);   // no run yet
    else memcpy(valid_h, p->entry_valid.data(), nb);
    return 0;
}

int dabgpu_pipe_set_packed(dabgpu_pipe *p, int on) {
    if (!p || on < 0 || on > (DABGPU_PACK_MSC | DABGPU_PACK_FIC)) return fail(DABGPU_E_ARG, "packing %d", on);
    p->packed = (on & DABGPU_PACK_MSC) != 0;
    p->fic_packed = (on & DABGPU_PACK_FIC) != 0;
    return 0;
}
int dabgpu_pipe_set_iq_format(dabgpu_pipe *p, int format) {
    if (!p || (format != DABGPU_IQ_F32 && format != DABGPU_IQ_S16 && format != DABGPU_IQ_U8))
        return fail(DABGPU_E_ARG, "bad args");
    p->iq_fmt = format;
    return 0;
}
int dabgpu_pipe_set_dabplus_compact(dabgpu_pipe *p, int on) {
    if (!p) return fail(DABGPU_E_ARG, "bad args");
    p->dp.compact = on != 0;
    return 0;
}
int dabgpu_pipe_fetch(dabgpu_pipe *p, void *dst_h, const void *src_d, size_t bytes) {
    if (!p || (bytes && (!dst_h || !src_d))) return fail(DABGPU_E_ARG, "bad args");
    if (p->run_idx == 0) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run to fetch from");
    if (!bytes) return 0;
    // on the last run's back-end stream, behind its channel decoding (and DAB+ layer)
    // (the runtime's copy is a blit kernel on this runtime; queued on a high-priority
    // stream of its own it delivered 10 % less -- it then takes wave slots from the next
    // run's ACS: profiles/r04_delivered_ab.txt)
    hipStream_t bs = p->back[p->cur].stream;
    // into pinned host memory the device can address (dabgpu_host_alloc), 16-byte
    // aligned: k_to_host's few waves; otherwise the runtime's copy
    static const int wgs = [] { const char *e = getenv("DABGPU_D2H_WGS"); return e ? atoi(e) : 4; }();
    void *dd = nullptr;
    if (wgs > 0 && !((((uintptr_t)dst_h | (uintptr_t)src_d | bytes) & 15)) &&
        hipHostGetDevicePointer(&dd, dst_h, 0) == hipSuccess && dd)
        HIPCHK(launch_to_host(bs, src_d, dd, bytes, wgs));
    else {
        (void)hipGetLastError();                  // a refused device-pointer query is not an error here
        HIPCHK(hipMemcpyAsync(dst_h, src_d, bytes, hipMemcpyDeviceToHost, bs));
    }
    // no ev_back record: the copy reads only this run's outputs, which the next run on
    // this stream (the run after next) overwrites in stream order; the front end of that
    // run does not wait for it
    return 0;
}
int dabgpu_pipe_set_display(dabgpu_pipe *p, int on) {
    if (!p) return fail(DABGPU_E_ARG, "bad args");
    if (on && !p->disp_d) {
        HIPCHK(hipStreamSynchronize(p->c->stream));
        HIPCHK(p->disp_d.zalloc((size_t)p->S * p->R * K));
    }
    p->display = on != 0;
    return 0;
}
int dabgpu_pipe_set_display_token(dabgpu_pipe *p, int token) {
    if (!p || token < 1 || token > NSYM) return fail(DABGPU_E_ARG, "display token %d outside 1..75", token);
    p->disp_token = token;
    return 0;
}
int dabgpu_pipe_iq_display(dabgpu_pipe *p, int stream, int frame, float *carriers_h) {
    if (!p || !carriers_h || stream < 0 || stream >= p->S || frame < 0 || frame >= p->F)
        return fail(DABGPU_E_ARG, "bad args");
    if (!p->display || !p->disp_d) return fail(DABGPU_E_STATE, "display feed off (dabgpu_pipe_set_display)");
    const size_t i = (size_t)stream * p->F + frame;
    if (p->last_info.size() <= i || !p->last_info[i].committed)
        return fail(DABGPU_E_STATE, "stream %d frame %d was not decoded in the last run", stream, frame);
    const int32_t slot = p->last_frames[i].out_slot;
    HIPCHK(hipMemcpyAsync(carriers_h, p->disp_d + (size_t)slot * K, sizeof(float2) * K, hipMemcpyDeviceToHost,
                          p->c->stream));
    HIPCHK(hipStreamSynchronize(p->c->stream));
    return 0;
}
int dabgpu_pipe_frames(dabgpu_pipe *p, dabgpu_frame *fr, int32_t *si) {
    if (!p) return fail(DABGPU_E_ARG, "bad args");
    if (fr) memcpy(fr, p->last_frames.data(), sizeof(dabgpu_frame) * p->last_frames.size());
    if (si) for (size_t i = 0; i < p->last_info.size(); i++) si[i] = p->last_info[i].start_index;
    return 0;
}

}  // extern "C"
