// dabgpu_pipe.cpp -- the C ABI (include/dabgpu.h), second half: the streaming pipeline that replaces
// ofdmProcessor::run + ficHandler + mscHandler for many ensembles at once (its receiver logic: front_replay.h)
#include <cstdlib>
#include <cstring>
#include <memory>
#include <algorithm>
#include "dabgpu_internal.h"
#include "front_replay.h"

using namespace dab;
using front::StreamSt;

// Channel decoding (FIC/MSC Viterbi, DAB+) of run r runs on back-end stream back[r & 1], so
// run r's back end overlaps run r+1's front end AND run r+1's back end (whose first waves
// fill the SIMDs run r's last Viterbi waves leave idle).  The ring holds 2F+4 frames per
// stream so run r+1's demod and MSC never touch a slot run r's MSC still reads; run r+2's
// front end waits for run r's ACS.  The caller gives consecutive runs different output
// buffers (or syncs).
//
// Destruction order, for every struct below: members go in reverse order of declaration, so
// each struct declares its stream last and dabgpu_pipe declares `back` and `acq` after its
// buffers -- a stream has drained and gone before the memory its kernels used is freed.
struct BackSlot {
    DevBuf<uint32_t> dec;            // Viterbi decisions: the MSC's, then the FIC's
    Event ev_copy;                   // the descriptor block's upload done (before its staging is reused)
    Event ev_back;                   // the run's back end done
    Event ev_acs;                    // the run's ACS done (the ring's last reader)
    Stream stream;
};
// Background null search (DABGPU_CTL_ACQ_ASYNC, the default since round 6): a stream that
// loses sync after an acquisition is searched on its own low-priority stream while the
// others keep decoding; its results are taken by the first dabgpu_pipe_run after they arrive
struct AcqBg {
    bool async = false;              // set true by dabgpu_pipe_create
    bool inflight = false;           // results pending (the event alone says recorded, not taken)
    Event ev;
    DevBuf<AcqJob> jobs_d;           // [S], and its pinned staging
    PinBuf<AcqJob> h_jobs;
    DevBuf<AcqResult> res_d;         // [S]
    PinBuf<AcqResult> h_res;
    std::vector<int> who;
    std::vector<char> acquiring;                     // [S]
    Stream stream;
};
// DAB+ superframe layer (mp4Processor per DAB+ subchannel and stream)
struct DabPlus {
    int max_rs = 0;
    // compact superframe output (dabgpu_pipe_set_dabplus_compact): the layer decodes into
    // this sparse scratch and stores the run's superframes in CIF order for the caller
    bool compact = false;
    DevBuf<uint8_t> sf_sparse_d;
    DevBuf<int32_t> sub_d;
    DevBuf<int16_t> br_d;
    DevBuf<int64_t> since_d;      // [S][NDP]
    DevBuf<uint8_t> ring_d;       // [S][NDP][120*DP_MAX_RS]
    DevBuf<DpState> state_d;      // [S][NDP]
    DevBuf<uint8_t> code_d;       // [S][NDP][4F] superframe verdict per candidate CIF
    Event ev;                     // the last superframe pass
};
// MPEG layer II layer (mp2Processor per classic-audio subchannel and stream): allocated only
// for a pipeline with caps.max_mp2 > 0
struct Mp2Layer {
    int fstride = 0;              // bytes per frame slot: 2 * 24 * max_bitrate bits
    DevBuf<int32_t> sub_d;
    DevBuf<int16_t> br_d;
    DevBuf<int64_t> since_d;      // [S][NMP]
    DevBuf<Mp2SyncState> sync_d;  // [S][NMP] the synchronisers
    DevBuf<uint8_t> part_d;       // [S][NMP][fstride] their frames in progress
    DevBuf<int16_t> vstate_d[2];  // [S][NMP][MP2_STATE_I16] the decoders: a pass reads [cur], writes [cur ^ 1]
    int cur = 0;
    DevBuf<uint8_t> frames_d;     // [S * NMP][4F][fstride] the frames that completed in the run
    DevBuf<uint8_t> present_d;    // [S * NMP][4F]
    Event ev;                     // the last pass
};
// Packet-mode data layer (an mscDatagroup's assembler per packet-mode subchannel and stream):
// allocated only while dabgpu_pipe_packet_caps' max_packet > 0
struct PacketLayer {
    int cap = 0, ncell = 0;       // max_group_bytes; cells per CIF the buffers hold (max_bitrate / 8)
    DevBuf<int32_t> sub_d;
    DevBuf<int16_t> br_d;
    DevBuf<int64_t> since_d;      // [S][NPK]
    DevBuf<PkState> state_d;      // [S][NPK] the assemblers
    DevBuf<uint8_t> carry_d[2];   // [S][NPK][cap] their series in flight: a pass reads [cur], writes [cur ^ 1]
    int cur = 0;
    DevBuf<uint32_t> rec_d;       // [S * NPK][4F][ncell] packet records of the run
    DevBuf<int2> take_d;          // [S * NPK][4F][ncell]
    DevBuf<int32_t> segtab_d;     // [S * NPK][1 + 4F * ncell]
    Event ev;                     // the last pass
};

// MOT layer (a motHandler per packet entry flagged DABGPU_SUBCH_MOT and stream): allocated
// only while dabgpu_pipe_mot_caps' max_mot > 0
struct MotLayer {
    int body = 0, body_cap = 0;   // max_body_bytes, and rounded up to 16
    size_t state_bytes = 0;       // dabgpu_mot_state_bytes(body)
    int gslots = 0;               // DABGPU_PKT_GROUP_SLOTS(F, max_bitrate)
    DevBuf<uint8_t> state_d;      // [S][NMOT][state_bytes] the motHandlers, updated in place
    DevBuf<int32_t> src_d;        // [S][NMOT] the packet slot (s * NPK + j) each reads, -1: absent
    DevBuf<int4> ops_d;           // [S * NMOT][2 * gslots] the pass's copy list
    DevBuf<int32_t> nops_d;       // [S * NMOT]
    Event ev;                     // the last pass
};

// PAD layer (a padHandler per DAB+ entry flagged DABGPU_SUBCH_PAD and stream): allocated only
// while dabgpu_pipe_pad_caps' max_pad > 0
struct PadLayer {
    DevBuf<uint8_t> state_d;      // [S][NPAD] PadState, the padHandlers, updated in place
    DevBuf<int32_t> src_d;        // [S][NPAD] the DAB+ slot (s * NDP + j) each reads, -1: absent
    Event ev;                     // the last pass
};

// FIC layer (a fib_processor's database per stream): allocated only while dabgpu_pipe_fic_caps is on
struct FicLayer {
    DevBuf<uint8_t> db_d;         // [S] dabgpu_fic_db, updated in place
    Event ev;                     // the last pass
    bool on = false;
};

struct dabgpu_pipe {
    dabgpu_ctx *c = nullptr;
    int S = 0, F = 0, NSUB = 0, R = 0, NDP = 0, NMP = 0, NPK = 0, NMOT = 0, NPAD = 0;
    int16_t threshold = 3;
    int16_t method = 1;              // freqSyncMethod
    bool scan = false;               // scanMode (No_Signal_Found after > 5 attempts)
    // Subchannel tables, one per stream (dabgpu_pipe_set_subch): NSUB = caps.max_subch output
    // rows and NDP = caps.max_dabplus DAB+ slots per stream, whatever the tables hold.
    // since[s][k]: the stream's cif_count when entry k was set (it delivers from since + 16).
    std::vector<std::vector<dabgpu_subch>> tab;
    std::vector<std::vector<int64_t>> since;
    int max_bitrate = 0, max_nbits = 0;
    // uniform: every stream has the same full table (NSUB entries, since 0) -- the kernels
    // take the shared-table path (VitJob::ent_prof null); else the per-(stream, entry)
    // descriptor tables below and the list of active pairs (rebuild_tables)
    bool uniform = true;
    int n_act = 0;
    DevBuf<int32_t> ent_prof_d, ent_start_d, act_d;
    DevBuf<int64_t> ent_since_d;
    std::vector<uint8_t> entry_valid;   // [S][4F][NSUB] of the last run (dabgpu_pipe_msc_entry_valid)
    std::vector<StreamSt> st;
    DevBuf<uint8_t> ring;            // [S][R][75][3072] RING8 bytes (soft bit + 127, dab_kernels.h)
    DevBuf<Profile> prof_d;          // [NSUB]
    DevBuf<Profile> ficprof_d;
    DevBuf<uint8_t> inv_d;           // the subchannel profiles' inverse depuncturing tables
    DevBuf<int32_t> substart_d;      // [NSUB]
    DevBuf<dabgpu_frame> frames_d;
    DevBuf<int32_t> si_d;
    DevBuf<int16_t> corr_d, snr_d;
    DevBuf<float> fc_d, fcpart_d;    // [S*F] float2, [S*F][kMaxChunks] float2
    // the back end's per-run descriptors, one block per back-end stream (parity), uploaded
    // with ONE copy per run (each runtime copy is a kernel of its own on the back-end
    // stream, ~6 us, in front of the ACS): [S] int64 CIF index of each stream's first CIF
    // slot | [S] int32 CIFs each stream delivered | [S * F] int32 FIC ring slots;
    // h_desc: their pinned staging, BackSlot::ev_copy marks the upload done before reuse
    DevBuf<uint8_t> desc_d;
    PinBuf<uint8_t> h_desc;
    size_t desc_sz = 0;
    int64_t *cif0_dev(int par) const { return (int64_t *)(desc_d + par * desc_sz); }
    int32_t *ncif_dev(int par) const { return (int32_t *)(desc_d + par * desc_sz + 8 * (size_t)S); }
    int32_t *slots_dev(int par) const { return (int32_t *)(desc_d + par * desc_sz + 12 * (size_t)S); }
    int64_t *h_cif0(int par) const { return (int64_t *)(h_desc + par * desc_sz); }
    int32_t *h_ncif(int par) const { return (int32_t *)(h_desc + par * desc_sz + 8 * (size_t)S); }
    int32_t *h_slots(int par) const { return (int32_t *)(h_desc + par * desc_sz + 12 * (size_t)S); }
    int cur = 0;                     // back-end stream of the last run
    int64_t run_idx = 0;
    int64_t dec_fic_off = 0;         // FIC decisions: words after the MSC's
    // pinned host staging of the front end's per-pass copies (frame descriptors in,
    // startIndex / FreqCorr out): DMA without the pageable bounce, each pass syncs
    // before the buffers are touched again
    PinBuf<dabgpu_frame> h_frames;
    PinBuf<int32_t> h_si;
    PinBuf<float2> h_fc;
    PinBuf<int16_t> h_snr;
    // the back-end streams' own error words (the front end's is the context's): the
    // Viterbi jobs of run r set berr_d[r & 1], which the back end publishes into
    // h_berr[r & 1] (and clears) as its last step; read once back[r & 1].ev_back completed
    DevBuf<int32_t> berr_d;
    PinBuf<int32_t> h_berr;
    // speculative back end (dabgpu_pipe_run): queued behind the first front pass
    bool speculate = true;                      // env DABGPU_NO_SPECULATE=1: off (A/B)
    Event ev_front;
    bool ev_front_demod = false;     // ev_front marks this pass's demod (the speculative back end's gate)
    std::vector<dabgpu_frame> last_frames;   // [S][F]
    std::vector<dabgpu_frame_info> last_info;   // [S][F] observables of the last run
    DabPlus dp;
    Mp2Layer mp2;
    PacketLayer pk;
    MotLayer mot;
    // the outputs of the run's dabgpu_pipe_packet call, which dabgpu_pipe_mot reads
    const uint8_t *pk_bytes = nullptr;
    const dabgpu_datagroup *pk_groups = nullptr;
    const dabgpu_packet_run *pk_run = nullptr;
    bool mot_pending = false;        // ... have not entered the MOT layer yet
    PadLayer pad;
    // the outputs of the run's dabgpu_pipe_dabplus call, which dabgpu_pipe_pad reads
    const uint8_t *dp_sf = nullptr;
    const dabgpu_superframe *dp_info = nullptr;
    int32_t dp_sf_stride = 0;
    bool dp_sf_compact = false;
    bool pad_pending = false;        // ... have not entered the PAD layer yet
    FicLayer fic;
    // the FIC outputs of the last run, which dabgpu_pipe_fic reads
    const uint8_t *last_fic = nullptr, *last_crc = nullptr;
    bool last_fic_packed = false;
    bool fic_pending = false;        // ... have not entered the FIC layer yet
    const uint8_t *last_msc = nullptr; // MSC bits of the last run
    bool dp_pending = false, mp2_pending = false, pk_pending = false;   // the last run's CIFs have not entered the layer yet
    int32_t last_msc_stride = 0;
    bool last_msc_packed = false;
    // the iqBuffer feed (dabgpu_pipe_set_display): symbol 2's display carriers per ring slot
    DevBuf<float2> disp_d;           // [S][R][K]
    bool display = false;
    int disp_token = 2;              // the display feed's symbol (ofdm-decoder.cpp:61 displayToken)
    bool packed = false;             // MSC output 8 bits per byte (dabgpu_pipe_set_packed)
    bool fic_packed = false;         // FIC output as FIB bytes (DABGPU_PACK_FIC)
    int iq_fmt = DABGPU_IQ_F32;      // sample format of the streams (dabgpu_pipe_set_iq_format)
    // fault injection (DABGPU_CTL_INJECT_BOUNDS): the next run's MSC job gets a subchannel
    // table whose first entry points past the ring, which the Viterbi loader refuses
    bool inject_bounds = false;
    DevBuf<int32_t> substart_bad_d;
    // optional per-stage kernel timing (HIP events on the stage's stream)
    int profiling = 0;                          // 1: last run, 2: every run since enabled, 3: 2 + stages alone
    std::vector<Event> ev_pool;
    std::vector<std::pair<int, int>> ev_rec;   // (stage, index of start event; end = +1)
    // the streams (of the back ends and the background null search) after every buffer above
    BackSlot back[2];
    AcqBg acq;
    ~dabgpu_pipe() {                 // the front end's stream is the context's: wait for it here
        if (c) (void)c->stream.sync();
        for (BackSlot &b : back) (void)b.stream.sync();
        (void)acq.stream.sync();     // a background null search still running
    }
};

static hipError_t prof_mark(dabgpu_pipe *p, int stage, bool start) {
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

// wait for everything the pipeline has enqueued on its front-end and back-end streams
static int sync_streams(dabgpu_pipe *p) {
    HIPCHK(p->c->stream.sync());
    for (BackSlot &b : p->back) HIPCHK(b.stream.sync());
    return 0;
}

// the streams a control call names: [first, end) -- one stream, or every stream for -1
static std::pair<int, int> stream_range(const dabgpu_pipe *p, int stream) {
    return stream < 0 ? std::make_pair(0, p->S) : std::make_pair(stream, stream + 1);
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

// A subchannel table against the reference's definitions and the pipeline's caps
// (dabgpu_pipe_create_caps and dabgpu_pipe_set_subch validate alike)
static int check_table(const dabgpu_subch *sub, int n, int max_subch, int max_bitrate, int max_dabplus, int max_mp2,
                       int max_packet, int max_mot, int max_pad) {
    if (n < 0 || (n > 0 && !sub)) return fail(DABGPU_E_ARG, "bad subchannel table");
    if (n > max_subch) return fail(DABGPU_E_ARG, "%d subchannels, the pipeline holds %d per stream", n, max_subch);
    int ndp = 0, nmp = 0, npk = 0, nmot = 0, npad = 0;
    for (int i = 0; i < n; i++) {
        Profile P;
        if (sub[i].flags & DABGPU_SUBCH_PAD) {
            if (!(sub[i].flags & DABGPU_SUBCH_DABPLUS)) return fail(DABGPU_E_ARG, "subchannel %d is flagged PAD and not DAB+", i);
            npad++;
        }
        if (sub[i].flags & DABGPU_SUBCH_MOT) {
            if (!(sub[i].flags & DABGPU_SUBCH_PACKET))
                return fail(DABGPU_E_ARG, "subchannel %d is flagged MOT and not packet mode", i);
            nmot++;
        }
        if (make_profile(sub[i], P)) return fail(DABGPU_E_UNSUP, "subchannel %d protection undefined", i);
        if (sub[i].startAddr < 0 || sub[i].startAddr + sub[i].length > 864 || P.frag > sub[i].length * 64)
            return fail(DABGPU_E_ARG, "subchannel %d does not fit its CUs", i);
        // packets are multiples of 24 bytes: a CIF of 3 * bitRate bytes holds bitRate / 8 cells
        if ((sub[i].flags & DABGPU_SUBCH_PACKET) && (sub[i].bitRate < 8 || sub[i].bitRate % 8 || sub[i].bitRate > max_bitrate))
            return fail(DABGPU_E_UNSUP, "packet-mode subchannel %d: bitRate %d is not a multiple of 8 in [8, %d]", i,
                        sub[i].bitRate, max_bitrate);
        if (sub[i].bitRate > max_bitrate)
            return fail(DABGPU_E_ARG, "subchannel %d: bitRate %d above the pipeline's %d", i, sub[i].bitRate, max_bitrate);
        if ((sub[i].flags & DABGPU_SUBCH_MP2) && (sub[i].flags & DABGPU_SUBCH_DABPLUS))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged both DAB+ and layer II", i);
        if (sub[i].flags & DABGPU_SUBCH_MP2) nmp++;
        if (sub[i].flags & DABGPU_SUBCH_PACKET) {
            if (sub[i].flags & (DABGPU_SUBCH_MP2 | DABGPU_SUBCH_DABPLUS))
                return fail(DABGPU_E_ARG, "subchannel %d is flagged packet mode and an audio layer", i);
            npk++;
        }
        if (!(sub[i].flags & DABGPU_SUBCH_DABPLUS)) continue;
        // DAB+ subchannels (mp4Processor: RSDims = bitRate / 8, mp4processor.cpp:83-84)
        const int br = sub[i].bitRate;
        if (br < 8 || br % 8 || br / 8 > DP_MAX_RS)
            return fail(DABGPU_E_UNSUP, "DAB+ subchannel %d: bitRate %d is not a multiple of 8 in [8, 384]", i, br);
        ndp++;
    }
    if (ndp > max_dabplus) return fail(DABGPU_E_ARG, "%d DAB+ subchannels, the pipeline holds %d per stream", ndp, max_dabplus);
    if (nmp > max_mp2) return fail(DABGPU_E_ARG, "%d layer II subchannels, the pipeline holds %d per stream", nmp, max_mp2);
    if (npk > max_packet)
        return fail(DABGPU_E_ARG, "%d packet-mode subchannels, the pipeline holds %d per stream", npk, max_packet);
    if (nmot > max_mot) return fail(DABGPU_E_ARG, "%d MOT subchannels, the pipeline holds %d per stream", nmot, max_mot);
    if (npad > max_pad) return fail(DABGPU_E_ARG, "%d PAD subchannels, the pipeline holds %d per stream", npad, max_pad);
    return 0;
}

static bool same_subch(const dabgpu_subch &a, const dabgpu_subch &b) {
    return a.startAddr == b.startAddr && a.length == b.length && a.bitRate == b.bitRate && a.protLevel == b.protLevel &&
           a.uepFlag == b.uepFlag && a.flags == b.flags;
}

// (Re)size the packet-mode layer to npk slots per stream and groups of cap bytes.  The
// assemblers of the slots both sizes hold go on (their carried bytes cut or padded to cap),
// every other slot is a new mscDatagroup.  The caller has waited for the streams.  The new
// layer is built beside the old one and takes its place only when everything succeeded: on
// an error the pipeline keeps the layer, and the assemblers, it had.
static int packet_size(dabgpu_pipe *p, int npk, int cap) {
    const PacketLayer &old = p->pk;
    const int S = p->S, old_n = p->NPK, old_cap = old.cap;
    std::vector<PkState> ost;
    std::vector<uint8_t> oca;
    if (old_n) {
        ost.resize((size_t)S * old_n);
        oca.resize((size_t)S * old_n * old_cap);
        HIPCHK(hipMemcpy(ost.data(), old.state_d, sizeof(PkState) * ost.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(oca.data(), old.carry_d[old.cur], oca.size(), hipMemcpyDeviceToHost));
    }
    PacketLayer k;
    if (!npk) {
        p->pk = std::move(k);
        p->NPK = 0;
        return 0;
    }
    k.cap = cap;
    k.ncell = std::max(1, p->max_bitrate / 8);
    const size_t ne = (size_t)S * npk, cells = (size_t)4 * p->F * k.ncell;
    HIPCHK(k.ev.create(hipEventDisableTiming));
    HIPCHK(k.sub_d.alloc(ne));
    HIPCHK(k.br_d.alloc(ne));
    HIPCHK(k.since_d.alloc(ne));
    HIPCHK(k.state_d.alloc(ne));
    HIPCHK(k.rec_d.alloc(ne * cells));
    HIPCHK(k.take_d.alloc(ne * cells));
    HIPCHK(k.segtab_d.alloc(ne * (1 + cells)));
    for (auto &c : k.carry_d) HIPCHK(c.alloc(ne * cap));
    std::vector<PkState> st(ne, PkState{0, -1, 0, 0, 0, 0, 0, 0});
    std::vector<uint8_t> ca(ne * cap, 0);
    for (int s = 0; s < S; s++)
        for (int j = 0; j < std::min(old_n, npk); j++) {
            st[(size_t)s * npk + j] = ost[(size_t)s * old_n + j];
            memcpy(ca.data() + ((size_t)s * npk + j) * cap, oca.data() + ((size_t)s * old_n + j) * old_cap, std::min(cap, old_cap));
        }
    HIPCHK(hipMemcpy(k.state_d, st.data(), sizeof(PkState) * ne, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.carry_d[0], ca.data(), ca.size(), hipMemcpyHostToDevice));
    p->pk = std::move(k);
    p->NPK = npk;
    return 0;
}

// (Re)size the MOT layer to nmot slots per stream and bodies of at most body bytes, as
// packet_size does: the motHandlers of the slots both sizes hold go on (an entry whose body no
// longer fits is flagged DABGPU_MOT_TOO_LARGE), every other slot is a new one; the new layer
// takes the old one's place only when everything succeeded.
static int mot_size(dabgpu_pipe *p, int nmot, int body) {
    const MotLayer &old = p->mot;
    const int S = p->S, old_n = p->NMOT;
    std::vector<uint8_t> ost;
    if (old_n) {
        ost.resize((size_t)S * old_n * old.state_bytes);
        HIPCHK(hipMemcpy(ost.data(), old.state_d, ost.size(), hipMemcpyDeviceToHost));
    }
    MotLayer m;
    if (!nmot) {
        p->mot = std::move(m);
        p->NMOT = 0;
        return 0;
    }
    m.body = body;
    m.body_cap = (body + 15) / 16 * 16;
    m.state_bytes = dabgpu_mot_state_bytes(body);
    m.gslots = DABGPU_PKT_GROUP_SLOTS(p->F, p->max_bitrate);
    const size_t ne = (size_t)S * nmot;
    HIPCHK(m.ev.create(hipEventDisableTiming));
    HIPCHK(m.state_d.alloc(ne * m.state_bytes));
    HIPCHK(m.src_d.alloc(ne));
    HIPCHK(m.ops_d.alloc(std::max<size_t>(1, ne * 2 * m.gslots)));
    HIPCHK(m.nops_d.alloc(ne));
    std::vector<uint8_t> st(ne * m.state_bytes, 0);
    for (int s = 0; s < S; s++)
        for (int j = 0; j < std::min(old_n, nmot); j++) {
            const uint8_t *o = ost.data() + ((size_t)s * old_n + j) * old.state_bytes;
            uint8_t *n = st.data() + ((size_t)s * nmot + j) * m.state_bytes;
            memcpy(n, o, MOT_TABLE_BYTES);
            auto *e = (dabgpu_mot_entry *)(n + sizeof(dabgpu_mot_head));
            for (int k = 0; k < DABGPU_MOT_ENTRIES; k++) {
                if (!e[k].order || (e[k].flags & DABGPU_MOT_TOO_LARGE)) continue;
                if (e[k].bodySize > body) {
                    e[k].flags |= DABGPU_MOT_TOO_LARGE;
                    continue;
                }
                memcpy(n + MOT_TABLE_BYTES + (size_t)k * m.body_cap, o + MOT_TABLE_BYTES + (size_t)k * old.body_cap,
                       (size_t)std::max(0, e[k].bodySize));
            }
        }
    HIPCHK(hipMemcpy(m.state_d, st.data(), st.size(), hipMemcpyHostToDevice));
    p->mot = std::move(m);
    p->NMOT = nmot;
    return 0;
}

// (Re)size the PAD layer to npad slots per stream, as mot_size does: the padHandlers of the
// slots both sizes hold go on, every other slot is a new one.
static int pad_size(dabgpu_pipe *p, int npad) {
    const PadLayer &old = p->pad;
    const int S = p->S, old_n = p->NPAD;
    std::vector<uint8_t> ost;
    if (old_n) {
        ost.resize((size_t)S * old_n * sizeof(PadState));
        HIPCHK(hipMemcpy(ost.data(), old.state_d, ost.size(), hipMemcpyDeviceToHost));
    }
    PadLayer m;
    if (!npad) {
        p->pad = std::move(m);
        p->NPAD = 0;
        return 0;
    }
    const size_t ne = (size_t)S * npad;
    HIPCHK(m.ev.create(hipEventDisableTiming));
    HIPCHK(m.state_d.alloc(ne * sizeof(PadState)));
    HIPCHK(m.src_d.alloc(ne));
    std::vector<uint8_t> st(ne * sizeof(PadState), 0);
    for (int s = 0; s < S; s++)
        for (int j = 0; j < std::min(old_n, npad); j++)
            memcpy(st.data() + ((size_t)s * npad + j) * sizeof(PadState), ost.data() + ((size_t)s * old_n + j) * sizeof(PadState),
                   sizeof(PadState));
    HIPCHK(hipMemcpy(m.state_d, st.data(), st.size(), hipMemcpyHostToDevice));
    p->pad = std::move(m);
    p->NPAD = npad;
    return 0;
}

// The device's descriptor tables from p->tab / p->since.  The caller has waited for the
// pipeline's streams (in-flight kernels read the old tables): the tables are replaced.
static int rebuild_tables(dabgpu_pipe *p) {
    const int S = p->S, NS = p->NSUB;
    p->uniform = true;
    for (int s = 0; s < S && p->uniform; s++) {
        if ((int)p->tab[s].size() != NS) p->uniform = false;
        for (int k = 0; k < (int)p->tab[s].size() && p->uniform; k++)
            if (p->since[s][k] != 0 || !same_subch(p->tab[s][k], p->tab[0][k])) p->uniform = false;
    }
    std::vector<Profile> profs;
    std::vector<uint8_t> inv;
    std::vector<int32_t> ss(std::max(1, NS), 0);
    std::vector<int32_t> eprof(std::max<size_t>(1, (size_t)S * NS), -1), estart(eprof.size(), 0), act;
    std::vector<int64_t> esince(eprof.size(), 0);
    auto add_profile = [&](const dabgpu_subch &sc, bool dedup) {
        Profile P;
        (void)make_profile(sc, P);                      // validated by check_table
        if (dedup)
            for (size_t i = 0; i < profs.size(); i++) {
                Profile Q = profs[i];
                Q.inv_off = 0;
                if (!memcmp(&Q, &P, sizeof P)) return (int32_t)i;
            }
        profs.push_back(P);
        profs.back().inv_off = (int32_t)inv.size();
        const std::vector<uint8_t> v = make_inv(P);
        inv.insert(inv.end(), v.begin(), v.end());
        return (int32_t)profs.size() - 1;
    };
    if (p->uniform) {                                   // profile k = entry k, as the kernels index it
        for (int k = 0; k < NS; k++) {
            add_profile(p->tab[0][k], false);
            ss[k] = p->tab[0][k].startAddr * 64;
        }
        p->n_act = S * NS;
    } else {
        // distinct profiles (and their inverse tables) once, whatever streams use them
        for (int s = 0; s < S; s++)
            for (int k = 0; k < (int)p->tab[s].size(); k++) {
                const size_t e = (size_t)s * NS + k;
                eprof[e] = add_profile(p->tab[s][k], true);
                estart[e] = p->tab[s][k].startAddr * 64;
                esince[e] = p->since[s][k];
                act.push_back((int32_t)e);
            }
        p->n_act = (int)act.size();
    }
    if (profs.empty()) profs.push_back(Profile());
    if (inv.empty()) inv.push_back(0);
    if (act.empty()) act.push_back(0);
    // DAB+ slots: slot j of a stream is its j-th entry flagged DABGPU_SUBCH_DABPLUS
    const size_t nd = std::max<size_t>(1, (size_t)S * p->NDP);
    std::vector<int32_t> dps(nd, -1);
    std::vector<int16_t> dpb(nd, 0);
    std::vector<int64_t> dpc(nd, 0);
    p->dp.max_rs = 0;
    for (int s = 0; s < S; s++) {
        int j = 0;
        for (int k = 0; k < (int)p->tab[s].size(); k++) {
            if (!(p->tab[s][k].flags & DABGPU_SUBCH_DABPLUS)) continue;
            const size_t i = (size_t)s * p->NDP + j++;
            dps[i] = k;
            dpb[i] = p->tab[s][k].bitRate;
            dpc[i] = p->since[s][k];
            p->dp.max_rs = std::max(p->dp.max_rs, p->tab[s][k].bitRate / 8);
        }
    }
    // put() replaces a table; the per-entry tables of a non-uniform set and the injected
    // table go (an empty buffer is assigned) and are built again when needed
    HIPCHK(p->prof_d.put(profs));
    HIPCHK(p->inv_d.put(inv));
    HIPCHK(p->substart_d.put(ss));
    p->ent_prof_d = {};
    p->ent_start_d = {};
    p->ent_since_d = {};
    p->act_d = {};
    p->substart_bad_d = {};
    if (!p->uniform) {
        HIPCHK(p->ent_prof_d.put(eprof));
        HIPCHK(p->ent_start_d.put(estart));
        HIPCHK(p->ent_since_d.put(esince));
        HIPCHK(p->act_d.put(act));
    }
    if (p->NMP) {                 // layer II slots: slot j of a stream is its j-th entry flagged DABGPU_SUBCH_MP2
        const size_t nm = (size_t)S * p->NMP;
        std::vector<int32_t> ms(nm, -1);
        std::vector<int16_t> mb(nm, 0);
        std::vector<int64_t> mc(nm, 0);
        for (int s = 0; s < S; s++)
            for (int k = 0, j = 0; k < (int)p->tab[s].size(); k++) {
                if (!(p->tab[s][k].flags & DABGPU_SUBCH_MP2)) continue;
                const size_t i = (size_t)s * p->NMP + j++;
                ms[i] = k;
                mb[i] = p->tab[s][k].bitRate;
                mc[i] = p->since[s][k];
            }
        HIPCHK(hipMemcpy(p->mp2.sub_d, ms.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->mp2.br_d, mb.data(), sizeof(int16_t) * nm, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->mp2.since_d, mc.data(), sizeof(int64_t) * nm, hipMemcpyHostToDevice));
    }
    if (p->NPK) {                 // packet slots: slot j of a stream is its j-th entry flagged DABGPU_SUBCH_PACKET
        const size_t nk = (size_t)S * p->NPK;
        std::vector<int32_t> ks(nk, -1);
        std::vector<int16_t> kb(nk, 0);
        std::vector<int64_t> kc(nk, 0);
        for (int s = 0; s < S; s++)
            for (int k = 0, j = 0; k < (int)p->tab[s].size(); k++) {
                if (!(p->tab[s][k].flags & DABGPU_SUBCH_PACKET)) continue;
                const size_t i = (size_t)s * p->NPK + j++;
                ks[i] = k;
                kb[i] = p->tab[s][k].bitRate;
                kc[i] = p->since[s][k];
            }
        HIPCHK(hipMemcpy(p->pk.sub_d, ks.data(), sizeof(int32_t) * nk, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->pk.br_d, kb.data(), sizeof(int16_t) * nk, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->pk.since_d, kc.data(), sizeof(int64_t) * nk, hipMemcpyHostToDevice));
    }
    if (p->NMOT) {                // MOT slots: slot m of a stream is its m-th entry flagged DABGPU_SUBCH_MOT
        std::vector<int32_t> src((size_t)S * p->NMOT, -1);
        for (int s = 0; s < S; s++)
            for (int k = 0, j = 0, m = 0; k < (int)p->tab[s].size(); k++) {
                if (!(p->tab[s][k].flags & DABGPU_SUBCH_PACKET)) continue;
                if (p->tab[s][k].flags & DABGPU_SUBCH_MOT) src[(size_t)s * p->NMOT + m++] = s * p->NPK + j;
                j++;
            }
        HIPCHK(hipMemcpy(p->mot.src_d, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice));
    }
    if (p->NPAD) {                // PAD slots: slot m of a stream is its m-th entry flagged DABGPU_SUBCH_PAD
        std::vector<int32_t> src((size_t)S * p->NPAD, -1);
        for (int s = 0; s < S; s++)
            for (int k = 0, j = 0, m = 0; k < (int)p->tab[s].size(); k++) {
                if (!(p->tab[s][k].flags & DABGPU_SUBCH_DABPLUS)) continue;
                if (p->tab[s][k].flags & DABGPU_SUBCH_PAD) src[(size_t)s * p->NPAD + m++] = s * p->NDP + j;
                j++;
            }
        HIPCHK(hipMemcpy(p->pad.src_d, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice));
    }
    if (p->NDP) {
        HIPCHK(hipMemcpy(p->dp.sub_d, dps.data(), sizeof(int32_t) * nd, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->dp.br_d, dpb.data(), sizeof(int16_t) * nd, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->dp.since_d, dpc.data(), sizeof(int64_t) * nd, hipMemcpyHostToDevice));
    }
    return 0;
}

int dabgpu_pipe_create(dabgpu_ctx *c, const dabgpu_pipe_cfg *cfg, dabgpu_pipe **out) {
    if (!c || !cfg || !out) return fail(DABGPU_E_ARG, "null arg");
    *out = nullptr;
    if (cfg->n_subch < 0 || (cfg->n_subch > 0 && !cfg->subch)) return fail(DABGPU_E_ARG, "bad sizes");
    // the caps of the table itself
    dabgpu_pipe_caps caps = {cfg->n_subch, 0, 0, 0};
    for (int i = 0; i < cfg->n_subch; i++) {
        caps.max_bitrate = std::max<int32_t>(caps.max_bitrate, cfg->subch[i].bitRate);
        if (cfg->subch[i].flags & DABGPU_SUBCH_DABPLUS) caps.max_dabplus++;
        if (cfg->subch[i].flags & DABGPU_SUBCH_MP2) caps.max_mp2++;
    }
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
    int npk = 0, nmot = 0, npad = 0;   // the packet-mode, MOT and PAD layers start with what the table flags (dabgpu_pipe_packet_caps)
    for (int i = 0; i < cfg->n_subch; i++) {
        if (cfg->subch[i].flags & DABGPU_SUBCH_PACKET) npk++;
        if (cfg->subch[i].flags & DABGPU_SUBCH_MOT) nmot++;
        if (cfg->subch[i].flags & DABGPU_SUBCH_PAD) npad++;
    }
    if (int rc = check_table(cfg->subch, cfg->n_subch, caps->max_subch, caps->max_bitrate, caps->max_dabplus, caps->max_mp2, npk,
                             nmot, npad))
        return rc;
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
        HIPCHK(p->dp.sub_d.alloc(nd));
        HIPCHK(p->dp.br_d.alloc(nd));
        HIPCHK(p->dp.since_d.alloc(nd));
        HIPCHK(p->dp.ring_d.alloc(nd * 120 * DP_MAX_RS));
        HIPCHK(p->dp.state_d.alloc(nd));
        HIPCHK(p->dp.code_d.alloc(nd * 4 * p->F));
        HIPCHK(hipMemset(p->dp.ring_d, 0, nd * 120 * DP_MAX_RS));
        HIPCHK(hipMemset(p->dp.state_d, 0, sizeof(DpState) * nd));
    }
    if (p->NMP) {
        Mp2Layer &m = p->mp2;
        const size_t nm = (size_t)p->S * p->NMP;
        m.fstride = 6 * std::max(p->max_bitrate, 1);
        HIPCHK(m.ev.create(hipEventDisableTiming));
        HIPCHK(m.sub_d.alloc(nm));
        HIPCHK(m.br_d.alloc(nm));
        HIPCHK(m.since_d.alloc(nm));
        HIPCHK(m.sync_d.alloc(nm));
        HIPCHK(m.part_d.alloc(nm * m.fstride));
        HIPCHK(m.frames_d.alloc(nm * 4 * p->F * m.fstride));
        HIPCHK(m.present_d.alloc(nm * 4 * p->F));
        HIPCHK(hipMemset(m.sync_d, 0, sizeof(Mp2SyncState) * nm));
        HIPCHK(hipMemset(m.part_d, 0, nm * m.fstride));
        for (auto &v : m.vstate_d) {
            HIPCHK(v.alloc(nm * MP2_STATE_I16));
            HIPCHK(hipMemset(v, 0, sizeof(int16_t) * nm * MP2_STATE_I16));
        }
    }
    if (npk)
        if (int rc = packet_size(p.get(), npk, DABGPU_PKT_GROUP_BYTES)) return rc;
    if (nmot)
        if (int rc = mot_size(p.get(), nmot, DABGPU_MOT_BODY_BYTES)) return rc;
    if (npad)
        if (int rc = pad_size(p.get(), npad)) return rc;
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
    p->last_msc = nullptr;
    p->fic_pending = false;
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
    p->last_msc = have_rows ? msc_bits : nullptr;
    p->dp_pending = p->mp2_pending = p->pk_pending = have_rows;
    p->mot_pending = false;                    // until this run's dabgpu_pipe_packet
    p->pad_pending = false;                    // until this run's dabgpu_pipe_dabplus
    p->last_fic = fic_bits;
    p->last_crc = fic_crc;
    p->last_fic_packed = p->fic_packed;
    p->fic_pending = fic_bits && fic_crc;
    p->last_msc_stride = msc_stride;
    p->last_msc_packed = p->packed;
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

int dabgpu_pipe_dabplus(dabgpu_pipe *p, uint8_t *sf_bytes, int32_t sf_stride, dabgpu_superframe *info) {
    if (!p || !sf_bytes || !info) return fail(DABGPU_E_ARG, "null arg");
    if (p->NDP == 0) return fail(DABGPU_E_STATE, "no DAB+ subchannel in this pipeline");
    if (!p->last_msc || !p->dp_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with MSC output to consume");
    if (sf_stride < 110 * p->dp.max_rs) return fail(DABGPU_E_ARG, "sf_stride %d < %d", sf_stride, 110 * p->dp.max_rs);
    dabgpu_ctx *c = p->c;
    DpJob J;
    memset(&J, 0, sizeof J);
    J.msc = p->last_msc;
    J.msc_stride = p->last_msc_stride;
    J.packed = p->last_msc_packed ? 1 : 0;
    J.ncif = 4 * p->F;
    J.nsub = p->NSUB;
    J.ndp = p->NDP;
    J.nstreams = p->S;
    J.cif0s = p->cif0_dev(p->cur);
    J.ncifs = p->ncif_dev(p->cur);
    J.dp_sub = p->dp.sub_d;
    J.dp_br = p->dp.br_d;
    J.dp_since = p->dp.since_d;
    J.ring = p->dp.ring_d;
    J.state = p->dp.state_d;
    J.code = p->dp.code_d;
    J.sf_out = sf_bytes;
    J.sf_stride = sf_stride;
    if (p->dp.compact) {
        if (p->F > 512) return fail(DABGPU_E_UNSUP, "compact DAB+ output: at most 512 frames per run");
        const size_t need = (size_t)p->S * 4 * p->F * p->NDP * (size_t)sf_stride;
        if (need > p->dp.sf_sparse_d.n) {
            // the layers that wrote the old scratch ran on this pipeline's back-end streams:
            // wait for those (not the whole device: other pipelines, the null search)
            for (BackSlot &b : p->back) HIPCHK(b.stream.sync());
            p->dp.sf_sparse_d.reset();
            HIPCHK(p->dp.sf_sparse_d.alloc(need));
        }
        J.sf_out = p->dp.sf_sparse_d;
        J.sf_compact = sf_bytes;
        J.kmax = DABGPU_SF_SLOTS(p->F);
    }
    J.info = info;
    J.tabs = c->dptab;
    // on the last run's back-end stream (after its MSC), after the previous
    // superframe pass (the 5-CIF rings carry state from run to run)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(p->dp.ev.wait_on(bs));
    HIPCHK(prof_mark(p, DABGPU_STAGE_DABPLUS, true));
    HIPCHK(launch_dabplus(bs, J));
    HIPCHK(prof_mark(p, DABGPU_STAGE_DABPLUS, false));
    HIPCHK(p->dp.ev.record(bs));
    // (the run after next does not wait for this: the layer reads this run's MSC output
    // and CIF counters, which that run's back end overwrites behind it on this stream)
    p->dp_pending = false;                     // each run's CIFs enter the superframe layer once
    p->dp_sf = sf_bytes;
    p->dp_info = info;
    p->dp_sf_stride = sf_stride;
    p->dp_sf_compact = p->dp.compact;
    p->pad_pending = p->NPAD > 0;
    return 0;
}

int dabgpu_pipe_pad(dabgpu_pipe *p, const uint8_t *sf_bytes, int32_t sf_stride, const dabgpu_superframe *info,
                    dabgpu_pad_label *labels, dabgpu_datagroup *groups, uint8_t *bytes, dabgpu_pad_run *run) {
    if (!p || !sf_bytes || !info || !labels || !groups || !bytes || !run) return fail(DABGPU_E_ARG, "null arg");
    if (p->NPAD == 0) return fail(DABGPU_E_STATE, "no PAD subchannel in this pipeline");
    if (!p->pad_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_dabplus call of this run to consume");
    if (sf_bytes != p->dp_sf || info != p->dp_info || sf_stride != p->dp_sf_stride)
        return fail(DABGPU_E_ARG, "sf_bytes_d, sf_stride and info_d are not those of this run's dabgpu_pipe_dabplus call");
    PadLayer &m = p->pad;
    PadJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S * p->NPAD;
    J.state = m.state_d;
    J.info = info;
    J.sf = sf_bytes;
    J.sf_stride = sf_stride;
    J.kmax = p->dp_sf_compact ? DABGPU_SF_SLOTS(p->F) : 0;
    J.ncif = 4 * p->F;
    J.ndp = p->NDP;
    J.src = m.src_d;
    J.labels = labels;
    J.label_slots = DABGPU_PAD_LABEL_SLOTS(p->F);
    J.groups = groups;
    J.group_slots = DABGPU_PAD_GROUP_SLOTS(p->F);
    J.bytes = bytes;
    J.arena = DABGPU_PAD_ARENA_BYTES((int64_t)p->F);
    J.run = run;
    // on the run's back-end stream, behind its DAB+ layer; after the previous pass (the
    // padHandlers are updated in place)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(m.ev.wait_on(bs));
    HIPCHK(launch_pad(bs, J));
    HIPCHK(m.ev.record(bs));
    p->pad_pending = false;                    // each run's AUs enter the layer once
    return 0;
}

int dabgpu_pipe_pad_caps(dabgpu_pipe *p, int max_pad) {
    if (!p || max_pad < 0 || max_pad > p->NDP) return fail(DABGPU_E_ARG, "bad args (max_pad <= max_dabplus)");
    if (max_pad && DABGPU_PAD_ARENA_BYTES((int64_t)p->F) > 0x7FFFFFFF) return fail(DABGPU_E_ARG, "an arena of 2 GiB and more");
    for (int s = 0; s < p->S; s++) {
        int n = 0;
        for (const dabgpu_subch &e : p->tab[s])
            if (e.flags & DABGPU_SUBCH_PAD) n++;
        if (n > max_pad) return fail(DABGPU_E_ARG, "stream %d's table has %d PAD subchannels", s, n);
    }
    if (int rc = sync_streams(p)) return rc;
    if (int rc = pad_size(p, max_pad)) return rc;
    p->pad_pending = false;
    return rebuild_tables(p);
}

int dabgpu_pipe_fic_caps(dabgpu_pipe *p, int on) {
    if (!p) return fail(DABGPU_E_ARG, "null pipe");
    if (int rc = sync_streams(p)) return rc;
    p->fic_pending = false;
    if (!on) {
        p->fic = FicLayer();
        return 0;
    }
    if (p->fic.on) return 0;                   // the databases stay
    const size_t nb = (size_t)p->S * sizeof(dabgpu_fic_db);
    HIPCHK(p->fic.db_d.alloc(nb));
    HIPCHK(p->fic.ev.create(hipEventDisableTiming));
    HIPCHK(hipMemset(p->fic.db_d, 0, nb));
    p->fic.on = true;
    return 0;
}

int dabgpu_pipe_fic(dabgpu_pipe *p, const uint8_t *fic_bits, const uint8_t *fic_crc, int want_flags, dabgpu_fic_event *events,
                    dabgpu_fic_table *table, dabgpu_fic_run *run) {
    if (!p || !fic_bits || !fic_crc || !events || !table || !run) return fail(DABGPU_E_ARG, "null arg");
    if (!p->fic.on) return fail(DABGPU_E_STATE, "no FIC layer in this pipeline (dabgpu_pipe_fic_caps)");
    if (!p->fic_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with FIC output to consume");
    if (fic_bits != p->last_fic || fic_crc != p->last_crc)
        return fail(DABGPU_E_ARG, "fic_bits_d and fic_crc_d are not those of the last dabgpu_pipe_run");
    FibJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S;
    J.n_fibs = 12 * p->F;
    J.db = (dabgpu_fic_db *)(uint8_t *)p->fic.db_d;
    J.fibs = fic_bits;
    J.bit_src = p->last_fic_packed ? 0 : 1;
    J.stride = (int64_t)J.n_fibs * (J.bit_src ? 256 : 32);
    J.ok = fic_crc;
    J.want = want_flags & (DABGPU_SUBCH_MP2 | DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT | DABGPU_SUBCH_PAD);
    J.events = events;
    J.event_slots = DABGPU_FIC_EVENT_SLOTS;
    J.table = table;
    J.run = run;
    // on the run's back-end stream, behind its FIC decode; after the previous pass (the
    // databases are updated in place)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(p->fic.ev.wait_on(bs));
    HIPCHK(launch_fib(bs, J));
    HIPCHK(p->fic.ev.record(bs));
    p->fic_pending = false;                    // each run's FIBs enter the layer once
    return 0;
}

int dabgpu_pipe_fic_db(dabgpu_pipe *p, int stream, dabgpu_fic_db *db_h) {
    if (!p || !db_h || stream < 0 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (!p->fic.on) return fail(DABGPU_E_STATE, "no FIC layer in this pipeline (dabgpu_pipe_fic_caps)");
    if (int rc = sync_streams(p)) return rc;
    HIPCHK(hipMemcpy(db_h, p->fic.db_d + (size_t)stream * sizeof(dabgpu_fic_db), sizeof(dabgpu_fic_db), hipMemcpyDeviceToHost));
    return 0;
}

int dabgpu_pipe_fic_clear(dabgpu_pipe *p, int stream) {
    if (!p || stream < -1 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (!p->fic.on) return fail(DABGPU_E_STATE, "no FIC layer in this pipeline (dabgpu_pipe_fic_caps)");
    if (int rc = sync_streams(p)) return rc;
    dabgpu_fic_db *db = (dabgpu_fic_db *)(uint8_t *)p->fic.db_d;
    HIPCHK(launch_fic_clear(p->c->stream, stream < 0 ? db : db + stream, stream < 0 ? p->S : 1));
    HIPCHK(hipStreamSynchronize(p->c->stream));
    return 0;
}

int dabgpu_pipe_mp2(dabgpu_pipe *p, int16_t *pcm, dabgpu_mp2_info *info) {
    if (!p || !pcm || !info) return fail(DABGPU_E_ARG, "null arg");
    if (p->NMP == 0) return fail(DABGPU_E_STATE, "no layer II subchannel in this pipeline");
    if (!p->last_msc || !p->mp2_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with MSC output to consume");
    Mp2Layer &m = p->mp2;
    Mp2SyncJob Y;
    memset(&Y, 0, sizeof Y);
    Y.msc = p->last_msc;
    Y.msc_stride = p->last_msc_stride;
    Y.packed = p->last_msc_packed ? 1 : 0;
    Y.ncif = 4 * p->F;
    Y.nsub = p->NSUB;
    Y.nmp = p->NMP;
    Y.nstreams = p->S;
    Y.cif0s = p->cif0_dev(p->cur);
    Y.ncifs = p->ncif_dev(p->cur);
    Y.mp_sub = m.sub_d;
    Y.mp_br = m.br_d;
    Y.mp_since = m.since_d;
    Y.state = m.sync_d;
    Y.part = m.part_d;
    Y.frames = m.frames_d;
    Y.fstride = m.fstride;
    Y.present = m.present_d;
    Y.info = info;
    Mp2Job J;
    memset(&J, 0, sizeof J);
    J.frames = m.frames_d;
    J.stride = m.fstride;
    J.n_chains = p->S * p->NMP;
    J.chain_len = 4 * p->F;
    J.present = m.present_d;
    J.state_in = m.vstate_d[m.cur];
    J.state_out = m.vstate_d[m.cur ^ 1];
    J.pcm = pcm;
    J.info = info;
    J.cdiv = p->NMP;
    J.idx_a = (int64_t)4 * p->F * p->NMP;
    J.idx_b = 1;
    J.idx_c = p->NMP;
    if (int rc = mp2_tables(p->c, &J.tabs)) return rc;
    // on the last run's back-end stream (after its MSC), after the previous pass (the
    // synchronisers, the decoders and the frame slots carry over or are reused)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(m.ev.wait_on(bs));
    HIPCHK(launch_mp2_sync(bs, Y));
    HIPCHK(launch_mp2_decode(bs, J));
    HIPCHK(m.ev.record(bs));
    m.cur ^= 1;
    p->mp2_pending = false;                    // each run's CIFs enter the layer once
    return 0;
}

int dabgpu_pipe_packet(dabgpu_pipe *p, uint8_t *bytes, dabgpu_datagroup *groups, dabgpu_packet_run *run,
                       dabgpu_packet_info *info) {
    if (!p || !bytes || !groups || !run || !info) return fail(DABGPU_E_ARG, "null arg");
    if (p->NPK == 0) return fail(DABGPU_E_STATE, "no packet-mode subchannel in this pipeline");
    if (!p->last_msc || !p->pk_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with MSC output to consume");
    PacketLayer &k = p->pk;
    PkJob J;
    memset(&J, 0, sizeof J);
    J.msc = p->last_msc;
    J.msc_stride = p->last_msc_stride;
    J.packed = p->last_msc_packed ? 1 : 0;
    J.ncif = 4 * p->F;
    J.nsub = p->NSUB;
    J.npk = p->NPK;
    J.nstreams = p->S;
    J.ncell = k.ncell;
    J.cap = k.cap;
    J.cif0s = p->cif0_dev(p->cur);
    J.ncifs = p->ncif_dev(p->cur);
    J.pk_sub = k.sub_d;
    J.pk_br = k.br_d;
    J.pk_since = k.since_d;
    J.state = k.state_d;
    J.carry_in = k.carry_d[k.cur];
    J.carry_out = k.carry_d[k.cur ^ 1];
    J.rec = k.rec_d;
    J.take = k.take_d;
    J.segtab = k.segtab_d;
    J.bytes = bytes;
    J.arena = DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, k.cap);
    J.groups = groups;
    J.gslots = DABGPU_PKT_GROUP_SLOTS(p->F, p->max_bitrate);
    J.run = run;
    J.info = info;
    // on the last run's back-end stream (after its MSC), after the previous pass (the
    // assemblers and the work buffers carry over or are reused)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(k.ev.wait_on(bs));
    HIPCHK(launch_packet(bs, J));
    HIPCHK(k.ev.record(bs));
    k.cur ^= 1;
    p->pk_pending = false;                     // each run's CIFs enter the layer once
    p->pk_bytes = bytes;
    p->pk_groups = groups;
    p->pk_run = run;
    p->mot_pending = p->NMOT > 0;
    return 0;
}

int dabgpu_pipe_mot(dabgpu_pipe *p, uint8_t *bytes, dabgpu_mot_object *objects, dabgpu_mot_run *run) {
    if (!p || !bytes || !objects || !run) return fail(DABGPU_E_ARG, "null arg");
    if (p->NMOT == 0) return fail(DABGPU_E_STATE, "no MOT subchannel in this pipeline");
    if (!p->mot_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_packet call of this run to consume");
    if ((uintptr_t)bytes & 15) return fail(DABGPU_E_ARG, "bytes_d must be 16-byte aligned");
    MotLayer &m = p->mot;
    MotJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S * p->NMOT;
    J.max_body = m.body;
    J.body_cap = m.body_cap;
    J.state_bytes = (int64_t)m.state_bytes;
    J.state = m.state_d;
    J.src = m.src_d;
    J.groups = p->pk_groups;
    J.gslots = m.gslots;
    J.bytes = p->pk_bytes;
    J.arena = DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, p->pk.cap);
    J.run = p->pk_run;
    J.objects = objects;
    J.out = bytes;
    J.out_arena = DABGPU_MOT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, m.body);
    J.mot_run = run;
    J.ops = m.ops_d;
    J.nops = m.nops_d;
    // on the run's back-end stream, behind its packet layer; after the previous pass (the
    // motHandlers are updated in place, the copy list is reused)
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(m.ev.wait_on(bs));
    HIPCHK(launch_mot(bs, J));
    HIPCHK(m.ev.record(bs));
    p->mot_pending = false;                    // each run's groups enter the layer once
    return 0;
}

int dabgpu_pipe_mot_caps(dabgpu_pipe *p, int max_mot, int max_body_bytes) {
    if (!p || max_mot < 0 || max_body_bytes < 0 || max_body_bytes > (1 << 24) || max_mot > p->NPK)
        return fail(DABGPU_E_ARG, "bad args (max_mot <= max_packet, max_body_bytes <= 1 << 24)");
    const int body = max_body_bytes ? max_body_bytes : DABGPU_MOT_BODY_BYTES;
    if (max_mot && (DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, p->pk.cap) > 0x7FFFFFFF ||
                    DABGPU_MOT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, body) > 0x7FFFFFFF))
        return fail(DABGPU_E_ARG, "arenas of 2 GiB and more");
    for (int s = 0; s < p->S; s++) {
        int n = 0;
        for (const dabgpu_subch &e : p->tab[s])
            if (e.flags & DABGPU_SUBCH_MOT) n++;
        if (n > max_mot) return fail(DABGPU_E_ARG, "stream %d's table has %d MOT subchannels", s, n);
    }
    if (int rc = sync_streams(p)) return rc;
    if (int rc = mot_size(p, max_mot, body)) return rc;
    p->mot_pending = false;
    return rebuild_tables(p);
}

int dabgpu_pipe_packet_caps(dabgpu_pipe *p, int max_packet, int max_group_bytes) {
    if (!p || max_packet < 0 || max_group_bytes < 0 || max_packet > p->NSUB) return fail(DABGPU_E_ARG, "bad args");
    if (max_packet < p->NMOT) return fail(DABGPU_E_ARG, "the MOT layer holds %d slots (dabgpu_pipe_mot_caps first)", p->NMOT);
    if (max_packet && p->max_bitrate < 8) return fail(DABGPU_E_ARG, "max_bitrate %d holds no packet-mode entry", p->max_bitrate);
    const int cap = max_group_bytes ? max_group_bytes : DABGPU_PKT_GROUP_BYTES;
    // the MOT layer indexes the packet arena in int32 (as dabgpu_pipe_mot_caps checks)
    if (p->NMOT && DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, (int64_t)cap) > 0x7FFFFFFF)
        return fail(DABGPU_E_ARG, "a packet arena of 2 GiB and more under the MOT layer");
    for (int s = 0; s < p->S; s++) {
        int n = 0;
        for (const dabgpu_subch &e : p->tab[s])
            if (e.flags & DABGPU_SUBCH_PACKET) n++;
        if (n > max_packet) return fail(DABGPU_E_ARG, "stream %d's table has %d packet-mode subchannels", s, n);
    }
    if (int rc = sync_streams(p)) return rc;
    if (int rc = packet_size(p, max_packet, cap)) return rc;
    p->mot_pending = false;
    return rebuild_tables(p);
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

// DABGPU_CTL_INJECT_BOUNDS: the table the next run's MSC job reads its start offsets from
static int inject_table(dabgpu_pipe *p) {
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
int dabgpu_pipe_set_subch(dabgpu_pipe *p, int stream, const dabgpu_subch *sub, int32_t n) {
    if (!p || stream < -1 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (int rc = check_table(sub, n, p->NSUB, p->max_bitrate, p->NDP, p->NMP, p->NPK, p->NMOT, p->NPAD)) return rc;   // the table stays on error
    // in-flight kernels read the device tables: a rare control call, so it waits for
    // everything the pipeline has enqueued (as dabgpu_pipe_set_profiling) instead of
    // double-buffering them
    if (int rc = sync_streams(p)) return rc;
    const size_t RB = 120 * DP_MAX_RS;
    for (auto [s, end] = stream_range(p, stream); s < end; s++) {
        const std::vector<dabgpu_subch> old = p->tab[s];
        const std::vector<int64_t> old_since = p->since[s];
        std::vector<int> old_slot(old.size(), -1);      // DAB+ slot of each old entry
        for (int k = 0, j = 0; k < (int)old.size(); k++)
            if (old[k].flags & DABGPU_SUBCH_DABPLUS) old_slot[k] = j++;
        // an entry whose index and fields are unchanged goes on (since_cif, DAB+ ring and
        // state kept, wherever its slot now lies); every other one starts like a new
        // dabConcurrent / mp4Processor at the stream's current CIF
        std::vector<uint8_t> rings, nrings;
        std::vector<DpState> sts, nsts;
        if (p->NDP) {
            rings.resize(p->NDP * RB);
            sts.resize(p->NDP);
            HIPCHK(hipMemcpy(rings.data(), p->dp.ring_d + (size_t)s * p->NDP * RB, rings.size(), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(sts.data(), p->dp.state_d + (size_t)s * p->NDP, sizeof(DpState) * p->NDP, hipMemcpyDeviceToHost));
            nrings.assign(rings.size(), 0);
            nsts.assign(p->NDP, DpState{0, 0});
        }
        // the layer II slots likewise: synchroniser, frame in progress and decoder of an
        // unchanged entry move to its new slot, every other slot is a new mp2Processor
        if (p->NMP) {
            Mp2Layer &m = p->mp2;
            const size_t NM = p->NMP, FS = m.fstride, o = (size_t)s * NM;
            std::vector<Mp2SyncState> sy(NM), nsy(NM, Mp2SyncState{0, 0, 0, 0});
            std::vector<uint8_t> pt(NM * FS), npt(NM * FS, 0);
            std::vector<int16_t> vs(NM * MP2_STATE_I16), nvs(NM * MP2_STATE_I16, 0);
            HIPCHK(hipMemcpy(sy.data(), m.sync_d + o, sizeof(Mp2SyncState) * NM, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(pt.data(), m.part_d + o * FS, NM * FS, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(vs.data(), m.vstate_d[m.cur] + o * MP2_STATE_I16, sizeof(int16_t) * vs.size(), hipMemcpyDeviceToHost));
            std::vector<int> oslot(old.size(), -1);
            for (int k = 0, j = 0; k < (int)old.size(); k++)
                if (old[k].flags & DABGPU_SUBCH_MP2) oslot[k] = j++;
            for (int k = 0, j = 0; k < n; k++) {
                if (!(sub[k].flags & DABGPU_SUBCH_MP2)) continue;
                if (k < (int)old.size() && same_subch(old[k], sub[k])) {
                    nsy[j] = sy[oslot[k]];
                    memcpy(npt.data() + j * FS, pt.data() + oslot[k] * FS, FS);
                    memcpy(nvs.data() + (size_t)j * MP2_STATE_I16, vs.data() + (size_t)oslot[k] * MP2_STATE_I16,
                           sizeof(int16_t) * MP2_STATE_I16);
                }
                j++;
            }
            HIPCHK(hipMemcpy(m.sync_d + o, nsy.data(), sizeof(Mp2SyncState) * NM, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(m.part_d + o * FS, npt.data(), NM * FS, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(m.vstate_d[m.cur] + o * MP2_STATE_I16, nvs.data(), sizeof(int16_t) * nvs.size(), hipMemcpyHostToDevice));
        }
        // the packet slots likewise: an unchanged entry's assembler and series in flight move
        // to its new slot, every other slot is a new mscDatagroup
        if (p->NPK) {
            PacketLayer &m = p->pk;
            const size_t NK = p->NPK, CB = m.cap, o = (size_t)s * NK;
            std::vector<PkState> ps(NK), nps(NK, PkState{0, -1, 0, 0, 0, 0, 0, 0});
            std::vector<uint8_t> ca(NK * CB), nca(NK * CB, 0);
            HIPCHK(hipMemcpy(ps.data(), m.state_d + o, sizeof(PkState) * NK, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ca.data(), m.carry_d[m.cur] + o * CB, NK * CB, hipMemcpyDeviceToHost));
            std::vector<int> oslot(old.size(), -1);
            for (int k = 0, j = 0; k < (int)old.size(); k++)
                if (old[k].flags & DABGPU_SUBCH_PACKET) oslot[k] = j++;
            for (int k = 0, j = 0; k < n; k++) {
                if (!(sub[k].flags & DABGPU_SUBCH_PACKET)) continue;
                if (k < (int)old.size() && same_subch(old[k], sub[k])) {
                    nps[j] = ps[oslot[k]];
                    memcpy(nca.data() + j * CB, ca.data() + oslot[k] * CB, CB);
                }
                j++;
            }
            HIPCHK(hipMemcpy(m.state_d + o, nps.data(), sizeof(PkState) * NK, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(m.carry_d[m.cur] + o * CB, nca.data(), NK * CB, hipMemcpyHostToDevice));
        }
        // the MOT slots likewise: an unchanged entry's motHandler moves to its new slot, every
        // other slot is a new one
        if (p->NMOT) {
            MotLayer &m = p->mot;
            const size_t NM = p->NMOT, SB = m.state_bytes, o = (size_t)s * NM * SB;
            std::vector<uint8_t> ms(NM * SB), nms(NM * SB, 0);
            HIPCHK(hipMemcpy(ms.data(), m.state_d + o, NM * SB, hipMemcpyDeviceToHost));
            std::vector<int> oslot(old.size(), -1);
            for (int k = 0, j = 0; k < (int)old.size(); k++)
                if (old[k].flags & DABGPU_SUBCH_MOT) oslot[k] = j++;
            for (int k = 0, j = 0; k < n; k++) {
                if (!(sub[k].flags & DABGPU_SUBCH_MOT)) continue;
                if (k < (int)old.size() && same_subch(old[k], sub[k])) memcpy(nms.data() + j * SB, ms.data() + oslot[k] * SB, SB);
                j++;
            }
            HIPCHK(hipMemcpy(m.state_d + o, nms.data(), NM * SB, hipMemcpyHostToDevice));
        }
        // the PAD slots likewise: an unchanged entry's padHandler moves to its new slot, every
        // other slot is a new one
        if (p->NPAD) {
            const size_t NM = p->NPAD, SB = sizeof(PadState), o = (size_t)s * NM * SB;
            std::vector<uint8_t> ms(NM * SB), nms(NM * SB, 0);
            HIPCHK(hipMemcpy(ms.data(), p->pad.state_d + o, NM * SB, hipMemcpyDeviceToHost));
            std::vector<int> oslot(old.size(), -1);
            for (int k = 0, j = 0; k < (int)old.size(); k++)
                if (old[k].flags & DABGPU_SUBCH_PAD) oslot[k] = j++;
            for (int k = 0, j = 0; k < n; k++) {
                if (!(sub[k].flags & DABGPU_SUBCH_PAD)) continue;
                if (k < (int)old.size() && same_subch(old[k], sub[k])) memcpy(nms.data() + j * SB, ms.data() + oslot[k] * SB, SB);
                j++;
            }
            HIPCHK(hipMemcpy(p->pad.state_d + o, nms.data(), NM * SB, hipMemcpyHostToDevice));
        }
        p->tab[s].assign(sub, sub + n);
        p->since[s].assign(n, p->st[s].cif_count);
        for (int k = 0, j = 0; k < n; k++) {
            const bool kept = k < (int)old.size() && same_subch(old[k], sub[k]);
            if (kept) p->since[s][k] = old_since[k];
            if (!(sub[k].flags & DABGPU_SUBCH_DABPLUS)) continue;
            if (kept) {
                memcpy(nrings.data() + (size_t)j * RB, rings.data() + (size_t)old_slot[k] * RB, RB);
                nsts[j] = sts[old_slot[k]];
            }
            j++;
        }
        if (p->NDP) {
            HIPCHK(hipMemcpy(p->dp.ring_d + (size_t)s * p->NDP * RB, nrings.data(), nrings.size(), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(p->dp.state_d + (size_t)s * p->NDP, nsts.data(), sizeof(DpState) * p->NDP, hipMemcpyHostToDevice));
        }
    }
    p->last_msc = nullptr;            // the last run's rows follow the old tables: no DAB+ layer over them now
    p->mot_pending = false;
    p->pad_pending = false;
    if (int rc = rebuild_tables(p)) return rc;
    if (p->inject_bounds) return inject_table(p);
    return 0;
}

int dabgpu_pipe_get_subch(dabgpu_pipe *p, int stream, dabgpu_subch *sub, int32_t *n, int64_t *since_cif) {
    if (!p || !n || stream < 0 || stream >= p->S || (!sub && !p->tab[stream].empty()))
        return fail(DABGPU_E_ARG, "bad args");
    *n = (int32_t)p->tab[stream].size();
    for (int k = 0; k < *n; k++) {
        sub[k] = p->tab[stream][k];
        if (since_cif) since_cif[k] = p->since[stream][k];
    }
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
        HIPCHK(p->disp_d.alloc((size_t)p->S * p->R * K));
        HIPCHK(hipMemset(p->disp_d, 0, sizeof(float2) * (size_t)p->S * p->R * K));
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
