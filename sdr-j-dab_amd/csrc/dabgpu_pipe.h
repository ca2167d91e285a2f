// dabgpu_pipe.h -- the streaming pipeline's state, shared by its two translation units:
// dabgpu_pipe.cpp (create / destroy, front and back end, dabgpu_pipe_run, control, state, display)
// and dabgpu_layers.cpp (the layers behind the MSC and the FIC, and the subchannel tables)
#pragma once
#include "dabgpu_internal.h"
#include "front_replay.h"
#include "layer_slots.h"

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
    dab::DevBuf<uint32_t> dec;       // Viterbi decisions: the MSC's, then the FIC's
    dab::Event ev_copy;              // the descriptor block's upload done (before its staging is reused)
    dab::Event ev_back;              // the run's back end done
    dab::Event ev_acs;               // the run's ACS done (the ring's last reader)
    dab::Stream stream;
};
// Background null search (DABGPU_CTL_ACQ_ASYNC, the default since round 6): a stream that
// loses sync after an acquisition is searched on its own low-priority stream while the
// others keep decoding; its results are taken by the first dabgpu_pipe_run after they arrive
struct AcqBg {
    bool async = false;              // set true by dabgpu_pipe_create
    bool inflight = false;           // results pending (the event alone says recorded, not taken)
    dab::Event ev;
    dab::DevBuf<dab::AcqJob> jobs_d; // [S], and its pinned staging
    dab::PinBuf<dab::AcqJob> h_jobs;
    dab::DevBuf<dab::AcqResult> res_d;   // [S]
    dab::PinBuf<dab::AcqResult> h_res;
    std::vector<int> who;
    std::vector<char> acquiring;                     // [S]
    dab::Stream stream;
};
// A layer's slot map, [S][slots per stream]: the table entry of each slot (-1: none), the entry's
// bitRate and its since (rebuild_tables)
struct SlotMap {
    dab::DevBuf<int32_t> sub_d;
    dab::DevBuf<int16_t> br_d;
    dab::DevBuf<int64_t> since_d;
    hipError_t alloc(size_t n) {
        hipError_t e = sub_d.alloc(n);
        if (e == hipSuccess) e = br_d.alloc(n);
        return e != hipSuccess ? e : since_d.alloc(n);
    }
    dab::SlotMapView view() const { return {sub_d, br_d, since_d}; }
};
// DAB+ superframe layer (mp4Processor per DAB+ subchannel and stream)
struct DabPlus {
    int max_rs = 0;
    // compact superframe output (dabgpu_pipe_set_dabplus_compact): the layer decodes into
    // this sparse scratch and stores the run's superframes in CIF order for the caller
    bool compact = false;
    dab::DevBuf<uint8_t> sf_sparse_d;
    SlotMap map;                       // [S][NDP]
    dab::DevBuf<uint8_t> ring_d;       // [S][NDP][120*DP_MAX_RS]
    dab::DevBuf<dab::DpState> state_d; // [S][NDP]
    dab::DevBuf<uint8_t> code_d;       // [S][NDP][4F] superframe verdict per candidate CIF
    dab::Event ev;                     // the last superframe pass
};
// MPEG layer II layer (mp2Processor per classic-audio subchannel and stream): allocated only
// for a pipeline with caps.max_mp2 > 0
struct Mp2Layer {
    int fstride = 0;                   // bytes per frame slot: 2 * 24 * max_bitrate bits
    SlotMap map;                       // [S][NMP]
    dab::DevBuf<dab::Mp2SyncState> sync_d;   // [S][NMP] the synchronisers
    dab::DevBuf<uint8_t> part_d;       // [S][NMP][fstride] their frames in progress
    dab::DevBuf<int16_t> vstate_d[2];  // [S][NMP][MP2_STATE_I16] the decoders: a pass reads [cur], writes [cur ^ 1]
    int cur = 0;
    dab::DevBuf<uint8_t> frames_d;     // [S * NMP][4F][fstride] the frames that completed in the run
    dab::DevBuf<uint8_t> present_d;    // [S * NMP][4F]
    dab::Event ev;                     // the last pass
};
// Packet-mode data layer (an mscDatagroup's assembler per packet-mode subchannel and stream):
// allocated only while dabgpu_pipe_packet_caps' max_packet > 0
struct PacketLayer {
    int cap = 0, ncell = 0;            // max_group_bytes; cells per CIF the buffers hold (max_bitrate / 8)
    SlotMap map;                       // [S][NPK]
    dab::DevBuf<dab::PkState> state_d; // [S][NPK] the assemblers
    dab::DevBuf<uint8_t> carry_d[2];   // [S][NPK][cap] their series in flight: a pass reads [cur], writes [cur ^ 1]
    int cur = 0;
    dab::DevBuf<uint32_t> rec_d;       // [S * NPK][4F][ncell] packet records of the run
    dab::DevBuf<int2> take_d;          // [S * NPK][4F][ncell]
    dab::DevBuf<int32_t> segtab_d;     // [S * NPK][1 + 4F * ncell]
    dab::Event ev;                     // the last pass
    // the IP layer over the packet slots (an ip_dataHandler per entry flagged DABGPU_SUBCH_IP and stream)
    dab::DevBuf<dabgpu_ip_state> ip_state_d;   // [S][NPK] their counters, updated in place
    dab::DevBuf<int32_t> ip_on_d;      // [S][NPK] 1: the slot's entry is flagged DABGPU_SUBCH_IP
    int n_ip = 0;                      // entries so flagged in the applied tables
    dab::Event ip_ev;                  // the last IP pass
};
// MOT layer (a motHandler per packet entry flagged DABGPU_SUBCH_MOT and stream): allocated
// only while dabgpu_pipe_mot_caps' max_mot > 0
struct MotLayer {
    int body = 0, body_cap = 0;        // max_body_bytes, and rounded up to 16
    size_t state_bytes = 0;            // dabgpu_mot_state_bytes(body)
    int gslots = 0;                    // DABGPU_PKT_GROUP_SLOTS(F, max_bitrate)
    dab::DevBuf<uint8_t> state_d;      // [S][NMOT][state_bytes] the motHandlers, updated in place
    dab::DevBuf<int32_t> src_d;        // [S][NMOT] the packet slot (s * NPK + j) each reads, -1: absent
    dab::DevBuf<int4> ops_d;           // [S * NMOT][2 * gslots] the pass's copy list
    dab::DevBuf<int32_t> nops_d;       // [S * NMOT]
    dab::Event ev;                     // the last pass
};
// PAD layer (a padHandler per DAB+ entry flagged DABGPU_SUBCH_PAD and stream): allocated only
// while dabgpu_pipe_pad_caps' max_pad > 0
struct PadLayer {
    dab::DevBuf<uint8_t> state_d;      // [S][NPAD] PadState, the padHandlers, updated in place
    dab::DevBuf<int32_t> src_d;        // [S][NPAD] the DAB+ slot (s * NDP + j) each reads, -1: absent
    dab::Event ev;                     // the last pass
};
// Audio output layer (an audioSink per layer II entry flagged DABGPU_SUBCH_AUDIO and stream):
// allocated only while dabgpu_pipe_audio_caps' max_audio > 0
struct AudioLayer {
    dab::DevBuf<dab::AudioState> state_d;   // [S][NAUDIO] the sinks' interpolators, updated in place
    dab::DevBuf<int32_t> src_d;        // [S][NAUDIO] the MP2 slot (s * NMP + j) each reads, -1: absent
    dab::Event ev;                     // the last pass
};
// FIC layer (a fib_processor's database per stream): allocated only while dabgpu_pipe_fic_caps is on
struct FicLayer {
    dab::DevBuf<uint8_t> db_d;         // [S] dabgpu_fic_db, updated in place
    dab::Event ev;                     // the last pass
    bool on = false;
};

// What the layers may consume: the last run's outputs, the outputs of the run's dabplus and
// packet calls (which the PAD and the MOT layer read), and whether each has entered its layer
struct LayerFeed {
    const uint8_t *last_msc = nullptr;   // MSC bits of the last run
    int32_t last_msc_stride = 0;
    bool last_msc_packed = false;
    // per slot kind: DAB+, layer II, packet -- the last run's CIFs have not entered the layer yet;
    // MOT, PAD, audio output -- nor the outputs below of the run's packet / dabplus / mp2 call
    bool pending[slots::NSLOTKIND] = {};
    bool ip_pending = false;             // the outputs of the run's packet call have not entered the IP layer yet
    const uint8_t *pk_bytes = nullptr;   // the run's dabgpu_pipe_packet call
    const dabgpu_datagroup *pk_groups = nullptr;
    const dabgpu_packet_run *pk_run = nullptr;
    const uint8_t *dp_sf = nullptr;      // the run's dabgpu_pipe_dabplus call
    const dabgpu_superframe *dp_info = nullptr;
    int32_t dp_sf_stride = 0;
    bool dp_sf_compact = false;
    const int16_t *mp2_pcm = nullptr;    // the run's dabgpu_pipe_mp2 call
    const dabgpu_mp2_info *mp2_info = nullptr;
    const uint8_t *last_fic = nullptr, *last_crc = nullptr;   // the FIC outputs of the last run
    bool last_fic_packed = false;
    bool fic_pending = false;            // ... have not entered the FIC layer yet
    // a run has delivered (the pointers above are the caller's, set beside this call)
    void new_run(bool have_rows, bool have_fic) {
        pending[slots::DABPLUS] = pending[slots::MP2] = pending[slots::PACKET] = have_rows;
        pending[slots::MOT] = false;     // until this run's dabgpu_pipe_packet
        pending[slots::PAD] = false;     // until this run's dabgpu_pipe_dabplus
        pending[slots::AUDIO] = false;   // until this run's dabgpu_pipe_mp2
        ip_pending = false;
        fic_pending = have_fic;
    }
    // the last run's rows follow the old tables: no layer over them now (the FIC's does not read tables)
    void tables_changed() {
        last_msc = nullptr;
        pending[slots::MOT] = false;
        pending[slots::PAD] = false;
        pending[slots::AUDIO] = false;
        ip_pending = false;
    }
};

// what check_table holds a table against: the pipeline's caps and the slots its layers hold now
struct TableLimits {
    int max_subch, max_bitrate;
    int max_slots[slots::NSLOTKIND];
};

struct dabgpu_pipe {
    dabgpu_ctx *c = nullptr;
    int S = 0, F = 0, NSUB = 0, R = 0, NDP = 0, NMP = 0, NPK = 0, NMOT = 0, NPAD = 0, NAUDIO = 0;
    TableLimits limits() const { return {NSUB, max_bitrate, {NDP, NMP, NPK, NMOT, NPAD, NAUDIO}}; }
    int nslot(int kind) const { return limits().max_slots[kind]; }   // slots per stream of a slots::kKinds kind
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
    dab::DevBuf<int32_t> ent_prof_d, ent_start_d, act_d;
    dab::DevBuf<int64_t> ent_since_d;
    std::vector<uint8_t> entry_valid;   // [S][4F][NSUB] of the last run (dabgpu_pipe_msc_entry_valid)
    std::vector<front::StreamSt> st;
    dab::DevBuf<uint8_t> ring;            // [S][R][75][3072] RING8 bytes (soft bit + 127, dab_kernels.h)
    dab::DevBuf<dab::Profile> prof_d;     // [NSUB]
    dab::DevBuf<dab::Profile> ficprof_d;
    dab::DevBuf<uint8_t> inv_d;           // the subchannel profiles' inverse depuncturing tables
    dab::DevBuf<int32_t> substart_d;      // [NSUB]
    dab::DevBuf<dabgpu_frame> frames_d;
    dab::DevBuf<int32_t> si_d;
    dab::DevBuf<int16_t> corr_d, snr_d;
    dab::DevBuf<float> fc_d, fcpart_d;    // [S*F] float2, [S*F][kMaxChunks] float2
    // the back end's per-run descriptors, one block per back-end stream (parity), uploaded
    // with ONE copy per run (each runtime copy is a kernel of its own on the back-end
    // stream, ~6 us, in front of the ACS): [S] int64 CIF index of each stream's first CIF
    // slot | [S] int32 CIFs each stream delivered | [S * F] int32 FIC ring slots;
    // h_desc: their pinned staging, BackSlot::ev_copy marks the upload done before reuse
    dab::DevBuf<uint8_t> desc_d;
    dab::PinBuf<uint8_t> h_desc;
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
    dab::PinBuf<dabgpu_frame> h_frames;
    dab::PinBuf<int32_t> h_si;
    dab::PinBuf<float2> h_fc;
    dab::PinBuf<int16_t> h_snr;
    // the back-end streams' own error words (the front end's is the context's): the
    // Viterbi jobs of run r set berr_d[r & 1], which the back end publishes into
    // h_berr[r & 1] (and clears) as its last step; read once back[r & 1].ev_back completed
    dab::DevBuf<int32_t> berr_d;
    dab::PinBuf<int32_t> h_berr;
    // speculative back end (dabgpu_pipe_run): queued behind the first front pass
    bool speculate = true;                      // env DABGPU_NO_SPECULATE=1: off (A/B)
    dab::Event ev_front;
    bool ev_front_demod = false;     // ev_front marks this pass's demod (the speculative back end's gate)
    std::vector<dabgpu_frame> last_frames;   // [S][F]
    std::vector<dabgpu_frame_info> last_info;   // [S][F] observables of the last run
    DabPlus dp;
    Mp2Layer mp2;
    PacketLayer pk;
    MotLayer mot;
    PadLayer pad;
    AudioLayer audio;
    FicLayer fic;
    LayerFeed feed;
    // the iqBuffer feed (dabgpu_pipe_set_display): symbol 2's display carriers per ring slot
    dab::DevBuf<float2> disp_d;      // [S][R][K]
    bool display = false;
    int disp_token = 2;              // the display feed's symbol (ofdm-decoder.cpp:61 displayToken)
    bool packed = false;             // MSC output 8 bits per byte (dabgpu_pipe_set_packed)
    bool fic_packed = false;         // FIC output as FIB bytes (DABGPU_PACK_FIC)
    int iq_fmt = DABGPU_IQ_F32;      // sample format of the streams (dabgpu_pipe_set_iq_format)
    // fault injection (DABGPU_CTL_INJECT_BOUNDS): the next run's MSC job gets a subchannel
    // table whose first entry points past the ring, which the Viterbi loader refuses
    bool inject_bounds = false;
    dab::DevBuf<int32_t> substart_bad_d;
    // optional per-stage kernel timing (HIP events on the stage's stream)
    int profiling = 0;                          // 1: last run, 2: every run since enabled, 3: 2 + stages alone
    std::vector<dab::Event> ev_pool;
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

namespace dab {

// wait for everything the pipeline has enqueued on its front-end and back-end streams
inline int sync_streams(dabgpu_pipe *p) {
    HIPCHK(p->c->stream.sync());
    for (BackSlot &b : p->back) HIPCHK(b.stream.sync());
    return 0;
}
// the streams a control call names: [first, end) -- one stream, or every stream for -1
inline std::pair<int, int> stream_range(const dabgpu_pipe *p, int stream) {
    return stream < 0 ? std::make_pair(0, p->S) : std::make_pair(stream, stream + 1);
}

// dabgpu_pipe.cpp
hipError_t prof_mark(dabgpu_pipe *p, int stage, bool start);
int inject_table(dabgpu_pipe *p);
// dabgpu_layers.cpp
int check_table(const dabgpu_subch *sub, int n, const TableLimits &lim);
int packet_size(dabgpu_pipe *p, int npk, int cap);
int mot_size(dabgpu_pipe *p, int nmot, int body);
int pad_size(dabgpu_pipe *p, int npad);
int audio_size(dabgpu_pipe *p, int naudio);
int rebuild_tables(dabgpu_pipe *p);

}  // namespace dab
