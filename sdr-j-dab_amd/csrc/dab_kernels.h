// dab_kernels.h -- host/device shared structs and kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dabgpu.h"
#include "msc_feed.h"

namespace dab {

constexpr int TU = 2048, TS = 2552, TG = 504, TNULL = 2656, TF = 196608, K = 1536, L = 76;
constexpr int NSYM = 75;                 // data symbols per frame
constexpr int SYMBITS = 2 * K;           // 3072 soft bits per symbol
constexpr int FRAME_SOFT = NSYM * SYMBITS;
constexpr int INPUT_RATE = 2048000;

// device tables for the OFDM kernels (built on the host with the reference's
// own float expressions, see dabgpu_ctx.cpp: HostTables)
// The NCO without its 16 MB table: oscillatorTable[t] (ofdm-processor.cpp:79-81) is
// float(e^{2 pi i t / 2048000}); with t = 16000 a + 128 b + c it is the float rounding
// of A[a] (B[b] C[c]) in double (fma complex products), A[a] = e^{2 pi i a/128},
// B[b] = e^{2 pi i b/16000}, C[c] = e^{2 pi i c/2048000}: 381 double2 that fit in LDS.
// The rounded product equals the table at every one of the 2048000 indices
// (tests/cpp/test_nco.c on the host, test_gpu_parity's exhaustive check on the GPU).
constexpr int NCO_A = 0, NCO_B = 128, NCO_C = 253, NCO_N = 384, NCO_USED = 381;

struct OfdmTables {
    const float2 *osc;      // oscillatorTable[2048000] (ofdm-processor.cpp:79-81)
    const double2 *nco;     // the factor tables above, [NCO_N]
    const float2 *ref;      // PRS refTable[2048] (phasereference.cpp:40-47), natural bin order
    const float *refarg;    // refArg[18] (ofdm-decoder.cpp:71-74)
    const float2 *w2048;    // W2048^j = e^{-2 pi i j/2048}, j < 2048 (double, rounded to float)
    const int16_t *carrier_of_bin;   // [2048] carrier index of an FFT bin (mapper.cpp), -1 if none
    const int16_t *stage_of_bin;     // [2048] the demod's soft-bit stage word of an FFT bin (stage_layout.h)
    const int16_t *stage_pair;       // [768] stage word of carrier pair p (carriers 2p, 2p+1)
    int32_t *err;           // device error word: kernels OR in DABGPU_KERR_* bits
};
// outputs of the front-end kernels besides the soft bits
struct DemodAux {
    int32_t *si;            // findIndex per frame (k_demod_wg<.., true>, k_prs_wg); null: frames give block0
    float *maxv, *sumv;     // optional: findIndex's Max and sum |r|
    int16_t *snr;           // optional: get_snr of block 0 per frame
    int32_t level;          // findIndex threshold
    float2 *disp;           // optional: [out_slot][K] symbol 2's FFT at bins [0, K/2) and
                            // [T_u-1-K/2, T_u-1) -- the iqBuffer feed of processToken
                            // (ofdm-decoder.cpp:192-206)
    int32_t ring8;          // soft bits as RING8 bytes (the pipeline's ring), else int16
    int32_t fmt;            // sample format of iq (DABGPU_IQ_F32 / S16 / U8)
    int32_t disp_token;     // the symbol disp receives (ofdmDecoder's displayToken, 2 by default)
    float2 *mix;            // test hook (dabgpu_ofdm_demod_mix): [out_slot][75][T_u] the NCO-mixed
                            // FFT input of every data symbol, as the demod's FFT sees it
    float2 *spec;           // with mix: [out_slot][75][T_u] that FFT's output, natural bin order
                            // (both in absolute units: the recorded formats' scale taken out)
};
// The pipeline's soft-bit ring holds each ibits value v as the byte v + 127: processToken's
// values are (int16_t)(q * 127.0) with |q| <= 1 (ofdm-decoder.cpp:188-189; a 0/0 gives 0),
// so v + 127 lies in 0..254, and v + 127 is exactly the Viterbi's branch-metric input
// (viterbi.cpp:230-233: (int16_t)(v + 127) clamped to 0..255, a no-op on that range).
constexpr int RING8_BIAS = 127;
constexpr int KERR_FRAME = 1;      // frame descriptor outside its stream / bad NCO phase
constexpr int KERR_VITERBI = 2;    // Viterbi source outside its buffer
constexpr int KERR_RATE = 4;       // rate conversion: a table entry outside its block or its staged piece

struct AcqJob {
    int64_t iq_base;
    int64_t start;
    int64_t end;
    int32_t local_phase;
    int32_t phase;          // coarse + fine
    int32_t attempts;       // ofdmProcessor::run's `attempts` carried in (ofdm-processor.cpp:274-314)
    int32_t scan;           // scanMode: count No_Signal_Found after > 5 failed attempts
};
struct AcqResult {
    int64_t window;
    int32_t local_phase;
    int32_t status;
    int32_t attempts;       // `attempts` after the search
    int32_t no_signal;      // No_Signal_Found emissions during the search
};

// ---- Viterbi ------------------------------------------------------------
// decision words: per chunk of DEC_WORD_STEPS trellis steps and codeword row, 64
// lanes x 32 bits, in blocks of 64 rows (one traceback wave) whose chunks are
// contiguous: dec[((row / 64 * dec_nch + chunk) * 64 + row % 64) * 64 + lane]
// (dec_word_index); rows padded to a whole block of 64
constexpr int DEC_WORD_STEPS = 30;
// mother-code positions (4 per trellis step) of one ACS branch-metric tile (two decision
// words, 60 steps): the inverse depuncturing tables hold positions within their tile
constexpr int VIT_TILE_POS = 4 * 2 * DEC_WORD_STEPS;
inline __host__ __device__ int64_t dec_rows(int n_cw) { return ((int64_t)n_cw + 63) / 64 * 64; }
inline __host__ __device__ int32_t dec_chunks(int nbits) { return (nbits + 6 + DEC_WORD_STEPS - 1) / DEC_WORD_STEPS; }
inline __host__ __device__ int64_t dec_bytes(int n_cw, int nbits) {
    return (int64_t)dec_chunks(nbits) * dec_rows(n_cw) * 64 * 4;
}
// The energy-dispersal sequence on the device (fic-handler.cpp:100-108; dab-concurrent.cpp:
// 183-190 builds it for 24 * bitRate bits), 32 bits per word.  It covers the longest
// subchannel the 864 CUs of a CIF hold: EEP 4-B at 1824 kbit/s (855 CU; EEP 4-A ends at
// 1728 kbit/s, 864 CU).  A traceback reads the words of its chunks' bits, whole chunks, and
// one word beyond (tb_body's hi word): dabgpu_msc_deconvolve refuses a bitRate above this.
constexpr int MSC_MAX_BITRATE = 1824;
constexpr int PRBS_WORDS =
    ((24 * MSC_MAX_BITRATE + 6 + DEC_WORD_STEPS - 1) / DEC_WORD_STEPS * DEC_WORD_STEPS + 31) / 32 + 1;
// first word of (row, chunk 0); chunk c of the row is 4096 words further on
inline __host__ __device__ int64_t dec_word_index(int64_t row, int32_t nch) {
    return ((row >> 6) * nch * 64 + (row & 63)) * 64;
}

// depuncturing profile: up to 4 (L_i, PI_i) segments + the 24-bit PI_X tail
// (deconvolve.cpp:172-237, fic-handler.cpp:254-288)
struct Profile {
    int32_t nbits;          // decoded bits N; trellis steps N+6
    int32_t nseg;           // 0 = no puncturing (mother code given directly)
    uint32_t mask[4];       // PI vectors as 32-bit masks (bit j = P_Code[j])
    int32_t blk_end[4];     // cumulative 128-bit blocks at end of segment
    int32_t in_base[5];     // input soft-bit index at segment start / tail start
    uint32_t tail_mask;     // PI_X (24 bits)
    int32_t frag;           // punctured input length (fragment size)
    int32_t inv_off;        // its inverse table in VitJob::inv (input -> mother position)
};

enum SrcKind : int32_t {
    SRC_MOTHER = 0,         // contiguous depunctured stream, stride 4*(N+6)
    SRC_FRAG = 1,           // contiguous punctured fragments, stride frag_stride
    SRC_FIC = 2,            // FIC blocks inside the demod soft-bit buffer
    SRC_MSC = 3,            // MSC subchannels with 16-CIF time de-interleave from the ring
};

struct VitJob {
    int32_t kind;
    int32_t n_cw;
    const int16_t *src;
    int64_t src_len;        // elements readable from src (bounds check)
    int32_t *err;           // device error word
    int64_t src_stride;     // SRC_MOTHER / SRC_FRAG: elements per codeword
    const Profile *prof;    // per-profile table
    const int32_t *cw_prof; // SRC_FRAG: profile per codeword; else null (profile 0 / by subch)
    // SRC_FIC: codeword = 4*i + blk over slots[i]
    const int32_t *slots;
    // SRC_MSC: codeword = ((stream * ncif) + c) * nsub + sub
    int32_t nsub, ncif, ring;      // subchannels, CIF slots per stream in this batch, ring frames
    const int64_t *cif0s;           // [stream] CIF index (count delivered so far) of the batch's first CIF
    const int32_t *ncifs;           // [stream] CIFs of the batch the stream delivered (<= ncif)
    const int32_t *sub_start;       // startAddr*64 per subchannel (up to 55232: int32)
    // SRC_MSC with per-stream subchannel tables (ent_prof non-null; null: the shared table
    // above -- profile = sub, sub_start, delivery from CIF 16).  Entry e = stream * nsub + sub:
    const int32_t *ent_prof;        // [S * nsub] index into prof (distinct profiles), -1: absent entry
    const int32_t *ent_start;       // [S * nsub] startAddr*64
    const int64_t *ent_since;       // [S * nsub] the stream's CIF count when the entry was set:
                                    // it delivers CIF c once c - since >= 16
    // ACS and traceback decode the active entries only: codeword = act pair * ncif + CIF
    // over act[0..n_act) (entries e in (stream, sub) order), n_acs = n_act * ncif of them,
    // which is also the codeword's decision row; n_cw stays the padded output row count
    // S * ncif * nsub (rows of out: (stream * ncif + CIF) * nsub + sub)
    const int32_t *act;
    int32_t n_acs;
    // outputs
    uint32_t *dec;                  // decision words (dec_bytes(n_cw, max nbits) bytes)
    int64_t dec_ncw;                // rows of the decision buffer: >= dec_rows(n_cw)
    int32_t dec_nch;                // chunks per row: dec_chunks(max nbits)
    uint8_t *out;
    int64_t out_stride;             // bytes per codeword
    int32_t prbs;                   // xor energy-dispersal sequence
    int32_t packed;                 // out: 8 bits per byte, msb first (else one bit per byte)
    const uint32_t *prbs_words;     // PRBS packed 32 bits per word, bit i = prbs[32w+i]
    const uint8_t *valid;           // optional per-codeword flag: 0 = skip
    int32_t ring8;                  // SRC_FIC / SRC_MSC: src holds RING8 bytes (v + 127), not int16
    // SRC_MSC / SRC_FIC: inverse depuncturing tables, Profile::frag bytes per profile at
    // Profile::inv_off (make_inv): each input's mother-code position within its 60-step
    // tile (q mod VIT_TILE_POS); null: step-major loader
    const uint8_t *inv;
};

// DAB+ superframe layer (k_dabplus.hip)
constexpr int DP_MAX_RS = 48;       // RSDims = bitRate / 8, bitRate <= 384
constexpr int DP_TAB_BYTES = 256 + 256 + 512 + 2560 + 512 + 2048 + 516;   // GF exp/log, fire, mul[10], crc, pow8, fibcrc
constexpr int FIBCRC_OFF = 256 + 256 + 512 + 2560 + 512 + 2048;   // uint16 bit contribution[256] + init effect
struct DpState {
    int32_t fill, blocks;           // blockFillIndex, blocksInBuffer (mp4processor.cpp:86-87)
};
struct DpJob {
    MscFeed feed;
    SlotMapView map;                // [S][ndp] the DAB+ slots
    int32_t ndp;
    uint8_t *ring;                  // [S][ndp][120*DP_MAX_RS] 5-CIF byte rings
    DpState *state;                 // [S][ndp]
    uint8_t *code;                  // [S][ndp][ncif] scratch: 0 fire code failed, 2 rejected, 3 decoded
    uint8_t *sf_out;                // [S][ncif][ndp][sf_stride]
    int64_t sf_stride;
    dabgpu_superframe *info;        // [S][ncif][ndp]
    const uint8_t *tabs;            // DP_TAB_BYTES: GF exp, log, fire table, alpha^i multiply, CRC
    // compact output (dabgpu_pipe_set_dabplus_compact): the superframes that complete in
    // the run, per (stream, DAB+ subchannel) in CIF order, at sf_compact[(s*ndp+dp)*kmax+k]
    // (stride sf_stride); sf_out is then the pipeline's own sparse scratch
    uint8_t *sf_compact;
    int32_t kmax;
};

// MPEG layer II layer (k_mp2.hip)
constexpr int MP2_STATE_I16 = 2 * 15 * 64;  // a decoder's carried state: the last 15 V vectors per channel
struct Mp2Tabs {
    int32_t D[512];                 // the synthesis window (mp2processor.cpp:68-133)
    int16_t N[64 * 32];             // the matrixing coefficients (:229-233)
    uint8_t band[3][32];            // per quantisation table and subband: allocation bits << 4 | allocation row
    uint8_t rowq[6][16];            // per allocation row and allocation value: quantiser 1..17, 0 none
};
// n_chains decoders, chain_len frame slots each; frame j of chain i at frames + (i * chain_len
// + j) * stride (stride bytes readable, zeros beyond).  Its outputs lie at index
// (i / cdiv) * idx_a + (i % cdiv) * idx_b + j * idx_c of pcm ([1152][2] int16 each), ret and info.
struct Mp2Job {
    const uint8_t *frames;
    int64_t stride;
    int32_t n_chains, chain_len;
    const uint8_t *present;         // optional [n_chains][chain_len]: 0 = the slot holds no frame
    const int16_t *state_in;        // [n_chains][MP2_STATE_I16]; not the memory of state_out
    int16_t *state_out;
    int16_t *pcm;
    int32_t *ret;                   // optional: mp2decodeFrame's return value (0 for an empty slot)
    dabgpu_mp2_info *info;          // optional: status 1 / 2 and frame_bytes of the slots that hold a frame
    int32_t cdiv;
    int64_t idx_a, idx_b, idx_c;
    const Mp2Tabs *tabs;
};
struct Mp2SyncState {               // mp2Processor's synchroniser, zero for a new one
    int32_t ok, hc, bc;             // MP2Header_OK, MP2headerCount, MP2bitCount
    int32_t half_rate;              // baudRate: 0 48000, 1 24000
};
struct Mp2SyncJob {
    MscFeed feed;
    SlotMapView map;                // [S][nmp] the MP2 slots
    int32_t nmp;
    Mp2SyncState *state;            // [S][nmp]
    uint8_t *part;                  // [S][nmp][fstride] the frame being collected, packed
    uint8_t *frames;                // [S * nmp][ncif][fstride] the frame that completed in each CIF
    int32_t fstride;                // >= 6 * the largest bitRate
    uint8_t *present;               // [S * nmp][ncif]
    dabgpu_mp2_info *info;          // [S][ncif][nmp]
};

// packet-mode data layer (k_packet.hip)
constexpr int PK_MAX_CELLS = 48;    // 24-byte cells of a CIF at 384 kbit/s
struct PkState {                    // an mscDatagroup's assembler, {0, -1, 0, 0, 0, 0, 0, 0} for a new one
    int32_t state, address;         // packetState, streamAddress
    int32_t handled, crc_errors;    // the 500-packet window (show_crcErrors)
    int32_t pending;                // bytes of the series in flight (its first `cap` lie in the carry)
    int32_t prev_state, prev_pending;   // state and pending at the start of the last pass (k_pkt_copy)
    int32_t reserved;
};
struct PkJob {
    MscFeed feed;
    SlotMapView map;                // [S][npk] the packet slots
    int32_t npk;
    int32_t ncell;                  // cells per CIF the buffers hold: max_bitrate / 8
    int32_t cap;                    // max_group_bytes
    PkState *state;                 // [S][npk]
    const uint8_t *carry_in;        // [S][npk][cap] the series in flight before the run
    uint8_t *carry_out;             // ... and after it (not the memory of carry_in)
    uint32_t *rec;                  // [S * npk][ncif][ncell] packet records (k_pkt_scan)
    int2 *take;                     // [S * npk][ncif][ncell] x: bytes taken | series << 7, y: byte offset in the series
    int32_t *segtab;                // [S * npk][1 + ncif * ncell] per series of the run (0: the one carried in):
                                    //   its group's arena offset, -1 dropped, -2 still in flight
    uint8_t *bytes;                 // [S * npk][arena]
    int64_t arena;
    dabgpu_datagroup *groups;       // [S * npk][gslots]
    int32_t gslots;
    dabgpu_packet_run *run;         // [S * npk]
    dabgpu_packet_info *info;       // [S][ncif][npk]
};

// MOT layer (k_mot.hip): n_slots motHandlers over the groups of a packet-layer pass
constexpr int MOT_TABLE_BYTES = (int)(sizeof(dabgpu_mot_head) + DABGPU_MOT_ENTRIES * sizeof(dabgpu_mot_entry));
static_assert(sizeof(dabgpu_mot_head) == 16 && sizeof(dabgpu_mot_entry) == 184 && sizeof(dabgpu_mot_object) == 156 &&
                  sizeof(dabgpu_mot_run) == 32 && MOT_TABLE_BYTES % 16 == 0,
              "the MOT records are read as bytes by the bindings");
struct MotJob {
    int32_t n_slots;
    int32_t max_body;               // max_body_bytes
    int32_t body_cap;               // max_body rounded up to 16: an entry's body bytes in the state
    int64_t state_bytes;            // MOT_TABLE_BYTES + DABGPU_MOT_ENTRIES * body_cap
    uint8_t *state;                 // [n_slots][state_bytes]
    const int32_t *src;             // optional [n_slots]: the packet slot (row of groups / bytes / run) a MOT
                                    //   slot reads, -1: absent; NULL: slot i reads row i
    const dabgpu_datagroup *groups; // [rows][gslots]
    int32_t gslots;
    const uint8_t *bytes;           // [rows][arena]
    int64_t arena;                  // < 2^31
    const dabgpu_packet_run *run;   // [rows]
    dabgpu_mot_object *objects;     // [n_slots][gslots]
    uint8_t *out;                   // [n_slots][out_arena]
    int64_t out_arena;              // < 2^31
    dabgpu_mot_run *mot_run;        // [n_slots]
    int4 *ops;                      // [n_slots][2 * gslots] the pass's copy list: x kind, y source, z destination, w bytes
    int32_t *nops;                  // [n_slots]
};

// IP layer (k_ip.hip): n_slots ip_dataHandlers over the groups of a packet-layer pass, row i for slot i
static_assert(sizeof(dabgpu_ip_state) == 8 && sizeof(dabgpu_ip_result) == 16 && sizeof(dabgpu_ip_run) == 48,
              "the IP records are read as bytes by the bindings");
struct IpJob {
    int32_t n_slots;
    dabgpu_ip_state *state;         // [n_slots]
    const int32_t *on;              // optional [n_slots]: 0: the slot's entry is not flagged, its run is zeroed and
                                    //   nothing else is read or written; NULL: every slot is walked
    const dabgpu_datagroup *groups; // [n_slots][gslots]
    int32_t gslots;
    const uint8_t *bytes;           // [n_slots][arena]
    int64_t arena;                  // < 2^31
    const dabgpu_packet_run *run;   // [n_slots]
    dabgpu_ip_result *results;      // [n_slots][gslots]
    uint8_t *out;                   // [n_slots][out_arena]
    int64_t out_arena;              // < 2^31
    dabgpu_ip_run *ip_run;          // [n_slots]
};

// PAD layer (k_pad.hip): n_slots padHandlers, each over its AUs in order
constexpr int PAD_BUFFER = 8192;    // msc_dataGroupBuffer
struct PadState {                   // a padHandler's carried state; all zero: a new one
    int32_t last_appType, last_set; // last_appType, and whether anything has written it (rule 3)
    int32_t started, index, length; // a length indicator has been seen; msc_dataGroupIndex / msc_dataGroupLength
    int32_t hiwater;                // bytes of the buffer ever written (rule 3)
    int32_t charset, cs_set;
    int32_t remain, is_last, more;  // dynamicLabel's statics remainDataLength, isLastSegment, moreXPad
    int32_t text_nbytes, text_npieces;  // dynamicLabelText: the full counts
    int32_t reserved[3];
    uint8_t piece_len[DABGPU_PAD_LABEL_PIECES];
    uint8_t text[DABGPU_PAD_LABEL_BYTES];
    uint8_t buffer[PAD_BUFFER];
};
static_assert(sizeof(PadState) == 64 + 64 + 256 + 8192 && sizeof(PadState) % 16 == 0 && sizeof(dabgpu_pad_label) == 344 &&
                  sizeof(dabgpu_pad_run) == 64 && sizeof(dabgpu_datagroup) == 32,
              "the PAD records are read as bytes by the bindings");
struct PadJob {
    int32_t n_slots, n_aus;
    uint8_t *state;                 // [n_slots] PadState
    const uint8_t *aus;             // [n_slots][n_aus][au_stride]
    int64_t au_stride;
    const int32_t *len;             // [n_slots][n_aus] aac_frame_length, negative: skipped
    const int32_t *cif;             // optional [n_slots][n_aus]: the records' cif (NULL: the AU's index)
    // the pipeline's source instead of aus / len (info != NULL): the outputs of a dabgpu_pipe_dabplus call
    const dabgpu_superframe *info;  // [S][ncif][ndp]
    const uint8_t *sf;              // sparse [S][ncif][ndp][sf_stride], or compact [S][ndp][kmax][sf_stride]
    int32_t sf_stride, kmax;        // kmax 0: sparse
    int32_t ncif, ndp;
    const int32_t *src;             // [n_slots]: the DAB+ slot (s * ndp + j) a handler reads, -1: absent
    dabgpu_pad_label *labels;       // [n_slots][label_slots]
    int32_t label_slots;
    dabgpu_datagroup *groups;       // [n_slots][group_slots]
    int32_t group_slots;
    uint8_t *bytes;                 // [n_slots][arena]
    int64_t arena;                  // < 2^31
    dabgpu_pad_run *run;            // [n_slots]
};

// FIC layer (k_fib.hip): n_slots fib_processors, each over its FIBs in order
static_assert(sizeof(dabgpu_fic_subch) == 16 && sizeof(dabgpu_fic_component) == 20 && sizeof(dabgpu_fic_service) == 32 &&
                  sizeof(dabgpu_fic_table) == 848 && sizeof(dabgpu_fic_db) == 5232 && sizeof(dabgpu_fic_db) % 16 == 0 &&
                  sizeof(dabgpu_fic_event) == 32 && sizeof(dabgpu_fic_run) == 64,
              "the FIC records are read as bytes by the bindings");
struct FibJob {
    int32_t n_slots, n_fibs;
    dabgpu_fic_db *db;              // [n_slots], 16-byte aligned
    const uint8_t *fibs;            // slot s, FIB i at fibs + s * stride + i * (bit_src ? 256 : 32)
    int64_t stride;
    int32_t bit_src;                // the FIBs are one bit per byte (the pipeline's unpacked FIC)
    const uint8_t *ok;              // [n_slots][n_fibs]
    int32_t want;                   // DABGPU_SUBCH_MP2 | PACKET | MOT | PAD | IP
    dabgpu_fic_event *events;       // [n_slots][event_slots]
    int32_t event_slots;
    dabgpu_fic_table *table;        // [n_slots]
    dabgpu_fic_run *run;            // [n_slots]
};

// audio output layer (k_audio.hip)
struct AudioState {                 // an audioSink's interpolators, zero for a new sink
    uint32_t hist[3][2];            // per filter (16000, 24000, 32000): its last and last-but-one input pair, int16 (left | right << 16)
    uint32_t reserved[2];
};
static_assert(sizeof(AudioState) == DABGPU_AUDIO_STATE_BYTES, "dabgpu.h");
// n_chains sinks, chain_len calls each.  Chain c = (s, a) = (c / cdiv, c % cdiv); its call j
//   reads amount pairs at pcm + (s * in_a + j * in_c + m) * in_pairs * 2, m = src ? src[c] - s * in_c : 0
//   (src[c] < 0: the chain has no calls), and its rate and amount from rates / amounts[c * chain_len + j],
//   or, with info, from info[s * in_a + j * in_c + m]: status 2 -> (sample_rate, fixed_amount), else no call;
//   writes row r = s * out_a + j * out_c + a of samples ([out_pairs][2] floats each) and of n_out.
struct AudioJob {
    const int16_t *pcm;
    int64_t in_pairs, in_a, in_c;
    int32_t n_chains, chain_len, cdiv, fixed_amount;
    const int32_t *src;             // optional [n_chains]
    const int32_t *rates, *amounts; // [n_chains][chain_len], or
    const dabgpu_mp2_info *info;
    AudioState *state;              // [n_chains], updated in place by the second launch
    const float *coef;              // [3][5] (DABGPU_TABLE_AUDIO_FIR), device
    float *samples;
    int32_t *n_out;
    int64_t out_pairs, out_a, out_c;
};

// input rate conversion (k_rate.hip)
struct RateTab {                    // airspyHandler's two tables for one rate (host/rate_converter.h)
    float frac[2048];               // mapTable_float
    int16_t base[2048];             // mapTable_int
};
constexpr int RATE_LDS_BYTES = 16384;   // input samples a workgroup stages at a time, as the stream holds them
constexpr int RATE_GROUP = 64;          // streams per launch: their block counts travel as kernel arguments
// Stream s (< n_streams <= RATE_GROUP) holds its samples in `format` at sample src_stride * s of src; block
// b < blocks[s] of it (inputs M b .. M b + M) becomes samples out_stride * s + 2048 b .. + 2047 of out.  A
// workgroup does its block in `passes` pieces of 2048 / passes outputs (1, 2, 4 or 8: the caller's choice,
// so that a piece's input span fits RATE_LDS_BYTES).
struct RateJob {
    const void *src;
    int64_t src_stride;
    float *out;
    int64_t out_stride;
    const RateTab *tab;             // device
    int32_t *err;                   // device error word
    int32_t M, passes, n_streams;
    int32_t first[8], last[8];      // per piece: the first and last sample of the block it reads (from the table)
    int32_t blocks[RATE_GROUP];
};
hipError_t launch_rate_convert(hipStream_t st, int format, const RateJob &job);

// iq: samples in format fmt (DABGPU_IQ_*); frame descriptors count samples
hipError_t launch_prs_sync(hipStream_t st, const void *iq, int fmt, const dabgpu_frame *fr, int n, const OfdmTables &T,
                           int level, int32_t *si, float *mx, float *sm, bool general);
hipError_t launch_block0(hipStream_t st, const void *iq, int fmt, const dabgpu_frame *fr, int n, const OfdmTables &T,
                         int method, int16_t *corr, int16_t *snr, bool general);
// aux.si non-null: every frame is placed by its own findIndex (block0 = window +
// startIndex), reported through aux; else the descriptors' block0 / lp_data are used
hipError_t launch_demod(hipStream_t st, const void *iq, const dabgpu_frame *fr, int n, int nchunks,
                        const OfdmTables &T, int16_t *soft, float *softf, float *fcpart, bool general,
                        const DemodAux &aux);
hipError_t launch_nco_eval(hipStream_t st, const OfdmTables &T, int32_t first, int32_t n, float2 *out);
hipError_t launch_snr(hipStream_t st, const float *spec, int16_t *out);
hipError_t launch_symbol(hipStream_t st, const float *smp, int kind, const OfdmTables &T, float *spec, int16_t *ibits);
hipError_t launch_fc_reduce(hipStream_t st, const float *part, int nchunks, int n, float *out);
hipError_t launch_take_error(hipStream_t st, int32_t *err, int32_t *h_err);
hipError_t launch_front_publish(hipStream_t st, const float *part, int nchunks, int n, float *fc_d, float *h_fc,
                                const int32_t *si_d, int32_t *h_si, const int16_t *snr_d, int16_t *h_snr,
                                int32_t *err, int32_t *h_err);
hipError_t launch_acquire(hipStream_t st, const void *iq, int fmt, const AcqJob *jobs, int n, const float2 *osc,
                          AcqResult *res);
hipError_t launch_viterbi(hipStream_t st, const VitJob &job);
hipError_t launch_acs(hipStream_t st, const VitJob &job);
hipError_t launch_traceback(hipStream_t st, const VitJob &job);
hipError_t launch_acs_msc_fic(hipStream_t st, const VitJob &msc, const VitJob &fic);
hipError_t launch_traceback_msc_fic(hipStream_t st, const VitJob &msc, const VitJob &fic);
hipError_t launch_fic_post(hipStream_t st, uint8_t *bits, uint8_t *crc_ok, int n_fib, const uint8_t *tabs,
                           const int32_t *slots = nullptr, bool packed = false);
hipError_t launch_dabplus(hipStream_t st, const DpJob &job);
hipError_t launch_iq_convert(hipStream_t st, int format, const void *src, int64_t n_values, float *dst);
// device -> mapped pinned host memory by `wgs` workgroups; src, dst, bytes 16-byte aligned
hipError_t launch_to_host(hipStream_t st, const void *src, void *dst, size_t bytes, int wgs);
hipError_t launch_rs(hipStream_t st, const uint8_t *in, int n, const uint8_t *tabs, uint8_t *out, int16_t *ret);
hipError_t launch_mp2_decode(hipStream_t st, const Mp2Job &job);
hipError_t launch_mp2_sync(hipStream_t st, const Mp2SyncJob &job);
hipError_t launch_packet(hipStream_t st, const PkJob &job);
hipError_t launch_mot(hipStream_t st, const MotJob &job);
hipError_t launch_ip(hipStream_t st, const IpJob &job);
hipError_t launch_pad(hipStream_t st, const PadJob &job);
hipError_t launch_audio(hipStream_t st, const AudioJob &job);
hipError_t launch_fib(hipStream_t st, const FibJob &job);
hipError_t launch_fic_clear(hipStream_t st, dabgpu_fic_db *db, int n_slots);

}  // namespace dab
