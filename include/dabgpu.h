/*
 * dabgpu.h -- C ABI of the MI355X-native DAB Mode-I demod/decode path.
 *
 * Plain C: pointers, sizes and PODs only (no HIP or torch types), so a C++
 * drop-in for sdr-j-dab's ofdmProcessor / ficHandler / mscHandler, a ctypes
 * or a cgo binding can all call it.  Every entry point names the reference
 * interface it replaces (paths relative to the sdr-j-dab v0.997 tree).
 *
 * Conventions
 *  - return value: 0 on success, a negative DABGPU_E* code on failure; the
 *    message of the last failure on this thread is dabgpu_last_error().
 *    No C++ exception crosses this boundary.
 *  - "_d" pointers are device (HBM) pointers obtained from dabgpu_alloc or
 *    any HIP allocation on the context's device; "_h" pointers are host.
 *  - every device-side call is asynchronous on the context's stream;
 *    dabgpu_sync() waits.  Calls that return host data synchronise.
 *  - one context per calling thread (contexts are independent streams).
 *  - data formats follow the reference: IQ is interleaved cf32 (re, im)
 *    scaled to about +-1 (virtual-input.h:51-70); soft bits are int16 in
 *    [-127, 127] (ofdm-decoder.cpp:186-189); decoded bits are one bit per
 *    uint8 (viterbi.cpp:240-241).
 */
#ifndef DABGPU_H
#define DABGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DABGPU_ABI_VERSION 7

/* error codes */
#define DABGPU_OK          0
#define DABGPU_E_ARG      -1   /* invalid argument / shape */
#define DABGPU_E_HIP      -2   /* HIP runtime error */
#define DABGPU_E_NODEV    -3   /* no usable gfx950 device */
#define DABGPU_E_NOMEM    -4
#define DABGPU_E_UNSUP    -5   /* configuration the reference does not define */
#define DABGPU_E_STATE    -6   /* call out of sequence */
#define DABGPU_E_BOUNDS   -7   /* a kernel refused a descriptor that points outside its stream */

/* Mode-I geometry (gui.cpp:1361-1371) */
#define DABGPU_TU     2048
#define DABGPU_TS     2552
#define DABGPU_TG     504
#define DABGPU_TNULL  2656
#define DABGPU_TF     196608
#define DABGPU_K      1536
#define DABGPU_L      76
#define DABGPU_CIF_BITS 55296

typedef struct dabgpu_ctx dabgpu_ctx;

/* Subchannel of the MSC, as produced by the FIB parser (dab-constants.h:151-176,
 * audiodata/packetdata: startAddr, length in CUs, uepFlag, protLevel, bitRate).
 * uepFlag == 0 selects UEP (deconvolve.cpp:130); otherwise protLevel carries
 * 0100|level (EEP-A) or 0200|level (EEP-B). */
typedef struct {
    int16_t startAddr;
    int16_t length;
    int16_t bitRate;
    int16_t protLevel;
    int16_t uepFlag;
    int16_t flags;          /* DABGPU_SUBCH_DABPLUS: feed the DAB+ superframe layer;
                               DABGPU_SUBCH_MP2: feed the MPEG layer II layer */
} dabgpu_subch;
#define DABGPU_SUBCH_DABPLUS 1
#define DABGPU_SUBCH_RAW     2   /* dabgpu_msc_deconvolve: no energy dispersal (the bare
                                    uep_/eep_deconvolve::deconvolve output) */
#define DABGPU_SUBCH_MP2     4   /* feed the MPEG layer II layer (dabgpu_pipe_mp2); not together
                                    with DABGPU_SUBCH_DABPLUS on one entry (DABGPU_E_ARG) */

#define DABGPU_SUBCH_PACKET  8   /* feed the packet-mode data layer (dabgpu_pipe_packet); not together
                                    with DABGPU_SUBCH_DABPLUS or DABGPU_SUBCH_MP2 on one entry
                                    (DABGPU_E_ARG); bitRate a multiple of 8 in [8, max_bitrate]
                                    (DABGPU_E_UNSUP otherwise) */

/* One CIF of one packet-mode subchannel through mscDatagroup::handlePackets
 * (msc-datagroup.cpp:221-319, show_crcErrors on). */
typedef struct {
    int16_t status;         /* -1 CIF not delivered or inside the entry's warm-up, 0 fed */
    int16_t packets;        /* packets handlePackets walked in this CIF */
    int16_t crc_errors;     /* ... of which check_CRC_bits refused */
    int16_t groups;         /* data groups completed in this CIF */
    int16_t quality;        /* what show_mscErrors emits in this CIF (100 - crcErrors / 5 when the
                               carried count of handled packets reaches 500, :250-254), else -1 */
    int16_t address;        /* streamAddress after the CIF, -1 before the latch */
} dabgpu_packet_info;
/* One (stream, packet slot) after a run */
typedef struct {
    int32_t n_groups;       /* groups completed in the run */
    int32_t n_bytes;        /* their stored bytes, packed back to back from offset 0 */
    int32_t state;          /* packetState after the run */
    int32_t pending_bytes;  /* length of the series in flight (0 in state 0) */
} dabgpu_packet_run;
/* One completed MSC data group: what my_dataHandler->add_mscDatagroup receives, as bytes, and
 * the generic header as mot_databuilder::add_mscDatagroup parses it (mot-databuilder.cpp:37-95) */
typedef struct {
    int32_t cif;            /* slot in the run of the packet that completed the group */
    int32_t offset;         /* of its first byte in the (stream, slot)'s arena */
    int32_t nbytes;         /* its length (stored: min(nbytes, max_group_bytes)) */
    int32_t data_offset;    /* the reference's next / 8: header bytes before the data field */
    int32_t data_nbytes;    /* the reference's sizeinBits / 8 (in int32), 0 when it would be negative */
    uint16_t flags;         /* DABGPU_DG_* */
    uint16_t segmentNumber;
    uint16_t transportId;
    uint8_t groupType;
    uint8_t CI;
    uint8_t lengthInd;
    uint8_t reserved[3];
} dabgpu_datagroup;
#define DABGPU_DG_EXTENSION   1
#define DABGPU_DG_CRC         2     /* the CRC flag */
#define DABGPU_DG_SEGMENT     4
#define DABGPU_DG_USER_ACCESS 8
#define DABGPU_DG_LAST        16    /* last segment */
#define DABGPU_DG_TRANSPORT   32    /* transport-id flag */
#define DABGPU_DG_ACCEPTED    64    /* nbytes > 0, not truncated, and no CRC flag or a good CRC:
                                       the groups add_mscDatagroup goes on with */
#define DABGPU_DG_TRUNCATED   128
#define DABGPU_PKT_GROUP_BYTES 8216 /* the default max_group_bytes: 2 + 2 + 2 + 16 header bytes,
                                       8191 data bytes and 2 CRC bytes, rounded up to 8 */
#define DABGPU_PKT_GROUP_SLOTS(n_frames, max_bitrate) (4 * (n_frames) * ((max_bitrate) / 8))
#define DABGPU_PKT_ARENA_BYTES(n_frames, max_bitrate, max_group_bytes) \
    ((max_group_bytes) + 4 * (n_frames) * ((max_bitrate) / 8) * 127)

#define DABGPU_SUBCH_MOT     16  /* feed the packet entry's data groups to the MOT layer (dabgpu_pipe_mot);
                                    only together with DABGPU_SUBCH_PACKET (DABGPU_E_ARG otherwise) */
/* One object motHandler delivered (mot-data.cpp:315-346): a slide where show_slide emits
 * the_picture, a file where handleComplete fopens, or an EPG object (contentType 7:
 * handle_epgTopElement returns at once, :355 -- recorded, no bytes). */
#define DABGPU_MOT_NAME_BYTES 128
typedef struct {
    int32_t group;          /* index, in the run's groups, of the group that completed the object */
    int32_t cif;            /* that group's cif */
    int32_t offset;         /* of the body in the (stream, slot)'s output arena, a multiple of 16 */
    int32_t nbytes;         /* bodySize; 0 for DABGPU_MOT_EPG and with DABGPU_MOT_OVERFLOW */
    uint16_t transportId;
    uint8_t contentType;
    uint8_t kind;           /* DABGPU_MOT_SLIDE, DABGPU_MOT_EPG or DABGPU_MOT_FILE */
    uint16_t contentsubType;
    uint16_t flags;         /* DABGPU_MOT_OVERFLOW */
    int32_t name_len;       /* the name's full length; name holds its first DABGPU_MOT_NAME_BYTES bytes */
    uint8_t name[DABGPU_MOT_NAME_BYTES];
} dabgpu_mot_object;
#define DABGPU_MOT_SLIDE 1
#define DABGPU_MOT_EPG   2
#define DABGPU_MOT_FILE  3
#define DABGPU_MOT_TOO_LARGE 1      /* dabgpu_mot_entry.flags: bodySize above max_body_bytes */
#define DABGPU_MOT_OVERFLOW  2      /* dabgpu_mot_object.flags: the body did not fit the output arena */
/* One (stream, MOT slot) after a run */
typedef struct {
    int32_t n_objects;      /* objects delivered in the run */
    int32_t n_bytes;        /* output arena bytes used */
    int32_t malformed;      /* groups dropped by rule 1 (or whose record points outside its arena) */
    int32_t bad_segment;    /* groups dropped by rule 2 */
    int32_t other_types;    /* groups that are neither a header (type 3, segment 0) nor type 4 (rule 6) */
    int32_t entries;        /* table entries in use after the run */
    int32_t reserved[2];
} dabgpu_mot_run;
/* A motHandler's carried state: this head, DABGPU_MOT_ENTRIES entries, then the entries'
 * bodies, each in (max_body_bytes rounded up to 16) bytes.  All zero is a new motHandler. */
#define DABGPU_MOT_ENTRIES 16
typedef struct {
    int32_t created;        /* entries made so far: the reference's ordernumber - 1 */
    int32_t old_slide;      /* 1 once a slide has been shown (old_slide != NULL) */
    int32_t reserved[2];
} dabgpu_mot_head;
typedef struct {            /* a motElement (mot-data.h:33-44) */
    int32_t order;          /* ordernumber; 0: free (the reference's -1) */
    int32_t transportId;
    int32_t bodySize;
    int32_t segmentSize;    /* -1 until a segment that is not the last latched it */
    int32_t numofSegments;  /* -1 until the last segment set it */
    int32_t contentType, contentsubType;
    int32_t flags;          /* DABGPU_MOT_TOO_LARGE */
    uint32_t marked[4];     /* bit n: segment n is in (as in the reference, newEntry leaves them) */
    int32_t name_len;
    int32_t reserved;
    uint8_t name[DABGPU_MOT_NAME_BYTES];
} dabgpu_mot_entry;
#define DABGPU_MOT_BODY_BYTES 65536 /* the default max_body_bytes */
/* Object slots and output arena bytes per (stream, MOT slot): a run completes at most one
 * object per group; the arena holds one carried body plus what a run's payload can complete,
 * each body at a multiple of 16 (127 payload bytes a packet and up to 15 bytes of alignment a
 * group; the size stays a multiple of 16).  A run can complete more only when several entries were
 * each left one segment short on purpose -- a hostile stream: such an object is recorded with
 * DABGPU_MOT_OVERFLOW and no bytes. */
#define DABGPU_MOT_OBJECT_SLOTS(n_frames, max_bitrate) DABGPU_PKT_GROUP_SLOTS(n_frames, max_bitrate)
#define DABGPU_MOT_ARENA_FOR(group_slots, max_body_bytes) \
    ((((max_body_bytes) + 15) / 16) * 16 + (group_slots) * 144)
#define DABGPU_MOT_ARENA_BYTES(n_frames, max_bitrate, max_body_bytes) \
    DABGPU_MOT_ARENA_FOR(DABGPU_PKT_GROUP_SLOTS(n_frames, max_bitrate), max_body_bytes)

#define DABGPU_SUBCH_IP      64  /* feed the packet entry's data groups to the IP layer (dabgpu_pipe_ip); only together
                                    with DABGPU_SUBCH_PACKET, not together with DABGPU_SUBCH_MOT (one my_dataHandler
                                    per mscDatagroup): DABGPU_E_ARG otherwise */
/* An ip_dataHandler's carried state (ip-datahandler.cpp:100-104, show_crcErrors on).  All zero: a new one. */
typedef struct {
    int32_t handled;        /* handledPackets */
    int32_t crc_errors;     /* crcErrors */
} dabgpu_ip_state;
/* What ip_dataHandler::add_mscDatagroup did with one group of the run; index = the group's index */
typedef struct {
    int32_t offset;         /* of the payload in the slot's output arena, a multiple of 16; 0 unless delivered */
    int32_t nbytes;         /* payload length (ipLength - 4 * headerSize - 8); 0 unless delivered */
    int16_t status;         /* DABGPU_IP_* */
    int16_t quality;        /* what show_ipErrors emits inside this group's call (100 - crcErrors), else -1 */
    int32_t ip_bytes;       /* ipLength, 0 when the group never got that far */
} dabgpu_ip_result;
#define DABGPU_IP_DELIVERED    0   /* writeDatagram: the UDP payload */
#define DABGPU_IP_NOT_ACCEPTED 1   /* no DABGPU_DG_ACCEPTED (:54), or rule 5 */
#define DABGPU_IP_TOO_LONG     2   /* ipLength >= the group's bytes (:80) */
#define DABGPU_IP_NOT_V4       3   /* (:85), or rule 2 */
#define DABGPU_IP_CHECKSUM     4   /* the header checksum (:108): counted in crcErrors */
#define DABGPU_IP_NOT_UDP      5   /* protocol != 17 (:117) */
#define DABGPU_IP_MALFORMED    6   /* rules 3 and 6 */
/* One (stream, packet slot) after a run */
typedef struct {
    int32_t n_datagrams;    /* groups that ended DABGPU_IP_DELIVERED */
    int32_t n_bytes;        /* their payload bytes */
    int32_t counts[7];      /* groups by status */
    int32_t reserved[3];
} dabgpu_ip_run;
/* Output arena bytes per slot: every payload lies inside its group, and each starts at a multiple of 16 */
#define DABGPU_IP_ARENA_FOR(group_slots, arena_bytes) ((arena_bytes) + 16 * (group_slots))

#define DABGPU_SUBCH_PAD     32  /* feed the DAB+ entry's good AUs to the PAD layer (dabgpu_pipe_pad); only together
                                    with DABGPU_SUBCH_DABPLUS (DABGPU_E_ARG otherwise).  PAD slot j of a stream is
                                    its j-th entry so flagged. */
#define DABGPU_SUBCH_AUDIO   128 /* feed the layer II entry's decoded frames to the audio output layer
                                    (dabgpu_pipe_audio); only together with DABGPU_SUBCH_MP2 (DABGPU_E_ARG
                                    otherwise).  Audio slot j of a stream is its j-th entry so flagged. */
/* One showLabel emission of padHandler::dynamicLabel (pad-handler.cpp:231-267).  text holds the
 * bytes the reference passed to toQStringUsingCharset, piece after piece, since the last clear,
 * unconverted; charset is charSet at the emission; piece_len keeps the boundaries of those
 * calls, so a caller that owns the reference's charsets.cpp reproduces the QString exactly:
 * clear, then append the conversion of each piece.  (No character table is part of the product.) */
#define DABGPU_PAD_LABEL_BYTES  256
#define DABGPU_PAD_LABEL_PIECES 64
typedef struct {
    int32_t cif;            /* of the AU that completed the label (dabgpu_pad_aus: see cif_d; dabgpu_pipe_pad: the
                               CIF slot in the run of the AU's superframe) */
    int32_t au;             /* that AU's index: in the call (dabgpu_pad_aus), in its superframe (dabgpu_pipe_pad) */
    int32_t charset;
    int32_t nbytes;         /* the full length; text holds the first DABGPU_PAD_LABEL_BYTES */
    int32_t n_pieces;       /* the full count; piece_len holds the first DABGPU_PAD_LABEL_PIECES */
    int32_t flags;          /* DABGPU_PAD_LABEL_TRUNCATED */
    uint8_t piece_len[DABGPU_PAD_LABEL_PIECES];     /* each piece's full length (1..48) */
    uint8_t text[DABGPU_PAD_LABEL_BYTES];
} dabgpu_pad_label;
#define DABGPU_PAD_LABEL_TRUNCATED 1
/* One padHandler after a dabgpu_pad_aus call */
typedef struct {
    int32_t n_labels;       /* labels shown in the run (records: the first label_slots of them) */
    int32_t n_groups;       /* X-PAD data groups completed (records: the first group_slots) */
    int32_t n_bytes;        /* their stored bytes, packed back to back from offset 0 */
    int32_t aus;            /* good AUs seen (length >= 0) */
    int32_t pads;           /* processPAD calls: AUs that open with a data stream element */
    int32_t unhandled;      /* PADs left at the first application type outside {1, 2, 3, 12, 13} (:141-145) */
    int32_t undefined[4];   /* PADs that met rule 1, 2, 3, 4 of dabgpu_pad_aus (a PAD counts once per rule) */
    int32_t crc_failed;     /* completed groups whose pad_crc failed */
    int32_t guard_dropped;  /* sub-fields add_MSC_element dropped at its 8192 guard (:285-288) */
    int32_t rejected_sf;    /* dabgpu_pipe_pad: status-2 superframes skipped (their AUs are not stored); else 0 */
    int32_t reserved[3];
} dabgpu_pad_run;
/* Sizes per padHandler for the AUs a run of n_frames frames can complete: a superframe holds at most 6 AUs;
 * a PAD carries at most four content indicators, and each sub-field shows at most one label or
 * completes at most one group; a group's bytes never exceed what was appended since its length
 * indicator: at most 8191 bytes carried, plus 4 x 48 bytes per AU. */
#define DABGPU_PAD_AU_SLOTS(n_frames)    (DABGPU_SF_SLOTS(n_frames) * 6)
#define DABGPU_PAD_LABEL_SLOTS(n_frames) (4 * DABGPU_PAD_AU_SLOTS(n_frames))
#define DABGPU_PAD_GROUP_SLOTS(n_frames) (4 * DABGPU_PAD_AU_SLOTS(n_frames))
#define DABGPU_PAD_ARENA_BYTES(n_frames) ((8192 + DABGPU_PAD_AU_SLOTS(n_frames) * 192 + 15) / 16 * 16)

/* One CIF of one classic-audio subchannel through mp2Processor::addtoFrame
 * (mp2processor.cpp:572-617) and, when a frame completed in it, mp2decodeFrame (:365-568). */
typedef struct {
    int32_t status;         /* -1 CIF not delivered or inside the entry's warm-up, 0 no frame completed
                               in this CIF, 1 a frame completed and its header was rejected, 2 decoded */
    int32_t sample_rate;    /* status >= 1: baudRate when the frame was handed over (48000 or 24000) */
    int32_t frame_bytes;    /* status 2: mp2decodeFrame's return value */
} dabgpu_mp2_info;
/* a decoder's carried state (the last 15 V vectors of both channels), opaque */
#define DABGPU_MP2_STATE_BYTES 3840

/* an audioSink's carried state (the last input pairs of its three interpolators), opaque */
#define DABGPU_AUDIO_STATE_BYTES 32

/* One CIF of one DAB+ subchannel through mp4Processor::addtoFrame
 * (mp4processor.cpp:107-145) and, when five blocks are buffered and the fire
 * code holds, processSuperframe (:146-292). */
typedef struct {
    int8_t  status;         /* -1 CIF not delivered (de-interleaver warm-up), 0 fewer than 5
                               blocks buffered, 1 fire code failed, 2 superframe rejected
                               (RS failure or impossible AU table), 3 superframe decoded */
    int8_t  num_aus;        /* AUs in the superframe (2, 3, 4 or 6) */
    int16_t n_corrected;    /* RS symbols corrected (sum over the RSDims codewords) */
    int16_t au_start[7];    /* au_start[0..num_aus] */
    uint8_t au_crc_ok;      /* bit i: AU i passed dabPlus_crc */
    uint8_t reserved;       /* compact output: the superframe's slot (0xFF: none); else 0 */
} dabgpu_superframe;

/* Per-frame front-end parameters (ofdm-processor.cpp:344-446), one per
 * (stream, frame).  Sample indices are relative to the stream's base.
 * The NCO follows getSamples: for the k-th sample read in a segment
 * (k = 1, 2, ...), localPhase = (lp - k*phase) mod 2048000 and the
 * sample is multiplied by oscillatorTable[localPhase]. */
typedef struct {
    int64_t iq_base;    /* sample offset of the stream in the IQ buffer */
    int64_t n_samples;  /* samples of this stream readable from iq_base (bounds check) */
    int64_t window;     /* first sample of the T_u sync window (SyncOnPhase) */
    int64_t block0;     /* first sample of block 0 = window + startIndex */
    int32_t lp_window;  /* localPhase before the window's first sample */
    int32_t phase_a;    /* coarse+fine while reading window and PRS (segment A) */
    int32_t lp_data;    /* localPhase before the first data-symbol sample */
    int32_t phase_b;    /* coarse+fine while reading symbols 1..75 (segment B) */
    int32_t out_slot;   /* output frame slot in the soft-bit buffer */
    int32_t flags;      /* bit0: run coarse AFC (f2Correction) in block0 */
} dabgpu_frame;

/* ---- host-side tables (no device needed; for pinning against the reference) --
 *   DABGPU_TABLE_PRS     float2[2048] refTable (phasereference.cpp:40-47), natural order
 *   DABGPU_TABLE_MAPPER  int16[1536]  permVector::mapIn (mapper.cpp:33-117)
 *   DABGPU_TABLE_REFARG  float[18]    refArg (ofdm-decoder.cpp:71-74)
 *   DABGPU_TABLE_OSC     float2[2048000] oscillatorTable (ofdm-processor.cpp:79-81)
 *   DABGPU_TABLE_NCO     double2[384] the factor tables the kernels rebuild
 *                        oscillatorTable from (128 e^{2pi i a/128}, 125 e^{2pi i b/16000},
 *                        128 e^{2pi i c/2048000}, 3 zero)
 *   DABGPU_TABLE_AUDIO_FIR float[3][5] the kernels of audioSink's LowPassFIR (5, 16000, 48000),
 *                        (5, 24000, 48000) and (5, 32000, 96000), in this order
 *                        (fir-filters.cpp:35-69) */
#define DABGPU_TABLE_PRS    1
#define DABGPU_TABLE_MAPPER 2
#define DABGPU_TABLE_REFARG 3
#define DABGPU_TABLE_OSC    4
#define DABGPU_TABLE_NCO    5
#define DABGPU_TABLE_AUDIO_FIR 6
int dabgpu_host_table(int which, void *out_h, size_t bytes);
/* The depuncturing profile the decoder uses for a subchannel (deconvolve.cpp:142-366;
 * uep_deconvolve's unknown-profile fallback to table row 1, :148-151): decoded bits,
 * fragment size consumed, and the non-empty (L_i blocks of 128, PI_i) segments in
 * order.  Returns 0, 1 when the UEP (bitRate, level) is not in the table (fallback),
 * DABGPU_E_UNSUP when the protection is undefined. */
int dabgpu_subch_profile(const dabgpu_subch *s, int32_t *nbits, int32_t *frag_size, int32_t *nseg,
                         int32_t *L /*[4]*/, int32_t *PI /*[4]*/);

/* ---- context ---------------------------------------------------------- */
int         dabgpu_abi_version(void);
const char *dabgpu_last_error(void);
int         dabgpu_device_count(void);
int         dabgpu_ctx_create(int device, dabgpu_ctx **out);
int         dabgpu_ctx_destroy(dabgpu_ctx *ctx);
int         dabgpu_sync(dabgpu_ctx *ctx);
int         dabgpu_alloc(dabgpu_ctx *ctx, size_t bytes, void **dptr);
int         dabgpu_free(dabgpu_ctx *ctx, void *dptr);
int         dabgpu_memcpy_h2d(dabgpu_ctx *ctx, void *dst_d, const void *src_h, size_t bytes);
int         dabgpu_memcpy_d2h(dabgpu_ctx *ctx, void *dst_h, const void *src_d, size_t bytes);
int         dabgpu_memset_d(dabgpu_ctx *ctx, void *dst_d, int value, size_t bytes);
/* page-locked host memory (DMA without the pageable bounce: dabgpu_pipe_fetch targets) */
int         dabgpu_host_alloc(dabgpu_ctx *ctx, size_t bytes, void **h);
int         dabgpu_host_free(dabgpu_ctx *ctx, void *h);
/* device-to-device copy on the context stream (asynchronous; regions must not overlap) */
int         dabgpu_memcpy_d2d(dabgpu_ctx *ctx, void *dst_d, const void *src_d, size_t bytes);
/* HIP events on the context stream, for timing (ms between two marks) */
int         dabgpu_event_record(dabgpu_ctx *ctx, int slot);
/* device-side bounds violations flagged by kernels since the last call (syncs; clears) */
int         dabgpu_kernel_errors(dabgpu_ctx *ctx);
int         dabgpu_event_elapsed(dabgpu_ctx *ctx, int slot_a, int slot_b, float *ms);

/* ---- recorded IQ formats ---------------------------- */
/* Convert device-resident recorded samples to the interleaved cf32 IQ every OFDM
 * entry point reads, with the reference file readers' scaling:
 *   DABGPU_IQ_U8   .raw: rawFiles::getSamples (rawfiles.cpp:100-118),
 *                  I/Q = float(x - 128) / 128.0
 *   DABGPU_IQ_S16  .sdr: 2-channel PCM16 WAV at 2.048 MHz, wavFiles (wavfiles.cpp:
 *                  64-69, readBuffer) through libsndfile's sf_readf_float: x / 32768
 * n_pairs I/Q pairs: src_d holds 2*n_pairs values, iq_d receives 2*n_pairs floats.
 * Asynchronous on the context stream (dabgpu_sync to wait). */
#define DABGPU_IQ_F32  0   /* interleaved cf32: what every entry point reads by default */
#define DABGPU_IQ_U8   1
#define DABGPU_IQ_S16  2
int dabgpu_iq_convert(dabgpu_ctx *ctx, int format, const void *src_d, int64_t n_pairs, float *iq_d);

/* ---- input rate conversion ------------------------------------------- */
/* Streams sampled at in_rate Hz to the 2.048 MHz cf32 every OFDM entry point reads: the linear
 * interpolation of airspyHandler::data_available (airspy-handler.cpp:138-148, 333-359), bit for
 * bit.  With M = in_rate / 1000, block b of a stream reads its samples M b .. M b + M and writes
 * its outputs 2048 b .. 2048 b + 2047:
 *   out[2048 b + j] = x[M b + base[j] + 1] * frac[j] + x[M b + base[j]] * (1.0f - frac[j])
 * (base / frac: the handler's mapTable_int / mapTable_float; every product, the difference and the
 * sum rounded to fp32 on its own).  Stream s holds n_in_h[s] samples in `format` at sample
 * src_stride * s of src_d and gets B = (n_in_h[s] < 1 ? 0 : (n_in_h[s] - 1) / M) blocks: its
 * output goes to sample iq_stride * s of iq_d (strides in I/Q pairs, as in dabgpu_pipe_run),
 * n_out_h[s] = 2048 B, n_used_h[s] = M B, and nothing past its n_out_h[s] samples is written.
 * Sample n_used_h[s] is the first sample of the stream's next call: there is no device-side state.
 * format: DABGPU_IQ_S12 (the handler's own), DABGPU_IQ_F32 (the samples as they are: cf32
 * recordings at another rate), DABGPU_IQ_S16 / DABGPU_IQ_U8 with dabgpu_iq_convert's scalings;
 * the arithmetic after the conversion to float is the same for all four.
 * DABGPU_E_ARG: in_rate no multiple of 1000 or outside 2048000 .. 10000000, an unknown format,
 * n_streams < 1, a negative count, iq_stride < 2048 B or src_stride < n_in_h[s] for some stream,
 * src_d or iq_d not aligned to one I/Q pair of its type.  Asynchronous on the context stream
 * (n_out_h / n_used_h are set on return and n_in_h is read before it; dabgpu_sync to wait for
 * the samples). */
#define DABGPU_IQ_S12 3   /* int16 I/Q pairs holding the Airspy's 12-bit samples: x / 2048
                             (airspy-handler.cpp:340-341); rate conversion only */
int dabgpu_rate_convert(dabgpu_ctx *ctx, int in_rate, int format,
                        const void *src_d, int64_t src_stride, int n_streams, const int64_t *n_in_h,
                        float *iq_d, int64_t iq_stride, int64_t *n_out_h, int64_t *n_used_h);

/* ---- OFDM front end (L3) ---------------------------------------------- */

/* phaseReference::findIndex batched (phasereference.cpp:60-88): for each of n
 * frames, FFT of the NCO-mixed T_u window, x conj(PRS), IFFT, argmax |.|.
 * start_index[i] follows the reference: argmax, or -|Max/mean|-1 (truncated)
 * when Max < level*mean.  maxv/sumv (optional) receive Max and sum |.|. */
int dabgpu_prs_sync(dabgpu_ctx *ctx, const float *iq_d, const dabgpu_frame *frames_d, int n,
                    int16_t level, int32_t *start_index_d, float *maxv_d, float *sumv_d);

/* ofdmDecoder::processBlock_0 batched (ofdm-decoder.cpp:85-162): FFT of block 0,
 * snr_d[i] (optional) = get_snr (ofdm-decoder.cpp:212-230), and when
 * frames[i].flags&1 the coarse offset estimate of freqSyncMethod `method`
 * (0 getMiddle, 1 phase-difference correlation, 2 pattern match), else 0. */
int dabgpu_block0(dabgpu_ctx *ctx, const float *iq_d, const dabgpu_frame *frames_d, int n, int method,
                  int16_t *correction_d, int16_t *snr_d);

/* ofdmDecoder::processToken for symbols 1..75 of n frames (ofdm-decoder.cpp:167-190):
 * FFT, x conj(previous symbol), frequency de-interleave (mapper.cpp:115),
 * ibits = (int16)(-re/(|re|+|im|)*127).  Output layout
 *   softbits_d[out_slot][75][3072]  (FIC = symbols 1..3, CIF c = symbols 4+18c..21+18c)
 * softf_d (optional, same layout, float -re/|.|, -im/|.|) for parity tests.
 * freqcorr_d (optional) float2[n]: sum over the frame of x[i]*conj(x[i-T_u]),
 * i in [T_u, T_s) (ofdm-processor.cpp:424-438), in unspecified float order. */
int dabgpu_ofdm_demod(dabgpu_ctx *ctx, const float *iq_d, const dabgpu_frame *frames_d, int n,
                      int16_t *softbits_d, float *softf_d, float *freqcorr_d);

/* The north-star fused front end, one workgroup per frame (k_demod_wg<.., SYNC>):
 * findIndex on the frame's T_u window (phasereference.cpp:60-88, threshold `level`;
 * start_index_d[i] as dabgpu_prs_sync), the frame placed at block0 = window +
 * startIndex with lp_data following getSamples (ofdm-processor.cpp:344-368),
 * get_snr of block 0 (snr_d, optional, ofdm-decoder.cpp:93) and processToken x 75
 * as dabgpu_ofdm_demod.  frames[i].block0 / lp_data are ignored; a frame whose
 * findIndex fails or whose symbols lie past n_samples is skipped (no soft bits). */
int dabgpu_ofdm_sync_demod(dabgpu_ctx *ctx, const float *iq_d, const dabgpu_frame *frames_d, int n, int16_t level,
                           int32_t *start_index_d, int16_t *snr_d, int16_t *softbits_d, float *softf_d,
                           float *freqcorr_d);

/* The kernels' NCO: oscillatorTable[first .. first+n-1] as the front-end kernels
 * compute it (float2 into out_d) -- for checking it against the table exhaustively. */
int dabgpu_nco_eval(dabgpu_ctx *ctx, int32_t first, int32_t n, float *out_d);
/* Test hook of the fused demod's NCO and FFT (getSamples' v *= oscillatorTable[localPhase],
 * ofdm-processor.cpp:76-81,202-226; fft.cpp:53-121): the demod with `chunks` workgroups per
 * frame (1: one recurrence over all 75 symbols, as the pipeline runs C3) that also writes
 * every data symbol's mixed FFT input, mix_d[out_slot][75][2048] cf32 (the samples
 * [T_g, T_s) of symbol l after the NCO), and that FFT's output, spec_d[out_slot][75][2048]
 * in natural bin order, both in absolute units (format's scale taken out, exactly), for
 * comparison with the reference's table and with the transform restated.
 *   start_index_d == NULL: the operator form (dabgpu_ofdm_demod: cf32 in, frames give
 *     block0 / lp_data, int16 soft bits [out_slot][75][3072] into softbits_d);
 *   start_index_d != NULL: the streaming pipeline's instantiation -- findIndex on the
 *     window (threshold `level`, as dabgpu_ofdm_sync_demod), samples read as `format`
 *     (DABGPU_IQ_F32 / S16 / U8) and converted in the loads, RING8 soft-bit bytes
 *     (ibits + 127, [out_slot][75][3072]) into softbits_d. */
int dabgpu_ofdm_demod_mix(dabgpu_ctx *ctx, const void *iq_d, int format, const dabgpu_frame *frames_d, int n,
                          int chunks, int16_t level, int32_t *start_index_d, float *mix_d, float *spec_d,
                          void *softbits_d);

/* One symbol at a time (the reference's ofdmDecoder call pattern, ofdm-decoder.cpp:
 * 85-190), samples already mixed by the caller: kind 0 = block 0 (samples_d holds
 * T_u samples; its spectrum becomes the phase reference), kind 1 = a data symbol
 * (T_s samples; ibits_d[3072] = processToken's soft bits against the stored
 * spectrum, which then becomes this symbol's).  spectrum_d: cf32[2048] state. */
int dabgpu_ofdm_symbol(dabgpu_ctx *ctx, const float *samples_d, int kind, float *spectrum_d, int16_t *ibits_d);

/* ofdmDecoder::get_snr (ofdm-decoder.cpp:212-230) of a T_u-point spectrum in natural
 * bin order (cf32[2048], device): get_db(mean |X| of the signal bins) - get_db(mean |X|
 * of the noise bins) into snr_d[0]. */
int dabgpu_get_snr(dabgpu_ctx *ctx, const float *spectrum_d, int16_t *snr_d);

/* ---- channel decoding (L4) -------------------------------------------- */

/* viterbi::deconvolve batched (viterbi.cpp:225-242): n_cw codewords of
 * 4*(nbits+6) depunctured soft bits -> nbits decoded bits each. */
int dabgpu_viterbi(dabgpu_ctx *ctx, const int16_t *in_d, int n_cw, int nbits, uint8_t *out_d);

/* ficHandler::process_ficInput batched (fic-handler.cpp:241-321): n blocks of
 * 2304 soft bits (contiguous, block stride 2304) -> 768 bits after energy
 * dispersal, with each FIB's CRC field inverted by the check exactly as
 * check_CRC_bits leaves it (dab-constants.h:316-317); crc_ok_d[3*n]. */
int dabgpu_fic_decode(dabgpu_ctx *ctx, const int16_t *fic_soft_d, int n, uint8_t *bits_d,
                      uint8_t *crc_ok_d);

/* FIC blocks straight from a demod soft-bit buffer: frames slots[0..n_frames)
 * each give 4 blocks (symbols 1..3 of the slot). Output [n_frames][4][768]. */
int dabgpu_fic_decode_frames(dabgpu_ctx *ctx, const int16_t *softbits_d, const int32_t *slots_h,
                             int n_frames, uint8_t *bits_d, uint8_t *crc_ok_d);

/* uep_/eep_deconvolve::deconvolve + energy dispersal (deconvolve.cpp:172-237,
 * 325-366; dab-concurrent.cpp:183-190; no dispersal with DABGPU_SUBCH_RAW) for n_cw codewords whose
 * fragmentSize = length*64 soft bits are given contiguous (already
 * time-de-interleaved), one subchannel description per codeword: codeword i reads
 * frag_d + i*frag_stride (frag_stride >= every fragmentSize, DABGPU_E_ARG otherwise).
 * Output: codeword i's 24*bitRate bits at bits_d + i*out_stride, one per byte (out_stride
 * in bytes, >= the longest codeword's 24*bitRate, DABGPU_E_ARG otherwise; any alignment
 * of bits_d and out_stride).  Only those bytes are written: the rest of a row -- the gap
 * up to out_stride, and behind a codeword shorter than the longest -- and everything
 * outside the rows is left as it was.
 * bitRate: whatever the protection defines, up to 1824 kbit/s (EEP 4-B, 855 CU, the
 * longest subchannel a CIF's 864 CUs hold; EEP 4-A ends at 1728): the energy-dispersal
 * sequence runs on for 24*bitRate bits as dab-concurrent.cpp:183-190 builds it.
 * DABGPU_E_UNSUP above that, and for a protection the reference does not define. */
int dabgpu_msc_deconvolve(dabgpu_ctx *ctx, const int16_t *frag_d, int64_t frag_stride,
                          const dabgpu_subch *subch_h, int n_cw, uint8_t *bits_d, int64_t out_stride);

/* reedSolomon::dec(rsIn, rsOut, 135) batched (reed-solomon.cpp:129-141; the
 * RS(255,245) code of mp4processor.cpp:74 shortened to (120,110)): n codewords of
 * 120 bytes -> 110 corrected bytes each; ret_d[i] = symbols corrected or -1. */
int dabgpu_rs_decode(dabgpu_ctx *ctx, const uint8_t *in_d, int n, uint8_t *out_d, int16_t *ret_d);

/* mp2Processor::mp2decodeFrame batched (mp2processor.cpp:365-568; the counterpart of
 * dabgpu_rs_decode): n_chains independent decoders, each taking chain_len frames in order.
 *   frames_d  frame j of chain i at frames_d + (i*chain_len + j)*frame_stride; frame_stride
 *             (>= 4) bytes are readable and the frame reads as zeros beyond them
 *   state_d   DABGPU_MP2_STATE_BYTES per chain, opaque, all-zero for a new mp2Processor,
 *             updated in place
 *   pcm_d     int16 [n_chains][chain_len][1152][2] (left, right), pcm[(idx<<6)|(j<<1)|ch] per
 *             block of 96 samples as the reference writes it; rows of frames that returned
 *             0 are left untouched
 *   ret_d     int32 [n_chains][chain_len]: mp2decodeFrame's return value, the frame size in
 *             bytes, or 0 for a rejected header (such a frame writes no PCM and leaves the
 *             state as it was: the frame after it continues from the one before it)
 * The arithmetic is the reference's, integer from the first bit to the sample.  Three things
 * the reference leaves to its compiler or to the contents of memory are fixed by rule:
 *   1. V is int16: (sum + 8192) >> 14 is stored modulo 2^16 (what the reference's int16_t V
 *      does with gcc; loud frames do wrap);
 *   2. bits past the end of a frame read as 0 (the reference reads on into its frame buffer,
 *      2*24*bitRate bytes it never initialises; the host mp2Processor zero-fills it);
 *   3. products and sums are int32, two's complement (signed overflow is undefined in the
 *      reference; for frames whose intermediates stay inside int32 nothing rests on this).
 * Asynchronous on the context stream. */
int dabgpu_mp2_decode(dabgpu_ctx *ctx, const uint8_t *frames_d, int64_t frame_stride, int n_chains, int chain_len,
                      void *state_d, int16_t *pcm_d, int32_t *ret_d);

/* audioSink::audioOut batched (audiosink.cpp:235-360 over LowPassFIR::Pass, fir-filters.cpp:78-92;
 * the counterpart of dabgpu_mp2_decode): n_chains independent sinks, each taking chain_len calls
 * audioOut (V, amount, rate) in order.  What a call delivers is what it puts into _O_Buffer when
 * that never fills: one 48 kHz float stereo signal.
 *   pcm_d      int16 (left, right) pairs: call j of chain i reads amounts_h[i*chain_len + j] pairs
 *              from pcm_d + (i*chain_len + j) * pcm_stride * 2 (pcm_stride in pairs)
 *   rates_h    int32 [n_chains][chain_len] (host): 16000, 24000 and 32000 go through their
 *              interpolator (x3, x2, x3 and every second result), every other rate is scaled only
 *              (the reference's default: label); 0 is "no call" and leaves all state as it was
 *   amounts_h  int32 [n_chains][chain_len] (host), each in 0 .. max_amount; an odd amount at
 *              32000 is DABGPU_E_ARG (the reference then puts one float it never wrote)
 *   state_d    DABGPU_AUDIO_STATE_BYTES per chain, 4-byte aligned, opaque, all-zero for a new sink,
 *              updated in place; a call at one rate leaves the other rates' filters as they were
 *   samples_d  float [n_chains][chain_len][max_amount*3][2] (8-byte aligned); rows of calls that
 *              deliver nothing are left untouched
 *   n_out_d    int32 [n_chains][chain_len]: pairs written (amount, 2*amount, 3*amount or
 *              3*amount/2; 0 for rate 0)
 * Each sample is (float)((double)(float)V / 32767.0); every product and sum of a filter is rounded
 * to fp32 on its own, in the reference's order (no fma).  Not modelled: the sink's back-pressure
 * (amount cut to the ring's room) and dumpFile.  Asynchronous on the context stream (rates_h and
 * amounts_h are read before the call returns). */
int dabgpu_audio_out(dabgpu_ctx *ctx, const int16_t *pcm_d, int64_t pcm_stride, int n_chains, int chain_len, int max_amount,
                     const int32_t *rates_h, const int32_t *amounts_h, void *state_d, float *samples_d, int32_t *n_out_d);

/* motHandler::process_mscGroup in header mode (mot-data.cpp:679-728) batched: n_slots
 * independent motHandlers, each taking the groups of one (stream, packet slot) of a
 * dabgpu_pipe_packet call, or buffers in that layout, in completion order.  Fed are the groups
 * mot_databuilder::add_mscDatagroup passes on (mot-databuilder.cpp:84-95): DABGPU_DG_ACCEPTED
 * and DABGPU_DG_TRANSPORT; data is the group's bytes from data_offset, data_nbytes of them.
 *   state_d    [n_slots][dabgpu_mot_state_bytes(max_body_bytes)], all zero for a new
 *              motHandler, updated in place (head, entries, bodies: see dabgpu_mot_head)
 *   groups_d   [n_slots][group_slots], run_d [n_slots] (n_groups is read), bytes_d
 *              [n_slots][arena_bytes]
 *   objects_d  [n_slots][group_slots], the first mot_run.n_objects written
 *   out_d      [n_slots][out_arena_bytes]: the bodies, each as it was when its object completed
 *              (later groups of the run may rewrite the entry)
 *   mot_run_d  [n_slots]
 * Kept bit for bit from the reference:
 *   - segmentSize = (d[0] & 0x1F) << 8 | d[1]; the header size exactly as process_mscGroup
 *     computes it, (d[5] & 0x0F) << 9 | d[6] | d[7] >> 7 (:687-689 -- d[6] is not shifted,
 *     unlike get_dirEntry :216-218): it ends the parameter walk and is where the body bytes of
 *     a header segment that is not the last begin (:128-132);
 *   - contentType, contentsubType from segment[5..6], the PLI walk (:62-111); the name is the
 *     bytes of every parameter 12 after its first, appended (:104-108);
 *   - a header whose transport id has an entry is ignored (:113-114); a new entry takes the
 *     first free one, else the one with the lowest ordernumber (:621-655), and inherits its
 *     marks (newEntry does not clear them);
 *   - processSegment (:278-312): unknown transport id and marked segment ignored, segmentSize
 *     latched by the first segment that is not the last, a last segment while it is -1
 *     dropped, n * segmentSize + size > bodySize dropped, numofSegments set by the last one;
 *   - completion (:315-346): contentType 2 is a slide, and every slide completion after the
 *     first ever shown clears the completing entry's marks (the first keeps them, so its
 *     repeat shows nothing); contentType 7 completes and delivers nothing; anything else is a
 *     file, name and body.
 * Where the reference is undefined or unbounded:
 *   1. bytes past a group's data field read 0; a group with data_nbytes < 2 or segmentSize + 2
 *      > data_nbytes is dropped and counted (malformed);
 *   2. a segment number >= 100 is dropped and counted (the reference writes past marked[100]);
 *   3. sizes are int32 (newEntry's int16_t size wraps from 32768 bytes on: the reference never
 *      completes such an object); a body above max_body_bytes gets an entry flagged
 *      DABGPU_MOT_TOO_LARGE whose segments are ignored;
 *   4. body bytes no segment wrote read 0 (newEntry clears the body); no write leaves
 *      [0, bodySize): a segment whose size is negative (segmentSize - headerSize < 0) is dropped;
 *   5. names keep their first DABGPU_MOT_NAME_BYTES bytes, name_len the full length;
 *      ordernumber is int32 and the entry replaced is the one with the least;
 *   6. directory mode is out of scope: group type 6, and every group that is neither a header
 *      (type 3, segment 0) nor type 4, is counted (other_types) and otherwise ignored, so
 *      theDirectory stays NULL.  (The reference analyses a directory before it is complete,
 *      :182-189 with num_dirSegments == -1, and getHandle :602-607 then reads ordernumbers
 *      nothing initialised: there is no defined behaviour to equal.)
 * max_body_bytes 0 means DABGPU_MOT_BODY_BYTES; at most 1 << 24.  DABGPU_E_ARG for a bad
 * size: group_slots < 0, arena sizes outside [0, 2^31), out_arena_bytes below
 * DABGPU_MOT_ARENA_FOR(0, max_body_bytes).  Asynchronous on the context stream. */
size_t dabgpu_mot_state_bytes(int max_body_bytes);
int dabgpu_mot_groups(dabgpu_ctx *ctx, void *state_d, int n_slots, int max_body_bytes,
                      const dabgpu_datagroup *groups_d, int group_slots, const uint8_t *bytes_d, int64_t arena_bytes,
                      const dabgpu_packet_run *run_d, dabgpu_mot_object *objects_d, uint8_t *out_d,
                      int64_t out_arena_bytes, dabgpu_mot_run *mot_run_d);

/* ip_dataHandler::add_mscDatagroup (ip-datahandler.cpp:40-127, show_crcErrors on) batched: n_slots
 * independent ip_dataHandlers, each taking the groups of one (stream, packet slot) of a
 * dabgpu_pipe_packet call, or buffers in that layout, in completion order.
 *   state_d    [n_slots], all zero for a new ip_dataHandler, updated in place
 *   groups_d   [n_slots][group_slots], run_d [n_slots] (n_groups is read), bytes_d
 *              [n_slots][arena_bytes]
 *   results_d  [n_slots][group_slots], the first run.n_groups written: one per group
 *   out_d      [n_slots][out_arena_bytes]: the payloads, in group order, each at a multiple of 16
 *              (DABGPU_IP_ARENA_FOR(group_slots, arena_bytes) holds whatever the groups carry);
 *              bytes between payloads are not written
 *   ip_run_d   [n_slots]
 * Kept bit for bit from the reference:
 *   - a group with the CRC flag and a bad CRC is ignored (:54); the layer skips every group
 *     without DABGPU_DG_ACCEPTED, so empty and truncated groups go the same way;
 *   - next (:57-74) is the packet layer's data_offset: the walk over the extension, segment and
 *     user access fields is, step for step, that of mot-databuilder.cpp:37-95 which that field
 *     restates -- the two do not differ anywhere;
 *   - ipLength is bytes 2..3 after next (:79) and the datagram is taken only when ipLength <
 *     the group's byte length, CRC bytes included (:80: msc.size () counts bits);
 *   - ipLength bytes are copied from next; the version test is (ipVector [0] >> 4) != 4 on a
 *     signed char (:85), which only 0x40..0x4F pass: 0xC? shifts to -4;
 *   - the window steps before the datagram's own checksum test (:100-104): ++handledPackets >=
 *     100 emits 100 - crcErrors and clears both counters;
 *   - the checksum covers 2 * headerSize big-endian 16-bit words, headerSize 0..15 as it comes
 *     (0 sums to 0 and fails), with one fold; (~sum & 0xFFFF) != 0 counts in crcErrors (:105-111);
 *   - only protocol 17 goes on (:113-119); the payload starts at 4 * headerSize + 8 and its
 *     length is ipSize - 4 * headerSize - 8, ipSize being the two bytes of ipLength (:124-127);
 *     the UDP header's length, ports and checksum are not looked at.
 * Where the reference is undefined or unbounded:
 *   1. bytes past a group's stored end read 0: the length field of a group that ends inside it
 *      (:79) and a datagram with next + ipLength > the group's bytes (:84).  Since next >= 2, that
 *      is every datagram with ipLength >= nbytes - 1.  A datagram that overlaps the two CRC
 *      bytes of a group with the CRC flag reads them complemented: check_CRC_bits inverts them in
 *      place (:54, dab-constants.h:321-322) before the copy, while the packet layer stores the
 *      group as it was received (tests/golden/ip_kat.npz pins this on the reference's own code);
 *   2. ipLength == 0 is DABGPU_IP_NOT_V4 and nothing is read (ipVector [0] of an empty array);
 *   3. header bytes past ipLength read 0 (the reference reads past its vector when 4 * headerSize
 *      or 10 > ipLength); a negative payload length is DABGPU_IP_MALFORMED, counted after the
 *      window and checksum steps, where the reference would have called writeDatagram with it;
 *      length 0 is delivered as an empty datagram;
 *   4. lengths are int32 (ipSize and headerSize are int16_t in the reference); quality is stored
 *      as int16;
 *   5. a group record that points outside its arena is DABGPU_IP_NOT_ACCEPTED;
 *   6. a payload that ends beyond out_arena_bytes is DABGPU_IP_MALFORMED; it still takes its
 *      place, rounded up to 16, in the count of offsets (with DABGPU_IP_ARENA_FOR only records
 *      that overlap in their arena get there).
 * DABGPU_E_ARG for a bad size: n_slots or group_slots < 0, arena sizes outside [0, 2^31).
 * Asynchronous on the context stream. */
int dabgpu_ip_groups(dabgpu_ctx *ctx, dabgpu_ip_state *state_d, int n_slots,
                     const dabgpu_datagroup *groups_d, int group_slots, const uint8_t *bytes_d, int64_t arena_bytes,
                     const dabgpu_packet_run *run_d, dabgpu_ip_result *results_d, uint8_t *out_d,
                     int64_t out_arena_bytes, dabgpu_ip_run *ip_run_d);

/* padHandler::processPAD (pad-handler.cpp) batched: n_slots independent padHandlers, each
 * taking its n_aus AUs in order, fed as mp4Processor feeds them (mp4processor.cpp:237-265).
 *   state_d   [n_slots][dabgpu_pad_state_bytes()], opaque, all zero for a new padHandler,
 *             updated in place (16-byte aligned)
 *   aus_d     [n_slots][n_aus][au_stride] bytes; len_d int32 [n_slots][n_aus]: the AU's
 *             aac_frame_length; negative: the AU failed its CRC and is skipped.  Bytes past an
 *             AU's length (and past au_stride) read 0: the reference copies the AU into a zeroed
 *             theAU[1920].  An AU whose (byte0 >> 5) & 7 != 4 -- no data stream element first
 *             -- is counted (aus) and ignored (:264).
 *   cif_d     int32 [n_slots][n_aus] or NULL: the value records carry as `cif` (NULL: the AU's
 *             index in the call)
 *   labels_d  [n_slots][label_slots], groups_d [n_slots][group_slots], bytes_d
 *             [n_slots][arena_bytes], run_d [n_slots]
 * Labels are dabgpu_pad_label records.  X-PAD groups are dabgpu_datagroup records plus bytes in
 * the packet layer's layout, so groups_d / bytes_d feed dabgpu_mot_groups unchanged (with a
 * dabgpu_packet_run whose n_groups is this run's).  The header is as build_MSC_segment parses it
 * (:299-357): every completed group is recorded, and DABGPU_DG_ACCEPTED is set exactly for the
 * groups it hands to process_mscGroup: CRC flag clear or pad_crc good; group type 3 or 4; a
 * user access field, if present, has the transport-id flag.  A group without the segment flag
 * has segmentNumber 0xFFFF (the reference's -1), one without a user access field transportId
 * 0xFFFF (the reference's int16_t -1 through a uint16_t parameter) with DABGPU_DG_TRANSPORT set
 * -- the reference passes it on -- and DABGPU_DG_USER_ACCESS clear.  nbytes is
 * msc_dataGroupLength, data_offset the reference's index (for a group it returns from early,
 * what index would be: the fields are parsed regardless; a user access field without the
 * transport-id flag leaves index at that field), data_nbytes = max(0, length - index - (CRC flag
 * ? 2 : 0)), CI the reference's continuityIndex, (b[1] & 0xF) >> 4, which is always 0,
 * reserved[0] the AU's index in the call (modulo 256; dabgpu_pipe_pad: its index in its superframe).
 * Kept bit for bit from the reference:
 *   - processPAD: count = AU[1] (255 is not an escape), the PAD is AU[2 .. 2+count); only
 *     F-PAD type 0; X-PAD indicator 1 is short, 2 variable, anything else is ignored;
 *   - short PAD (:73-82): the CI is always read at count-3, the data is the three bytes below
 *     it, reversed; only application types 2 and 3;
 *   - variable PAD (:97-173): CI flag 0 ignored; up to four CIs, an end marker costs one byte;
 *     sub-fields reversed, lengths 4, 6, 8, 12, 16, 24, 32, 48; type 1 always takes 4 bytes,
 *     sets length and index and does `continue` (without the :168 check); the first type
 *     outside {1, 2, 3, 12, 13} records itself in last_appType and drops the rest of the PAD;
 *     type 12 is taken only after type 1, type 13 only after 12 or 13;
 *   - dynamicLabel (:177-269) entirely: the first / last / C flags, charSet set only by a
 *     first segment, the clear command, moreXPad / remainDataLength / isLastSegment, and the
 *     stale moreXPad a clear command leaves behind (type-3 sub-fields after it are appended to
 *     the cleared text).  Its five function-local statics are per-handler state here: a process
 *     with one padHandler cannot tell the difference, and a new handler starts them at their
 *     initialisers;
 *   - add_MSC_element (:274-297, MOT_BASICS__ defined, as both of the reference's build files
 *     do): index < 0 returns; a sub-field with index + length >= 8192 is dropped; completion at
 *     index >= msc_dataGroupLength, with that many bytes; index then goes back to 0, so further
 *     type-13 sub-fields fill a new group of the same length;
 *   - pad_crc (:360-381): CRC-16 0x1021 from all ones over length - 2 bytes against the
 *     complement of the last two.  Its left shifts of a negative int16_t are undefined before
 *     C++20; what is computed is the two's-complement result C++20 defines (and the pin is
 *     compiled as C++20 for that reason).
 * Where the reference is undefined or unbounded; each PAD that meets a rule is counted:
 *   1. count < 2: the PAD is ignored (the reference reads buffer[-1] or buffer[-2]);
 *   2. a read below byte 0 of the PAD reads 0, control flow otherwise the reference's, its
 *      :168-171 check included (a short PAD with count < 6, a sub-field or a length indicator
 *      longer than what is left, CIs down to byte 0);
 *   3. a new handler has last_appType 0, no group in progress (index -1: a type-13 sub-field
 *      that reaches add_MSC_element before any length indicator returns there), length 0,
 *      charSet 0 and a zeroed 8192-byte buffer.  The buffer is part of the state: header
 *      fields past a short group's end read its stale bytes, as in the reference (counted only
 *      where the byte was never written).  A group with the CRC flag and a length below 2 has
 *      a bad CRC.  For a group's data field rule 1 of dabgpu_mot_groups applies downstream;
 *   4. the label text is unbounded in the reference while segments without `first` keep
 *      arriving: past DABGPU_PAD_LABEL_BYTES bytes or DABGPU_PAD_LABEL_PIECES pieces the record
 *      keeps the first bytes and pieces, reports the full nbytes and n_pieces and sets
 *      DABGPU_PAD_LABEL_TRUNCATED.
 * Beyond the slots: labels and groups past label_slots / group_slots are counted and not
 * recorded; a group that does not fit the arena is recorded without bytes, flagged
 * DABGPU_DG_TRUNCATED and not accepted (neither happens with the DABGPU_PAD_* sizes).
 * DABGPU_E_ARG for negative sizes, an arena below DABGPU_PAD_ARENA_BYTES(0) or of 2 GiB and
 * more.  Asynchronous on the context stream. */
size_t dabgpu_pad_state_bytes(void);
int dabgpu_pad_aus(dabgpu_ctx *ctx, void *state_d, int n_slots, const uint8_t *aus_d, int64_t au_stride,
                   const int32_t *len_d, int n_aus, const int32_t *cif_d, dabgpu_pad_label *labels_d, int label_slots,
                   dabgpu_datagroup *groups_d, int group_slots, uint8_t *bytes_d, int64_t arena_bytes,
                   dabgpu_pad_run *run_d);

/* ---- FIC layer: FIBs to the service database and the subchannel table (fib-processor.cpp) ----
 * dabgpu_fic_db is what a fib_processor holds, as a plain record: the per-slot device state of
 * dabgpu_fib_parse and what a caller downloads (host/fib_processor's export_db / import_db speak
 * it too).  All zero is a new fib_processor; padding and reserved bytes stay zero, so two
 * databases compare with memcmp.  Fields the reference never reads in a free entry are kept
 * canonical: a service that is not inUse has serviceId 0 (the reference's -1 is never read), a
 * component that was never bound has service 0.  Labels are the 16 bytes as transmitted with
 * their charset (host: label_text for UTF-8). */
typedef struct {            /* ficList[SubChId] (fib-processor.h: channelMap) */
    int16_t SubChId;        /* never written by a FIG (FIG 0/14 matches it: only id 0 takes effect) */
    int16_t StartAddr, Length, uepFlag, protLevel, BitRate, FEC_scheme;
    uint8_t inUse;          /* a FIG 0/1 described it */
    uint8_t reserved;
} dabgpu_fic_subch;
typedef struct {            /* components[i] (serviceComponent) */
    uint8_t inUse;
    int8_t TMid;
    int16_t service;        /* index into services */
    int16_t componentNr, ASCTy, PS_flag, subchannelId;
    uint16_t SCId;
    uint8_t CAflag;
    int8_t DGflag;
    int16_t DSCTy, packetAddress;
} dabgpu_fic_component;
typedef struct {            /* listofServices[i] (serviceId) */
    int32_t serviceId;
    uint8_t inUse, hasName, hasLanguage;
    uint8_t charset;        /* of label */
    int16_t language, programType;
    uint8_t data_suffix;    /* the label came by FIG 1/5: its text ends in " (data)" */
    uint8_t reserved[3];
    uint8_t label[16];
} dabgpu_fic_service;
typedef struct {            /* what fib_processor::subchannels returns: the table dabgpu_pipe_set_subch takes */
    int32_t n;
    int32_t reserved[3];
    dabgpu_subch sub[64];   /* the first n, in SubChId order; the rest zero */
    uint8_t ids[64];        /* each entry's SubChId */
} dabgpu_fic_table;
typedef struct {
    dabgpu_fic_subch sub[64];
    dabgpu_fic_component components[64];
    dabgpu_fic_service services[64];
    int32_t EId;            /* of the nameofEnsemble signal */
    uint8_t charset;
    uint8_t named;          /* nameofEnsemble has been raised: the reference's firstTime, inverted */
    uint8_t reserved[2];
    uint8_t label[16];      /* the ensemble label of that signal */
    uint8_t reserved2[8];
    dabgpu_fic_table table; /* the table of the last dabgpu_fib_parse call on this record (all zero
                               before the first; export_db leaves it alone, clearEnsemble too) */
} dabgpu_fic_db;
#define DABGPU_FIC_NAME_ENSEMBLE 1  /* nameofEnsemble (id, label): id = EId */
#define DABGPU_FIC_ADD_SERVICE   2  /* addtoEnsemble (label): id = the service's slot */
typedef struct {
    int32_t kind;           /* DABGPU_FIC_* */
    int32_t fib;            /* index in the call of the FIB that raised it */
    int32_t id;
    int32_t charset;
    uint8_t label[16];
} dabgpu_fic_event;
#define DABGPU_FIC_EVENT_SLOTS 65   /* the most one call can raise without a clear between */
typedef struct {
    int32_t parsed, skipped;        /* FIBs walked / with ok == 0 */
    int32_t figs[8];                /* FIG headers met, by type (7: the end marker) */
    int32_t n_events;               /* raised; the first min(n_events, event_slots) are recorded */
    int32_t overrun;                /* FIBs that met the overrun rule */
    int32_t table_changed;          /* the table differs from the record's previous one */
    int32_t reserved[3];
} dabgpu_fic_run;
/* fib_processor::process_FIB per slot: n_slots independent databases db_d [n_slots], updated in
 * place.  Slot s takes the FIBs fibs_d + s * fib_stride + 32 * i, i < n_fibs, in order: 32 bytes
 * each, msb first, the CRC bytes as delivered; FIBs with ok_d [n_slots][n_fibs] == 0 are skipped.
 * Parsed as host/fib_processor.cpp does it, which cites the reference line by line: FIG 0/1, 0/2,
 * 0/3, 0/14, 0/16, 0/17, FIG 1/0, 1/1, 1/5, FIG 2/5; find_service (the in-use entry, else the
 * first free slot, else entry 0), find_packet_component and bind (once per service and
 * component number, in the first free slot).
 * Outputs per slot: events_d [n_slots][event_slots] in the order raised, each with the FIB that
 * caused it (events past event_slots are counted and not recorded; the slots a call does not
 * fill are zeroed); table_d [n_slots]:
 * fib_processor::subchannels(ids, classic_audio, packet_data, mot, pad, ip) at the end of the call,
 * the five booleans being the bits DABGPU_SUBCH_MP2 | PACKET | MOT | PAD | IP of want_flags; run_d
 * [n_slots].
 * Where the reference is undefined:
 *   1. the overrun rule: a read at or past bit 256 of the FIB reads 0, control flow otherwise the
 *      reference's (a FIG near the end of the data field whose length, component list or label
 *      runs on; the reference reads whatever follows in its FIC buffer).  Such a FIB is counted
 *      in overrun.  Counted are the reads host/fib_processor.cpp makes, in its order: the fields
 *      this parser stores or branches on (the reference also reads fields it then drops, such as
 *      FIG 0/3's CAOrg or the labels of FIG 1/3, 1/4 and 1/6);
 *   2. a bind with the component table full writes nothing (the reference writes slot -1).
 * Every index into the database, the event slots and the table is checked: no FIB makes the
 * kernel leave its slot.  DABGPU_E_ARG for negative sizes or fib_stride < 32 * n_fibs.
 * Asynchronous on the context stream. */
size_t dabgpu_fic_db_bytes(void);
int dabgpu_fib_parse(dabgpu_ctx *ctx, dabgpu_fic_db *db_d, int n_slots, const uint8_t *fibs_d, int64_t fib_stride,
                     const uint8_t *ok_d, int n_fibs, int want_flags, dabgpu_fic_event *events_d, int event_slots,
                     dabgpu_fic_table *table_d, dabgpu_fic_run *run_d);
/* fib_processor::clearEnsemble for the slots with which_h[s] != 0 (host array [n_slots]; NULL:
 * all): components, subchannels, services' inUse / serviceId / label and the ensemble's name go;
 * each service's language, programType, hasLanguage (and hasName, until the entry is taken again)
 * stay, as in the reference (:1149-1163). */
int dabgpu_fic_clear(dabgpu_ctx *ctx, dabgpu_fic_db *db_d, int n_slots, const uint8_t *which_h);

/* ---- streaming pipeline (ofdmProcessor::run + ficHandler + mscHandler) ---
 * n_streams independent ensembles; each call decodes n_frames frames per
 * stream.  Sync, AFC, DQPSK references and the 16-CIF time de-interleaver
 * state (dab-concurrent.cpp:162-175: the first 16 CIFs are warm-up) are
 * carried across calls.  subch lists the subchannels decoded for every
 * stream (the reference decodes one selected subchannel; this decodes all) until
 * dabgpu_pipe_set_subch gives a stream a table of its own. */
typedef struct dabgpu_pipe dabgpu_pipe;
typedef struct {
    int32_t n_streams;
    int32_t n_frames;          /* frames per dabgpu_pipe_run call */
    int32_t n_subch;
    int16_t threshold;         /* findIndex level (gui.cpp:98-99, default 3) */
    int16_t freq_sync_method;  /* processBlock_0's coarse AFC: 0 getMiddle, 1 phase-difference
                                  correlation (main.cpp:91 default), 2 pattern match
                                  (ofdm-decoder.cpp:103-161) */
    const dabgpu_subch *subch;
} dabgpu_pipe_cfg;

typedef struct {
    int64_t next_pos;          /* stream index of the next window (SyncOnPhase) */
    int32_t local_phase;
    int32_t coarse;            /* coarseCorrector */
    int16_t fine;              /* fineCorrector */
    int16_t f2correction;
    int16_t prev1, prev2;
    int32_t synced;
    int64_t cif_count;         /* CIFs delivered to the MSC so far */
    int32_t last_start_index;
    int32_t resyncs;           /* sync losses (findIndex failed: goto notSynced, ofdm-processor.cpp:354-357) */
    int32_t acquisitions;      /* null-symbol searches completed (SyncOnNull..SyncOnEndNull) */
    int32_t attempts;          /* the reference's `attempts` counter (ofdm-processor.cpp:274-314) */
    int32_t no_signal;         /* No_Signal_Found emissions (scan mode, > 5 failed attempts) */
    int32_t frames_run;        /* frames this stream committed in the last dabgpu_pipe_run */
    int32_t acquiring;         /* 1: a background null search (DABGPU_CTL_ACQ_ASYNC) is running */
} dabgpu_stream_state;

/* Per-frame record of the last run (the observables ofdmProcessor / ofdmDecoder
 * report to the GUI, ofdm-processor.cpp:172-175,344-446, ofdm-decoder.cpp:93-97). */
typedef struct {
    int64_t window;            /* first sample of the frame's T_u sync window */
    int32_t start_index;       /* findIndex result */
    int32_t coarse;            /* coarseCorrector used for symbols 1..75 */
    int16_t fine;              /* fineCorrector used for symbols 1..75 */
    int16_t correction;        /* processBlock_0's return (0 when f2Correction was off) */
    int16_t snr;               /* get_snr of block 0 (ofdm-decoder.cpp:212-230), before the IIR */
    int16_t committed;         /* 1: the frame was decoded in this run */
} dabgpu_frame_info;

int dabgpu_pipe_create(dabgpu_ctx *ctx, const dabgpu_pipe_cfg *cfg, dabgpu_pipe **out);
/* Per-stream subchannel tables, changeable between runs (entry points added within ABI 7;
 * a pipeline that never calls them behaves as before).  Two multiplexes never share a
 * subchannel organisation, and a receiver learns it from the FIC (FIG 0/1, 0/2) only after
 * it has started decoding: the reference starts a new dabConcurrent for a newly selected
 * subchannel (mscHandler::set_audioChannel / set_dataChannel, msc-handler.cpp), with its
 * own 16-CIF warm-up (dab-concurrent.cpp:162-175).
 * The caps size the pipeline; every stream's table then holds up to max_subch entries. */
typedef struct {
    int32_t max_subch;     /* table entries per stream; the MSC output's row count */
    int32_t max_bitrate;   /* largest bitRate any entry may have (sizes decisions, msc_stride check) */
    int32_t max_dabplus;   /* DAB+ entries per stream; the DAB+ outputs' slot count */
    int32_t max_mp2;       /* layer II entries per stream; the dabgpu_pipe_mp2 outputs' slot count
                              (0: no layer II state is allocated) */
} dabgpu_pipe_caps;
/* dabgpu_pipe_create with buffers sized by caps: cfg->subch[0..n_subch) is every stream's
 * initial table (n_subch = 0: a FIC-only pipeline until dabgpu_pipe_set_subch).
 * dabgpu_pipe_create is this call with the caps of its table (n_subch, its largest bitRate,
 * its numbers of DAB+ and of layer II entries).  A pipeline with max_mp2 == 0 allocates and
 * launches nothing for the layer II layer.  Output layouts with caps:
 *   msc_bits_d [n_streams][4*n_frames][max_subch][msc_stride]: entry k of a stream is row k;
 *              rows of absent or not-yet-valid entries are left untouched
 *   sf_bytes_d / info_d (and the compact form): max_dabplus in place of n_dabplus; DAB+
 *              slot j of a stream is its j-th entry flagged DABGPU_SUBCH_DABPLUS; the info
 *              records of absent slots have status -1. */
int dabgpu_pipe_create_caps(dabgpu_ctx *ctx, const dabgpu_pipe_cfg *cfg, const dabgpu_pipe_caps *caps,
                            dabgpu_pipe **out);
/* Replace the table of one stream (stream = -1: of every stream) for the runs that follow.
 * Validates as create does: DABGPU_E_UNSUP for an undefined protection or a bad DAB+
 * bitRate, DABGPU_E_ARG for an entry outside its CUs, for n > max_subch, a bitRate above
 * max_bitrate, more DAB+ entries than max_dabplus, more layer II entries than max_mp2, more
 * packet-mode entries than dabgpu_pipe_packet_caps allows, more MOT entries than
 * dabgpu_pipe_mot_caps allows, an entry flagged DABGPU_SUBCH_MOT without DABGPU_SUBCH_PACKET, more
 * PAD entries than dabgpu_pipe_pad_caps allows, an entry flagged DABGPU_SUBCH_PAD without
 * DABGPU_SUBCH_DABPLUS, more audio output entries than dabgpu_pipe_audio_caps allows, an entry
 * flagged DABGPU_SUBCH_AUDIO without DABGPU_SUBCH_MP2 or an entry flagged for two layers;
 * DABGPU_E_UNSUP for a packet-mode bitRate that is no multiple of 8; on any error the table
 * is unchanged.  (A packet-mode entry that is not unchanged is a new mscDatagroup, and a new
 * motHandler when it is flagged DABGPU_SUBCH_MOT; an unchanged one keeps both.)
 * Waits for everything the pipeline has enqueued (as dabgpu_pipe_set_profiling): call
 * dabgpu_pipe_dabplus / dabgpu_pipe_mp2 / dabgpu_pipe_packet for the last run before it (the
 * layers refuse a run decoded under the old table: its rows are not the new slots').
 * An entry whose index and all six fields are unchanged keeps its since_cif and its DAB+ or
 * layer II state and decodes without interruption.  Every other entry gets since_cif = the
 * stream's cif_count at the call, its DAB+ ring and state zeroed (a new mp4Processor) or its
 * synchroniser and decoder zeroed (a new mp2Processor), and delivers
 * CIF c only when the stream delivered c and c >= since_cif + 16: all 16 source CIFs of
 * such a codeword lie at or after the switch, so the result equals a reference decoder
 * started at the switch.  Initial entries have since_cif 0. */
int dabgpu_pipe_set_subch(dabgpu_pipe *p, int stream, const dabgpu_subch *subch, int32_t n);
/* The stream's table: subch[max_subch], *n entries, since_cif[max_subch] (or NULL). */
int dabgpu_pipe_get_subch(dabgpu_pipe *p, int stream, dabgpu_subch *subch, int32_t *n, int64_t *since_cif);
/* Per entry, for the last run: valid_h [n_streams][4*n_frames][max_subch], 1 where the
 * stream delivered the CIF and it is past the entry's own warm-up (dabgpu_pipe_run's
 * msc_valid_h stays stream level: past the stream's first 16 CIFs). */
int dabgpu_pipe_msc_entry_valid(dabgpu_pipe *p, uint8_t *valid_h);
int dabgpu_pipe_destroy(dabgpu_pipe *p);
/* Acquire (notSynced/SyncOnNull/SyncOnEndNull, ofdm-processor.cpp:274-338)
 * every stream not yet synchronised from sample start_h[s] of its IQ (device,
 * stream s at sample stream_stride*s of iq_d, n_avail_h[s] samples).  Optional:
 * dabgpu_pipe_run acquires unsynchronised streams itself, from their current
 * position (sample 0 for a new pipeline). */
int dabgpu_pipe_acquire(dabgpu_pipe *p, const void *iq_d, int64_t stream_stride,
                        const int64_t *start_h, const int64_t *n_avail_h);
/* Decode the next n_frames frames of every stream, as ofdmProcessor::run does:
 * a stream whose findIndex fails goes back to the null-symbol search from where it
 * is (goto notSynced, ofdm-processor.cpp:354-357) and continues with the frames
 * after it.  Outputs (device memory, or dabgpu_host_alloc memory through its device
 * address: the decoders then write across PCIe themselves -- zero copy, slower than
 * dabgpu_pipe_fetch behind the decoding on MI355X; not for a pipeline with DAB+
 * subchannels, whose layer reads msc_bits_d back):
 *   fic_bits_d  [n_streams][n_frames][4][768] (DABGPU_PACK_FIC: [4][96] FIB bytes),
 *               fic_crc_d [n_streams][n_frames][12]
 *               (frame f of stream s: its f-th frame of this run; frames past
 *               dabgpu_stream_state.frames_run have CRC flags 0)
 *   msc_bits_d  [n_streams][4*n_frames][n_subch][msc_stride] (24*bitRate used)
 *   msc_valid_h [n_streams][4*n_frames] (host, optional): 1 where the stream
 *               delivered the CIF and it is past the 16-CIF warm-up.
 * Returns 0 when every stream decoded n_frames frames, DABGPU_E_STATE when one
 * ran out of samples (its decoded frames are still delivered; see
 * dabgpu_pipe_state). */
int dabgpu_pipe_run(dabgpu_pipe *p, const void *iq_d, int64_t stream_stride, const int64_t *n_avail_h,
                    uint8_t *fic_bits_d, uint8_t *fic_crc_d, uint8_t *msc_bits_d, int32_t msc_stride,
                    uint8_t *msc_valid_h);
/* DAB+ superframe layer for the CIFs of the last dabgpu_pipe_run (call once per
 * run, after it): mp4Processor::addtoFrame/processSuperframe
 * (mp4processor.cpp:107-292) for every subchannel flagged DABGPU_SUBCH_DABPLUS,
 * state (5-CIF byte ring, blockFillIndex, blocksInBuffer) carried across runs.
 * Outputs (device), DAB+ subchannels numbered in cfg order:
 *   sf_bytes_d [n_streams][4*n_frames][n_dabplus][sf_stride]: the 110*RSDims
 *              corrected superframe bytes where info.status == 3
 *   info_d     [n_streams][4*n_frames][n_dabplus] */
int dabgpu_pipe_dabplus(dabgpu_pipe *p, uint8_t *sf_bytes_d, int32_t sf_stride, dabgpu_superframe *info_d);
/* MPEG layer II layer for the CIFs of the last dabgpu_pipe_run (call once per run, after it,
 * before or after dabgpu_pipe_dabplus: each layer takes a run's CIFs once): for every entry
 * flagged DABGPU_SUBCH_MP2, mp2Processor::addtoFrame over the CIFs dabgpu_pipe_msc_entry_valid
 * reports as 1, in order (what dabConcurrent feeds it after its 16-CIF warm-up), and
 * mp2decodeFrame for every frame that completes (see dabgpu_mp2_decode for the arithmetic).
 * Synchroniser and decoder state are carried across runs; dabgpu_pipe_set_subch keeps them
 * for an unchanged entry and gives every other one a new mp2Processor.  At most one frame
 * completes per CIF and entry.  Outputs (device), MP2 slot j of a stream being its j-th
 * entry flagged DABGPU_SUBCH_MP2:
 *   pcm_d  int16 [n_streams][4*n_frames][max_mp2][1152][2], written where info.status == 2
 *   info_d [n_streams][4*n_frames][max_mp2]
 * Runs on the run's back-end stream behind its MSC (dabgpu_pipe_sync to wait).  Like the
 * DAB+ layer it reads msc_bits_d back: not for a run whose msc_bits_d is host memory.
 * DABGPU_E_STATE for a pipeline with max_mp2 == 0 or without a run to consume. */
int dabgpu_pipe_mp2(dabgpu_pipe *p, int16_t *pcm_d, dabgpu_mp2_info *info_d);
/* Audio output layer for the frames of the run's dabgpu_pipe_mp2 call (call once per run, after
 * it): for every entry flagged DABGPU_SUBCH_MP2 | DABGPU_SUBCH_AUDIO, audio slot j of a stream
 * being its j-th such entry, every frame with info.status == 2 goes through audioSink::audioOut
 * (pcm, 1152, info.sample_rate) in CIF order (mp2processor.cpp:584-588; see dabgpu_audio_out for
 * the arithmetic).  pcm_d and info_d are those of that call (DABGPU_E_ARG otherwise); they are read
 * and never written.  The sinks are carried across runs; dabgpu_pipe_set_subch keeps the one of an
 * unchanged entry and gives every other entry a new one, together with its mp2Processor.
 * Outputs (device):
 *   samples_d float [n_streams][4*n_frames][max_audio][2304][2], written where n_out > 0
 *   n_out_d   int32 [n_streams][4*n_frames][max_audio]: 0, 1152 (a 48 kHz frame) or 2304 (24 kHz)
 * Runs on the run's back-end stream behind the layer II layer.  DABGPU_E_STATE without a layer
 * (max_audio == 0), without a dabgpu_pipe_mp2 call for the run, or on a second call. */
int dabgpu_pipe_audio(dabgpu_pipe *p, const int16_t *pcm_d, const dabgpu_mp2_info *info_d, float *samples_d, int32_t *n_out_d);
/* Size the audio output layer: max_audio slots per stream (<= max_mp2), as dabgpu_pipe_pad_caps
 * sizes the PAD layer.  Both create calls start with the number of flagged entries of their
 * table; with max_audio == 0 nothing is allocated or launched.  Between runs; waits for
 * everything enqueued.  The sinks of the slots both sizes hold are kept.  DABGPU_E_ARG for a
 * negative value, max_audio > max_mp2 or fewer slots than an applied table flags. */
int dabgpu_pipe_audio_caps(dabgpu_pipe *p, int max_audio);
/* Packet-mode data layer for the CIFs of the last dabgpu_pipe_run (call once per run, after
 * it, in any order with dabgpu_pipe_dabplus / dabgpu_pipe_mp2): for every entry flagged
 * DABGPU_SUBCH_PACKET, mscDatagroup::handlePackets + handlePacket (msc-datagroup.cpp:221-319,
 * show_crcErrors on) over the CIFs dabgpu_pipe_msc_entry_valid reports as 1, in order, and for
 * every completed series the header parse and CRC of mot_databuilder::add_mscDatagroup
 * (mot-databuilder.cpp:37-95) -- bit for bit what host/msc_consumers' packetAssembler
 * delivers, its quirks included: the copy takes usefulLength bytes from byte 3 whatever the
 * packet's length (a CRC-good packet whose useful length exceeds its data field reads its
 * own CRC bytes complemented, as check_CRC_bits leaves them, then the following packets'
 * bytes) and stops at the CIF's end.  Where the reference is undefined or unbounded:
 *   1. header fields past a group's end read as 0 (and a group with the CRC flag and fewer
 *      than 2 bytes has a bad CRC);
 *   2. lengths are int32 (the reference's int16_t sizeinBits wraps above 4095 bytes);
 *   3. a series longer than max_group_bytes keeps its first max_group_bytes bytes, is
 *      reported with its full nbytes, flagged DABGPU_DG_TRUNCATED and not accepted.
 * Out of scope: DSCTy 5 with the DG flag (handleTDCAsyncstream delivers nothing: do not
 * flag such entries) and the FEC scheme (the reference ignores it).
 * Assembler state (packetState, streamAddress, the 500-packet window, the series in flight)
 * is carried across runs; dabgpu_pipe_set_subch keeps it for an unchanged entry and gives
 * every other one a new mscDatagroup.  Outputs (device), packet slot j of a stream being its
 * j-th entry flagged DABGPU_SUBCH_PACKET:
 *   info_d   [n_streams][4*n_frames][max_packet]
 *   run_d    [n_streams][max_packet]
 *   groups_d [n_streams][max_packet][DABGPU_PKT_GROUP_SLOTS(n_frames, max_bitrate)], in
 *            completion order, the first run.n_groups written
 *   bytes_d  [n_streams][max_packet][DABGPU_PKT_ARENA_BYTES(n_frames, max_bitrate,
 *            max_group_bytes)], the groups' stored bytes back to back (the most a run can
 *            complete, the over-read included)
 * Runs on the run's back-end stream behind its MSC (dabgpu_pipe_sync to wait); reads
 * msc_bits_d (one bit per byte or DABGPU_PACK_MSC bytes) and never writes it: not for a run
 * whose msc_bits_d is host memory.  DABGPU_E_STATE without a layer (max_packet == 0) or
 * without a run to consume. */
int dabgpu_pipe_packet(dabgpu_pipe *p, uint8_t *bytes_d, dabgpu_datagroup *groups_d, dabgpu_packet_run *run_d,
                       dabgpu_packet_info *info_d);
/* Size the packet-mode layer: max_packet slots per stream, groups of at most max_group_bytes
 * (0: DABGPU_PKT_GROUP_BYTES).  Both create calls start with the number of flagged entries
 * of their table and the default group size; with max_packet == 0 nothing is allocated or
 * launched.  Between runs; waits for everything enqueued, as dabgpu_pipe_set_subch.  The
 * state of the existing entries is kept (a series in flight longer than a smaller
 * max_group_bytes keeps its first bytes).  DABGPU_E_ARG for negative values, max_packet >
 * max_subch, fewer slots than an applied table flags, fewer than the MOT layer holds
 * (dabgpu_pipe_mot_caps first) or, with a MOT layer, a packet arena of 2 GiB and more. */
int dabgpu_pipe_packet_caps(dabgpu_pipe *p, int max_packet, int max_group_bytes);
/* MOT layer for the groups of the run's dabgpu_pipe_packet call (call once per run, after
 * it): dabgpu_mot_groups for every entry flagged DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT, MOT
 * slot j of a stream being its j-th such entry.  bytes_d, groups_d and run_d of that packet
 * call are read (keep them alive until the run's work is done) and never written.  The
 * motHandlers are carried across runs; dabgpu_pipe_set_subch keeps the one of an unchanged
 * entry and gives every other entry a new one.  Outputs (device):
 *   bytes_d   [n_streams][max_mot][DABGPU_MOT_ARENA_BYTES(n_frames, max_bitrate, max_body_bytes)]
 *   objects_d [n_streams][max_mot][DABGPU_MOT_OBJECT_SLOTS(n_frames, max_bitrate)]
 *   run_d     [n_streams][max_mot]
 * Runs on the run's back-end stream behind the packet layer.  DABGPU_E_STATE without a layer
 * (max_mot == 0), without a dabgpu_pipe_packet call for the run, or on a second call. */
int dabgpu_pipe_mot(dabgpu_pipe *p, uint8_t *bytes_d, dabgpu_mot_object *objects_d, dabgpu_mot_run *run_d);
/* Size the MOT layer: max_mot slots per stream (<= max_packet), bodies of at most
 * max_body_bytes (0: DABGPU_MOT_BODY_BYTES).  Both create calls start with the number of
 * flagged entries of their table and the default body size; with max_mot == 0 nothing is
 * allocated or launched.  Between runs; waits for everything enqueued.  The state of the
 * slots both sizes hold is kept (an entry whose body no longer fits becomes
 * DABGPU_MOT_TOO_LARGE).  DABGPU_E_ARG for negative values, max_mot > max_packet,
 * max_body_bytes > 1 << 24 or fewer slots than an applied table flags. */
int dabgpu_pipe_mot_caps(dabgpu_pipe *p, int max_mot, int max_body_bytes);
/* IP layer for the groups of the run's dabgpu_pipe_packet call (call once per run, after it):
 * dabgpu_ip_groups for every entry flagged DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP.  The outputs are
 * indexed by packet slot; the slot of an entry that is not flagged gets an all-zero dabgpu_ip_run
 * and is not walked.  It reads that call's bytes_d, groups_d and run_d (keep them alive and
 * unchanged).  The ip_dataHandlers' counters live beside the packet layer's assemblers (8 bytes
 * per packet slot, allocated with the packet layer: there is no caps call): dabgpu_pipe_set_subch
 * keeps those of an unchanged entry, flags included, every other entry starts at zero, and
 * dabgpu_pipe_packet_caps keeps those of the slots both sizes hold.
 *   bytes_d   [n_streams][max_packet][DABGPU_IP_ARENA_FOR(DABGPU_PKT_GROUP_SLOTS(n_frames,
 *             max_bitrate), DABGPU_PKT_ARENA_BYTES(n_frames, max_bitrate, max_group_bytes))]
 *   results_d [n_streams][max_packet][DABGPU_PKT_GROUP_SLOTS(n_frames, max_bitrate)]
 *   run_d     [n_streams][max_packet]
 * Runs on the run's back-end stream behind the packet layer.  DABGPU_E_STATE without a packet
 * layer (max_packet == 0), without a dabgpu_pipe_packet call for the run, on a second call, or
 * when no applied table flags an entry DABGPU_SUBCH_IP (nothing is launched then); DABGPU_E_ARG
 * when the packet layer's arena is 2 GiB and more. */
int dabgpu_pipe_ip(dabgpu_pipe *p, uint8_t *bytes_d, dabgpu_ip_result *results_d, dabgpu_ip_run *run_d);
/* One stream's ip_dataHandler counters, by packet slot, to host memory: state_h [max_packet] (a
 * slot whose entry is not flagged holds zeros).  Waits for everything the pipeline has enqueued.
 * DABGPU_E_ARG for a bad stream, DABGPU_E_STATE without a packet layer. */
int dabgpu_pipe_ip_state(dabgpu_pipe *p, int stream, dabgpu_ip_state *state_h);
/* PAD layer for the AUs of the run's dabgpu_pipe_dabplus call (call once per run, after it):
 * dabgpu_pad_aus for every entry flagged DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD, PAD slot j of
 * a stream being its j-th such entry.  sf_bytes_d, sf_stride and info_d are those of that call
 * (DABGPU_E_ARG otherwise), sparse or compact as it wrote them; they are read (keep them alive
 * until the run's work is done) and never written.  Taken are the AUs of status-3 superframes in
 * CIF and AU order: AU i is aac_frame_length = au_start[i+1] - au_start[i] - 2 bytes from
 * au_start[i], skipped where au_crc_ok has its bit clear.  One stated limit: k_dp_layer stores
 * no bytes for a superframe rejected for an impossible AU table (status 2), whose earlier AUs the
 * reference would already have processed: such superframes are counted in rejected_sf and
 * skipped.  The padHandlers are carried across runs; dabgpu_pipe_set_subch keeps the one of an
 * unchanged entry and gives every other entry a new one.  Outputs (device):
 *   labels_d [n_streams][max_pad][DABGPU_PAD_LABEL_SLOTS(n_frames)]
 *   groups_d [n_streams][max_pad][DABGPU_PAD_GROUP_SLOTS(n_frames)]
 *   bytes_d  [n_streams][max_pad][DABGPU_PAD_ARENA_BYTES(n_frames)]
 *   run_d    [n_streams][max_pad]
 * Runs on the run's back-end stream behind the DAB+ layer.  DABGPU_E_STATE without a layer
 * (max_pad == 0), without a dabgpu_pipe_dabplus call for the run, or on a second call.
 * X-PAD slides inside the pipeline are not part of this: dabgpu_mot_groups on these groups is
 * the path. */
int dabgpu_pipe_pad(dabgpu_pipe *p, const uint8_t *sf_bytes_d, int32_t sf_stride, const dabgpu_superframe *info_d,
                    dabgpu_pad_label *labels_d, dabgpu_datagroup *groups_d, uint8_t *bytes_d, dabgpu_pad_run *run_d);
/* Size the PAD layer: max_pad slots per stream (<= max_dabplus).  Both create calls start with
 * the number of flagged entries of their table; with max_pad == 0 nothing is allocated or
 * launched.  Between runs; waits for everything enqueued.  The state of the slots both sizes
 * hold is kept.  DABGPU_E_ARG for a negative value, max_pad > max_dabplus or fewer slots than an
 * applied table flags. */
int dabgpu_pipe_pad_caps(dabgpu_pipe *p, int max_pad);
/* FIC layer for the FIBs of the last dabgpu_pipe_run (call once per run, after it, in any order
 * with the MSC layers): dabgpu_fib_parse on one database per stream, which is carried across
 * runs.  fic_bits_d and fic_crc_d are those of that run (DABGPU_E_ARG otherwise), read as it wrote
 * them -- one bit per byte [4][768] or DABGPU_PACK_FIC bytes [4][96] per frame -- and never
 * written: each stream's 12 * n_frames FIBs in order, fic_crc_d as the ok flags (frames past
 * frames_run have flags 0: a stream that ran out of samples commits fewer FIBs).  Outputs
 * (device):
 *   events_d [n_streams][DABGPU_FIC_EVENT_SLOTS]  (fib = 12 * frame + FIB of the frame)
 *   table_d  [n_streams]: what dabgpu_pipe_set_subch takes (table.sub, table.n), with want_flags
 *   run_d    [n_streams]
 * Runs on the run's back-end stream behind its FIC decode (dabgpu_pipe_sync to wait).  The table
 * is not applied on the device: dabgpu_pipe_set_subch is the host's call.  DABGPU_E_STATE without
 * a layer (dabgpu_pipe_fic_caps), without a run with FIC output and CRC flags to consume, or on a
 * second call for the same run. */
int dabgpu_pipe_fic(dabgpu_pipe *p, const uint8_t *fic_bits_d, const uint8_t *fic_crc_d, int want_flags,
                    dabgpu_fic_event *events_d, dabgpu_fic_table *table_d, dabgpu_fic_run *run_d);
/* The FIC layer on (one new database per stream; a layer that is on keeps its databases) or off
 * (they are freed).  A pipeline starts without it and then allocates and launches nothing for
 * it.  Between runs; waits for everything enqueued. */
int dabgpu_pipe_fic_caps(dabgpu_pipe *p, int on);
/* one stream's database to db_h (host); waits for everything enqueued */
int dabgpu_pipe_fic_db(dabgpu_pipe *p, int stream, dabgpu_fic_db *db_h);
/* fib_processor::clearEnsemble for one stream's database (-1: every stream's), see dabgpu_fic_clear */
int dabgpu_pipe_fic_clear(dabgpu_pipe *p, int stream);
/* Compact superframe bytes for the following dabgpu_pipe_dabplus calls (on = 1): only the
 * superframes that complete in the run are stored, per (stream, DAB+ subchannel) in CIF
 * order -- sf_bytes_d [n_streams][n_dabplus][DABGPU_SF_SLOTS(n_frames)][sf_stride], the
 * k-th at slot k, and its info record's `reserved` byte is k (0xFF for records without
 * bytes).  One CIF in five carries a superframe, so this is the form to copy to the host
 * (dabgpu_pipe_fetch).  At most 512 frames per run. */
#define DABGPU_SF_SLOTS(n_frames) ((4 * (n_frames) + 4) / 5 + 1)
int dabgpu_pipe_set_dabplus_compact(dabgpu_pipe *p, int on);
/* Sample format of the streams dabgpu_pipe_acquire / dabgpu_pipe_run read (default
 * DABGPU_IQ_F32): DABGPU_IQ_S16 (interleaved int16, the .sdr recording's PCM16) or
 * DABGPU_IQ_U8 (interleaved u8, the .raw recording / dabstick) are converted exactly
 * in the kernels' sample loads, with the file readers' scaling (see dabgpu_iq_convert),
 * so the decode equals that of the converted cf32 stream; the stream stride and
 * n_avail stay in samples.  Takes effect at the next call. */
int dabgpu_pipe_set_iq_format(dabgpu_pipe *p, int format);
/* dabgpu_pipe_state takes a finished background null search's results first, so
 * st->acquiring is 0 once the search no longer reads iq_d. */
int dabgpu_pipe_state(dabgpu_pipe *p, int stream, dabgpu_stream_state *st);
/* [n_streams][n_frames] records of the last dabgpu_pipe_run */
int dabgpu_pipe_frame_info(dabgpu_pipe *p, dabgpu_frame_info *info_h);
/* ofdmProcessor's control methods, for one stream (stream = -1: every stream):
 *   DABGPU_CTL_RESET        reset(): fine = coarse = 0, f2Correction on (ofdm-processor.cpp:476-479)
 *   DABGPU_CTL_COARSE_ON    coarseCorrectorOn(): f2Correction on, coarse = 0 (:498-501)
 *   DABGPU_CTL_COARSE_OFF   coarseCorrectorOff() (:503-505)
 *   DABGPU_CTL_SCAN_ON/OFF  set_scanMode(bool) (:507-509): count No_Signal_Found
 *   DABGPU_CTL_RESYNC       drop sync: the next run searches the null symbol again from
 *                           the stream's current position (goto notSynced)
 *   DABGPU_CTL_ACQ_ASYNC    (default since ABI 6; stream ignored) a stream that needs the null
 *                           search after it had been synchronised -- a sync loss,
 *                           ofdm-processor.cpp:354-357 -- gets it in the background on a
 *                           low-priority stream while the run goes on without it; the first
 *                           run after the search finished continues that stream from where it
 *                           found the null (its frames are the same, delivered later: it
 *                           decodes fewer than n_frames in the runs it misses, with
 *                           DABGPU_OK).  A stream's first search (before any frame) stays
 *                           inside the run.  iq_d must stay valid until the search ends
 *                           (dabgpu_stream_state.acquiring, or dabgpu_pipe_acquire_wait).
 *                           dabgpu_pipe_sync does not wait for a background search; the
 *                           other control ops do (its result is applied first, so the
 *                           control is the last word)
 *   DABGPU_CTL_ACQ_SYNC     the reference's order: the run waits for every search and
 *                           delivers n_frames (a one-ensemble caller loses nothing by it)
 *   DABGPU_CTL_INJECT_BOUNDS fault injection (stream ignored): the next run's MSC decoder
 *                           is handed a subchannel offset past the soft-bit ring; its
 *                           kernels refuse it (erasures read instead: the depunctured
 *                           value 0, RING8 byte 127), and dabgpu_pipe_sync or
 *                           the next run reports DABGPU_E_BOUNDS once -- the error path of
 *                           the back-end streams, for tests */
#define DABGPU_CTL_RESET      1
#define DABGPU_CTL_COARSE_ON  2
#define DABGPU_CTL_COARSE_OFF 3
#define DABGPU_CTL_SCAN_ON    4
#define DABGPU_CTL_SCAN_OFF   5
#define DABGPU_CTL_RESYNC     6
#define DABGPU_CTL_ACQ_ASYNC  7
#define DABGPU_CTL_ACQ_SYNC   8
#define DABGPU_CTL_INJECT_BOUNDS 9
int dabgpu_pipe_control(dabgpu_pipe *p, int stream, int op);
/* Wait until everything the pipeline enqueued is done.  The FIC/MSC/DAB+ outputs
 * of run r are written by back-end stream r & 1 (overlapping run r+1's OFDM front
 * end and channel decoding): call this before reading them, and give run r+1
 * output buffers other than run r's unless this was called in between.  Also
 * reports a kernel that refused out-of-bounds work (DABGPU_E_BOUNDS). */
int dabgpu_pipe_sync(dabgpu_pipe *p);
/* Wait for a background null search (DABGPU_CTL_ACQ_ASYNC) in flight and apply its
 * result; afterwards no search reads iq_d.  0 when none is in flight. */
int dabgpu_pipe_acquire_wait(dabgpu_pipe *p);
/* per-stage kernel time (HIP events on each stage's stream, no synchronisation added):
 * dabgpu_pipe_set_profiling(p, 1) times the last dabgpu_pipe_run, (p, 2) every run
 * since the call (summed; launches counts them); 0 turns it off.  Mode 3 is mode 2
 * with every timed stage run alone (the device drained before and after its launch):
 * per-kernel times without the overlap of the front end and the channel decoders,
 * for rooflines -- slower, never for throughput.  set_profiling waits for the
 * pipeline's streams; dabgpu_pipe_timing waits for the recorded work. */
#define DABGPU_STAGE_PRS      0   /* k_prs_sync   (findIndex)          */
#define DABGPU_STAGE_BLOCK0   1   /* k_block0     (processBlock_0 AFC) */
#define DABGPU_STAGE_DEMOD    2   /* k_demod      (processToken x 75)  */
#define DABGPU_STAGE_FIC      3   /* FIC Viterbi + CRC (CRC only when the run also
                                     decodes MSC: the FIC's Viterbi then shares the
                                     MSC's ACS and traceback launches)  */
#define DABGPU_STAGE_MSC_ACS  4   /* MSC Viterbi add-compare-select    */
#define DABGPU_STAGE_MSC_TB   5   /* MSC chainback + energy dispersal  */
#define DABGPU_STAGE_DABPLUS  6   /* k_dabplus (superframe, RS, AU CRC) */
#define DABGPU_NSTAGE         7
int dabgpu_pipe_set_profiling(dabgpu_pipe *p, int on);
int dabgpu_pipe_timing(dabgpu_pipe *p, float *ms /*[DABGPU_NSTAGE]*/, int32_t *launches /*[DABGPU_NSTAGE] or NULL*/);
/* device soft-bit ring of the last run ([n_streams][ring][75][3072] bytes) and the slot
 * of (stream, frame) in it, for tests and the ofdmProcessor drop-in.  Each byte is the
 * ibits value v of processToken (ofdm-decoder.cpp:188-189, always in -127..127) plus 127:
 * the Viterbi's branch-metric input itself (viterbi.cpp:230-233), half the bytes of int16. */
int dabgpu_pipe_softbits(dabgpu_pipe *p, const uint8_t **soft_d, int32_t *ring_frames);
int dabgpu_pipe_frame_slot(dabgpu_pipe *p, int frame, int32_t *slot);
/* per-frame front-end record of the last run: [n_streams][n_frames] */
int dabgpu_pipe_frames(dabgpu_pipe *p, dabgpu_frame *frames_h, int32_t *start_index_h);
/* The constellation display of ofdmDecoder::processToken (ofdm-decoder.cpp:192-206,
 * displayToken 2): with on = 1 the demod keeps, for every frame it decodes, the FFT
 * of symbol 2 at bins [0, K/2) and [T_u-1-K/2, T_u-1) -- the K values processToken
 * pushes into iqBuffer, in that order; dabgpu_pipe_iq_display copies those of
 * (stream, frame) of the last dabgpu_pipe_run (a decoded frame) to carriers_h[K][2].
 * Which frames the GUI is shown (every 8th) is the caller's choice, as in the
 * reference.  Costs 12 KB of HBM writes per frame while on. */
int dabgpu_pipe_set_display(dabgpu_pipe *p, int on);
/* The symbol (1..75) the display feed keeps, ofdmDecoder::set_displayToken (declared in
 * ofdm-decoder.h:50, displayToken = 2 at ofdm-decoder.cpp:61); takes effect at the next run. */
int dabgpu_pipe_set_display_token(dabgpu_pipe *p, int token);
/* Output format of the following runs, a mask (0 = the default: one bit per byte, as
 * deconvolve / process_ficInput deliver them, viterbi.cpp:240-241, fic-handler.cpp:270-292):
 *   DABGPU_PACK_MSC  MSC eight bits per byte, msb first (the packing of
 *                    mp4Processor::addtoFrame, mp4processor.cpp:115-121 -- numpy packbits
 *                    order): msc_stride is then in bytes (>= 3 * bitRate).  The DAB+ layer
 *                    reads either.
 *   DABGPU_PACK_FIC  FIC as FIB bytes, msb first: fic_bits holds [n_frames][4][96] bytes per
 *                    stream (3 FIBs of 32 bytes per FIC block, the last 2 bytes of each FIB
 *                    its CRC, inverted in place as check_CRC_bits leaves it,
 *                    dab-constants.h:310-340) instead of [4][768] bits -- an eighth of the
 *                    bytes a host (or dabgpu_pipe_fetch) has to move; fic_crc unchanged.
 * Any other value: DABGPU_E_ARG. */
#define DABGPU_PACK_MSC 1
#define DABGPU_PACK_FIC 2
int dabgpu_pipe_set_packed(dabgpu_pipe *p, int on);
/* Copy bytes from an output buffer of the last dabgpu_pipe_run (or dabgpu_pipe_dabplus)
 * to host memory, asynchronously, behind that run's channel decoding on its back-end
 * stream: the results reach the host while the next run decodes.  Complete after
 * dabgpu_pipe_sync (the run after next does not wait for it; its channel decoding, which
 * may reuse the output buffers, is queued behind it).  dst_h should be dabgpu_host_alloc
 * memory: with it (and 16-byte aligned pointers and size) a kernel of a few waves writes
 * the mapped host buffer directly; other memory goes through the runtime's copy, which
 * may synchronise. */
int dabgpu_pipe_fetch(dabgpu_pipe *p, void *dst_h, const void *src_d, size_t bytes);
int dabgpu_pipe_iq_display(dabgpu_pipe *p, int stream, int frame, float *carriers_h);

#ifdef __cplusplus
}
#endif
#endif
