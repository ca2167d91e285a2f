// dabgpu_dropin.h -- C++ host classes with the interfaces of sdr-j-dab's hot-path
// classes, running on MI355X through the C ABI (include/dabgpu.h).
//
// Same class names, constructor arguments, method signatures and argument
// meaning as the reference (paths relative to the sdr-j-dab v0.997 tree), minus
// Qt: where the reference emits a Qt signal or calls into the GUI, these classes
// take a std::function callback instead.  They live in namespace dabgpu so a
// build can switch with a using-declaration.
//
// Errors: the reference signals hard errors by `throw int` out of its worker
// threads (ofdm-processor.cpp:200-240); here a failing GPU call throws
// dabgpu::error (std::runtime_error with dabgpu_last_error()).  Decoding
// outcomes (CRC failures, RS failures) are return values, as in the reference.
//
// Threading: one HIP context per calling thread (thread_local), as the
// reference runs OFDM, FIC and MSC on separate threads.
#pragma once
#include <complex>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <vector>

#include <atomic>
#include <cstdio>
#include <memory>
#include <mutex>
#include <thread>

#ifdef DABGPU_HAVE_SNDFILE
#include <sndfile.h>          // a build with libsndfile (the reference's gui.cpp / wavfiles)
#endif

#include "dabgpu.h"
#include "fib_processor.h"
#include "msc_consumers.h"
#include "ringbuffer.h"

namespace dabgpu {

typedef std::complex<float> DSPCOMPLEX;   // dab-constants.h: DSPCOMPLEX

// ---- reference data types (dab-constants.h:72-73,137-176) -------------------------
#define DAB      0100
#define DAB_PLUS 0101
struct DabParams {
    uint8_t dabMode;
    int16_t L, K, T_null;
    int32_t T_F;
    int16_t T_s, T_u, guardLength, carrierDiff;
};
// RadioInterface::setModeParameters (gui.cpp:1361-1371); the GPU path is Mode I only
void setModeParameters(DabParams *p, uint8_t mode = 1);
// packetdata / audiodata (dab-constants.h:152-177): fib_processor.h

// virtualInput (src/input/virtual-input.h:51-70): the device the front end pulls
// samples from; getSamples copies up to n cf32 samples scaled to about +-1.
class virtualInput {
public:
    virtual ~virtualInput() = default;
    virtual int32_t getSamples(DSPCOMPLEX *v, int32_t n) = 0;
    virtual int32_t Samples() = 0;
    virtual bool restartReader() { return true; }
    virtual void stopReader() {}
    virtual int16_t bitDepth() { return 10; }
};

struct error : std::runtime_error {
    int code;
    error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

// HIP device used by contexts created from now on in this process (default 0)
void set_device(int device);
// this thread's context (created on first use)
dabgpu_ctx *thread_context();

// device buffer owned by the calling thread's context
class devbuf {
public:
    devbuf() = default;
    explicit devbuf(size_t bytes) { resize(bytes); }
    ~devbuf();
    devbuf(const devbuf &) = delete;
    devbuf &operator=(const devbuf &) = delete;
    void resize(size_t bytes);
    void *get() const { return p_; }
    size_t size() const { return n_; }
    void upload(const void *h, size_t bytes);
    void download(void *h, size_t bytes) const;
private:
    void *p_ = nullptr;
    size_t n_ = 0;
};

// viterbi.h:66-85 -- k=7 R=1/4 decoder for wordlength info bits
class viterbi {
public:
    explicit viterbi(int16_t wordlength);
    virtual ~viterbi() = default;
    // input: 4*(wordlength+6) soft bits in [-127, 127]; output: wordlength bits (one per byte)
    void deconvolve(int16_t *input, uint8_t *output);
protected:
    int16_t wordlength_;
    devbuf in_, out_;
};

// deconvolve.h: uep_deconvolve (deconvolve.cpp:142-237)
class uep_deconvolve : public viterbi {
public:
    uep_deconvolve(int16_t bitRate, int16_t protLevel);
    // v: fragmentSize punctured soft bits; out: 24*bitRate bits (no energy dispersal,
    // exactly what the reference's deconvolve delivers). False for an undefined profile.
    bool deconvolve(int16_t *v, int32_t size, uint8_t *outBuffer);
private:
    dabgpu_subch sub_;
};

// deconvolve.h: eep_deconvolve (deconvolve.cpp:238-366), protLevel = 0100|n (A) or 0200|n (B)
class eep_deconvolve : public viterbi {
public:
    eep_deconvolve(int16_t bitRate, int16_t protLevel);
    bool deconvolve(int16_t *v, int32_t size, uint8_t *outBuffer);
private:
    dabgpu_subch sub_;
};

// reed-solomon.h -- only the DAB+ code (8, 0435, 0, 1, 10) is supported on the GPU
class reedSolomon {
public:
    reedSolomon(uint16_t symsize = 8, uint16_t gfpoly = 0435, uint16_t fcr = 0, uint16_t prim = 1,
                uint16_t nroots = 10);
    // cutlen must be 135 (RS(120,110), mp4processor.cpp:171); returns corrected symbols or -1
    int16_t dec(const uint8_t *data_in, uint8_t *data_out, int16_t cutlen);
private:
    devbuf in_, out_, ret_;
};

// phasereference.h -- findIndex on T_u samples already mixed by getSamples
class phaseReference {
public:
    explicit phaseReference(int16_t threshold);
    int32_t findIndex(DSPCOMPLEX *v);
private:
    int16_t threshold_;
    devbuf iq_, fr_, si_;
};

// ficHandler without Qt (fic-handler.cpp:143-321, fic-handler.h:44-52): process_ficBlock
// accumulates symbols 1..3 of a frame into the 4 FIC blocks and decodes each on the GPU
// (depuncture, Viterbi, energy dispersal, CRC); every CRC-good FIB goes to the owned
// fib_processor under the fibHandling lock, as process_ficInput does (:304-320), so the
// GUI's service lookups (kindofService, dataforAudioService, dataforDataService,
// clearEnsemble) work on this class as on the reference's.  QString& arguments are
// std::string (UTF-8, the 16 characters of the label as transmitted).  Signals are
// callbacks: show_ficCRC per FIB, nameofEnsemble / addtoEnsemble from the FIG parser.
// Optionally every FIB (256 bits, CRC field inverted as check_CRC_bits leaves it) with
// its CRC verdict goes to a raw callback as well.
// The reference runs the decoding on its own thread behind a 3-slot queue and stop()
// ends that thread; here decoding happens in the caller's thread (the GPU is the
// parallel part) and after stop() process_ficBlock drops its input.
class ficHandler {
public:
    using fib_cb = std::function<void(const uint8_t *fib /*256 bits*/, bool crc_ok, int16_t ficno)>;
    struct signals {
        std::function<void(bool)> show_ficCRC;
        fib_processor::ensemble_cb nameofEnsemble;
        fib_processor::service_cb addtoEnsemble;
    };
    explicit ficHandler(signals sig, int16_t bitsperBlock = 2 * DABGPU_K);
    explicit ficHandler(fib_cb cb, int16_t bitsperBlock = 2 * DABGPU_K);
    void process_ficBlock(int16_t *data, int16_t blkno);   // blkno 1..3
    void clearEnsemble();
    int16_t get_ficRatio() const;                           // % of FIBs with a good CRC (*)
    uint8_t kindofService(const std::string &s);
    void dataforDataService(const std::string &s, packetdata *d);
    void dataforAudioService(const std::string &s, audiodata *d);
    void stop();
    void on_fib(fib_cb cb) { cb_ = std::move(cb); }
    // (*) the reference's ficRatio is never updated in v0.997 (fic-handler.cpp:186-188)
    // the database, for callers that want more than the reference's lookups (under the lock)
    template <class F> auto with_fib_processor(F f) {
        std::lock_guard<std::mutex> g(fibHandling_);
        return f(fibProcessor_);
    }
private:
    void init(int16_t bitsperBlock);
    fib_cb cb_;
    signals sig_;
    std::vector<int16_t> ofdm_input_;
    int index_ = 0, ficno_ = 0;
    int good_ = 0, total_ = 0;
    std::atomic<bool> running_{true};
    std::mutex fibHandling_;
    fib_processor fibProcessor_;
    std::vector<std::function<void()>> pending_;   // GUI signals raised under fibHandling_, fired after it
    devbuf in_, bits_, crc_;
};

// ---- MSC back end ----------------------------------------------------------------
// mp4Processor::addtoFrame / processSuperframe (mp4processor.cpp:107-292) minus faad:
// 5-CIF superframe window, fire code, RS(120,110) of the RSDims columns on the GPU
// (one dabgpu_rs_decode launch per superframe), AU table and AU CRCs; each AU goes to
// the callback where the reference hands it to the AAC decoder.
class mp4Processor : public dabProcessor {
public:
    struct au_info {
        uint8_t dacRate, sbrFlag, aacChannelMode, mpegSurround;
        int16_t n_corrected;           // RS symbols corrected in the superframe
    };
    using au_cb = std::function<void(const uint8_t *au, int16_t len, bool crc_ok, const au_info &)>;
    mp4Processor(int16_t bitRate, au_cb cb);
    void addtoFrame(uint8_t *v, int16_t nbits) override;
    // optional PAD hook, fed where the reference calls my_padHandler.processPAD
    // (mp4processor.cpp:255-265): an AU with a good CRC whose first syntactic element is a data
    // stream element, as theAU -- 1920 bytes, the AU's len bytes and zeros behind them.  No hook
    // (the default): nothing changes.  A padAssembler takes it as
    //   set_pad_hook([&](const uint8_t *theAU, int16_t len) { pad.processAU(theAU, 1920, len); });
    using pad_cb = std::function<void(const uint8_t *theAU, int16_t len)>;
    void set_pad_hook(pad_cb f) { pad_ = std::move(f); }
    int32_t superframes() const { return superframes_; }
    int32_t frameErrors() const { return frameErrors_; }
private:
    bool processSuperframe(int base);
    int16_t bitRate_, RSDims_;
    au_cb cb_;
    pad_cb pad_;
    std::vector<uint8_t> frameBytes_, outVector_;
    int16_t blockFillIndex_ = 0, blocksInBuffer_ = 0;
    int32_t superframes_ = 0, frameErrors_ = 0;
    devbuf rsin_, rsout_, rsret_;
};

// dabConcurrent (dab-concurrent.cpp:34-202) without its thread: each CIF fragment is
// time-de-interleaved (16 branches, delays 15 - brev4(i), the first 16 CIFs are warm-up),
// then depunctured + Viterbi-decoded + energy-dispersed on the GPU
// (dabgpu_msc_deconvolve) and handed to the dabProcessor.  (The reference's thread hands
// CIF n over when CIF n+1 arrives; here it is decoded on arrival.)
class dabConcurrent : public dabVirtual {
public:
    dabConcurrent(uint8_t dabModus, int16_t fragmentSize, int16_t bitRate, int16_t uepFlag, int16_t protLevel,
                  std::unique_ptr<dabProcessor> processor);
    int32_t process(int16_t *v, int16_t cnt) override;
    void setFiles(FILE *mp2, FILE *mp4) override;   // dab-concurrent.cpp:196-200
    dabProcessor *processor() { return proc_.get(); }
protected:
    bool deinterleave(const int16_t *v);       // false during the warm-up
    uint8_t dabModus_;
    int16_t fragmentSize_, bitRate_;
    dabgpu_subch sub_;
    std::vector<int16_t> delay_;               // [16][fragmentSize] ring of past fragments
    std::vector<int16_t> data_;
    int32_t countforInterleaver_ = 0, cif_ = 0;
    std::vector<uint8_t> outV_;
    std::unique_ptr<dabProcessor> proc_;
    devbuf in_, out_;
};

// mscDatagroup (msc-datagroup.cpp:44-339) without its thread: the same de-interleave and
// GPU decode, then packets -> MSC data groups (packetAssembler) for the data handler.
class mscDatagroup : public dabConcurrent {
public:
    mscDatagroup(uint8_t DSCTy, int16_t packetAddress, int16_t fragmentSize, int16_t bitRate, int16_t uepFlag,
                 int16_t protLevel, uint8_t DGflag, int16_t FEC_scheme, packetAssembler::datagroup_cb cb,
                 motAssembler::object_cb mot = nullptr, ipAssembler::datagram_cb datagram = nullptr,
                 ipAssembler::quality_cb ip_quality = nullptr);
    int32_t process(int16_t *v, int16_t cnt) override;
    const packetAssembler &assembler() const { return pa_; }
    // DSCTy 60 (my_dataHandler = new mot_databuilder, msc-datagroup.cpp:82-84): every data group
    // also goes through the host motAssembler, whose slides and files go to the mot callback
    // (nullptr for any other DSCTy)
    const motAssembler *mot() const { return mot_.get(); }
    // DSCTy 59 (my_dataHandler = new ip_dataHandler): every data group also goes through the host
    // ipAssembler, whose UDP payloads go to the datagram callback (where the reference sends them
    // to port 8888) and whose show_ipErrors values go to ip_quality (nullptr for any other DSCTy)
    const ipAssembler *ip() const { return ip_.get(); }
private:
    std::unique_ptr<motAssembler> mot_;        // before pa_, whose callback feeds it
    std::unique_ptr<ipAssembler> ip_;          // likewise
    packetAssembler pa_;
};

// mscHandler (msc-handler.cpp:41-193): collects the 18 MSC symbols of a CIF
// (process_mscBlock with blkno 4..75), and for the selected subchannel hands the
// CIF's slice [startAddr * 64, + Length * 64) to a dabConcurrent (audio: mp2Processor
// for DAB, mp4Processor for DAB+ (ASCTy 077)) or an mscDatagroup (data).  The channel
// set by set_audioChannel / set_dataChannel (any thread, under the lock) takes effect
// at the next process_mscBlock.  The decoded output goes to the callbacks; setFiles
// (msc-handler.cpp:208-212) dumps the DAB audio's MPEG frames into the mp2 file instead
// (see mp2Processor), and keeps both files for the channels selected later
// (msc-handler.cpp:147-150).
class mscHandler {
public:
    struct outputs {
        mp2Processor::frame_cb mp2;            // MPEG-1/2 layer II frames (DAB)
        mp4Processor::au_cb aac;               // AAC access units (DAB+)
        packetAssembler::datagroup_cb datagroup;
        motAssembler::object_cb mot;           // slides and files of a DSCTy 60 data channel (the_picture, fopen)
        ipAssembler::datagram_cb datagram;     // UDP payloads of a DSCTy 59 data channel (writeDatagram)
        ipAssembler::quality_cb ip_quality;    // ... and its show_ipErrors values
    };
    mscHandler(DabParams *p, outputs out, uint8_t concurrent = 1);
    void process_mscBlock(int16_t *fbits, int16_t blkno);
    void set_audioChannel(audiodata *d);
    void set_dataChannel(packetdata *d);
    int16_t getLanguage();
    int16_t getType();
    void stop();
    void stopProcessing();
    void setFiles(FILE *mp2, FILE *mp4);
    dabVirtual *handler() { return dabHandler_.get(); }
private:
    std::mutex locker_;
    outputs out_;
    FILE *mp2File_ = nullptr, *mp4File_ = nullptr;
    int16_t BitsperBlock_, numberofblocksperCIF_;
    std::vector<int16_t> cifVector_;
    std::unique_ptr<dabVirtual> dabHandler_;
    bool audioService_ = true, work_to_be_done_ = false, newChannel_ = false;
    int16_t startAddr_ = 0, Length_ = 0;
    audiodata na_{};
    packetdata np_{};
    int16_t new_language_ = 0, new_type_ = 0;
};

// ---- libsndfile (the .sdr dump) -------------------------------------------------------
// gui.cpp:861-893 opens the dump with sf_open (path, SFM_WRITE, {INPUT_RATE, 2 channels,
// SF_FORMAT_WAV | SF_FORMAT_PCM_16}) and hands the SNDFILE* to ofdmProcessor::startDumping,
// which writes interleaved PCM16 frames with sf_writef_short (ofdm-processor.cpp:150-157).
// Built with -DDABGPU_HAVE_SNDFILE (and -lsndfile), dabgpu:: names libsndfile's own types
// and calls, so the GUI's ::SNDFILE* binds to startDumping unchanged.  Without it (this
// image has no libsndfile) a stand-in with the subset those calls use writes the same
// RIFF/WAVE PCM16 file (the header's sizes are filled in by sf_close).
#ifdef DABGPU_HAVE_SNDFILE
using ::SF_INFO;
using ::SNDFILE;
using ::sf_close;
using ::sf_open;
using ::sf_writef_short;
using ::SFM_WRITE;
using ::SF_FORMAT_WAV;
using ::SF_FORMAT_PCM_16;
#else
struct SF_INFO {
    int64_t frames;
    int samplerate, channels, format, sections, seekable;
};
struct SNDFILE;
constexpr int SFM_WRITE = 0x20;
constexpr int SF_FORMAT_WAV = 0x010000, SF_FORMAT_PCM_16 = 0x0002;
SNDFILE *sf_open(const char *path, int mode, SF_INFO *info);   // SFM_WRITE, WAV PCM16 only (else nullptr)
int64_t sf_writef_short(SNDFILE *f, const int16_t *ptr, int64_t frames);
int sf_close(SNDFILE *f);
#endif

// ---- OFDM front end ----------------------------------------------------------------
// ofdmDecoder (ofdm-decoder.cpp:37-230, ofdm-decoder.h:40-48) one symbol per call on the
// GPU: processBlock_0 = get_snr (IIR 0.7/0.3, show_snr every 11 blocks) + coarse offset of
// freqSyncMethod 0/1/2 + the spectrum as phase reference; processToken = FFT + DQPSK +
// frequency de-interleave -> 3072 soft bits, and every 8th displayToken (blkno 2) the
// carriers fft_buffer[0, K/2) and [T_u-1-K/2, T_u-1) into iqBuffer + showIQ(K)
// (ofdm-decoder.cpp:192-206; the counter is shared by every decoder, as the reference's
// function-static cnt).  Samples are the caller's, already NCO-mixed.  The reference's
// RadioInterface* is the signals struct; refTable (phaseReference::getTable) only feeds
// refArg (ofdm-decoder.cpp:71-74), which the device tables hold already.
class ofdmDecoder {
public:
    struct signals {
        std::function<void(int)> show_snr, showIQ;
    };
    ofdmDecoder(DabParams *p, RingBuffer<DSPCOMPLEX> *iqBuffer, DSPCOMPLEX *refTable, signals sig,
                uint8_t freqSyncMethod);
    ofdmDecoder(DabParams *p, uint8_t freqSyncMethod = 1, std::function<void(int)> show_snr = nullptr);
    int16_t processBlock_0(DSPCOMPLEX *vi, bool flag);
    void processToken(DSPCOMPLEX *inv, int16_t *ibits, int32_t blkno);
    // get_snr (ofdm-decoder.cpp:212-230) of a T_u-point spectrum (natural bin order)
    int16_t get_snr(DSPCOMPLEX *v);
    int16_t snr() const { return snr_; }
    // the symbol whose carriers feed iqBuffer (ofdm-decoder.cpp:61,197; the reference
    // declares set_displayToken, ofdm-decoder.h:50, without defining it: here it works)
    void set_displayToken(int16_t t) { displayToken = t; }
    // processToken's `static int cnt` (ofdm-decoder.cpp:171): one count per process
    static std::atomic<int> iq_count;
    static constexpr int16_t defaultDisplayToken = 2;          // ofdm-decoder.cpp:61
    int16_t displayToken = defaultDisplayToken;
private:
    uint8_t method_;
    RingBuffer<DSPCOMPLEX> *iqBuffer_ = nullptr;
    signals sig_;
    int16_t snr_ = 0, snrCount_ = 0;
    devbuf smp_, spec_, fr_, corr_, snrd_, bits_;
};

// ofdmProcessor (ofdm-processor.cpp:34-509, ofdm-processor.h:49-59): the constructor
// starts the thread that pulls samples from the virtualInput into a sliding window in
// HBM and runs the GPU front end (the dabgpu_pipe_* engine for one stream: null search,
// findIndex, coarse/fine AFC, demod); every decoded frame's symbols go to
// ficHandler::process_ficBlock (blkno 1..3) and mscHandler::process_mscBlock (4..75) with
// the reference's soft bits.  The GUI signals are callbacks (the RadioInterface* of the
// reference): show_avgTokenLength (every 11 frames), setSynced, No_Signal_Found (scan
// mode), show_snr, and at the reference's sample positions -- the end of the getSample /
// getSamples call that takes the sample count past INPUT_RATE/7, replayed from the
// frames the GPU decoded -- show_fineCorrector / show_coarseCorrector and, with a
// spectrumBuffer (HAVE_SPECTRUM), the 32768 raw samples read since the previous one
// into the ring + showSpectrum(32768) (ofdm-processor.cpp:161-180,220-238).  With an
// iqBuffer every 8th frame's symbol-2 carriers go into it + showIQ(K), as the
// reference's ofdmDecoder does (ofdm-decoder.cpp:192-206; the GPU demod exports them,
// dabgpu_pipe_iq_display).  startDumping writes the raw samples as interleaved PCM16
// (the .sdr payload, ofdm-processor.cpp:150-157) with the reference's scaling, through
// sf_writef_short (SNDFILE*) or as bare PCM16 into a FILE*.
class ficHandler;
class ofdmProcessor {
public:
    struct signals {
        std::function<void(int)> show_fineCorrector, show_coarseCorrector, show_avgTokenLength, show_snr;
        std::function<void(char)> setSynced;
        std::function<void()> No_Signal_Found;
        std::function<void(int)> showSpectrum, showIQ;
    };
    // the reference's argument list (spectrumBuffer: HAVE_SPECTRUM builds; either ring may be null)
    ofdmProcessor(virtualInput *theRig, DabParams *p, signals sig, mscHandler *msc, ficHandler *fic,
                  int16_t threshold, RingBuffer<DSPCOMPLEX> *spectrumBuffer, RingBuffer<DSPCOMPLEX> *iqBuffer,
                  uint8_t freqSyncMethod);
    // without display rings (a build without HAVE_SPECTRUM and no IQ scope)
    ofdmProcessor(virtualInput *theRig, DabParams *p, signals sig, mscHandler *msc, ficHandler *fic,
                  int16_t threshold = 3, uint8_t freqSyncMethod = 1);
    ~ofdmProcessor();
    void reset();
    void stop();
    void coarseCorrectorOn();
    void coarseCorrectorOff();
    void set_scanMode(bool b);
    void startDumping(SNDFILE *f);
    void startDumping(FILE *f);
    void stopDumping();
    // the display symbol of the decoder this processor drives (ofdmDecoder::set_displayToken,
    // ofdm-decoder.h:50; the reference's ofdmProcessor owns its ofdmDecoder): 1..75, from
    // the next frame on.  A value outside 1..75 selects no symbol: in the reference such a
    // token never matches blkno (ofdm-decoder.cpp:192-195), so the display feed stops and the
    // decode goes on -- the setter keeps the last valid token and turns the feed off
    void set_displayToken(int16_t t) {
        if (t >= 1 && t <= 75) { displayToken_ = t; displayOff_ = false; }
        else displayOff_ = true;
    }
    int64_t frames() const { return frames_.load(); }
    static constexpr int32_t spectrumSize = 32768;          // bufferSize (ofdm-processor.cpp:97)
private:
    void run();
    void emit_frame(const dabgpu_frame_info &fi);
    // the reference's getSample / getSamples calls, replayed for the spectrum feed
    void consume_singles(int64_t to, const dabgpu_frame_info *fi);
    void consume_block(int64_t n, const dabgpu_frame_info *fi);
    void spectrum_emit(const dabgpu_frame_info *fi);
    void write_dump(const DSPCOMPLEX *v, int32_t n);
    virtualInput *theRig_;
    signals sig_;
    mscHandler *msc_;
    ficHandler *fic_;
    int16_t threshold_;
    uint8_t method_;
    RingBuffer<DSPCOMPLEX> *spectrumBuffer_ = nullptr, *iqBuffer_ = nullptr;
    std::thread thread_;
    std::atomic<bool> running_{false};
    std::atomic<int64_t> frames_{0};
    std::mutex ctl_;
    std::vector<int> pending_ops_;
    std::atomic<FILE *> dumpFile_{nullptr};
    std::atomic<SNDFILE *> dumpSnd_{nullptr};
    int16_t dumpScaler_ = 512;
    std::atomic<int16_t> displayToken_{ofdmDecoder::defaultDisplayToken};
    std::atomic<bool> displayOff_{false};
    // observables state
    int64_t last_block0_ = -1;
    int32_t avgTokenLength_ = 196608, tokenCount_ = 0;
    int16_t snr_ = 0, snrCount_ = 0;
    int32_t no_signal_ = 0, resyncs_ = 0;
    bool synced_ = false;
    // spectrum feed replay: samples consumed, sampleCnt, first sample of localBuffer
    int64_t consumed_ = 0, spec_cnt_ = 0, spec_start_ = 0;
    int16_t last_fine_ = 0;
    int32_t last_coarse_ = 0;
    // the device sample window (run()): the spectrum block is read back from it
    const float *win_ = nullptr;
    int64_t win_base_ = 0;
    std::vector<DSPCOMPLEX> specbuf_;
};

// The streaming engine: ofdmProcessor::run + ficHandler + mscHandler (+ DAB+
// mp4Processor layer) for many ensembles at once (dabgpu_pipe_*).  Each stream's
// cf32 samples are handed over as host arrays (a recorded or synthetic
// virtualInput); they are uploaded once and decoded n_frames at a time.
class ensembleDecoder {
public:
    struct config {
        int n_streams = 1;
        int n_frames = 8;                    // frames per step
        int16_t threshold = 3;               // gui.cpp:98-99
        std::vector<dabgpu_subch> subch;     // every stream's initial table (set_subch replaces a stream's)
        // dabgpu_pipe_caps: table entries, largest bitRate and DAB+ entries a stream's table
        // may hold (0: what subch needs)
        int max_subch = 0, max_bitrate = 0, max_dabplus = 0;
        int max_mp2 = 0;                     // layer II (DABGPU_SUBCH_MP2) entries likewise
        // dabgpu_pipe_audio_caps: layer II entries also flagged DABGPU_SUBCH_AUDIO a stream's table
        // may hold (0: what subch flags; at most max_mp2)
        int max_audio = 0;
        // dabgpu_pipe_packet_caps: packet-mode (DABGPU_SUBCH_PACKET) entries a stream's table may
        // hold (0: what subch flags) and the largest data group (0: DABGPU_PKT_GROUP_BYTES)
        int max_packet = 0, max_group_bytes = 0;
        // dabgpu_pipe_mot_caps: entries also flagged DABGPU_SUBCH_MOT a stream's table may hold
        // (0: what subch flags; at most max_packet) and the largest MOT body (0: DABGPU_MOT_BODY_BYTES)
        int max_mot = 0, max_body_bytes = 0;
        // dabgpu_pipe_pad_caps: DAB+ entries also flagged DABGPU_SUBCH_PAD a stream's table may hold
        // (0: what subch flags; at most max_dabplus)
        int max_pad = 0;
        // FIC first: each stream's table follows its own FIG 0/1 and 0/2 (a fib_processor per
        // stream, fed its CRC-good FIBs).  At the end of a step() a stream's parsed table is
        // applied (set_subch) when it is non-empty, equals the one parsed at the end of the
        // previous step and differs from the applied one; one that exceeds the caps throws
        // dabgpu::error.
        bool auto_layout = false;
        // With auto_layout: the FIBs are parsed on the GPU (dabgpu_pipe_fic, a database per stream
        // on the device) instead of by the host's fib_processors.  step() then downloads the run
        // records, tables and events, applies the same rule to the device's table, and moves the
        // FIC to the host only while on_fib is set.
        bool fic_on_gpu = false;
    };
    using fib_cb = std::function<void(int stream, int64_t frame, int ficno, const uint8_t *bits256, bool crc_ok)>;
    using msc_cb = std::function<void(int stream, int64_t cif, int subch, const uint8_t *bits, int nbits)>;
    using sf_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_superframe &info,
                                     const uint8_t *bytes, int nbytes)>;
    explicit ensembleDecoder(const config &cfg);
    ~ensembleDecoder();
    void on_fib(fib_cb f) { fic_.on_fib = std::move(f); }
    void on_msc(msc_cb f) { msc_.on_msc = std::move(f); }
    void on_superframe(sf_cb f) { dabplus_.on_superframe = std::move(f); }
    // With auto_layout: the signals nameofEnsemble (FIG 1/0, once until clearEnsemble) and
    // addtoEnsemble (FIG 1/1, once per service) of each stream's fib_processor, from the host's
    // parse or, with fic_on_gpu, from the device's events: frame is the frame whose FIB carried
    // the label, the text UTF-8 (fib_processor::label_text), 16 characters as transmitted.
    using ensemble_name_cb = std::function<void(int stream, int64_t frame, uint32_t EId, const std::string &name)>;
    using service_name_cb = std::function<void(int stream, int64_t frame, const std::string &label)>;
    void on_ensemble_name(ensemble_name_cb f) { fic_.on_ensemble_name = std::move(f); }
    void on_service_name(service_name_cb f) { fic_.on_service_name = std::move(f); }
    // With auto_layout: the stream's service database as a fib_processor -- the host's own, or
    // with fic_on_gpu one loaded from the device's record (dabgpu_pipe_fic_db, import_db) -- to ask
    // kindofService / dataforAudioService / dataforDataService / serviceLabels.
    fib_processor database(int stream) const;
    // Decoded classic DAB audio, where audioSink::audioOut stands in the reference
    // (mp2processor.cpp:584-588): one call per MPEG layer II frame of an entry flagged
    // DABGPU_SUBCH_MP2 that mp2decodeFrame accepted (dabgpu_pipe_mp2), pcm = n_samples
    // (1152) stereo pairs, rate = the processor's baudRate (48000 or 24000); cif is the CIF
    // in which the frame completed.  With auto_layout, sub-channels whose audio component
    // has ASCTy 0 are flagged when this callback is set before the table is applied.
    using pcm_cb = std::function<void(int stream, int64_t cif, int subch, const int16_t *pcm, int n_samples, int rate)>;
    void on_pcm(pcm_cb f) { mp2_.on_pcm = std::move(f); }
    // The same audio as audioSink::audioOut puts it into _O_Buffer (audiosink.cpp:235-360): 48 kHz
    // float stereo pairs, 24 kHz frames interpolated by the reference's LowPassFIR (dabgpu_pipe_audio
    // after the step's dabgpu_pipe_mp2), for the entries flagged DABGPU_SUBCH_MP2 |
    // DABGPU_SUBCH_AUDIO: one call per accepted frame (n_pairs 1152 or 2304), after the step's on_pcm
    // calls; a caller concatenates an entry's calls to its signal.  With auto_layout, sub-channels
    // whose audio component has ASCTy 0 are flagged DABGPU_SUBCH_MP2 | DABGPU_SUBCH_AUDIO when this
    // callback is set before the table is applied (config::max_mp2 and max_audio say how many).
    // With the callback unset nothing is flagged, allocated or launched.
    using audio_cb = std::function<void(int stream, int64_t cif, int subch, const float *samples, int n_pairs)>;
    void on_audio(audio_cb f) { audio_.on_audio = std::move(f); }
    // MSC data groups of the packet-mode entries (DABGPU_SUBCH_PACKET, dabgpu_pipe_packet), where
    // my_dataHandler->add_mscDatagroup stands in the reference (msc-datagroup.cpp:285, :304):
    // one call per completed group, accepted or not, as bytes (the reference passes one bit per
    // byte) with its parsed header; nbytes is what is stored, min(g.nbytes, max_group_bytes);
    // cif is the CIF of the packet that completed it.  With auto_layout, sub-channels with a
    // packet-mode component (not DSCTy 5 with the DG flag) are flagged when this callback is
    // set before the table is applied.
    using datagroup_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_datagroup &g,
                                            const uint8_t *bytes, int nbytes)>;
    void on_datagroup(datagroup_cb f) { packet_.on_datagroup = std::move(f); }
    // show_mscErrors (msc-datagroup.cpp:250-254): 100 - crcErrors / 5 per 500 handled packets
    using packet_quality_cb = std::function<void(int stream, int64_t cif, int subch, int value)>;
    void on_packet_quality(packet_quality_cb f) { packet_.on_quality = std::move(f); }
    // MOT objects of the packet-mode entries also flagged DABGPU_SUBCH_MOT (dabgpu_pipe_mot, after
    // the step's dabgpu_pipe_packet), where motHandler emits the_picture or fopens (mot-data.cpp:
    // 315-346): one call per completed object in completion order, after the step's on_datagroup
    // calls; body holds o.nbytes bytes (none for DABGPU_MOT_EPG or with DABGPU_MOT_OVERFLOW); cif
    // is the CIF of the group that completed it.  With auto_layout, sub-channels with a DSCTy 60
    // packet-mode component are flagged DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT when this callback
    // is set before the table is applied (config::max_packet and max_mot say how many).
    using mot_object_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_mot_object &o,
                                             const uint8_t *body)>;
    void on_mot_object(mot_object_cb f) { mot_.on_object = std::move(f); }
    // UDP payloads of the packet-mode entries also flagged DABGPU_SUBCH_IP (dabgpu_pipe_ip, after the
    // step's dabgpu_pipe_packet), where ip_dataHandler emits writeDatagram (ip-datahandler.cpp:
    // 124-127), and the numbers it emits with show_ipErrors every 100 datagrams: in group order,
    // a group's quality before its datagram, after the step's on_datagroup calls; cif is the CIF of
    // the group that held the datagram.  With auto_layout, sub-channels with a DSCTy 59 packet-mode
    // component are flagged DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP when on_datagram is set before the
    // table is applied (config::max_packet says how many).
    using datagram_cb = std::function<void(int stream, int subch, int64_t cif, const uint8_t *bytes, int n)>;
    using ip_quality_cb = std::function<void(int stream, int subch, int value)>;
    void on_datagram(datagram_cb f) { ip_.on_datagram = std::move(f); }
    void on_ip_quality(ip_quality_cb f) { ip_.on_quality = std::move(f); }
    // DAB+ PAD of the entries flagged DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD (dabgpu_pipe_pad after
    // the step's dabgpu_pipe_dabplus): the dynamic label where padHandler emits showLabel (the
    // record holds the bytes, pieces and charSet the reference hands to toQStringUsingCharset:
    // INTEGRATION section 6), every completed X-PAD data group with its bytes (g.flags &
    // DABGPU_DG_ACCEPTED: the ones padHandler hands to its motHandler), and, with on_pad_object
    // set, the slides and files of padHandler::my_motHandler: the decoder then owns one MOT state
    // per stream and PAD slot and runs dabgpu_mot_groups on the layer's groups.  (A stream's
    // set_subch that changes its PAD entries gives the stream new MOT states.)  cif is the CIF of
    // the AU that completed the label or group.  With auto_layout, DAB+ audio components are
    // flagged DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD when one of the three is set before the table
    // is applied (config::max_pad says how many).
    using dynamic_label_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_pad_label &l)>;
    using pad_datagroup_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_datagroup &g,
                                                const uint8_t *bytes, int nbytes)>;
    using pad_object_cb = std::function<void(int stream, int64_t cif, int subch, const dabgpu_mot_object &o,
                                             const uint8_t *body)>;
    void on_dynamic_label(dynamic_label_cb f) { pad_.on_label = std::move(f); }
    void on_pad_datagroup(pad_datagroup_cb f) { pad_.on_datagroup = std::move(f); }
    void on_pad_object(pad_object_cb f) { pad_mot_.on_object = std::move(f); }
    // samples[s] -> n[s] cf32 samples of stream s (copied to HBM)
    void load(const std::vector<const DSPCOMPLEX *> &samples, const std::vector<int64_t> &n);
    // the streams as recorded: format DABGPU_IQ_S16 (.sdr PCM16 I/Q pairs) or DABGPU_IQ_U8
    // (.raw bytes), n[s] pairs each, copied to HBM as they are -- the pipeline converts them
    // in its sample loads with the readers' scaling (wavfiles.cpp:172, rawfiles.cpp:115-117)
    void load_recorded(int format, const std::vector<const void *> &samples, const std::vector<int64_t> &n);
    // streams sampled at rate Hz (whole kHz, 2048000 .. 10000000), n[s] I/Q pairs each in format
    // DABGPU_IQ_S12 (the Airspy's int16 pairs, x / 2048), _S16, _U8 or _F32: uploaded as they are, in
    // pieces, and converted on the device to the 2.048 MHz cf32 the decoder then holds, as
    // airspyHandler::data_available converts them (dabgpu_rate_convert; rate_converter.h is the same
    // on the host).  Stream s then holds 2048 * ((n[s] - 1) / (rate / 1000)) samples, as after load.
    void load_rate(int rate, int format, const std::vector<const void *> &samples, const std::vector<int64_t> &n);
    // one recording file per stream, all .sdr (RIFF/WAVE PCM16, 2 channels, 2048000 Hz, as
    // wavFiles accepts them: wavfiles.cpp:56-69) or all .raw (u8 I/Q): read in pieces straight
    // into HBM, unconverted.  Throws dabgpu::error for any other file.
    void load_files(const std::vector<std::string> &paths);
    // null search (ofdm-processor.cpp:274-338) for every unsynchronised stream from its
    // current position (optional: step() acquires such streams itself)
    void acquire();
    // decode the next n_frames frames of every stream (a stream that loses sync searches
    // the next null symbol and continues, as ofdmProcessor::run); false when a stream
    // ran out of samples (the frames it decoded were delivered)
    bool step();
    dabgpu_stream_state state(int stream) const;
    // Replace the table of one stream (-1: of every stream) for the steps that follow
    // (dabgpu_pipe_set_subch: unchanged entries go on, the others deliver from the stream's
    // current CIF + 16).  The subch argument of msc_cb / sf_cb is the entry's index in its
    // stream's table.
    void set_subch(int stream, const std::vector<dabgpu_subch> &subch);
    // the stream's table (dabgpu_pipe_get_subch); since_cif (optional) per entry
    std::vector<dabgpu_subch> get_subch(int stream, std::vector<int64_t> *since_cif = nullptr) const;
private:
    // (the implementation: ensemble_decoder.cpp)
    // a typed device array: devbuf in counts of T
    template <class T> class devarr {
    public:
        void resize(size_t n) { b_.resize(n * sizeof(T)); }
        T *get() const { return static_cast<T *>(b_.get()); }
        size_t size() const { return b_.size() / sizeof(T); }
        void upload(const std::vector<T> &h) { b_.upload(h.data(), h.size() * sizeof(T)); }
        // elements [first, first + count) into h (h keeps at least one element, so h.data() stands)
        void download(std::vector<T> &h, size_t first, size_t count) const;
    private:
        devbuf b_;
    };
    // what a layer leaves per element e = stream * slots of the layer + slot: up to `slots` records and
    // their bytes, packed into an arena of `arena` bytes
    template <class T> struct slot_store {
        devarr<T> records;
        devarr<uint8_t> bytes;
        size_t slots = 0, arena = 0;
        void resize(size_t elements, size_t slots_each, size_t arena_each) {
            slots = slots_each;
            arena = arena_each;
            bytes.resize(elements * arena);
            records.resize(elements && slots ? elements * slots : 1);
        }
        // element e's first n records and the first nbytes of its arena: what the run completed
        void fetch(size_t e, int n, int nbytes, std::vector<T> &r, std::vector<uint8_t> &b) const {
            records.download(r, e * slots, (size_t)n);
            bytes.download(b, e * arena, (size_t)nbytes);
        }
    };
    // One struct per layer, in the order of a step: n is the layer's slot count per stream
    struct {                                          // FIC: the run's FIBs and CRC flags
        devarr<uint8_t> fibs, crc;
        devarr<dabgpu_fic_event> events;              // fic_on_gpu: the FIC layer's events, tables, run records
        devarr<dabgpu_fic_table> tables;
        devarr<dabgpu_fic_run> runs;
        std::vector<dabgpu_fic_table> table;          // fic_on_gpu: [stream] the tables of this step
        std::vector<fib_processor> parser;            // auto_layout: [stream]
        int64_t frame = 0;                            // the frame of the FIB the host's fib_processor is parsing
        fib_cb on_fib;
        ensemble_name_cb on_ensemble_name;
        service_name_cb on_service_name;
    } fic_;
    struct {                                          // MSC rows, packed
        int n = 0, stride = 0, maxbits = 0;
        devarr<uint8_t> rows;
        msc_cb on_msc;
    } msc_;
    struct {                                          // DAB+ superframes
        int n = 0, stride = 0;
        devarr<uint8_t> bytes;
        devarr<dabgpu_superframe> info;
        sf_cb on_superframe;
    } dabplus_;
    struct {                                          // PAD: label records, X-PAD groups, run records
        int n = 0;
        devarr<dabgpu_pad_label> labels;
        slot_store<dabgpu_datagroup> groups;
        devarr<dabgpu_pad_run> runs;
        dynamic_label_cb on_label;
        pad_datagroup_cb on_datagroup;
    } pad_;
    struct {                                          // on_pad_object (first use): a MOT state per stream and PAD slot
        devarr<uint8_t> states;
        devarr<dabgpu_packet_run> group_runs;         // what dabgpu_mot_groups reads: the PAD layer's run records
        slot_store<dabgpu_mot_object> objects;
        devarr<dabgpu_mot_run> runs;
        pad_object_cb on_object;
    } pad_mot_;
    struct {                                          // layer II PCM
        int n = 0;
        devarr<int16_t> pcm;
        devarr<dabgpu_mp2_info> info;
        pcm_cb on_pcm;
    } mp2_;
    struct {                                          // audio output (buffers on first use): samples and pair counts
        int n = 0;
        devarr<float> samples;
        devarr<int32_t> pairs;
        audio_cb on_audio;
    } audio_;
    struct {                                          // packet mode: data groups, run records, per-CIF records
        int n = 0, cap = 0;                           // cap: the largest stored group
        slot_store<dabgpu_datagroup> groups;
        devarr<dabgpu_packet_run> runs;
        devarr<dabgpu_packet_info> info;
        datagroup_cb on_datagroup;
        packet_quality_cb on_quality;
    } packet_;
    struct {                                          // MOT objects of the packet entries
        int n = 0;
        slot_store<dabgpu_mot_object> objects;
        devarr<dabgpu_mot_run> runs;
        mot_object_cb on_object;
    } mot_;
    struct {                                          // IP (first use): a result per group of the packet slots
        slot_store<dabgpu_ip_result> results;
        devarr<dabgpu_ip_run> runs;
        datagram_cb on_datagram;
        ip_quality_cb on_quality;
    } ip_;
    config cfg_;
    dabgpu_pipe *pipe_ = nullptr;
    devbuf iq_;                                       // the streams' samples as loaded (cf32, s16 or u8 pairs)
    int64_t stride_ = 0;
    std::vector<int64_t> navail_;
    std::vector<std::vector<dabgpu_subch>> tab_;      // [stream] the applied tables
    std::vector<std::vector<dabgpu_subch>> parsed_;   // auto_layout: [stream] parsed at the end of the last step
    std::vector<int64_t> frames_done_;                // frames delivered per stream
    std::vector<dabgpu_frame_info> frame_info_;       // [stream][frame] of this step
    void start_auto_layout();
    // the loaders' shared start (one array per stream, stride_, iq_ sized) and end
    void begin_load(const char *who, size_t given, const std::vector<int64_t> &n, size_t bytes_per_pair);
    void finish_load(const std::vector<int64_t> &n, int format);
    char *stream_iq(int s, size_t bytes_per_pair) const { return static_cast<char *>(iq_.get()) + bytes_per_pair * stride_ * s; }
    bool gpu_fic() const { return cfg_.auto_layout && cfg_.fic_on_gpu; }
    int wanted() const;                               // the DABGPU_SUBCH_* bits auto_layout asks the FIC for
    // step(), in this order
    bool run_pipeline();
    void deliver_fic_names();
    void deliver_fibs();
    void deliver_msc();
    void run_dabplus();
    void run_pad();
    void run_pad_mot(const std::vector<dabgpu_pad_run> &run, std::vector<dabgpu_mot_run> &mrun);
    void deliver_pad(const std::vector<dabgpu_pad_run> &run, const std::vector<dabgpu_mot_run> &mrun);
    void run_mp2();
    void run_audio();
    void run_packet();
    void run_mot();
    void run_ip();
    void advance_frames();
    void apply_tables();
};

}  // namespace dabgpu
