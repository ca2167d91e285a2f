// dabgpu_dropin.cpp -- see dabgpu_dropin.h.  Every class is a thin host shell over
// the C ABI: buffers are allocated once per object, each call is one upload, one
// (or a few) kernel launches and one download on the thread's HIP stream.
#include "dabgpu_dropin.h"

#include <cstdio>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

namespace dabgpu {

namespace {
int g_device = 0;

struct ctx_holder {
    dabgpu_ctx *c = nullptr;
    ~ctx_holder() {
        if (c) dabgpu_ctx_destroy(c);
    }
};
thread_local ctx_holder t_ctx;

void chk(int rc, const char *what) {
    if (rc != DABGPU_OK) throw error(rc, std::string(what) + ": " + dabgpu_last_error());
}
}  // namespace

void set_device(int device) { g_device = device; }

dabgpu_ctx *thread_context() {
    if (!t_ctx.c) chk(dabgpu_ctx_create(g_device, &t_ctx.c), "dabgpu_ctx_create");
    return t_ctx.c;
}

devbuf::~devbuf() {
    if (p_ && t_ctx.c) dabgpu_free(t_ctx.c, p_);
}

void devbuf::resize(size_t bytes) {
    if (bytes <= n_) return;
    dabgpu_ctx *c = thread_context();
    if (p_) dabgpu_free(c, p_);
    p_ = nullptr;
    n_ = 0;
    chk(dabgpu_alloc(c, bytes, &p_), "dabgpu_alloc");
    n_ = bytes;
}

void devbuf::upload(const void *h, size_t bytes) {
    resize(bytes);
    chk(dabgpu_memcpy_h2d(thread_context(), p_, h, bytes), "dabgpu_memcpy_h2d");
}

void devbuf::download(void *h, size_t bytes) const {
    chk(dabgpu_memcpy_d2h(thread_context(), h, p_, bytes), "dabgpu_memcpy_d2h");
}

// ---- viterbi family --------------------------------------------------------
viterbi::viterbi(int16_t wordlength) : wordlength_(wordlength) {
    in_.resize(sizeof(int16_t) * 4 * (wordlength + 6));
    out_.resize(wordlength + 16);
}

void viterbi::deconvolve(int16_t *input, uint8_t *output) {
    in_.upload(input, sizeof(int16_t) * 4 * (wordlength_ + 6));
    chk(dabgpu_viterbi(thread_context(), (const int16_t *)in_.get(), 1, wordlength_, (uint8_t *)out_.get()),
        "dabgpu_viterbi");
    out_.download(output, wordlength_);
}

namespace {
bool msc_one(const dabgpu_subch &sub, devbuf &in, devbuf &out, int16_t *v, int32_t size, uint8_t *outBuffer) {
    const int nbits = 24 * sub.bitRate;
    in.upload(v, sizeof(int16_t) * size);
    const int rc = dabgpu_msc_deconvolve(thread_context(), (const int16_t *)in.get(), size, &sub, 1,
                                         (uint8_t *)out.get(), nbits);
    if (rc == DABGPU_E_UNSUP || rc == DABGPU_E_ARG) return false;   // profile undefined / fragment too short
    chk(rc, "dabgpu_msc_deconvolve");
    out.download(outBuffer, nbits);
    return true;
}
}  // namespace

uep_deconvolve::uep_deconvolve(int16_t bitRate, int16_t protLevel) : viterbi(24 * bitRate) {
    sub_ = dabgpu_subch{0, 0, bitRate, protLevel, 0, DABGPU_SUBCH_RAW};
}

bool uep_deconvolve::deconvolve(int16_t *v, int32_t size, uint8_t *outBuffer) {
    return msc_one(sub_, in_, out_, v, size, outBuffer);
}

eep_deconvolve::eep_deconvolve(int16_t bitRate, int16_t protLevel) : viterbi(24 * bitRate) {
    sub_ = dabgpu_subch{0, 0, bitRate, protLevel, 1, DABGPU_SUBCH_RAW};
}

bool eep_deconvolve::deconvolve(int16_t *v, int32_t size, uint8_t *outBuffer) {
    return msc_one(sub_, in_, out_, v, size, outBuffer);
}

// ---- reedSolomon -------------------------------------------------------------
reedSolomon::reedSolomon(uint16_t symsize, uint16_t gfpoly, uint16_t fcr, uint16_t prim, uint16_t nroots) {
    if (symsize != 8 || gfpoly != 0435 || fcr != 0 || prim != 1 || nroots != 10)
        throw error(DABGPU_E_UNSUP, "reedSolomon: only the DAB+ code (8, 0435, 0, 1, 10) runs on the GPU");
    in_.resize(120);
    out_.resize(112);
    ret_.resize(16);
}

int16_t reedSolomon::dec(const uint8_t *data_in, uint8_t *data_out, int16_t cutlen) {
    if (cutlen != 135) throw error(DABGPU_E_UNSUP, "reedSolomon::dec: only cutlen 135 (RS(120,110))");
    in_.upload(data_in, 120);
    chk(dabgpu_rs_decode(thread_context(), (const uint8_t *)in_.get(), 1, (uint8_t *)out_.get(), (int16_t *)ret_.get()),
        "dabgpu_rs_decode");
    int16_t r = 0;
    out_.download(data_out, 110);
    ret_.download(&r, sizeof r);
    return r;
}

// ---- phaseReference ------------------------------------------------------------
phaseReference::phaseReference(int16_t threshold) : threshold_(threshold) {
    iq_.resize(sizeof(float) * 2 * DABGPU_TU);
    fr_.resize(sizeof(dabgpu_frame));
    si_.resize(16);
}

int32_t phaseReference::findIndex(DSPCOMPLEX *v) {
    iq_.upload(v, sizeof(float) * 2 * DABGPU_TU);
    dabgpu_frame f;
    std::memset(&f, 0, sizeof f);
    f.n_samples = DABGPU_TU;                      // samples already mixed: NCO phase 0
    fr_.upload(&f, sizeof f);
    chk(dabgpu_prs_sync(thread_context(), (const float *)iq_.get(), (const dabgpu_frame *)fr_.get(), 1, threshold_,
                        (int32_t *)si_.get(), nullptr, nullptr),
        "dabgpu_prs_sync");
    int32_t r = 0;
    si_.download(&r, sizeof r);
    return r;
}

// ---- ficHandler -------------------------------------------------------------------
// The reference's signals are queued to the GUI thread (Qt); here the FIG parser's
// events are collected under fibHandling_ and fired after it is released, so a slot may
// call back into kindofService / dataforAudioService / clearEnsemble without deadlock.
ficHandler::ficHandler(signals sig, int16_t bitsperBlock) : sig_(std::move(sig)) {
    init(bitsperBlock);
    if (sig_.nameofEnsemble)
        fibProcessor_.on_ensemble([this](uint32_t id, const std::string &name) {
            pending_.push_back([this, id, name] { sig_.nameofEnsemble(id, name); });
        });
    if (sig_.addtoEnsemble)
        fibProcessor_.on_service([this](const std::string &label) {
            pending_.push_back([this, label] { sig_.addtoEnsemble(label); });
        });
}

ficHandler::ficHandler(fib_cb cb, int16_t bitsperBlock) : cb_(std::move(cb)) { init(bitsperBlock); }

void ficHandler::init(int16_t bitsperBlock) {
    if (bitsperBlock != 2 * DABGPU_K) throw error(DABGPU_E_UNSUP, "ficHandler: Mode I (3072 bits per block) only");
    ofdm_input_.assign(2304, 0);
    in_.resize(sizeof(int16_t) * 2304);
    bits_.resize(768);
    crc_.resize(16);
}

void ficHandler::process_ficBlock(int16_t *data, int16_t blkno) {   // fic-handler.cpp:192-224
    if (!running_.load()) return;
    if (blkno == 1) {
        index_ = 0;
        ficno_ = 0;
    }
    for (int i = 0; i < 2 * DABGPU_K; i++) {
        ofdm_input_[index_++] = data[i];
        if (index_ >= 2304) {
            // process_ficInput (fic-handler.cpp:241-321) on the GPU
            in_.upload(ofdm_input_.data(), sizeof(int16_t) * 2304);
            chk(dabgpu_fic_decode(thread_context(), (const int16_t *)in_.get(), 1, (uint8_t *)bits_.get(),
                                  (uint8_t *)crc_.get()),
                "dabgpu_fic_decode");
            uint8_t bits[768], ok[3];
            bits_.download(bits, 768);
            crc_.download(ok, 3);
            std::vector<std::function<void()>> events;
            {
                std::lock_guard<std::mutex> g(fibHandling_);          // fic-handler.cpp:304-320
                for (int k = 0; k < 3; k++) {
                    total_++;
                    good_ += ok[k] ? 1 : 0;
                    if (sig_.show_ficCRC) {
                        const bool b = ok[k] != 0;
                        pending_.push_back([this, b] { sig_.show_ficCRC(b); });
                    }
                    if (ok[k]) fibProcessor_.process_FIB(bits + 256 * k, (uint16_t)ficno_);
                }
                events.swap(pending_);
            }
            for (auto &e : events) e();                               // outside the lock
            for (int k = 0; k < 3; k++)
                if (cb_) cb_(bits + 256 * k, ok[k] != 0, (int16_t)ficno_);
            index_ = 0;
            ficno_++;
        }
    }
}

int16_t ficHandler::get_ficRatio() const { return total_ ? (int16_t)(100 * good_ / total_) : 0; }

void ficHandler::clearEnsemble() {                                   // fic-handler.cpp:159-163
    std::lock_guard<std::mutex> g(fibHandling_);
    fibProcessor_.clearEnsemble();
}

uint8_t ficHandler::kindofService(const std::string &s) {           // fic-handler.cpp:165-171
    std::lock_guard<std::mutex> g(fibHandling_);
    return fibProcessor_.kindofService(s);
}

void ficHandler::dataforAudioService(const std::string &s, audiodata *d) {   // :174-178
    std::lock_guard<std::mutex> g(fibHandling_);
    (void)fibProcessor_.dataforAudioService(s, d);
}

void ficHandler::dataforDataService(const std::string &s, packetdata *d) {   // :180-184
    std::lock_guard<std::mutex> g(fibHandling_);
    (void)fibProcessor_.dataforDataService(s, d);
}

void ficHandler::stop() { running_.store(false); }                  // fic-handler.cpp:155-157

// ---- ensembleDecoder -------------------------------------------------------------
ensembleDecoder::ensembleDecoder(const config &cfg) : cfg_(cfg) {
    dabgpu_pipe_cfg pc;
    std::memset(&pc, 0, sizeof pc);
    pc.n_streams = cfg.n_streams;
    pc.n_frames = cfg.n_frames;
    pc.n_subch = (int32_t)cfg.subch.size();
    pc.threshold = cfg.threshold;
    pc.freq_sync_method = 1;
    pc.subch = cfg.subch.data();
    dabgpu_pipe_caps caps = {(int32_t)cfg.subch.size(), 0, 0, 0};        // what the table needs ...
    for (const dabgpu_subch &sc : cfg.subch) {
        caps.max_bitrate = std::max<int32_t>(caps.max_bitrate, sc.bitRate);
        if (sc.flags & DABGPU_SUBCH_DABPLUS) caps.max_dabplus++;
        if (sc.flags & DABGPU_SUBCH_MP2) caps.max_mp2++;
    }
    if (cfg.max_mp2) caps.max_mp2 = cfg.max_mp2;
    if (cfg.max_subch) caps.max_subch = cfg.max_subch;                    // ... or what the caller allows
    if (cfg.max_bitrate) caps.max_bitrate = cfg.max_bitrate;
    if (cfg.max_dabplus) caps.max_dabplus = cfg.max_dabplus;
    chk(dabgpu_pipe_create_caps(thread_context(), &pc, &caps, &pipe_), "dabgpu_pipe_create_caps");
    nsub_ = caps.max_subch;
    ndp_ = caps.max_dabplus;
    const int maxbits = std::max(768, 24 * (int)caps.max_bitrate);
    tab_.assign(cfg.n_streams, cfg.subch);
    if (cfg.auto_layout) {
        fibs_.resize(cfg.n_streams);
        parsed_.resize(cfg.n_streams);
        for (int s = 0; s < cfg.n_streams; s++)
            fibs_[s].on_event([this, s](int kind, int32_t id, const uint8_t *raw, int charset) {
                const std::string text = fib_processor::label_text(raw, 16, charset);
                if (kind == DABGPU_FIC_NAME_ENSEMBLE && ens_name_cb_) ens_name_cb_(s, fib_frame_, (uint32_t)id, text);
                if (kind == DABGPU_FIC_ADD_SERVICE && svc_name_cb_) svc_name_cb_(s, fib_frame_, text);
            });
        if (cfg.fic_on_gpu) {
            chk(dabgpu_pipe_fic_caps(pipe_, 1), "dabgpu_pipe_fic_caps");
            fce_.resize((size_t)cfg.n_streams * DABGPU_FIC_EVENT_SLOTS * sizeof(dabgpu_fic_event));
            fct_.resize((size_t)cfg.n_streams * sizeof(dabgpu_fic_table));
            fcr_.resize((size_t)cfg.n_streams * sizeof(dabgpu_fic_run));
            fic_tab_.resize(cfg.n_streams);
        }
    }
    // the MSC and the FIBs leave the GPU packed (8 bits per byte, 1/8 of the bytes over
    // PCIe) and are unpacked here for the one-bit-per-byte consumers (dab-concurrent.cpp:191,
    // fibProcessor::process_FIB)
    chk(dabgpu_pipe_set_packed(pipe_, DABGPU_PACK_MSC | DABGPU_PACK_FIC), "dabgpu_pipe_set_packed");
    msc_stride_ = ((maxbits + 7) / 8 + 15) / 16 * 16;
    maxbits_ = maxbits;
    sf_stride_ = std::max(16, 110 * (int)(caps.max_bitrate / 8));
    const size_t SF = (size_t)cfg.n_streams * cfg.n_frames;
    // only the superframes a run completes cross PCIe (DABGPU_SF_SLOTS per subchannel)
    if (ndp_) chk(dabgpu_pipe_set_dabplus_compact(pipe_, 1), "dabgpu_pipe_set_dabplus_compact");
    fic_.resize(SF * 4 * 96);
    crc_.resize(SF * 12);
    msc_.resize(std::max<size_t>(1, SF * 4 * nsub_ * msc_stride_));
    if (ndp_) {
        sf_.resize(SF * 4 * ndp_ * sf_stride_);
        sfi_.resize(SF * 4 * ndp_ * sizeof(dabgpu_superframe));
    }
    nmp_ = caps.max_mp2;
    if (nmp_) {
        pcm_.resize(SF * 4 * nmp_ * 2304 * sizeof(int16_t));
        mp2i_.resize(SF * 4 * nmp_ * sizeof(dabgpu_mp2_info));
    }
    for (const dabgpu_subch &sc : cfg.subch)
        if (sc.flags & DABGPU_SUBCH_AUDIO) naudio_++;
    if (cfg.max_audio) {
        naudio_ = cfg.max_audio;
        chk(dabgpu_pipe_audio_caps(pipe_, naudio_), "dabgpu_pipe_audio_caps");
    }
    for (const dabgpu_subch &sc : cfg.subch)
        if (sc.flags & DABGPU_SUBCH_PACKET) npk_++;
    pk_cap_ = cfg.max_group_bytes ? cfg.max_group_bytes : DABGPU_PKT_GROUP_BYTES;
    if (cfg.max_packet || cfg.max_group_bytes) {
        npk_ = cfg.max_packet ? cfg.max_packet : npk_;
        chk(dabgpu_pipe_packet_caps(pipe_, npk_, cfg.max_group_bytes), "dabgpu_pipe_packet_caps");
    }
    if (npk_) {
        pk_slots_ = DABGPU_PKT_GROUP_SLOTS(cfg.n_frames, (int)caps.max_bitrate);
        pk_arena_ = DABGPU_PKT_ARENA_BYTES((size_t)cfg.n_frames, (int)caps.max_bitrate, pk_cap_);
        const size_t ne = (size_t)cfg.n_streams * npk_;
        pkb_.resize(ne * pk_arena_);
        pkg_.resize(std::max<size_t>(1, ne * pk_slots_) * sizeof(dabgpu_datagroup));
        pkr_.resize(ne * sizeof(dabgpu_packet_run));
        pki_.resize(SF * 4 * npk_ * sizeof(dabgpu_packet_info));
    }
    for (const dabgpu_subch &sc : cfg.subch)
        if (sc.flags & DABGPU_SUBCH_MOT) nmot_++;
    if (cfg.max_mot || cfg.max_body_bytes) {
        nmot_ = cfg.max_mot ? cfg.max_mot : nmot_;
        chk(dabgpu_pipe_mot_caps(pipe_, nmot_, cfg.max_body_bytes), "dabgpu_pipe_mot_caps");
    }
    for (const dabgpu_subch &sc : cfg.subch)
        if (sc.flags & DABGPU_SUBCH_PAD) npad_++;
    if (cfg.max_pad) {
        npad_ = cfg.max_pad;
        chk(dabgpu_pipe_pad_caps(pipe_, npad_), "dabgpu_pipe_pad_caps");
    }
    if (npad_) {
        pad_slots_ = DABGPU_PAD_LABEL_SLOTS(cfg.n_frames);
        pad_arena_ = DABGPU_PAD_ARENA_BYTES((size_t)cfg.n_frames);
        const size_t ne = (size_t)cfg.n_streams * npad_;
        pdl_.resize(ne * pad_slots_ * sizeof(dabgpu_pad_label));
        pdg_.resize(ne * pad_slots_ * sizeof(dabgpu_datagroup));
        pdb_.resize(ne * pad_arena_);
        pdr_.resize(ne * sizeof(dabgpu_pad_run));
    }
    if (nmot_) {
        mot_arena_ = DABGPU_MOT_ARENA_BYTES((size_t)cfg.n_frames, (int)caps.max_bitrate,
                                            (size_t)(cfg.max_body_bytes ? cfg.max_body_bytes : DABGPU_MOT_BODY_BYTES));
        const size_t ne = (size_t)cfg.n_streams * nmot_;
        mob_.resize(ne * mot_arena_);
        moo_.resize(std::max<size_t>(1, ne * pk_slots_) * sizeof(dabgpu_mot_object));
        mor_.resize(ne * sizeof(dabgpu_mot_run));
    }
}

void ensembleDecoder::set_subch(int stream, const std::vector<dabgpu_subch> &subch) {
    chk(dabgpu_pipe_set_subch(pipe_, stream, subch.data(), (int32_t)subch.size()), "dabgpu_pipe_set_subch");
    auto pads = [](const std::vector<dabgpu_subch> &t) {
        std::vector<dabgpu_subch> v;
        for (const dabgpu_subch &e : t)
            if (e.flags & DABGPU_SUBCH_PAD) v.push_back(e);
        return v;
    };
    for (int s = 0; s < cfg_.n_streams; s++) {
        if (stream >= 0 && s != stream) continue;
        // the PAD slots' MOT states (on_pad_object): new ones unless the stream's PAD entries stay as they are
        const std::vector<dabgpu_subch> a = pads(tab_[s]), b = pads(subch);
        if (pms_.size() && (a.size() != b.size() || (!a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(dabgpu_subch))))) {
            const size_t sb = dabgpu_mot_state_bytes(0);
            chk(dabgpu_memset_d(thread_context(), (uint8_t *)pms_.get() + (size_t)s * npad_ * sb, 0, (size_t)npad_ * sb), "dabgpu_memset_d");
        }
        tab_[s] = subch;
    }
}

std::vector<dabgpu_subch> ensembleDecoder::get_subch(int stream, std::vector<int64_t> *since_cif) const {
    std::vector<dabgpu_subch> v(std::max(1, nsub_));
    std::vector<int64_t> since(v.size());
    int32_t n = 0;
    chk(dabgpu_pipe_get_subch(pipe_, stream, v.data(), &n, since.data()), "dabgpu_pipe_get_subch");
    v.resize(n);
    since.resize(n);
    if (since_cif) *since_cif = since;
    return v;
}

ensembleDecoder::~ensembleDecoder() {
    if (pipe_) dabgpu_pipe_destroy(pipe_);
}

void ensembleDecoder::load(const std::vector<const DSPCOMPLEX *> &samples, const std::vector<int64_t> &n) {
    if ((int)samples.size() != cfg_.n_streams || (int)n.size() != cfg_.n_streams)
        throw error(DABGPU_E_ARG, "ensembleDecoder::load: one sample array per stream");
    stride_ = 0;
    for (int64_t k : n) stride_ = std::max(stride_, k);
    iq_.resize(sizeof(float) * 2 * (size_t)stride_ * cfg_.n_streams);
    for (int s = 0; s < cfg_.n_streams; s++)
        chk(dabgpu_memcpy_h2d(thread_context(), (float *)iq_.get() + 2 * stride_ * s, samples[s],
                              sizeof(float) * 2 * n[s]),
            "dabgpu_memcpy_h2d");
    navail_ = n;
    frames_done_.assign(cfg_.n_streams, 0);
    chk(dabgpu_pipe_set_iq_format(pipe_, DABGPU_IQ_F32), "dabgpu_pipe_set_iq_format");
}

void ensembleDecoder::load_recorded(int format, const std::vector<const void *> &samples, const std::vector<int64_t> &n) {
    if ((int)samples.size() != cfg_.n_streams || (int)n.size() != cfg_.n_streams)
        throw error(DABGPU_E_ARG, "ensembleDecoder::load_recorded: one sample array per stream");
    if (format != DABGPU_IQ_S16 && format != DABGPU_IQ_U8)
        throw error(DABGPU_E_ARG, "ensembleDecoder::load_recorded: format DABGPU_IQ_S16 or DABGPU_IQ_U8");
    const size_t bps = format == DABGPU_IQ_S16 ? 4 : 2;      // bytes per I/Q pair
    stride_ = 0;
    for (int64_t k : n) stride_ = std::max(stride_, k);
    iq_.resize(bps * (size_t)stride_ * cfg_.n_streams);
    for (int s = 0; s < cfg_.n_streams; s++)
        chk(dabgpu_memcpy_h2d(thread_context(), (char *)iq_.get() + bps * stride_ * s, samples[s], bps * n[s]),
            "dabgpu_memcpy_h2d");
    navail_ = n;
    frames_done_.assign(cfg_.n_streams, 0);
    chk(dabgpu_pipe_set_iq_format(pipe_, format), "dabgpu_pipe_set_iq_format");
}

namespace {
// the data chunk of an .sdr recording: what wavFiles accepts (wavfiles.cpp:56-69 via
// libsndfile: 2 channels, 2048000 Hz, 16-bit PCM; WAVE_FORMAT_EXTENSIBLE with the PCM
// subformat too).  Returns the payload's byte offset and size.
std::pair<int64_t, int64_t> sdr_payload(std::FILE *f, const std::string &path) {
    auto u32 = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
    auto u16 = [](const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8; };
    uint8_t h[12];
    if (std::fread(h, 1, 12, f) != 12 || std::memcmp(h, "RIFF", 4) || std::memcmp(h + 8, "WAVE", 4))
        throw error(DABGPU_E_ARG, path + ": not a RIFF/WAVE file");
    int64_t off = 12;
    bool fmt_ok = false, have_fmt = false;
    for (;;) {
        uint8_t ck[8];
        if (std::fread(ck, 1, 8, f) != 8) throw error(DABGPU_E_ARG, path + ": no data chunk");
        const int64_t n = u32(ck + 4);
        off += 8;
        if (!std::memcmp(ck, "fmt ", 4)) {
            std::vector<uint8_t> b((size_t)n);
            if (n < 16 || std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) throw error(DABGPU_E_ARG, path + ": bad fmt chunk");
            uint32_t tag = u16(&b[0]);
            if (tag == 0xFFFE && n >= 26) tag = u16(&b[24]);       // WAVE_FORMAT_EXTENSIBLE: the subformat
            fmt_ok = tag == 1 && u16(&b[2]) == 2 && u32(&b[4]) == 2048000 && u16(&b[14]) == 16;
            have_fmt = true;
            if (n & 1) std::fseek(f, 1, SEEK_CUR);
        } else if (!std::memcmp(ck, "data", 4)) {
            if (!have_fmt || !fmt_ok)
                throw error(DABGPU_E_ARG, path + ": not a recorded DAB file (need PCM16, 2 channels, 2048000 Hz)");
            return {off, n};
        } else {
            std::fseek(f, (long)(n + (n & 1)), SEEK_CUR);
        }
        off += n + (n & 1);
    }
}
}  // namespace

void ensembleDecoder::load_files(const std::vector<std::string> &paths) {
    if ((int)paths.size() != cfg_.n_streams) throw error(DABGPU_E_ARG, "ensembleDecoder::load_files: one file per stream");
    auto is_raw = [](const std::string &p) { return p.size() >= 4 && p.compare(p.size() - 4, 4, ".raw") == 0; };
    const bool raw = !paths.empty() && is_raw(paths[0]);
    for (const std::string &p : paths)
        if (is_raw(p) != raw) throw error(DABGPU_E_ARG, "ensembleDecoder::load_files: .raw and .sdr files mixed");
    const int format = raw ? DABGPU_IQ_U8 : DABGPU_IQ_S16;
    const size_t bps = raw ? 2 : 4;
    struct closer { void operator()(std::FILE *f) const { if (f) std::fclose(f); } };
    std::vector<std::unique_ptr<std::FILE, closer>> files;
    std::vector<std::pair<int64_t, int64_t>> payload;
    std::vector<int64_t> n;
    for (const std::string &p : paths) {
        std::unique_ptr<std::FILE, closer> f(std::fopen(p.c_str(), "rb"));
        if (!f) throw error(DABGPU_E_ARG, p + ": cannot open");
        std::pair<int64_t, int64_t> pl{0, 0};
        if (raw) {
            std::fseek(f.get(), 0, SEEK_END);
            pl = {0, (int64_t)std::ftell(f.get())};
        } else {
            pl = sdr_payload(f.get(), p);
            std::fseek(f.get(), 0, SEEK_END);
            pl.second = std::min<int64_t>(pl.second, (int64_t)std::ftell(f.get()) - pl.first);   // a truncated recording
        }
        n.push_back(pl.second / (int64_t)bps);
        payload.push_back(pl);
        files.push_back(std::move(f));
    }
    stride_ = 0;
    for (int64_t k : n) stride_ = std::max(stride_, k);
    iq_.resize(bps * (size_t)stride_ * cfg_.n_streams);
    std::vector<char> piece((size_t)1 << 24);
    for (int s = 0; s < cfg_.n_streams; s++) {
        std::FILE *f = files[s].get();
        std::fseek(f, (long)payload[s].first, SEEK_SET);
        for (int64_t done = 0, total = n[s] * (int64_t)bps; done < total;) {
            const size_t want = (size_t)std::min<int64_t>((int64_t)piece.size(), total - done);
            if (std::fread(piece.data(), 1, want, f) != want) throw error(DABGPU_E_ARG, paths[s] + ": short read");
            chk(dabgpu_memcpy_h2d(thread_context(), (char *)iq_.get() + bps * stride_ * s + done, piece.data(), want),
                "dabgpu_memcpy_h2d");
            done += (int64_t)want;
        }
    }
    navail_ = n;
    frames_done_.assign(cfg_.n_streams, 0);
    chk(dabgpu_pipe_set_iq_format(pipe_, format), "dabgpu_pipe_set_iq_format");
}

void ensembleDecoder::acquire() {
    // unsynchronised streams search from where they are (sample 0 for a new decoder,
    // the position after a sync loss otherwise: notSynced continues, ofdm-processor.cpp:274)
    std::vector<int64_t> start(cfg_.n_streams, 0);
    for (int s = 0; s < cfg_.n_streams; s++) {
        dabgpu_stream_state st;
        chk(dabgpu_pipe_state(pipe_, s, &st), "dabgpu_pipe_state");
        start[s] = st.next_pos;
    }
    const int rc = dabgpu_pipe_acquire(pipe_, (const float *)iq_.get(), stride_, start.data(), navail_.data());
    if (rc != DABGPU_OK && rc != DABGPU_E_STATE) chk(rc, "dabgpu_pipe_acquire");
}

bool ensembleDecoder::step() {
    const int S = cfg_.n_streams, F = cfg_.n_frames, NS = nsub_;
    std::vector<uint8_t> valid((size_t)S * 4 * F);
    const int rc = dabgpu_pipe_run(pipe_, (const float *)iq_.get(), stride_, navail_.data(), (uint8_t *)fic_.get(),
                                   (uint8_t *)crc_.get(), NS ? (uint8_t *)msc_.get() : nullptr, msc_stride_,
                                   valid.data());
    if (rc != DABGPU_OK && rc != DABGPU_E_STATE) chk(rc, "dabgpu_pipe_run");
    const bool ok = rc == DABGPU_OK;
    const bool gpu_fic = cfg_.auto_layout && cfg_.fic_on_gpu;
    if (gpu_fic) {                 // behind the run's FIC decode, on its back-end stream
        const int want = ((pcm_cb_ || (audio_cb_ && naudio_ > 0)) && nmp_ > 0 ? DABGPU_SUBCH_MP2 : 0) | (dg_cb_ && npk_ > 0 ? DABGPU_SUBCH_PACKET : 0) |
                         (mot_cb_ && nmot_ > 0 ? DABGPU_SUBCH_MOT : 0) | (ip_cb_ && npk_ > 0 ? DABGPU_SUBCH_IP : 0) |
                         ((label_cb_ || pad_dg_cb_ || pad_obj_cb_) && npad_ > 0 ? DABGPU_SUBCH_PAD : 0);
        chk(dabgpu_pipe_fic(pipe_, (const uint8_t *)fic_.get(), (const uint8_t *)crc_.get(), want, (dabgpu_fic_event *)fce_.get(),
                            (dabgpu_fic_table *)fct_.get(), (dabgpu_fic_run *)fcr_.get()), "dabgpu_pipe_fic");
    }
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    // frames committed per stream (a stream that lost sync re-acquired inside the run;
    // one that ran out of samples committed fewer): FIC and MSC for those
    std::vector<dabgpu_frame_info> fr((size_t)S * F);
    chk(dabgpu_pipe_frame_info(pipe_, fr.data()), "dabgpu_pipe_frame_info");
    if (gpu_fic) {                 // the names, where the host's parse delivers them; the tables for the end of the step
        std::vector<dabgpu_fic_run> run(S);
        std::vector<dabgpu_fic_event> ev((size_t)S * DABGPU_FIC_EVENT_SLOTS);
        fcr_.download(run.data(), run.size() * sizeof(dabgpu_fic_run));
        fct_.download(fic_tab_.data(), fic_tab_.size() * sizeof(dabgpu_fic_table));
        bool any = false;
        for (const dabgpu_fic_run &r : run) any |= r.n_events > 0;
        if (any && (ens_name_cb_ || svc_name_cb_)) fce_.download(ev.data(), ev.size() * sizeof(dabgpu_fic_event));
        for (int s = 0; s < S && (ens_name_cb_ || svc_name_cb_); s++)
            for (int i = 0; i < std::min(run[s].n_events, DABGPU_FIC_EVENT_SLOTS); i++) {
                const dabgpu_fic_event &e = ev[(size_t)s * DABGPU_FIC_EVENT_SLOTS + i];
                const std::string text = fib_processor::label_text(e.label, 16, e.charset);
                if (e.kind == DABGPU_FIC_NAME_ENSEMBLE && ens_name_cb_) ens_name_cb_(s, frames_done_[s] + e.fib / 12, (uint32_t)e.id, text);
                if (e.kind == DABGPU_FIC_ADD_SERVICE && svc_name_cb_) svc_name_cb_(s, frames_done_[s] + e.fib / 12, text);
            }
    }
    if (fib_cb_ || (cfg_.auto_layout && !gpu_fic)) {
        std::vector<uint8_t> fic((size_t)S * F * 4 * 96), crc((size_t)S * F * 12);
        fic_.download(fic.data(), fic.size());
        crc_.download(crc.data(), crc.size());
        uint8_t fib[256];
        for (int s = 0; s < S; s++)
            for (int f = 0; f < F; f++) {
                if (!fr[(size_t)s * F + f].committed) continue;
                fib_frame_ = frames_done_[s] + f;
                for (int b = 0; b < 4; b++)
                    for (int k = 0; k < 3; k++) {
                        const uint8_t *pk = fic.data() + (((size_t)s * F + f) * 4 + b) * 96 + 32 * k;   // FIB bytes
                        for (int i = 0; i < 256; i++) fib[i] = (uint8_t)((pk[i >> 3] >> (7 - (i & 7))) & 1);
                        const bool good = crc[((size_t)s * F + f) * 12 + 3 * b + k] != 0;
                        if (cfg_.auto_layout && !gpu_fic && good) fibs_[s].process_FIB(fib, (uint16_t)b);
                        if (fib_cb_) fib_cb_(s, frames_done_[s] + f, b, fib, good);
                    }
            }
    }
    if (NS && msc_cb_) {
        std::vector<uint8_t> msc((size_t)S * 4 * F * NS * msc_stride_), bits(maxbits_), ev((size_t)S * 4 * F * NS);
        msc_.download(msc.data(), msc.size());
        // per entry: delivered and past the entry's own 16-CIF warm-up
        chk(dabgpu_pipe_msc_entry_valid(pipe_, ev.data()), "dabgpu_pipe_msc_entry_valid");
        for (int s = 0; s < S; s++)
            for (int c = 0; c < 4 * F; c++)
                for (int k = 0; k < (int)tab_[s].size(); k++) {
                    if (!ev[((size_t)s * 4 * F + c) * NS + k]) continue;
                    const uint8_t *pk = msc.data() + (((size_t)s * 4 * F + c) * NS + k) * msc_stride_;
                    const int nbits = 24 * tab_[s][k].bitRate;
                    for (int i = 0; i < nbits; i++) bits[i] = (uint8_t)((pk[i >> 3] >> (7 - (i & 7))) & 1);
                    msc_cb_(s, 4 * frames_done_[s] + c, k, bits.data(), nbits);
                }
    }
    if (NS && ndp_) {
        chk(dabgpu_pipe_dabplus(pipe_, (uint8_t *)sf_.get(), sf_stride_, (dabgpu_superframe *)sfi_.get()),
            "dabgpu_pipe_dabplus");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        if (sf_cb_) {
            std::vector<dabgpu_superframe> info((size_t)S * 4 * F * ndp_);
            const int slots = DABGPU_SF_SLOTS(F);
            std::vector<uint8_t> bytes((size_t)S * ndp_ * slots * sf_stride_);
            sfi_.download(info.data(), info.size() * sizeof(dabgpu_superframe));
            sf_.download(bytes.data(), bytes.size());
            // DAB+ slot d of a stream is its d-th entry flagged DABGPU_SUBCH_DABPLUS
            std::vector<std::vector<int>> dpi(S);
            for (int s = 0; s < S; s++)
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if (tab_[s][k].flags & DABGPU_SUBCH_DABPLUS) dpi[s].push_back(k);
            for (size_t r = 0; r < info.size(); r++) {
                if (info[r].status < 0) continue;
                const int d = (int)(r % ndp_);
                const int c = (int)((r / ndp_) % (4 * F));
                const int s = (int)(r / ndp_ / (4 * F));
                if (d >= (int)dpi[s].size()) continue;
                const int k = dpi[s][d];
                const int slot = info[r].reserved;           // compact output: the superframe's slot
                const bool has = info[r].status == 3 && slot < slots;
                sf_cb_(s, 4 * frames_done_[s] + c, k, info[r],
                       bytes.data() + (((size_t)s * ndp_ + d) * slots + (has ? slot : 0)) * sf_stride_,
                       has ? 110 * (tab_[s][k].bitRate / 8) : 0);
            }
        }
    }
    if (NS && ndp_ && npad_) {
        chk(dabgpu_pipe_pad(pipe_, (const uint8_t *)sf_.get(), sf_stride_, (const dabgpu_superframe *)sfi_.get(),
                            (dabgpu_pad_label *)pdl_.get(), (dabgpu_datagroup *)pdg_.get(), (uint8_t *)pdb_.get(),
                            (dabgpu_pad_run *)pdr_.get()), "dabgpu_pipe_pad");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        if (label_cb_ || pad_dg_cb_ || pad_obj_cb_) {
            const size_t ne = (size_t)S * npad_;
            std::vector<dabgpu_pad_run> run(ne);
            pdr_.download(run.data(), run.size() * sizeof(dabgpu_pad_run));
            std::vector<dabgpu_mot_run> mrun(ne);
            if (pad_obj_cb_) {
                // padHandler::my_motHandler: one MOT state per stream and PAD slot, the layer's groups as they are
                const size_t sb = dabgpu_mot_state_bytes(0);
                if (!pms_.size()) {
                    pad_mot_arena_ = DABGPU_MOT_ARENA_FOR((size_t)pad_slots_, DABGPU_MOT_BODY_BYTES);
                    pms_.resize(ne * sb);
                    chk(dabgpu_memset_d(thread_context(), pms_.get(), 0, ne * sb), "dabgpu_memset_d");
                    pmr_.resize(ne * sizeof(dabgpu_packet_run));
                    pmo_.resize(ne * pad_slots_ * sizeof(dabgpu_mot_object));
                    pmb_.resize(ne * pad_mot_arena_);
                    pmm_.resize(ne * sizeof(dabgpu_mot_run));
                }
                std::vector<dabgpu_packet_run> pr(ne);
                for (size_t e = 0; e < ne; e++) pr[e] = {std::min(run[e].n_groups, pad_slots_), run[e].n_bytes, 0, 0};
                pmr_.upload(pr.data(), pr.size() * sizeof(dabgpu_packet_run));
                chk(dabgpu_mot_groups(thread_context(), pms_.get(), (int)ne, 0, (const dabgpu_datagroup *)pdg_.get(), pad_slots_,
                                      (const uint8_t *)pdb_.get(), (int64_t)pad_arena_, (const dabgpu_packet_run *)pmr_.get(),
                                      (dabgpu_mot_object *)pmo_.get(), (uint8_t *)pmb_.get(), (int64_t)pad_mot_arena_,
                                      (dabgpu_mot_run *)pmm_.get()), "dabgpu_mot_groups");
                chk(dabgpu_sync(thread_context()), "dabgpu_sync");
                pmm_.download(mrun.data(), mrun.size() * sizeof(dabgpu_mot_run));
            }
            std::vector<dabgpu_pad_label> labels;
            std::vector<dabgpu_datagroup> groups;
            std::vector<dabgpu_mot_object> objects;
            std::vector<uint8_t> bytes;
            for (int s = 0; s < S; s++) {
                std::vector<int> slot;               // PAD slot j of a stream is its j-th entry flagged for both
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if ((tab_[s][k].flags & DABGPU_SUBCH_DABPLUS) && (tab_[s][k].flags & DABGPU_SUBCH_PAD)) slot.push_back(k);
                for (int j = 0; j < (int)slot.size() && j < npad_; j++) {
                    const size_t e = (size_t)s * npad_ + j;
                    const int nl = std::min(run[e].n_labels, pad_slots_), ng = std::min(run[e].n_groups, pad_slots_);
                    if (label_cb_ && nl > 0) {
                        labels.resize(nl);
                        chk(dabgpu_memcpy_d2h(thread_context(), labels.data(), (const dabgpu_pad_label *)pdl_.get() + e * pad_slots_,
                                              labels.size() * sizeof(dabgpu_pad_label)), "dabgpu_memcpy_d2h");
                        for (const dabgpu_pad_label &l : labels) label_cb_(s, 4 * frames_done_[s] + l.cif, slot[j], l);
                    }
                    if (pad_dg_cb_ && ng > 0) {
                        groups.resize(ng);
                        bytes.resize(std::max(1, run[e].n_bytes));
                        chk(dabgpu_memcpy_d2h(thread_context(), groups.data(), (const dabgpu_datagroup *)pdg_.get() + e * pad_slots_,
                                              groups.size() * sizeof(dabgpu_datagroup)), "dabgpu_memcpy_d2h");
                        chk(dabgpu_memcpy_d2h(thread_context(), bytes.data(), (const uint8_t *)pdb_.get() + e * pad_arena_, run[e].n_bytes),
                            "dabgpu_memcpy_d2h");
                        for (const dabgpu_datagroup &g : groups)
                            pad_dg_cb_(s, 4 * frames_done_[s] + g.cif, slot[j], g, bytes.data() + g.offset,
                                       (g.flags & DABGPU_DG_TRUNCATED) ? 0 : g.nbytes);
                    }
                    if (pad_obj_cb_ && mrun[e].n_objects > 0) {
                        objects.resize(mrun[e].n_objects);
                        bytes.resize(std::max(1, mrun[e].n_bytes));
                        chk(dabgpu_memcpy_d2h(thread_context(), objects.data(), (const dabgpu_mot_object *)pmo_.get() + e * pad_slots_,
                                              objects.size() * sizeof(dabgpu_mot_object)), "dabgpu_memcpy_d2h");
                        chk(dabgpu_memcpy_d2h(thread_context(), bytes.data(), (const uint8_t *)pmb_.get() + e * pad_mot_arena_,
                                              mrun[e].n_bytes), "dabgpu_memcpy_d2h");
                        for (const dabgpu_mot_object &o : objects)
                            pad_obj_cb_(s, 4 * frames_done_[s] + o.cif, slot[j], o, bytes.data() + o.offset);
                    }
                }
            }
        }
    }
    if (NS && nmp_) {
        chk(dabgpu_pipe_mp2(pipe_, (int16_t *)pcm_.get(), (dabgpu_mp2_info *)mp2i_.get()), "dabgpu_pipe_mp2");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        if (pcm_cb_) {
            std::vector<dabgpu_mp2_info> info((size_t)S * 4 * F * nmp_);
            std::vector<int16_t> pcm(info.size() * 2304);
            mp2i_.download(info.data(), info.size() * sizeof(dabgpu_mp2_info));
            pcm_.download(pcm.data(), pcm.size() * sizeof(int16_t));
            for (int s = 0; s < S; s++) {
                std::vector<int> slot;               // MP2 slot j of a stream is its j-th flagged entry
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if (tab_[s][k].flags & DABGPU_SUBCH_MP2) slot.push_back(k);
                for (int c = 0; c < 4 * F; c++)
                    for (int j = 0; j < (int)slot.size() && j < nmp_; j++) {
                        const size_t r = ((size_t)s * 4 * F + c) * nmp_ + j;
                        if (info[r].status == 2)
                            pcm_cb_(s, 4 * frames_done_[s] + c, slot[j], pcm.data() + r * 2304, 1152, info[r].sample_rate);
                    }
            }
        }
        bool flagged = false;                        // (an unset callback or no flagged entry: nothing is launched)
        for (int s = 0; s < S && audio_cb_ && naudio_; s++)
            for (const dabgpu_subch &e : tab_[s]) flagged |= (e.flags & DABGPU_SUBCH_AUDIO) != 0;
        if (flagged) {
            const size_t rows = (size_t)S * 4 * F * naudio_;
            if (!aus_.get()) {
                aus_.resize(rows * 2304 * 2 * sizeof(float));
                aun_.resize(rows * sizeof(int32_t));
            }
            chk(dabgpu_pipe_audio(pipe_, (const int16_t *)pcm_.get(), (const dabgpu_mp2_info *)mp2i_.get(), (float *)aus_.get(),
                                  (int32_t *)aun_.get()), "dabgpu_pipe_audio");
            chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
            std::vector<int32_t> n_out(rows);
            aun_.download(n_out.data(), rows * sizeof(int32_t));
            // one download per stream that delivered, its rows as they lie (the on_pcm path's bulk copy)
            const size_t per_stream = (size_t)4 * F * naudio_ * 2304 * 2;
            std::vector<float> samples(per_stream);
            for (int s = 0; s < S; s++) {
                std::vector<int> slot;               // audio slot j of a stream is its j-th flagged entry
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if (tab_[s][k].flags & DABGPU_SUBCH_AUDIO) slot.push_back(k);
                bool any = false;
                for (size_t r = (size_t)s * 4 * F * naudio_; r < (size_t)(s + 1) * 4 * F * naudio_; r++) any |= n_out[r] > 0;
                if (!any || slot.empty()) continue;
                chk(dabgpu_memcpy_d2h(thread_context(), samples.data(), (const float *)aus_.get() + s * per_stream,
                                      per_stream * sizeof(float)), "dabgpu_memcpy_d2h");
                for (int c = 0; c < 4 * F; c++)
                    for (int j = 0; j < (int)slot.size() && j < naudio_; j++) {
                        const size_t r = ((size_t)s * 4 * F + c) * naudio_ + j;
                        if (n_out[r] <= 0 || n_out[r] > 2304) continue;
                        audio_cb_(s, 4 * frames_done_[s] + c, slot[j], samples.data() + ((size_t)c * naudio_ + j) * 2304 * 2, n_out[r]);
                    }
            }
        }
    }
    if (NS && npk_) {
        chk(dabgpu_pipe_packet(pipe_, (uint8_t *)pkb_.get(), (dabgpu_datagroup *)pkg_.get(), (dabgpu_packet_run *)pkr_.get(),
                               (dabgpu_packet_info *)pki_.get()), "dabgpu_pipe_packet");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        if (dg_cb_ || pq_cb_) {
            // only what the run completed crosses PCIe: the run records, then per (stream,
            // slot) its group records and its arena's used bytes
            std::vector<dabgpu_packet_run> run((size_t)S * npk_);
            std::vector<dabgpu_packet_info> info((size_t)S * 4 * F * npk_);
            pkr_.download(run.data(), run.size() * sizeof(dabgpu_packet_run));
            pki_.download(info.data(), info.size() * sizeof(dabgpu_packet_info));
            std::vector<dabgpu_datagroup> groups;
            std::vector<uint8_t> bytes;
            for (int s = 0; s < S; s++) {
                std::vector<int> slot;               // packet slot j of a stream is its j-th flagged entry
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if (tab_[s][k].flags & DABGPU_SUBCH_PACKET) slot.push_back(k);
                for (int j = 0; j < (int)slot.size() && j < npk_; j++) {
                    const size_t e = (size_t)s * npk_ + j;
                    for (int c = 0; c < 4 * F && pq_cb_; c++) {
                        const dabgpu_packet_info &i = info[((size_t)s * 4 * F + c) * npk_ + j];
                        if (i.status == 0 && i.quality >= 0) pq_cb_(s, 4 * frames_done_[s] + c, slot[j], i.quality);
                    }
                    if (!dg_cb_ || run[e].n_groups <= 0) continue;
                    groups.resize(run[e].n_groups);
                    bytes.resize(std::max(1, run[e].n_bytes));
                    chk(dabgpu_memcpy_d2h(thread_context(), groups.data(), (const dabgpu_datagroup *)pkg_.get() + e * pk_slots_,
                                          groups.size() * sizeof(dabgpu_datagroup)), "dabgpu_memcpy_d2h");
                    chk(dabgpu_memcpy_d2h(thread_context(), bytes.data(), (const uint8_t *)pkb_.get() + e * pk_arena_, run[e].n_bytes),
                        "dabgpu_memcpy_d2h");
                    for (const dabgpu_datagroup &g : groups)
                        dg_cb_(s, 4 * frames_done_[s] + g.cif, slot[j], g, bytes.data() + g.offset, std::min(g.nbytes, pk_cap_));
                }
            }
        }
    }
    if (NS && nmot_) {
        chk(dabgpu_pipe_mot(pipe_, (uint8_t *)mob_.get(), (dabgpu_mot_object *)moo_.get(), (dabgpu_mot_run *)mor_.get()),
            "dabgpu_pipe_mot");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        if (mot_cb_) {
            // as for the groups: the run records, then per (stream, slot) what the run completed
            std::vector<dabgpu_mot_run> run((size_t)S * nmot_);
            mor_.download(run.data(), run.size() * sizeof(dabgpu_mot_run));
            std::vector<dabgpu_mot_object> objects;
            std::vector<uint8_t> bytes;
            for (int s = 0; s < S; s++) {
                std::vector<int> slot;               // MOT slot j of a stream is its j-th entry flagged for both
                for (int k = 0; k < (int)tab_[s].size(); k++)
                    if ((tab_[s][k].flags & DABGPU_SUBCH_PACKET) && (tab_[s][k].flags & DABGPU_SUBCH_MOT)) slot.push_back(k);
                for (int j = 0; j < (int)slot.size() && j < nmot_; j++) {
                    const size_t e = (size_t)s * nmot_ + j;
                    if (run[e].n_objects <= 0) continue;
                    objects.resize(run[e].n_objects);
                    bytes.resize(std::max(1, run[e].n_bytes));
                    chk(dabgpu_memcpy_d2h(thread_context(), objects.data(), (const dabgpu_mot_object *)moo_.get() + e * pk_slots_,
                                          objects.size() * sizeof(dabgpu_mot_object)), "dabgpu_memcpy_d2h");
                    chk(dabgpu_memcpy_d2h(thread_context(), bytes.data(), (const uint8_t *)mob_.get() + e * mot_arena_, run[e].n_bytes),
                        "dabgpu_memcpy_d2h");
                    for (const dabgpu_mot_object &o : objects)
                        mot_cb_(s, 4 * frames_done_[s] + o.cif, slot[j], o, bytes.data() + o.offset);
                }
            }
        }
    }
    bool any_ip = false;
    for (int s = 0; s < S; s++)
        for (const dabgpu_subch &e : tab_[s]) any_ip |= (e.flags & DABGPU_SUBCH_PACKET) && (e.flags & DABGPU_SUBCH_IP);
    if (NS && npk_ && any_ip && (ip_cb_ || ipq_cb_)) {
        const size_t ne = (size_t)S * npk_;
        if (!ipr_.size()) {                          // on first use; npk_, pk_slots_ and pk_arena_ are the constructor's for good
            ip_arena_ = DABGPU_IP_ARENA_FOR(pk_slots_, pk_arena_);
            ipb_.resize(ne * ip_arena_);
            ipo_.resize(std::max<size_t>(1, ne * pk_slots_) * sizeof(dabgpu_ip_result));
            ipr_.resize(ne * sizeof(dabgpu_ip_run));
        }
        chk(dabgpu_pipe_ip(pipe_, (uint8_t *)ipb_.get(), (dabgpu_ip_result *)ipo_.get(), (dabgpu_ip_run *)ipr_.get()), "dabgpu_pipe_ip");
        chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
        // as for the groups: the run records, then per flagged (stream, slot) what the run delivered
        std::vector<dabgpu_packet_run> prun(ne);
        std::vector<dabgpu_ip_run> run(ne);
        pkr_.download(prun.data(), prun.size() * sizeof(dabgpu_packet_run));
        ipr_.download(run.data(), run.size() * sizeof(dabgpu_ip_run));
        std::vector<dabgpu_ip_result> results;
        std::vector<dabgpu_datagroup> groups;
        std::vector<uint8_t> bytes;
        for (int s = 0; s < S; s++) {
            std::vector<int> slot;                   // packet slot j of a stream is its j-th flagged entry
            for (int k = 0; k < (int)tab_[s].size(); k++)
                if (tab_[s][k].flags & DABGPU_SUBCH_PACKET) slot.push_back(k);
            for (int j = 0; j < (int)slot.size() && j < npk_; j++) {
                const size_t e = (size_t)s * npk_ + j;
                const int ng = std::min<int>(prun[e].n_groups, (int)pk_slots_);
                if (!(tab_[s][slot[j]].flags & DABGPU_SUBCH_IP) || ng <= 0) continue;
                // nothing reached process_ipVector: neither a datagram nor a show_ipErrors value to deliver
                const int32_t *c = run[e].counts;
                if (c[DABGPU_IP_DELIVERED] + c[DABGPU_IP_CHECKSUM] + c[DABGPU_IP_NOT_UDP] + c[DABGPU_IP_MALFORMED] == 0) continue;
                results.resize(ng);
                groups.resize(ng);
                chk(dabgpu_memcpy_d2h(thread_context(), results.data(), (const dabgpu_ip_result *)ipo_.get() + e * pk_slots_,
                                      results.size() * sizeof(dabgpu_ip_result)), "dabgpu_memcpy_d2h");
                if (run[e].n_datagrams > 0)          // (the groups only for their CIFs)
                    chk(dabgpu_memcpy_d2h(thread_context(), groups.data(), (const dabgpu_datagroup *)pkg_.get() + e * pk_slots_,
                                          groups.size() * sizeof(dabgpu_datagroup)), "dabgpu_memcpy_d2h");
                size_t used = 0;
                for (const dabgpu_ip_result &r : results)
                    if (r.status == DABGPU_IP_DELIVERED) used = std::max(used, (size_t)r.offset + r.nbytes);
                bytes.resize(std::max<size_t>(1, used));
                if (used)
                    chk(dabgpu_memcpy_d2h(thread_context(), bytes.data(), (const uint8_t *)ipb_.get() + e * ip_arena_, used),
                        "dabgpu_memcpy_d2h");
                for (int g = 0; g < ng; g++) {
                    const dabgpu_ip_result &r = results[g];
                    if (r.quality >= 0 && ipq_cb_) ipq_cb_(s, slot[j], r.quality);
                    if (r.status == DABGPU_IP_DELIVERED && ip_cb_)
                        ip_cb_(s, slot[j], 4 * frames_done_[s] + groups[g].cif, bytes.data() + r.offset, r.nbytes);
                }
            }
        }
    }
    for (int s = 0; s < S; s++) {
        dabgpu_stream_state st;
        chk(dabgpu_pipe_state(pipe_, s, &st), "dabgpu_pipe_state");
        frames_done_[s] += st.frames_run;
    }
    // FIC first: a table parsed twice alike (two steps) and not yet applied is applied now
    for (int s = 0; s < S && cfg_.auto_layout; s++) {
        std::vector<dabgpu_subch> now;
        if (cfg_.fic_on_gpu) {     // the device's table of this step (dabgpu_pipe_fic)
            const dabgpu_fic_table &t = fic_tab_[s];
            now.assign(t.sub, t.sub + std::max(0, std::min(t.n, 64)));
        } else {
            for (const fib_subch &e : fibs_[s].subchannels(nullptr, (pcm_cb_ || (audio_cb_ && naudio_ > 0)) && nmp_ > 0,
                                                           dg_cb_ != nullptr && npk_ > 0,
                                                           mot_cb_ != nullptr && nmot_ > 0,
                                                           (label_cb_ || pad_dg_cb_ || pad_obj_cb_) && npad_ > 0,
                                                           ip_cb_ != nullptr && npk_ > 0))
                now.push_back({e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags});
        }
        // on_audio: the layer II entries also feed the audio output layer, as far as its slots go
        for (int k = 0, j = 0; k < (int)now.size() && audio_cb_ && j < naudio_; k++)
            if (now[k].flags & DABGPU_SUBCH_MP2) {
                now[k].flags |= DABGPU_SUBCH_AUDIO;
                j++;
            }
        auto same = [](const std::vector<dabgpu_subch> &x, const std::vector<dabgpu_subch> &y) {
            return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(dabgpu_subch)));
        };
        if (!now.empty() && same(now, parsed_[s]) && !same(now, tab_[s])) set_subch(s, now);
        parsed_[s] = now;
    }
    return ok;
}

// the two spellings of the database record are one layout (fib_processor.h stands without dabgpu.h)
static_assert(sizeof(fib_db) == sizeof(dabgpu_fic_db) && sizeof(fib_db::subch) == sizeof(dabgpu_fic_subch) &&
                  sizeof(fib_db::component) == sizeof(dabgpu_fic_component) && sizeof(fib_db::service) == sizeof(dabgpu_fic_service) &&
                  offsetof(fib_db, components) == offsetof(dabgpu_fic_db, components) &&
                  offsetof(fib_db, services) == offsetof(dabgpu_fic_db, services) && offsetof(fib_db, EId) == offsetof(dabgpu_fic_db, EId) &&
                  offsetof(fib_db, named) == offsetof(dabgpu_fic_db, named) && offsetof(fib_db, label) == offsetof(dabgpu_fic_db, label) &&
                  offsetof(fib_db, table) == offsetof(dabgpu_fic_db, table) &&
                  offsetof(fib_db::component, SCId) == offsetof(dabgpu_fic_component, SCId) &&
                  offsetof(fib_db::component, packetAddress) == offsetof(dabgpu_fic_component, packetAddress) &&
                  offsetof(fib_db::service, data_suffix) == offsetof(dabgpu_fic_service, data_suffix) &&
                  offsetof(fib_db::service, label) == offsetof(dabgpu_fic_service, label) &&
                  offsetof(fib_db::subch, inUse) == offsetof(dabgpu_fic_subch, inUse),
              "fib_db (fib_processor.h) is dabgpu_fic_db (dabgpu.h)");

fib_processor ensembleDecoder::database(int stream) const {
    if (!cfg_.auto_layout || stream < 0 || stream >= cfg_.n_streams)
        throw error(DABGPU_E_ARG, "ensembleDecoder::database: auto_layout and a stream of this decoder");
    if (!cfg_.fic_on_gpu) {
        fib_processor p = fibs_[stream];
        p.on_event(nullptr);                   // (the copy signals nobody)
        return p;
    }
    fib_db db;
    chk(dabgpu_pipe_fic_db(pipe_, stream, reinterpret_cast<dabgpu_fic_db *>(&db)), "dabgpu_pipe_fic_db");
    fib_processor p;
    p.import_db(db);
    return p;
}

dabgpu_stream_state ensembleDecoder::state(int stream) const {
    dabgpu_stream_state st;
    chk(dabgpu_pipe_state(pipe_, stream, &st), "dabgpu_pipe_state");
    return st;
}

}  // namespace dabgpu
