// dabgpu_dropin.cpp -- see dabgpu_dropin.h.  Every class is a thin host shell over
// the C ABI: buffers are allocated once per object, each call is one upload, one
// (or a few) kernel launches and one download on the thread's HIP stream.  The streaming
// engine, ensembleDecoder, is in ensemble_decoder.cpp.
#include "dropin_chk.h"

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

}  // namespace dabgpu
