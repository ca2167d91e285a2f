// ensemble_decoder.cpp -- ensembleDecoder (dabgpu_dropin.h), the streaming engine over
// dabgpu_pipe_*: the constructor sizes each layer through its struct, step() runs them in the same
// order, one member function per layer.  The pure pieces (slot rule, bit unpacking, the .sdr
// header, the flags auto_layout asks for) are in ensemble_util.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "dropin_chk.h"
#include "ensemble_util.h"
#include "rate_converter.h"

namespace dabgpu {

template <class T>
void ensembleDecoder::devarr<T>::download(std::vector<T> &h, size_t first, size_t count) const {
    h.resize(std::max<size_t>(1, count));
    chk(dabgpu_memcpy_d2h(thread_context(), h.data(), get() + first, count * sizeof(T)), "dabgpu_memcpy_d2h");
}

void ensembleDecoder::start_auto_layout() {
    const int S = cfg_.n_streams;
    fic_.parser.resize(S);
    parsed_.resize(S);
    for (int s = 0; s < S; s++)
        fic_.parser[s].on_event([this, s](int kind, int32_t id, const uint8_t *raw, int charset) {
            const std::string text = fib_processor::label_text(raw, 16, charset);
            if (kind == DABGPU_FIC_NAME_ENSEMBLE && fic_.on_ensemble_name) fic_.on_ensemble_name(s, fic_.frame, (uint32_t)id, text);
            if (kind == DABGPU_FIC_ADD_SERVICE && fic_.on_service_name) fic_.on_service_name(s, fic_.frame, text);
        });
    if (!cfg_.fic_on_gpu) return;
    chk(dabgpu_pipe_fic_caps(pipe_, 1), "dabgpu_pipe_fic_caps");
    fic_.events.resize((size_t)S * DABGPU_FIC_EVENT_SLOTS);
    fic_.tables.resize(S);
    fic_.runs.resize(S);
    fic_.table.resize(S);
}

ensembleDecoder::ensembleDecoder(const config &cfg) : cfg_(cfg) {
    dabgpu_pipe_cfg pc;
    std::memset(&pc, 0, sizeof pc);
    pc.n_streams = cfg_.n_streams;
    pc.n_frames = cfg_.n_frames;
    pc.n_subch = (int32_t)cfg_.subch.size();
    pc.threshold = cfg_.threshold;
    pc.freq_sync_method = 1;
    pc.subch = cfg_.subch.data();
    // what the table needs ...
    dabgpu_pipe_caps caps = {(int32_t)cfg_.subch.size(), 0, count_flagged(cfg_.subch, DABGPU_SUBCH_DABPLUS),
                             count_flagged(cfg_.subch, DABGPU_SUBCH_MP2)};
    for (const dabgpu_subch &sc : cfg_.subch) caps.max_bitrate = std::max<int32_t>(caps.max_bitrate, sc.bitRate);
    if (cfg_.max_mp2) caps.max_mp2 = cfg_.max_mp2;                        // ... or what the caller allows
    if (cfg_.max_subch) caps.max_subch = cfg_.max_subch;
    if (cfg_.max_bitrate) caps.max_bitrate = cfg_.max_bitrate;
    if (cfg_.max_dabplus) caps.max_dabplus = cfg_.max_dabplus;
    chk(dabgpu_pipe_create_caps(thread_context(), &pc, &caps, &pipe_), "dabgpu_pipe_create_caps");
    const int br = caps.max_bitrate;
    const size_t S = cfg.n_streams, F = cfg.n_frames, SF = S * F;
    tab_.assign(cfg.n_streams, cfg.subch);
    if (cfg.auto_layout) start_auto_layout();
    fic_.fibs.resize(SF * 4 * 96);
    fic_.crc.resize(SF * 12);
    // the MSC and the FIBs leave the GPU packed (8 bits per byte, 1/8 of the bytes over
    // PCIe) and are unpacked here for the one-bit-per-byte consumers (dab-concurrent.cpp:191,
    // fibProcessor::process_FIB)
    chk(dabgpu_pipe_set_packed(pipe_, DABGPU_PACK_MSC | DABGPU_PACK_FIC), "dabgpu_pipe_set_packed");
    msc_.n = caps.max_subch;
    msc_.maxbits = std::max(768, 24 * br);
    msc_.stride = ((msc_.maxbits + 7) / 8 + 15) / 16 * 16;
    msc_.rows.resize(std::max<size_t>(1, SF * 4 * msc_.n * msc_.stride));
    dabplus_.n = caps.max_dabplus;
    dabplus_.stride = std::max(16, 110 * (br / 8));
    if (dabplus_.n) {
        // only the superframes a run completes cross PCIe (DABGPU_SF_SLOTS per subchannel)
        chk(dabgpu_pipe_set_dabplus_compact(pipe_, 1), "dabgpu_pipe_set_dabplus_compact");
        dabplus_.bytes.resize(SF * 4 * dabplus_.n * dabplus_.stride);
        dabplus_.info.resize(SF * 4 * dabplus_.n);
    }
    pad_.n = cfg.max_pad ? cfg.max_pad : count_flagged(cfg.subch, DABGPU_SUBCH_PAD);
    if (cfg.max_pad) chk(dabgpu_pipe_pad_caps(pipe_, pad_.n), "dabgpu_pipe_pad_caps");
    if (pad_.n) {
        pad_.groups.resize(S * pad_.n, DABGPU_PAD_LABEL_SLOTS(cfg.n_frames), DABGPU_PAD_ARENA_BYTES(F));
        pad_.labels.resize(S * pad_.n * pad_.groups.slots);
        pad_.runs.resize(S * pad_.n);
    }
    mp2_.n = caps.max_mp2;
    if (mp2_.n) {
        mp2_.pcm.resize(SF * 4 * mp2_.n * 2304);
        mp2_.info.resize(SF * 4 * mp2_.n);
    }
    audio_.n = cfg.max_audio ? cfg.max_audio : count_flagged(cfg.subch, DABGPU_SUBCH_AUDIO);
    if (cfg.max_audio) chk(dabgpu_pipe_audio_caps(pipe_, audio_.n), "dabgpu_pipe_audio_caps");
    packet_.n = cfg.max_packet ? cfg.max_packet : count_flagged(cfg.subch, DABGPU_SUBCH_PACKET);
    packet_.cap = cfg.max_group_bytes ? cfg.max_group_bytes : DABGPU_PKT_GROUP_BYTES;
    if (cfg.max_packet || cfg.max_group_bytes)
        chk(dabgpu_pipe_packet_caps(pipe_, packet_.n, cfg.max_group_bytes), "dabgpu_pipe_packet_caps");
    if (packet_.n) {
        packet_.groups.resize(S * packet_.n, DABGPU_PKT_GROUP_SLOTS(cfg.n_frames, br), DABGPU_PKT_ARENA_BYTES(F, br, packet_.cap));
        packet_.runs.resize(S * packet_.n);
        packet_.info.resize(SF * 4 * packet_.n);
    }
    mot_.n = cfg.max_mot ? cfg.max_mot : count_flagged(cfg.subch, DABGPU_SUBCH_MOT);
    if (cfg.max_mot || cfg.max_body_bytes) chk(dabgpu_pipe_mot_caps(pipe_, mot_.n, cfg.max_body_bytes), "dabgpu_pipe_mot_caps");
    if (mot_.n) {
        const size_t body = cfg.max_body_bytes ? cfg.max_body_bytes : DABGPU_MOT_BODY_BYTES;
        mot_.objects.resize(S * mot_.n, packet_.groups.slots, DABGPU_MOT_ARENA_BYTES(F, br, body));
        mot_.runs.resize(S * mot_.n);
    }
}

static bool same_table(const std::vector<dabgpu_subch> &x, const std::vector<dabgpu_subch> &y) {
    return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(dabgpu_subch)));
}

void ensembleDecoder::set_subch(int stream, const std::vector<dabgpu_subch> &subch) {
    chk(dabgpu_pipe_set_subch(pipe_, stream, subch.data(), (int32_t)subch.size()), "dabgpu_pipe_set_subch");
    auto pads = [](const std::vector<dabgpu_subch> &t) {
        std::vector<dabgpu_subch> v;
        for (int k : entries_flagged(t, DABGPU_SUBCH_PAD, (int)t.size())) v.push_back(t[k]);
        return v;
    };
    for (int s = 0; s < cfg_.n_streams; s++) {
        if (stream >= 0 && s != stream) continue;
        // the PAD slots' MOT states (on_pad_object): new ones unless the stream's PAD entries stay as they are
        if (pad_mot_.states.size() && !same_table(pads(tab_[s]), pads(subch))) {
            const size_t sb = dabgpu_mot_state_bytes(0);
            chk(dabgpu_memset_d(thread_context(), pad_mot_.states.get() + (size_t)s * pad_.n * sb, 0, (size_t)pad_.n * sb), "dabgpu_memset_d");
        }
        tab_[s] = subch;
    }
}

std::vector<dabgpu_subch> ensembleDecoder::get_subch(int stream, std::vector<int64_t> *since_cif) const {
    std::vector<dabgpu_subch> v(std::max(1, msc_.n));
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

// ---- the loaders -----------------------------------------------------------------------
void ensembleDecoder::begin_load(const char *who, size_t given, const std::vector<int64_t> &n, size_t bytes_per_pair) {
    if ((int)given != cfg_.n_streams || (int)n.size() != cfg_.n_streams) throw error(DABGPU_E_ARG, who);
    stride_ = 0;
    for (int64_t k : n) stride_ = std::max(stride_, k);
    iq_.resize(bytes_per_pair * (size_t)stride_ * cfg_.n_streams);
}

void ensembleDecoder::finish_load(const std::vector<int64_t> &n, int format) {
    navail_ = n;
    frames_done_.assign(cfg_.n_streams, 0);
    chk(dabgpu_pipe_set_iq_format(pipe_, format), "dabgpu_pipe_set_iq_format");
}

void ensembleDecoder::load(const std::vector<const DSPCOMPLEX *> &samples, const std::vector<int64_t> &n) {
    begin_load("ensembleDecoder::load: one sample array per stream", samples.size(), n, sizeof(float) * 2);
    for (int s = 0; s < cfg_.n_streams; s++)
        chk(dabgpu_memcpy_h2d(thread_context(), stream_iq(s, sizeof(float) * 2), samples[s], sizeof(float) * 2 * n[s]), "dabgpu_memcpy_h2d");
    finish_load(n, DABGPU_IQ_F32);
}

void ensembleDecoder::load_recorded(int format, const std::vector<const void *> &samples, const std::vector<int64_t> &n) {
    if (format != DABGPU_IQ_S16 && format != DABGPU_IQ_U8)
        throw error(DABGPU_E_ARG, "ensembleDecoder::load_recorded: format DABGPU_IQ_S16 or DABGPU_IQ_U8");
    const size_t bps = format == DABGPU_IQ_S16 ? 4 : 2;      // bytes per I/Q pair
    begin_load("ensembleDecoder::load_recorded: one sample array per stream", samples.size(), n, bps);
    for (int s = 0; s < cfg_.n_streams; s++)
        chk(dabgpu_memcpy_h2d(thread_context(), stream_iq(s, bps), samples[s], bps * n[s]), "dabgpu_memcpy_h2d");
    finish_load(n, format);
}

void ensembleDecoder::load_rate(int rate, int format, const std::vector<const void *> &samples, const std::vector<int64_t> &n) {
    const char *who = "ensembleDecoder::load_rate: one sample array per stream";
    if (!rate_valid(rate) || !rate_format_valid(format))
        throw error(DABGPU_E_ARG, "ensembleDecoder::load_rate: a rate of whole kHz in 2048000 .. 10000000 and a DABGPU_IQ_* format");
    if ((int)n.size() != cfg_.n_streams) throw error(DABGPU_E_ARG, who);
    const int64_t M = rate / 1000, bps = rate_format_bytes(format);
    std::vector<int64_t> n_out(n.size());
    int64_t most = 0;                                        // blocks of the longest stream
    for (size_t s = 0; s < n.size(); s++) {
        if (n[s] < 0) throw error(DABGPU_E_ARG, who);
        n_out[s] = 2048 * (n[s] < 1 ? 0 : (n[s] - 1) / M);
        most = std::max(most, n_out[s] / 2048);
    }
    begin_load(who, samples.size(), n_out, sizeof(float) * 2);
    // K blocks of every stream at a time through a staging buffer of at most 256 MB: a piece holds M K + 1
    // samples, the last of them the first of the next piece (dabgpu_rate_convert's n_used)
    const int64_t K = std::max<int64_t>(1, std::min(most, ((int64_t)1 << 28) / (bps * M * cfg_.n_streams)));
    const int64_t piece = M * K + 1;
    devbuf stage((size_t)(bps * piece * cfg_.n_streams));
    std::vector<int64_t> count(n.size()), made(n.size()), used(n.size());
    for (int64_t first = 0; first < most; first += K) {
        for (int s = 0; s < cfg_.n_streams; s++) {
            count[s] = std::max<int64_t>(0, std::min(piece, n[s] - M * first));
            if (count[s])
                chk(dabgpu_memcpy_h2d(thread_context(), static_cast<char *>(stage.get()) + bps * piece * s,
                                      static_cast<const char *>(samples[s]) + bps * M * first, (size_t)(bps * count[s])), "dabgpu_memcpy_h2d");
        }
        chk(dabgpu_rate_convert(thread_context(), rate, format, stage.get(), piece, cfg_.n_streams, count.data(),
                                reinterpret_cast<float *>(stream_iq(0, sizeof(float) * 2)) + 2 * 2048 * first, stride_, made.data(), used.data()),
            "dabgpu_rate_convert");
    }
    chk(dabgpu_sync(thread_context()), "dabgpu_sync");       // (the staging buffer goes)
    finish_load(n_out, DABGPU_IQ_F32);
}

void ensembleDecoder::load_files(const std::vector<std::string> &paths) {
    const char *who = "ensembleDecoder::load_files: one file per stream";
    if ((int)paths.size() != cfg_.n_streams) throw error(DABGPU_E_ARG, who);      // (before a file is opened)
    auto is_raw = [](const std::string &p) { return p.size() >= 4 && p.compare(p.size() - 4, 4, ".raw") == 0; };
    const bool raw = !paths.empty() && is_raw(paths[0]);
    for (const std::string &p : paths)
        if (is_raw(p) != raw) throw error(DABGPU_E_ARG, "ensembleDecoder::load_files: .raw and .sdr files mixed");
    const size_t bps = raw ? 2 : 4;
    struct closer { void operator()(std::FILE *f) const { if (f) std::fclose(f); } };
    std::vector<std::unique_ptr<std::FILE, closer>> files;
    std::vector<int64_t> first, n;                           // the payload's offset in the file, its pairs
    for (const std::string &p : paths) {
        std::unique_ptr<std::FILE, closer> f(std::fopen(p.c_str(), "rb"));
        if (!f) throw error(DABGPU_E_ARG, p + ": cannot open");
        std::pair<int64_t, int64_t> pl{0, INT64_MAX};
        if (!raw) pl = sdr_payload<error>(f.get(), p);
        std::fseek(f.get(), 0, SEEK_END);
        pl.second = std::min<int64_t>(pl.second, (int64_t)std::ftell(f.get()) - pl.first);   // a truncated recording
        first.push_back(pl.first);
        n.push_back(pl.second / (int64_t)bps);
        files.push_back(std::move(f));
    }
    begin_load(who, paths.size(), n, bps);
    std::vector<char> piece((size_t)1 << 24);
    for (int s = 0; s < cfg_.n_streams; s++) {
        std::FILE *f = files[s].get();
        std::fseek(f, (long)first[s], SEEK_SET);
        for (int64_t done = 0, total = n[s] * (int64_t)bps; done < total;) {
            const size_t want = (size_t)std::min<int64_t>((int64_t)piece.size(), total - done);
            if (std::fread(piece.data(), 1, want, f) != want) throw error(DABGPU_E_ARG, paths[s] + ": short read");
            chk(dabgpu_memcpy_h2d(thread_context(), stream_iq(s, bps) + done, piece.data(), want), "dabgpu_memcpy_h2d");
            done += (int64_t)want;
        }
    }
    finish_load(n, raw ? DABGPU_IQ_U8 : DABGPU_IQ_S16);
}

void ensembleDecoder::acquire() {
    // unsynchronised streams search from where they are (sample 0 for a new decoder,
    // the position after a sync loss otherwise: notSynced continues, ofdm-processor.cpp:274)
    std::vector<int64_t> start(cfg_.n_streams, 0);
    for (int s = 0; s < cfg_.n_streams; s++) start[s] = state(s).next_pos;
    const int rc = dabgpu_pipe_acquire(pipe_, iq_.get(), stride_, start.data(), navail_.data());
    if (rc != DABGPU_OK && rc != DABGPU_E_STATE) chk(rc, "dabgpu_pipe_acquire");
}

// ---- a step ------------------------------------------------------------------------------
int ensembleDecoder::wanted() const {
    return wanted_flags({mp2_.on_pcm != nullptr, audio_.on_audio != nullptr, packet_.on_datagroup != nullptr, mot_.on_object != nullptr,
                         ip_.on_datagram != nullptr, pad_.on_label || pad_.on_datagroup || pad_mot_.on_object, mp2_.n, audio_.n, packet_.n,
                         mot_.n, pad_.n});
}

bool ensembleDecoder::step() {
    const bool ok = run_pipeline();        // + the GPU's FIC pass where configured
    deliver_fic_names();
    deliver_fibs();
    deliver_msc();
    run_dabplus();
    run_pad();
    run_mp2();
    run_audio();
    run_packet();
    run_mot();
    run_ip();
    advance_frames();
    apply_tables();
    return ok;
}

bool ensembleDecoder::run_pipeline() {
    const int S = cfg_.n_streams, F = cfg_.n_frames;
    std::vector<uint8_t> valid((size_t)S * 4 * F);
    const int rc = dabgpu_pipe_run(pipe_, iq_.get(), stride_, navail_.data(), fic_.fibs.get(), fic_.crc.get(),
                                   msc_.n ? msc_.rows.get() : nullptr, msc_.stride, valid.data());
    if (rc != DABGPU_OK && rc != DABGPU_E_STATE) chk(rc, "dabgpu_pipe_run");
    if (gpu_fic())                 // behind the run's FIC decode, on its back-end stream
        chk(dabgpu_pipe_fic(pipe_, fic_.fibs.get(), fic_.crc.get(), wanted(), fic_.events.get(), fic_.tables.get(), fic_.runs.get()),
            "dabgpu_pipe_fic");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    // frames committed per stream (a stream that lost sync re-acquired inside the run;
    // one that ran out of samples committed fewer): FIC and MSC for those
    frame_info_.resize((size_t)S * F);
    chk(dabgpu_pipe_frame_info(pipe_, frame_info_.data()), "dabgpu_pipe_frame_info");
    return rc == DABGPU_OK;
}

// fic_on_gpu: the names, where the host's parse delivers them; the tables for the end of the step
void ensembleDecoder::deliver_fic_names() {
    if (!gpu_fic()) return;
    const int S = cfg_.n_streams;
    std::vector<dabgpu_fic_run> run;
    fic_.runs.download(run, 0, S);
    fic_.tables.download(fic_.table, 0, S);
    bool any = false;
    for (const dabgpu_fic_run &r : run) any |= r.n_events > 0;
    if (!any || !(fic_.on_ensemble_name || fic_.on_service_name)) return;
    std::vector<dabgpu_fic_event> ev;
    fic_.events.download(ev, 0, (size_t)S * DABGPU_FIC_EVENT_SLOTS);
    for (int s = 0; s < S; s++)
        for (int i = 0; i < std::min(run[s].n_events, DABGPU_FIC_EVENT_SLOTS); i++) {
            const dabgpu_fic_event &e = ev[(size_t)s * DABGPU_FIC_EVENT_SLOTS + i];
            const std::string text = fib_processor::label_text(e.label, 16, e.charset);
            const int64_t frame = frames_done_[s] + e.fib / 12;
            if (e.kind == DABGPU_FIC_NAME_ENSEMBLE && fic_.on_ensemble_name) fic_.on_ensemble_name(s, frame, (uint32_t)e.id, text);
            if (e.kind == DABGPU_FIC_ADD_SERVICE && fic_.on_service_name) fic_.on_service_name(s, frame, text);
        }
}

// the FIBs to on_fib and, without fic_on_gpu, to auto_layout's parsers (downloaded for these only)
void ensembleDecoder::deliver_fibs() {
    const bool parse = cfg_.auto_layout && !gpu_fic();
    if (!fic_.on_fib && !parse) return;
    const int S = cfg_.n_streams, F = cfg_.n_frames;
    std::vector<uint8_t> fic, crc;
    fic_.fibs.download(fic, 0, (size_t)S * F * 4 * 96);
    fic_.crc.download(crc, 0, (size_t)S * F * 12);
    uint8_t fib[256];
    for (int s = 0; s < S; s++)
        for (int f = 0; f < F; f++) {
            if (!frame_info_[(size_t)s * F + f].committed) continue;
            fic_.frame = frames_done_[s] + f;
            for (int b = 0; b < 4; b++)
                for (int k = 0; k < 3; k++) {
                    unpack_bits(fic.data() + (((size_t)s * F + f) * 4 + b) * 96 + 32 * k, 256, fib);
                    const bool good = crc[((size_t)s * F + f) * 12 + 3 * b + k] != 0;
                    if (parse && good) fic_.parser[s].process_FIB(fib, (uint16_t)b);
                    if (fic_.on_fib) fic_.on_fib(s, frames_done_[s] + f, b, fib, good);
                }
        }
}

void ensembleDecoder::deliver_msc() {
    if (!msc_.n || !msc_.on_msc) return;
    const int S = cfg_.n_streams, C = 4 * cfg_.n_frames, NS = msc_.n;
    std::vector<uint8_t> msc, bits(msc_.maxbits), ev((size_t)S * C * NS);
    msc_.rows.download(msc, 0, (size_t)S * C * NS * msc_.stride);
    // per entry: delivered and past the entry's own 16-CIF warm-up
    chk(dabgpu_pipe_msc_entry_valid(pipe_, ev.data()), "dabgpu_pipe_msc_entry_valid");
    for (int s = 0; s < S; s++)
        for (int c = 0; c < C; c++)
            for (int k = 0; k < (int)tab_[s].size(); k++) {
                const size_t row = ((size_t)s * C + c) * NS + k;
                if (!ev[row]) continue;
                const int nbits = 24 * tab_[s][k].bitRate;
                unpack_bits(msc.data() + row * msc_.stride, nbits, bits.data());
                msc_.on_msc(s, 4 * frames_done_[s] + c, k, bits.data(), nbits);
            }
}

void ensembleDecoder::run_dabplus() {
    if (!msc_.n || !dabplus_.n) return;
    chk(dabgpu_pipe_dabplus(pipe_, dabplus_.bytes.get(), dabplus_.stride, dabplus_.info.get()), "dabgpu_pipe_dabplus");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    if (!dabplus_.on_superframe) return;
    const int S = cfg_.n_streams, C = 4 * cfg_.n_frames, ND = dabplus_.n, slots = DABGPU_SF_SLOTS(cfg_.n_frames);
    std::vector<dabgpu_superframe> info;
    std::vector<uint8_t> bytes;
    dabplus_.info.download(info, 0, (size_t)S * C * ND);
    dabplus_.bytes.download(bytes, 0, (size_t)S * ND * slots * dabplus_.stride);
    for (int s = 0; s < S; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_DABPLUS, ND);
        for (int c = 0; c < C; c++)
            for (int d = 0; d < (int)entry.size(); d++) {
                const dabgpu_superframe &i = info[((size_t)s * C + c) * ND + d];
                if (i.status < 0) continue;
                const int slot = i.reserved;                 // compact output: the superframe's slot
                const bool has = i.status == 3 && slot < slots;
                dabplus_.on_superframe(s, 4 * frames_done_[s] + c, entry[d], i,
                                       bytes.data() + (((size_t)s * ND + d) * slots + (has ? slot : 0)) * dabplus_.stride,
                                       has ? 110 * (tab_[s][entry[d]].bitRate / 8) : 0);
            }
    }
}

void ensembleDecoder::run_pad() {
    if (!msc_.n || !dabplus_.n || !pad_.n) return;
    chk(dabgpu_pipe_pad(pipe_, dabplus_.bytes.get(), dabplus_.stride, dabplus_.info.get(), pad_.labels.get(), pad_.groups.records.get(),
                        pad_.groups.bytes.get(), pad_.runs.get()), "dabgpu_pipe_pad");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    if (!pad_.on_label && !pad_.on_datagroup && !pad_mot_.on_object) return;
    std::vector<dabgpu_pad_run> run;
    pad_.runs.download(run, 0, (size_t)cfg_.n_streams * pad_.n);
    std::vector<dabgpu_mot_run> mrun(run.size());
    if (pad_mot_.on_object) run_pad_mot(run, mrun);
    deliver_pad(run, mrun);
}

// padHandler::my_motHandler: one MOT state per stream and PAD slot, the layer's groups as they are
void ensembleDecoder::run_pad_mot(const std::vector<dabgpu_pad_run> &run, std::vector<dabgpu_mot_run> &mrun) {
    const size_t ne = run.size(), sb = dabgpu_mot_state_bytes(0), slots = pad_.groups.slots;
    if (!pad_mot_.states.size()) {
        pad_mot_.states.resize(ne * sb);
        chk(dabgpu_memset_d(thread_context(), pad_mot_.states.get(), 0, ne * sb), "dabgpu_memset_d");
        pad_mot_.group_runs.resize(ne);
        pad_mot_.objects.resize(ne, slots, DABGPU_MOT_ARENA_FOR(slots, DABGPU_MOT_BODY_BYTES));
        pad_mot_.runs.resize(ne);
    }
    std::vector<dabgpu_packet_run> pr(ne);
    for (size_t e = 0; e < ne; e++) pr[e] = {std::min(run[e].n_groups, (int)slots), run[e].n_bytes, 0, 0};
    pad_mot_.group_runs.upload(pr);
    chk(dabgpu_mot_groups(thread_context(), pad_mot_.states.get(), (int)ne, 0, pad_.groups.records.get(), (int)slots, pad_.groups.bytes.get(),
                          (int64_t)pad_.groups.arena, pad_mot_.group_runs.get(), pad_mot_.objects.records.get(), pad_mot_.objects.bytes.get(),
                          (int64_t)pad_mot_.objects.arena, pad_mot_.runs.get()), "dabgpu_mot_groups");
    chk(dabgpu_sync(thread_context()), "dabgpu_sync");
    pad_mot_.runs.download(mrun, 0, ne);
}

void ensembleDecoder::deliver_pad(const std::vector<dabgpu_pad_run> &run, const std::vector<dabgpu_mot_run> &mrun) {
    const int slots = (int)pad_.groups.slots;
    std::vector<dabgpu_pad_label> labels;
    std::vector<dabgpu_datagroup> groups;
    std::vector<dabgpu_mot_object> objects;
    std::vector<uint8_t> bytes;
    for (int s = 0; s < cfg_.n_streams; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD, pad_.n);
        const int64_t cif0 = 4 * frames_done_[s];
        for (int j = 0; j < (int)entry.size(); j++) {
            const size_t e = (size_t)s * pad_.n + j;
            const int nl = std::min(run[e].n_labels, slots), ng = std::min(run[e].n_groups, slots);
            if (pad_.on_label && nl > 0) {
                pad_.labels.download(labels, e * slots, nl);
                for (const dabgpu_pad_label &l : labels) pad_.on_label(s, cif0 + l.cif, entry[j], l);
            }
            if (pad_.on_datagroup && ng > 0) {
                pad_.groups.fetch(e, ng, run[e].n_bytes, groups, bytes);
                for (const dabgpu_datagroup &g : groups)
                    pad_.on_datagroup(s, cif0 + g.cif, entry[j], g, bytes.data() + g.offset, (g.flags & DABGPU_DG_TRUNCATED) ? 0 : g.nbytes);
            }
            if (pad_mot_.on_object && mrun[e].n_objects > 0) {
                pad_mot_.objects.fetch(e, mrun[e].n_objects, mrun[e].n_bytes, objects, bytes);
                for (const dabgpu_mot_object &o : objects) pad_mot_.on_object(s, cif0 + o.cif, entry[j], o, bytes.data() + o.offset);
            }
        }
    }
}

void ensembleDecoder::run_mp2() {
    if (!msc_.n || !mp2_.n) return;
    chk(dabgpu_pipe_mp2(pipe_, mp2_.pcm.get(), mp2_.info.get()), "dabgpu_pipe_mp2");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    if (!mp2_.on_pcm) return;
    const int S = cfg_.n_streams, C = 4 * cfg_.n_frames;
    std::vector<dabgpu_mp2_info> info;
    std::vector<int16_t> pcm;
    mp2_.info.download(info, 0, (size_t)S * C * mp2_.n);
    mp2_.pcm.download(pcm, 0, (size_t)S * C * mp2_.n * 2304);
    for (int s = 0; s < S; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_MP2, mp2_.n);
        for (int c = 0; c < C; c++)
            for (int j = 0; j < (int)entry.size(); j++) {
                const size_t r = ((size_t)s * C + c) * mp2_.n + j;
                if (info[r].status == 2) mp2_.on_pcm(s, 4 * frames_done_[s] + c, entry[j], pcm.data() + r * 2304, 1152, info[r].sample_rate);
            }
    }
}

// after the step's dabgpu_pipe_mp2 (an unset callback or no flagged entry: nothing is allocated or launched)
void ensembleDecoder::run_audio() {
    if (!msc_.n || !mp2_.n || !audio_.on_audio || !audio_.n) return;
    const int S = cfg_.n_streams, C = 4 * cfg_.n_frames, NA = audio_.n;
    bool flagged = false;
    for (int s = 0; s < S; s++) flagged |= count_flagged(tab_[s], DABGPU_SUBCH_AUDIO) > 0;
    if (!flagged) return;
    const size_t rows = (size_t)S * C * NA, per_stream = (size_t)C * NA * 2304 * 2;
    if (!audio_.samples.get()) {
        audio_.samples.resize(rows * 2304 * 2);
        audio_.pairs.resize(rows);
    }
    chk(dabgpu_pipe_audio(pipe_, mp2_.pcm.get(), mp2_.info.get(), audio_.samples.get(), audio_.pairs.get()), "dabgpu_pipe_audio");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    std::vector<int32_t> n_out;
    audio_.pairs.download(n_out, 0, rows);
    std::vector<float> samples;
    for (int s = 0; s < S; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_AUDIO, NA);
        bool any = false;
        for (size_t r = (size_t)s * C * NA; r < (size_t)(s + 1) * C * NA; r++) any |= n_out[r] > 0;
        if (!any || entry.empty()) continue;
        // one download per stream that delivered, its rows as they lie (the on_pcm path's bulk copy)
        audio_.samples.download(samples, s * per_stream, per_stream);
        for (int c = 0; c < C; c++)
            for (int j = 0; j < (int)entry.size(); j++) {
                const int32_t n = n_out[((size_t)s * C + c) * NA + j];
                if (n > 0 && n <= 2304) audio_.on_audio(s, 4 * frames_done_[s] + c, entry[j], samples.data() + ((size_t)c * NA + j) * 2304 * 2, n);
            }
    }
}

void ensembleDecoder::run_packet() {
    if (!msc_.n || !packet_.n) return;
    chk(dabgpu_pipe_packet(pipe_, packet_.groups.bytes.get(), packet_.groups.records.get(), packet_.runs.get(), packet_.info.get()),
        "dabgpu_pipe_packet");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    if (!packet_.on_datagroup && !packet_.on_quality) return;
    // only what the run completed crosses PCIe: the run records, then per (stream, slot) its
    // group records and its arena's used bytes
    const int S = cfg_.n_streams, C = 4 * cfg_.n_frames, NP = packet_.n;
    std::vector<dabgpu_packet_run> run;
    std::vector<dabgpu_packet_info> info;
    packet_.runs.download(run, 0, (size_t)S * NP);
    packet_.info.download(info, 0, (size_t)S * C * NP);
    std::vector<dabgpu_datagroup> groups;
    std::vector<uint8_t> bytes;
    for (int s = 0; s < S; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_PACKET, NP);
        for (int j = 0; j < (int)entry.size(); j++) {
            const size_t e = (size_t)s * NP + j;
            for (int c = 0; c < C && packet_.on_quality; c++) {
                const dabgpu_packet_info &i = info[((size_t)s * C + c) * NP + j];
                if (i.status == 0 && i.quality >= 0) packet_.on_quality(s, 4 * frames_done_[s] + c, entry[j], i.quality);
            }
            if (!packet_.on_datagroup || run[e].n_groups <= 0) continue;
            packet_.groups.fetch(e, run[e].n_groups, run[e].n_bytes, groups, bytes);
            for (const dabgpu_datagroup &g : groups)
                packet_.on_datagroup(s, 4 * frames_done_[s] + g.cif, entry[j], g, bytes.data() + g.offset, std::min(g.nbytes, packet_.cap));
        }
    }
}

void ensembleDecoder::run_mot() {
    if (!msc_.n || !mot_.n) return;
    chk(dabgpu_pipe_mot(pipe_, mot_.objects.bytes.get(), mot_.objects.records.get(), mot_.runs.get()), "dabgpu_pipe_mot");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    if (!mot_.on_object) return;
    // as for the groups: the run records, then per (stream, slot) what the run completed
    std::vector<dabgpu_mot_run> run;
    mot_.runs.download(run, 0, (size_t)cfg_.n_streams * mot_.n);
    std::vector<dabgpu_mot_object> objects;
    std::vector<uint8_t> bytes;
    for (int s = 0; s < cfg_.n_streams; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT, mot_.n);
        for (int j = 0; j < (int)entry.size(); j++) {
            const size_t e = (size_t)s * mot_.n + j;
            if (run[e].n_objects <= 0) continue;
            mot_.objects.fetch(e, run[e].n_objects, run[e].n_bytes, objects, bytes);
            for (const dabgpu_mot_object &o : objects) mot_.on_object(s, 4 * frames_done_[s] + o.cif, entry[j], o, bytes.data() + o.offset);
        }
    }
}

// after the step's dabgpu_pipe_packet (no IP entry or no callback: nothing is allocated or launched)
void ensembleDecoder::run_ip() {
    const int S = cfg_.n_streams, NP = packet_.n;
    bool any_ip = false;
    for (int s = 0; s < S; s++) any_ip |= count_flagged(tab_[s], DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP) > 0;
    if (!msc_.n || !NP || !any_ip || !(ip_.on_datagram || ip_.on_quality)) return;
    const size_t ne = (size_t)S * NP, slots = packet_.groups.slots;
    if (!ip_.runs.size()) {                          // on first use; the packet layer's sizes are the constructor's for good
        ip_.results.resize(ne, slots, DABGPU_IP_ARENA_FOR(slots, packet_.groups.arena));
        ip_.runs.resize(ne);
    }
    chk(dabgpu_pipe_ip(pipe_, ip_.results.bytes.get(), ip_.results.records.get(), ip_.runs.get()), "dabgpu_pipe_ip");
    chk(dabgpu_pipe_sync(pipe_), "dabgpu_pipe_sync");
    // as for the groups: the run records, then per flagged (stream, slot) what the run delivered
    std::vector<dabgpu_packet_run> prun;
    std::vector<dabgpu_ip_run> run;
    packet_.runs.download(prun, 0, ne);
    ip_.runs.download(run, 0, ne);
    std::vector<dabgpu_ip_result> results;
    std::vector<dabgpu_datagroup> groups;
    std::vector<uint8_t> bytes;
    for (int s = 0; s < S; s++) {
        const std::vector<int> entry = entries_flagged(tab_[s], DABGPU_SUBCH_PACKET, NP);
        for (int j = 0; j < (int)entry.size(); j++) {
            const size_t e = (size_t)s * NP + j;
            const int ng = std::min<int>(prun[e].n_groups, (int)slots);
            if (!(tab_[s][entry[j]].flags & DABGPU_SUBCH_IP) || ng <= 0) continue;
            // nothing reached process_ipVector: neither a datagram nor a show_ipErrors value to deliver
            const int32_t *c = run[e].counts;
            if (c[DABGPU_IP_DELIVERED] + c[DABGPU_IP_CHECKSUM] + c[DABGPU_IP_NOT_UDP] + c[DABGPU_IP_MALFORMED] == 0) continue;
            ip_.results.records.download(results, e * slots, ng);
            groups.resize(ng);
            if (run[e].n_datagrams > 0) packet_.groups.records.download(groups, e * slots, ng);   // (the groups only for their CIFs)
            size_t used = 0;
            for (const dabgpu_ip_result &r : results)
                if (r.status == DABGPU_IP_DELIVERED) used = std::max(used, (size_t)r.offset + r.nbytes);
            bytes.resize(std::max<size_t>(1, used));
            if (used) ip_.results.bytes.download(bytes, e * ip_.results.arena, used);
            for (int g = 0; g < ng; g++) {
                const dabgpu_ip_result &r = results[g];
                if (r.quality >= 0 && ip_.on_quality) ip_.on_quality(s, entry[j], r.quality);
                if (r.status == DABGPU_IP_DELIVERED && ip_.on_datagram)
                    ip_.on_datagram(s, entry[j], 4 * frames_done_[s] + groups[g].cif, bytes.data() + r.offset, r.nbytes);
            }
        }
    }
}

void ensembleDecoder::advance_frames() {
    for (int s = 0; s < cfg_.n_streams; s++) frames_done_[s] += state(s).frames_run;
}

// FIC first: a table parsed twice alike (two steps) and not yet applied is applied now
void ensembleDecoder::apply_tables() {
    const int want = wanted();
    for (int s = 0; s < cfg_.n_streams && cfg_.auto_layout; s++) {
        std::vector<dabgpu_subch> now;
        if (cfg_.fic_on_gpu) {     // the device's table of this step (dabgpu_pipe_fic)
            const dabgpu_fic_table &t = fic_.table[s];
            now.assign(t.sub, t.sub + std::max(0, std::min(t.n, 64)));
        } else {
            for (const fib_subch &e : fic_.parser[s].subchannels(nullptr, want & DABGPU_SUBCH_MP2, want & DABGPU_SUBCH_PACKET, want & DABGPU_SUBCH_MOT,
                                                                want & DABGPU_SUBCH_PAD, want & DABGPU_SUBCH_IP))
                now.push_back({e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags});
        }
        // on_audio: the layer II entries also feed the audio output layer, as far as its slots go
        if (audio_.on_audio)
            for (int k : entries_flagged(now, DABGPU_SUBCH_MP2, audio_.n)) now[k].flags |= DABGPU_SUBCH_AUDIO;
        if (!now.empty() && same_table(now, parsed_[s]) && !same_table(now, tab_[s])) set_subch(s, now);
        parsed_[s] = now;
    }
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
        fib_processor p = fic_.parser[stream];
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
