// dabgpu_layers.cpp -- the C ABI (include/dabgpu.h), the pipeline's layers: the subchannel tables
// and the per-slot state behind them (which entry owns which slot: layer_slots.h), and the layers'
// entry points (DAB+, layer II, packet mode, MOT, PAD over the MSC; the FIC's databases)
#include <cstring>
#include "dabgpu_pipe.h"

using namespace dab;
using slots::kKinds;

namespace {

// One per-slot state buffer of a layer: nslot slots per stream, `bytes` each; a slot that starts
// anew holds `fresh` (null: zeros)
struct SlotBuf {
    void *d;
    size_t bytes;
    const void *fresh;
};
const PkState kFreshPk{0, -1, 0, 0, 0, 0, 0, 0};     // a new mscDatagroup

void fill_fresh(const SlotBuf &b, std::vector<uint8_t> &img) {
    if (b.fresh)
        for (size_t i = 0; i < img.size(); i += b.bytes) memcpy(img.data() + i, b.fresh, b.bytes);
}

// stream s's slots of a buffer after a table change: new slot j takes old slot plan[j]'s state,
// or a fresh one (slots::carry_plan)
int carry_buf(const SlotBuf &b, int s, const std::vector<int> &plan) {
    const size_t row = plan.size() * b.bytes;
    uint8_t *d = (uint8_t *)b.d + (size_t)s * row;
    std::vector<uint8_t> o(row), n(row, 0);
    HIPCHK(hipMemcpy(o.data(), d, row, hipMemcpyDeviceToHost));
    fill_fresh(b, n);
    for (size_t j = 0; j < plan.size(); j++)
        if (plan[j] >= 0) memcpy(n.data() + j * b.bytes, o.data() + (size_t)plan[j] * b.bytes, b.bytes);
    HIPCHK(hipMemcpy(d, n.data(), row, hipMemcpyHostToDevice));
    return 0;
}

// a resized layer's buffer `to` (new_n slots per stream) from the old layer's `from` (old_n): the
// slots both sizes hold go on through copy(new slot, old slot), every other slot is fresh
template <class Copy>
int resize_buf(int S, const SlotBuf &from, int old_n, const SlotBuf &to, int new_n, Copy copy) {
    std::vector<uint8_t> o((size_t)S * old_n * from.bytes), n((size_t)S * new_n * to.bytes, 0);
    if (old_n) HIPCHK(hipMemcpy(o.data(), from.d, o.size(), hipMemcpyDeviceToHost));
    fill_fresh(to, n);
    for (int s = 0; s < S; s++)
        for (int j = 0; j < std::min(old_n, new_n); j++)
            copy(n.data() + ((size_t)s * new_n + j) * to.bytes, o.data() + ((size_t)s * old_n + j) * from.bytes);
    HIPCHK(hipMemcpy(to.d, n.data(), n.size(), hipMemcpyHostToDevice));
    return 0;
}
// ... their bytes cut or padded to the new size
int resize_buf(int S, const SlotBuf &from, int old_n, const SlotBuf &to, int new_n) {
    const size_t nb = std::min(from.bytes, to.bytes);
    return resize_buf(S, from, old_n, to, new_n, [nb](uint8_t *n, const uint8_t *o) { memcpy(n, o, nb); });
}

// the state buffers of a slot kind's layer that go on across a table change
std::vector<SlotBuf> state_bufs(dabgpu_pipe *p, int kind) {
    switch (kind) {
    case slots::DABPLUS: return {{p->dp.ring_d.ptr, 120 * DP_MAX_RS, nullptr}, {p->dp.state_d.ptr, sizeof(DpState), nullptr}};
    case slots::MP2:
        return {{p->mp2.sync_d.ptr, sizeof(Mp2SyncState), nullptr},
                {p->mp2.part_d.ptr, (size_t)p->mp2.fstride, nullptr},
                {p->mp2.vstate_d[p->mp2.cur].ptr, sizeof(int16_t) * MP2_STATE_I16, nullptr}};
    case slots::PACKET:
        return {{p->pk.state_d.ptr, sizeof(PkState), &kFreshPk},
                {p->pk.carry_d[p->pk.cur].ptr, (size_t)p->pk.cap, nullptr},
                {p->pk.ip_state_d.ptr, sizeof(dabgpu_ip_state), nullptr}};
    case slots::MOT: return {{p->mot.state_d.ptr, p->mot.state_bytes, nullptr}};
    case slots::AUDIO: return {{p->audio.state_d.ptr, sizeof(AudioState), nullptr}};
    default: return {{p->pad.state_d.ptr, sizeof(PadState), nullptr}};
    }
}

// no stream's table flags more than max entries of a kind (before its layer shrinks)
int tables_fit(const dabgpu_pipe *p, int kind, int max) {
    for (int s = 0; s < p->S; s++) {
        const int n = slots::count_flag(p->tab[s].data(), (int)p->tab[s].size(), kKinds[kind].flag);
        if (n > max) return fail(DABGPU_E_ARG, "stream %d's table has %d %s subchannels", s, n, kKinds[kind].name);
    }
    return 0;
}

// a layer's slot map from the tables
int put_slot_map(const dabgpu_pipe *p, int kind, const SlotMap &m) {
    const int nslot = p->nslot(kind);
    const size_t ne = (size_t)p->S * nslot;
    if (!ne) return 0;
    std::vector<int32_t> sub(ne);
    std::vector<int16_t> br(ne);
    std::vector<int64_t> since(ne);
    for (int s = 0; s < p->S; s++) {
        const size_t o = (size_t)s * nslot;
        slots::entry_of_slot(p->tab[s].data(), p->since[s].data(), (int)p->tab[s].size(), kKinds[kind].flag, nslot, &sub[o], &br[o],
                             &since[o]);
    }
    HIPCHK(hipMemcpy(m.sub_d, sub.data(), sizeof(int32_t) * ne, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.br_d, br.data(), sizeof(int16_t) * ne, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.since_d, since.data(), sizeof(int64_t) * ne, hipMemcpyHostToDevice));
    return 0;
}

// a child layer's src_d ([S][nslot]): the parent kind's slot each of its slots reads
int put_child_src(const dabgpu_pipe *p, int kind, int32_t *src_d) {
    const int nslot = p->nslot(kind), parent = kKinds[kind].parent;
    if (!nslot) return 0;
    std::vector<int32_t> src((size_t)p->S * nslot);
    for (int s = 0; s < p->S; s++)
        slots::parent_slot_of_slot(p->tab[s].data(), (int)p->tab[s].size(), kKinds[kind].flag, kKinds[parent].flag, s,
                                   p->nslot(parent), nslot, &src[(size_t)s * nslot]);
    HIPCHK(hipMemcpy(src_d, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice));
    return 0;
}

// A layer's call may run: the pipeline holds slots of its kind, and what it consumes -- the last
// run's MSC rows, or the outputs of the run's call of its parent's layer -- has not entered it yet
int layer_ready(const dabgpu_pipe *p, int kind) {
    if (p->nslot(kind) == 0) return fail(DABGPU_E_STATE, "no %s subchannel in this pipeline", kKinds[kind].name);
    if (kKinds[kind].parent < 0) {
        if (!p->feed.last_msc || !p->feed.pending[kind]) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with MSC output to consume");
    } else if (!p->feed.pending[kind]) {
        return fail(DABGPU_E_STATE, "no dabgpu_pipe_%s call of this run to consume",
                    kind == slots::MOT ? "packet" : kind == slots::AUDIO ? "mp2" : "dabplus");
    }
    return 0;
}

// the last run's MSC rows
MscFeed msc_feed(const dabgpu_pipe *p) {
    MscFeed f;
    f.msc = p->feed.last_msc;
    f.msc_stride = p->feed.last_msc_stride;
    f.ncif = 4 * p->F;
    f.nsub = p->NSUB;
    f.nstreams = p->S;
    f.packed = p->feed.last_msc_packed ? 1 : 0;
    f.cif0s = p->cif0_dev(p->cur);
    f.ncifs = p->ncif_dev(p->cur);
    return f;
}

// A layer's pass on the last run's back-end stream (behind its channel decoding and the layers
// called before), after the layer's previous pass: its state carries over from run to run.
// (The run after next does not wait for the pass: it reads this run's outputs and CIF counters,
// which that run's back end overwrites behind it on this stream.)  stage: its DABGPU_STAGE_*, if timed.
template <class Launch>
int layer_pass(dabgpu_pipe *p, Event &ev, Launch launch, int stage = -1) {
    hipStream_t bs = p->back[p->cur].stream;
    HIPCHK(ev.wait_on(bs));
    if (stage >= 0) HIPCHK(prof_mark(p, stage, true));
    HIPCHK(launch(bs));
    if (stage >= 0) HIPCHK(prof_mark(p, stage, false));
    HIPCHK(ev.record(bs));
    return 0;
}

}  // namespace

namespace dab {

// A subchannel table against the reference's definitions and the pipeline's caps
// (dabgpu_pipe_create_caps and dabgpu_pipe_set_subch validate alike)
int check_table(const dabgpu_subch *sub, int n, const TableLimits &lim) {
    if (n < 0 || (n > 0 && !sub)) return fail(DABGPU_E_ARG, "bad subchannel table");
    if (n > lim.max_subch) return fail(DABGPU_E_ARG, "%d subchannels, the pipeline holds %d per stream", n, lim.max_subch);
    for (int i = 0; i < n; i++) {
        Profile P;
        const int fl = sub[i].flags, br = sub[i].bitRate;
        if ((fl & DABGPU_SUBCH_PAD) && !(fl & DABGPU_SUBCH_DABPLUS))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged PAD and not DAB+", i);
        if ((fl & DABGPU_SUBCH_AUDIO) && !(fl & DABGPU_SUBCH_MP2))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged audio output and not layer II", i);
        if ((fl & DABGPU_SUBCH_MOT) && !(fl & DABGPU_SUBCH_PACKET))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged MOT and not packet mode", i);
        if ((fl & DABGPU_SUBCH_IP) && !(fl & DABGPU_SUBCH_PACKET))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged IP and not packet mode", i);
        if ((fl & DABGPU_SUBCH_IP) && (fl & DABGPU_SUBCH_MOT))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged both IP and MOT", i);
        if (make_profile(sub[i], P)) return fail(DABGPU_E_UNSUP, "subchannel %d protection undefined", i);
        if (sub[i].startAddr < 0 || sub[i].startAddr + sub[i].length > 864 || P.frag > sub[i].length * 64)
            return fail(DABGPU_E_ARG, "subchannel %d does not fit its CUs", i);
        // packets are multiples of 24 bytes: a CIF of 3 * bitRate bytes holds bitRate / 8 cells
        if ((fl & DABGPU_SUBCH_PACKET) && (br < 8 || br % 8 || br > lim.max_bitrate))
            return fail(DABGPU_E_UNSUP, "packet-mode subchannel %d: bitRate %d is not a multiple of 8 in [8, %d]", i, br,
                        lim.max_bitrate);
        if (br > lim.max_bitrate)
            return fail(DABGPU_E_ARG, "subchannel %d: bitRate %d above the pipeline's %d", i, br, lim.max_bitrate);
        if ((fl & DABGPU_SUBCH_MP2) && (fl & DABGPU_SUBCH_DABPLUS))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged both DAB+ and layer II", i);
        if ((fl & DABGPU_SUBCH_PACKET) && (fl & (DABGPU_SUBCH_MP2 | DABGPU_SUBCH_DABPLUS)))
            return fail(DABGPU_E_ARG, "subchannel %d is flagged packet mode and an audio layer", i);
        // DAB+ subchannels (mp4Processor: RSDims = bitRate / 8, mp4processor.cpp:83-84)
        if ((fl & DABGPU_SUBCH_DABPLUS) && (br < 8 || br % 8 || br / 8 > DP_MAX_RS))
            return fail(DABGPU_E_UNSUP, "DAB+ subchannel %d: bitRate %d is not a multiple of 8 in [8, 384]", i, br);
    }
    for (int kind = 0; kind < slots::NSLOTKIND; kind++) {
        const int c = slots::count_flag(sub, n, kKinds[kind].flag);
        if (c > lim.max_slots[kind])
            return fail(DABGPU_E_ARG, "%d %s subchannels, the pipeline holds %d per stream", c, kKinds[kind].name,
                        lim.max_slots[kind]);
    }
    return 0;
}

// (Re)size the packet-mode layer to npk slots per stream and groups of cap bytes.  The
// assemblers of the slots both sizes hold go on (their carried bytes cut or padded to cap),
// every other slot is a new mscDatagroup.  The caller has waited for the streams.  The new
// layer is built beside the old one and takes its place only when everything succeeded: on
// an error the pipeline keeps the layer, and the assemblers, it had.
int packet_size(dabgpu_pipe *p, int npk, int cap) {
    const PacketLayer &old = p->pk;
    PacketLayer k;
    if (npk) {
        k.cap = cap;
        k.ncell = std::max(1, p->max_bitrate / 8);
        const size_t ne = (size_t)p->S * npk, cells = (size_t)4 * p->F * k.ncell;
        HIPCHK(k.ev.create(hipEventDisableTiming));
        HIPCHK(k.map.alloc(ne));
        HIPCHK(k.state_d.alloc(ne));
        HIPCHK(k.rec_d.alloc(ne * cells));
        HIPCHK(k.take_d.alloc(ne * cells));
        HIPCHK(k.segtab_d.alloc(ne * (1 + cells)));
        HIPCHK(k.ip_ev.create(hipEventDisableTiming));
        HIPCHK(k.ip_state_d.alloc(ne));
        HIPCHK(k.ip_on_d.alloc(ne));
        for (auto &c : k.carry_d) HIPCHK(c.alloc(ne * cap));
        if (int rc = resize_buf(p->S, {old.state_d.ptr, sizeof(PkState), nullptr}, p->NPK,
                                {k.state_d.ptr, sizeof(PkState), &kFreshPk}, npk))
            return rc;
        if (int rc = resize_buf(p->S, {old.carry_d[old.cur].ptr, (size_t)old.cap, nullptr}, p->NPK,
                                {k.carry_d[0].ptr, (size_t)cap, nullptr}, npk))
            return rc;
        if (int rc = resize_buf(p->S, {old.ip_state_d.ptr, sizeof(dabgpu_ip_state), nullptr}, p->NPK,
                                {k.ip_state_d.ptr, sizeof(dabgpu_ip_state), nullptr}, npk))
            return rc;
    }
    p->pk = std::move(k);
    p->NPK = npk;
    return 0;
}

// (Re)size the MOT layer to nmot slots per stream and bodies of at most body bytes, as
// packet_size does: the motHandlers of the slots both sizes hold go on (an entry whose body no
// longer fits is flagged DABGPU_MOT_TOO_LARGE), every other slot is a new one; the new layer
// takes the old one's place only when everything succeeded.
int mot_size(dabgpu_pipe *p, int nmot, int body) {
    const MotLayer &old = p->mot;
    MotLayer m;
    if (nmot) {
        m.body = body;
        m.body_cap = (body + 15) / 16 * 16;
        m.state_bytes = dabgpu_mot_state_bytes(body);
        m.gslots = DABGPU_PKT_GROUP_SLOTS(p->F, p->max_bitrate);
        const size_t ne = (size_t)p->S * nmot;
        HIPCHK(m.ev.create(hipEventDisableTiming));
        HIPCHK(m.state_d.alloc(ne * m.state_bytes));
        HIPCHK(m.src_d.alloc(ne));
        HIPCHK(m.ops_d.alloc(std::max<size_t>(1, ne * 2 * m.gslots)));
        HIPCHK(m.nops_d.alloc(ne));
        // the directory as it is, every body to its place under the new body_cap
        const auto relay = [&](uint8_t *n, const uint8_t *o) {
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
        };
        if (int rc = resize_buf(p->S, {old.state_d.ptr, old.state_bytes, nullptr}, p->NMOT,
                                {m.state_d.ptr, m.state_bytes, nullptr}, nmot, relay))
            return rc;
    }
    p->mot = std::move(m);
    p->NMOT = nmot;
    return 0;
}

// (Re)size the PAD layer to npad slots per stream, as mot_size does: the padHandlers of the
// slots both sizes hold go on, every other slot is a new one.
int pad_size(dabgpu_pipe *p, int npad) {
    PadLayer m;
    if (npad) {
        const size_t ne = (size_t)p->S * npad;
        HIPCHK(m.ev.create(hipEventDisableTiming));
        HIPCHK(m.state_d.alloc(ne * sizeof(PadState)));
        HIPCHK(m.src_d.alloc(ne));
        if (int rc = resize_buf(p->S, {p->pad.state_d.ptr, sizeof(PadState), nullptr}, p->NPAD,
                                {m.state_d.ptr, sizeof(PadState), nullptr}, npad))
            return rc;
    }
    p->pad = std::move(m);
    p->NPAD = npad;
    return 0;
}

// (Re)size the audio output layer to naudio slots per stream, as pad_size does: the sinks of the
// slots both sizes hold go on, every other slot is a new one.
int audio_size(dabgpu_pipe *p, int naudio) {
    AudioLayer m;
    if (naudio) {
        const size_t ne = (size_t)p->S * naudio;
        HIPCHK(m.ev.create(hipEventDisableTiming));
        HIPCHK(m.state_d.alloc(ne));
        HIPCHK(m.src_d.alloc(ne));
        if (int rc = resize_buf(p->S, {p->audio.state_d.ptr, sizeof(AudioState), nullptr}, p->NAUDIO,
                                {m.state_d.ptr, sizeof(AudioState), nullptr}, naudio))
            return rc;
    }
    p->audio = std::move(m);
    p->NAUDIO = naudio;
    return 0;
}

// The device's descriptor tables from p->tab / p->since.  The caller has waited for the
// pipeline's streams (in-flight kernels read the old tables): the tables are replaced.
int rebuild_tables(dabgpu_pipe *p) {
    const int S = p->S, NS = p->NSUB;
    p->uniform = true;
    for (int s = 0; s < S && p->uniform; s++) {
        if ((int)p->tab[s].size() != NS) p->uniform = false;
        for (int k = 0; k < (int)p->tab[s].size() && p->uniform; k++)
            if (p->since[s][k] != 0 || !slots::same_subch(p->tab[s][k], p->tab[0][k])) p->uniform = false;
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
    p->dp.max_rs = 0;
    for (const auto &tab : p->tab)
        for (const dabgpu_subch &e : tab)
            if (e.flags & DABGPU_SUBCH_DABPLUS) p->dp.max_rs = std::max(p->dp.max_rs, e.bitRate / 8);
    // slot j of a stream is its j-th entry flagged for the layer; slot m of a child layer reads
    // the parent layer's slot of its m-th entry
    const SlotMap *const maps[] = {&p->dp.map, &p->mp2.map, &p->pk.map};     // slots::DABPLUS, MP2, PACKET
    for (int kind = slots::DABPLUS; kind <= slots::PACKET; kind++)
        if (int rc = put_slot_map(p, kind, *maps[kind])) return rc;
    // which packet slots the IP layer walks
    p->pk.n_ip = 0;
    if (p->NPK) {
        std::vector<int32_t> on((size_t)S * p->NPK, 0);
        for (int s = 0; s < S; s++) {
            const std::vector<int> slot = slots::slot_of_entry(p->tab[s].data(), (int)p->tab[s].size(), DABGPU_SUBCH_PACKET);
            for (size_t k = 0; k < slot.size(); k++)
                if (slot[k] >= 0 && slot[k] < p->NPK && (p->tab[s][k].flags & DABGPU_SUBCH_IP)) {
                    on[(size_t)s * p->NPK + slot[k]] = 1;
                    p->pk.n_ip++;
                }
        }
        HIPCHK(hipMemcpy(p->pk.ip_on_d, on.data(), sizeof(int32_t) * on.size(), hipMemcpyHostToDevice));
    }
    int32_t *const srcs[] = {p->mot.src_d, p->pad.src_d, p->audio.src_d};    // slots::MOT, PAD, AUDIO
    for (int kind = slots::MOT; kind <= slots::AUDIO; kind++)
        if (int rc = put_child_src(p, kind, srcs[kind - slots::MOT])) return rc;
    return 0;
}

}  // namespace dab

extern "C" {

int dabgpu_pipe_set_subch(dabgpu_pipe *p, int stream, const dabgpu_subch *sub, int32_t n) {
    if (!p || stream < -1 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (int rc = check_table(sub, n, p->limits())) return rc;   // the table stays on error
    // in-flight kernels read the device tables: a rare control call, so it waits for
    // everything the pipeline has enqueued (as dabgpu_pipe_set_profiling) instead of
    // double-buffering them
    if (int rc = sync_streams(p)) return rc;
    for (auto [s, end] = stream_range(p, stream); s < end; s++) {
        // an entry whose index and fields are unchanged goes on (since_cif and its state in every
        // layer kept, wherever its slots now lie); every other one starts like a new dabConcurrent
        // and new handlers (mp4Processor, mp2Processor, mscDatagroup, motHandler, padHandler, audioSink) at
        // the stream's current CIF
        const std::vector<dabgpu_subch> &old = p->tab[s];
        for (int kind = 0; kind < slots::NSLOTKIND; kind++) {
            if (!p->nslot(kind)) continue;
            const std::vector<int> plan = slots::carry_plan(old.data(), (int)old.size(), sub, n, kKinds[kind].flag, p->nslot(kind));
            for (const SlotBuf &b : state_bufs(p, kind))
                if (int rc = carry_buf(b, s, plan)) return rc;
        }
        p->since[s] = slots::carry_since(old.data(), p->since[s].data(), (int)old.size(), sub, n, p->st[s].cif_count);
        p->tab[s].assign(sub, sub + n);
    }
    p->feed.tables_changed();
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

int dabgpu_pipe_dabplus(dabgpu_pipe *p, uint8_t *sf_bytes, int32_t sf_stride, dabgpu_superframe *info) {
    if (!p || !sf_bytes || !info) return fail(DABGPU_E_ARG, "null arg");
    if (int rc = layer_ready(p, slots::DABPLUS)) return rc;
    if (sf_stride < 110 * p->dp.max_rs) return fail(DABGPU_E_ARG, "sf_stride %d < %d", sf_stride, 110 * p->dp.max_rs);
    DpJob J = {};
    J.feed = msc_feed(p);
    J.map = p->dp.map.view();
    J.ndp = p->NDP;
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
    J.tabs = p->c->dptab;
    // (the 5-CIF rings carry state from run to run)
    if (int rc = layer_pass(p, p->dp.ev, [&](hipStream_t bs) { return launch_dabplus(bs, J); }, DABGPU_STAGE_DABPLUS)) return rc;
    LayerFeed &f = p->feed;
    f.pending[slots::DABPLUS] = false;         // each run's CIFs enter the superframe layer once
    f.dp_sf = sf_bytes;
    f.dp_info = info;
    f.dp_sf_stride = sf_stride;
    f.dp_sf_compact = p->dp.compact;
    f.pending[slots::PAD] = p->NPAD > 0;
    return 0;
}

int dabgpu_pipe_pad(dabgpu_pipe *p, const uint8_t *sf_bytes, int32_t sf_stride, const dabgpu_superframe *info,
                    dabgpu_pad_label *labels, dabgpu_datagroup *groups, uint8_t *bytes, dabgpu_pad_run *run) {
    if (!p || !sf_bytes || !info || !labels || !groups || !bytes || !run) return fail(DABGPU_E_ARG, "null arg");
    if (int rc = layer_ready(p, slots::PAD)) return rc;
    if (sf_bytes != p->feed.dp_sf || info != p->feed.dp_info || sf_stride != p->feed.dp_sf_stride)
        return fail(DABGPU_E_ARG, "sf_bytes_d, sf_stride and info_d are not those of this run's dabgpu_pipe_dabplus call");
    PadLayer &m = p->pad;
    PadJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S * p->NPAD;
    J.state = m.state_d;
    J.info = info;
    J.sf = sf_bytes;
    J.sf_stride = sf_stride;
    J.kmax = p->feed.dp_sf_compact ? DABGPU_SF_SLOTS(p->F) : 0;
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
    // behind the run's DAB+ layer (the padHandlers are updated in place)
    if (int rc = layer_pass(p, m.ev, [&](hipStream_t bs) { return launch_pad(bs, J); })) return rc;
    p->feed.pending[slots::PAD] = false;       // each run's AUs enter the layer once
    return 0;
}

int dabgpu_pipe_pad_caps(dabgpu_pipe *p, int max_pad) {
    if (!p || max_pad < 0 || max_pad > p->NDP) return fail(DABGPU_E_ARG, "bad args (max_pad <= max_dabplus)");
    if (max_pad && DABGPU_PAD_ARENA_BYTES((int64_t)p->F) > 0x7FFFFFFF) return fail(DABGPU_E_ARG, "an arena of 2 GiB and more");
    if (int rc = tables_fit(p, slots::PAD, max_pad)) return rc;
    if (int rc = sync_streams(p)) return rc;
    if (int rc = pad_size(p, max_pad)) return rc;
    p->feed.pending[slots::PAD] = false;
    return rebuild_tables(p);
}

int dabgpu_pipe_fic_caps(dabgpu_pipe *p, int on) {
    if (!p) return fail(DABGPU_E_ARG, "null pipe");
    if (int rc = sync_streams(p)) return rc;
    p->feed.fic_pending = false;
    if (!on) {
        p->fic = FicLayer();
        return 0;
    }
    if (p->fic.on) return 0;                   // the databases stay
    HIPCHK(p->fic.db_d.zalloc((size_t)p->S * sizeof(dabgpu_fic_db)));
    HIPCHK(p->fic.ev.create(hipEventDisableTiming));
    p->fic.on = true;
    return 0;
}

int dabgpu_pipe_fic(dabgpu_pipe *p, const uint8_t *fic_bits, const uint8_t *fic_crc, int want_flags, dabgpu_fic_event *events,
                    dabgpu_fic_table *table, dabgpu_fic_run *run) {
    if (!p || !fic_bits || !fic_crc || !events || !table || !run) return fail(DABGPU_E_ARG, "null arg");
    if (!p->fic.on) return fail(DABGPU_E_STATE, "no FIC layer in this pipeline (dabgpu_pipe_fic_caps)");
    if (!p->feed.fic_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_run with FIC output to consume");
    if (fic_bits != p->feed.last_fic || fic_crc != p->feed.last_crc)
        return fail(DABGPU_E_ARG, "fic_bits_d and fic_crc_d are not those of the last dabgpu_pipe_run");
    FibJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S;
    J.n_fibs = 12 * p->F;
    J.db = (dabgpu_fic_db *)(uint8_t *)p->fic.db_d;
    J.fibs = fic_bits;
    J.bit_src = p->feed.last_fic_packed ? 0 : 1;
    J.stride = (int64_t)J.n_fibs * (J.bit_src ? 256 : 32);
    J.ok = fic_crc;
    J.want = want_flags & (DABGPU_SUBCH_MP2 | DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT | DABGPU_SUBCH_PAD | DABGPU_SUBCH_IP);
    J.events = events;
    J.event_slots = DABGPU_FIC_EVENT_SLOTS;
    J.table = table;
    J.run = run;
    // behind the run's FIC decode (the databases are updated in place)
    if (int rc = layer_pass(p, p->fic.ev, [&](hipStream_t bs) { return launch_fib(bs, J); })) return rc;
    p->feed.fic_pending = false;               // each run's FIBs enter the layer once
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
    if (int rc = layer_ready(p, slots::MP2)) return rc;
    Mp2Layer &m = p->mp2;
    Mp2SyncJob Y = {};
    Y.feed = msc_feed(p);
    Y.map = m.map.view();
    Y.nmp = p->NMP;
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
    // (the synchronisers, the decoders and the frame slots carry over or are reused)
    if (int rc = layer_pass(p, m.ev, [&](hipStream_t bs) {
            const hipError_t e = launch_mp2_sync(bs, Y);
            return e != hipSuccess ? e : launch_mp2_decode(bs, J);
        }))
        return rc;
    m.cur ^= 1;
    LayerFeed &f = p->feed;
    f.pending[slots::MP2] = false;             // each run's CIFs enter the layer once
    f.mp2_pcm = pcm;
    f.mp2_info = info;
    f.pending[slots::AUDIO] = p->NAUDIO > 0;
    return 0;
}

int dabgpu_pipe_audio(dabgpu_pipe *p, const int16_t *pcm, const dabgpu_mp2_info *info, float *samples, int32_t *n_out) {
    if (!p || !pcm || !info || !samples || !n_out) return fail(DABGPU_E_ARG, "null arg");
    if (int rc = layer_ready(p, slots::AUDIO)) return rc;
    if (pcm != p->feed.mp2_pcm || info != p->feed.mp2_info)
        return fail(DABGPU_E_ARG, "pcm_d and info_d are not those of this run's dabgpu_pipe_mp2 call");
    if (((uintptr_t)pcm & 3) || ((uintptr_t)samples & 7))
        return fail(DABGPU_E_ARG, "pcm_d must be 4-byte aligned, samples_d 8-byte aligned");
    AudioLayer &m = p->audio;
    AudioJob J;
    memset(&J, 0, sizeof J);
    J.pcm = pcm;
    J.in_pairs = 1152;
    J.in_a = (int64_t)4 * p->F * p->NMP;
    J.in_c = p->NMP;
    J.n_chains = p->S * p->NAUDIO;
    J.chain_len = 4 * p->F;
    J.cdiv = p->NAUDIO;
    J.fixed_amount = 1152;
    J.src = m.src_d;
    J.info = info;
    J.state = m.state_d;
    J.samples = samples;
    J.n_out = n_out;
    J.out_pairs = 2304;
    J.out_a = (int64_t)4 * p->F * p->NAUDIO;
    J.out_c = p->NAUDIO;
    if (int rc = audio_tables(p->c, &J.coef)) return rc;
    // behind the run's layer II layer (the sinks are updated in place, by the pass's second launch)
    if (int rc = layer_pass(p, m.ev, [&](hipStream_t bs) { return launch_audio(bs, J); })) return rc;
    p->feed.pending[slots::AUDIO] = false;     // each run's frames enter the layer once
    return 0;
}

int dabgpu_pipe_audio_caps(dabgpu_pipe *p, int max_audio) {
    if (!p || max_audio < 0 || max_audio > p->NMP) return fail(DABGPU_E_ARG, "bad args (max_audio <= max_mp2)");
    if (int rc = tables_fit(p, slots::AUDIO, max_audio)) return rc;
    if (int rc = sync_streams(p)) return rc;
    if (int rc = audio_size(p, max_audio)) return rc;
    p->feed.pending[slots::AUDIO] = false;
    return rebuild_tables(p);
}

int dabgpu_pipe_packet(dabgpu_pipe *p, uint8_t *bytes, dabgpu_datagroup *groups, dabgpu_packet_run *run,
                       dabgpu_packet_info *info) {
    if (!p || !bytes || !groups || !run || !info) return fail(DABGPU_E_ARG, "null arg");
    if (int rc = layer_ready(p, slots::PACKET)) return rc;
    PacketLayer &k = p->pk;
    PkJob J = {};
    J.feed = msc_feed(p);
    J.map = k.map.view();
    J.npk = p->NPK;
    J.ncell = k.ncell;
    J.cap = k.cap;
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
    // (the assemblers and the work buffers carry over or are reused)
    if (int rc = layer_pass(p, k.ev, [&](hipStream_t bs) { return launch_packet(bs, J); })) return rc;
    k.cur ^= 1;
    LayerFeed &f = p->feed;
    f.pending[slots::PACKET] = false;          // each run's CIFs enter the layer once
    f.pk_bytes = bytes;
    f.pk_groups = groups;
    f.pk_run = run;
    f.pending[slots::MOT] = p->NMOT > 0;
    f.ip_pending = true;
    return 0;
}

int dabgpu_pipe_ip(dabgpu_pipe *p, uint8_t *bytes, dabgpu_ip_result *results, dabgpu_ip_run *run) {
    if (!p || !bytes || !results || !run) return fail(DABGPU_E_ARG, "null arg");
    if (p->NPK == 0) return fail(DABGPU_E_STATE, "no packet-mode subchannel in this pipeline");
    if (!p->feed.ip_pending) return fail(DABGPU_E_STATE, "no dabgpu_pipe_packet call of this run to consume");
    PacketLayer &k = p->pk;
    if (k.n_ip == 0) return fail(DABGPU_E_STATE, "no subchannel is flagged IP");
    IpJob J;
    memset(&J, 0, sizeof J);
    J.n_slots = p->S * p->NPK;
    J.state = k.ip_state_d;
    J.on = k.ip_on_d;
    J.groups = p->feed.pk_groups;
    J.gslots = DABGPU_PKT_GROUP_SLOTS(p->F, p->max_bitrate);
    J.bytes = p->feed.pk_bytes;
    J.arena = DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, k.cap);
    J.run = p->feed.pk_run;
    J.results = results;
    J.out = bytes;
    J.out_arena = DABGPU_IP_ARENA_FOR((int64_t)J.gslots, J.arena);
    J.ip_run = run;
    if (J.out_arena > 0x7FFFFFFF) return fail(DABGPU_E_ARG, "a packet arena of 2 GiB and more under the IP layer");
    // behind the run's packet layer (the counters are updated in place)
    if (int rc = layer_pass(p, k.ip_ev, [&](hipStream_t bs) { return launch_ip(bs, J); })) return rc;
    p->feed.ip_pending = false;                // each run's groups enter the layer once
    return 0;
}

int dabgpu_pipe_ip_state(dabgpu_pipe *p, int stream, dabgpu_ip_state *state_h) {
    if (!p || !state_h || stream < 0 || stream >= p->S) return fail(DABGPU_E_ARG, "bad args");
    if (p->NPK == 0) return fail(DABGPU_E_STATE, "no packet-mode subchannel in this pipeline");
    if (int rc = sync_streams(p)) return rc;
    HIPCHK(hipMemcpy(state_h, p->pk.ip_state_d + (size_t)stream * p->NPK, sizeof(dabgpu_ip_state) * p->NPK, hipMemcpyDeviceToHost));
    return 0;
}

int dabgpu_pipe_mot(dabgpu_pipe *p, uint8_t *bytes, dabgpu_mot_object *objects, dabgpu_mot_run *run) {
    if (!p || !bytes || !objects || !run) return fail(DABGPU_E_ARG, "null arg");
    if (int rc = layer_ready(p, slots::MOT)) return rc;
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
    J.groups = p->feed.pk_groups;
    J.gslots = m.gslots;
    J.bytes = p->feed.pk_bytes;
    J.arena = DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, p->pk.cap);
    J.run = p->feed.pk_run;
    J.objects = objects;
    J.out = bytes;
    J.out_arena = DABGPU_MOT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, m.body);
    J.mot_run = run;
    J.ops = m.ops_d;
    J.nops = m.nops_d;
    // behind the run's packet layer (the motHandlers are updated in place, the copy list is reused)
    if (int rc = layer_pass(p, m.ev, [&](hipStream_t bs) { return launch_mot(bs, J); })) return rc;
    p->feed.pending[slots::MOT] = false;       // each run's groups enter the layer once
    return 0;
}

int dabgpu_pipe_mot_caps(dabgpu_pipe *p, int max_mot, int max_body_bytes) {
    if (!p || max_mot < 0 || max_body_bytes < 0 || max_body_bytes > (1 << 24) || max_mot > p->NPK)
        return fail(DABGPU_E_ARG, "bad args (max_mot <= max_packet, max_body_bytes <= 1 << 24)");
    const int body = max_body_bytes ? max_body_bytes : DABGPU_MOT_BODY_BYTES;
    if (max_mot && (DABGPU_PKT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, p->pk.cap) > 0x7FFFFFFF ||
                    DABGPU_MOT_ARENA_BYTES((int64_t)p->F, p->max_bitrate, body) > 0x7FFFFFFF))
        return fail(DABGPU_E_ARG, "arenas of 2 GiB and more");
    if (int rc = tables_fit(p, slots::MOT, max_mot)) return rc;
    if (int rc = sync_streams(p)) return rc;
    if (int rc = mot_size(p, max_mot, body)) return rc;
    p->feed.pending[slots::MOT] = false;
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
    if (int rc = tables_fit(p, slots::PACKET, max_packet)) return rc;
    if (int rc = sync_streams(p)) return rc;
    if (int rc = packet_size(p, max_packet, cap)) return rc;
    p->feed.pending[slots::MOT] = false;
    p->feed.ip_pending = false;
    return rebuild_tables(p);
}

}  // extern "C"
