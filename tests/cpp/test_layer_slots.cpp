// The pipeline layers' slot logic (sdr-j-dab_amd/csrc/layer_slots.h: which table entry owns which
// slot, which slot's state goes on across a table change) against the loops it replaced: one per
// layer as rebuild_tables had them and one per layer as dabgpu_pipe_set_subch had them, restated
// here as they stood -- five times over and un-shared on purpose, so a slip in the shared form
// shows against five independent ones.  Host code only: the header needs no GPU.
//
// A slot's state is stood for by a number: old slot i holds state i, a fresh slot holds -1; what
// the old loops leave in the new slots is then the plan carry_plan must give.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "layer_slots.h"

typedef std::vector<dabgpu_subch> Tab;
typedef std::vector<int> Ints;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

static bool same(const dabgpu_subch &a, const dabgpu_subch &b) {
    return a.startAddr == b.startAddr && a.length == b.length && a.bitRate == b.bitRate && a.protLevel == b.protLevel &&
           a.uepFlag == b.uepFlag && a.flags == b.flags;
}

// ---- rebuild_tables, as it stood: one stream's row of each layer's tables ------------------------
struct Map { std::vector<int32_t> sub; std::vector<int16_t> br; std::vector<int64_t> since; };

static Map ref_map_dabplus(const Tab &tab, const std::vector<int64_t> &since, int NDP) {
    Map m{std::vector<int32_t>(NDP, -1), std::vector<int16_t>(NDP, 0), std::vector<int64_t>(NDP, 0)};
    int j = 0;
    for (int k = 0; k < (int)tab.size(); k++) {
        if (!(tab[k].flags & DABGPU_SUBCH_DABPLUS)) continue;
        const size_t i = j++;
        m.sub[i] = k;
        m.br[i] = tab[k].bitRate;
        m.since[i] = since[k];
    }
    return m;
}
static Map ref_map_mp2(const Tab &tab, const std::vector<int64_t> &since, int NMP) {
    Map m{std::vector<int32_t>(NMP, -1), std::vector<int16_t>(NMP, 0), std::vector<int64_t>(NMP, 0)};
    for (int k = 0, j = 0; k < (int)tab.size(); k++) {
        if (!(tab[k].flags & DABGPU_SUBCH_MP2)) continue;
        const size_t i = j++;
        m.sub[i] = k;
        m.br[i] = tab[k].bitRate;
        m.since[i] = since[k];
    }
    return m;
}
static Map ref_map_packet(const Tab &tab, const std::vector<int64_t> &since, int NPK) {
    Map m{std::vector<int32_t>(NPK, -1), std::vector<int16_t>(NPK, 0), std::vector<int64_t>(NPK, 0)};
    for (int k = 0, j = 0; k < (int)tab.size(); k++) {
        if (!(tab[k].flags & DABGPU_SUBCH_PACKET)) continue;
        const size_t i = j++;
        m.sub[i] = k;
        m.br[i] = tab[k].bitRate;
        m.since[i] = since[k];
    }
    return m;
}
static std::vector<int32_t> ref_src_mot(const Tab &tab, int s, int NPK, int NMOT) {
    std::vector<int32_t> src(NMOT, -1);
    for (int k = 0, j = 0, m = 0; k < (int)tab.size(); k++) {
        if (!(tab[k].flags & DABGPU_SUBCH_PACKET)) continue;
        if (tab[k].flags & DABGPU_SUBCH_MOT) src[m++] = s * NPK + j;
        j++;
    }
    return src;
}
static std::vector<int32_t> ref_src_pad(const Tab &tab, int s, int NDP, int NPAD) {
    std::vector<int32_t> src(NPAD, -1);
    for (int k = 0, j = 0, m = 0; k < (int)tab.size(); k++) {
        if (!(tab[k].flags & DABGPU_SUBCH_DABPLUS)) continue;
        if (tab[k].flags & DABGPU_SUBCH_PAD) src[m++] = s * NDP + j;
        j++;
    }
    return src;
}

// ---- dabgpu_pipe_set_subch, as it stood: the new slots' states from the old ones' ------------------
// (the DAB+ block ran inside the loop that also set the entries' since)
static Ints ref_carry_dabplus(const Tab &old, const std::vector<int64_t> &old_since, const Tab &sub, int NDP, int64_t cif_count,
                              std::vector<int64_t> &since) {
    const int n = (int)sub.size();
    std::vector<int> old_slot(old.size(), -1);
    for (int k = 0, j = 0; k < (int)old.size(); k++)
        if (old[k].flags & DABGPU_SUBCH_DABPLUS) old_slot[k] = j++;
    Ints sts(NDP), nsts(NDP, -1);
    for (int i = 0; i < NDP; i++) sts[i] = i;
    since.assign(n, cif_count);
    for (int k = 0, j = 0; k < n; k++) {
        const bool kept = k < (int)old.size() && same(old[k], sub[k]);
        if (kept) since[k] = old_since[k];
        if (!(sub[k].flags & DABGPU_SUBCH_DABPLUS)) continue;
        if (kept) nsts[j] = sts[old_slot[k]];
        j++;
    }
    return nsts;
}
static Ints ref_carry_mp2(const Tab &old, const Tab &sub, int NM) {
    const int n = (int)sub.size();
    Ints sy(NM), nsy(NM, -1);
    for (int i = 0; i < NM; i++) sy[i] = i;
    std::vector<int> oslot(old.size(), -1);
    for (int k = 0, j = 0; k < (int)old.size(); k++)
        if (old[k].flags & DABGPU_SUBCH_MP2) oslot[k] = j++;
    for (int k = 0, j = 0; k < n; k++) {
        if (!(sub[k].flags & DABGPU_SUBCH_MP2)) continue;
        if (k < (int)old.size() && same(old[k], sub[k])) nsy[j] = sy[oslot[k]];
        j++;
    }
    return nsy;
}
static Ints ref_carry_packet(const Tab &old, const Tab &sub, int NK) {
    const int n = (int)sub.size();
    Ints ps(NK), nps(NK, -1);
    for (int i = 0; i < NK; i++) ps[i] = i;
    std::vector<int> oslot(old.size(), -1);
    for (int k = 0, j = 0; k < (int)old.size(); k++)
        if (old[k].flags & DABGPU_SUBCH_PACKET) oslot[k] = j++;
    for (int k = 0, j = 0; k < n; k++) {
        if (!(sub[k].flags & DABGPU_SUBCH_PACKET)) continue;
        if (k < (int)old.size() && same(old[k], sub[k])) nps[j] = ps[oslot[k]];
        j++;
    }
    return nps;
}
static Ints ref_carry_mot(const Tab &old, const Tab &sub, int NM) {
    const int n = (int)sub.size();
    Ints ms(NM), nms(NM, -1);
    for (int i = 0; i < NM; i++) ms[i] = i;
    std::vector<int> oslot(old.size(), -1);
    for (int k = 0, j = 0; k < (int)old.size(); k++)
        if (old[k].flags & DABGPU_SUBCH_MOT) oslot[k] = j++;
    for (int k = 0, j = 0; k < n; k++) {
        if (!(sub[k].flags & DABGPU_SUBCH_MOT)) continue;
        if (k < (int)old.size() && same(old[k], sub[k])) nms[j] = ms[oslot[k]];
        j++;
    }
    return nms;
}
static Ints ref_carry_pad(const Tab &old, const Tab &sub, int NM) {
    const int n = (int)sub.size();
    Ints ms(NM), nms(NM, -1);
    for (int i = 0; i < NM; i++) ms[i] = i;
    std::vector<int> oslot(old.size(), -1);
    for (int k = 0, j = 0; k < (int)old.size(); k++)
        if (old[k].flags & DABGPU_SUBCH_PAD) oslot[k] = j++;
    for (int k = 0, j = 0; k < n; k++) {
        if (!(sub[k].flags & DABGPU_SUBCH_PAD)) continue;
        if (k < (int)old.size() && same(old[k], sub[k])) nms[j] = ms[oslot[k]];
        j++;
    }
    return nms;
}

// ---- the comparison ----------------------------------------------------------------------------
static int count(const Tab &t, int flag) {
    int c = 0;
    for (const dabgpu_subch &e : t) c += (e.flags & flag) ? 1 : 0;
    return c;
}

// every function of the header on one (old table, new table) pair of a stream s, each layer holding
// `extra` slots more than the larger of the two tables flags for it
static void check_pair(const Tab &old, const std::vector<int64_t> &old_since, const Tab &sub, int64_t cif_count, int s, int extra) {
    int N[slots::NKIND];
    for (int kind = 0; kind < slots::NKIND; kind++) {
        const int flag = slots::kKinds[kind].flag;
        N[kind] = std::max(count(old, flag), count(sub, flag)) + extra;
        CHECK(slots::count_flag(sub.data(), (int)sub.size(), flag) == count(sub, flag));
        const Ints so = slots::slot_of_entry(sub.data(), (int)sub.size(), flag);
        CHECK(so.size() == sub.size());
        for (int k = 0, j = 0; k < (int)sub.size(); k++) CHECK(so[k] == ((sub[k].flags & flag) ? j++ : -1));
    }
    // the carry-over: the plan of each kind, and since (from the old DAB+ block)
    std::vector<int64_t> want_since;
    const Ints want[slots::NKIND] = {ref_carry_dabplus(old, old_since, sub, N[slots::DABPLUS], cif_count, want_since),
                                     ref_carry_mp2(old, sub, N[slots::MP2]), ref_carry_packet(old, sub, N[slots::PACKET]),
                                     ref_carry_mot(old, sub, N[slots::MOT]), ref_carry_pad(old, sub, N[slots::PAD])};
    for (int kind = 0; kind < slots::NKIND; kind++) {
        const Ints plan = slots::carry_plan(old.data(), (int)old.size(), sub.data(), (int)sub.size(), slots::kKinds[kind].flag, N[kind]);
        CHECK(plan.size() == want[kind].size());
        for (size_t j = 0; j < plan.size() && j < want[kind].size(); j++) CHECK(plan[j] == want[kind][j]);
    }
    const std::vector<int64_t> since =
        slots::carry_since(old.data(), old_since.data(), (int)old.size(), sub.data(), (int)sub.size(), cif_count);
    CHECK(since.size() == want_since.size());
    for (size_t k = 0; k < since.size() && k < want_since.size(); k++) CHECK(since[k] == want_since[k]);
    // the device tables of the new table
    const Map maps[3] = {ref_map_dabplus(sub, since, N[slots::DABPLUS]), ref_map_mp2(sub, since, N[slots::MP2]),
                         ref_map_packet(sub, since, N[slots::PACKET])};
    for (int kind = 0; kind < 3; kind++) {
        const int n = N[kind];
        std::vector<int32_t> e(n, 77);
        std::vector<int16_t> br(n, 77);
        std::vector<int64_t> sc(n, 77);
        slots::entry_of_slot(sub.data(), since.data(), (int)sub.size(), slots::kKinds[kind].flag, n, e.data(), br.data(), sc.data());
        for (int j = 0; j < n; j++) CHECK(e[j] == maps[kind].sub[j] && br[j] == maps[kind].br[j] && sc[j] == maps[kind].since[j]);
    }
    const std::vector<int32_t> srcs[2] = {ref_src_mot(sub, s, N[slots::PACKET], N[slots::MOT]),
                                          ref_src_pad(sub, s, N[slots::DABPLUS], N[slots::PAD])};
    for (int kind = slots::MOT; kind <= slots::PAD; kind++) {
        const int parent = slots::kKinds[kind].parent;
        std::vector<int32_t> src(N[kind], 77);
        slots::parent_slot_of_slot(sub.data(), (int)sub.size(), slots::kKinds[kind].flag, slots::kKinds[parent].flag, s, N[parent], N[kind],
                                   src.data());
        for (int m = 0; m < N[kind]; m++) CHECK(src[m] == srcs[kind - slots::MOT][m]);
    }
}
static void check_pair(const Tab &old, const Tab &sub) {
    std::vector<int64_t> since(old.size());
    for (size_t k = 0; k < old.size(); k++) since[k] = 100 + 3 * (int64_t)k;
    for (int extra = 0; extra < 3; extra++) check_pair(old, since, sub, 5000, extra, extra);
}

static dabgpu_subch entry(int k, int flags) { return dabgpu_subch{(int16_t)(12 * k), 12, 16, 2, 0, (int16_t)flags}; }
static Tab table(const Ints &flags) {
    Tab t;
    for (size_t k = 0; k < flags.size(); k++) t.push_back(entry((int)k, flags[k]));
    return t;
}

enum { DP = DABGPU_SUBCH_DABPLUS, M2 = DABGPU_SUBCH_MP2, PK = DABGPU_SUBCH_PACKET, MOT = DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT,
       PAD = DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD };

static Ints plan_of(const Tab &old, const Tab &sub, int kind, int nslot) {
    return slots::carry_plan(old.data(), (int)old.size(), sub.data(), (int)sub.size(), slots::kKinds[kind].flag, nslot);
}

static void fixed_cases() {
    CHECK(slots::kKinds[slots::MOT].parent == slots::PACKET && slots::kKinds[slots::PAD].parent == slots::DABPLUS);
    CHECK(slots::kKinds[slots::DABPLUS].parent < 0 && slots::kKinds[slots::MP2].parent < 0 && slots::kKinds[slots::PACKET].parent < 0);
    // 0, 1 and 64 entries; nothing, everything, only the first, only the last flagged
    const int each[] = {DP, M2, PK, MOT, PAD};
    for (int f : each) {
        Ints none(64, 0), all(64, f), first(64, 0), last(64, 0);
        first[0] = f;
        last[63] = f;
        const Tab tabs[] = {Tab(), table({0}), table({f}), table(none), table(all), table(first), table(last)};
        for (const Tab &a : tabs)
            for (const Tab &b : tabs) check_pair(a, b);
    }
    {   // more slots than flagged entries: the map ends in -1 / 0 / 0, the plan in -1
        const Tab t = table({0, PK, 0, PK});
        const int64_t since[4] = {1, 2, 3, 4};
        int32_t e[4];
        int16_t br[4];
        int64_t sc[4];
        slots::entry_of_slot(t.data(), since, 4, PK, 4, e, br, sc);
        CHECK(e[0] == 1 && e[1] == 3 && e[2] == -1 && e[3] == -1 && br[0] == 16 && br[2] == 0 && sc[1] == 4 && sc[3] == 0);
        CHECK(plan_of(t, t, slots::PACKET, 4) == (Ints{0, 1, -1, -1}));
    }
    {   // children with parents before and after them (stream 2; five packet, four DAB+ slots)
        const Tab t = table({PK, MOT, DP, PK, PAD, MOT, PAD, DP, PK});
        int32_t src[3];
        slots::parent_slot_of_slot(t.data(), (int)t.size(), DABGPU_SUBCH_MOT, DABGPU_SUBCH_PACKET, 2, 5, 3, src);
        CHECK(src[0] == 2 * 5 + 1 && src[1] == 2 * 5 + 3 && src[2] == -1);
        slots::parent_slot_of_slot(t.data(), (int)t.size(), DABGPU_SUBCH_PAD, DABGPU_SUBCH_DABPLUS, 2, 4, 3, src);
        CHECK(src[0] == 2 * 4 + 1 && src[1] == 2 * 4 + 2 && src[2] == -1);
        check_pair(t, t);
    }
    {   // a kept entry's slot moves down (an earlier entry lost the flag) and up (one gained it)
        const Tab a = table({PK, PK, PK, M2}), down = table({0, PK, PK, M2}), up = table({PK, PK, PK, M2});
        Tab gained = table({0, PK, PK, M2});
        CHECK(plan_of(a, down, slots::PACKET, 3) == (Ints{1, 2, -1}));
        CHECK(plan_of(gained, up, slots::PACKET, 3) == (Ints{-1, 0, 1}));
        CHECK(plan_of(a, down, slots::MP2, 1) == (Ints{0}));
        check_pair(a, down);
        check_pair(gained, up);
    }
    {   // a new table shorter and longer than the old one
        const Tab a = table({DP, PAD, PK, MOT, M2}), shorter = table({DP, PAD}), longer = table({DP, PAD, PK, MOT, M2, PK, PAD, M2});
        CHECK(plan_of(a, shorter, slots::PAD, 2) == (Ints{0, -1}));
        CHECK(plan_of(a, longer, slots::PACKET, 3) == (Ints{0, 1, -1}));
        const int64_t os[5] = {10, 11, 12, 13, 14};
        CHECK(slots::carry_since(a.data(), os, 5, longer.data(), 8, 99) == (std::vector<int64_t>{10, 11, 12, 13, 14, 99, 99, 99}));
        check_pair(a, shorter);
        check_pair(a, longer);
        check_pair(shorter, longer);
        check_pair(longer, shorter);
    }
    // one field changed, each of the six: the entry starts anew, its neighbours go on
    for (int field = 0; field < 6; field++) {
        const Tab a = table({PK, PK, PK});
        Tab b = a;
        dabgpu_subch &e = b[1];
        switch (field) {
        case 0: e.startAddr += 1; break;
        case 1: e.length += 1; break;
        case 2: e.bitRate += 8; break;
        case 3: e.protLevel += 1; break;
        case 4: e.uepFlag ^= 1; break;
        default: e.flags |= DABGPU_SUBCH_MOT; break;
        }
        CHECK(!slots::same_subch(a[1], b[1]) && slots::same_subch(a[0], b[0]));
        CHECK(plan_of(a, b, slots::PACKET, 3) == (Ints{0, -1, 2}));
        const int64_t os[3] = {1, 2, 3};
        CHECK(slots::carry_since(a.data(), os, 3, b.data(), 3, 50) == (std::vector<int64_t>{1, 50, 3}));
        check_pair(a, b);
    }
}

// ---- random pairs -------------------------------------------------------------------------------
static uint32_t seed = 20240611u;
static int rnd(int n) {                                  // 0 .. n-1
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (uint32_t)n);
}
static dabgpu_subch rnd_entry() {
    // mostly what check_table admits, now and then a child without its parent or two layers at once
    static const int kinds[] = {0, DP, DP, PAD, M2, PK, MOT, MOT, DABGPU_SUBCH_MOT, DABGPU_SUBCH_PAD, DP | M2};
    return dabgpu_subch{(int16_t)(6 * rnd(4)), (int16_t)(6 + 6 * rnd(2)), (int16_t)(8 + 8 * rnd(2)), (int16_t)rnd(2),
                        (int16_t)rnd(2), (int16_t)kinds[rnd(11)]};
}
static void random_pairs() {
    for (int it = 0; it < 2000; it++) {
        const int sizes[] = {0, 1, 2, 5, 17, 64};
        const int n_old = rnd(4) ? rnd(65) : sizes[rnd(6)];
        Tab old(n_old);
        std::vector<int64_t> since(n_old);
        for (int k = 0; k < n_old; k++) {
            old[k] = rnd_entry();
            since[k] = rnd(1000);
        }
        // the new table: the old one cut or extended, a few entries changed
        const int n_new = rnd(3) ? n_old : rnd(65);
        Tab sub(n_new);
        for (int k = 0; k < n_new; k++) sub[k] = (k < n_old && rnd(4)) ? old[k] : rnd_entry();
        check_pair(old, since, sub, 1000 + rnd(100000), rnd(4), rnd(3));
    }
}

int main() {
    fixed_cases();
    random_pairs();
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("LAYER SLOTS OK\n");
    return 0;
}
