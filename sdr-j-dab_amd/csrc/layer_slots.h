// layer_slots.h -- which table entry owns which slot of a pipeline layer, and which slot's state
// goes on across a table change.  Slot j of a stream is its j-th entry flagged for the layer; an
// entry whose index and fields are unchanged keeps its state wherever its slot now lies.  No HIP
// here: include/dabgpu.h and <vector> only (tests/cpp/test_layer_slots.cpp checks it on the CPU).
#pragma once
#include <vector>
#include "../../include/dabgpu.h"

namespace slots {

// The slot kinds.  parent >= 0: the kind's src_d row names slots of the parent kind (a MOT slot
// reads a packet slot, a PAD slot a DAB+ slot, an audio output slot a layer II slot).  name: as the
// error texts spell it.  NKIND counts the kinds up to PAD; NSLOTKIND counts them all.
enum { DABPLUS = 0, MP2, PACKET, MOT, PAD, NKIND };
enum { AUDIO = NKIND, NSLOTKIND };
struct Kind {
    int flag, parent;
    const char *name;
};
constexpr Kind kKinds[NSLOTKIND] = {{DABGPU_SUBCH_DABPLUS, -1, "DAB+"},
                                {DABGPU_SUBCH_MP2, -1, "layer II"},
                                {DABGPU_SUBCH_PACKET, -1, "packet-mode"},
                                {DABGPU_SUBCH_MOT, PACKET, "MOT"},
                                {DABGPU_SUBCH_PAD, DABPLUS, "PAD"},
                                {DABGPU_SUBCH_AUDIO, MP2, "audio output"}};

inline bool same_subch(const dabgpu_subch &a, const dabgpu_subch &b) {
    return a.startAddr == b.startAddr && a.length == b.length && a.bitRate == b.bitRate && a.protLevel == b.protLevel &&
           a.uepFlag == b.uepFlag && a.flags == b.flags;
}

inline int count_flag(const dabgpu_subch *tab, int n, int flag) {
    int c = 0;
    for (int k = 0; k < n; k++)
        if (tab[k].flags & flag) c++;
    return c;
}

// the slot of each entry, -1: not flagged
inline std::vector<int> slot_of_entry(const dabgpu_subch *tab, int n, int flag) {
    std::vector<int> slot(n, -1);
    for (int k = 0, j = 0; k < n; k++)
        if (tab[k].flags & flag) slot[k] = j++;
    return slot;
}

// One stream's row of a layer's slot map: the table entry of each of its nslot slots, the entry's
// bitRate and its since; -1 / 0 / 0 past the flagged entries.  (A table flags at most nslot
// entries -- check_table; more are left out.)
inline void entry_of_slot(const dabgpu_subch *tab, const int64_t *since, int n, int flag, int nslot, int32_t *sub,
                          int16_t *br, int64_t *since_out) {
    for (int j = 0; j < nslot; j++) {
        sub[j] = -1;
        br[j] = 0;
        since_out[j] = 0;
    }
    for (int k = 0, j = 0; k < n && j < nslot; k++) {
        if (!(tab[k].flags & flag)) continue;
        sub[j] = k;
        br[j] = (int16_t)tab[k].bitRate;
        since_out[j] = since[k];
        j++;
    }
}

// Stream s's src row of a child kind: slot m is the m-th entry flagged `flag` among the entries
// flagged `parent_flag`, and reads parent slot s * nparent + j, that entry being the stream's j-th
// parent entry; -1 past them
inline void parent_slot_of_slot(const dabgpu_subch *tab, int n, int flag, int parent_flag, int s, int nparent, int nslot,
                                int32_t *src) {
    for (int m = 0; m < nslot; m++) src[m] = -1;
    for (int k = 0, j = 0, m = 0; k < n && m < nslot; k++) {
        if (!(tab[k].flags & parent_flag)) continue;
        if (tab[k].flags & flag) src[m++] = s * nparent + j;
        j++;
    }
}

// entry k goes on across the change: its index and fields are unchanged
inline bool kept(const dabgpu_subch *old_tab, int old_n, const dabgpu_subch *new_tab, int k) {
    return k < old_n && same_subch(old_tab[k], new_tab[k]);
}

// For each of a layer's nslot slots under the new table: the old slot its state comes from, -1: a
// fresh state (the slot of a new or changed entry, or of none)
inline std::vector<int> carry_plan(const dabgpu_subch *old_tab, int old_n, const dabgpu_subch *new_tab, int new_n, int flag,
                                   int nslot) {
    const std::vector<int> old_slot = slot_of_entry(old_tab, old_n, flag);
    std::vector<int> plan(nslot, -1);
    for (int k = 0, j = 0; k < new_n && j < nslot; k++) {
        if (!(new_tab[k].flags & flag)) continue;
        if (kept(old_tab, old_n, new_tab, k) && old_slot[k] < nslot) plan[j] = old_slot[k];
        j++;
    }
    return plan;
}

// The since of each new entry: a kept one's stays, every other one starts at the stream's cif_count
inline std::vector<int64_t> carry_since(const dabgpu_subch *old_tab, const int64_t *old_since, int old_n,
                                        const dabgpu_subch *new_tab, int new_n, int64_t cif_count) {
    std::vector<int64_t> since(new_n, cif_count);
    for (int k = 0; k < new_n; k++)
        if (kept(old_tab, old_n, new_tab, k)) since[k] = old_since[k];
    return since;
}

}  // namespace slots
