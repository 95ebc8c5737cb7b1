// Slot -> row map of a fused-attention tile (ablk.h AbAtom; Graph::tile_desc), free of HIP so that the host compiler can
// enumerate it (tests/ablk_rows_host_main.cpp). A tile's 32 NQ token slots hold atom A (slot 0 = its centre token, slots
// 1 .. TA - 1 its neighbours = CSR rows startA ..) and possibly a second atom B behind it (slot TA = its centre token, then
// CSR rows startB ..); slots past the last token repeat it. So the tile's rows are two contiguous CSR ranges,
//   slot s < TA:  startA - 1 + s        slot s >= TA:  startB - 1 - TA + s,
// and two centre rows (slots 0 and TA). Everything but the slot is wave-uniform: the kernels form AbTileRows once per tile
// and ab_slot_row is integer selects on it -- no branch, no early return, no choice between pointers (a per-lane choice
// of 64-bit addresses was compiled as nested divergent control flow, once per request: DESIGN 4.3).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AB_ROWS_FN __host__ __device__ __forceinline__
#else
#define AB_ROWS_FN inline
#endif

namespace pet {

struct AbTileRows {  // the wave-uniform part
    int TA, last;    // tokens of atom A; last token slot T - 1
    int atomA, atomB;
    int baseA, baseB;  // CSR row of slot s: base + s
};
AB_ROWS_FN AbTileRows ab_tile_rows(int atomA, int startA, int TA, int atomB, int startB, int TB) {
    AbTileRows t;
    t.TA = TA; t.last = TA + TB - 1;
    t.atomA = atomA; t.atomB = atomB;
    t.baseA = startA - 1; t.baseB = startB - 1 - TA;
    return t;
}

struct AbSlotRow {
    int centre;  // 1: the slot is a centre token (row `atom` of the per-atom arrays), 0: a neighbour (CSR row `edge`)
    int atom;    // the atom the slot belongs to
    int edge;    // CSR row of a neighbour slot (of a centre slot: the row in front of the atom's range, never to be touched)
};
AB_ROWS_FN AbSlotRow ab_slot_row(const AbTileRows& t, int s) {
    s = s < t.last ? s : t.last;
    const int b = s >= t.TA;
    AbSlotRow r;
    r.atom = b ? t.atomB : t.atomA;
    r.edge = (b ? t.baseB : t.baseA) + s;
    r.centre = (s == 0) | (s == t.TA);
    return r;
}
// row of the token stream [E edge rows | centre tokens]
template <class I>
AB_ROWS_FN I ab_token_row(const AbSlotRow& r, I E) {
    return r.centre ? E + (I)r.atom : (I)r.edge;
}

}  // namespace pet
