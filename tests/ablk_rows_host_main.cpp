// Stand-alone host program over csrc/ablk_rows.h (tests/test_ablk_rows_cpu.py builds and runs it): prints the slot -> row map of
// every tile shape the fused attention kernels meet, one line per (tile, slot),
//   TA TB slot centre atom edge token_row
// for every paired or single 32-slot tile (1 <= TA, 0 <= TB, TA + TB <= 32; slots 0 .. 31) and every single atom of a 64-slot
// tile (33 <= TA <= 64; slots 0 .. 63). The descriptor fields are fixed functions of (TA, TB), chosen so that the two CSR ranges
// and the two centre rows cannot be confused; E is past 2^31 so that the 64-bit row type is exercised too.
#include <cstdint>
#include <cstdio>

#include "ablk_rows.h"

static void tile(int TA, int TB, int slots) {
    const int atomA = 1000 + 7 * TA + TB, atomB = 5000 + 11 * TB + TA;
    const int startA = 100000 + 64 * TA, startB = 300 + 3 * TB;  // (B's range in front of A's: the planner pairs any two atoms)
    const int64_t E = (int64_t(1) << 33) + 12345;
    const pet::AbTileRows t = pet::ab_tile_rows(atomA, startA, TA, atomB, startB, TB);
    for (int s = 0; s < slots; s++) {
        const pet::AbSlotRow r = pet::ab_slot_row(t, s);
        std::printf("%d %d %d %d %d %d %lld\n", TA, TB, s, r.centre, r.atom, r.edge, (long long)pet::ab_token_row<int64_t>(r, E));
    }
}

int main() {
    for (int TA = 1; TA <= 32; TA++)
        for (int TB = 0; TA + TB <= 32; TB++) tile(TA, TB, 32);
    for (int TA = 33; TA <= 64; TA++) tile(TA, 0, 64);
    return 0;
}
