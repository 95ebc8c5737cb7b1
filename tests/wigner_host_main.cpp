// Stand-alone host program over csrc/wigner.h (tests/test_wigner_cpu.py builds and runs it): reads l_max and then 3x3 matrices
// (nine fp64 numbers each) from standard input and prints, per matrix, one line
//   parity table[0] table[1] ... table[W - 1]
// with the table built level by level as k_o3_wigner builds it, every entry plus the poison, but left in fp64 (the device rounds
// each to fp32 once): seventeen significant digits identify an fp64 value.
#include <cstdio>
#include <vector>

#include "wigner.h"

int main() {
    int l_max = 0;
    if (std::scanf("%d", &l_max) != 1 || l_max < 0 || l_max > 8) return 2;
    const int W = pet::wigner_width(l_max);
    std::vector<double> prev(17 * 17), cur(17 * 17);
    std::vector<double> table(W);
    for (;;) {
        double O[9];
        int got = 0;
        for (; got < 9; got++) {
            if (std::scanf("%lf", &O[got]) != 1) break;
        }
        if (got == 0) return 0;
        if (got != 9) return 2;
        double D1[9], poison;
        const double parity = pet::wigner_prepare(O, D1, &poison);
        table[0] = 1.0 + poison;
        if (l_max >= 1)
            for (int i = 0; i < 9; i++) table[1 + i] = (prev[i] = D1[i]) + poison;
        for (int l = 2; l <= l_max; l++) {
            const int w = 2 * l + 1;
            for (int m = -l; m <= l; m++)
                for (int n = -l; n <= l; n++) cur[(m + l) * w + n + l] = pet::wigner_entry(l, m, n, D1, prev.data());
            for (int i = 0; i < w * w; i++) table[pet::wigner_offset(l) + i] = cur[i] + poison;
            prev.swap(cur);
        }
        std::printf("%.17g", parity);
        for (int i = 0; i < W; i++) std::printf(" %.17g", table[i]);
        std::printf("\n");
    }
}
