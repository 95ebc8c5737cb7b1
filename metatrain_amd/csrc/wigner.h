// Real Wigner-D matrices of a proper rotation by the Ivanic-Ruedenberg recursion (J. Phys. Chem. 100, 6342 (1996) with the
// additions and corrections of J. Phys. Chem. A 102, 9099 (1998)): D^l from D^(l-1) and D^1, every entry a polynomial of degree l
// in the entries of the 3x3 matrix -- no angles, no poles, and a slightly non-orthogonal matrix gives a slightly non-orthogonal D.
// Convention (utils/testing/output.py:940-944 of the reference): Y_l(Q u) = D^l(Q) Y_l(u) with the orthonormal real spherical
// harmonics in the order m = -l..l without the Condon-Shortley phase, Y_1 = sqrt(3/4pi) (y, z, x), so D^1 = P Q P^T with P the
// permutation (x,y,z) -> (y,z,x), and a block transforms as t'[m] = sum_m' D^l[m,m'] t[m'].
// Plain C++ with no device-only construct: hipcc compiles it for the device (wigner.hip), a host compiler for the host, which
// is where the recursion is tested without a GPU. fp64 throughout.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define PET_WIGNER_FN __host__ __device__ inline
#else
#define PET_WIGNER_FN inline
#endif

namespace pet {

// D^l of block l starts here in a system's table; a table up to l_max holds wigner_width(l_max) values
PET_WIGNER_FN int wigner_offset(int l) { return l * (4 * l * l - 1) / 3; }
PET_WIGNER_FN int wigner_width(int l_max) { return (l_max + 1) * (2 * l_max + 1) * (2 * l_max + 3) / 3; }

// The proper part of one matrix O [3,3] (the device passes its fp32 entries, which fp64 holds exactly): returns det = +-1, the
// sign of the fp64 determinant (NaN when that is NaN), writes D^1 = P (det O) P^T [3,3] and `poison`, which is 0 for finite
// entries and NaN when any entry is a NaN or an infinity. Adding the poison to every entry of a table carries a NaN into the
// entries whose polynomial does not contain the bad entry.
PET_WIGNER_FN double wigner_prepare(const double* q, double* D1, double* poison) {
    double sum = 0.0;
    for (int i = 0; i < 9; i++) sum += q[i];
    const double det = q[0] * (q[4] * q[8] - q[5] * q[7]) - q[1] * (q[3] * q[8] - q[5] * q[6]) + q[2] * (q[3] * q[7] - q[4] * q[6]);
    *poison = 0.0 * sum;
    const double sign = det != det ? det : (det < 0.0 ? -1.0 : 1.0);
    const int perm[3] = {1, 2, 0};  // (y, z, x)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) D1[3 * i + j] = sign * q[3 * perm[i] + perm[j]];
    return sign;
}

// the recursion's P_i(a, b): row i of D^1 (i = -1, 0, 1) against row a of M = D^(l-1), for column b of D^l
PET_WIGNER_FN double wigner_p(int i, int l, int a, int b, const double* D1, const double* M) {
    const int w = 2 * l - 1;  // M is [w, w], indices -(l-1)..(l-1)
    const double* r = D1 + 3 * (i + 1);
    const double* row = M + (a + l - 1) * w;
    if (b == l) return r[2] * row[w - 1] - r[0] * row[0];
    if (b == -l) return r[2] * row[0] + r[0] * row[w - 1];
    return r[1] * row[b + l - 1];
}

// D^l[m, n] for l >= 2 from D^1 [3,3] and prev = D^(l-1) [2l-1, 2l-1], both row-major with indices from -l' to l'
PET_WIGNER_FN double wigner_entry(int l, int m, int n, const double* D1, const double* prev) {
    const int am = m < 0 ? -m : m, an = n < 0 ? -n : n;
    const double denom = an < l ? (double)((l + n) * (l - n)) : (double)(2 * l * (2 * l - 1));
    const double d0 = m == 0 ? 1.0 : 0.0;
    const double u = sqrt((double)((l + m) * (l - m)) / denom);
    const double v = 0.5 * sqrt((1.0 + d0) * (double)((l + am - 1) * (l + am)) / denom) * (1.0 - 2.0 * d0);
    const double w = -0.5 * sqrt((double)((l - am - 1) * (l - am)) / denom) * (1.0 - d0);
    double out = 0.0;
    if (am < l) out += u * wigner_p(0, l, m, n, D1, prev);  // (u = 0 for |m| = l, whose row D^(l-1) does not have)
    {
        double V;
        if (m == 0)
            V = wigner_p(1, l, 1, n, D1, prev) + wigner_p(-1, l, -1, n, D1, prev);
        else if (m > 0)
            V = m == 1 ? sqrt(2.0) * wigner_p(1, l, 0, n, D1, prev)
                       : wigner_p(1, l, m - 1, n, D1, prev) - wigner_p(-1, l, -m + 1, n, D1, prev);
        else
            V = m == -1 ? sqrt(2.0) * wigner_p(-1, l, 0, n, D1, prev)
                        : wigner_p(1, l, m + 1, n, D1, prev) + wigner_p(-1, l, -m - 1, n, D1, prev);
        out += v * V;
    }
    if (m != 0 && am + 1 < l) {  // (w = 0 for m = 0 and for |m| >= l - 1, whose rows |m| + 1 D^(l-1) does not have)
        const double W = m > 0 ? wigner_p(1, l, m + 1, n, D1, prev) + wigner_p(-1, l, -m - 1, n, D1, prev)
                               : wigner_p(1, l, m - 1, n, D1, prev) - wigner_p(-1, l, -m + 1, n, D1, prev);
        out += w * W;
    }
    return out;
}

}  // namespace pet
