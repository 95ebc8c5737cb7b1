// Rotational augmentation (utils/augmentation.py:O3Augmenter): a random element of O(3) per system of a collated batch, applied to
// positions, cells and the Cartesian targets on the device.
//   pet_o3_draw   one matrix per system from a counter-based generator: matrix = f(key, counter, system ordinal), nothing else
//   pet_o3_apply  up to PET_O3_MAX_ARRAYS arrays in ONE launch, out of place: VECTOR rows [3, P] -> R x, TENSOR2 rows [3, 3, P] ->
//                 R T R^T, each row with the matrix of its system
// Generator. Philox-4x32-10 (Salmon et al., SC'11), written out here: the 128-bit counter block is (counter low, counter high,
// system ordinal, 0), the 64-bit key is the caller's. One block gives the four 32-bit words a matrix needs: three uniforms
// u = (w + 1/2) / 2^32 for Shoemake's uniformly distributed unit quaternion (Graphics Gems III, 1992)
//   q = (sqrt(1-u1) sin 2 pi u2, sqrt(1-u1) cos 2 pi u2, sqrt(u1) sin 2 pi u3, sqrt(u1) cos 2 pi u3)
// and the top bit of the fourth word for the sign (an improper rotation with probability 1/2; the same bit under both groups).
// The quaternion, the nine products and the sign are fp64; the nine entries are rounded to fp32 once, so R^T R - I is at fp32
// rounding level. A thread reads nothing but its own index: no atomics, no state, no host read-back, the same bits whatever the
// grid, the batch size or what else was drawn.
// Apply. One thread per (row, property), consecutive lanes on consecutive properties and then consecutive rows; the row's matrix
// is read once into registers; fp32 fused multiply-adds. Every output component is a sum over ALL components of its input
// vector / tensor, with no product skipped: a NaN (or an infinity) anywhere in a vector or tensor makes that whole output
// vector or tensor NaN -- a partly known vector cannot be rotated -- and no other row. Zero rows (the cell of a non-periodic
// system) come out exactly zero, and under +-identity every output is exactly +-input (VECTOR) or the input (TENSOR2).
// A system index outside [0, n_systems) is not followed: the row comes out NaN.
#include <cmath>

#include "common.h"
#include "model.h"

namespace pet {

namespace {

constexpr int O3_BLOCK = 256;

struct O3Batch {
    pet_o3_array_t a[PET_O3_MAX_ARRAYS];
    int first_block[PET_O3_MAX_ARRAYS + 1];  // array k owns blocks [first_block[k], first_block[k + 1])
    int n;
};

__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

__device__ inline void philox4x32_10(uint32_t (&c)[4], uint64_t key) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(O3_BLOCK) void k_o3_draw(uint64_t key, uint64_t counter, int group, int S, float* __restrict__ out) {
    const int s = blockIdx.x * O3_BLOCK + threadIdx.x;
    if (s >= S) return;
    uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)s, 0u};
    philox4x32_10(c, key);
    const double sign = (c[3] >> 31) ? -1.0 : 1.0;
    double m[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (group == PET_O3_GROUP_O3) {
        const double inv = 1.0 / 4294967296.0;
        const double u1 = ((double)c[0] + 0.5) * inv, u2 = ((double)c[1] + 0.5) * inv, u3 = ((double)c[2] + 0.5) * inv;
        double s2, c2, s3, c3;
        sincospi(2.0 * u2, &s2, &c2);
        sincospi(2.0 * u3, &s3, &c3);
        const double a = sqrt(1.0 - u1), b = sqrt(u1);
        const double x = a * s2, y = a * c2, z = b * s3, w = b * c3;
        m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - z * w);       m[2] = 2.0 * (x * z + y * w);
        m[3] = 2.0 * (x * y + z * w);       m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - x * w);
        m[6] = 2.0 * (x * z - y * w);       m[7] = 2.0 * (y * z + x * w);       m[8] = 1.0 - 2.0 * (x * x + y * y);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) out[(int64_t)s * 9 + k] = (float)(sign * m[k]);
}

__global__ __launch_bounds__(O3_BLOCK) void k_o3_apply(const float* __restrict__ mats, int S, O3Batch b) {
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.first_block[k + 1]) k++;  // the same array for the whole workgroup
    const pet_o3_array_t d = b.a[k];
    const int64_t P = d.n_properties;
    const int64_t t = (int64_t)(blockIdx.x - b.first_block[k]) * O3_BLOCK + threadIdx.x;
    if (t >= d.rows * P) return;
    const int64_t row = t / P, p = t - row * P;
    const int64_t sys = d.system_of_row ? (int64_t)d.system_of_row[row] : row;
    float R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (sys >= 0 && sys < S) ? mats[sys * 9 + i] : NAN;
    if (d.kind == PET_O3_VECTOR) {
        const float* x = d.src + row * 3 * P + p;
        float* o = d.dst + row * 3 * P + p;
        const float x0 = x[0], x1 = x[P], x2 = x[2 * P];
#pragma unroll
        for (int a = 0; a < 3; a++) o[a * P] = R[3 * a] * x0 + R[3 * a + 1] * x1 + R[3 * a + 2] * x2;
    } else {
        const float* x = d.src + row * 9 * P + p;
        float* o = d.dst + row * 9 * P + p;
        float T[9], U[9];
#pragma unroll
        for (int i = 0; i < 9; i++) T[i] = x[i * P];
#pragma unroll
        for (int a = 0; a < 3; a++)  // U = R T
#pragma unroll
            for (int c = 0; c < 3; c++) U[3 * a + c] = R[3 * a] * T[c] + R[3 * a + 1] * T[3 + c] + R[3 * a + 2] * T[6 + c];
#pragma unroll
        for (int a = 0; a < 3; a++)  // out = U R^T
#pragma unroll
            for (int c = 0; c < 3; c++) o[(3 * a + c) * P] = U[3 * a] * R[3 * c] + U[3 * a + 1] * R[3 * c + 1] + U[3 * a + 2] * R[3 * c + 2];
    }
}

}  // namespace

}  // namespace pet

using namespace pet;

extern "C" {

int pet_o3_draw(uint64_t key, uint64_t counter, int32_t group, int64_t n_systems, float* d_matrices, void* stream) {
    PET_REQUIRE(group == PET_O3_GROUP_O3 || group == PET_O3_GROUP_INVERSIONS, PET_ERR_ARGUMENT,
                "unknown transformation group " + std::to_string(group));
    PET_REQUIRE(n_systems >= 0 && n_systems <= INT32_MAX - O3_BLOCK, PET_ERR_ARGUMENT, "n_systems outside [0, 2^31)");
    if (n_systems == 0) return PET_OK;
    PET_REQUIRE(d_matrices, PET_ERR_ARGUMENT, "null argument");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("o3_draw", st, 0.0, (double)n_systems * 36.0);
    k_o3_draw<<<cdiv(n_systems, O3_BLOCK), O3_BLOCK, 0, st>>>(key, counter, group, (int)n_systems, d_matrices);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_o3_apply(const float* d_matrices, int64_t n_systems, int32_t n_arrays, const pet_o3_array_t* h_arrays, void* stream) {
    PET_REQUIRE(n_arrays >= 0 && n_arrays <= PET_O3_MAX_ARRAYS, PET_ERR_ARGUMENT,
                "n_arrays outside [0, " + std::to_string(PET_O3_MAX_ARRAYS) + "]");
    PET_REQUIRE(n_systems >= 0 && n_systems <= INT32_MAX, PET_ERR_ARGUMENT, "n_systems outside [0, 2^31)");
    if (n_arrays == 0) return PET_OK;
    PET_REQUIRE(h_arrays, PET_ERR_ARGUMENT, "null argument");
    O3Batch b{};
    int64_t blocks = 0;
    double bytes = 0.0;
    for (int i = 0; i < n_arrays; i++) {
        const pet_o3_array_t& d = h_arrays[i];
        const std::string which = "array " + std::to_string(i) + ": ";
        PET_REQUIRE(d.kind == PET_O3_VECTOR || d.kind == PET_O3_TENSOR2, PET_ERR_ARGUMENT, which + "unknown kind " + std::to_string(d.kind));
        PET_REQUIRE(d.rows >= 0 && d.n_properties >= 0, PET_ERR_ARGUMENT, which + "negative row or property count");
        PET_REQUIRE(d.rows <= INT32_MAX, PET_ERR_ARGUMENT, which + "too many rows");
        PET_REQUIRE(d.system_of_row || d.rows <= n_systems, PET_ERR_ARGUMENT,
                    which + "more rows than systems and no system_of_row");
        const int64_t threads = d.rows * (int64_t)d.n_properties;
        if (threads == 0) continue;  // nothing to transform
        PET_REQUIRE(d.src && d.dst, PET_ERR_ARGUMENT, which + "null argument");
        PET_REQUIRE(d.src != d.dst, PET_ERR_ARGUMENT, which + "the transformation is out of place: dst must not be src");
        PET_REQUIRE(n_systems > 0 && d_matrices, PET_ERR_ARGUMENT, which + "rows but no matrices");
        b.a[b.n] = d;
        b.first_block[b.n] = (int)blocks;
        blocks += (threads + O3_BLOCK - 1) / O3_BLOCK;
        PET_REQUIRE(blocks <= INT32_MAX, PET_ERR_ARGUMENT, "too many rows in one call");
        bytes += (double)threads * (d.kind == PET_O3_VECTOR ? 24.0 : 72.0) + (double)d.rows * (d.system_of_row ? 4.0 : 0.0);
        b.n++;
    }
    if (b.n == 0) return PET_OK;
    b.first_block[b.n] = (int)blocks;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("o3_apply", st, 0.0, bytes);
    k_o3_apply<<<(unsigned)blocks, O3_BLOCK, 0, st>>>(d_matrices, (int)n_systems, b);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // extern "C"
