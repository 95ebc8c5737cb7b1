// Rotational augmentation of spherical targets (utils/augmentation.py:158-180, 97-124 for o3_lambda > 0): real Wigner-D matrices of
// every system's matrix, and their application to blocks [2l+1, P].
//   pet_o3_wigner           d_wigner [S, W(l_max)]: D^l(det O * O) for l = 0..l_max, row-major, one after the other; d_parity [S]: det
//   pet_o3_apply_spherical  up to PET_O3_MAX_ARRAYS arrays in ONE launch, out of place: rows [2l+1, P] -> f D^l x, each row with the
//                           block of its system; f = 1 for a proper system, o3_sigma (-1)^l for an improper one
// Wigner. One workgroup per system; the recursion of wigner.h level by level, level l - 1 and level l in two fp64 LDS images, one
// thread per entry (strided where a level has more entries than the workgroup threads). Every entry is a function of the system's
// nine numbers alone, computed in one fixed order: no atomics, no state, the same bits whatever the grid or the batch. fp64
// arithmetic; an entry is rounded to fp32 once, on its way to the table. The poison of wigner.h is added to every entry, so a NaN
// (or an infinity) in a matrix makes that system's whole table NaN; an exact +-identity gives exact identity blocks.
// Apply. One thread per (row, property), consecutive lanes on consecutive properties and then consecutive rows, as k_o3_apply.
// The per-atom arrays that dominate have hundreds of consecutive rows of one system, so each wave stages the block of its first
// lane's system in LDS (289 floats at l = 8) and the lanes of that system read it from there -- the same address in every lane:
// a broadcast, no bank conflict. A lane of another system (a system boundary inside the wave; per-system arrays, where every
// row has its own block) reads its block from global memory. Both paths run the same fused multiply-adds in the same order on
// the same numbers, so which path served a row does not show in its bits. A thread keeps its 2l+1 inputs in registers and one
// accumulator at a time: 17 + 1 values at l = 8, far below the 64 registers that still allow eight waves per SIMD. Every output
// is a sum over ALL m' with no product skipped: a NaN anywhere in a (row, property) multiplet makes that whole multiplet NaN and
// no other, a zero multiplet stays exactly zero, and under +-identity the output is exactly +-input. A system index outside
// [0, n_systems) is not followed: the row comes out NaN.
#include <cmath>

#include "common.h"
#include "model.h"
#include "wigner.h"

namespace pet {

namespace {

constexpr int WIGNER_BLOCK = 256;
constexpr int SPH_BLOCK = 256;
constexpr int SPH_WAVES = SPH_BLOCK / 64;
constexpr int MAX_W = 2 * PET_O3_MAX_L + 1;
constexpr int SPH_SLOT = (MAX_W * MAX_W + 3) / 4 * 4;  // floats per wave's block image, a multiple of 16 bytes

struct SphBatch {
    pet_o3_spherical_array_t a[PET_O3_MAX_ARRAYS];
    float improper_factor[PET_O3_MAX_ARRAYS];  // o3_sigma (-1)^l
    int first_block[PET_O3_MAX_ARRAYS + 1];    // array k owns blocks [first_block[k], first_block[k + 1])
    int n;
};

__global__ __launch_bounds__(WIGNER_BLOCK) void k_o3_wigner(const float* __restrict__ mats, int l_max, int W, float* __restrict__ table,
                                                            float* __restrict__ parity) {
    __shared__ double level[2][MAX_W * MAX_W];
    const int64_t s = blockIdx.x;
    double q[9], D1[9], poison;
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = (double)mats[s * 9 + i];
    const double det = wigner_prepare(q, D1, &poison);
    float* t = table + s * W;
    const int tid = threadIdx.x;
    if (tid == 0) {
        parity[s] = (float)det;
        t[0] = (float)(1.0 + poison);
    }
    if (l_max >= 1 && tid < 9) {
        double d = D1[0];
#pragma unroll
        for (int i = 1; i < 9; i++) d = tid == i ? D1[i] : d;  // (no runtime index into the register array)
        level[1][tid] = d;
        t[1 + tid] = (float)(d + poison);
    }
    __syncthreads();
    for (int l = 2; l <= l_max; l++) {
        const double* prev = level[(l - 1) & 1];
        double* cur = level[l & 1];  // (the image level l - 2 was read from; every such read is behind the barrier above)
        const int w = 2 * l + 1, off = wigner_offset(l);
        for (int e = tid; e < w * w; e += WIGNER_BLOCK) {
            const int m = e / w;
            const double v = wigner_entry(l, m - l, e - m * w - l, D1, prev);
            cur[e] = v;
            t[off + e] = (float)(v + poison);
        }
        __syncthreads();
    }
}

template <int L>
__device__ inline void sph_product(const float* D, const float (&x)[2 * L + 1], float* o, int64_t P, float f) {
    constexpr int w = 2 * L + 1;
#pragma unroll
    for (int m = 0; m < w; m++) {
        float acc = D[m * w] * x[0];
#pragma unroll
        for (int k = 1; k < w; k++) acc = fmaf(D[m * w + k], x[k], acc);
        o[m * P] = f * acc;
    }
}

// one (row, property) multiplet of a block of o3_lambda = L: D from the wave's LDS image, from global memory, or (nullptr) a system
// index that is not followed
template <int L>
__device__ inline void sph_multiplet(const float* lds_block, const float* global_block, bool from_lds, const float* x_in, float* o,
                                     int64_t P, float f) {
    constexpr int w = 2 * L + 1;
    float x[w];
#pragma unroll
    for (int k = 0; k < w; k++) x[k] = x_in[k * P];
    if (from_lds) {
        sph_product<L>(lds_block, x, o, P, f);
    } else if (global_block) {
        sph_product<L>(global_block, x, o, P, f);
    } else {
#pragma unroll
        for (int m = 0; m < w; m++) o[m * P] = NAN;
    }
}

__global__ __launch_bounds__(SPH_BLOCK) void k_o3_apply_spherical(const float* __restrict__ table, const float* __restrict__ parity, int W,
                                                                  int S, SphBatch b) {
    __shared__ __attribute__((aligned(16))) float image[SPH_WAVES][SPH_SLOT];
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.first_block[k + 1]) k++;  // the same array for the whole workgroup
    const pet_o3_spherical_array_t d = b.a[k];
    const int64_t P = d.n_properties;
    const int l = d.o3_lambda, w = 2 * l + 1, off = wigner_offset(l);
    const int64_t t = (int64_t)(blockIdx.x - b.first_block[k]) * SPH_BLOCK + threadIdx.x;
    const bool active = t < d.rows * P;  // (threads past the end stay until the barrier and follow no index)
    const int64_t row = active ? t / P : 0, p = active ? t - row * P : 0;
    int sys = -1;
    if (active) sys = d.system_of_row ? d.system_of_row[row] : (int)row;
    const bool followed = sys >= 0 && sys < S;
    // the wave's image: the block of its first lane's system (NaN where that index is not followed)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wave_sys = __builtin_amdgcn_readfirstlane(sys);
    const bool wave_followed = wave_sys >= 0 && wave_sys < S;
    const float* wave_block = table + (wave_followed ? (int64_t)wave_sys * W + off : 0);
    for (int e = lane; e < w * w; e += 64) image[wave][e] = wave_followed ? wave_block[e] : NAN;
    __syncthreads();
    if (!active) return;
    const float f = (followed && parity[sys] < 0.0f) ? b.improper_factor[k] : 1.0f;
    const float* global_block = followed ? table + (int64_t)sys * W + off : nullptr;
    const float* x = d.src + row * w * P + p;
    float* o = d.dst + row * w * P + p;
    const bool from_lds = sys == wave_sys;
    switch (l) {
        case 0: sph_multiplet<0>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 1: sph_multiplet<1>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 2: sph_multiplet<2>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 3: sph_multiplet<3>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 4: sph_multiplet<4>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 5: sph_multiplet<5>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 6: sph_multiplet<6>(image[wave], global_block, from_lds, x, o, P, f); break;
        case 7: sph_multiplet<7>(image[wave], global_block, from_lds, x, o, P, f); break;
        default: sph_multiplet<8>(image[wave], global_block, from_lds, x, o, P, f); break;
    }
}

}  // namespace

}  // namespace pet

using namespace pet;

extern "C" {

int pet_o3_wigner(const float* d_matrices, int64_t n_systems, int32_t l_max, float* d_wigner, float* d_parity, void* stream) {
    PET_REQUIRE(l_max >= 0 && l_max <= PET_O3_MAX_L, PET_ERR_ARGUMENT, "l_max outside [0, " + std::to_string(PET_O3_MAX_L) + "]");
    PET_REQUIRE(n_systems >= 0 && n_systems <= INT32_MAX, PET_ERR_ARGUMENT, "n_systems outside [0, 2^31)");
    if (n_systems == 0) return PET_OK;
    PET_REQUIRE(d_matrices && d_wigner && d_parity, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE((const void*)d_wigner != (const void*)d_matrices && (const void*)d_parity != (const void*)d_matrices && d_wigner != d_parity,
                PET_ERR_ARGUMENT, "the table, the parities and the matrices must be three buffers");
    const int W = wigner_width(l_max);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("o3_wigner", st, 0.0, (double)n_systems * (36.0 + 4.0 + 4.0 * W));
    k_o3_wigner<<<(unsigned)n_systems, WIGNER_BLOCK, 0, st>>>(d_matrices, l_max, W, d_wigner, d_parity);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_o3_apply_spherical(const float* d_wigner, const float* d_parity, int32_t l_max, int64_t n_systems, int32_t n_arrays,
                           const pet_o3_spherical_array_t* h_arrays, void* stream) {
    PET_REQUIRE(l_max >= 0 && l_max <= PET_O3_MAX_L, PET_ERR_ARGUMENT, "l_max outside [0, " + std::to_string(PET_O3_MAX_L) + "]");
    PET_REQUIRE(n_arrays >= 0 && n_arrays <= PET_O3_MAX_ARRAYS, PET_ERR_ARGUMENT,
                "n_arrays outside [0, " + std::to_string(PET_O3_MAX_ARRAYS) + "]");
    PET_REQUIRE(n_systems >= 0 && n_systems <= INT32_MAX, PET_ERR_ARGUMENT, "n_systems outside [0, 2^31)");
    if (n_arrays == 0) return PET_OK;
    PET_REQUIRE(h_arrays, PET_ERR_ARGUMENT, "null argument");
    SphBatch b{};
    int64_t blocks = 0;
    double bytes = 0.0;
    for (int i = 0; i < n_arrays; i++) {
        const pet_o3_spherical_array_t& d = h_arrays[i];
        const std::string which = "array " + std::to_string(i) + ": ";
        PET_REQUIRE(d.o3_lambda >= 0 && d.o3_lambda <= PET_O3_MAX_L, PET_ERR_ARGUMENT,
                    which + "o3_lambda outside [0, " + std::to_string(PET_O3_MAX_L) + "]");
        PET_REQUIRE(d.o3_lambda <= l_max, PET_ERR_ARGUMENT, which + "o3_lambda above the table's l_max");
        PET_REQUIRE(d.o3_sigma == 1 || d.o3_sigma == -1, PET_ERR_ARGUMENT, which + "o3_sigma must be +1 or -1");
        PET_REQUIRE(d.rows >= 0 && d.n_properties >= 0, PET_ERR_ARGUMENT, which + "negative row or property count");
        PET_REQUIRE(d.rows <= INT32_MAX, PET_ERR_ARGUMENT, which + "too many rows");
        PET_REQUIRE(d.system_of_row || d.rows <= n_systems, PET_ERR_ARGUMENT,
                    which + "more rows than systems and no system_of_row");
        const int64_t threads = d.rows * (int64_t)d.n_properties;
        if (threads == 0) continue;  // nothing to transform
        PET_REQUIRE(d.src && d.dst, PET_ERR_ARGUMENT, which + "null argument");
        PET_REQUIRE(d.src != d.dst, PET_ERR_ARGUMENT, which + "the transformation is out of place: dst must not be src");
        PET_REQUIRE(n_systems > 0 && d_wigner && d_parity, PET_ERR_ARGUMENT, which + "rows but no table");
        b.a[b.n] = d;
        b.improper_factor[b.n] = (float)(d.o3_sigma * ((d.o3_lambda & 1) ? -1 : 1));
        b.first_block[b.n] = (int)blocks;
        blocks += (threads + SPH_BLOCK - 1) / SPH_BLOCK;
        PET_REQUIRE(blocks <= INT32_MAX, PET_ERR_ARGUMENT, "too many rows in one call");
        bytes += (double)threads * 8.0 * (2 * d.o3_lambda + 1) + (double)d.rows * (d.system_of_row ? 4.0 : 0.0);
        b.n++;
    }
    if (b.n == 0) return PET_OK;
    b.first_block[b.n] = (int)blocks;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("o3_apply_spherical", st, 0.0, bytes);
    k_o3_apply_spherical<<<(unsigned)blocks, SPH_BLOCK, 0, st>>>(d_wigner, d_parity, wigner_width(l_max), (int)n_systems, b);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // extern "C"
