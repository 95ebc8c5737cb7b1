// Long-range (Ewald) features of `long_range: {enable: true}`: a periodic Coulomb sum over C channels of per-atom charges and
// its adjoints. The definition, the convention constants and the closed-form adjoints are in include/pet_hip.h (pet_ewald_*).
// Layout. Every heavy sum is a GEMM on the fp32 matrix core (v_mfma_f32_32x32x2_f32: exact fp32 products) of 32 rows per
// workgroup, four waves:
//   k_ew_sfac    S'[k][re|im][c] = w_k sum_j e^{i k.r_j} X[j][c]     rows k, contraction over the system's atoms, A GENERATED
//   k_ew_gather  V[i][c] = sum_k cos(k.r_i) S're + sin(k.r_i) S'im   rows atoms, contraction over k, A GENERATED
//   k_ew_pairs   V[i][c] = sum_{j != i} K(d_ij) X[j][c]               rows atoms, contraction over atoms, A GENERATED (open systems)
//   k_ew_force   acc[i][col] = [g_i | q_i] . [column operand]         rows atoms, contraction over 2 C channels; the generated
//                factor (phase and k, or K'(d) D / d) is applied to the product tile, which is then summed over its columns
// A generated phase is the product of three entries of the per-axis tables e^{2 pi i n s_a} (k_ew_tables: fp64 sincospi of
// the fractional coordinate, rounded once), staged in LDS for the 32 atoms a workgroup works on: cos(k.r) of a large fp32
// argument is never formed. Only one of every pair (k, -k) is walked (weight w_k = 2 G(k) / Omega).
// Order. A workgroup walks the contraction index from the system's first atom / first k-vector in chunks of 32, waves
// split columns (or column tiles, summed in wave order afterwards): every result is a function of its system alone and the
// same bits run to run. No atomics. The exclusion term and its adjoint are CSR row sums (one wave per atom, fp64 rows).
// Each chunk of 32 contraction indices is summed on its own and then added to a total, and a system's k-vectors are listed by
// descending |k| (small terms first): the k-space sum and the self term cancel to a few tenths of either, and one running
// fp32 sum over 7 000 k-vectors left 8.9e-6 of the largest potential where this order leaves 3.5e-7.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "model.h"

namespace pet {

namespace {

constexpr double EW_PREFACTOR = 0.5;  // P: torch-pme's Calculator halves the pair sum (convention table)
constexpr double EW_PI = 3.14159265358979323846;

struct EwSys {
    double inv[9];  // cell^{-1}, row-major: s_b = sum_a r_a inv[3 a + b]
    double vol;
    int periodic;
    int first_atom, n_atoms;
    int first_k, n_k;  // the walked half of the k-set
    int nm;            // table entries per axis this system uses
};

struct EwK {
    int n0, n1, n2;
    float w;           // 2 G(k) / Omega
    float kx, ky, kz;
    float k2;
};

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// e^{2 pi i n.s} of one atom from its three table rows T[0..NM), T[NM..2NM), T[2NM..3NM)
__device__ __forceinline__ void ew_phase(const float2* T, int NM, int n0, int n1, int n2, float& c, float& s) {
    float2 a = T[abs(n0)], b = T[NM + abs(n1)], d = T[2 * NM + abs(n2)];
    if (n0 < 0) a.y = -a.y;
    if (n1 < 0) b.y = -b.y;
    if (n2 < 0) d.y = -d.y;
    const float abx = a.x * b.x - a.y * b.y, aby = a.x * b.y + a.y * b.x;
    c = abx * d.x - aby * d.y;
    s = abx * d.y + aby * d.x;
}

// tab[atom][axis][m] = e^{2 pi i m s_axis}, m < NM (zero for the atoms of an open system)
__global__ void k_ew_tables(const float* __restrict__ pos, const int* __restrict__ gsys, const EwSys* __restrict__ sys, int N,
                            int NM, float2* __restrict__ tab) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * 3 * NM) return;
    const int m = (int)(idx % NM), ax = (int)((idx / NM) % 3), i = (int)(idx / (3 * NM));
    const EwSys& s = sys[gsys[i]];
    float2 out = make_float2(0.f, 0.f);
    if (s.periodic && m < s.nm) {
        double f = (double)pos[3 * (int64_t)i] * s.inv[ax] + (double)pos[3 * (int64_t)i + 1] * s.inv[3 + ax] +
                   (double)pos[3 * (int64_t)i + 2] * s.inv[6 + ax];
        f -= floor(f);
        double sn, cs;
        sincospi(2.0 * (double)m * f, &sn, &cs);
        out = make_float2((float)cs, (float)sn);
    }
    tab[idx] = out;
}

__device__ __forceinline__ void ew_stage_tables(float2* T, const float2* __restrict__ tab, int NM, int first_abs, int n_left) {
    const int per = 3 * NM;
    for (int idx = threadIdx.x; idx < 32 * per; idx += 256) {
        const int jj = idx / per;
        T[idx] = jj < n_left ? tab[(int64_t)first_abs * per + idx] : make_float2(0.f, 0.f);
    }
}

__global__ __launch_bounds__(256) void k_ew_sfac(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                 const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                 const float* __restrict__ X, int C, float* __restrict__ S) {
    extern __shared__ float2 T[];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int kidx = tile.y + r;
    int n0 = 0, n1 = 0, n2 = 0;
    if (kidx < s.n_k) {
        const EwK k = klist[s.first_k + kidx];
        n0 = k.n0; n1 = k.n1; n2 = k.n2;
    }
    const int c0 = blockIdx.y * 256 + wave * 64;
    const bool active = c0 < C;
    const bool in0 = c0 + r < C, in1 = c0 + 32 + r < C;
    // a chunk of 32 atoms is summed on its own and then added to the totals: rounding errors grow with the number of
    // chunks, not of terms
    f32x16 re0, im0, re1, im1, tre0, tim0, tre1, tim1;
#pragma unroll
    for (int i = 0; i < 16; i++) tre0[i] = tim0[i] = tre1[i] = tim1[i] = 0.f;
    for (int j0 = 0; j0 < s.n_atoms; j0 += 32) {
        __syncthreads();
        ew_stage_tables(T, tab, NM, s.first_atom + j0, s.n_atoms - j0);
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int i = 0; i < 16; i++) re0[i] = im0[i] = re1[i] = im1[i] = 0.f;
#pragma unroll 4
        for (int s2 = 0; s2 < 16; s2++) {
            const int jj = 2 * s2 + half;
            float c, sn;
            ew_phase(T + jj * 3 * NM, NM, n0, n1, n2, c, sn);
            const bool jin = j0 + jj < s.n_atoms;
            const float* row = X + (int64_t)(s.first_atom + j0 + jj) * C + c0 + r;
            const float b0 = jin && in0 ? row[0] : 0.f, b1 = jin && in1 ? row[32] : 0.f;
            re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, b0, re0, 0, 0, 0);
            im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sn, b0, im0, 0, 0, 0);
            re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, b1, re1, 0, 0, 0);
            im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sn, b1, im1, 0, 0, 0);
        }
        tre0 += re0; tim0 += im0; tre1 += re1; tim1 += im1;
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int kk = tile.y + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (kk >= s.n_k) continue;
        const int64_t kabs = s.first_k + kk;
        const float w = klist[kabs].w;
        float* o = S + kabs * 2 * C + c0 + r;
        if (in0) { o[0] = w * tre0[i]; o[C] = w * tim0[i]; }
        if (in1) { o[32] = w * tre1[i]; o[C + 32] = w * tim1[i]; }
    }
}

__global__ __launch_bounds__(256) void k_ew_gather(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                   const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                   const float* __restrict__ S, int C, float* __restrict__ V) {
    extern __shared__ float2 T[];
    __shared__ int4 kn[32];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int a0 = tile.y;
    ew_stage_tables(T, tab, NM, s.first_atom + a0, s.n_atoms - a0);
    const int c0 = blockIdx.y * 256 + wave * 64;
    const bool active = c0 < C;
    const bool in0 = c0 + r < C, in1 = c0 + 32 + r < C;
    const float2* Tr = T + r * 3 * NM;
    // chunks of 32 k-vectors are summed on their own and then added to the totals; the plan lists a system's k-vectors by
    // descending |k|, so the small terms come first
    f32x16 v0, v1, t0, t1;
#pragma unroll
    for (int i = 0; i < 16; i++) t0[i] = t1[i] = 0.f;
    for (int k0 = 0; k0 < s.n_k; k0 += 32) {
        __syncthreads();
        if (threadIdx.x < 32) {
            int4 n = make_int4(0, 0, 0, 0);
            if (k0 + (int)threadIdx.x < s.n_k) {
                const EwK k = klist[s.first_k + k0 + threadIdx.x];
                n = make_int4(k.n0, k.n1, k.n2, 1);
            }
            kn[threadIdx.x] = n;
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int i = 0; i < 16; i++) v0[i] = v1[i] = 0.f;
#pragma unroll 4
        for (int s2 = 0; s2 < 16; s2++) {
            const int kk = 2 * s2 + half;
            const int4 n = kn[kk];
            float c, sn;
            ew_phase(Tr, NM, n.x, n.y, n.z, c, sn);
            const float* row = S + (int64_t)(s.first_k + k0 + kk) * 2 * C + c0 + r;
            const bool kin = n.w != 0;
            const float br0 = kin && in0 ? row[0] : 0.f, bi0 = kin && in0 ? row[C] : 0.f;
            const float br1 = kin && in1 ? row[32] : 0.f, bi1 = kin && in1 ? row[C + 32] : 0.f;
            v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, br0, v0, 0, 0, 0);
            v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sn, bi0, v0, 0, 0, 0);
            v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, br1, v1, 0, 0, 0);
            v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sn, bi1, v1, 0, 0, 0);
        }
        t0 += v0; t1 += v1;
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int a = a0 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (a >= s.n_atoms) continue;
        float* o = V + (int64_t)(s.first_atom + a) * C + c0 + r;
        if (in0) o[0] = t0[i];
        if (in1) o[32] = t1[i];
    }
}

// K(d) = (1 - f(d)) / d and K'(d); 1 - f = sin^2(pi d / 2R) inside R
__device__ __forceinline__ float ew_open_kernel(float d, float inv_R) {
    if (d * inv_R >= 1.f) return 1.f / d;
    const float sn = sinpif(0.5f * d * inv_R);
    return sn * sn / d;
}
__device__ __forceinline__ float ew_open_kernel_d(float d, float inv_R) {
    if (d * inv_R >= 1.f) return -1.f / (d * d);
    const float sn = sinpif(0.5f * d * inv_R);
    return (0.5f * (float)EW_PI * inv_R * sinpif(d * inv_R) - sn * sn / d) / d;
}

__global__ __launch_bounds__(256) void k_ew_pairs(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                  const float* __restrict__ pos, float inv_R, const float* __restrict__ X,
                                                  int C, float* __restrict__ V) {
    __shared__ float4 ps[32];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int a0 = tile.y;
    const int i = a0 + r;
    float3 ri = make_float3(0.f, 0.f, 0.f);
    if (i < s.n_atoms) {
        const float* p = pos + 3 * (int64_t)(s.first_atom + i);
        ri = make_float3(p[0], p[1], p[2]);
    }
    const int c0 = blockIdx.y * 256 + wave * 64;
    const bool active = c0 < C;
    const bool in0 = c0 + r < C, in1 = c0 + 32 + r < C;
    f32x16 v0, v1, t0, t1;  // chunk sums and totals, as in k_ew_gather
#pragma unroll
    for (int q = 0; q < 16; q++) t0[q] = t1[q] = 0.f;
    for (int j0 = 0; j0 < s.n_atoms; j0 += 32) {
        __syncthreads();
        if (threadIdx.x < 32) {
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j0 + (int)threadIdx.x < s.n_atoms) {
                const float* q = pos + 3 * (int64_t)(s.first_atom + j0 + threadIdx.x);
                p = make_float4(q[0], q[1], q[2], 1.f);
            }
            ps[threadIdx.x] = p;
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int q = 0; q < 16; q++) v0[q] = v1[q] = 0.f;
#pragma unroll 4
        for (int s2 = 0; s2 < 16; s2++) {
            const int jj = 2 * s2 + half;
            const float4 pj = ps[jj];
            const float dx = pj.x - ri.x, dy = pj.y - ri.y, dz = pj.z - ri.z;
            const bool pair = pj.w != 0.f && i < s.n_atoms && j0 + jj != i;
            const float kern = pair ? ew_open_kernel(sqrtf(dx * dx + dy * dy + dz * dz), inv_R) : 0.f;
            const float* row = X + (int64_t)(s.first_atom + j0 + jj) * C + c0 + r;
            const bool jin = pj.w != 0.f;
            const float b0 = jin && in0 ? row[0] : 0.f, b1 = jin && in1 ? row[32] : 0.f;
            v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(kern, b0, v0, 0, 0, 0);
            v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kern, b1, v1, 0, 0, 0);
        }
        t0 += v0; t1 += v1;
    }
    if (!active) return;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int a = a0 + (q & 3) + 8 * (q >> 2) + 4 * half;
        if (a >= s.n_atoms) continue;
        float* o = V + (int64_t)(s.first_atom + a) * C + c0 + r;
        if (in0) o[0] = (float)EW_PREFACTOR * t0[q];
        if (in1) o[32] = (float)EW_PREFACTOR * t1[q];
    }
}

// sums[s][c] = sum over the atoms of system s of X[atom][c], in atom order (fp64)
__global__ __launch_bounds__(256) void k_ew_colsum(const EwSys* __restrict__ sys, const float* __restrict__ X, int C,
                                                   float* __restrict__ sums) {
    const EwSys& s = sys[blockIdx.x];
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (int a = 0; a < s.n_atoms; a++) acc += (double)X[(int64_t)(s.first_atom + a) * C + c];
    sums[(int64_t)blockIdx.x * C + c] = (float)acc;
}

// w(d) = erf(d / a) f(d) / d of an exclusion edge
__device__ __forceinline__ float ew_excl(float d, float inv_a, float inv_R) {
    if (d * inv_R >= 1.f) return 0.f;
    return erff(d * inv_a) * 0.5f * (1.f + cospif(d * inv_R)) / d;
}

// periodic systems: V <- P (V - q_i self - bg sums - sum_{row i} w(d) q_nbr); one wave per atom, lanes over channels
__global__ __launch_bounds__(256) void k_ew_finish(const EwSys* __restrict__ sys, const int* __restrict__ gsys,
                                                   const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                   const float4* __restrict__ geo, const float* __restrict__ X,
                                                   const float* __restrict__ sums, int N, int C, float self_c, float bg_c,
                                                   float inv_a, float inv_R, float* __restrict__ V) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int si = gsys[i];
    const EwSys& s = sys[si];
    if (!s.periodic) return;
    const int p0 = rowptr[i], p1 = rowptr[i + 1];
    const float bg = bg_c / (float)s.vol;
    for (int c = lane; c < C; c += 64) {
        float acc = 0.f;
        for (int p = p0; p < p1; p++) acc += ew_excl(geo[p].w, inv_a, inv_R) * X[(int64_t)nbr[p] * C + c];
        const int64_t o = (int64_t)i * C + c;
        V[o] = (float)EW_PREFACTOR * (V[o] - X[o] * self_c - bg * sums[(int64_t)si * C + c] - acc);
    }
}

__device__ __forceinline__ f32x4 ew_load4(bool valid, const float* p1, const float* p2, int ch, int C, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!valid) return v;
    if (vec) {
        if (ch < C) v = *reinterpret_cast<const f32x4*>(p1 + ch);
        else if (ch < 2 * C) v = *reinterpret_cast<const f32x4*>(p2 + ch - C);
        return v;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = ch + u;
        v[u] = c < C ? p1[c] : c < 2 * C ? p2[c - C] : 0.f;
    }
    return v;
}

// The position adjoint of the k-space sum (PER) / of the open all-pairs sum: F[i] = P sum_col gen(i, col) acc[i][col] with
// acc = [g_i | q_i] . [column operand] over 2 C channels (8 per step: a lane's float4 holds channels 8 t + 4 half + u, the same
// map for both operands). PER: columns are k-vectors, acc_a against [Im S'q | Im S'g], acc_b against [Re S'q | Re S'g],
// gen = k (cos acc_a - sin acc_b). Open: columns are atoms j, acc against [q_j | g_j], gen = -K'(d) (r_j - r_i) / d.
// Waves take column tiles wave, wave + 4, ...; their partial rows are added in wave order.
template <bool PER>
__global__ __launch_bounds__(256) void k_ew_force(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                  const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                  const float* __restrict__ pos, float inv_R, const float* __restrict__ G,
                                                  const float* __restrict__ Q, const float* __restrict__ Sq,
                                                  const float* __restrict__ Sg, int C, bool vec, float* __restrict__ F) {
    extern __shared__ float2 T[];
    __shared__ float4 ps[32];
    __shared__ float red[4 * 32 * 3];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int a0 = tile.y;
    if (PER) ew_stage_tables(T, tab, NM, s.first_atom + a0, s.n_atoms - a0);
    if (threadIdx.x < 32) {
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a0 + (int)threadIdx.x < s.n_atoms) {
            const float* q = pos + 3 * (int64_t)(s.first_atom + a0 + threadIdx.x);
            p = make_float4(q[0], q[1], q[2], 1.f);
        }
        ps[threadIdx.x] = p;
    }
    __syncthreads();
    const bool vi = a0 + r < s.n_atoms;
    const float* gi = G + (int64_t)(s.first_atom + a0 + r) * C;
    const float* qi = Q + (int64_t)(s.first_atom + a0 + r) * C;
    const int ncols = PER ? s.n_k : s.n_atoms;
    const int nsteps = (2 * C + 7) / 8;
    float f[16][3];
#pragma unroll
    for (int i = 0; i < 16; i++) f[i][0] = f[i][1] = f[i][2] = 0.f;
    for (int col0 = wave * 32; col0 < ncols; col0 += 128) {
        const int col = col0 + r;
        const bool vc = col < ncols;
        const float *a1, *a2, *b1 = nullptr, *b2 = nullptr;
        if (PER) {
            const int64_t kabs = s.first_k + col;
            a1 = Sq + (kabs * 2 + 1) * C; a2 = Sg + (kabs * 2 + 1) * C;
            b1 = Sq + kabs * 2 * C; b2 = Sg + kabs * 2 * C;
        } else {
            a1 = Q + (int64_t)(s.first_atom + col) * C; a2 = G + (int64_t)(s.first_atom + col) * C;
        }
        f32x16 acc_a, acc_b;
#pragma unroll
        for (int i = 0; i < 16; i++) acc_a[i] = acc_b[i] = 0.f;
        for (int t = 0; t < nsteps; t++) {
            const int ch = 8 * t + 4 * half;
            const f32x4 A = ew_load4(vi, gi, qi, ch, C, vec);
            const f32x4 Ba = ew_load4(vc, a1, a2, ch, C, vec);
#pragma unroll
            for (int u = 0; u < 4; u++) acc_a = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Ba[u], acc_a, 0, 0, 0);
            if (PER) {
                const f32x4 Bb = ew_load4(vc, b1, b2, ch, C, vec);
#pragma unroll
                for (int u = 0; u < 4; u++) acc_b = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Bb[u], acc_b, 0, 0, 0);
            }
        }
        if (PER) {
            int n0 = 0, n1 = 0, n2 = 0;
            float kx = 0.f, ky = 0.f, kz = 0.f;
            if (vc) {
                const EwK k = klist[s.first_k + col];
                n0 = k.n0; n1 = k.n1; n2 = k.n2; kx = k.kx; ky = k.ky; kz = k.kz;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
                float c, sn;
                ew_phase(T + row * 3 * NM, NM, n0, n1, n2, c, sn);
                const float x = c * acc_a[i] - sn * acc_b[i];
                f[i][0] += kx * x; f[i][1] += ky * x; f[i][2] += kz * x;
            }
        } else {
            float3 pj = make_float3(0.f, 0.f, 0.f);
            if (vc) {
                const float* q = pos + 3 * (int64_t)(s.first_atom + col);
                pj = make_float3(q[0], q[1], q[2]);
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
                const float4 pi = ps[row];
                if (!vc || pi.w == 0.f || col == a0 + row) continue;
                const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
                const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                const float co = -ew_open_kernel_d(d, inv_R) / d * acc_a[i];
                f[i][0] += co * dx; f[i][1] += co * dy; f[i][2] += co * dz;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            float v = f[i][a];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (r == 0) red[(wave * 32 + row) * 3 + a] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < 96) {
        const int row = threadIdx.x / 3, a = threadIdx.x % 3;
        if (a0 + row < s.n_atoms) {
            float v = red[row * 3 + a];
            for (int w = 1; w < 4; w++) v += red[(w * 32 + row) * 3 + a];
            F[3 * (int64_t)(s.first_atom + a0 + row) + a] = (float)EW_PREFACTOR * v;
        }
    }
}

// adjoint of the exclusion rows, one wave per atom; adds the k-space / all-pairs part F and leaves the per-atom part of
// dL/dcell (exclusion edges through S.cell, and -s_i F_i of the phases)
__global__ __launch_bounds__(64) void k_ew_edge_bwd(const EwSys* __restrict__ sys, const int* __restrict__ gsys,
                                                    const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                    const int* __restrict__ shift, const float4* __restrict__ geo,
                                                    const float* __restrict__ pos, const float* __restrict__ G,
                                                    const float* __restrict__ Q, const float* __restrict__ F, int C,
                                                    double sigma, double Rcut, float* __restrict__ gpos,
                                                    float* __restrict__ cell_part) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const EwSys& s = sys[gsys[i]];
    double fp[3] = {0.0, 0.0, 0.0}, cp[9];
#pragma unroll
    for (int k = 0; k < 9; k++) cp[k] = 0.0;
    const float fk[3] = {F[3 * (int64_t)i], F[3 * (int64_t)i + 1], F[3 * (int64_t)i + 2]};
    if (s.periodic) {
        const double inv_a = 1.0 / (sqrt(2.0) * sigma);
        const float* gi = G + (int64_t)i * C;
        const float* qi = Q + (int64_t)i * C;
        for (int p = rowptr[i]; p < rowptr[i + 1]; p++) {
            const int j = nbr[p];
            const float4 g4 = geo[p];
            const double d = (double)g4.w;
            if (d >= Rcut) continue;
            const float* gj = G + (int64_t)j * C;
            const float* qj = Q + (int64_t)j * C;
            float b = 0.f, bp = 0.f;
            for (int c = lane; c < C; c += 64) {
                b += gi[c] * qj[c];
                bp += gj[c] * qi[c];
            }
            b = wsum(b);
            bp = wsum(bp);
            const double x = d * inv_a, er = erf(x), cutf = 0.5 * (1.0 + cos(EW_PI * d / Rcut));
            const double dcut = -0.5 * EW_PI / Rcut * sin(EW_PI * d / Rcut);
            const double dw = (2.0 / sqrt(EW_PI) * inv_a * exp(-x * x) * cutf + er * dcut) / d - er * cutf / (d * d);
            const double co = EW_PREFACTOR * dw / d;
            const double D[3] = {(double)g4.x, (double)g4.y, (double)g4.z};
            const double bb = j == i ? 0.0 : (double)b + (double)bp;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                fp[a] += co * bb * D[a];
                const double sa = (double)shift[3 * (int64_t)p + a];
#pragma unroll
                for (int c = 0; c < 3; c++) cp[3 * a + c] -= co * (double)b * sa * D[c];
            }
        }
        double fr[3];
#pragma unroll
        for (int b = 0; b < 3; b++)
            fr[b] = (double)pos[3 * (int64_t)i] * s.inv[b] + (double)pos[3 * (int64_t)i + 1] * s.inv[3 + b] +
                    (double)pos[3 * (int64_t)i + 2] * s.inv[6 + b];
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int c = 0; c < 3; c++) cp[3 * b + c] -= fr[b] * (double)fk[c];
    }
    if (lane < 3) gpos[3 * (int64_t)i + lane] = (float)((double)fk[lane] + fp[lane]);
    if (cell_part && lane < 9) cell_part[9 * (int64_t)i + lane] = (float)cp[lane];
}

// per k-vector: its share of dL/dcell through G(k) and 1/Omega, kpart[k][9] (fp64); one wave per k
__global__ __launch_bounds__(256) void k_ew_zk(const EwSys* __restrict__ sys, const int* __restrict__ ksys,
                                               const EwK* __restrict__ klist, const float* __restrict__ Sq,
                                               const float* __restrict__ Sg, int C, int K, double sigma,
                                               double* __restrict__ kpart) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    const float* a = Sq + (int64_t)k * 2 * C;
    const float* b = Sg + (int64_t)k * 2 * C;
    float z = 0.f;
    for (int c = lane; c < 2 * C; c += 64) z += a[c] * b[c];
    z = wsum(z);
    if (lane < 9) {
        const EwSys& s = sys[ksys[k]];
        const EwK kk = klist[k];
        const double kv[3] = {(double)kk.kx, (double)kk.ky, (double)kk.kz};
        const int bb = lane / 3, cc = lane % 3;
        const double m = s.inv[bb] * kv[0] + s.inv[3 + bb] * kv[1] + s.inv[6 + bb] * kv[2];
        const double co = EW_PREFACTOR * (double)z / (double)kk.w;
        kpart[9 * (int64_t)k + lane] = co * ((sigma * sigma + 2.0 / (double)kk.k2) * m * kv[cc] - s.inv[3 * cc + bb]);
    }
}

// dL/dcell of system s: its atoms' parts, its k-vectors' parts (both in index order, 28 interleaved partial sums) and the
// background term
__global__ __launch_bounds__(256) void k_ew_cell(const EwSys* __restrict__ sys, const float* __restrict__ cell_part,
                                                 const double* __restrict__ kpart, const float* __restrict__ sum_g,
                                                 const float* __restrict__ sum_q, int C, double sigma,
                                                 float* __restrict__ out) {
    __shared__ double red[28][9];
    __shared__ double bg;
    const EwSys& s = sys[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 255) {
        double acc = 0.0;
        if (s.periodic)
            for (int c = 0; c < C; c++) acc += (double)sum_g[(int64_t)blockIdx.x * C + c] * (double)sum_q[(int64_t)blockIdx.x * C + c];
        bg = s.periodic ? EW_PREFACTOR * 2.0 * EW_PI * sigma * sigma / s.vol * acc : 0.0;
    }
    const int k = t / 9, c = t % 9;
    if (t < 252) {
        double acc = 0.0;
        for (int a = k; a < s.n_atoms; a += 28) acc += (double)cell_part[9 * (int64_t)(s.first_atom + a) + c];
        for (int q = k; q < s.n_k; q += 28) acc += kpart[9 * (int64_t)(s.first_k + q) + c];
        red[k][c] = acc;
    }
    __syncthreads();
    if (t < 9) {
        double v = 0.0;
        for (int j = 0; j < 28; j++) v += red[j][t];
        if (s.periodic) v += bg * s.inv[3 * (t % 3) + t / 3];
        out[9 * (int64_t)blockIdx.x + t] = (float)v;
    }
}

#ifndef PET_EWALD_SHARED_ONLY  // (p3m.hip compiles the kernels above together with its own and stops here)
// the walked half of the k-set of one cell: n with the first non-zero index positive, 0 < |k| <= kmax
int ew_half_kset(const double* cell, double lambda, double* inv, double* vol, std::vector<EwK>* out, int* nm) {
    const double* h = cell;
    const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
    if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) return -1;
    inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
    inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
    inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
    *vol = std::fabs(det);
    const double kmax = 2.0 * EW_PI / lambda;
    int nmax[3];
    for (int a = 0; a < 3; a++) {
        const double len = std::sqrt(h[3 * a] * h[3 * a] + h[3 * a + 1] * h[3 * a + 1] + h[3 * a + 2] * h[3 * a + 2]);
        const double m = std::floor(kmax * len / (2.0 * EW_PI) + 1e-9);
        if (m > 1e6) return -2;
        nmax[a] = (int)m;
    }
    *nm = std::max(nmax[0], std::max(nmax[1], nmax[2])) + 1;
    if (!out) return 0;
    for (int n0 = 0; n0 <= nmax[0]; n0++)
        for (int n1 = -nmax[1]; n1 <= nmax[1]; n1++)
            for (int n2 = -nmax[2]; n2 <= nmax[2]; n2++) {
                if (n0 == 0 && (n1 < 0 || (n1 == 0 && n2 <= 0))) continue;
                double k[3];
                for (int a = 0; a < 3; a++) k[a] = 2.0 * EW_PI * (inv[3 * a] * n0 + inv[3 * a + 1] * n1 + inv[3 * a + 2] * n2);
                const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
                if (!(k2 > 0.0) || k2 > kmax * kmax) continue;
                EwK e;
                e.n0 = n0; e.n1 = n1; e.n2 = n2;
                e.w = 0.f;
                e.kx = (float)k[0]; e.ky = (float)k[1]; e.kz = (float)k[2];
                e.k2 = (float)k2;
                out->push_back(e);
            }
    return 0;
}
#endif

}  // namespace

// P3M mode (csrc/p3m.hip): mesh descriptors and influence functions in place of k lists
struct P3mPlan;
void p3m_release(P3mPlan* p);
// geometry [S][10] = cell^{-1} and Omega; has_mesh [S]; chunks [S][2] receives every system's (first, count) reduction chunks
int p3m_plan_build(double sigma, double spacing, int nodes, const double* h_cells, const double* geometry, const int* has_mesh,
                   int64_t n_systems, int* chunks, P3mPlan** out);

}  // namespace pet

using namespace pet;

struct pet_ewald {
    double sigma = 0.0, lambda = 0.0, cutoff = 0.0;
    bool planned = false;
    int device = -1;
    int64_t n_atoms = 0, n_systems = 0, n_k = 0;
    int nm = 1;
    int p3m_nodes = 0;         // 0: Ewald mode; 1..5: P3M mode (pet_ewald_set_p3m)
    P3mPlan* p3m = nullptr;    // owned; rebuilt by every plan of a P3M-mode handle
    std::vector<EwSys> sys;
    std::vector<int2> ktiles, atiles_p, atiles_n;
    // device copies (made by pet_ewald_plan, kept until the next plan / destroy)
    EwSys* d_sys = nullptr;
    EwK* d_k = nullptr;
    int* d_ksys = nullptr;
    int2 *d_ktiles = nullptr, *d_atiles_p = nullptr, *d_atiles_n = nullptr;
    void release() {
        (void)hipFree(d_sys); (void)hipFree(d_k); (void)hipFree(d_ksys);
        (void)hipFree(d_ktiles); (void)hipFree(d_atiles_p); (void)hipFree(d_atiles_n);
        d_sys = nullptr; d_k = nullptr; d_ksys = nullptr; d_ktiles = d_atiles_p = d_atiles_n = nullptr;
        p3m_release(p3m);
        p3m = nullptr;
        planned = false;
    }
};

namespace {

template <class T>
int ew_upload(T** dst, const std::vector<T>& src) {
    const size_t n = std::max<size_t>(src.size(), 1);
    PET_HIP_CHECK(hipMalloc(dst, n * sizeof(T)));
    if (!src.empty()) PET_HIP_CHECK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PET_OK;
}


// what both modes ask of the graph
int ew_check_graph(const pet_ewald_t* e, const pet_graph_t* pg, int32_t C) {
    PET_REQUIRE(e && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->planned, PET_ERR_ARGUMENT, "pet_ewald_plan has not been called");
    PET_REQUIRE(C >= 1, PET_ERR_ARGUMENT, "n_channels must be at least 1");
    const Graph& g = pg->g;
    PET_REQUIRE(g.sys && (g.n_edges == 0 || g.shift), PET_ERR_ARGUMENT,
                "the long-range exclusion term needs a pet_graph_build handle (cell shifts, system indices): a "
                "pet_graph_from_batch handle has none");
    PET_REQUIRE(!g.adaptive, PET_ERR_ARGUMENT,
                "long range on a graph built under an adaptive cutoff: it drops edges inside the exclusion radius");
    PET_REQUIRE(pg->strict, PET_ERR_ARGUMENT,
                "long range needs the graph of a model with nl_is_strict (long_range.enable): every pair inside the cutoff");
    PET_REQUIRE(std::fabs((double)pg->cutoff - e->cutoff) <= 1e-5 * e->cutoff, PET_ERR_ARGUMENT,
                "the graph's cutoff " + std::to_string(pg->cutoff) + " is not the exclusion radius " +
                    std::to_string(e->cutoff) + " of this pet_ewald_t");
    PET_REQUIRE(g.n_nodes == e->n_atoms && g.n_systems == e->n_systems, PET_ERR_ARGUMENT,
                "the graph has " + std::to_string(g.n_nodes) + " atoms in " + std::to_string(g.n_systems) +
                    " systems, the plan " + std::to_string(e->n_atoms) + " in " + std::to_string(e->n_systems));
    int device = 0;
    PET_HIP_CHECK(hipGetDevice(&device));
    PET_REQUIRE(device == e->device, PET_ERR_ARGUMENT, "the plan was made on another device");
    return PET_OK;
}

}  // namespace

#ifndef PET_EWALD_SHARED_ONLY
namespace {

struct EwWs {
    float2* tab;
    float *S1, *S2, *sum1, *sum2, *F, *cell_part;
    double* kpart;
};

size_t ew_carve(const pet_ewald_t* e, int64_t C, void* base, EwWs& w) {
    Carver c(base);
    const size_t N = (size_t)std::max<int64_t>(e->n_atoms, 1), K = (size_t)std::max<int64_t>(e->n_k, 1);
    const size_t S = (size_t)std::max<int64_t>(e->n_systems, 1);
    w.tab = c.take<float2>(N * 3 * e->nm);
    w.S1 = c.take<float>(K * 2 * C);
    w.S2 = c.take<float>(K * 2 * C);
    w.sum1 = c.take<float>(S * C);
    w.sum2 = c.take<float>(S * C);
    w.F = c.take<float>(N * 3);
    w.cell_part = c.take<float>(N * 9);
    w.kpart = c.take<double>(K * 9);
    return c.off;
}

int ew_check(const pet_ewald_t* e, const pet_graph_t* pg, int32_t C, const void* ws, int64_t ws_bytes) {
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes == 0, PET_ERR_ARGUMENT,
                "a pet_ewald_* entry point on a P3M-mode handle (pet_ewald_set_p3m): use pet_p3m_spread / _filter / _finish / "
                "_backward");
    PET_TRY(ew_check_graph(e, pg, C));
    EwWs w;
    PET_REQUIRE(e->n_atoms == 0 || (ws && ws_bytes >= (int64_t)ew_carve(e, C, nullptr, w)), PET_ERR_ARGUMENT,
                "Ewald workspace too small (pet_ewald_workspace_bytes)");
    return PET_OK;
}

size_t ew_table_lds(const pet_ewald_t* e) { return (size_t)32 * 3 * e->nm * sizeof(float2); }

int ew_tables(const pet_ewald_t* e, const Graph& g, const float* pos, const EwWs& w, hipStream_t st) {
    const int64_t n = e->n_atoms * 3 * e->nm;
    k_ew_tables<<<cdiv(n, 256), 256, 0, st>>>(pos, g.sys, e->d_sys, (int)e->n_atoms, e->nm, w.tab);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// out = the operator applied to X [N, C]; leaves S'(X) in Sbuf and the per-system column sums in sums
int ew_apply(const pet_ewald_t* e, const Graph& g, const float* pos, const float* X, int C, float* out, const EwWs& w,
             float* Sbuf, float* sums, hipStream_t st) {
    const unsigned cy = (unsigned)cdiv(C, 256);
    const size_t lds = ew_table_lds(e);
    if (!e->ktiles.empty())
        k_ew_sfac<<<dim3((unsigned)e->ktiles.size(), cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, X, C, Sbuf);
    if (!e->atiles_p.empty())
        k_ew_gather<<<dim3((unsigned)e->atiles_p.size(), cy), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, Sbuf,
                                                                            C, out);
    if (!e->atiles_n.empty())
        k_ew_pairs<<<dim3((unsigned)e->atiles_n.size(), cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, (float)(1.0 / e->cutoff),
                                                                          X, C, out);
    k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, X, C, sums);
    k_ew_finish<<<cdiv(e->n_atoms, 4), 256, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.geo, X, sums, (int)e->n_atoms, C,
                                                     (float)(std::sqrt(2.0 / EW_PI) / e->sigma),
                                                     (float)(2.0 * EW_PI * e->sigma * e->sigma),
                                                     (float)(1.0 / (std::sqrt(2.0) * e->sigma)), (float)(1.0 / e->cutoff), out);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace

extern "C" {

int pet_ewald_create(double smearing, double kspace_resolution, double cutoff, pet_ewald_t** out) {
    PET_REQUIRE(out, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(smearing > 0.0 && std::isfinite(smearing), PET_ERR_ARGUMENT, "smearing must be a positive number");
    PET_REQUIRE(kspace_resolution > 0.0 && std::isfinite(kspace_resolution), PET_ERR_ARGUMENT,
                "kspace_resolution must be a positive number");
    PET_REQUIRE(cutoff > 0.0 && std::isfinite(cutoff), PET_ERR_ARGUMENT, "cutoff must be a positive number");
    pet_ewald_t* e = new pet_ewald_t();
    e->sigma = smearing;
    e->lambda = kspace_resolution;
    e->cutoff = cutoff;
    *out = e;
    return PET_OK;
}

void pet_ewald_destroy(pet_ewald_t* e) {
    if (!e) return;
    e->release();
    delete e;
}

int64_t pet_ewald_kvectors_host(const double* h_cell, double kspace_resolution, double* h_out, int64_t capacity) {
    if (!h_cell || !(kspace_resolution > 0.0)) return -1;
    double inv[9], vol;
    int nm;
    std::vector<EwK> half;
    if (ew_half_kset(h_cell, kspace_resolution, inv, &vol, &half, &nm) != 0) return -1;
    const int64_t n = 2 * (int64_t)half.size();
    if (h_out && capacity >= n)
        for (size_t i = 0; i < half.size(); i++)
            for (int sgn = 0; sgn < 2; sgn++) {
                const double f = sgn ? -1.0 : 1.0;
                const EwK& k = half[i];
                for (int a = 0; a < 3; a++)
                    h_out[3 * (2 * i + sgn) + a] = f * 2.0 * EW_PI * (inv[3 * a] * k.n0 + inv[3 * a + 1] * k.n1 + inv[3 * a + 2] * k.n2);
            }
    return n;
}

int pet_ewald_plan(pet_ewald_t* e, const double* h_cells, const int32_t* h_pbc, const int64_t* h_first_atom,
                   int64_t n_systems) {
    PET_REQUIRE(e && h_first_atom && (n_systems == 0 || (h_cells && h_pbc)), PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(n_systems >= 0 && n_systems < (1 << 24), PET_ERR_ARGUMENT, "bad n_systems");
    std::vector<EwSys> sys((size_t)n_systems);
    std::vector<EwK> ks;
    std::vector<int> ksys;
    std::vector<int2> ktiles, ap, an;
    int nm_all = 1;
    PET_REQUIRE(h_first_atom[0] == 0, PET_ERR_ARGUMENT, "h_first_atom must start at 0");
    for (int64_t s = 0; s < n_systems; s++) {
        EwSys& y = sys[(size_t)s];
        const int64_t a0 = h_first_atom[s], a1 = h_first_atom[s + 1];
        PET_REQUIRE(a1 >= a0 && a1 < (int64_t(1) << 30), PET_ERR_ARGUMENT, "h_first_atom must be non-decreasing");
        const int np = (h_pbc[3 * s] != 0) + (h_pbc[3 * s + 1] != 0) + (h_pbc[3 * s + 2] != 0);
        PET_REQUIRE(np == 0 || np == 3, PET_ERR_UNSUPPORTED,
                    "long range with mixed pbc (system " + std::to_string(s) + "): only fully periodic and fully open "
                    "systems are served (the reference refuses 1D and leaves 2D to torch-pme)");
        for (int k = 0; k < 9; k++) y.inv[k] = 0.0;
        y.vol = 1.0;
        y.periodic = np == 3;
        y.first_atom = (int)a0;
        y.n_atoms = (int)(a1 - a0);
        y.first_k = (int)ks.size();
        y.n_k = 0;
        y.nm = 1;
        if (y.periodic && e->p3m_nodes) {
            // P3M mode: the inverse cell and the volume only; no k list and no limit on the cell's length
            const int rc = ew_half_kset(h_cells + 9 * s, e->lambda, y.inv, &y.vol, nullptr, &y.nm);
            PET_REQUIRE(rc != -1, PET_ERR_ARGUMENT, "the cell of periodic system " + std::to_string(s) + " is singular");
            y.nm = 1;
        } else if (y.periodic) {
            const size_t before = ks.size();
            const int rc = ew_half_kset(h_cells + 9 * s, e->lambda, y.inv, &y.vol, nullptr, &y.nm);
            PET_REQUIRE(rc != -1, PET_ERR_ARGUMENT, "the cell of periodic system " + std::to_string(s) + " is singular");
            PET_REQUIRE(rc == 0 && y.nm - 1 <= PET_EWALD_MAX_INDEX, PET_ERR_UNSUPPORTED,
                        "system " + std::to_string(s) + " needs reciprocal indices up to " + std::to_string(y.nm - 1) +
                            " at this kspace_resolution; at most " + std::to_string(PET_EWALD_MAX_INDEX) +
                            " are served (the Ewald sum costs O(N K): large boxes are what P3M is for: pet_ewald_set_p3m)");
            (void)ew_half_kset(h_cells + 9 * s, e->lambda, y.inv, &y.vol, &ks, &y.nm);
            y.n_k = (int)(ks.size() - before);
            // by descending |k| (ties in enumeration order): the gather adds the small terms first
            std::stable_sort(ks.begin() + (std::ptrdiff_t)before, ks.end(), [](const EwK& a, const EwK& b) { return a.k2 > b.k2; });
            for (size_t i = before; i < ks.size(); i++) {
                // G(k) from the fp64 k of the integer triple
                double k[3], kk = 0.0;
                for (int a = 0; a < 3; a++) {
                    k[a] = 2.0 * EW_PI * (y.inv[3 * a] * ks[i].n0 + y.inv[3 * a + 1] * ks[i].n1 + y.inv[3 * a + 2] * ks[i].n2);
                    kk += k[a] * k[a];
                }
                ks[i].w = (float)(2.0 * 4.0 * EW_PI * std::exp(-0.5 * e->sigma * e->sigma * kk) / kk / y.vol);
                ksys.push_back((int)s);
            }
            nm_all = std::max(nm_all, y.nm);
            for (int k0 = 0; k0 < y.n_k; k0 += 32) ktiles.push_back(make_int2((int)s, k0));
        }
        for (int a = 0; a < y.n_atoms; a += 32) (y.periodic ? ap : an).push_back(make_int2((int)s, a));
    }
    PET_REQUIRE(ks.size() < (size_t(1) << 28), PET_ERR_UNSUPPORTED, "too many k-vectors in one batch");
    P3mPlan* mesh_plan = nullptr;
    if (e->p3m_nodes) {
        std::vector<double> geometry((size_t)n_systems * 10);
        std::vector<int> has_mesh((size_t)n_systems), chunks((size_t)n_systems * 2);
        for (int64_t s = 0; s < n_systems; s++) {
            for (int k = 0; k < 9; k++) geometry[(size_t)s * 10 + k] = sys[(size_t)s].inv[k];
            geometry[(size_t)s * 10 + 9] = sys[(size_t)s].vol;
            has_mesh[(size_t)s] = sys[(size_t)s].periodic && sys[(size_t)s].n_atoms > 0;
        }
        PET_TRY(p3m_plan_build(e->sigma, e->lambda, e->p3m_nodes, h_cells, geometry.data(), has_mesh.data(), n_systems,
                               chunks.data(), &mesh_plan));
        // k_ew_cell walks a system's reduction chunks where it walks k-vectors in Ewald mode
        for (int64_t s = 0; s < n_systems; s++) {
            sys[(size_t)s].first_k = chunks[(size_t)s * 2];
            sys[(size_t)s].n_k = chunks[(size_t)s * 2 + 1];
        }
    }
    e->release();
    e->p3m = mesh_plan;
    PET_HIP_CHECK(hipGetDevice(&e->device));
    PET_TRY(ew_upload(&e->d_sys, sys));
    PET_TRY(ew_upload(&e->d_k, ks));
    PET_TRY(ew_upload(&e->d_ksys, ksys));
    PET_TRY(ew_upload(&e->d_ktiles, ktiles));
    PET_TRY(ew_upload(&e->d_atiles_p, ap));
    PET_TRY(ew_upload(&e->d_atiles_n, an));
    e->sys = sys;
    e->ktiles = ktiles;
    e->atiles_p = ap;
    e->atiles_n = an;
    e->n_systems = n_systems;
    e->n_atoms = n_systems ? h_first_atom[n_systems] : 0;
    e->n_k = (int64_t)ks.size();
    e->nm = nm_all;
    e->planned = true;
    return PET_OK;
}

int64_t pet_ewald_num_kvectors(const pet_ewald_t* e, int64_t system) {
    if (!e || !e->planned || e->p3m_nodes || system < 0 || system >= e->n_systems) return -1;
    return 2 * (int64_t)e->sys[(size_t)system].n_k;
}

int64_t pet_ewald_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || e->p3m_nodes || n_channels < 1) return -1;
    EwWs w;
    return (int64_t)ew_carve(e, n_channels, nullptr, w);
}

int pet_ewald_potential(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                        int32_t C, float* d_potential, void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = ew_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    if (e->n_atoms == 0) return PET_OK;
    PET_REQUIRE(d_positions && d_charges && d_potential, PET_ERR_ARGUMENT, "null argument");
    hipStream_t st = (hipStream_t)stream;
    EwWs w;
    ew_carve(e, C, d_workspace, w);
    ProfScope ps("ewald_fwd", st, 0.0, 0.0);
    PET_TRY(ew_tables(e, pg->g, d_positions, w, st));
    return ew_apply(e, pg->g, d_positions, d_charges, C, d_potential, w, w.S1, w.sum1, st);
}

int pet_ewald_backward(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                       const float* d_grad_potential, int32_t C, float* d_grad_charges, float* d_grad_positions,
                       float* d_grad_cells, void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = ew_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Graph& g = pg->g;
    if (e->n_atoms == 0) {
        if (d_grad_cells && e->n_systems > 0)
            PET_HIP_CHECK(hipMemsetAsync(d_grad_cells, 0, (size_t)e->n_systems * 9 * sizeof(float), st));
        return PET_OK;
    }
    PET_REQUIRE(d_positions && d_charges && d_grad_potential && d_grad_charges && d_grad_positions, PET_ERR_ARGUMENT,
                "null argument");
    EwWs w;
    ew_carve(e, C, d_workspace, w);
    ProfScope ps("ewald_bwd", st, 0.0, 0.0);
    PET_TRY(ew_tables(e, g, d_positions, w, st));
    // dL/dq = the operator applied to g: leaves S'(g) in S2 and the column sums of g in sum2
    PET_TRY(ew_apply(e, g, d_positions, d_grad_potential, C, d_grad_charges, w, w.S2, w.sum2, st));
    const unsigned cy = (unsigned)cdiv(C, 256);
    const size_t lds = ew_table_lds(e);
    if (!e->ktiles.empty())
        k_ew_sfac<<<dim3((unsigned)e->ktiles.size(), cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, d_charges,
                                                                          C, w.S1);
    k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, d_charges, C, w.sum1);
    const bool vec = C % 4 == 0 && ((uintptr_t)d_charges & 15) == 0 && ((uintptr_t)d_grad_potential & 15) == 0;
    const float inv_R = (float)(1.0 / e->cutoff);
    if (!e->atiles_p.empty())
        k_ew_force<true><<<(unsigned)e->atiles_p.size(), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, d_positions,
                                                                         inv_R, d_grad_potential, d_charges, w.S1, w.S2, C, vec, w.F);
    if (!e->atiles_n.empty())
        k_ew_force<false><<<(unsigned)e->atiles_n.size(), 256, 0, st>>>(e->d_atiles_n, e->d_sys, e->d_k, w.tab, e->nm, d_positions,
                                                                        inv_R, d_grad_potential, d_charges, w.S1, w.S2, C, vec, w.F);
    k_ew_edge_bwd<<<(unsigned)e->n_atoms, 64, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.shift, g.geo, d_positions,
                                                       d_grad_potential, d_charges, w.F, C, e->sigma, e->cutoff, d_grad_positions,
                                                       d_grad_cells ? w.cell_part : nullptr);
    if (d_grad_cells) {
        if (e->n_k > 0)
            k_ew_zk<<<cdiv(e->n_k, 4), 256, 0, st>>>(e->d_sys, e->d_ksys, e->d_k, w.S1, w.S2, C, (int)e->n_k, e->sigma, w.kpart);
        k_ew_cell<<<(unsigned)e->n_systems, 256, 0, st>>>(e->d_sys, w.cell_part, w.kpart, w.sum2, w.sum1, C, e->sigma, d_grad_cells);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // extern "C"
#endif  // PET_EWALD_SHARED_ONLY
