// The long-range operator (q [N, C] -> V [N, C], its adjoint and its second-order operation) behind ONE internal interface, and
// what its two evaluations share: ewald.hip (the reciprocal-space sum over a k list) and p3m.hip (the same sum on a mesh).
//
// THE INTERFACE is the first part of this header, which gen_train.hip and abi.hip include as it is: a
// call context (LrCall) and four functions that decide the handle's mode in one place (ewald.hip). The extern "C" entry
// points of a mode run the functions that the interface dispatches to, so every launch list is stated once.
//
// THE SHARED PART, for the two translation units that define LONG_RANGE_SHARED_PART before they include this header (they
// include nothing of each other): the handle (pet_ewald), its per-system record, the one cell inverse, what both ask of a
// graph and of a second-order call, and the LOCAL terms (self, background, exclusion, the open all-pairs sum) with their
// adjoints: kernels and the host functions that launch them. The operator's convention constants (include/pet_hip.h, DESIGN.md
// section 18) are EW_PREFACTOR and the three coefficients of ew_local_forward; a mode adds only its weight 2 G(k) / Omega
// (ewald.hip: ew_plan_klist) or G^(n) / Omega (p3m.hip: p3m_influence_point).
// k_ew_pairs<true>, k_ew_force2, k_ew_edge_second and ew_open_kernel_dd serve both modes' second derivatives (p3m.hip has no k
// tiles and instantiates k_ew_force2<false> alone); k_ew_uprime, k_ew_edge_cell and ew_local_cell both modes' cell tangents.
// Kernels and functions of the shared part have internal linkage: each translation unit is compiled on its own (build.py:
// NO_RDC) with its own copy of what it launches. Only the two record types, the P3M plan's entry points and a mode's half of
// the interface (p3m_*) have names that cross objects.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "model.h"

struct pet_ewald;

namespace pet {

// One call of the operator from inside a running entry point: a planned handle that the caller has checked against the graph
// (lr_check, or a mode's own entry check), at C channels, on a workspace of lr_workspace_bytes(e, C, cell) that lies ws_offset
// bytes into that entry point's d_workspace (what a P3M handle's transform hook counts its offsets from; the Ewald sum
// ignores it). A call without a cell tangent runs on either size: the cell workspace begins with the other.
struct LrCall {
    const pet_ewald* e;
    const Graph* g;
    const float* pos;
    int C;
    void* ws;
    int64_t ws_offset;
    hipStream_t st;
};
// Ewald mode, or P3M mode with a transform hook (pet_p3m_set_transform); then what both modes ask of the graph
int lr_check(const pet_ewald* e, const pet_graph_t* pg, int C, const char* who);
int64_t lr_workspace_bytes(const pet_ewald* e, int C, bool cell);
// out = A X
int lr_potential(const LrCall& c, const float* X, float* out);
// gq = A G and gpos = grad_r Phi(r; G, Q); with gcell also dL/dcell [S, 3, 3] (Ewald mode: the mesh operator's needs the two
// unfiltered spectra that its staged entry point pet_p3m_backward is given)
int lr_backward(const LrCall& c, const float* Q, const float* G, float* gq, float* gpos, float* gcell = nullptr);
// The second-order operation along (Uq [N, C], Ur [N, 3], Ucell [S, 3, 3]; each may be null, not all): a null result is not
// formed and the launches that serve it alone are skipped; Q may be null where only out_q is asked for, G where only out_g is.
// out_r together with Ucell is not built (mixed position / cell second derivatives).
int lr_second(const LrCall& c, const float* Q, const float* G, const float* Uq, const float* Ur, const float* Ucell, float* out_q,
              float* out_g, float* out_r);

}  // namespace pet

#ifdef LONG_RANGE_SHARED_PART

namespace pet {

// One system of a plan, uploaded as it is. first_k / n_k is the system's range of RECIPROCAL-SPACE PARTS, the entries of kpart
// that k_ew_cell adds into dL/dcell in index order: in Ewald mode the walked half of the k-set (also its range of the k list),
// in P3M mode the system's reduction chunks of P3M_CHUNK half-spectrum points (written by k_p3m_cell; there is no k list).
struct EwSys {
    double inv[9];  // cell^{-1}, row-major: s_b = sum_a r_a inv[3 a + b]
    double vol;
    int periodic;
    int first_atom, n_atoms;
    int first_k, n_k;  // reciprocal-space parts (above)
    int nm;            // table entries per axis this system uses (Ewald mode; 1 otherwise)
};

struct EwK {
    int n0, n1, n2;
    float w;           // 2 G(k) / Omega
    float kx, ky, kz;
    float k2;
};

namespace {

constexpr double EW_PREFACTOR = 0.5;  // P: torch-pme's Calculator halves the pair sum (convention table)
constexpr double EW_PI = 3.14159265358979323846;

// cell^{-1} (row-major) and |det|; false for a singular cell
inline bool ew_cell_inverse(const double* h, double* inv, double* vol) {
    const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
    if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) return false;
    inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
    inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
    inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
    *vol = std::fabs(det);
    return true;
}

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

__device__ __forceinline__ void ew_stage_tables(float2* T, const float2* __restrict__ tab, int NM, int first_abs, int n_left) {
    const int per = 3 * NM;
    for (int idx = threadIdx.x; idx < 32 * per; idx += 256) {
        const int jj = idx / per;
        T[idx] = jj < n_left ? tab[(int64_t)first_abs * per + idx] : make_float2(0.f, 0.f);
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

// K''(d), with A = sin^2(pi d / 2R): K = A / d, K'' = A''/d - 2 A'/d^2 + 2 A/d^3 (f = 0 beyond R: f'' jumps there)
__device__ __forceinline__ float ew_open_kernel_dd(float d, float inv_R) {
    if (d * inv_R >= 1.f) return 2.f / (d * d * d);
    const float sn = sinpif(0.5f * d * inv_R);
    const float a1 = 0.5f * (float)EW_PI * inv_R * sinpif(d * inv_R);
    const float a2 = 0.5f * (float)(EW_PI * EW_PI) * inv_R * inv_R * cospif(d * inv_R);
    return (a2 - 2.f * (a1 - sn * sn / d) / d) / d;
}

// DIR: the directional derivative along U [N, 3] in place of the sum itself, V[i][c] += P sum_{j != i} K'(d) (n . (u_j - u_i))
// X[j][c] with n = (r_j - r_i) / d, ADDED to V (pet_ewald_second)
template <bool DIR>
__global__ __launch_bounds__(256) void k_ew_pairs(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                  const float* __restrict__ pos, float inv_R, const float* __restrict__ X,
                                                  int C, float* __restrict__ V, const float* __restrict__ U) {
    __shared__ float4 ps[32];
    __shared__ float4 us[DIR ? 32 : 1];
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
    float3 ui = make_float3(0.f, 0.f, 0.f);
    if (DIR && i < s.n_atoms) {
        const float* p = U + 3 * (int64_t)(s.first_atom + i);
        ui = make_float3(p[0], p[1], p[2]);
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
        if (DIR && threadIdx.x >= 64 && threadIdx.x < 96) {
            const int jj = threadIdx.x - 64;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j0 + jj < s.n_atoms) {
                const float* q = U + 3 * (int64_t)(s.first_atom + j0 + jj);
                u = make_float4(q[0], q[1], q[2], 0.f);
            }
            us[jj] = u;
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
            float kern = 0.f;
            if (DIR) {
                if (pair) {
                    const float4 uj = us[jj];
                    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                    kern = ew_open_kernel_d(d, inv_R) * (dx * (uj.x - ui.x) + dy * (uj.y - ui.y) + dz * (uj.z - ui.z)) / d;
                }
            } else {
                kern = pair ? ew_open_kernel(sqrtf(dx * dx + dy * dy + dz * dz), inv_R) : 0.f;
            }
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
        if (DIR) {
            if (in0) o[0] += (float)EW_PREFACTOR * t0[q];
            if (in1) o[32] += (float)EW_PREFACTOR * t1[q];
        } else {
            if (in0) o[0] = (float)EW_PREFACTOR * t0[q];
            if (in1) o[32] = (float)EW_PREFACTOR * t1[q];
        }
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

// The position Hessian of Phi = sum_c g^T A q applied to the direction U [N, 3] (pet_ewald_second), k-space (PER) / open
// all-pairs part, in the form of k_ew_force: F[i] = P sum_col gen(i, col) . [product tiles], rows [g_i | q_i] over 2 C channels.
// PER: four tiles per column tile of 32 k-vectors, against [Re S'_q | Re S'_g], [Im S'_q | Im S'_g] and the same of the
// weighted structure factors S'_{uq} | S'_{ug}: gen = k [ (c Re_u + s Im_u) - (k.u_i) (c Re + s Im) ].
// Open: one tile against [q_j | g_j], gen = -M_K (u_j - u_i), M_K = K'' n n^T + (K'/d) (I - n n^T), n = (r_j - r_i) / d.
template <bool PER>
__global__ __launch_bounds__(256) void k_ew_force2(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                   const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                   const float* __restrict__ pos, float inv_R, const float* __restrict__ G,
                                                   const float* __restrict__ Q, const float* __restrict__ Sq,
                                                   const float* __restrict__ Sg, const float* __restrict__ Suq,
                                                   const float* __restrict__ Sug, const float* __restrict__ U, int C, bool vec,
                                                   float* __restrict__ F) {
    extern __shared__ float2 T[];
    __shared__ float4 ps[32];
    __shared__ float4 us[32];
    __shared__ float red[4 * 32 * 3];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int a0 = tile.y;
    if (PER) ew_stage_tables(T, tab, NM, s.first_atom + a0, s.n_atoms - a0);
    if (threadIdx.x < 32) {
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a0 + (int)threadIdx.x < s.n_atoms) {
            const float* q = pos + 3 * (int64_t)(s.first_atom + a0 + threadIdx.x);
            const float* v = U + 3 * (int64_t)(s.first_atom + a0 + threadIdx.x);
            p = make_float4(q[0], q[1], q[2], 1.f);
            u = make_float4(v[0], v[1], v[2], 0.f);
        }
        ps[threadIdx.x] = p;
        us[threadIdx.x] = u;
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
        f32x16 acc_r, acc_i, acu_r, acu_i;  // (open: acc_r alone)
#pragma unroll
        for (int i = 0; i < 16; i++) acc_r[i] = acc_i[i] = acu_r[i] = acu_i[i] = 0.f;
        if (PER) {
            const int64_t kabs = s.first_k + col;
            const float *re1 = Sq + kabs * 2 * C, *re2 = Sg + kabs * 2 * C, *ur1 = Suq + kabs * 2 * C, *ur2 = Sug + kabs * 2 * C;
            for (int t = 0; t < nsteps; t++) {
                const int ch = 8 * t + 4 * half;
                const f32x4 A = ew_load4(vi, gi, qi, ch, C, vec);
                const f32x4 Br = ew_load4(vc, re1, re2, ch, C, vec), Bi = ew_load4(vc, re1 + C, re2 + C, ch, C, vec);
                const f32x4 Ur = ew_load4(vc, ur1, ur2, ch, C, vec), Ui = ew_load4(vc, ur1 + C, ur2 + C, ch, C, vec);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Br[u], acc_r, 0, 0, 0);
                    acc_i = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Bi[u], acc_i, 0, 0, 0);
                    acu_r = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Ur[u], acu_r, 0, 0, 0);
                    acu_i = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Ui[u], acu_i, 0, 0, 0);
                }
            }
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
                const float4 u = us[row];
                const float ku = kx * u.x + ky * u.y + kz * u.z;
                const float x = (c * acu_r[i] + sn * acu_i[i]) - ku * (c * acc_r[i] + sn * acc_i[i]);
                f[i][0] += kx * x; f[i][1] += ky * x; f[i][2] += kz * x;
            }
        } else {
            const float* a1 = Q + (int64_t)(s.first_atom + col) * C;
            const float* a2 = G + (int64_t)(s.first_atom + col) * C;
            for (int t = 0; t < nsteps; t++) {
                const int ch = 8 * t + 4 * half;
                const f32x4 A = ew_load4(vi, gi, qi, ch, C, vec);
                const f32x4 Ba = ew_load4(vc, a1, a2, ch, C, vec);
#pragma unroll
                for (int u = 0; u < 4; u++) acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(A[u], Ba[u], acc_r, 0, 0, 0);
            }
            float3 pj = make_float3(0.f, 0.f, 0.f), uj = make_float3(0.f, 0.f, 0.f);
            if (vc) {
                const float* q = pos + 3 * (int64_t)(s.first_atom + col);
                const float* v = U + 3 * (int64_t)(s.first_atom + col);
                pj = make_float3(q[0], q[1], q[2]);
                uj = make_float3(v[0], v[1], v[2]);
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
                const float4 pi = ps[row];
                if (!vc || pi.w == 0.f || col == a0 + row) continue;
                const float4 u = us[row];
                const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
                const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                const float nx = dx / d, ny = dy / d, nz = dz / d;
                const float ex = uj.x - u.x, ey = uj.y - u.y, ez = uj.z - u.z;
                const float nd = nx * ex + ny * ey + nz * ez;
                const float kd = ew_open_kernel_d(d, inv_R) / d, kdd = ew_open_kernel_dd(d, inv_R);
                const float along = (kdd - kd) * nd;  // M_K e = (K'' - K'/d) (n.e) n + (K'/d) e
                f[i][0] -= acc_r[i] * (along * nx + kd * ex);
                f[i][1] -= acc_r[i] * (along * ny + kd * ey);
                f[i][2] -= acc_r[i] * (along * nz + kd * ez);
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

// The exclusion rows' share of all three results of pet_ewald_second, one wave per atom, fp64 like k_ew_edge_bwd. Per edge
// p = (i -> j, S) with e = u_j - u_i, n = D / d:  out_g[i] -= P w'(d) (n.e) q_j,  out_q[i] -= P w'(d) (n.e) g_j  and
// out_r[i] += P (B_p + B'_p) M_w e,  M_w = w'' n n^T + (w'/d) (I - n n^T). Lanes take one edge each of a chunk of 64 for w', w''
// and M_w e, then all lanes walk the chunk's edges for the channel sums. Adds F2 (k_ew_force2) into out_r for every atom.
// A null result is not formed (ew_second, p3m_second): without out_r neither F2 nor the channel products are read, without out_g
// (out_q) Q (G) is not read in the channel sums; each sum is its own accumulator, so the others keep their bits.
__global__ __launch_bounds__(64) void k_ew_edge_second(const EwSys* __restrict__ sys, const int* __restrict__ gsys,
                                                       const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                       const float4* __restrict__ geo, const float* __restrict__ G,
                                                       const float* __restrict__ Q, const float* __restrict__ U,
                                                       const float* __restrict__ F2, int C, double sigma, double Rcut,
                                                       float* __restrict__ out_g, float* __restrict__ out_q,
                                                       float* __restrict__ out_r) {
    __shared__ int sj[64];
    __shared__ double sco[64], sm[64][3];
    const int i = blockIdx.x, lane = threadIdx.x;
    const EwSys& s = sys[gsys[i]];
    double fp[3] = {0.0, 0.0, 0.0};
    if (s.periodic) {
        const double inv_a = 1.0 / (sqrt(2.0) * sigma);
        const float* gi = out_r ? G + (int64_t)i * C : nullptr;
        const float* qi = out_r ? Q + (int64_t)i * C : nullptr;
        const double ui[3] = {(double)U[3 * (int64_t)i], (double)U[3 * (int64_t)i + 1], (double)U[3 * (int64_t)i + 2]};
        const int p1 = rowptr[i + 1];
        for (int p0 = rowptr[i]; p0 < p1; p0 += 64) {
            __syncthreads();
            const int p = p0 + lane;
            int j = i;
            double co = 0.0, m[3] = {0.0, 0.0, 0.0};
            if (p < p1) {
                j = nbr[p];
                const float4 g4 = geo[p];
                const double d = (double)g4.w;
                if (d < Rcut && j != i) {
                    const double x = d * inv_a, er = erf(x), der = 2.0 / sqrt(EW_PI) * inv_a * exp(-x * x), dder = -2.0 * x * inv_a * der;
                    const double cutf = 0.5 * (1.0 + cos(EW_PI * d / Rcut)), dcut = -0.5 * EW_PI / Rcut * sin(EW_PI * d / Rcut);
                    const double ddcut = -0.5 * (EW_PI / Rcut) * (EW_PI / Rcut) * cos(EW_PI * d / Rcut);
                    const double n0 = er * cutf, n1 = der * cutf + er * dcut, n2 = dder * cutf + 2.0 * der * dcut + er * ddcut;
                    const double dw = n1 / d - n0 / (d * d), ddw = n2 / d - 2.0 * n1 / (d * d) + 2.0 * n0 / (d * d * d);
                    const double n[3] = {(double)g4.x / d, (double)g4.y / d, (double)g4.z / d};
                    double e[3], nd = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        e[a] = (double)U[3 * (int64_t)j + a] - ui[a];
                        nd += n[a] * e[a];
                    }
                    co = -EW_PREFACTOR * dw * nd;
#pragma unroll
                    for (int a = 0; a < 3; a++) m[a] = EW_PREFACTOR * ((ddw - dw / d) * nd * n[a] + dw / d * e[a]);
                }
            }
            sj[lane] = j;
            sco[lane] = co;
            sm[lane][0] = m[0]; sm[lane][1] = m[1]; sm[lane][2] = m[2];
            __syncthreads();
            const int ne = min(64, p1 - p0);
            for (int q = 0; out_r && q < ne; q++) {
                const int jq = sj[q];
                if (jq == i) continue;
                const float* gj = G + (int64_t)jq * C;
                const float* qj = Q + (int64_t)jq * C;
                float b = 0.f, bp = 0.f;
                for (int c = lane; c < C; c += 64) {
                    b += gi[c] * qj[c];
                    bp += gj[c] * qi[c];
                }
                const double bb = (double)wsum(b) + (double)wsum(bp);
#pragma unroll
                for (int a = 0; a < 3; a++) fp[a] += bb * sm[q][a];
            }
            for (int c = lane; c < C; c += 64) {
                double ag = 0.0, aq = 0.0;
                for (int q = 0; q < ne; q++) {
                    const int64_t o = (int64_t)sj[q] * C + c;
                    if (out_g) ag += sco[q] * (double)Q[o];
                    if (out_q) aq += sco[q] * (double)G[o];
                }
                if (out_g) out_g[(int64_t)i * C + c] += (float)ag;
                if (out_q) out_q[(int64_t)i * C + c] += (float)aq;
            }
        }
    }
    if (out_r && lane < 3) out_r[3 * (int64_t)i + lane] += (float)((double)F2[3 * (int64_t)i + lane] + fp[lane]);
}

// ---- cell tangents of the second-order operation (pet_ewald_second_cell / pet_p3m_second_cell) ----------
// U = cell^{-1} u_c of one periodic system (fp64), u_c [3, 3] one row of d_u_cells
__device__ __forceinline__ void ew_cell_U(const double* inv, const float* uc, double* U) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            U[3 * a + b] = inv[3 * a] * (double)uc[b] + inv[3 * a + 1] * (double)uc[3 + b] + inv[3 * a + 2] * (double)uc[6 + b];
}

// u'_i = u_i - r_i U on the atoms of periodic systems (the direction that moves the fractional coordinates as (u, u_c) does),
// u_i elsewhere; formed in fp64 and rounded once. u may be null (zero).
__global__ __launch_bounds__(256) void k_ew_uprime(const float* __restrict__ pos, const int* __restrict__ gsys,
                                                   const EwSys* __restrict__ sys, const float* __restrict__ u,
                                                   const float* __restrict__ ucell, int N, float* __restrict__ up) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int si = gsys[i];
    const EwSys& s = sys[si];
    double v[3] = {0.0, 0.0, 0.0};
    if (u)
        for (int b = 0; b < 3; b++) v[b] = (double)u[3 * (int64_t)i + b];
    if (s.periodic) {
        double U[9];
        ew_cell_U(s.inv, ucell + 9 * (int64_t)si, U);
        const double r[3] = {(double)pos[3 * (int64_t)i], (double)pos[3 * (int64_t)i + 1], (double)pos[3 * (int64_t)i + 2]};
        for (int b = 0; b < 3; b++) v[b] -= r[0] * U[b] + r[1] * U[3 + b] + r[2] * U[6 + b];
    }
    for (int b = 0; b < 3; b++) up[3 * (int64_t)i + b] = (float)v[b];
}

// The local terms' share of (D A) X along (u, u_c), in place of k_ew_edge_second where there is a cell tangent: one wave per
// atom of a periodic system, fp64, the chunk walk of k_ew_edge_second. Per edge p = (i -> j, S), self-image edges included,
// the edge vector moves by dD = u_j - u_i + S u_c:  out_g[i] -= P w'(d) (n.dD) q_j,  out_q[i] -= P w'(d) (n.dD) g_j;  then the
// background, out_g[i] += P (2 pi sigma^2 / Omega) tr(U) sum_j q_j (sum_q, sum_g: k_ew_colsum of Q and of G). U may be null.
__global__ __launch_bounds__(64) void k_ew_edge_cell(const EwSys* __restrict__ sys, const int* __restrict__ gsys,
                                                     const int* __restrict__ rowptr, const int* __restrict__ nbr,
                                                     const int* __restrict__ shift, const float4* __restrict__ geo,
                                                     const float* __restrict__ G, const float* __restrict__ Q,
                                                     const float* __restrict__ U, const float* __restrict__ ucell,
                                                     const float* __restrict__ sum_q, const float* __restrict__ sum_g, int C,
                                                     double sigma, double Rcut, float* __restrict__ out_g,
                                                     float* __restrict__ out_q) {
    __shared__ int sj[64];
    __shared__ double sco[64];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int si = gsys[i];
    const EwSys& s = sys[si];
    if (!s.periodic) return;
    const float* uc = ucell + 9 * (int64_t)si;
    const double inv_a = 1.0 / (sqrt(2.0) * sigma);
    double ui[3] = {0.0, 0.0, 0.0};
    if (U)
        for (int a = 0; a < 3; a++) ui[a] = (double)U[3 * (int64_t)i + a];
    const int p1 = rowptr[i + 1];
    for (int p0 = rowptr[i]; p0 < p1; p0 += 64) {
        __syncthreads();
        const int p = p0 + lane;
        int j = i;
        double co = 0.0;
        if (p < p1) {
            j = nbr[p];
            const float4 g4 = geo[p];
            const double d = (double)g4.w;
            if (d < Rcut) {
                const double x = d * inv_a, er = erf(x), der = 2.0 / sqrt(EW_PI) * inv_a * exp(-x * x);
                const double cutf = 0.5 * (1.0 + cos(EW_PI * d / Rcut)), dcut = -0.5 * EW_PI / Rcut * sin(EW_PI * d / Rcut);
                const double n0 = er * cutf, n1 = der * cutf + er * dcut;
                const double dw = n1 / d - n0 / (d * d);
                const double n[3] = {(double)g4.x / d, (double)g4.y / d, (double)g4.z / d};
                double nd = 0.0;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    double e = U ? (double)U[3 * (int64_t)j + a] - ui[a] : 0.0;
#pragma unroll
                    for (int b = 0; b < 3; b++) e += (double)shift[3 * (int64_t)p + b] * (double)uc[3 * b + a];
                    nd += n[a] * e;
                }
                co = -EW_PREFACTOR * dw * nd;
            }
        }
        sj[lane] = j;
        sco[lane] = co;
        __syncthreads();
        const int ne = min(64, p1 - p0);
        for (int c = lane; c < C; c += 64) {
            double ag = 0.0, aq = 0.0;
            for (int q = 0; q < ne; q++) {
                const int64_t o = (int64_t)sj[q] * C + c;
                if (out_g) ag += sco[q] * (double)Q[o];
                if (out_q) aq += sco[q] * (double)G[o];
            }
            if (out_g) out_g[(int64_t)i * C + c] += (float)ag;
            if (out_q) out_q[(int64_t)i * C + c] += (float)aq;
        }
    }
    double Um[9];
    ew_cell_U(s.inv, uc, Um);
    const double bg = EW_PREFACTOR * 2.0 * EW_PI * sigma * sigma / s.vol * (Um[0] + Um[4] + Um[8]);
    for (int c = lane; c < C; c += 64) {
        if (out_g) out_g[(int64_t)i * C + c] += (float)(bg * (double)sum_q[(int64_t)si * C + c]);
        if (out_q) out_q[(int64_t)i * C + c] += (float)(bg * (double)sum_g[(int64_t)si * C + c]);
    }
}

}  // namespace

// P3M mode (csrc/p3m.hip): mesh descriptors and influence functions in place of k lists
struct P3mPlan;
void p3m_release(P3mPlan* p);
// reads every system's cell^{-1}, Omega, pbc and atom count from sys and leaves its range of reduction chunks in first_k / n_k
int p3m_plan_build(double sigma, double spacing, int nodes, const double* h_cells, std::vector<EwSys>& sys, P3mPlan** out);
// the mesh operator's half of the interface above (ewald.hip holds the other half and the `if` between them): a planned
// P3M-mode handle WITH a transform hook
int64_t p3m_workspace_bytes(const pet_ewald_t* e, int C, bool cell);
int p3m_potential(const LrCall& c, const float* X, float* out);
int p3m_backward(const LrCall& c, const float* Q, const float* G, float* gq, float* gpos);
int p3m_second(const LrCall& c, const float* Q, const float* G, const float* Uq, const float* Ur, const float* Ucell, float* out_q,
               float* out_g, float* out_r);

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
    // the caller's rfftn / irfftn between two offsets of the running entry point's workspace (pet_p3m_set_transform); kept
    // across plans. Without one a P3M-mode handle has no second-order entry and no place in the dual pass.
    int (*p3m_transform)(void*, int32_t, int64_t, int64_t, int32_t) = nullptr;
    void* p3m_transform_user = nullptr;
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

// What the four second-order entry points (`entry`: pet_ewald_second, pet_ewald_second_cell, pet_p3m_second,
// pet_p3m_second_cell) check before they run lr_second's half of their mode, in this order: the handle and its mode, the graph,
// the transform hook (`mesh`), the cotangents, an empty plan (PET_OK with *run false: nothing to launch, and zero-sized buffers
// may be null), the workspace, the inputs, the results (`no_results`: what to say where `results` is false).
int ew_second_check(const pet_ewald_t* e, const pet_graph_t* pg, int32_t C, const char* entry, bool mesh, bool cell, bool cotangent,
                    const void* ws, int64_t ws_bytes, bool inputs, bool results, const char* no_results, bool* run) {
    *run = false;
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    if (mesh)
        PET_REQUIRE(e->p3m_nodes != 0, PET_ERR_ARGUMENT,
                    "a pet_p3m_* entry point on an Ewald-mode handle: call pet_ewald_set_p3m before pet_ewald_plan");
    else
        PET_REQUIRE(e->p3m_nodes == 0, PET_ERR_ARGUMENT,
                    std::string(entry) + " on a P3M-mode handle (pet_ewald_set_p3m): the mesh operator's " +
                        (cell ? "cell tangents are pet_p3m_second_cell's" : "second derivatives are pet_p3m_second's"));
    PET_TRY(ew_check_graph(e, pg, C));
    PET_REQUIRE(!mesh || e->p3m_transform, PET_ERR_ARGUMENT,
                std::string(entry) + " on a P3M-mode handle without a transform hook: the mesh operator's second derivatives "
                "and its place in the dual pass need the caller's transforms (pet_p3m_set_transform)");
    PET_REQUIRE(cotangent, PET_ERR_ARGUMENT,
                cell ? "d_u_charges, d_u_positions and d_u_cells are all NULL" : "d_u_charges and d_u_positions are both NULL");
    if (e->n_atoms == 0) return PET_OK;
    PET_REQUIRE(ws && ws_bytes >= lr_workspace_bytes(e, C, cell), PET_ERR_ARGUMENT,
                std::string(mesh ? "P3M workspace missing or too small (" : "Ewald workspace too small (") + entry +
                    "_workspace_bytes)");
    PET_REQUIRE(inputs, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(results, PET_ERR_ARGUMENT, no_results);
    *run = true;
    return PET_OK;
}

// ---- the local terms, launched by both modes around their reciprocal-space part ------------------------------------------------
// Forward. out holds a mode's reciprocal-space sum on the atoms of periodic systems; this adds the rest of the operator on
// X [N, C]: the open all-pairs sum, then V <- P (V - self - background - exclusion), the column sums of X left in sums. The three
// coefficients of k_ew_finish (self sqrt(2 / pi) / sigma, background 2 pi sigma^2, 1 / a = 1 / (sqrt(2) sigma)) are formed HERE only.
int ew_local_forward(const pet_ewald_t* e, const Graph& g, const float* pos, const float* X, int C, float* out, float* sums,
                     hipStream_t st) {
    const unsigned cy = (unsigned)cdiv(C, 256);
    if (!e->atiles_n.empty())
        k_ew_pairs<false><<<dim3((unsigned)e->atiles_n.size(), cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos,
                                                                                 (float)(1.0 / e->cutoff), X, C, out, nullptr);
    k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, X, C, sums);
    k_ew_finish<<<cdiv(e->n_atoms, 4), 256, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.geo, X, sums, (int)e->n_atoms, C,
                                                     (float)(std::sqrt(2.0 / EW_PI) / e->sigma),
                                                     (float)(2.0 * EW_PI * e->sigma * e->sigma),
                                                     (float)(1.0 / (std::sqrt(2.0) * e->sigma)), (float)(1.0 / e->cutoff), out);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// whether k_ew_force may take its operands by 16-byte loads
inline bool ew_vec_loads(int C, const float* q, const float* g) {
    return C % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0;
}

// Workspace of the adjoint that both modes carve: F [N, 3] (a mode's reciprocal-space forces on periodic atoms, written before
// ew_local_backward), cell_part [N, 9], kpart [parts, 9] and the column sums of q and of dL/dV (read by k_ew_cell alone: the
// adjoint fills them where it has a cell gradient to form)
struct EwLocalWs {
    float *F, *cell_part, *sum_q, *sum_g;
    double* kpart;
};

// Adjoint. k_ew_force<false> on the open tiles (into w.F beside the caller's reciprocal-space forces), k_ew_edge_bwd (dL/dR, and
// the per-atom parts of dL/dcell), and with d_grad_cells: kspace_cell(), the caller's launch that fills w.kpart with its
// reciprocal-space parts, then k_ew_cell.
template <class KSpaceCell>
int ew_local_backward(const pet_ewald_t* e, const Graph& g, const float* pos, const float* Q, const float* G, int C,
                      const EwLocalWs& w, float* d_grad_positions, float* d_grad_cells, hipStream_t st, KSpaceCell kspace_cell) {
    if (!e->atiles_n.empty())
        k_ew_force<false><<<(unsigned)e->atiles_n.size(), 256, 0, st>>>(e->d_atiles_n, e->d_sys, nullptr, nullptr, 1, pos,
                                                                        (float)(1.0 / e->cutoff), G, Q, nullptr, nullptr, C,
                                                                        ew_vec_loads(C, Q, G), w.F);
    k_ew_edge_bwd<<<(unsigned)e->n_atoms, 64, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.shift, g.geo, pos, G, Q, w.F, C,
                                                       e->sigma, e->cutoff, d_grad_positions, d_grad_cells ? w.cell_part : nullptr);
    if (d_grad_cells) {
        kspace_cell();
        k_ew_cell<<<(unsigned)e->n_systems, 256, 0, st>>>(e->d_sys, w.cell_part, w.kpart, w.sum_g, w.sum_q, C, e->sigma, d_grad_cells);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// The cell tangent's local terms (section 23) ADDED to out_g / out_q (a null one is not formed): the column sums of Q / of G,
// then k_ew_edge_cell. U [N, 3] is the caller's position direction (may be null), not u'.
int ew_local_cell(const pet_ewald_t* e, const Graph& g, const float* Q, const float* G, const float* U, const float* ucell, int C,
                  const EwLocalWs& w, float* out_g, float* out_q, hipStream_t st) {
    const unsigned cy = (unsigned)cdiv(C, 256);
    if (out_g) k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, Q, C, w.sum_q);
    if (out_q) k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, G, C, w.sum_g);
    k_ew_edge_cell<<<(unsigned)e->n_atoms, 64, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.shift, g.geo, G, Q, U, ucell, w.sum_q,
                                                        w.sum_g, C, e->sigma, e->cutoff, out_g, out_q);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// the adjoint of a plan without atoms: nothing to launch, and dL/dcell (where asked for) is zeros
int ew_backward_empty(const pet_ewald_t* e, float* d_grad_cells, hipStream_t st) {
    if (d_grad_cells && e->n_systems > 0)
        PET_HIP_CHECK(hipMemsetAsync(d_grad_cells, 0, (size_t)e->n_systems * 9 * sizeof(float), st));
    return PET_OK;
}

}  // namespace

#endif  // LONG_RANGE_SHARED_PART
