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
// Second derivatives (pet_ewald_second) are variants in the same form: k_ew_sfac<true> (the phase carries
// k.u_j), k_ew_gather<true> (the directional derivative, a contraction of twice the length), k_ew_force2 (the position Hessian
// applied to a direction: four product tiles per k tile, or M_K (u_j - u_i) for open systems), k_ew_pairs<true> and
// k_ew_edge_second (the exclusion rows, fp64); the <false> instantiations are the first-order kernels, bit for bit. k_ew_force2,
// k_ew_pairs and k_ew_edge_second are in long_range.h: pet_p3m_second launches them for the same local terms.
// Cell tangents (pet_ewald_second_cell): k_ew_uprime (long_range.h) turns (u, u_c) into the position
// direction u' that moves the phases alike, k_ew_wdot folds the weights' tangent into the weighted structure factors before
// the one k_ew_gather<true>, and ew_local_cell (k_ew_edge_cell) takes the place of k_ew_edge_second. New kernels and launches
// only: every instantiation above is what it was.
// Here: the k-space part (k_ew_tables, k_ew_sfac, k_ew_gather, k_ew_force<true>, k_ew_zk, the k list) and pet_ewald_*, among
// them the plan of both modes, and lr_* (the operator's interface of long_range.h, where the handle's mode is decided: the
// dual pass calls it, pet_ewald_* run its Ewald half). The handle, k_ew_force and the local terms' kernels are in
// long_range.h, shared with p3m.hip.
#define LONG_RANGE_SHARED_PART
#include "long_range.h"

namespace pet {

namespace {

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

// DIR: the structure factor weighted by the direction U [N, 3], S'_{uX} = w sum_j (k.u_j) X_j e^{i k.r_j} (pet_ewald_second):
// u of the chunk's 32 atoms is staged next to the tables, k is the row's
template <bool DIR>
__global__ __launch_bounds__(256) void k_ew_sfac(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                 const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                 const float* __restrict__ X, int C, float* __restrict__ S,
                                                 const float* __restrict__ U) {
    extern __shared__ float2 T[];
    __shared__ float4 us[DIR ? 32 : 1];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int kidx = tile.y + r;
    int n0 = 0, n1 = 0, n2 = 0;
    float kx = 0.f, ky = 0.f, kz = 0.f;
    if (kidx < s.n_k) {
        const EwK k = klist[s.first_k + kidx];
        n0 = k.n0; n1 = k.n1; n2 = k.n2;
        if (DIR) { kx = k.kx; ky = k.ky; kz = k.kz; }
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
        if (DIR && threadIdx.x < 32) {
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j0 + (int)threadIdx.x < s.n_atoms) {
                const float* p = U + 3 * (int64_t)(s.first_atom + j0 + threadIdx.x);
                u = make_float4(p[0], p[1], p[2], 0.f);
            }
            us[threadIdx.x] = u;
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int i = 0; i < 16; i++) re0[i] = im0[i] = re1[i] = im1[i] = 0.f;
#pragma unroll 4
        for (int s2 = 0; s2 < 16; s2++) {
            const int jj = 2 * s2 + half;
            float c, sn;
            ew_phase(T + jj * 3 * NM, NM, n0, n1, n2, c, sn);
            if (DIR) {
                const float4 u = us[jj];
                const float ku = kx * u.x + ky * u.y + kz * u.z;
                c *= ku; sn *= ku;
            }
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

// DIR: the directional derivative of the k-space sum along U [N, 3] (pet_ewald_second), ADDED to V with the prefactor:
//   V[i][c] -= P sum_k [ (c Im S'_{uX} - s Re S'_{uX}) - (k.u_i) (c Im S'_X - s Re S'_X) ],  S = S'_X, Su = S'_{uX}:
// the generated operand is (-s, c) against Su and -(k.u_i) (-s, c) against S, one contraction of twice the length
template <bool DIR>
__global__ __launch_bounds__(256) void k_ew_gather(const int2* __restrict__ tiles, const EwSys* __restrict__ sys,
                                                   const EwK* __restrict__ klist, const float2* __restrict__ tab, int NM,
                                                   const float* __restrict__ S, int C, float* __restrict__ V,
                                                   const float* __restrict__ Su, const float* __restrict__ U) {
    extern __shared__ float2 T[];
    __shared__ int4 kn[32];
    __shared__ float4 kv[DIR ? 32 : 1];
    const int2 tile = tiles[blockIdx.x];
    const EwSys s = sys[tile.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
    const int a0 = tile.y;
    ew_stage_tables(T, tab, NM, s.first_atom + a0, s.n_atoms - a0);
    const int c0 = blockIdx.y * 256 + wave * 64;
    const bool active = c0 < C;
    const bool in0 = c0 + r < C, in1 = c0 + 32 + r < C;
    const float2* Tr = T + r * 3 * NM;
    float3 ui = make_float3(0.f, 0.f, 0.f);
    if (DIR && a0 + r < s.n_atoms) {
        const float* p = U + 3 * (int64_t)(s.first_atom + a0 + r);
        ui = make_float3(p[0], p[1], p[2]);
    }
    // chunks of 32 k-vectors are summed on their own and then added to the totals; the plan lists a system's k-vectors by
    // descending |k|, so the small terms come first
    f32x16 v0, v1, t0, t1;
#pragma unroll
    for (int i = 0; i < 16; i++) t0[i] = t1[i] = 0.f;
    for (int k0 = 0; k0 < s.n_k; k0 += 32) {
        __syncthreads();
        if (threadIdx.x < 32) {
            int4 n = make_int4(0, 0, 0, 0);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + (int)threadIdx.x < s.n_k) {
                const EwK k = klist[s.first_k + k0 + threadIdx.x];
                n = make_int4(k.n0, k.n1, k.n2, 1);
                v = make_float4(k.kx, k.ky, k.kz, 0.f);
            }
            kn[threadIdx.x] = n;
            if (DIR) kv[threadIdx.x] = v;
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
            if (DIR) {
                const float* urow = Su + (int64_t)(s.first_k + k0 + kk) * 2 * C + c0 + r;
                const float ur0 = kin && in0 ? urow[0] : 0.f, ui0 = kin && in0 ? urow[C] : 0.f;
                const float ur1 = kin && in1 ? urow[32] : 0.f, ui1 = kin && in1 ? urow[C + 32] : 0.f;
                const float4 k = kv[kk];
                const float ku = k.x * ui.x + k.y * ui.y + k.z * ui.z;
                const float pr = ku * sn, pi = -ku * c;
                v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(-sn, ur0, v0, 0, 0, 0);
                v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, ui0, v0, 0, 0, 0);
                v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pr, br0, v0, 0, 0, 0);
                v0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pi, bi0, v0, 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(-sn, ur1, v1, 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c, ui1, v1, 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pr, br1, v1, 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pi, bi1, v1, 0, 0, 0);
                continue;
            }
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
        if (DIR) {
            if (in0) o[0] -= (float)EW_PREFACTOR * t0[i];
            if (in1) o[32] -= (float)EW_PREFACTOR * t1[i];
            continue;
        }
        if (in0) o[0] = t0[i];
        if (in1) o[32] = t1[i];
    }
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

// The weights' share of the cell tangent (pet_ewald_second_cell), folded into the weighted structure factor that k_ew_gather<true>
// reads: with f_k = w_k' / w_k = (sigma^2 + 2 / k^2) (k U k^T) - tr U along u_c (U = cell^{-1} u_c; fp64 from the integer triple
// and the plan's inverse cell, rounded once), Su[k] += f_k (Im S'[k], -Re S'[k]), which that gather turns into
// + P sum_k f_k Re(e^{-i k.r_i} S'_X(k)). One block per k-vector, threads over channels.
__global__ __launch_bounds__(256) void k_ew_wdot(const EwSys* __restrict__ sys, const int* __restrict__ ksys,
                                                 const EwK* __restrict__ klist, const float* __restrict__ ucell,
                                                 const float* __restrict__ S, int C, double sigma, float* __restrict__ Su) {
    __shared__ float fs;
    const int64_t k = blockIdx.x;
    if (threadIdx.x == 0) {
        const int si = ksys[k];
        const EwSys& s = sys[si];
        const EwK kk = klist[k];
        double U[9], kv[3], k2 = 0.0, kuk = 0.0;
        ew_cell_U(s.inv, ucell + 9 * (int64_t)si, U);
        for (int a = 0; a < 3; a++) {
            kv[a] = 2.0 * EW_PI * (s.inv[3 * a] * kk.n0 + s.inv[3 * a + 1] * kk.n1 + s.inv[3 * a + 2] * kk.n2);
            k2 += kv[a] * kv[a];
        }
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) kuk += kv[a] * U[3 * a + b] * kv[b];
        fs = (float)((sigma * sigma + 2.0 / k2) * kuk - (U[0] + U[4] + U[8]));
    }
    __syncthreads();
    const float f = fs;
    const float* re = S + k * 2 * C;
    float* ure = Su + k * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float a = re[c], b = re[C + c];
        ure[c] += f * b;
        ure[C + c] -= f * a;
    }
}

// the largest reciprocal index along every axis of a cell inside |k| <= 2 pi / lambda; false where one is beyond 1e6
bool ew_index_bounds(const double* h, double lambda, int* nmax) {
    const double kmax = 2.0 * EW_PI / lambda;
    for (int a = 0; a < 3; a++) {
        const double len = std::sqrt(h[3 * a] * h[3 * a] + h[3 * a + 1] * h[3 * a + 1] + h[3 * a + 2] * h[3 * a + 2]);
        const double m = std::floor(kmax * len / (2.0 * EW_PI) + 1e-9);
        if (m > 1e6) return false;
        nmax[a] = (int)m;
    }
    return true;
}

// the walked half of the k-set of one cell (inv = cell^{-1}): n inside the bounds with the first non-zero index positive,
// 0 < |k| <= kmax; the weights are the plan's
void ew_half_kset(const double* inv, double lambda, const int* nmax, std::vector<EwK>& out) {
    const double kmax = 2.0 * EW_PI / lambda;
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
                out.push_back(e);
            }
}

// The per-system part of a plan that both modes share: pbc, the atom range and, for a periodic system, cell^{-1} and Omega
int ew_plan_system(int64_t s, const double* h_cell, const int32_t* h_pbc, int64_t a0, int64_t a1, EwSys& y) {
    PET_REQUIRE(a1 >= a0 && a1 < (int64_t(1) << 30), PET_ERR_ARGUMENT, "h_first_atom must be non-decreasing");
    const int np = (h_pbc[0] != 0) + (h_pbc[1] != 0) + (h_pbc[2] != 0);
    PET_REQUIRE(np == 0 || np == 3, PET_ERR_UNSUPPORTED,
                "long range with mixed pbc (system " + std::to_string(s) + "): only fully periodic and fully open "
                "systems are served (the reference refuses 1D and leaves 2D to torch-pme)");
    for (int k = 0; k < 9; k++) y.inv[k] = 0.0;
    y.vol = 1.0;
    y.periodic = np == 3;
    y.first_atom = (int)a0;
    y.n_atoms = (int)(a1 - a0);
    y.first_k = y.n_k = 0;  // (the mode's part of the plan fills them)
    y.nm = 1;
    PET_REQUIRE(!y.periodic || ew_cell_inverse(h_cell, y.inv, &y.vol), PET_ERR_ARGUMENT,
                "the cell of periodic system " + std::to_string(s) + " is singular");
    return PET_OK;
}

// Ewald mode: the k list of periodic system s appended to ks (with its system per entry and its tiles of 32), after the
// index limit has been checked on the bounds alone
int ew_plan_klist(const pet_ewald_t* e, int64_t s, const double* h_cell, EwSys& y, std::vector<EwK>& ks, std::vector<int>& ksys,
                  std::vector<int2>& ktiles) {
    int nmax[3];
    const bool bounded = ew_index_bounds(h_cell, e->lambda, nmax);
    if (bounded) y.nm = std::max(nmax[0], std::max(nmax[1], nmax[2])) + 1;
    PET_REQUIRE(bounded && y.nm - 1 <= PET_EWALD_MAX_INDEX, PET_ERR_UNSUPPORTED,
                "system " + std::to_string(s) + " needs reciprocal indices up to " + std::to_string(y.nm - 1) +
                    " at this kspace_resolution; at most " + std::to_string(PET_EWALD_MAX_INDEX) +
                    " are served (the Ewald sum costs O(N K): large boxes are what P3M is for: pet_ewald_set_p3m)");
    const size_t before = ks.size();  // (= y.first_k)
    ew_half_kset(y.inv, e->lambda, nmax, ks);
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
    for (int k0 = 0; k0 < y.n_k; k0 += 32) ktiles.push_back(make_int2((int)s, k0));
    return PET_OK;
}

// the workspace: the per-atom phase tables, S'(q) and S'(dL/dV), and what the local terms' adjoint asks for
struct EwWs {
    float2* tab;
    float *S1, *S2;
    EwLocalWs loc;
};

size_t ew_carve(const pet_ewald_t* e, int64_t C, void* base, EwWs& w) {
    Carver c(base);
    const size_t N = (size_t)std::max<int64_t>(e->n_atoms, 1), K = (size_t)std::max<int64_t>(e->n_k, 1);
    const size_t S = (size_t)std::max<int64_t>(e->n_systems, 1);
    w.tab = c.take<float2>(N * 3 * e->nm);
    w.S1 = c.take<float>(K * 2 * C);
    w.S2 = c.take<float>(K * 2 * C);
    w.loc.sum_q = c.take<float>(S * C);
    w.loc.sum_g = c.take<float>(S * C);
    w.loc.F = c.take<float>(N * 3);
    w.loc.cell_part = c.take<float>(N * 9);
    w.loc.kpart = c.take<double>(K * 9);
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
        k_ew_sfac<false><<<dim3((unsigned)e->ktiles.size(), cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, X, C,
                                                                                 Sbuf, nullptr);
    if (!e->atiles_p.empty())
        k_ew_gather<false><<<dim3((unsigned)e->atiles_p.size(), cy), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm,
                                                                                   Sbuf, C, out, nullptr, nullptr);
    return ew_local_forward(e, g, pos, X, C, out, sums, st);
}

// the workspace of the second-order operation: that of the first-order entry points, then S'(u_q) and the two weighted
// structure factors, then (cell: pet_ewald_second_cell) u' [N, 3]
struct EwWs2 {
    EwWs w;
    float *S3, *Su1, *Su2;
    float* up;
};

size_t ew_carve2(const pet_ewald_t* e, int64_t C, void* base, EwWs2& w2, bool cell) {
    Carver c(base);
    c.off = ew_carve(e, C, base, w2.w);
    const size_t K = (size_t)std::max<int64_t>(e->n_k, 1);
    w2.S3 = c.take<float>(K * 2 * C);
    w2.Su1 = c.take<float>(K * 2 * C);
    w2.Su2 = c.take<float>(K * 2 * C);
    w2.up = cell ? c.take<float>((size_t)std::max<int64_t>(e->n_atoms, 1) * 3) : nullptr;
    return c.off;
}

// ---- the Ewald sum's half of the interface (long_range.h). Every call rebuilds the phase tables (positions do not change inside
// a sweep of the dual pass, but the tables are a fraction of one structure-factor launch). The first-order pair touches the
// first-order workspace alone, which every workspace of this mode begins with.
// out = A X
int ew_potential(const LrCall& c, const float* X, float* out) {
    EwWs w;
    ew_carve(c.e, c.C, c.ws, w);
    ProfScope ps("ewald_fwd", c.st, 0.0, 0.0);
    PET_TRY(ew_tables(c.e, *c.g, c.pos, w, c.st));
    return ew_apply(c.e, *c.g, c.pos, X, c.C, out, w, w.S1, w.loc.sum_q, c.st);
}

// gq = A G, gpos = grad_r Phi(r; G, Q) and, with gcell, dL/dcell: the column sums of Q and the k-vectors' parts (k_ew_zk) are
// the cell gradient's alone
int ew_backward(const LrCall& c, const float* Q, const float* G, float* gq, float* gpos, float* gcell) {
    const pet_ewald_t* e = c.e;
    const int C = c.C;
    hipStream_t st = c.st;
    EwWs w;
    ew_carve(e, C, c.ws, w);
    ProfScope ps("ewald_bwd", st, 0.0, 0.0);
    PET_TRY(ew_tables(e, *c.g, c.pos, w, st));
    // dL/dq = the operator applied to g: leaves S'(g) in S2 and the column sums of g in sum_g
    PET_TRY(ew_apply(e, *c.g, c.pos, G, C, gq, w, w.S2, w.loc.sum_g, st));
    const unsigned cy = (unsigned)cdiv(C, 256);
    const size_t lds = ew_table_lds(e);
    if (!e->ktiles.empty())
        k_ew_sfac<false><<<dim3((unsigned)e->ktiles.size(), cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, Q, C,
                                                                                 w.S1, nullptr);
    if (gcell) k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, Q, C, w.loc.sum_q);
    if (!e->atiles_p.empty())
        k_ew_force<true><<<(unsigned)e->atiles_p.size(), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, c.pos,
                                                                         (float)(1.0 / e->cutoff), G, Q, w.S1, w.S2, C,
                                                                         ew_vec_loads(C, Q, G), w.loc.F);
    return ew_local_backward(e, *c.g, c.pos, Q, G, C, w.loc, gpos, gcell, st, [&] {
        if (e->n_k > 0)
            k_ew_zk<<<cdiv(e->n_k, 4), 256, 0, st>>>(e->d_sys, e->d_ksys, e->d_k, w.S1, w.S2, C, (int)e->n_k, e->sigma, w.loc.kpart);
    });
}

// The second-order operation with selectable results: a null out_q / out_g / out_r is not formed and the launches that serve it
// alone are skipped. With all three it is the launch list pet_ewald_second always had. Q may be null where only out_q is asked
// for (it is a function of (G, Ur) alone), G where only out_g is (a function of (Q, Uq, Ur)).
// With Ucell (pet_ewald_second_cell; no out_r): the position direction becomes u' = u - r U (k_ew_uprime), k_ew_wdot folds the
// weights' tangent into the two weighted structure factors and ew_local_cell takes the place of k_ew_edge_second; nothing
// else differs.
int ew_second(const LrCall& c, const float* Q, const float* G, const float* Uq, const float* U, const float* Ucell, float* out_q,
              float* out_g, float* out_r) {
    const pet_ewald_t* e = c.e;
    const Graph& g = *c.g;
    const float* pos = c.pos;
    const int C = c.C;
    hipStream_t st = c.st;
    EwWs2 w2;
    ew_carve2(e, C, c.ws, w2, Ucell != nullptr);
    const EwWs& w = w2.w;
    const int64_t N = e->n_atoms;
    const unsigned cy = (unsigned)cdiv(C, 256), nk = (unsigned)e->ktiles.size(), np = (unsigned)e->atiles_p.size(),
                   nn = (unsigned)e->atiles_n.size();
    const size_t lds = ew_table_lds(e);
    const float inv_R = (float)(1.0 / e->cutoff);
    const float* Ur = U;  // the direction of the position tangent: the caller's, or u' under a cell tangent
    if (Ucell) {
        k_ew_uprime<<<cdiv(N, 256), 256, 0, st>>>(pos, g.sys, e->d_sys, U, Ucell, (int)N, w2.up);
        Ur = w2.up;
    }
    // (the profiler's stage names tell the selections apart: all three results, the dual forward's, the two reverses')
    ProfScope ps(Ucell ? (out_g && out_q ? "ewald_second_cell" : out_g ? "ewald_second_cell_g" : "ewald_second_cell_q")
                 : out_q && out_g && out_r ? "ewald_second" : out_g ? "ewald_second_g" : out_r ? "ewald_second_qr" : "ewald_second_q",
                 st, 0.0, 0.0);
    PET_TRY(ew_tables(e, g, pos, w, st));
    // S'(g) serves out_r of both halves and out_q
    if (nk && (out_r || (out_q && Ur)))
        k_ew_sfac<false><<<dim3(nk, cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, G, C, w.S2, nullptr);
    if (Uq) {
        // out_g = A u_q (leaves S'(u_q) in S3), out_r = grad_r Phi(r; u_q, g): the first-order adjoint with (g, q) := (u_q, g)
        if (out_g) PET_TRY(ew_apply(e, g, pos, Uq, C, out_g, w, w2.S3, w.loc.sum_g, st));
        else if (out_r && nk)
            k_ew_sfac<false><<<dim3(nk, cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, Uq, C, w2.S3, nullptr);
        if (out_r) {
            if (np)
                k_ew_force<true><<<np, 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, pos, inv_R, Uq, G, w.S2, w2.S3,
                                                       C, ew_vec_loads(C, G, Uq), w.loc.F);
            PET_TRY(ew_local_backward(e, g, pos, G, Uq, C, w.loc, out_r, nullptr, st, [] {}));
        }
    } else {
        if (out_g) PET_HIP_CHECK(hipMemsetAsync(out_g, 0, (size_t)N * C * sizeof(float), st));
        if (out_r) PET_HIP_CHECK(hipMemsetAsync(out_r, 0, (size_t)N * 3 * sizeof(float), st));
    }
    if (out_q) PET_HIP_CHECK(hipMemsetAsync(out_q, 0, (size_t)N * C * sizeof(float), st));
    if (Ur) {
        // out_g += (D_u A) q, out_q = (D_u A) g, out_r += H u_r: k-space and open parts, then the exclusion rows
        if (nk) {
            if (out_g || out_r) {
                k_ew_sfac<false><<<dim3(nk, cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, Q, C, w.S1, nullptr);
                k_ew_sfac<true><<<dim3(nk, cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, Q, C, w2.Su1, Ur);
            }
            if (out_q || out_r)
                k_ew_sfac<true><<<dim3(nk, cy), 256, lds, st>>>(e->d_ktiles, e->d_sys, e->d_k, w.tab, e->nm, G, C, w2.Su2, Ur);
            if (Ucell && out_g) k_ew_wdot<<<(unsigned)e->n_k, 256, 0, st>>>(e->d_sys, e->d_ksys, e->d_k, Ucell, w.S1, C, e->sigma, w2.Su1);
            if (Ucell && out_q) k_ew_wdot<<<(unsigned)e->n_k, 256, 0, st>>>(e->d_sys, e->d_ksys, e->d_k, Ucell, w.S2, C, e->sigma, w2.Su2);
        }
        if (np) {
            if (out_g)
                k_ew_gather<true><<<dim3(np, cy), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, w.S1, C, out_g,
                                                                  w2.Su1, Ur);
            if (out_q)
                k_ew_gather<true><<<dim3(np, cy), 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, w.S2, C, out_q,
                                                                  w2.Su2, Ur);
            if (out_r)
                k_ew_force2<true><<<np, 256, lds, st>>>(e->d_atiles_p, e->d_sys, e->d_k, w.tab, e->nm, pos, inv_R, G, Q, w.S1, w.S2,
                                                        w2.Su1, w2.Su2, Ur, C, ew_vec_loads(C, Q, G), w.loc.F);
        }
        if (nn) {
            if (out_g) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, Q, C, out_g, Ur);
            if (out_q) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, G, C, out_q, Ur);
            if (out_r)
                k_ew_force2<false><<<nn, 256, 0, st>>>(e->d_atiles_n, e->d_sys, nullptr, nullptr, 1, pos, inv_R, G, Q, nullptr, nullptr,
                                                       nullptr, nullptr, Ur, C, ew_vec_loads(C, Q, G), w.loc.F);
        }
        if (Ucell) PET_TRY(ew_local_cell(e, g, Q, G, U, Ucell, C, w.loc, out_g, out_q, st));
        else
            k_ew_edge_second<<<(unsigned)N, 64, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.geo, G, Q, Ur, w.loc.F, C, e->sigma,
                                                         e->cutoff, out_g, out_q, out_r);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// the context of an extern "C" entry point's own call: its d_workspace is the operator's
LrCall ew_entry_call(const pet_ewald_t* e, const pet_graph_t* pg, const float* pos, int C, void* ws, void* stream) {
    return LrCall{e, &pg->g, pos, C, ws, 0, (hipStream_t)stream};
}

}  // namespace

// ---- the interface (long_range.h): the handle's mode is decided here and nowhere else --------------------------------------------
int lr_check(const pet_ewald_t* e, const pet_graph_t* pg, int C, const char* who) {
    PET_REQUIRE(e && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes == 0 || e->p3m_transform, PET_ERR_UNSUPPORTED,
                std::string(who) + " on a P3M-mode handle (pet_ewald_set_p3m) without a transform hook: second derivatives "
                "through P3M need the caller's transforms (pet_p3m_set_transform)");
    return ew_check_graph(e, pg, C);
}

int64_t lr_workspace_bytes(const pet_ewald_t* e, int C, bool cell) {
    if (e->p3m_nodes) return p3m_workspace_bytes(e, C, cell);
    EwWs2 w;
    return (int64_t)ew_carve2(e, C, nullptr, w, cell);
}

int lr_potential(const LrCall& c, const float* X, float* out) {
    if (c.e->p3m_nodes) return p3m_potential(c, X, out);
    return ew_potential(c, X, out);
}

int lr_backward(const LrCall& c, const float* Q, const float* G, float* gq, float* gpos, float* gcell) {
    if (!c.e->p3m_nodes) return ew_backward(c, Q, G, gq, gpos, gcell);
    PET_REQUIRE(!gcell, PET_ERR_UNSUPPORTED,
                "dL/dcell of the mesh operator inside an entry point is not built: it needs the unfiltered spectra of q and of "
                "dL/dV, which the staged entry point pet_p3m_backward is given");
    return p3m_backward(c, Q, G, gq, gpos);
}

int lr_second(const LrCall& c, const float* Q, const float* G, const float* Uq, const float* Ur, const float* Ucell, float* out_q,
              float* out_g, float* out_r) {
    PET_REQUIRE(!(Ucell && out_r), PET_ERR_UNSUPPORTED,
                "the position result of the second-order operation under a cell tangent (mixed position / cell second "
                "derivatives) is not built");
    if (c.e->p3m_nodes) return p3m_second(c, Q, G, Uq, Ur, Ucell, out_q, out_g, out_r);
    return ew_second(c, Q, G, Uq, Ur, Ucell, out_q, out_g, out_r);
}

}  // namespace pet

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
    int nmax[3];
    std::vector<EwK> half;
    if (!ew_cell_inverse(h_cell, inv, &vol) || !ew_index_bounds(h_cell, kspace_resolution, nmax)) return -1;
    ew_half_kset(inv, kspace_resolution, nmax, half);
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
        PET_TRY(ew_plan_system(s, h_cells + 9 * s, h_pbc + 3 * s, h_first_atom[s], h_first_atom[s + 1], y));
        y.first_k = (int)ks.size();
        if (y.periodic && !e->p3m_nodes) {
            PET_TRY(ew_plan_klist(e, s, h_cells + 9 * s, y, ks, ksys, ktiles));
            nm_all = std::max(nm_all, y.nm);
        }
        for (int a = 0; a < y.n_atoms; a += 32) (y.periodic ? ap : an).push_back(make_int2((int)s, a));
    }
    PET_REQUIRE(ks.size() < (size_t(1) << 28), PET_ERR_UNSUPPORTED, "too many k-vectors in one batch");
    // P3M mode: meshes and influence functions in place of the k lists, and no limit on a cell's length
    P3mPlan* mesh_plan = nullptr;
    if (e->p3m_nodes) PET_TRY(p3m_plan_build(e->sigma, e->lambda, e->p3m_nodes, h_cells, sys, &mesh_plan));
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
    return ew_potential(ew_entry_call(e, pg, d_positions, C, d_workspace, stream), d_charges, d_potential);
}

int pet_ewald_backward(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                       const float* d_grad_potential, int32_t C, float* d_grad_charges, float* d_grad_positions,
                       float* d_grad_cells, void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = ew_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    if (e->n_atoms == 0) return ew_backward_empty(e, d_grad_cells, (hipStream_t)stream);
    PET_REQUIRE(d_positions && d_charges && d_grad_potential && d_grad_charges && d_grad_positions, PET_ERR_ARGUMENT,
                "null argument");
    return ew_backward(ew_entry_call(e, pg, d_positions, C, d_workspace, stream), d_charges, d_grad_potential, d_grad_charges,
                       d_grad_positions, d_grad_cells);
}

int64_t pet_ewald_second_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || e->p3m_nodes || n_channels < 1) return -1;
    return lr_workspace_bytes(e, (int)n_channels, false);
}

int pet_ewald_second(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                     const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions, int32_t C,
                     float* d_out_charges, float* d_out_grad_potential, float* d_out_positions, void* d_workspace,
                     int64_t workspace_bytes, void* stream) {
    bool run;
    PET_TRY(ew_second_check(e, pg, C, "pet_ewald_second", false, false, d_u_charges || d_u_positions, d_workspace, workspace_bytes,
                            d_positions && d_charges && d_grad_potential,
                            d_out_charges && d_out_grad_potential && d_out_positions, "null argument", &run));
    if (!run) return PET_OK;
    return ew_second(ew_entry_call(e, pg, d_positions, C, d_workspace, stream), d_charges, d_grad_potential, d_u_charges,
                     d_u_positions, nullptr, d_out_charges, d_out_grad_potential, d_out_positions);
}

int64_t pet_ewald_second_cell_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || e->p3m_nodes || n_channels < 1) return -1;
    return lr_workspace_bytes(e, (int)n_channels, true);
}

int pet_ewald_second_cell(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                          const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions,
                          const float* d_u_cells, int32_t C, float* d_out_charges, float* d_out_grad_potential, void* d_workspace,
                          int64_t workspace_bytes, void* stream) {
    bool run;
    PET_TRY(ew_second_check(e, pg, C, "pet_ewald_second_cell", false, true, d_u_charges || d_u_positions || d_u_cells, d_workspace,
                            workspace_bytes, d_positions && d_charges && d_grad_potential, d_out_charges || d_out_grad_potential,
                            "both results are NULL", &run));
    if (!run) return PET_OK;
    return ew_second(ew_entry_call(e, pg, d_positions, C, d_workspace, stream), d_charges, d_grad_potential, d_u_charges,
                     d_u_positions, d_u_cells, d_out_charges, d_out_grad_potential, nullptr);
}

}  // extern "C"
