// Last-layer prediction rigidity (LLPR, llpr/model.py): uncertainties and last-layer ensembles on the last-layer features.
//   features:   per-atom LLF [N, F] of every readout layer, F = 2 L d_head, columns node0 | edge0 | node1 | edge1 | ...
//               (pet/model.py:788-875): the heads of pet_predict, the edge part cutoff-weighted and summed per atom;
//   rows:       per-system sums of the LLF (evaluation rows) or sums / atom count (covariance rows, llpr/model.py:898-908),
//               optionally over selected atoms only; a two-stage fixed-order segmented reduction (slices, then their sum);
//   covariance: C64 += X^T X (llpr/model.py:912): fp32 MFMA partials of the upper-triangle 64x64 tiles over 256-row
//               chunks, added into the fp64 [F, F] buffer chunk by chunk in a fixed order (no atomics); finalize mirrors;
//   variance:   sigma_r = alpha sqrt(|M x_r|^2), M = L^-1 lower triangular (llpr/model.py:427-436): one [R, F] x [F, F]
//               product per 64-row tile with a square-and-row-sum epilogue, the tiles above M's diagonal skipped;
//   ensemble:   Y = X W^T, W [K P, F] member-major (index k P + p), then Y - mean_k Y + prediction (llpr/model.py:578-587).
// Every product is v_mfma_f32_16x16x4_f32 (fp32; gfx950 has no xf32). Every result is the same bits run to run.
#include <algorithm>
#include <vector>

#include "common.h"
#include "model.h"

namespace pet {

namespace {

constexpr int TT = 64;    // output tile (rows x cols) of one 256-thread block: 4 waves of 32 x 32
constexpr int KC = 32;    // k chunk staged in LDS by the NT products
constexpr int LDK = KC + 1;
constexpr int CR = 256;   // covariance rows per fp32 partial
constexpr int CSUB = 32;  // covariance rows staged at once
constexpr int LDC = TT + 4;
constexpr int COV_SLAB = 64;  // chunks per covariance launch (bounds the partial buffer)

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ inline f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// stage rows [r0, r0 + 64) x cols [k0, k0 + 32) of a row-major [nrows, ld] matrix into s[64][LDK], zero outside
__device__ inline void stage_rows(const float* __restrict__ A, int64_t ld, int64_t nrows, int64_t r0, int kend, int k0,
                                  float* s) {
    const int t = threadIdx.x, r = t >> 2, kq = (t & 3) * 8;
    const int64_t row = r0 + r;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int k = k0 + kq + j;
        s[r * LDK + kq + j] = (row < nrows && k < kend) ? A[row * ld + k] : 0.f;
    }
}

// acc[m][n] += Xs[wr 32 + m 16 ..][kk] * Bs[wc 32 + n 16 ..][kk] over the 32 staged k
__device__ inline void nt_chunk(const float* Xs, const float* Bs, f4 acc[2][2]) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
#pragma unroll
    for (int kk = 0; kk < KC / 4; kk++) {
        const int k = kk * 4 + (l >> 4);
        float a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; m++) a[m] = Xs[(wr * 32 + m * 16 + (l & 15)) * LDK + k];
#pragma unroll
        for (int n = 0; n < 2; n++) b[n] = Bs[(wc * 32 + n * 16 + (l & 15)) * LDK + k];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++) acc[m][n] = mfma4(a[m], b[n], acc[m][n]);
    }
}

}  // namespace

// ---- full last-layer features ---------------------------------------------------------------------------------------
// llf[i][col0 + c] = hn[i][c], llf[i][col0 + DH + c] = sum_{p in row i} fc[p] he[p][c] (CSR order)
__global__ void k_llpr_pack(const float* __restrict__ hn, const float* __restrict__ he, const float* __restrict__ fc,
                            const int* __restrict__ rowptr, int64_t N, int DH, int F, int col0, float* __restrict__ llf) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * DH) return;
    const int64_t i = t / DH;
    const int c = (int)(t % DH);
    llf[i * F + col0 + c] = hn[i * DH + c];
    float s = 0.f;
    if (he)
        for (int p = rowptr[i]; p < rowptr[i + 1]; p++) s += fc[p] * he[(int64_t)p * DH + c];
    llf[i * F + col0 + DH + c] = s;
}

__global__ void k_llpr_add(float* __restrict__ y, const float* __restrict__ x, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] += x[t];
}

int llpr_features(const Model& m, const Graph& g, const char* target, const char* block, const float* const* node_feats,
                  const float* const* edge_feats, int n_layers, float* atomic, float* llf, hipStream_t st) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    const int L = m.num_readout_layers(), DH = m.h.d_head, F = 2 * L * DH;
    PET_REQUIRE(n_layers == L, PET_ERR_ARGUMENT, "expected one feature pair per readout layer (" + std::to_string(L) + ")");
    if (N == 0) return PET_OK;
    std::vector<const HeadW*> H(L);
    std::vector<const LastW*> Lw(L);
    for (int l = 0; l < L; l++) {
        const std::string hk = std::string(target) + "|" + std::to_string(l);
        const auto hi = m.heads.find(hk);
        PET_REQUIRE(hi != m.heads.end(), PET_ERR_ARGUMENT, "no heads were uploaded for target '" + std::string(target) +
                                                               "', readout layer " + std::to_string(l));
        const auto li = m.lasts.find(hk + "|" + block);
        PET_REQUIRE(li != m.lasts.end(), PET_ERR_ARGUMENT, "no last layer was uploaded for block '" + std::string(block) + "'");
        H[l] = &hi->second;
        Lw[l] = &li->second;
        PET_REQUIRE(node_feats[l] && (edge_feats[l] || E == 0), PET_ERR_ARGUMENT, "null features of a readout layer");
    }
    const int P = Lw[0]->P;
    const int64_t Ea = E > 0 ? E : 1;
    const int64_t pred = predict_scratch_floats(N, E);
    PoolBuf buf;
    PET_HIP_CHECK(buf.alloc((size_t)(N * DH + Ea * DH + pred + N * P) * sizeof(float), st));
    float* hn = buf.as<float>();
    float* he = hn + N * DH;
    float* scratch = he + Ea * DH;
    float* atmp = scratch + pred;
    for (int l = 0; l < L; l++) {
        float* a = (atomic && l == 0) ? atomic : atmp;
        int rc = predict(m, g, *H[l], *Lw[l], node_feats[l], edge_feats[l], nullptr, a, hn, E > 0 ? he : nullptr, scratch, st);
        if (rc) return rc;
        if (atomic && l > 0) k_llpr_add<<<cdiv(N * P, 256), 256, 0, st>>>(atomic, atmp, N * P);
        k_llpr_pack<<<cdiv(N * DH, 256), 256, 0, st>>>(hn, E > 0 ? he : nullptr, g.fc, g.rowptr, N, DH, F, 2 * l * DH, llf);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---- per-system rows ------------------------------------------------------------------------------------------------
// Two fixed-order stages so that a few large systems still fill the machine. Stage 1, block (system s, 64 columns, part k):
// the k-th of `split` equal slices of the system's atoms; wave w sums atoms w, w + 4, ... of the slice in order (fp64), the
// four waves are added in wave order into part[s][k][c]. Stage 2: one thread per (s, c) adds the parts in k order; mean != 0
// divides by the system's atom count (every atom, selected or not: llpr/model.py:898-908). `split` is a function of (N, S)
// only, so a repeat gives the same bits.
__device__ inline int64_t first_atom_of(const int* __restrict__ sysidx, int64_t N, int key) {  // non-decreasing runs
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sysidx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_llpr_rows_part(const float* __restrict__ llf, int64_t N, int F, const int* __restrict__ sysidx,
                                 const uint8_t* __restrict__ mask, int split, double* __restrict__ part) {
    __shared__ double wsum[4][64];
    __shared__ int64_t range[2];
    const int s = blockIdx.x, k = blockIdx.z, w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (threadIdx.x < 2) range[threadIdx.x] = first_atom_of(sysidx, N, s + threadIdx.x);
    __syncthreads();
    const int64_t n = range[1] - range[0];
    const int64_t a0 = range[0] + n * k / split, a1 = range[0] + n * (k + 1) / split;
    const int c = blockIdx.y * 64 + l;
    double acc = 0.0;
    if (c < F)
        for (int64_t i = a0 + w; i < a1; i += 4)
            if (!mask || mask[i]) acc += (double)llf[i * F + c];
    wsum[w][l] = acc;
    __syncthreads();
    if (w == 0 && c < F) part[((int64_t)s * split + k) * F + c] = ((wsum[0][l] + wsum[1][l]) + wsum[2][l]) + wsum[3][l];
}

__global__ void k_llpr_rows_sum(const double* __restrict__ part, int64_t N, int64_t S, int F, const int* __restrict__ sysidx,
                                int split, int mean, float* __restrict__ rows) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S * F) return;
    const int64_t s = t / F;
    const int c = (int)(t % F);
    double v = 0.0;
    for (int k = 0; k < split; k++) v += part[(s * split + k) * F + c];
    if (mean) {
        const int64_t n = first_atom_of(sysidx, N, (int)s + 1) - first_atom_of(sysidx, N, (int)s);
        v = n > 0 ? v / (double)n : 0.0;
    }
    rows[t] = (float)v;
}

int llpr_rows(const float* llf, int64_t N, int F, const int* sysidx, int64_t S, const uint8_t* mask, int mean, float* rows,
              hipStream_t st) {
    if (S == 0) return PET_OK;
    // about 256 atoms per slice, at most 64 slices per system
    const int split = (int)std::max<int64_t>(1, std::min<int64_t>(64, N / (S * 256)));
    PoolBuf buf;
    PET_HIP_CHECK(buf.alloc((size_t)S * split * F * sizeof(double), st));
    double* part = buf.as<double>();
    k_llpr_rows_part<<<dim3((unsigned)S, (unsigned)cdiv(F, 64), (unsigned)split), 256, 0, st>>>(llf, N, F, sysidx, mask,
                                                                                                 split, part);
    k_llpr_rows_sum<<<cdiv(S * F, 256), 256, 0, st>>>(part, N, S, F, sysidx, split, mean, rows);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---- covariance -----------------------------------------------------------------------------------------------------
__device__ inline void tile_pair(int p, int nT, int& ti, int& tj) {
    ti = 0;
    while (p >= nT - ti) { p -= nT - ti; ti++; }
    tj = ti + p;
}

// block (pair of column tiles ti <= tj, chunk c): part[c][pair][a][b] = sum_{r in chunk} X[r][ti 64 + a] X[r][tj 64 + b]
__global__ __launch_bounds__(256) void k_llpr_cov_partial(const float* __restrict__ X, int64_t R, int F, int nT,
                                                          int64_t row0, float* __restrict__ part) {
    __shared__ float Xa[CSUB * LDC];
    __shared__ float Xb[CSUB * LDC];
    int ti, tj;
    tile_pair(blockIdx.x, nT, ti, tj);
    const int npairs = gridDim.x;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
    const int64_t rbase = row0 + (int64_t)blockIdx.y * CR;
    f4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = f4{0.f, 0.f, 0.f, 0.f};
    const int sr = t >> 3, sc = (t & 7) * 8;
    for (int sub = 0; sub < CR / CSUB; sub++) {
        const int64_t r = rbase + sub * CSUB + sr;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int ca = ti * TT + sc + j, cb = tj * TT + sc + j;
            Xa[sr * LDC + sc + j] = (r < R && ca < F) ? X[r * F + ca] : 0.f;
            Xb[sr * LDC + sc + j] = (r < R && cb < F) ? X[r * F + cb] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CSUB / 4; kk++) {
            const int k = kk * 4 + (l >> 4);
            float a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; m++) a[m] = Xa[k * LDC + wr * 32 + m * 16 + (l & 15)];
#pragma unroll
            for (int n = 0; n < 2; n++) b[n] = Xb[k * LDC + wc * 32 + n * 16 + (l & 15)];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int n = 0; n < 2; n++) acc[m][n] = mfma4(a[m], b[n], acc[m][n]);
        }
    }
    float* out = part + ((int64_t)blockIdx.y * npairs + blockIdx.x) * (TT * TT);
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int v = 0; v < 4; v++)
                out[(wr * 32 + m * 16 + (l >> 4) * 4 + v) * TT + wc * 32 + n * 16 + (l & 15)] = acc[m][n][v];
}

// C64[ti 64 + a][tj 64 + b] += sum over the slab's chunks in chunk order (fp64)
__global__ void k_llpr_cov_reduce(const float* __restrict__ part, int nchunks, int npairs, int nT, int F,
                                  double* __restrict__ C) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)npairs * TT * TT) return;
    const int p = (int)(t / (TT * TT)), e = (int)(t % (TT * TT));
    int ti, tj;
    tile_pair(p, nT, ti, tj);
    const int a = ti * TT + e / TT, b = tj * TT + e % TT;
    if (a >= F || b >= F) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; c++) s += (double)part[((int64_t)c * npairs + p) * (TT * TT) + e];
    C[(int64_t)a * F + b] += s;
}

__global__ void k_llpr_cov_mirror(double* __restrict__ C, int F) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)F * F) return;
    const int a = (int)(t / F), b = (int)(t % F);
    if (a > b) C[t] = C[(int64_t)b * F + a];
}

int llpr_covariance_accumulate(const float* X, int64_t R, int F, double* C, hipStream_t st) {
    if (R == 0) return PET_OK;
    const int nT = cdiv(F, TT), npairs = nT * (nT + 1) / 2;
    const int64_t chunks = (R + CR - 1) / CR;
    const int64_t slab = std::min<int64_t>(chunks, COV_SLAB);
    PoolBuf buf;
    PET_HIP_CHECK(buf.alloc((size_t)slab * npairs * TT * TT * sizeof(float), st));
    float* part = buf.as<float>();
    for (int64_t c0 = 0; c0 < chunks; c0 += COV_SLAB) {
        const int nc = (int)std::min<int64_t>(COV_SLAB, chunks - c0);
        k_llpr_cov_partial<<<dim3((unsigned)npairs, (unsigned)nc), 256, 0, st>>>(X, R, F, nT, c0 * CR, part);
        k_llpr_cov_reduce<<<cdiv((int64_t)npairs * TT * TT, 256), 256, 0, st>>>(part, nc, npairs, nT, F, C);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int llpr_covariance_finalize(double* C, int F, hipStream_t st) {
    k_llpr_cov_mirror<<<cdiv((int64_t)F * F, 256), 256, 0, st>>>(C, F);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---- variance -------------------------------------------------------------------------------------------------------
// block: rows [r0, r0 + 64); for each 64-row tile `it` of M: (X M^T)[r][i] over j < (it + 1) 64 (M[i][j] = 0 for j > i),
// squared and summed over i inside the tile (lanes, then the two column waves in order), added in fp64 in tile order
__global__ __launch_bounds__(256) void k_llpr_variance(const float* __restrict__ X, int64_t R, int F,
                                                       const float* __restrict__ M, float alpha, float* __restrict__ sigma) {
    __shared__ float Xs[TT * LDK];
    __shared__ float Ms[TT * LDK];
    __shared__ float red[2][TT];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
    const int64_t r0 = (int64_t)blockIdx.x * TT;
    double tot = 0.0;
    const int nT = (F + TT - 1) / TT;
    for (int it = 0; it < nT; it++) {
        f4 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++) acc[m][n] = f4{0.f, 0.f, 0.f, 0.f};
        const int jend = min(F, (it + 1) * TT);
        for (int k0 = 0; k0 < jend; k0 += KC) {
            __syncthreads();
            stage_rows(X, F, R, r0, jend, k0, Xs);
            stage_rows(M, F, F, (int64_t)it * TT, jend, k0, Ms);
            __syncthreads();
            nt_chunk(Xs, Ms, acc);
        }
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                float s = acc[m][0][v] * acc[m][0][v] + acc[m][1][v] * acc[m][1][v];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
                if ((l & 15) == 0) red[wc][wr * 32 + m * 16 + (l >> 4) * 4 + v] = s;
            }
        __syncthreads();
        if (t < TT) tot += (double)red[0][t] + (double)red[1][t];
    }
    if (t < TT && r0 + t < R) sigma[r0 + t] = alpha * (float)sqrt(tot);
}

int llpr_variance(const float* X, int64_t R, int F, const float* M, float alpha, float* sigma, hipStream_t st) {
    if (R == 0) return PET_OK;
    k_llpr_variance<<<cdiv(R, TT), 256, 0, st>>>(X, R, F, M, alpha, sigma);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---- ensemble -------------------------------------------------------------------------------------------------------
// Y[r][c] = sum_k X[r][k] W[c][k]: block tile 64 rows x 64 members
__global__ __launch_bounds__(256) void k_llpr_ens_gemm(const float* __restrict__ X, int64_t R, int F,
                                                       const float* __restrict__ W, int KP, float* __restrict__ Y) {
    __shared__ float Xs[TT * LDK];
    __shared__ float Ws[TT * LDK];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
    const int64_t r0 = (int64_t)blockIdx.x * TT;
    const int c0 = blockIdx.y * TT;
    f4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = f4{0.f, 0.f, 0.f, 0.f};
    // two levels: each 32-wide k chunk is summed from zero (8 chained products) and then added to the running total, so a
    // result is a chain of 8 + F / 32 roundings, not F / 4 -- at F = 288 .. 512 (SOAP-BPNN) the single chain
    // missed twice fp32 torch's own error
    for (int k0 = 0; k0 < F; k0 += KC) {
        __syncthreads();
        stage_rows(X, F, R, r0, F, k0, Xs);
        stage_rows(W, F, KP, c0, F, k0, Ws);
        __syncthreads();
        f4 part[2][2];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++) part[m][n] = f4{0.f, 0.f, 0.f, 0.f};
        nt_chunk(Xs, Ws, part);
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int n = 0; n < 2; n++) acc[m][n] += part[m][n];
    }
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int64_t r = r0 + wr * 32 + m * 16 + (l >> 4) * 4 + v;
                const int c = c0 + wc * 32 + n * 16 + (l & 15);
                if (r < R && c < KP) Y[r * KP + c] = acc[m][n][v];
            }
}

// one wave per (row r, property p): Y[r][k P + p] += pred[r][p] - mean_k Y[r][k P + p] (lane-strided fp64 sums, xor tree)
__global__ void k_llpr_ens_center(float* __restrict__ Y, int64_t R, int K, int P, const float* __restrict__ pred) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (q >= R * P) return;
    const int64_t r = q / P;
    const int p = (int)(q % P);
    float* y = Y + r * (int64_t)K * P + p;
    double s = 0.0;
    for (int k = l; k < K; k += 64) s += (double)y[(int64_t)k * P];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float shift = pred[r * P + p] - (float)(s / (double)K);
    for (int k = l; k < K; k += 64) y[(int64_t)k * P] += shift;
}

int llpr_ensemble(const float* X, int64_t R, int F, const float* W, int K, int P, const float* pred, float* Y, hipStream_t st) {
    if (R == 0) return PET_OK;
    const int KP = K * P;
    k_llpr_ens_gemm<<<dim3((unsigned)cdiv(R, TT), (unsigned)cdiv(KP, TT)), 256, 0, st>>>(X, R, F, W, KP, Y);
    if (pred) k_llpr_ens_center<<<cdiv(R * P, 4), 256, 0, st>>>(Y, R, K, P, pred);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace pet
