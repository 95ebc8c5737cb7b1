// P3M (particle-particle particle-mesh) evaluation of the long-range operator's reciprocal-space sum: the second implementation
// of the k-space term of ewald.hip, O(N p^3 C + M log M) where the Ewald sum costs O(N K C). The definition, the convention
// table and the adjoints are in include/pet_hip.h (block pet_p3m_*) and DESIGN.md section 19. The self, background, exclusion
// and open-system terms, their adjoints and the handle are those of long_range.h, which this file shares with ewald.hip.
// Stages (the transforms between them are the caller's: torch.fft on the same stream, no second FFT library in this one):
//   pet_p3m_spread   k_p3m_bin_* (weights [N,3,p] in fp64 from wrapped fractional coordinates, rounded once; a stable counting
//                    sort of the atoms by the mesh cell of their stencil origin) and k_p3m_spread in owner-computes form
//   pet_p3m_filter   k_p3m_filter: half spectrum times G^/Omega (k_p3m_influence at plan time, fp64 -> fp32)
//   pet_p3m_finish   k_p3m_gather, then ew_local_forward (k_ew_pairs / k_ew_colsum / k_ew_finish)
//   pet_p3m_backward k_p3m_force, then ew_local_backward (k_ew_force<false>, k_ew_edge_bwd, k_ew_cell) with k_p3m_cell before k_ew_cell
// Second order (pet_p3m_second) and the dual pass (the mesh operator's half of long_range.h's interface:
// p3m_potential / p3m_backward / p3m_second) run the whole operator inside ONE call: the
// transforms come back through the handle's hook (pet_p3m_set_transform), between a mesh and a half spectrum inside the call's
// own workspace. k_p3m_spread2 / k_p3m_gather2 / k_p3m_force2 are the three mesh kernels with the tangent and Hessian weights
// beside the plain ones; the local terms are long_range.h's (k_ew_pairs<true>, k_ew_force2<false>, k_ew_edge_second).
// Cell tangents (pet_p3m_second_cell): the position tangent at u' (k_ew_uprime), and the filter's tangent
// K' = sum_bc d(G^/Omega)/dcell_bc u_c,bc (k_p3m_gdot) applied to the spectrum that p3m_solve has in hand anyway
// (k_p3m_filter_dot keeps it aside, k_p3m_spec_add adds it to the mesh the tangent gather reads): no transform is added.
// Layout. CHANNEL-FIRST: the mesh of a system is [C, N_x, N_y, N_z] (z fastest), its half spectrum [C, N_x, N_y, N_z/2 + 1]
// complex; the meshes of a batch's periodic, non-empty systems are packed one after another (system s starts at mesh_off_s * C).
// The transforms run over contiguous planes with batch stride M and need no copy; the price is on this side: k_p3m_spread owns
// mesh points with lanes over POINTS (coalesced stores, the bin walk repeated per chunk of 8 channels) and k_p3m_gather /
// k_p3m_force read one mesh row per lane (lanes over channels, stride M).
// Order. A mesh point walks its p^3 origin bins in (t_x, t_y, t_z) order and a bin's atoms in atom order; an atom walks its
// p^3 nodes in the same order; channels are reduced by the butterfly of k_ew_force; per-point parts of dL/dcell are reduced per
// chunk of 1024 half-spectrum points by a fixed tree and then in chunk order (k_ew_cell). The only atomics are integer counters
// of the counting sort, whose result (a bin's atoms in atom order, after k_p3m_bin_sort) does not depend on their order.
#define LONG_RANGE_SHARED_PART
#include "long_range.h"

namespace pet {

constexpr int P3M_MAX_AXIS = PET_P3M_MAX_AXIS;
constexpr int P3M_CHUNK = 1024;  // half-spectrum points per reduction chunk of k_p3m_cell (and per block of k_p3m_filter)
constexpr int P3M_CH = 8;        // channels a thread of k_p3m_spread carries through one bin walk

struct P3mSysD {
    int n[3];
    int nzh;        // N_z / 2 + 1
    int64_t moff;   // first mesh point of this system in the packed batch (points, not floats)
    int64_t soff;   // first half-spectrum point
    double inv[9];  // cell^{-1}, as EwSys
    double vol;
};

struct P3mPlan {
    std::vector<P3mSysD> sys;
    std::vector<int2> mtiles, stiles;  // (system, first point) per 256 mesh points / per P3M_CHUNK half-spectrum points
    int64_t m_total = 0, s_total = 0;
    P3mSysD* d_sys = nullptr;
    int2 *d_mtiles = nullptr, *d_stiles = nullptr;
    float* d_infl = nullptr;  // G^/Omega per half-spectrum point
};

void p3m_release(P3mPlan* p) {
    if (!p) return;
    (void)hipFree(p->d_sys); (void)hipFree(p->d_mtiles); (void)hipFree(p->d_stiles); (void)hipFree(p->d_infl);
    delete p;
}

namespace {

// ---- the definition's scalar pieces, shared by host and device -------------------------------------------------------------
__host__ __device__ inline int p3m_pow2_at_least(double ratio) {
    int n = 1;
    while ((double)n < ratio && n < (1 << 20)) n *= 2;
    return n;
}

// N_a = the smallest power of two >= |cell row a| / spacing (at least 1)
__host__ __device__ inline void p3m_mesh_shape(const double* h, double spacing, int* n) {
    for (int a = 0; a < 3; a++) {
        const double len = sqrt(h[3 * a] * h[3 * a] + h[3 * a + 1] * h[3 * a + 1] + h[3 * a + 2] * h[3 * a + 2]);
        n[a] = p3m_pow2_at_least(len / spacing);
    }
}

// the cardinal B-spline M_n(x) on [0, n] by the Cox-de Boor recursion (n <= 5); M_0 = 0
__host__ __device__ inline double p3m_bspline(int n, double x) {
    if (n <= 0) return 0.0;
    double a[5];
    for (int k = 0; k < n; k++) {
        const double xk = x - k;
        a[k] = xk >= 0.0 && xk < 1.0 ? 1.0 : 0.0;
    }
    for (int m = 2; m <= n; m++)
        for (int k = 0; k <= n - m; k++) {
            const double xk = x - k;
            a[k] = (xk * a[k] + ((double)m - xk) * a[k + 1]) / (double)(m - 1);
        }
    return a[0];
}

__host__ __device__ inline double p3m_sinc(double x) {
    if (x == 0.0) return 1.0;
    const double y = EW_PI * x;
    return sin(y) / y;
}

__host__ __device__ inline int p3m_signed(int i, int n) { return 2 * i < n ? i : i - n; }

// G^(n) / Omega of one mesh point n (signed indices) and, with grad != nullptr, its derivative by cell_bc at fixed n (U_m
// does not depend on the cell): alias term by alias term, G/Omega times (sigma^2 + 2/k^2)(cell^{-T}k)_b k_c - (cell^{-T})_bc
__host__ __device__ inline double p3m_influence_point(const double* inv, double vol, const int* N, const int* n, double sigma,
                                                      int p, double* grad) {
    if (grad)
        for (int k = 0; k < 9; k++) grad[k] = 0.0;
    if (n[0] == 0 && n[1] == 0 && n[2] == 0) return 0.0;
    double num = 0.0, den = 0.0;
    for (int m0 = -2; m0 <= 2; m0++)
        for (int m1 = -2; m1 <= 2; m1++)
            for (int m2 = -2; m2 <= 2; m2++) {
                const double nu[3] = {(double)n[0] + (double)m0 * N[0], (double)n[1] + (double)m1 * N[1],
                                      (double)n[2] + (double)m2 * N[2]};
                const double u = p3m_sinc(nu[0] / N[0]) * p3m_sinc(nu[1] / N[1]) * p3m_sinc(nu[2] / N[2]);
                double u2 = 1.0;
                for (int q = 0; q < p; q++) u2 *= u * u;
                den += u2;
                double k[3], k2 = 0.0;
                for (int c = 0; c < 3; c++) {
                    k[c] = 2.0 * EW_PI * (inv[3 * c] * nu[0] + inv[3 * c + 1] * nu[1] + inv[3 * c + 2] * nu[2]);
                    k2 += k[c] * k[c];
                }
                if (!(k2 > 0.0)) continue;
                const double g = u2 * 4.0 * EW_PI * exp(-0.5 * sigma * sigma * k2) / k2 / vol;
                num += g;
                if (grad)
                    for (int b = 0; b < 3; b++) {
                        const double mb = inv[b] * k[0] + inv[3 + b] * k[1] + inv[6 + b] * k[2];
                        for (int c = 0; c < 3; c++) grad[3 * b + c] += g * ((sigma * sigma + 2.0 / k2) * mb * k[c] - inv[3 * c + b]);
                    }
            }
    const double d2 = 1.0 / (den * den);
    if (grad)
        for (int k = 0; k < 9; k++) grad[k] *= d2;
    return num * d2;
}

__device__ __forceinline__ int p3m_wrap(int i, int n) {
    const int r = i % n;
    return r < 0 ? r + n : r;
}

// half-spectrum point idx of a system -> signed reciprocal indices
__device__ __forceinline__ void p3m_spec_index(const P3mSysD& m, int idx, int* n) {
    const int iz = idx % m.nzh, iy = (idx / m.nzh) % m.n[1], ix = idx / (m.nzh * m.n[1]);
    n[0] = p3m_signed(ix, m.n[0]); n[1] = p3m_signed(iy, m.n[1]); n[2] = p3m_signed(iz, m.n[2]);
}

// ---- plan time ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_p3m_influence(P3mSysD m, double sigma, int p, int count, float* __restrict__ infl) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    int n[3];
    p3m_spec_index(m, idx, n);
    infl[m.soff + idx] = (float)p3m_influence_point(m.inv, m.vol, m.n, n, sigma, p, nullptr);
}

// ---- binning ------------------------------------------------------------------------------------------------------------------
// per atom of a periodic system: weights and their derivatives by u (fp64, rounded once), the wrapped stencil origin and its bin.
// With d2wts (pet_p3m_second): the second derivatives M_{p-2}(x) - 2 M_{p-2}(x-1) + M_{p-2}(x-2) as well, and with a direction
// Ur [N, 3] the atom's du = N (.) (u_r cell^{-1}) in mesh units (zero without one, and on atoms of open systems).
__global__ __launch_bounds__(256) void k_p3m_bin_count(const float* __restrict__ pos, const int* __restrict__ gsys,
                                                       const EwSys* __restrict__ sys, const P3mSysD* __restrict__ msys, int N,
                                                       int p, float* __restrict__ wts, float* __restrict__ dwts,
                                                       int4* __restrict__ org, int* __restrict__ start,
                                                       float* __restrict__ d2wts, const float* __restrict__ Ur,
                                                       float* __restrict__ du) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int si = gsys[i];
    const EwSys& s = sys[si];
    const P3mSysD& m = msys[si];
    int o[3] = {0, 0, 0};
    for (int ax = 0; ax < 3; ax++) {
        float* w = wts + ((int64_t)i * 3 + ax) * p;
        float* dw = dwts + ((int64_t)i * 3 + ax) * p;
        float* d2w = d2wts ? d2wts + ((int64_t)i * 3 + ax) * p : nullptr;
        if (!s.periodic) {
            for (int t = 0; t < p; t++) w[t] = dw[t] = 0.f;
            for (int t = 0; d2w && t < p; t++) d2w[t] = 0.f;
            if (du) du[3 * (int64_t)i + ax] = 0.f;
            continue;
        }
        double f = (double)pos[3 * (int64_t)i] * s.inv[ax] + (double)pos[3 * (int64_t)i + 1] * s.inv[3 + ax] +
                   (double)pos[3 * (int64_t)i + 2] * s.inv[6 + ax];
        f -= floor(f);
        const double u = f * (double)m.n[ax];
        const double base = (p & 1) ? floor(u + 0.5) - (double)((p - 1) / 2) : floor(u) - (double)(p / 2 - 1);
        for (int t = 0; t < p; t++) {
            const double x = u - (base + (double)t) + 0.5 * (double)p;
            w[t] = (float)p3m_bspline(p, x);
            dw[t] = (float)(p3m_bspline(p - 1, x) - p3m_bspline(p - 1, x - 1.0));
            if (d2w) d2w[t] = (float)(p3m_bspline(p - 2, x) - 2.0 * p3m_bspline(p - 2, x - 1.0) + p3m_bspline(p - 2, x - 2.0));
        }
        if (du)
            du[3 * (int64_t)i + ax] =
                Ur ? (float)((double)m.n[ax] * ((double)Ur[3 * (int64_t)i] * s.inv[ax] + (double)Ur[3 * (int64_t)i + 1] * s.inv[3 + ax] +
                                                (double)Ur[3 * (int64_t)i + 2] * s.inv[6 + ax]))
                   : 0.f;
        o[ax] = p3m_wrap((int)base, m.n[ax]);
    }
    int key = -1;
    if (s.periodic) {
        key = (int)(m.moff + ((int64_t)o[0] * m.n[1] + o[1]) * m.n[2] + o[2]);
        atomicAdd(&start[key], 1);
    }
    org[i] = make_int4(o[0], o[1], o[2], key);
}

// exclusive prefix sum of a[0..n) in place: blocks of 1024, their totals, and the totals added back
__global__ __launch_bounds__(256) void k_p3m_bin_scan1(int* __restrict__ a, int n, int* __restrict__ bsum) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * 1024 + 4 * t;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = base + k < n ? a[base + k] : 0;
    const int tot = v[0] + v[1] + v[2] + v[3];
    s[t] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int x = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    int run = s[t] - tot;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) a[base + k] = run;
        run += v[k];
    }
    if (t == 255) bsum[blockIdx.x] = s[255];
}

__global__ __launch_bounds__(256) void k_p3m_bin_scan2(int* __restrict__ bsum, int nb) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    int carry = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int v = c0 + t < nb ? bsum[c0 + t] : 0;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int x = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (c0 + t < nb) bsum[c0 + t] = carry + s[t] - v;
        carry += s[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_p3m_bin_scan3(int* __restrict__ a, int n, const int* __restrict__ bsum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] += bsum[i / 1024];
}

__global__ __launch_bounds__(256) void k_p3m_bin_place(const int4* __restrict__ org, const int* __restrict__ start,
                                                       int* __restrict__ fill, int N, int* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int key = org[i].w;
    if (key < 0) return;
    order[start[key] + atomicAdd(&fill[key], 1)] = i;
}

// a bin's atoms into atom order (insertion sort by one thread: bins hold a handful of atoms)
__global__ __launch_bounds__(256) void k_p3m_bin_sort(const int* __restrict__ start, int nbins, int* __restrict__ order) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nbins) return;
    const int lo = start[b], hi = start[b + 1];
    for (int a = lo + 1; a < hi; a++) {
        const int v = order[a];
        int c = a - 1;
        while (c >= lo && order[c] > v) {
            order[c + 1] = order[c];
            c--;
        }
        order[c + 1] = v;
    }
}

// ---- mesh kernels -----------------------------------------------------------------------------------------------------------
// owner computes: a thread owns one mesh point and P3M_CH channels; it walks the p^3 bins whose atoms reach the point
__global__ __launch_bounds__(256) void k_p3m_spread(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                    const int* __restrict__ start, const int* __restrict__ order,
                                                    const float* __restrict__ wts, int p, const float* __restrict__ X, int C,
                                                    bool vec, float* __restrict__ mesh) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const int idx = tile.y + threadIdx.x;
    if (idx >= M) return;
    const int z = idx % m.n[2], y = (idx / m.n[2]) % m.n[1], x = idx / (m.n[2] * m.n[1]);
    const int c0 = blockIdx.y * P3M_CH;
    float acc[P3M_CH];
#pragma unroll
    for (int u = 0; u < P3M_CH; u++) acc[u] = 0.f;
    for (int tx = 0; tx < p; tx++) {
        const int bx = p3m_wrap(x - tx, m.n[0]);
        for (int ty = 0; ty < p; ty++) {
            const int by = p3m_wrap(y - ty, m.n[1]);
            for (int tz = 0; tz < p; tz++) {
                const int bz = p3m_wrap(z - tz, m.n[2]);
                const int64_t bin = m.moff + ((int64_t)bx * m.n[1] + by) * m.n[2] + bz;
                const int lo = start[bin], hi = start[bin + 1];
                for (int a = lo; a < hi; a++) {
                    const int j = order[a];
                    const float* wj = wts + (int64_t)j * 3 * p;
                    const float w = wj[tx] * wj[p + ty] * wj[2 * p + tz];
                    const float* row = X + (int64_t)j * C + c0;
                    if (vec) {
                        const f32x4 r0 = *reinterpret_cast<const f32x4*>(row);
                        const f32x4 r1 = *reinterpret_cast<const f32x4*>(row + 4);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            acc[u] += w * r0[u];
                            acc[4 + u] += w * r1[u];
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < P3M_CH; u++)
                            if (c0 + u < C) acc[u] += w * row[u];
                    }
                }
            }
        }
    }
    float* out = mesh + m.moff * C + idx;
#pragma unroll
    for (int u = 0; u < P3M_CH; u++)
        if (c0 + u < C) out[(int64_t)(c0 + u) * M] = acc[u];
}

// spectrum[c][n] *= G^(n)/Omega, in place; a block takes P3M_CHUNK points of one system, gridDim.y strides the channels
__global__ __launch_bounds__(256) void k_p3m_filter(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                    const float* __restrict__ infl, int C, float2* __restrict__ spec) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int Mh = m.n[0] * m.n[1] * m.nzh;
    for (int r = 0; r < P3M_CHUNK / 256; r++) {
        const int idx = tile.y + r * 256 + threadIdx.x;
        if (idx >= Mh) return;
        const float g = infl[m.soff + idx];
        for (int c = blockIdx.y; c < C; c += gridDim.y) {
            float2* v = spec + m.soff * C + (int64_t)c * Mh + idx;
            const float2 a = *v;
            *v = make_float2(a.x * g, a.y * g);
        }
    }
}

// one wave per atom of a periodic system, lanes over channels: V[i][c] = sum over the p^3 nodes of W Phi[c][node]
__global__ __launch_bounds__(256) void k_p3m_gather(const int* __restrict__ gsys, const P3mSysD* __restrict__ msys,
                                                    const int4* __restrict__ org, const float* __restrict__ wts, int p,
                                                    const float* __restrict__ phi, int N, int C, float* __restrict__ V) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int4 o = org[i];
    if (o.w < 0) return;
    const P3mSysD& m = msys[gsys[i]];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const float* wi = wts + (int64_t)i * 3 * p;
    const float* base = phi + m.moff * C;
    for (int c = lane; c < C; c += 64) {
        const float* plane = base + (int64_t)c * M;
        float acc = 0.f;
        for (int tx = 0; tx < p; tx++) {
            const int ix = p3m_wrap(o.x + tx, m.n[0]);
            for (int ty = 0; ty < p; ty++) {
                const int iy = p3m_wrap(o.y + ty, m.n[1]);
                const float wxy = wi[tx] * wi[p + ty];
                for (int tz = 0; tz < p; tz++) {
                    const int iz = p3m_wrap(o.z + tz, m.n[2]);
                    acc += wxy * wi[2 * p + tz] * plane[((int64_t)ix * m.n[1] + iy) * m.n[2] + iz];
                }
            }
        }
        V[(int64_t)i * C + c] = acc;
    }
}

// the position adjoint of the mesh sum: F_i = P sum_c sum_nodes grad_r W_i(node) [g_ic Phi_q + q_ic Phi_g](node, c), with
// dW/dr_b = sum_a N_a (cell^{-1})_{ba} dW/du_a. One wave per atom, lanes over channels, reduced by the butterfly of k_ew_force
__global__ __launch_bounds__(256) void k_p3m_force(const int* __restrict__ gsys, const P3mSysD* __restrict__ msys,
                                                   const int4* __restrict__ org, const float* __restrict__ wts,
                                                   const float* __restrict__ dwts, int p, const float* __restrict__ phi_q,
                                                   const float* __restrict__ phi_g, const float* __restrict__ G,
                                                   const float* __restrict__ Q, int N, int C, float* __restrict__ F) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int4 o = org[i];
    if (o.w < 0) return;
    const P3mSysD& m = msys[gsys[i]];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const float* wi = wts + (int64_t)i * 3 * p;
    const float* di = dwts + (int64_t)i * 3 * p;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float* pq = phi_q + m.moff * C + (int64_t)c * M;
        const float* pg = phi_g + m.moff * C + (int64_t)c * M;
        const float gi = G[(int64_t)i * C + c], qi = Q[(int64_t)i * C + c];
        for (int tx = 0; tx < p; tx++) {
            const int ix = p3m_wrap(o.x + tx, m.n[0]);
            for (int ty = 0; ty < p; ty++) {
                const int iy = p3m_wrap(o.y + ty, m.n[1]);
                for (int tz = 0; tz < p; tz++) {
                    const int iz = p3m_wrap(o.z + tz, m.n[2]);
                    const int64_t node = ((int64_t)ix * m.n[1] + iy) * m.n[2] + iz;
                    const float v = gi * pq[node] + qi * pg[node];
                    f0 += di[tx] * wi[p + ty] * wi[2 * p + tz] * v;
                    f1 += wi[tx] * di[p + ty] * wi[2 * p + tz] * v;
                    f2 += wi[tx] * wi[p + ty] * di[2 * p + tz] * v;
                }
            }
        }
    }
    f0 = wsum(f0); f1 = wsum(f1); f2 = wsum(f2);
    if (lane < 3) {
        const double a0 = (double)f0 * m.n[0], a1 = (double)f1 * m.n[1], a2 = (double)f2 * m.n[2];
        F[3 * (int64_t)i + lane] = (float)(EW_PREFACTOR * (m.inv[3 * lane] * a0 + m.inv[3 * lane + 1] * a1 + m.inv[3 * lane + 2] * a2));
    }
}

// ---- second order (pet_p3m_second) -----------------------------------------------------------------------
// Positions enter the mesh sum A = W^T K W through W alone. Along a direction u_r, with du_i = N (.) (u_r,i cell^{-1}) per atom,
//   (D_u W)_i(node) = dW_x du_x W_y W_z + W_x dW_y du_y W_z + W_x W_y dW_z du_z                  (the TANGENT weight)
//   (grad grad W . du)_a = d/du_a of the tangent weight                                          (the Hessian weight)
// The three kernels below are k_p3m_spread, k_p3m_gather and k_p3m_force with those weights beside the plain ones, in the same
// walks and orders.

// k_p3m_spread with two operands: mesh = W X1 + (D_u W) X2, either may be null (not both)
__global__ __launch_bounds__(256) void k_p3m_spread2(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                     const int* __restrict__ start, const int* __restrict__ order,
                                                     const float* __restrict__ wts, const float* __restrict__ dwts,
                                                     const float* __restrict__ du, int p, const float* __restrict__ X1,
                                                     const float* __restrict__ X2, int C, float* __restrict__ mesh) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const int idx = tile.y + threadIdx.x;
    if (idx >= M) return;
    const int z = idx % m.n[2], y = (idx / m.n[2]) % m.n[1], x = idx / (m.n[2] * m.n[1]);
    const int c0 = blockIdx.y * P3M_CH;
    float acc[P3M_CH];
#pragma unroll
    for (int u = 0; u < P3M_CH; u++) acc[u] = 0.f;
    for (int tx = 0; tx < p; tx++) {
        const int bx = p3m_wrap(x - tx, m.n[0]);
        for (int ty = 0; ty < p; ty++) {
            const int by = p3m_wrap(y - ty, m.n[1]);
            for (int tz = 0; tz < p; tz++) {
                const int bz = p3m_wrap(z - tz, m.n[2]);
                const int64_t bin = m.moff + ((int64_t)bx * m.n[1] + by) * m.n[2] + bz;
                const int lo = start[bin], hi = start[bin + 1];
                for (int a = lo; a < hi; a++) {
                    const int j = order[a];
                    const float* wj = wts + (int64_t)j * 3 * p;
                    const float wx = wj[tx], wy = wj[p + ty], wz = wj[2 * p + tz];
                    if (X1) {
                        const float w = wx * wy * wz;
                        const float* row = X1 + (int64_t)j * C + c0;
#pragma unroll
                        for (int u = 0; u < P3M_CH; u++)
                            if (c0 + u < C) acc[u] += w * row[u];
                    }
                    if (X2) {
                        const float* dj = dwts + (int64_t)j * 3 * p;
                        const float* uj = du + 3 * (int64_t)j;
                        const float tw = dj[tx] * uj[0] * wy * wz + wx * (dj[p + ty] * uj[1]) * wz + wx * wy * (dj[2 * p + tz] * uj[2]);
                        const float* row = X2 + (int64_t)j * C + c0;
#pragma unroll
                        for (int u = 0; u < P3M_CH; u++)
                            if (c0 + u < C) acc[u] += tw * row[u];
                    }
                }
            }
        }
    }
    float* out = mesh + m.moff * C + idx;
#pragma unroll
    for (int u = 0; u < P3M_CH; u++)
        if (c0 + u < C) out[(int64_t)(c0 + u) * M] = acc[u];
}

// k_p3m_gather of two mesh potentials in one stencil walk: V[i][c] = scale sum_nodes [ W phi_a + (D_u W) phi_b ], phi_b may be null.
// The tangent weights of an atom add up to zero, so on an atom whose surroundings are symmetric (a one-atom cell) the result
// is what is left of terms 1e4 times its size: the products and the two sums are fp64, which keeps the kernel's own rounding
// out of that residue (the walk waits for its node loads, not for these).
__global__ __launch_bounds__(256) void k_p3m_gather2(const int* __restrict__ gsys, const P3mSysD* __restrict__ msys,
                                                     const int4* __restrict__ org, const float* __restrict__ wts,
                                                     const float* __restrict__ dwts, const float* __restrict__ du, int p,
                                                     const float* __restrict__ phi_a, const float* __restrict__ phi_b, int N,
                                                     int C, float scale, float* __restrict__ V) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int4 o = org[i];
    if (o.w < 0) return;
    const P3mSysD& m = msys[gsys[i]];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const float* wi = wts + (int64_t)i * 3 * p;
    const float* di = dwts + (int64_t)i * 3 * p;
    const double u0 = du[3 * (int64_t)i], u1 = du[3 * (int64_t)i + 1], u2 = du[3 * (int64_t)i + 2];
    for (int c = lane; c < C; c += 64) {
        const float* pa = phi_a + m.moff * C + (int64_t)c * M;
        const float* pb = phi_b ? phi_b + m.moff * C + (int64_t)c * M : nullptr;
        double acc_a = 0.0, acc_b = 0.0;
        for (int tx = 0; tx < p; tx++) {
            const int ix = p3m_wrap(o.x + tx, m.n[0]);
            for (int ty = 0; ty < p; ty++) {
                const int iy = p3m_wrap(o.y + ty, m.n[1]);
                const double wxy = (double)wi[tx] * (double)wi[p + ty];
                const double txy = (double)di[tx] * u0 * (double)wi[p + ty] + (double)wi[tx] * ((double)di[p + ty] * u1);
                for (int tz = 0; tz < p; tz++) {
                    const int iz = p3m_wrap(o.z + tz, m.n[2]);
                    const int64_t node = ((int64_t)ix * m.n[1] + iy) * m.n[2] + iz;
                    const double wz = wi[2 * p + tz];
                    acc_a += wxy * wz * (double)pa[node];
                    if (pb) acc_b += (txy * wz + wxy * ((double)di[2 * p + tz] * u2)) * (double)pb[node];
                }
            }
        }
        V[(int64_t)i * C + c] = (float)((double)scale * (acc_a + acc_b));
    }
}

// k_p3m_force with the second-order terms, from four mesh potentials in one walk (phi_q = K W q, phi_g = K W g,
// phi_a = K (W u_q + (D_u W) q), phi_dg = K (D_u W) g):
//   F_i = P sum_c sum_nodes { grad W [ u_q phi_g + g phi_a + q phi_dg ] + (grad grad W . du) [ g phi_q + q phi_g ] }
// = the mesh part of grad_r Phi(r; u_q, g) + H_Phi(r; g, q) u_r. Uq may be null (zero). fp64 products and per-lane sums, as
// k_p3m_gather2 (the gradient weights add up to zero as well); the butterfly over channels is the fp32 one of k_ew_force.
__global__ __launch_bounds__(256) void k_p3m_force2(const int* __restrict__ gsys, const P3mSysD* __restrict__ msys,
                                                    const int4* __restrict__ org, const float* __restrict__ wts,
                                                    const float* __restrict__ dwts, const float* __restrict__ d2wts,
                                                    const float* __restrict__ du, int p, const float* __restrict__ phi_q,
                                                    const float* __restrict__ phi_g, const float* __restrict__ phi_a,
                                                    const float* __restrict__ phi_dg, const float* __restrict__ G,
                                                    const float* __restrict__ Q, const float* __restrict__ Uq, int N, int C,
                                                    float* __restrict__ F) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int4 o = org[i];
    if (o.w < 0) return;
    const P3mSysD& m = msys[gsys[i]];
    const int M = m.n[0] * m.n[1] * m.n[2];
    const float* wi = wts + (int64_t)i * 3 * p;
    const float* di = dwts + (int64_t)i * 3 * p;
    const float* ei = d2wts + (int64_t)i * 3 * p;
    const double u0 = du[3 * (int64_t)i], u1 = du[3 * (int64_t)i + 1], u2 = du[3 * (int64_t)i + 2];
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const int64_t plane = m.moff * C + (int64_t)c * M;
        const float *pq = phi_q + plane, *pg = phi_g + plane, *pa = phi_a + plane, *pd = phi_dg + plane;
        const double gi = G[(int64_t)i * C + c], qi = Q[(int64_t)i * C + c], ui = Uq ? Uq[(int64_t)i * C + c] : 0.f;
        for (int tx = 0; tx < p; tx++) {
            const int ix = p3m_wrap(o.x + tx, m.n[0]);
            const double wx = wi[tx], dx = di[tx], bx = dx * u0, ex = (double)ei[tx] * u0;
            for (int ty = 0; ty < p; ty++) {
                const int iy = p3m_wrap(o.y + ty, m.n[1]);
                const double wy = wi[p + ty], dy = di[p + ty], by = dy * u1, ey = (double)ei[p + ty] * u1;
                for (int tz = 0; tz < p; tz++) {
                    const int iz = p3m_wrap(o.z + tz, m.n[2]);
                    const double wz = wi[2 * p + tz], dz = di[2 * p + tz], bz = dz * u2, ez = (double)ei[2 * p + tz] * u2;
                    const int64_t node = ((int64_t)ix * m.n[1] + iy) * m.n[2] + iz;
                    const double vq = pq[node], vg = pg[node];
                    const double v1 = ui * vg + gi * (double)pa[node] + qi * (double)pd[node];
                    const double v2 = gi * vq + qi * vg;
                    f0 += dx * wy * wz * v1 + (ex * wy * wz + dx * (by * wz + wy * bz)) * v2;
                    f1 += wx * dy * wz * v1 + (ey * wx * wz + dy * (bx * wz + wx * bz)) * v2;
                    f2 += wx * wy * dz * v1 + (ez * wx * wy + dz * (bx * wy + wx * by)) * v2;
                }
            }
        }
    }
    const float s0 = wsum((float)f0), s1 = wsum((float)f1), s2 = wsum((float)f2);
    if (lane < 3) {
        const double a0 = (double)s0 * m.n[0], a1 = (double)s1 * m.n[1], a2 = (double)s2 * m.n[2];
        F[3 * (int64_t)i + lane] = (float)(EW_PREFACTOR * (m.inv[3 * lane] * a0 + m.inv[3 * lane + 1] * a1 + m.inv[3 * lane + 2] * a2));
    }
}

// the reciprocal part of dL/dcell through G^/Omega: per chunk of P3M_CHUNK half-spectrum points of one system,
// kpart[chunk][9] = P sum_n w_n Re(conj(g^_n) q^_n) d(G^_n/Omega)/dcell (fp64, points in index order per thread, then a fixed
// tree over the block); k_ew_cell adds a system's chunks in order
__global__ __launch_bounds__(256) void k_p3m_cell(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                  const float2* __restrict__ spec_q, const float2* __restrict__ spec_g, int C,
                                                  double sigma, int p, double* __restrict__ kpart) {
    __shared__ double red[256][9];
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int Mh = m.n[0] * m.n[1] * m.nzh;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = 0.0;
    for (int r = 0; r < P3M_CHUNK / 256; r++) {
        const int idx = tile.y + r * 256 + threadIdx.x;
        if (idx >= Mh) break;
        double zsum = 0.0;
        for (int c = 0; c < C; c++) {
            const int64_t at = m.soff * C + (int64_t)c * Mh + idx;
            const float2 a = spec_g[at], b = spec_q[at];
            zsum += (double)(a.x * b.x + a.y * b.y);
        }
        int n[3];
        p3m_spec_index(m, idx, n);
        const int iz = idx % m.nzh;
        const double w = (iz == 0 || 2 * iz == m.n[2]) ? 1.0 : 2.0;
        double grad[9];
        (void)p3m_influence_point(m.inv, m.vol, m.n, n, sigma, p, grad);
#pragma unroll
        for (int k = 0; k < 9; k++) acc[k] += w * zsum * grad[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) red[threadIdx.x][k] = acc[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 9; k++) red[threadIdx.x][k] += red[threadIdx.x + o][k];
        __syncthreads();
    }
    if (threadIdx.x < 9) kpart[9 * (int64_t)blockIdx.x + threadIdx.x] = EW_PREFACTOR * red[0][threadIdx.x];
}

// ---- cell tangents (pet_p3m_second_cell) -----------------------------------------------------------------
// At fixed fractional coordinates the mesh sum A = W^T K W depends on the cell through the filter alone: along u_c it is
// W^T K' W with G^/Omega replaced by gdot = sum_bc d(G^/Omega)/dcell_bc u_c,bc (p3m_influence_point's gradient, fp64, rounded
// once). K' X shares X's forward transform with K X: k_p3m_filter_dot keeps gdot (.) spectrum aside before the filter runs, and
// k_p3m_spec_add adds it to the filtered spectrum of the mesh that the tangent gather reads, before that one's inverse
// transform. No transform is added.
__global__ __launch_bounds__(256) void k_p3m_gdot(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                  const float* __restrict__ ucell, double sigma, int p,
                                                  float* __restrict__ gdot) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int Mh = m.n[0] * m.n[1] * m.nzh;
    const float* uc = ucell + 9 * (int64_t)tile.x;
    for (int r = 0; r < P3M_CHUNK / 256; r++) {
        const int idx = tile.y + r * 256 + threadIdx.x;
        if (idx >= Mh) return;
        int n[3];
        p3m_spec_index(m, idx, n);
        double grad[9], acc = 0.0;
        (void)p3m_influence_point(m.inv, m.vol, m.n, n, sigma, p, grad);
#pragma unroll
        for (int k = 0; k < 9; k++) acc += grad[k] * (double)uc[k];
        gdot[m.soff + idx] = (float)acc;
    }
}

// side[c][n] = gdot(n) spectrum[c][n] (the unfiltered spectrum), in the tiling of k_p3m_filter
__global__ __launch_bounds__(256) void k_p3m_filter_dot(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys,
                                                        const float* __restrict__ gdot, int C, const float2* __restrict__ spec,
                                                        float2* __restrict__ side) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int Mh = m.n[0] * m.n[1] * m.nzh;
    for (int r = 0; r < P3M_CHUNK / 256; r++) {
        const int idx = tile.y + r * 256 + threadIdx.x;
        if (idx >= Mh) return;
        const float g = gdot[m.soff + idx];
        for (int c = blockIdx.y; c < C; c += gridDim.y) {
            const int64_t at = m.soff * C + (int64_t)c * Mh + idx;
            const float2 a = spec[at];
            side[at] = make_float2(a.x * g, a.y * g);
        }
    }
}

// spectrum[c][n] += side[c][n]
__global__ __launch_bounds__(256) void k_p3m_spec_add(const int2* __restrict__ tiles, const P3mSysD* __restrict__ msys, int C,
                                                      const float2* __restrict__ side, float2* __restrict__ spec) {
    const int2 tile = tiles[blockIdx.x];
    const P3mSysD& m = msys[tile.x];
    const int Mh = m.n[0] * m.n[1] * m.nzh;
    for (int r = 0; r < P3M_CHUNK / 256; r++) {
        const int idx = tile.y + r * 256 + threadIdx.x;
        if (idx >= Mh) return;
        for (int c = blockIdx.y; c < C; c += gridDim.y) {
            const int64_t at = m.soff * C + (int64_t)c * Mh + idx;
            const float2 a = spec[at], b = side[at];
            spec[at] = make_float2(a.x + b.x, a.y + b.y);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct P3mWs {
    float *wts, *dwts;
    int4* org;
    int *start, *fill, *order, *bsum;
    EwLocalWs loc;  // kpart: one entry per reduction chunk
};

size_t p3m_carve(const pet_ewald_t* e, int64_t C, void* base, P3mWs& w) {
    Carver c(base);
    const P3mPlan* mp = e->p3m;
    const size_t N = (size_t)std::max<int64_t>(e->n_atoms, 1), S = (size_t)std::max<int64_t>(e->n_systems, 1);
    const size_t M = (size_t)mp->m_total, p = (size_t)e->p3m_nodes;
    w.wts = c.take<float>(N * 3 * p);
    w.dwts = c.take<float>(N * 3 * p);
    w.org = c.take<int4>(N);
    w.start = c.take<int>(M + 1);
    w.fill = c.take<int>(M + 1);
    w.order = c.take<int>(N);
    w.bsum = c.take<int>((M + 1 + 1023) / 1024 + 1);
    w.loc.sum_q = c.take<float>(S * C);
    w.loc.sum_g = c.take<float>(S * C);
    w.loc.F = c.take<float>(N * 3);
    w.loc.cell_part = c.take<float>(N * 9);
    w.loc.kpart = c.take<double>(std::max<size_t>(mp->stiles.size(), 1) * 9);
    return c.off;
}

int p3m_check(const pet_ewald_t* e, const pet_graph_t* pg, int32_t C, const void* ws, int64_t ws_bytes) {
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes != 0, PET_ERR_ARGUMENT,
                "a pet_p3m_* entry point on an Ewald-mode handle: call pet_ewald_set_p3m before pet_ewald_plan");
    PET_TRY(ew_check_graph(e, pg, C));
    P3mWs w;
    PET_REQUIRE(e->n_atoms == 0 || (ws && ws_bytes >= (int64_t)p3m_carve(e, C, nullptr, w)), PET_ERR_ARGUMENT,
                "P3M workspace missing or too small (pet_p3m_workspace_bytes)");
    return PET_OK;
}

// weights, origins and the stable counting sort of the atoms by origin bin
int p3m_bin(const pet_ewald_t* e, const Graph& g, const float* pos, const P3mWs& w, hipStream_t st, float* d2wts = nullptr,
            const float* Ur = nullptr, float* du = nullptr) {
    const P3mPlan* mp = e->p3m;
    const int N = (int)e->n_atoms, nb = (int)mp->m_total + 1;
    PET_HIP_CHECK(hipMemsetAsync(w.start, 0, (size_t)nb * sizeof(int), st));
    PET_HIP_CHECK(hipMemsetAsync(w.fill, 0, (size_t)nb * sizeof(int), st));
    k_p3m_bin_count<<<cdiv(N, 256), 256, 0, st>>>(pos, g.sys, e->d_sys, mp->d_sys, N, e->p3m_nodes, w.wts, w.dwts, w.org, w.start,
                                                      d2wts, Ur, du);
    const int blocks = cdiv(nb, 1024);
    k_p3m_bin_scan1<<<blocks, 256, 0, st>>>(w.start, nb, w.bsum);
    k_p3m_bin_scan2<<<1, 256, 0, st>>>(w.bsum, blocks);
    k_p3m_bin_scan3<<<cdiv(nb, 256), 256, 0, st>>>(w.start, nb, w.bsum);
    k_p3m_bin_place<<<cdiv(N, 256), 256, 0, st>>>(w.org, w.start, w.fill, N, w.order);
    if (mp->m_total > 0) k_p3m_bin_sort<<<cdiv(mp->m_total, 256), 256, 0, st>>>(w.start, (int)mp->m_total, w.order);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// The workspace of the second-order operation and of the dual pass: that of the staged entry points, then the
// second-derivative weights, the per-atom directions, FOUR packed meshes and ONE packed half spectrum (the transforms of an
// entry point run one after another on its stream); then (cell: pet_p3m_second_cell) u' [N, 3], gdot per half-spectrum point
// and the side spectrum. The byte offsets are what the transform hook is given: they count from the d_workspace of the entry
// point that is running, ws_offset bytes before this workspace (the dual pass keeps its own rows in front of the operator's).
enum { MESH_Q = 0, MESH_G = 1, MESH_A = 2, MESH_DG = 3 };
struct P3mWs2 {
    P3mWs w;
    float *d2wts, *du;
    float* mesh[4];
    float2* spec;
    int64_t mesh_off[4], spec_off;
    float *up, *gdot;
    float2* side;
};

size_t p3m_carve2(const pet_ewald_t* e, int64_t C, void* base, P3mWs2& w2, bool cell, int64_t ws_offset = 0) {
    Carver c(base);
    c.off = p3m_carve(e, C, base, w2.w);
    const P3mPlan* mp = e->p3m;
    const size_t N = (size_t)std::max<int64_t>(e->n_atoms, 1), p = (size_t)e->p3m_nodes;
    w2.d2wts = c.take<float>(N * 3 * p);
    w2.du = c.take<float>(N * 3);
    for (int k = 0; k < 4; k++) {
        w2.mesh_off[k] = ws_offset + (int64_t)c.off;
        w2.mesh[k] = c.take<float>((size_t)std::max<int64_t>(mp->m_total, 1) * C);
    }
    w2.spec_off = ws_offset + (int64_t)c.off;
    w2.spec = c.take<float2>((size_t)std::max<int64_t>(mp->s_total, 1) * C);
    w2.up = w2.gdot = nullptr;
    w2.side = nullptr;
    if (cell) {
        const size_t Sp = (size_t)std::max<int64_t>(mp->s_total, 1);
        w2.up = c.take<float>(N * 3);
        w2.gdot = c.take<float>(Sp);
        w2.side = c.take<float2>(Sp * C);
    }
    return c.off;
}

// mesh[slot] <- K mesh[slot]: the hook's rfftn into the half spectrum, the filter, the hook's irfftn back. Under a cell tangent
// the filter's tangent rides on the same transforms: CELL_KEEP keeps (gdot . the unfiltered spectrum) in the side spectrum,
// CELL_ADD adds the side spectrum to the filtered one. Two hook calls either way.
enum { CELL_NONE = -1, CELL_KEEP = 0, CELL_ADD = 1 };
int p3m_solve(const pet_ewald_t* e, int C, const P3mWs2& w2, int slot, hipStream_t st, int what = CELL_NONE) {
    const P3mPlan* mp = e->p3m;
    if (mp->stiles.empty()) return PET_OK;
    const dim3 grid((unsigned)mp->stiles.size(), (unsigned)std::min(C, 256));
    for (int inverse = 0; inverse < 2; inverse++) {
        const int rc = e->p3m_transform(e->p3m_transform_user, inverse, w2.mesh_off[slot], w2.spec_off, C);
        PET_REQUIRE(rc == 0, PET_ERR_ARGUMENT,
                    "the transform hook (pet_p3m_set_transform) returned " + std::to_string(rc) + " for the " +
                        (inverse ? "inverse" : "forward") + " transform");
        if (inverse) continue;
        if (what == CELL_KEEP) k_p3m_filter_dot<<<grid, 256, 0, st>>>(mp->d_stiles, mp->d_sys, w2.gdot, C, w2.spec, w2.side);
        k_p3m_filter<<<grid, 256, 0, st>>>(mp->d_stiles, mp->d_sys, mp->d_infl, C, w2.spec);
        if (what == CELL_ADD) k_p3m_spec_add<<<grid, 256, 0, st>>>(mp->d_stiles, mp->d_sys, C, w2.side, w2.spec);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---- the three launches that the staged entry points (pet_p3m_spread / _finish / _backward) share with the interface ----------
// mesh <- W X on the bins that p3m_bin left in w
void p3m_spread(const pet_ewald_t* e, const float* X, int C, const P3mWs& w, float* mesh, hipStream_t st) {
    const P3mPlan* mp = e->p3m;
    if (mp->mtiles.empty()) return;
    const bool vec = C % P3M_CH == 0 && ((uintptr_t)X & 15) == 0;
    k_p3m_spread<<<dim3((unsigned)mp->mtiles.size(), (unsigned)cdiv(C, P3M_CH)), 256, 0, st>>>(
        mp->d_mtiles, mp->d_sys, w.start, w.order, w.wts, e->p3m_nodes, X, C, vec, mesh);
}
// out <- W^T phi on the atoms of periodic systems
void p3m_gather(const pet_ewald_t* e, const Graph& g, const P3mWs& w, const float* phi, int C, float* out, hipStream_t st) {
    if (e->p3m->m_total > 0)
        k_p3m_gather<<<cdiv(e->n_atoms, 4), 256, 0, st>>>(g.sys, e->p3m->d_sys, w.org, w.wts, e->p3m_nodes, phi, (int)e->n_atoms, C, out);
}
// w.loc.F <- the mesh part of grad_r Phi(r; G, Q) from the two mesh potentials
void p3m_force(const pet_ewald_t* e, const Graph& g, const P3mWs& w, const float* phi_q, const float* phi_g, const float* G,
               const float* Q, int C, hipStream_t st) {
    if (e->p3m->m_total > 0)
        k_p3m_force<<<cdiv(e->n_atoms, 4), 256, 0, st>>>(g.sys, e->p3m->d_sys, w.org, w.wts, w.dwts, e->p3m_nodes, phi_q, phi_g, G, Q,
                                                         (int)e->n_atoms, C, w.loc.F);
}
// out = W^T phi, then the local terms of the operator on X: what follows the mesh potential of X
int p3m_finish(const pet_ewald_t* e, const Graph& g, const float* pos, const float* X, int C, const float* phi, float* out,
               const P3mWs& w, hipStream_t st) {
    p3m_gather(e, g, w, phi, C, out, st);
    return ew_local_forward(e, g, pos, X, C, out, w.loc.sum_q, st);
}

// mesh[slot] <- K W X with the kernels of the staged entry points (the dual pass' first-order calls keep their bits)
int p3m_potential_mesh(const pet_ewald_t* e, const float* X, int C, const P3mWs2& w2, int slot, hipStream_t st) {
    if (e->p3m->mtiles.empty()) return PET_OK;
    p3m_spread(e, X, C, w2.w, w2.mesh[slot], st);
    return p3m_solve(e, C, w2, slot, st);
}

}  // namespace

// ---- the mesh operator's half of the interface (long_range.h). Every call bins anew (six small launches; the positions do not
// change inside a sweep, but neither do the calls share more than that) and nothing is kept between calls. -------------------
int64_t p3m_workspace_bytes(const pet_ewald_t* e, int C, bool cell) {
    P3mWs2 w2;
    return (int64_t)p3m_carve2(e, C, nullptr, w2, cell);
}

int p3m_potential(const LrCall& c, const float* X, float* out) {
    P3mWs2 w2;
    p3m_carve2(c.e, c.C, c.ws, w2, false, c.ws_offset);
    ProfScope ps("p3m_fwd", c.st, 0.0, 0.0);
    PET_TRY(p3m_bin(c.e, *c.g, c.pos, w2.w, c.st));
    PET_TRY(p3m_potential_mesh(c.e, X, c.C, w2, MESH_Q, c.st));
    return p3m_finish(c.e, *c.g, c.pos, X, c.C, w2.mesh[MESH_Q], out, w2.w, c.st);
}

int p3m_backward(const LrCall& c, const float* Q, const float* G, float* gq, float* gpos) {
    const pet_ewald_t* e = c.e;
    P3mWs2 w2;
    p3m_carve2(e, c.C, c.ws, w2, false, c.ws_offset);
    const P3mWs& w = w2.w;
    ProfScope ps("p3m_bwd", c.st, 0.0, 0.0);
    PET_TRY(p3m_bin(e, *c.g, c.pos, w, c.st));
    PET_TRY(p3m_potential_mesh(e, G, c.C, w2, MESH_G, c.st));
    PET_TRY(p3m_potential_mesh(e, Q, c.C, w2, MESH_Q, c.st));
    p3m_gather(e, *c.g, w, w2.mesh[MESH_G], c.C, gq, c.st);
    p3m_force(e, *c.g, w, w2.mesh[MESH_Q], w2.mesh[MESH_G], G, Q, c.C, c.st);
    PET_TRY(ew_local_forward(e, *c.g, c.pos, G, c.C, gq, w.loc.sum_g, c.st));
    return ew_local_backward(e, *c.g, c.pos, Q, G, c.C, w.loc, gpos, nullptr, c.st, [] {});
}

// The second-order operation with selectable results, as ew_second: a null out_q / out_g / out_r is not formed, and the meshes,
// transform pairs and launches that serve it alone are skipped. Q may be null where only out_q is asked for, G where only
// out_g is. Transform pairs with both cotangents: out_g alone 2 (phi_q, phi_a), out_q alone 2 (phi_g, phi_dg), out_r or all
// three 4; with u_q alone 1 / 0 / 2, with u_r alone as with both.
// With Ucell (pet_p3m_second_cell; no out_r): out_g = A u_q + (D A) q, out_q = (D A) g along (u_r, u_c). The position tangent is
// taken at u' = u_r - r U; the filter's tangent rides on the same transforms (p3m_solve); the local terms are k_ew_pairs<true> at
// u' and ew_local_cell. Transform pairs: 2 per result formed (4 hook calls), whatever the cotangents.
int p3m_second(const LrCall& c, const float* Q, const float* G, const float* Uq, const float* Ur, const float* Ucell, float* out_q,
               float* out_g, float* out_r) {
    const pet_ewald_t* e = c.e;
    const Graph& g = *c.g;
    const float* pos = c.pos;
    const int C = c.C;
    hipStream_t st = c.st;
    P3mWs2 w2;
    p3m_carve2(e, C, c.ws, w2, Ucell != nullptr, c.ws_offset);
    const P3mPlan* mp = e->p3m;
    const P3mWs& w = w2.w;
    const int N = (int)e->n_atoms, p = e->p3m_nodes;
    const bool per = mp->m_total > 0;
    const unsigned cy = (unsigned)cdiv(C, 256), nn = (unsigned)e->atiles_n.size(), na = (unsigned)cdiv(N, 4);
    const float inv_R = (float)(1.0 / e->cutoff);
    ProfScope ps(Ucell ? (out_g && out_q ? "p3m_second_cell" : out_g ? "p3m_second_cell_g" : "p3m_second_cell_q")
                 : out_q && out_g && out_r ? "p3m_second" : out_g ? "p3m_second_g" : out_r ? "p3m_second_qr" : "p3m_second_q",
                 st, 0.0, 0.0);
    auto mesh_of = [&](int slot, const float* X1, const float* X2, int what = CELL_NONE) -> int {
        if (!per) return PET_OK;
        k_p3m_spread2<<<dim3((unsigned)mp->mtiles.size(), (unsigned)cdiv(C, P3M_CH)), 256, 0, st>>>(
            mp->d_mtiles, mp->d_sys, w.start, w.order, w.wts, w.dwts, w2.du, p, X1, X2, C, w2.mesh[slot]);
        return p3m_solve(e, C, w2, slot, st, what);
    };
    auto gather = [&](const float* phi_a, const float* phi_b, float scale, float* out) {
        if (per)
            k_p3m_gather2<<<na, 256, 0, st>>>(g.sys, mp->d_sys, w.org, w.wts, w.dwts, w2.du, p, phi_a, phi_b, N, C, scale, out);
    };
    if (Ucell) {
        k_ew_uprime<<<cdiv(N, 256), 256, 0, st>>>(pos, g.sys, e->d_sys, Ur, Ucell, N, w2.up);
        PET_TRY(p3m_bin(e, g, pos, w, st, nullptr, w2.up, w2.du));
        if (!mp->stiles.empty())
            k_p3m_gdot<<<(unsigned)mp->stiles.size(), 256, 0, st>>>(mp->d_stiles, mp->d_sys, Ucell, e->sigma, p, w2.gdot);
        if (out_g) {
            // phi_q = K W q, then K (W u_q + (D_u' W) q) + K' W q as ONE mesh
            PET_TRY(mesh_of(MESH_Q, Q, nullptr, CELL_KEEP));
            PET_TRY(mesh_of(MESH_A, Uq, Q, CELL_ADD));
            if (Uq) {
                gather(w2.mesh[MESH_A], w2.mesh[MESH_Q], 1.f, out_g);
                PET_TRY(ew_local_forward(e, g, pos, Uq, C, out_g, w.loc.sum_g, st));
            } else {
                PET_HIP_CHECK(hipMemsetAsync(out_g, 0, (size_t)N * C * sizeof(float), st));
                gather(w2.mesh[MESH_A], w2.mesh[MESH_Q], (float)EW_PREFACTOR, out_g);
            }
        }
        if (out_q) {
            PET_TRY(mesh_of(MESH_G, G, nullptr, CELL_KEEP));
            PET_TRY(mesh_of(MESH_DG, nullptr, G, CELL_ADD));
            PET_HIP_CHECK(hipMemsetAsync(out_q, 0, (size_t)N * C * sizeof(float), st));
            gather(w2.mesh[MESH_DG], w2.mesh[MESH_G], (float)EW_PREFACTOR, out_q);
        }
        if (nn) {
            if (out_g) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, Q, C, out_g, w2.up);
            if (out_q) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, G, C, out_q, w2.up);
        }
        return ew_local_cell(e, g, Q, G, Ur, Ucell, C, w.loc, out_g, out_q, st);
    }
    PET_TRY(p3m_bin(e, g, pos, w, st, w2.d2wts, Ur, w2.du));
    if (Ur && (out_g || out_r)) PET_TRY(mesh_of(MESH_Q, Q, nullptr));
    if (out_r || (Ur && out_q)) PET_TRY(mesh_of(MESH_G, G, nullptr));
    if (out_g || out_r) PET_TRY(mesh_of(MESH_A, Uq, Ur ? Q : nullptr));  // W u_q + (D_u W) q as ONE mesh
    if (Ur && (out_q || out_r)) PET_TRY(mesh_of(MESH_DG, nullptr, G));
    if (Uq) {
        // out_g = A u_q + (D_u A) q on the mesh, then the local terms of A u_q; out_r = grad_r Phi(r; u_q, g): the first-order
        // adjoint with (g, q) := (u_q, g), whose mesh part waits for k_p3m_force2 where there is a direction
        if (out_g) {
            gather(w2.mesh[MESH_A], Ur ? w2.mesh[MESH_Q] : nullptr, 1.f, out_g);
            PET_TRY(ew_local_forward(e, g, pos, Uq, C, out_g, w.loc.sum_g, st));
        }
        if (out_r) {
            if (Ur) PET_HIP_CHECK(hipMemsetAsync(w.loc.F, 0, (size_t)N * 3 * sizeof(float), st));
            else p3m_force(e, g, w, w2.mesh[MESH_G], w2.mesh[MESH_A], Uq, G, C, st);
            PET_TRY(ew_local_backward(e, g, pos, G, Uq, C, w.loc, out_r, nullptr, st, [] {}));
        }
    } else {
        if (out_g) {
            PET_HIP_CHECK(hipMemsetAsync(out_g, 0, (size_t)N * C * sizeof(float), st));
            gather(w2.mesh[MESH_A], w2.mesh[MESH_Q], (float)EW_PREFACTOR, out_g);
        }
        if (out_r) PET_HIP_CHECK(hipMemsetAsync(out_r, 0, (size_t)N * 3 * sizeof(float), st));
    }
    if (out_q) PET_HIP_CHECK(hipMemsetAsync(out_q, 0, (size_t)N * C * sizeof(float), st));
    if (Ur) {
        // out_q = (D_u A) g, out_r += H u_r: mesh and open parts, then the exclusion rows (which add w.loc.F into out_r)
        if (out_q) gather(w2.mesh[MESH_DG], w2.mesh[MESH_G], (float)EW_PREFACTOR, out_q);
        if (out_r && per)
            k_p3m_force2<<<na, 256, 0, st>>>(g.sys, mp->d_sys, w.org, w.wts, w.dwts, w2.d2wts, w2.du, p, w2.mesh[MESH_Q],
                                             w2.mesh[MESH_G], w2.mesh[MESH_A], w2.mesh[MESH_DG], G, Q, Uq, N, C, w.loc.F);
        if (nn) {
            if (out_g) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, Q, C, out_g, Ur);
            if (out_q) k_ew_pairs<true><<<dim3(nn, cy), 256, 0, st>>>(e->d_atiles_n, e->d_sys, pos, inv_R, G, C, out_q, Ur);
            if (out_r)
                k_ew_force2<false><<<nn, 256, 0, st>>>(e->d_atiles_n, e->d_sys, nullptr, nullptr, 1, pos, inv_R, G, Q, nullptr, nullptr,
                                                       nullptr, nullptr, Ur, C, ew_vec_loads(C, Q, G), w.loc.F);
        }
        k_ew_edge_second<<<(unsigned)N, 64, 0, st>>>(e->d_sys, g.sys, g.rowptr, g.nbr, g.geo, G, Q, Ur, w.loc.F, C, e->sigma, e->cutoff,
                                                     out_g, out_q, out_r);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// pet_ewald_plan of a P3M-mode handle: mesh descriptors and influence functions instead of k lists, for the systems the shared
// part of the plan has described in sys. A periodic system with atoms gets a mesh; every system's range of reduction chunks
// (what k_ew_cell walks in this mode) goes into its first_k / n_k.
int p3m_plan_build(double sigma, double spacing, int nodes, const double* h_cells, std::vector<EwSys>& sys, P3mPlan** out) {
    P3mPlan* mp = new P3mPlan();
    struct Guard {
        P3mPlan* p;
        ~Guard() { p3m_release(p); }
    } guard{mp};
    const size_t n_systems = sys.size();
    mp->sys.resize(n_systems);
    for (size_t s = 0; s < n_systems; s++) {
        P3mSysD& m = mp->sys[s];
        m.n[0] = m.n[1] = m.n[2] = 0;
        m.nzh = 0;
        m.moff = mp->m_total;
        m.soff = mp->s_total;
        for (int k = 0; k < 9; k++) m.inv[k] = sys[s].inv[k];
        m.vol = sys[s].vol;
        sys[s].first_k = (int)mp->stiles.size();
        sys[s].n_k = 0;
        if (!sys[s].periodic || sys[s].n_atoms == 0) continue;
        p3m_mesh_shape(h_cells + 9 * s, spacing, m.n);
        for (int a = 0; a < 3; a++)
            PET_REQUIRE(m.n[a] <= P3M_MAX_AXIS, PET_ERR_UNSUPPORTED,
                        "system " + std::to_string(s) + " needs a mesh of " + std::to_string(m.n[a]) + " points along axis " +
                            std::to_string(a) + " at this kspace_resolution; at most " + std::to_string(P3M_MAX_AXIS) +
                            " per mesh axis are served");
        m.nzh = m.n[2] / 2 + 1;
        const int64_t M = (int64_t)m.n[0] * m.n[1] * m.n[2], Mh = (int64_t)m.n[0] * m.n[1] * m.nzh;
        for (int64_t i = 0; i < M; i += 256) mp->mtiles.push_back(make_int2((int)s, (int)i));
        for (int64_t i = 0; i < Mh; i += P3M_CHUNK) mp->stiles.push_back(make_int2((int)s, (int)i));
        sys[s].n_k = (int)mp->stiles.size() - sys[s].first_k;
        mp->m_total += M;
        mp->s_total += Mh;
        PET_REQUIRE(mp->m_total < (int64_t(1) << 30), PET_ERR_UNSUPPORTED, "the meshes of one batch hold more than 2^30 points");
    }
    PET_TRY(ew_upload(&mp->d_sys, mp->sys));
    PET_TRY(ew_upload(&mp->d_mtiles, mp->mtiles));
    PET_TRY(ew_upload(&mp->d_stiles, mp->stiles));
    PET_HIP_CHECK(hipMalloc(&mp->d_infl, (size_t)std::max<int64_t>(mp->s_total, 1) * sizeof(float)));
    for (size_t s = 0; s < (size_t)n_systems; s++) {
        const P3mSysD& m = mp->sys[s];
        const int count = m.n[0] * m.n[1] * m.nzh;
        if (count > 0) k_p3m_influence<<<cdiv(count, 256), 256>>>(m, sigma, nodes, count, mp->d_infl);
    }
    PET_HIP_CHECK(hipGetLastError());
    PET_HIP_CHECK(hipDeviceSynchronize());
    guard.p = nullptr;
    *out = mp;
    return PET_OK;
}

}  // namespace pet

extern "C" {

int pet_ewald_set_p3m(pet_ewald_t* e, int32_t interpolation_nodes) {
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(interpolation_nodes >= 1 && interpolation_nodes <= 5, PET_ERR_ARGUMENT,
                "interpolation_nodes must be 1..5, got " + std::to_string(interpolation_nodes));
    PET_REQUIRE(!e->planned, PET_ERR_ARGUMENT, "pet_ewald_set_p3m must come before pet_ewald_plan");
    e->p3m_nodes = interpolation_nodes;
    return PET_OK;
}

int pet_p3m_mesh_shape_host(const double* h_cell, double spacing, int32_t* out) {
    if (!h_cell || !out || !(spacing > 0.0) || !std::isfinite(spacing)) return -1;
    double inv[9], vol;
    if (!ew_cell_inverse(h_cell, inv, &vol)) return -1;
    int n[3];
    p3m_mesh_shape(h_cell, spacing, n);
    for (int a = 0; a < 3; a++) out[a] = n[a];
    return 0;
}

int64_t pet_p3m_influence_host(const double* h_cell, double smearing, double spacing, int32_t interpolation_nodes,
                               double* h_out, int64_t capacity) {
    if (!h_cell || !(spacing > 0.0) || !(smearing > 0.0) || interpolation_nodes < 1 || interpolation_nodes > 5) return -1;
    double inv[9], vol;
    if (!ew_cell_inverse(h_cell, inv, &vol)) return -1;
    int N[3];
    p3m_mesh_shape(h_cell, spacing, N);
    const int nzh = N[2] / 2 + 1;
    const int64_t count = (int64_t)N[0] * N[1] * nzh;
    if (h_out && capacity >= count)
        for (int ix = 0; ix < N[0]; ix++)
            for (int iy = 0; iy < N[1]; iy++)
                for (int iz = 0; iz < nzh; iz++) {
                    const int n[3] = {p3m_signed(ix, N[0]), p3m_signed(iy, N[1]), p3m_signed(iz, N[2])};
                    h_out[((int64_t)ix * N[1] + iy) * nzh + iz] = p3m_influence_point(inv, vol, N, n, smearing, interpolation_nodes, nullptr);
                }
    return count;
}

int pet_p3m_mesh_shape(const pet_ewald_t* e, int64_t system, int32_t* out) {
    PET_REQUIRE(e && out, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes != 0 && e->planned && e->p3m, PET_ERR_ARGUMENT, "pet_p3m_mesh_shape needs a planned P3M-mode handle");
    PET_REQUIRE(system >= 0 && system < e->n_systems, PET_ERR_ARGUMENT, "no such system");
    for (int a = 0; a < 3; a++) out[a] = e->p3m->sys[(size_t)system].n[a];
    return PET_OK;
}

int64_t pet_p3m_mesh_elements(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || !e->p3m || n_channels < 1) return -1;
    return e->p3m->m_total * n_channels;
}

int64_t pet_p3m_spectrum_elements(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || !e->p3m || n_channels < 1) return -1;
    return e->p3m->s_total * n_channels;
}

int64_t pet_p3m_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || !e->p3m || n_channels < 1) return -1;
    P3mWs w;
    return (int64_t)p3m_carve(e, n_channels, nullptr, w);
}

int pet_p3m_spread(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges, int32_t C,
                   float* d_mesh, void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = p3m_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    if (e->n_atoms == 0) return PET_OK;
    PET_REQUIRE(d_positions && d_charges, PET_ERR_ARGUMENT, "null argument");
    const P3mPlan* mp = e->p3m;
    PET_REQUIRE(d_mesh || mp->m_total == 0, PET_ERR_ARGUMENT, "no mesh buffer (pet_p3m_mesh_elements)");
    hipStream_t st = (hipStream_t)stream;
    P3mWs w;
    p3m_carve(e, C, d_workspace, w);
    ProfScope ps("p3m_spread", st, 0.0, 0.0);
    PET_TRY(p3m_bin(e, pg->g, d_positions, w, st));
    p3m_spread(e, d_charges, C, w, d_mesh, st);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_p3m_filter(const pet_ewald_t* e, int32_t C, void* d_spectrum, void* stream) {
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes != 0, PET_ERR_ARGUMENT,
                "a pet_p3m_* entry point on an Ewald-mode handle: call pet_ewald_set_p3m before pet_ewald_plan");
    PET_REQUIRE(e->planned && e->p3m, PET_ERR_ARGUMENT, "pet_ewald_plan has not been called");
    PET_REQUIRE(C >= 1, PET_ERR_ARGUMENT, "n_channels must be at least 1");
    const P3mPlan* mp = e->p3m;
    if (mp->stiles.empty()) return PET_OK;
    PET_REQUIRE(d_spectrum, PET_ERR_ARGUMENT, "no spectrum buffer (pet_p3m_spectrum_elements)");
    hipStream_t st = (hipStream_t)stream;
    k_p3m_filter<<<dim3((unsigned)mp->stiles.size(), (unsigned)std::min(C, 256)), 256, 0, st>>>(
        mp->d_stiles, mp->d_sys, mp->d_infl, C, (float2*)d_spectrum);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_p3m_finish(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges, int32_t C,
                   const float* d_mesh_potential, float* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = p3m_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    if (e->n_atoms == 0) return PET_OK;
    PET_REQUIRE(d_positions && d_charges && d_out, PET_ERR_ARGUMENT, "null argument");
    const P3mPlan* mp = e->p3m;
    PET_REQUIRE(d_mesh_potential || mp->m_total == 0, PET_ERR_ARGUMENT, "no mesh buffer (pet_p3m_mesh_elements)");
    hipStream_t st = (hipStream_t)stream;
    P3mWs w;
    p3m_carve(e, C, d_workspace, w);
    ProfScope ps("p3m_finish", st, 0.0, 0.0);
    return p3m_finish(e, pg->g, d_positions, d_charges, C, d_mesh_potential, d_out, w, st);
}

int pet_p3m_backward(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                     const float* d_grad_potential, int32_t C, const float* d_phi_q, const float* d_phi_g,
                     const void* d_spec_q, const void* d_spec_g, float* d_grad_positions, float* d_grad_cells,
                     void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = p3m_check(e, pg, C, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Graph& g = pg->g;
    if (e->n_atoms == 0) return ew_backward_empty(e, d_grad_cells, st);
    PET_REQUIRE(d_positions && d_charges && d_grad_potential && d_grad_positions, PET_ERR_ARGUMENT, "null argument");
    const P3mPlan* mp = e->p3m;
    PET_REQUIRE(mp->m_total == 0 || (d_phi_q && d_phi_g), PET_ERR_ARGUMENT, "no mesh potentials (pet_p3m_mesh_elements)");
    PET_REQUIRE(!d_grad_cells || mp->s_total == 0 || (d_spec_q && d_spec_g), PET_ERR_ARGUMENT,
                "dL/dcell needs the unfiltered half spectra of q and of dL/dV (pet_p3m_spectrum_elements)");
    P3mWs w;
    p3m_carve(e, C, d_workspace, w);
    ProfScope ps("p3m_bwd", st, 0.0, 0.0);
    if (d_grad_cells) {  // (k_ew_cell alone reads the column sums)
        const unsigned cy = (unsigned)cdiv(C, 256);
        k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, d_charges, C, w.loc.sum_q);
        k_ew_colsum<<<dim3((unsigned)e->n_systems, cy), 256, 0, st>>>(e->d_sys, d_grad_potential, C, w.loc.sum_g);
    }
    p3m_force(e, g, w, d_phi_q, d_phi_g, d_grad_potential, d_charges, C, st);
    return ew_local_backward(e, g, d_positions, d_charges, d_grad_potential, C, w.loc, d_grad_positions, d_grad_cells, st, [&] {
        if (!mp->stiles.empty())
            k_p3m_cell<<<(unsigned)mp->stiles.size(), 256, 0, st>>>(mp->d_stiles, mp->d_sys, (const float2*)d_spec_q,
                                                                   (const float2*)d_spec_g, C, e->sigma, e->p3m_nodes, w.loc.kpart);
    });
}

int pet_p3m_set_transform(pet_ewald_t* e, pet_p3m_transform_fn fn, void* user) {
    PET_REQUIRE(e, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(e->p3m_nodes != 0, PET_ERR_ARGUMENT,
                "a pet_p3m_* entry point on an Ewald-mode handle: call pet_ewald_set_p3m before pet_ewald_plan");
    e->p3m_transform = fn;
    e->p3m_transform_user = fn ? user : nullptr;
    return PET_OK;
}

int64_t pet_p3m_second_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || !e->p3m || n_channels < 1) return -1;
    return p3m_workspace_bytes(e, (int)n_channels, false);
}

int pet_p3m_second(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                   const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions, int32_t C,
                   float* d_out_charges, float* d_out_grad_potential, float* d_out_positions, void* d_workspace,
                   int64_t workspace_bytes, void* stream) {
    bool run;
    PET_TRY(ew_second_check(e, pg, C, "pet_p3m_second", true, false, d_u_charges || d_u_positions, d_workspace, workspace_bytes,
                            d_positions && d_charges && d_grad_potential,
                            d_out_charges || d_out_grad_potential || d_out_positions, "all three results are NULL", &run));
    if (!run) return PET_OK;
    return p3m_second(LrCall{e, &pg->g, d_positions, C, d_workspace, 0, (hipStream_t)stream}, d_charges, d_grad_potential,
                      d_u_charges, d_u_positions, nullptr, d_out_charges, d_out_grad_potential, d_out_positions);
}

int64_t pet_p3m_second_cell_workspace_bytes(const pet_ewald_t* e, int64_t n_channels) {
    if (!e || !e->planned || !e->p3m || n_channels < 1) return -1;
    return p3m_workspace_bytes(e, (int)n_channels, true);
}

int pet_p3m_second_cell(const pet_ewald_t* e, const pet_graph_t* pg, const float* d_positions, const float* d_charges,
                        const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions,
                        const float* d_u_cells, int32_t C, float* d_out_charges, float* d_out_grad_potential, void* d_workspace,
                        int64_t workspace_bytes, void* stream) {
    bool run;
    PET_TRY(ew_second_check(e, pg, C, "pet_p3m_second_cell", true, true, d_u_charges || d_u_positions || d_u_cells, d_workspace,
                            workspace_bytes, d_positions && d_charges && d_grad_potential, d_out_charges || d_out_grad_potential,
                            "both results are NULL", &run));
    if (!run) return PET_OK;
    return p3m_second(LrCall{e, &pg->g, d_positions, C, d_workspace, 0, (hipStream_t)stream}, d_charges, d_grad_potential,
                      d_u_charges, d_u_positions, d_u_cells, d_out_charges, d_out_grad_potential, nullptr);
}

}  // extern "C"
