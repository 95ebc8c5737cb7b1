// What the translation units of the SOAP-BPNN pass share: the model and its dimensions, the workspace, the per-pair device
// building blocks (spherical harmonics, radial splines, cutoff) and block reductions that more than one file uses, and the
// host entry points of each file. soap.hip has the model, the plan (soap_plan.h) and the two drivers; soap_expand.hip,
// soap_ps.hip and soap_tail.hip one stage each, both generations and the adjoints, with the stage's launchers;
// soap_train.hip the training pass; soap_hvp.hip the Hessian-vector product; soap_llpr.hip the last-layer features and the
// soap_llpr_* entry points.
#pragma once
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/soap_hip.h"
#include "common.h"
#include "model.h"
#include "tile.h"

namespace pet {

// pet_bwd.hip (shared geometry adjoint: dE/dR_a = sum_{p in row a} (dv[rev p] - dv[p]), dE/dcell)
__global__ void k_pos_grad(const float4* __restrict__ dv, const int* __restrict__ rowptr, const int* __restrict__ rev,
                           float* __restrict__ gpos, int N);
__global__ void k_cell_grad(const float4* __restrict__ dv, const int* __restrict__ shift, const int* __restrict__ ctr,
                            const int* __restrict__ sys, const int* __restrict__ rowptr, float* __restrict__ gcell,
                            int N, int64_t E, int accumulate);

// abi.hip
__global__ void k_pack(const float* __restrict__ W, int64_t s_n, int64_t s_k, int n_out, int k_in,
                       float4* __restrict__ out);
constexpr int MAXL = SOAP_MAX_L;
constexpr int PC = 32;  // pairs per LDS chunk

struct SoapDims {
    int L, C, F, NLM, NCOEF, ITEMS, S, H, NH, ns, legacy, layernorm, n_grid;
    int n_per_l[MAXL + 1], rad_off[MAXL + 1], coef_off[MAXL + 2], feat_off[MAXL + 2];
    int ncmax;             // largest n_per_l[l] * C
    // packed power spectrum (round 6): p_l[a][b] = p_l[b][a], so the inference path stores the upper triangle a <= b of every
    // l block only -- Sp = sum_l nc (nc + 1) / 2 floats per atom instead of S = sum_l nc^2 (2 360 against 4 544 for the default
    // basis) -- at pfeat_off[l] + a nc - a (a - 1) / 2 + (b - a); the first Linear and the LayerNorm are folded accordingly
    // (k_soap_prep_wallp). Halves the feature traffic of the four kernels that stream [N][S].
    int Sp, pfeat_off[MAXL + 2];
    float rc, width, inv_h;
};
__host__ __device__ __forceinline__ int soap_tri(int nc, int lo, int hi) { return lo * nc - lo * (lo - 1) / 2 + (hi - lo); }

constexpr int MAXNH = 8;  // hidden layers of the tail (soap_bpnn/documentation.py: num_hidden_layers, default 2)
struct SoapSet {  // weights of one (centre-species) set
    const float *ln_w = nullptr, *ln_b = nullptr, *W1 = nullptr, *W2 = nullptr, *w3 = nullptr;
    const float* Wh[MAXNH - 1] = {};  // hidden Linear k + 2 of the stack ("bpnn.<s>.<2 (k + 1)>.weight"); Wh[0] == W2
};

struct SoapModel {
    soap_hypers_t h;
    SoapDims d;
    std::map<std::string, std::pair<float*, int64_t>> raw;
    // training (soap_train.hip): gradient slot and Adam moments of every trainable parameter, keyed like `raw`
    std::map<std::string, std::pair<float*, int64_t>> grad;
    std::map<std::string, float*> adam_m, adam_v;
    std::vector<void*> owned;
    float* table = nullptr;      // [n_grid][F][2]
    float* curv = nullptr;       // [n_grid][F][2] curvature slopes of the radial spline (radial_two), or null: no second order
    float* shnorm = nullptr;     // [(L+1)*(L+1)] normalisation (sqrt 2 folded in for m > 0)
    int* coef_lut = nullptr;     // [NCOEF] lm | rn << 8 | a << 16
    int* item_lut = nullptr;     // [ITEMS] lm | rn << 8 | base << 16
    int2* feat_lut = nullptr;    // [S]     coefficient offsets of c[.][a], c[.][b] | M << 16 | nc << 24
    int2* out_lut = nullptr;     // [NCOEF] offset of G[0][a] in the feature row, offset of c[m][0] | nc << 16
    float* species_w = nullptr;  // [ns, C]
    const float* enc = nullptr;  // [ns, S] or null
    SoapSet* sets = nullptr;     // device array [n_sets]
    int n_sets = 0;
    // MFMA tail: all sets' first Linear stacked (LayerNorm weight folded in), zero padded to [NOUTP][Kp]
    int NT = 0, NOUTP = 0, Kp = 0;
    float* wall = nullptr;       // [NOUTP][Kp]
    float4 *wall_fwd = nullptr, *wall_bwd = nullptr;
    float *wall_rs = nullptr, *wall_b = nullptr;  // [NOUTP] row sums, W1 beta
    float4 *wall_fwd_set = nullptr, *wall_bwd_set = nullptr;  // per network: [n_sets][1][Kp/8][64], [n_sets][Kp/32][4][64]
    // packed power spectrum (SoapDims::Sp): the first Linear of every network over the upper-triangle layout,
    // W'[j][(a, b)] = gamma W1[j][(a, b)] + gamma W1[j][(b, a)] (a < b), for the adjoint with the diagonal doubled
    int Kpp = 0;
    float *wallp = nullptr, *wallpb = nullptr;
    float4 *wallp_fwd_set = nullptr, *wallp_bwd_set = nullptr;
    bool finalized = false;
};

inline int salloc(SoapModel& m, void** p, size_t bytes) {
    PET_HIP_CHECK(hipMalloc(p, bytes > 0 ? bytes : 4));
    m.owned.push_back(*p);
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// per-pair building blocks
// ---------------------------------------------------------------------------------------------
// Orthonormal real spherical harmonics of a unit vector (x, y, z), Y[l*l + l + m], by the standard recurrences
//   c_m + i s_m = (x + i y)^m,   Q_m^m = (-1)^m (2m-1)!!,   Q_{m+1}^m = (2m+1) z Q_m^m,
//   Q_l^m = ((2l-1) z Q_{l-1}^m - (l+m-1) Q_{l-2}^m) / (l-m),     Y_l^{+-m} = F_lm Q_l^m {c_m | s_m}
// (shn[l*(L+1)+m] = F_lm, with sqrt(2) folded in for m > 0), and the gradient of their polynomial extension
// by differentiating the recurrences.
// One m-chain (all l >= m for one pair): the per-pair work is split over (pair, m) threads.
__device__ __forceinline__ void sh_chain(float x, float y, float z, int m, int L, const float* __restrict__ shn,
                                         float* Y, float* Gx, float* Gy, float* Gz, float ir) {
    float cm = 1.f, sm = 0.f, cp = 1.f, sp_ = 0.f;  // (c_m, s_m) and (c_{m-1}, s_{m-1})
    float qmm = 1.f;
    for (int k = 1; k <= m; k++) {
        cp = cm; sp_ = sm;
        cm = x * cp - y * sp_;
        sm = x * sp_ + y * cp;
        qmm *= -(2 * k - 1);
    }
    float q2 = 0.f, dq2 = 0.f, q1 = qmm, dq1 = 0.f;
    for (int l = m; l <= L; l++) {
        float q, dq;
        if (l == m) { q = qmm; dq = 0.f; }
        else if (l == m + 1) { q = (2 * m + 1) * z * q1; dq = (2 * m + 1) * q1; }
        else {
            const float inv = 1.0f / (l - m);
            q = ((2 * l - 1) * z * q1 - (l + m - 1) * q2) * inv;
            dq = ((2 * l - 1) * (q1 + z * dq1) - (l + m - 1) * dq2) * inv;
        }
        const float f = shn[l * (L + 1) + m];
        const int ip = l * l + l + m, im = l * l + l - m;
        // value and gradient of the polynomial extension, then the chain through u = v / r: (I - u u^T) / r
        float yv[2], gx[2], gy[2], gz[2];
        if (m == 0) {
            yv[0] = f * q; gx[0] = 0.f; gy[0] = 0.f; gz[0] = f * dq;
        } else {
            const float fm = f * q * m;
            yv[0] = f * q * cm; gx[0] = fm * cp;  gy[0] = -fm * sp_; gz[0] = f * dq * cm;
            yv[1] = f * q * sm; gx[1] = fm * sp_; gy[1] = fm * cp;   gz[1] = f * dq * sm;
        }
        for (int k = 0; k < (m == 0 ? 1 : 2); k++) {
            const int idx = k == 0 ? ip : im;
            Y[idx] = yv[k];
            if (Gx) {
                const float dot = x * gx[k] + y * gy[k] + z * gz[k];
                Gx[idx] = (gx[k] - x * dot) * ir; Gy[idx] = (gy[k] - y * dot) * ir; Gz[idx] = (gz[k] - z * dot) * ir;
            }
        }
        if (l > m) { q2 = q1; dq2 = dq1; }
        q1 = q; dq1 = dq;
        if (l == m) { q2 = 0.f; dq2 = 0.f; }
    }
}

// Hermite spline of radial function f at distance r: R fc and (optionally) d(R fc)/dr
__device__ __forceinline__ void radial_one(const SoapDims& d, const float* __restrict__ table, int f, float r, float fc,
                                           float dfc, float* R, float* dR) {
    float t = r * d.inv_h;
    int k = (int)t;
    if (k > d.n_grid - 2) k = d.n_grid - 2;
    const float s = t - k, h = 1.0f / d.inv_h;
    const float s2 = s * s, om = 1.f - s;
    const float h00 = (1.f + 2.f * s) * om * om, h10 = s * om * om, h01 = s2 * (3.f - 2.f * s), h11 = s2 * (s - 1.f);
    // table entry: (R, dR/dr, chord slope (R[k+1] - R[k]) / h, 0). The derivative of the Hermite cubic needs the chord
    // slope; taken from the fp32 node values it is a difference of two numbers 2e-3 relative apart times 1 / h = 410:
    // 4e-5 |R| of rounding noise in dR/dr, which showed as 1.1e-5 .. 1.5e-5 in dE/dR of dilute systems (round-2 sweep,
    // tests/debug/fuzz_soap.py). The host computes it in fp64.
    const float4 a = reinterpret_cast<const float4*>(table)[(size_t)k * d.F + f];
    const float4 b = reinterpret_cast<const float4*>(table)[(size_t)(k + 1) * d.F + f];
    const float v = h00 * a.x + h10 * h * a.y + h01 * b.x + h11 * h * b.y;
    *R = v * fc;
    if (dR) {
        const float g00 = 6.f * s2 - 6.f * s, g10 = 3.f * s2 - 4.f * s + 1.f, g11 = 3.f * s2 - 2.f * s;
        const float dv = g10 * a.y + g11 * b.y - g00 * a.z;
        *dR = dv * fc + v * dfc;
    }
}

__device__ __forceinline__ float shifted_cosine(float r, float rc, float w, float* dfc) {
    float s = (r - (rc - w)) / w;
    if (r >= rc) { if (dfc) *dfc = 0.f; return 0.f; }
    if (s <= 0.f) { if (dfc) *dfc = 0.f; return 1.f; }
    if (dfc) *dfc = -0.5f * 3.14159274f * sinf(3.14159274f * s) / w;
    return 0.5f * (1.0f + cosf(3.14159274f * s));
}

// ---------------------------------------------------------------------------------------------
// second-order forms (soap_hvp.hip): the same blocks with their derivative along a direction v' of the pair vector
// ---------------------------------------------------------------------------------------------
// sh_chain in forward mode along v': besides Y and G = grad Y (w.r.t. the pair vector v, through u = v / r) it returns
// Y' = G . v' and G' = (grad grad Y) v', the derivative of G along v' -- three tangent components per lm, never the 3 x 3
// Hessian of Y. (xd, yd, zd) = u' = (v' - u (u . v')) / r and ird = (1 / r)' = -(u . v') / r^2 are the tangents of the
// chain's inputs; every recurrence of sh_chain is carried as a (value, tangent) pair, and the polynomial Q_l^m gets its
// second z derivative by differentiating the recurrence once more. r = 0: ir = 0 and all tangents 0 (the caller's guard).
__device__ __forceinline__ void sh_chain2(float x, float y, float z, float xd, float yd, float zd, int m, int L,
                                          const float* __restrict__ shn, float* Y, float* Yd, float* Gx, float* Gy,
                                          float* Gz, float* Gxd, float* Gyd, float* Gzd, float ir, float ird) {
    float cm = 1.f, sm = 0.f, cp = 1.f, sp_ = 0.f;      // (c_m, s_m) and (c_{m-1}, s_{m-1})
    float cmd = 0.f, smd = 0.f, cpd = 0.f, spd = 0.f;   // their tangents
    float qmm = 1.f;
    for (int k = 1; k <= m; k++) {
        cp = cm; sp_ = sm; cpd = cmd; spd = smd;
        cm = x * cp - y * sp_;
        sm = x * sp_ + y * cp;
        cmd = xd * cp + x * cpd - yd * sp_ - y * spd;
        smd = xd * sp_ + x * spd + yd * cp + y * cpd;
        qmm *= -(2 * k - 1);
    }
    float q2 = 0.f, dq2 = 0.f, ddq2 = 0.f, q1 = qmm, dq1 = 0.f, ddq1 = 0.f;
    for (int l = m; l <= L; l++) {
        float q, dq, ddq;
        if (l == m) { q = qmm; dq = 0.f; ddq = 0.f; }
        else if (l == m + 1) { q = (2 * m + 1) * z * q1; dq = (2 * m + 1) * q1; ddq = 0.f; }
        else {
            const float inv = 1.0f / (l - m);
            q = ((2 * l - 1) * z * q1 - (l + m - 1) * q2) * inv;
            dq = ((2 * l - 1) * (q1 + z * dq1) - (l + m - 1) * dq2) * inv;
            ddq = ((2 * l - 1) * (2.f * dq1 + z * ddq1) - (l + m - 1) * ddq2) * inv;
        }
        const float qt = dq * zd, dqt = ddq * zd;   // tangents of q and dq: both depend on z alone
        const float f = shn[l * (L + 1) + m];
        const int ip = l * l + l + m, im = l * l + l - m;
        float yv[2], gx[2], gy[2], gz[2], yt[2], gxt[2], gyt[2], gzt[2];
        if (m == 0) {
            yv[0] = f * q; gx[0] = 0.f; gy[0] = 0.f; gz[0] = f * dq;
            yt[0] = f * qt; gxt[0] = 0.f; gyt[0] = 0.f; gzt[0] = f * dqt;
        } else {
            const float fm = f * q * m, fmt = f * qt * m;
            yv[0] = f * q * cm; gx[0] = fm * cp;  gy[0] = -fm * sp_; gz[0] = f * dq * cm;
            yv[1] = f * q * sm; gx[1] = fm * sp_; gy[1] = fm * cp;   gz[1] = f * dq * sm;
            yt[0] = f * (qt * cm + q * cmd); gxt[0] = fmt * cp + fm * cpd;  gyt[0] = -(fmt * sp_ + fm * spd);
            yt[1] = f * (qt * sm + q * smd); gxt[1] = fmt * sp_ + fm * spd; gyt[1] = fmt * cp + fm * cpd;
            gzt[0] = f * (dqt * cm + dq * cmd);
            gzt[1] = f * (dqt * sm + dq * smd);
        }
        for (int k = 0; k < (m == 0 ? 1 : 2); k++) {
            const int idx = k == 0 ? ip : im;
            Y[idx] = yv[k];
            Yd[idx] = yt[k];
            // G = (g - u (u . g)) / r and its tangent
            const float dot = x * gx[k] + y * gy[k] + z * gz[k];
            const float dott = xd * gx[k] + yd * gy[k] + zd * gz[k] + x * gxt[k] + y * gyt[k] + z * gzt[k];
            const float px = gx[k] - x * dot, py = gy[k] - y * dot, pz = gz[k] - z * dot;
            Gx[idx] = px * ir; Gy[idx] = py * ir; Gz[idx] = pz * ir;
            Gxd[idx] = (gxt[k] - xd * dot - x * dott) * ir + px * ird;
            Gyd[idx] = (gyt[k] - yd * dot - y * dott) * ir + py * ird;
            Gzd[idx] = (gzt[k] - zd * dot - z * dott) * ir + pz * ird;
        }
        if (l > m) { q2 = q1; dq2 = dq1; ddq2 = ddq1; }
        q1 = q; dq1 = dq; ddq1 = ddq;
        if (l == m) { q2 = 0.f; dq2 = 0.f; ddq2 = 0.f; }
    }
}

// second derivative of the cutoff factor: fc'' = -(pi^2 / 2 w^2) cos(pi s) inside the taper, 0 outside
__device__ __forceinline__ float shifted_cosine_dd(float r, float rc, float w) {
    const float s = (r - (rc - w)) / w;
    if (r >= rc || s <= 0.f) return 0.f;
    return -0.5f * 3.14159274f * 3.14159274f * cosf(3.14159274f * s) / (w * w);
}

// radial_one to second order: R fc, (R fc)' and (R fc)'' = p'' fc + 2 p' fc' + p fc''. p and p' are radial_one's own
// arithmetic (fc = 1, fc' = 0 hands them out unscaled); p''(s) = (4 - 6 s) d0 + (6 s - 2) d1 is the exact derivative of that
// p', with the interval's curvature slopes d0 = (chord - m_k) / h, d1 = (m_{k+1} - chord) / h from the second table
// [n_grid][F][2], which the host forms in fp64 (radial.curvature_table: formed from the fp32 table they would be rounding
// noise divided by h twice).
__device__ __forceinline__ void radial_two(const SoapDims& d, const float* __restrict__ table, const float* __restrict__ curv,
                                           int f, float r, float fc, float dfc, float ddfc, float* R, float* dR, float* ddR) {
    float p, dp;
    radial_one(d, table, f, r, 1.f, 0.f, &p, &dp);
    const float t = r * d.inv_h;
    int k = (int)t;
    if (k > d.n_grid - 2) k = d.n_grid - 2;
    const float s = t - k;
    const float2 c = reinterpret_cast<const float2*>(curv)[(size_t)k * d.F + f];
    const float ddp = (4.f - 6.f * s) * c.x + (6.f * s - 2.f) * c.y;
    *R = p * fc;
    *dR = dp * fc + p * dfc;
    *ddR = ddp * fc + 2.f * dp * dfc + p * ddfc;
}

constexpr int MAXK = 12;  // coefficients per thread (NCOEF <= 256 * MAXK)
constexpr int MAXI = 8;   // (lm, n) items per lane of the wave expansion (ITEMS <= 64 * MAXI)

__device__ __forceinline__ float block_sum(float v, float* red /*[8]*/) {
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float silu(float x) { return x * sigm(x); }
__device__ __forceinline__ float dsilu(float x) { const float s = sigm(x); return s * (1.0f + x * (1.0f - s)); }
constexpr int MAXH = 64;  // neurons per hidden layer; the MFMA tails serve 32 (the default), other widths the per-atom kernels

constexpr int SP_MAXSETS = 8;         // networks of the species-sorted tiles (soap_sorted_ok; m.NT is built up to 8)
constexpr int SP_TRAIN_MAXSETS = 16;  // networks of the training pass's bucket table (soap_train.hip; refused beyond)
// The bucket table and the k_sp_* kernels are sized by MS at compile time: the forward keeps MS = 8 (eight ballots per
// atom in k_sp_fill), the training pass of a model with more networks takes MS = 16. An atom of a network >= MS would
// index every array here out of range, so each host path checks n_sets <= MS before the first launch.
template <int MS>
struct SpInfoT {  // device-side bucket table
    int count[MS], cursor[MS], offs[MS + 1], tstart[MS + 1];
};
using SpInfo = SpInfoT<SP_MAXSETS>;

struct SoapWs {
    float *Cf, *feats, *tail, *dF, *dCf, *dv;
    float *tail_ext, *da2;  // num_hidden_layers > 2: a3 .. a_NH [N][NH - 2][H] and the adjoint of a2 [N][H]
    int* perm;     // [N] atoms bucketed by network (species-sorted tail tiles)
    SpInfo* info;
    size_t bytes;
};
inline void carve_soap(const SoapDims& d, int64_t N, int64_t E, void* base, SoapWs& w) {
    Carver c(base);
    const int64_t Na = N > 0 ? N : 1, Ea = E > 0 ? E : 1;
    w.Cf = c.take<float>(Na * d.NCOEF);
    w.feats = c.take<float>(Na * d.S);
    w.tail = c.take<float>(Na * (2 + 2 * d.H));
    w.dF = c.take<float>(Na * d.S);
    w.dCf = c.take<float>(Na * d.NCOEF);
    w.dv = c.take<float>(Ea * 4);
    w.perm = c.take<int>(Na);
    w.info = reinterpret_cast<SpInfo*>(c.take<int>((sizeof(SpInfo) + 3) / 4));
    w.tail_ext = c.take<float>(d.NH > 2 ? Na * (d.NH - 2) * d.H : 1);
    w.da2 = c.take<float>(d.NH > 2 ? Na * d.H : 1);
    w.bytes = c.off;
}

// ---------------------------------------------------------------------------------------------
// One launcher per stage, next to its kernels. Each takes the plan (soap_plan.h), computes the dynamic-LDS size, opts its
// kernel in above 64 KB and holds the stage's ProfScope; none of them chooses. (allow_big_lds only on the path that launches
// the kernel: hipFuncSetAttribute changes no result, and a call that is not made cannot leave an error behind.)
// ---------------------------------------------------------------------------------------------
// soap_expand.hip: w.Cf from the graph's pairs; w.dv from w.dCf
void launch_soap_expand(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st);
void launch_soap_expand_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st);
// soap_ps.hip: w.feats (+ the LayerNorm statistics in w.tail) from w.Cf; w.dCf from w.dF
void launch_soap_ps(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st);
void launch_soap_ps_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st);
// the full-layout power spectrum on the matrix core (k_soap_ps_m<false>) by itself: the Mfma form of launch_soap_ps, and the
// training pass's rebuild of the full layout behind a packed forward
void soap_ps_full(const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st);
// soap_tail.hip: energies from w.feats (a Sorted plan buckets the atoms first; a deep tail continues per atom); w.dF from gA
int launch_soap_tail(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, float* atomic, hipStream_t st);
void launch_soap_tail_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, const float* gA,
                          hipStream_t st);
// atoms bucketed by network into perm, on the forward's table of SP_MAXSETS networks or (wide) the training pass's of
// SP_TRAIN_MAXSETS; *offs = the table's offs[n_sets + 1] (device pointer)
int soap_bucket(bool wide, const int* sp, int legacy, int N, int n_sets, void* info, int* perm, const int** offs,
                hipStream_t st);
// the folded forms of the networks' first Linear (soap_finalize launches them)
__global__ void k_soap_prep_wall(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int NOUTP, int Kp,
                                 float* __restrict__ wall);
__global__ void k_soap_prep_rows(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int NOUTP, int Kp,
                                 const float* __restrict__ wall, float* __restrict__ rs, float* __restrict__ bs);
__global__ void k_soap_prep_wallp(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int Kpp, int diag2,
                                  float* __restrict__ wallp);

// soap.hip
int soap_finalize(SoapModel& m, hipStream_t st);

// soap_train.hip
int64_t soap_train_ws_bytes(const SoapModel& m, int64_t n_nodes, int64_t n_edges);
int soap_zero_grad(SoapModel& m, hipStream_t st);
int soap_train_grads(SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, void* tws, int64_t tws_bytes, const float* gA,
                     const float* u, const float* ucell, float* tangent_atomic, hipStream_t st);
int soap_adam(SoapModel& m, float lr, float b1, float b2, float eps, int64_t step, hipStream_t st);
// kernels of the training pass that the Hessian-vector product launches too (the same sweep with gA = 0, carried on to the pairs)
__global__ void k_edge_tangent(const float* __restrict__ u, const int* __restrict__ ctr, const int* __restrict__ nbr,
                               const int* __restrict__ shift, const int* __restrict__ sys, const float* __restrict__ ucell,
                               float4* __restrict__ vd, int64_t E);
__global__ __launch_bounds__(256) void k_soap_expand_jvp(SoapDims d, const float4* __restrict__ geo, const float4* __restrict__ vdot,
                                  const int* __restrict__ rowptr, const int* __restrict__ sp_nbr,
                                  const float* __restrict__ table, const float* __restrict__ shn,
                                  const int* __restrict__ lut, const float* __restrict__ spw, float* __restrict__ Cd);
__global__ __launch_bounds__(256) void k_soap_ps_jvp(SoapDims d, const float* __restrict__ Cf, const float* __restrict__ Cd,
                              const int* __restrict__ sp, const float* __restrict__ enc, const int2* __restrict__ flut,
                              float* __restrict__ xd);
__host__ __device__ inline int soap_pack_size(int H, int NH) { return 4 + 4 * H * NH; }
__global__ __launch_bounds__(256) void k_soap_tail_train(SoapDims d, const float* __restrict__ feats, const float* __restrict__ xd /* may be null */,
                                  const int* __restrict__ sp, const SoapSet* __restrict__ sets,
                                  const float* __restrict__ gA /* null: zeros */, float seed_tangent,
                                  float* __restrict__ pack, float* __restrict__ edot);
__global__ __launch_bounds__(256) void k_soap_ps_rev2(SoapDims d, const float* __restrict__ Cf, const float* __restrict__ Cd,
                               const float* __restrict__ NP, const float* __restrict__ LP, float* __restrict__ NC,
                               float* __restrict__ LC);

// soap_hvp.hip
int64_t soap_hvp_ws_bytes(const SoapModel& m, int64_t n_nodes, int64_t n_edges);
int soap_hvp(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, void* hws, int64_t hws_bytes, const float* u,
             const float* ucell, float* hvp_pos, float* hvp_cell, float* tangent_atomic, hipStream_t st);

// soap_llpr.hip: the last-layer features [N, F] (F = soap_llpr_width) from what the tail kernels left in the workspace
inline int soap_llpr_width(const SoapDims& d) { return d.legacy ? d.ns * d.H : d.H; }
int soap_llpr_feats(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, int back, float* llf, hipStream_t st);

}  // namespace pet

struct soap_model {  // (soap_model_t of include/soap_hip.h: the entry points of soap.hip and soap_llpr.hip)
    pet::SoapModel m;
};
