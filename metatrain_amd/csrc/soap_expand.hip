// SOAP-BPNN, spherical expansion and its adjoint, both generations, with their launchers:
//
//   c[i][l][m][n][a] = sum_{p in row i} Y_lm(r_p / |r_p|) R_nl(|r_p|) fc(|r_p|) w_a(species of neighbour)   (a17, spex)
//
// Everything is HBM / latency bound; per-pair quantities are staged in LDS or kept in registers, CSR rows give coalesced
// per-atom reads, reductions are fixed-order (no float atomics): bit-reproducible.
#include <type_traits>

#include "soap.h"

namespace pet {

// ---------------------------------------------------------------------------------------------
// a17: spherical expansion, one workgroup per atom
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_soap_expand(SoapDims d, const float4* __restrict__ geo,
                                                     const int* __restrict__ rowptr, const int* __restrict__ sp_nbr,
                                                     const float* __restrict__ table, const float* __restrict__ shn,
                                                     const int* __restrict__ lut, const float* __restrict__ spw,
                                                     float* __restrict__ Cf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ys = smem;                     // [PC][NLM]
    float* Rs = Ys + PC * d.NLM;          // [PC][F]
    float* us = Rs + PC * d.F;            // [PC][8] unit vector, r, 1/r, fc, dfc
    int* sps = reinterpret_cast<int*>(us + PC * 8);
    const int i = blockIdx.x, tid = threadIdx.x;
    const int p0 = rowptr[i], p1 = rowptr[i + 1];
    float acc[MAXK];
    int code[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; k++) {
        acc[k] = 0.f;
        const int idx = tid + 256 * k;
        code[k] = idx < d.NCOEF ? lut[idx] : -1;
    }
    for (int base = p0; base < p1; base += PC) {
        const int npc = min(PC, p1 - base);
        __syncthreads();
        if (tid < npc) {
            const float4 g = geo[base + tid];
            const float r = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
            const float ir = r > 0.f ? 1.0f / r : 0.f;
            float* u = us + tid * 8;
            u[0] = g.x * ir; u[1] = g.y * ir; u[2] = g.z * ir; u[3] = r; u[4] = ir;
            u[5] = shifted_cosine(r, d.rc, d.width, nullptr);
            sps[tid] = sp_nbr[base + tid];
        }
        __syncthreads();
        // per-pair quantities, spread over the workgroup: (pair, m) chains of Y_lm and (pair, f) spline values
        for (int idx = tid; idx < npc * (d.L + 1); idx += 256) {
            const int pp = idx / (d.L + 1), mm = idx % (d.L + 1);
            const float* u = us + pp * 8;
            sh_chain(u[0], u[1], u[2], mm, d.L, shn, Ys + pp * d.NLM, nullptr, nullptr, nullptr, 0.f);
        }
        for (int idx = tid; idx < npc * d.F; idx += 256) {
            const int pp = idx / d.F, f = idx % d.F;
            radial_one(d, table, f, us[pp * 8 + 3], us[pp * 8 + 5], 0.f, Rs + pp * d.F + f, nullptr);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAXK; k++) {
            if (code[k] < 0) continue;
            const int lm = code[k] & 255, rn = (code[k] >> 8) & 255, a = code[k] >> 16;
            float s = acc[k];
            for (int pp = 0; pp < npc; pp++) s += Ys[pp * d.NLM + lm] * Rs[pp * d.F + rn] * spw[sps[pp] * d.C + a];
            acc[k] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < MAXK; k++)
        if (code[k] >= 0) Cf[(size_t)i * d.NCOEF + tid + 256 * k] = acc[k];
}

// reverse of the expansion: dv[p] = d/d(edge vector) for every pair of the row
__global__ __launch_bounds__(256) void k_soap_expand_bwd(SoapDims d, const float4* __restrict__ geo,
                                                         const int* __restrict__ rowptr,
                                                         const int* __restrict__ sp_nbr,
                                                         const float* __restrict__ table,
                                                         const float* __restrict__ shn, const int* __restrict__ ilut,
                                                         const float* __restrict__ spw,
                                                         const float* __restrict__ dCf, float4* __restrict__ dv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dCs = smem;                       // [NCOEF]
    float* Ys = dCs + d.NCOEF;               // [PC][NLM] and three gradient components w.r.t. the edge vector
    float* Gx = Ys + PC * d.NLM;
    float* Gy = Gx + PC * d.NLM;
    float* Gz = Gy + PC * d.NLM;
    float* Rs = Gz + PC * d.NLM;             // [PC][F] R fc, d(R fc)/dr
    float* dRs = Rs + PC * d.F;
    float* us = dRs + PC * d.F;              // [PC][8] unit vector, r, 1/r, fc, dfc
    int* sps = reinterpret_cast<int*>(us + PC * 8);
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < d.NCOEF; k += 256) dCs[k] = dCf[(size_t)i * d.NCOEF + k];
    const int p0 = rowptr[i], p1 = rowptr[i + 1];
    for (int base = p0; base < p1; base += PC) {
        const int npc = min(PC, p1 - base);
        __syncthreads();
        if (tid < npc) {
            const float4 g = geo[base + tid];
            const float r = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
            const float ir = r > 0.f ? 1.0f / r : 0.f;
            float* u = us + tid * 8;
            u[0] = g.x * ir; u[1] = g.y * ir; u[2] = g.z * ir; u[3] = r; u[4] = ir;
            float dfc;
            u[5] = shifted_cosine(r, d.rc, d.width, &dfc);
            u[6] = dfc;
            sps[tid] = sp_nbr[base + tid];
        }
        __syncthreads();
        for (int idx = tid; idx < npc * (d.L + 1); idx += 256) {
            const int pp = idx / (d.L + 1), mm = idx % (d.L + 1);
            const float* u = us + pp * 8;
            sh_chain(u[0], u[1], u[2], mm, d.L, shn, Ys + pp * d.NLM, Gx + pp * d.NLM, Gy + pp * d.NLM, Gz + pp * d.NLM,
                     u[4]);
        }
        for (int idx = tid; idx < npc * d.F; idx += 256) {
            const int pp = idx / d.F, f = idx % d.F;
            const float* u = us + pp * 8;
            radial_one(d, table, f, u[3], u[5], u[6], Rs + pp * d.F + f, dRs + pp * d.F + f);
        }
        __syncthreads();
        for (int pp = wave; pp < npc; pp += 4) {
            const float* w = spw + sps[pp] * d.C;
            const float ux = us[pp * 8], uy = us[pp * 8 + 1], uz = us[pp * 8 + 2];
            float ax = 0.f, ay = 0.f, az = 0.f;
            for (int it = lane; it < d.ITEMS; it += 64) {
                const int code = ilut[it];
                const int lm = code & 255, rn = (code >> 8) & 255, cb = code >> 16;
                float A = 0.f;
                for (int a = 0; a < d.C; a++) A += dCs[cb + a] * w[a];
                const float y = Ys[pp * d.NLM + lm], rf = Rs[pp * d.F + rn], drf = dRs[pp * d.F + rn];
                const float radial = A * drf * y;   // along the unit vector
                const float ang = A * rf;
                ax += radial * ux + ang * Gx[pp * d.NLM + lm];
                ay += radial * uy + ang * Gy[pp * d.NLM + lm];
                az += radial * uz + ang * Gz[pp * d.NLM + lm];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); az += __shfl_xor(az, o);
            }
            if (lane == 0) dv[base + pp] = make_float4(ax, ay, az, 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// a17, second generation: no workgroup barriers, every lane busy.
//   k_soap_expand_w      one WAVE per atom: lanes 0..31 run the spherical-harmonic levels of one pair each, lanes
//                        32..63 that pair's radial splines, into wave-private LDS; then every lane owns up to
//                        MAXI (lm, n) items and sums them over the pairs with the C = 4 species channels as one
//                        float4 accumulator (the first generation looped 1120 scalar coefficients x pairs behind
//                        three __syncthreads, one workgroup per atom, and re-read the species weight from global).
//   k_soap_expand_bwd_p  one LANE per pair, flat over the CSR: the pair's Y_lm levels (with gradients) and splines
//                        stay in registers, dC rows of the centre atom come through L1 (the ~26 pairs of an atom
//                        sit in the same one or two waves), no LDS, no reduction, no barrier.
// Both need C == 4 (float4 channels; Alchemical default and 4-species legacy) and at most 64 * MAXI items;
// otherwise the plan (soap_plan.h) names the first-generation kernels (pet_config_set("soap_pair", 0) too).
// ---------------------------------------------------------------------------------------------

template <int LMAX>
struct ShLevels {  // the recurrences of sh_chain, all m-chains advanced one l at a time
    float x, y, z, ir;
    float cm[LMAX + 1], sm[LMAX + 1], q1[LMAX + 1], q2[LMAX + 1], dq1[LMAX + 1], dq2[LMAX + 1];
    __device__ __forceinline__ void init(float x_, float y_, float z_, float ir_) {
        x = x_; y = y_; z = z_; ir = ir_;
        cm[0] = 1.f; sm[0] = 0.f;
        float qmm = 1.f;
#pragma unroll
        for (int m = 0; m <= LMAX; m++) {
            if (m > 0) {
                cm[m] = x * cm[m - 1] - y * sm[m - 1];
                sm[m] = x * sm[m - 1] + y * cm[m - 1];
                qmm *= -(2 * m - 1);
            }
            q1[m] = qmm; q2[m] = 0.f; dq1[m] = 0.f; dq2[m] = 0.f;
        }
    }
    // level l (compile-time after unrolling): Y / G[mi], mi = l + m (cos) and l - m (sin)
    template <bool GRAD>
    __device__ __forceinline__ void level(int l, const float* __restrict__ shn, int L, float* Y, float* Gx, float* Gy,
                                          float* Gz) {
#pragma unroll
        for (int m = 0; m <= LMAX; m++) {
            if (m > l) continue;
            float q, dq;
            if (l == m) { q = q1[m]; dq = 0.f; }
            else if (l == m + 1) { q = (2 * m + 1) * z * q1[m]; dq = (2 * m + 1) * q1[m]; }
            else {
                const float inv = 1.0f / (l - m);
                q = ((2 * l - 1) * z * q1[m] - (l + m - 1) * q2[m]) * inv;
                dq = ((2 * l - 1) * (q1[m] + z * dq1[m]) - (l + m - 1) * dq2[m]) * inv;
            }
            const float f = shn[l * (L + 1) + m];
            if (m == 0) {
                Y[l] = f * q;
                if (GRAD) {
                    const float gz = f * dq, dot = z * gz;
                    Gx[l] = (-x * dot) * ir; Gy[l] = (-y * dot) * ir; Gz[l] = (gz - z * dot) * ir;
                }
            } else {
                const float fq = f * q, fm = fq * m, cp = cm[m - 1], sp = sm[m - 1];
                Y[l + m] = fq * cm[m];
                Y[l - m] = fq * sm[m];
                if (GRAD) {
                    float gx = fm * cp, gy = -fm * sp, gz = f * dq * cm[m];
                    float dot = x * gx + y * gy + z * gz;
                    Gx[l + m] = (gx - x * dot) * ir; Gy[l + m] = (gy - y * dot) * ir; Gz[l + m] = (gz - z * dot) * ir;
                    gx = fm * sp; gy = fm * cp; gz = f * dq * sm[m];
                    dot = x * gx + y * gy + z * gz;
                    Gx[l - m] = (gx - x * dot) * ir; Gy[l - m] = (gy - y * dot) * ir; Gz[l - m] = (gz - z * dot) * ir;
                }
            }
            if (l > m) { q2[m] = q1[m]; dq2[m] = dq1[m]; }
            q1[m] = q; dq1[m] = dq;
            if (l == m) { q2[m] = 0.f; dq2[m] = 0.f; }
        }
    }
};

template <int LMAX>
__global__ __launch_bounds__(256) void k_soap_expand_w(SoapDims d, const float4* __restrict__ geo,
                                                       const int* __restrict__ rowptr, const int* __restrict__ sp_nbr,
                                                       const float* __restrict__ table, const float* __restrict__ shn,
                                                       const int* __restrict__ ilut, const float* __restrict__ spw,
                                                       float* __restrict__ Cf, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= N) return;
    const int ld = ((d.NLM + d.F + 4 + 3) & ~3) + 4;   // row: Y[NLM] | R fc [F] | species weights [4] | r, fc (16 B aligned)
    float* rows = smem + (size_t)wave * 32 * ld;
    const int wo = ld - 8;
    const int p0 = rowptr[i], p1 = rowptr[i + 1];
    float4 acc[MAXI];
    int code[MAXI];
#pragma unroll
    for (int k = 0; k < MAXI; k++) {
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int it = lane + 64 * k;
        code[k] = it < d.ITEMS ? ilut[it] : -1;
    }
    for (int base = p0; base < p1; base += 32) {
        const int npc = min(32, p1 - base);
        const int pp = lane & 31;
        if (pp < npc) {
            const float4 g = geo[base + pp];
            const float r = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
            const float ir = r > 0.f ? 1.0f / r : 0.f;
            float* row = rows + pp * ld;
            if (lane < 32) {
                ShLevels<LMAX> sh;
                sh.init(g.x * ir, g.y * ir, g.z * ir, ir);
#pragma unroll
                for (int l = 0; l <= LMAX; l++) {
                    if (l > d.L) break;
                    float Y[2 * LMAX + 1];
                    sh.template level<false>(l, shn, d.L, Y, nullptr, nullptr, nullptr);
#pragma unroll
                    for (int mi = 0; mi < 2 * LMAX + 1; mi++)
                        if (mi <= 2 * l) row[l * l + mi] = Y[mi];
                }
                *reinterpret_cast<float4*>(row + wo) = *reinterpret_cast<const float4*>(spw + sp_nbr[base + pp] * 4);
            } else {
                row[wo + 4] = r;
                row[wo + 5] = shifted_cosine(r, d.rc, d.width, nullptr);
            }
        }
        __builtin_amdgcn_wave_barrier();  // same wave wrote the rows; LDS serves a wave's requests in order
        // the radial functions: (pair, function) items over ALL 64 lanes -- the two spline nodes of an item are independent
        // loads, where 32 lanes walking the functions of their own pair waited for each pair of them in turn (and the
        // spherical-harmonic half of the wave sat idle behind the same branch)
        for (int it = lane; it < npc * d.F; it += 64) {
            const int q = it / d.F, f = it - q * d.F;
            float* rq = rows + q * ld;
            radial_one(d, table, f, rq[wo + 4], rq[wo + 5], 0.f, rq + d.NLM + f, nullptr);
        }
        __builtin_amdgcn_wave_barrier();
        for (int q = 0; q < npc; q++) {
            const float* row = rows + q * ld;
            const float4 w4 = *reinterpret_cast<const float4*>(row + wo);
#pragma unroll
            for (int k = 0; k < MAXI; k++) {
                if (code[k] < 0) continue;
                const float yr = row[code[k] & 255] * row[d.NLM + ((code[k] >> 8) & 255)];
                acc[k].x += yr * w4.x; acc[k].y += yr * w4.y; acc[k].z += yr * w4.z; acc[k].w += yr * w4.w;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int k = 0; k < MAXI; k++)
        if (code[k] >= 0) *reinterpret_cast<float4*>(Cf + (size_t)i * d.NCOEF + (code[k] >> 16)) = acc[k];
}

template <int LMAX>
__global__ __launch_bounds__(256) void k_soap_expand_bwd_p(SoapDims d, const float4* __restrict__ geo,
                                                           const int* __restrict__ ctr, const int* __restrict__ sp_nbr,
                                                           const float* __restrict__ table,
                                                           const float* __restrict__ shn, const float* __restrict__ spw,
                                                           const float* __restrict__ dCf, float4* __restrict__ dv,
                                                           int64_t E, int lds_floats) {
    // The 256 pairs of a workgroup are consecutive in CSR order, i.e. they belong to ~10 consecutive centres: those
    // centres' adjoint coefficient rows (NCOEF floats each) are staged in LDS once, and the 343 float4 a pair reads come
    // from there (lanes of one centre read the same address: a broadcast) instead of as many dependent L1 round trips.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int64_t plast = (p0 + 255 < E ? p0 + 255 : E - 1);
    const int c0 = ctr[p0], c1 = ctr[plast];
    const bool staged = (int64_t)(c1 - c0 + 1) * d.NCOEF <= lds_floats;
    if (staged) {
        const float4* src = reinterpret_cast<const float4*>(dCf + (size_t)c0 * d.NCOEF);
        const int n4 = (c1 - c0 + 1) * (d.NCOEF / 4);
        for (int k = threadIdx.x; k < n4; k += 256) reinterpret_cast<float4*>(smem)[k] = src[k];
        __syncthreads();
    }
    const int64_t p = p0 + threadIdx.x;
    if (p >= E) return;
    const float4 g = geo[p];
    const float r = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    const float ir = r > 0.f ? 1.0f / r : 0.f;
    const float ux = g.x * ir, uy = g.y * ir, uz = g.z * ir;
    float dfc;
    const float fc = shifted_cosine(r, d.rc, d.width, &dfc);
    const float4 w4 = *reinterpret_cast<const float4*>(spw + sp_nbr[p] * 4);
    const float* dC = staged ? smem + (size_t)(ctr[p] - c0) * d.NCOEF : dCf + (size_t)ctr[p] * d.NCOEF;
    ShLevels<LMAX> sh;
    sh.init(ux, uy, uz, ir);
    double ax = 0.0, ay = 0.0, az = 0.0, along = 0.0;  // `along` multiplies the unit vector; fp64 sums (280 items)
#pragma unroll
    for (int l = 0; l <= LMAX; l++) {
        if (l > d.L) break;
        float Y[2 * LMAX + 1], Gx[2 * LMAX + 1], Gy[2 * LMAX + 1], Gz[2 * LMAX + 1], T[2 * LMAX + 1];
        sh.template level<true>(l, shn, d.L, Y, Gx, Gy, Gz);
#pragma unroll
        for (int mi = 0; mi < 2 * LMAX + 1; mi++) T[mi] = 0.f;
        const int nl = d.n_per_l[l];
        const float* dCl = dC + d.coef_off[l];
        for (int n = 0; n < nl; n++) {
            float R, dR;
            // (requesting the spline nodes of function n + 1 before evaluating function n was measured in round 6: 1.04 - 1.08
            // against 0.97 - 0.98 ms; three waves per SIMD at 168 registers and 52 KB of staging: 1.07 ms)
            radial_one(d, table, d.rad_off[l] + n, r, fc, dfc, &R, &dR);
            float ay_ = 0.f;  // sum over m of A Y in fp32 (at most 2 l + 1 terms), then one fp64 add per radial function
#pragma unroll
            for (int mi = 0; mi < 2 * LMAX + 1; mi++) {
                if (mi > 2 * l) continue;
                const float4 c = *reinterpret_cast<const float4*>(dCl + (size_t)(mi * nl + n) * 4);
                const float A = c.x * w4.x + c.y * w4.y + c.z * w4.z + c.w * w4.w;
                ay_ = fmaf(A, Y[mi], ay_);
                T[mi] += A * R;
            }
            along += (double)(ay_ * dR);
        }
#pragma unroll
        for (int mi = 0; mi < 2 * LMAX + 1; mi++) {
            if (mi > 2 * l) continue;
            ax += (double)(T[mi] * Gx[mi]); ay += (double)(T[mi] * Gy[mi]); az += (double)(T[mi] * Gz[mi]);
        }
    }
    dv[p] = make_float4((float)(ax + along * ux), (float)(ay + along * uy), (float)(az + along * uz), 0.f);
}


// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// f(LMAX as a compile-time constant): the instantiation of the wave kernels the plan names
template <class F>
static void with_lmax(bool wide_l, F&& f) {
    if (wide_l) f(std::integral_constant<int, MAXL>{});
    else f(std::integral_constant<int, 6>{});
}

void launch_soap_expand(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    ProfScope ps("soap_expand", st, 2.0 * (double)g.n_edges * d.NCOEF, (double)g.n_edges * 20 + (double)N * d.NCOEF * 4);
    switch (p.expand) {
    case SoapPlan::Expand::Wave: {
        const size_t lds = (size_t)4 * 32 * (((d.NLM + d.F + 4 + 3) & ~3) + 4) * 4;
        with_lmax(p.wide_l, [&](auto lmax) {
            constexpr int LMAX = decltype(lmax)::value;
            allow_big_lds(k_soap_expand_w<LMAX>, lds);
            k_soap_expand_w<LMAX><<<cdiv(N, 4), 256, lds, st>>>(d, g.geo, g.rowptr, g.sp_nbr, m.table, m.shnorm, m.item_lut,
                                                                 m.species_w, w.Cf, N);
        });
        break;
    }
    case SoapPlan::Expand::PerAtom: {
        const size_t lds = (size_t)PC * (d.NLM + d.F + 8 + 1) * 4;
        k_soap_expand<<<N, 256, lds, st>>>(d, g.geo, g.rowptr, g.sp_nbr, m.table, m.shnorm, m.coef_lut, m.species_w, w.Cf);
        break;
    }
    }
}

void launch_soap_expand_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    float4* dv = reinterpret_cast<float4*>(w.dv);
    ProfScope ps("soap_expand_bwd", st, 2.0 * (double)g.n_edges * (d.NCOEF + 8.0 * d.ITEMS),
                 (double)g.n_edges * 36 + (double)N * d.NCOEF * 4);
    switch (p.expand) {
    case SoapPlan::Expand::Wave: {
        const size_t lds = (size_t)p.lds_rows * 4;  // 64 KB: the rows of up to ~14 centres of the default basis
        with_lmax(p.wide_l, [&](auto lmax) {
            constexpr int LMAX = decltype(lmax)::value;
            allow_big_lds(k_soap_expand_bwd_p<LMAX>, lds);
            k_soap_expand_bwd_p<LMAX><<<cdiv(g.n_edges, 256), 256, lds, st>>>(d, g.geo, g.ctr, g.sp_nbr, m.table, m.shnorm,
                                                                               m.species_w, w.dCf, dv, g.n_edges, p.lds_rows);
        });
        break;
    }
    case SoapPlan::Expand::PerAtom: {
        const size_t lds = ((size_t)d.NCOEF + (size_t)PC * (4 * d.NLM + 2 * d.F + 8 + 1)) * 4;
        allow_big_lds(k_soap_expand_bwd, lds);
        k_soap_expand_bwd<<<N, 256, lds, st>>>(d, g.geo, g.rowptr, g.sp_nbr, m.table, m.shnorm, m.item_lut, m.species_w,
                                               w.dCf, dv);
        break;
    }
    }
}

}  // namespace pet
