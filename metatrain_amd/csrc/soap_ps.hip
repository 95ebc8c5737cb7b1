// SOAP-BPNN, power spectrum (+ centre encoding, LayerNorm statistics) and its adjoint, every generation, with their launchers:
//
//   ps[i][l][(n a), (n' a')] = sum_m c[i][l][m][n a] c[i][l][m][n' a']        power_spectrum.py:125-136
//
// One workgroup or one wave per atom, fixed-order sums (no float atomics): bit-reproducible.
#include "soap.h"

namespace pet {

// power spectrum (+ centre encoding): feats[i][feat_off[l] + p1 * nc + p2] = sum_m c[l][m][p1] c[l][m][p2]
__global__ __launch_bounds__(256) void k_soap_ps(SoapDims d, const float* __restrict__ Cf, const int* __restrict__ sp,
                                                 const float* __restrict__ enc, float* __restrict__ feats,
                                                 float* __restrict__ tail) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[8];
    const int i = blockIdx.x;
    for (int k = threadIdx.x; k < d.NCOEF; k += 256) smem[k] = Cf[(size_t)i * d.NCOEF + k];
    __syncthreads();
    float sum = 0.f;
    const float* e = enc ? enc + (size_t)sp[i] * d.S : nullptr;
    for (int idx = threadIdx.x; idx < d.S; idx += 256) {
        int l = 0;
        while (idx >= d.feat_off[l + 1]) l++;
        const int nc = d.n_per_l[l] * d.C, q = idx - d.feat_off[l];
        const int a = q / nc, b = q % nc;
        const float* base = smem + d.coef_off[l];
        float s = 0.f;
        for (int m = 0; m < 2 * l + 1; m++) s += base[m * nc + a] * base[m * nc + b];
        const float v = e ? s * e[idx] : s;
        feats[(size_t)i * d.S + idx] = v;
        sum += v;
    }
    if (!d.layernorm) return;
    // LayerNorm statistics (two passes: mean, then centred variance) for the tail
    const float mean = block_sum(sum, red) / d.S;
    float var = 0.f;
    for (int idx = threadIdx.x; idx < d.S; idx += 256) {
        const float c = feats[(size_t)i * d.S + idx] - mean;  // this thread's own writes
        var += c * c;
    }
    const float rstd = rsqrtf(block_sum(var, red) / d.S + 1e-5f);
    if (threadIdx.x == 0) {
        tail[(size_t)i * (2 + 2 * d.H)] = mean;
        tail[(size_t)i * (2 + 2 * d.H) + 1] = rstd;
    }
}

// ---------------------------------------------------------------------------------------------
// Power spectrum and its adjoint, second generation (pet_config_set("soap_pair", 1), with the expansion kernels):
//   k_soap_ps_w     one wave per atom, features decoded by a table (no division per feature), LayerNorm statistics
//                   as fp64 sum / sum of squares in the same pass (the first version re-read its own output);
//   k_soap_ps_bwd_s one workgroup per atom: the atom's dF row is staged in LDS and symmetrised in place
//                   (G[a][b] = dF[a][b] + dF[b][a]), after which dC[m][a] = sum_b G[b][a] c[m][b] reads consecutive
//                   addresses across lanes (the first version re-read dF from global 2 (2l+1) times).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_soap_ps_w(SoapDims d, const float* __restrict__ Cf, const int* __restrict__ sp,
                                                   const float* __restrict__ enc, const int2* __restrict__ flut,
                                                   float* __restrict__ feats, float* __restrict__ tail, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= N) return;
    float* cs = smem + (size_t)wave * d.NCOEF;
    for (int k = lane; k < d.NCOEF; k += 64) cs[k] = Cf[(size_t)i * d.NCOEF + k];
    __builtin_amdgcn_wave_barrier();
    const float* e = enc ? enc + (size_t)sp[i] * d.S : nullptr;
    double s1 = 0.0, s2 = 0.0;
    for (int idx = lane; idx < d.S; idx += 64) {
        const int2 code = flut[idx];
        const int pa = code.x, pb = code.y & 0xffff, M = (code.y >> 16) & 0xff, nc = code.y >> 24;
        float v = 0.f;
        for (int m = 0; m < M; m++) v += cs[pa + m * nc] * cs[pb + m * nc];
        if (e) v *= e[idx];
        feats[(size_t)i * d.S + idx] = v;
        s1 += (double)v;
        s2 += (double)v * (double)v;
    }
    if (!d.layernorm) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane == 0) {
        const double mean = s1 / d.S, var = s2 / d.S - mean * mean;
        tail[(size_t)i * (2 + 2 * d.H)] = (float)mean;
        tail[(size_t)i * (2 + 2 * d.H) + 1] = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + 1e-5));
    }
}

// The same on the fp32 matrix core (ncmax <= 32): p_l = C_l^T C_l is a [nc x (2l+1)] x [(2l+1) x nc] product and both MFMA
// operands are the SAME register -- lane (a = lane & 31, m = 2 s + (lane >> 5)) holds c[l][m][a] as A[a][m] and as B[m][a] --
// so an l block costs ceil((2l+1) / 2) v_mfma_f32_32x32x2_f32 and as many ds_read_b32 (exact fp32 products, fp32 sums, as
// the scalar loop). One wave per atom; the 32 x 32 tile leaves as rows of nc consecutive floats; LayerNorm statistics in fp64.
// PACKED: only the upper triangle a <= b leaves (SoapDims::Sp floats per atom); the LayerNorm statistics count an
// off-diagonal entry twice, so mean and rstd are those of the full S-vector.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_soap_ps_m(SoapDims d, const float* __restrict__ Cf, const int* __restrict__ sp,
                                                   const float* __restrict__ enc, float* __restrict__ feats,
                                                   float* __restrict__ tail, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= N) return;
    // PACKED: behind the coefficients a staging tile for one l block's triangle (528 floats for nc = 32): the triangle's rows are
    // nc - p1 floats long, so storing them from the accumulator layout is 16 partial-line store instructions per block; through
    // the tile the block leaves as whole 8-byte-per-lane stores (every block starts at an even float: nc is a multiple of C = 4)
    const int stg_len = PACKED ? (d.ncmax * (d.ncmax + 1) / 2 + 3) & ~3 : 0;
    float* cs = smem + (size_t)wave * (d.NCOEF + stg_len);
    float* stg = cs + d.NCOEF;
    for (int k = lane; k < d.NCOEF; k += 64) cs[k] = Cf[(size_t)i * d.NCOEF + k];
    __builtin_amdgcn_wave_barrier();
    const float* e = enc ? enc + (size_t)sp[i] * d.S : nullptr;
    float* out = feats + (size_t)i * (PACKED ? d.Sp : d.S);
    const int a = lane & 31, mh = lane >> 5;
    double s1 = 0.0, s2 = 0.0;
    for (int l = 0; l <= d.L; l++) {
        const int nc = d.n_per_l[l] * d.C, M = 2 * l + 1;
        const float* c = cs + d.coef_off[l];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        {   // (at most MAXL + 1 K steps: unrolled, the LDS reads of a block in flight together)
            float cv[MAXL + 1];
#pragma unroll
            for (int s9 = 0; s9 <= MAXL; s9++) {
                const int m = 2 * s9 + mh;
                const bool ok = m < M && a < nc;
                const float t = c[ok ? m * nc + a : 0];
                cv[s9] = ok ? t : 0.f;
            }
#pragma unroll
            for (int s9 = 0; s9 <= MAXL; s9++)
                if (2 * s9 < M) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cv[s9], cv[s9], acc, 0, 0, 0);
        }
        if (a < nc) {  // this lane: column b = a of rows p1(r)
            const int f0 = d.feat_off[l];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int p1 = (r & 3) + 8 * (r >> 2) + 4 * mh;
                if (PACKED) {
                    if (p1 <= a) {  // row p1 of the triangle: nc - p1 consecutive floats across the lanes
                        const float v = acc[r];
                        stg[soap_tri(nc, p1, a)] = v;
                        const double wv = p1 == a ? (double)v : 2.0 * (double)v;
                        s1 += wv;
                        s2 += wv * (double)v;
                    }
                } else if (p1 < nc) {
                    const int idx = f0 + p1 * nc + a;
                    float v = acc[r];
                    if (e) v *= e[idx];
                    out[idx] = v;
                    s1 += (double)v;
                    s2 += (double)v * (double)v;
                }
            }
        }
        if (PACKED) {
            __builtin_amdgcn_wave_barrier();
            const int n2 = nc * (nc + 1) / 4;  // float2 per block (nc (nc + 1) / 2 is even)
            float2* dst = reinterpret_cast<float2*>(out + d.pfeat_off[l]);
            for (int k = lane; k < n2; k += 64) dst[k] = reinterpret_cast<const float2*>(stg)[k];
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (!d.layernorm) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane == 0) {
        const double mean = s1 / d.S, var = s2 / d.S - mean * mean;
        tail[(size_t)i * (2 + 2 * d.H)] = (float)mean;
        tail[(size_t)i * (2 + 2 * d.H) + 1] = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + 1e-5));
    }
}

__global__ __launch_bounds__(256) void k_soap_ps_bwd_s(SoapDims d, const float* __restrict__ Cf,
                                                       const float* __restrict__ dF, const int2* __restrict__ olut,
                                                       float* __restrict__ dCf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* cs = smem;             // [NCOEF]
    float* G = smem + d.NCOEF;    // [S]
    const int i = blockIdx.x;
    for (int k = threadIdx.x; k < d.NCOEF; k += 256) cs[k] = Cf[(size_t)i * d.NCOEF + k];
    for (int k = threadIdx.x; k < d.S / 4; k += 256)
        reinterpret_cast<float4*>(G)[k] = reinterpret_cast<const float4*>(dF + (size_t)i * d.S)[k];
    __syncthreads();
    for (int l = 0; l <= d.L; l++) {  // symmetrise each block in place: pairs a < b, the diagonal doubles
        const int nc = d.n_per_l[l] * d.C;
        float* g = G + d.feat_off[l];
        for (int q = threadIdx.x; q < nc * nc; q += 256) {
            const int a = q / nc, b = q - a * nc;
            if (a > b) continue;
            const float t = g[a * nc + b] + g[b * nc + a];
            g[a * nc + b] = t;
            g[b * nc + a] = t;
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < d.NCOEF; o += 256) {
        const int2 code = olut[o];
        const int g0 = code.x, c0 = code.y & 0xffff, nc = code.y >> 16;
        double v = 0.0;
        for (int b = 0; b < nc; b++) v += (double)(G[g0 + b * nc] * cs[c0 + b]);
        dCf[(size_t)i * d.NCOEF + o] = (float)v;
    }
}

// The adjoint on the fp32 matrix core: dC_l [(2l+1) x nc] = C_l [(2l+1) x nc] (dF_l + dF_l^T) [nc x nc] as 16 x 16 x 4 tiles (m
// is at most 2 L + 1 = 13 .. 17 rows: the 32-row tile would waste more than half of itself), two MFMAs per K step -- one
// with dF[b][a], one with dF[a][b] -- instead of a symmetrisation pass over the staged row; the workgroup's four waves take
// the l blocks in turn. fp32 products and sums (the scalar kernel summed its 28 terms in fp64).
// PACKED: dF arrives as the symmetrised upper triangle G[a][b] = dx[a][b] + dx[b][a] (k_soap_tail_bwd_set with the packed
// weights): one MFMA per K step, half the staged row.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <bool PACKED>
__global__ __launch_bounds__(256) void k_soap_ps_bwd_m(SoapDims d, const float* __restrict__ Cf,
                                                       const float* __restrict__ dF, float* __restrict__ dCf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* cs = smem;             // [NCOEF]
    float* G = smem + d.NCOEF;    // [S] (PACKED: [Sp])
    const int i = blockIdx.x;
    const int SF = PACKED ? d.Sp : d.S;
    for (int k = threadIdx.x; k < d.NCOEF; k += 256) cs[k] = Cf[(size_t)i * d.NCOEF + k];
    for (int k = threadIdx.x; k < SF / 4; k += 256)
        reinterpret_cast<float4*>(G)[k] = reinterpret_cast<const float4*>(dF + (size_t)i * SF)[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    // (collecting the result in LDS and storing it as whole lines behind a workgroup barrier was measured in round 6: 0.63 against
    // 0.56 ms -- the four waves' own 64-byte row pieces overlap with the slower waves' products)
    float* out = dCf + (size_t)i * d.NCOEF;
    for (int l = wave; l <= d.L; l += 4) {
        const int nc = d.n_per_l[l] * d.C, M = 2 * l + 1;
        const float* c = cs + d.coef_off[l];
        const float* g = G + (PACKED ? d.pfeat_off[l] : d.feat_off[l]);
        for (int m0 = 0; m0 < M; m0 += 16)
            for (int a0 = 0; a0 < nc; a0 += 16) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                const int mi = m0 + li, aj = a0 + li;
                if (PACKED) {
                    // (ncmax <= 32: eight K steps, unrolled with clamped addresses and zeroed operands past the block, so that the
                    // sixteen LDS reads are in flight together; the rolled loop waited for two dependent reads per MFMA)
                    float av[8], bv[8];
#pragma unroll
                    for (int s8 = 0; s8 < 8; s8++) {
                        const int b = 4 * s8 + kq;
                        const bool oka = mi < M && b < nc, okb = aj < nc && b < nc;
                        const float ta = c[oka ? mi * nc + b : 0];
                        const float tb = g[okb ? soap_tri(nc, b < aj ? b : aj, b < aj ? aj : b) : 0];  // G[a][b] = G[b][a]
                        av[s8] = oka ? ta : 0.f;
                        bv[s8] = okb ? tb : 0.f;
                    }
#pragma unroll
                    for (int s8 = 0; s8 < 8; s8++)
                        if (4 * s8 < nc) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s8], bv[s8], acc, 0, 0, 0);
                } else
                for (int b0 = 0; b0 < nc; b0 += 4) {
                    const int b = b0 + kq;
                    const float av = (mi < M && b < nc) ? c[mi * nc + b] : 0.f;
                    const bool ok = aj < nc && b < nc;
                    if (PACKED) {
                        const float bv = ok ? g[soap_tri(nc, b < aj ? b : aj, b < aj ? aj : b)] : 0.f;  // G[a][b] = G[b][a]
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
                    } else {
                        const float bv = ok ? g[b * nc + aj] : 0.f, bt = ok ? g[aj * nc + b] : 0.f;  // dF[b][a], dF[a][b]
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bt, acc, 0, 0, 0);
                    }
                }
                if (aj < nc) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int mm = m0 + 4 * kq + r;
                        if (mm < M) out[d.coef_off[l] + mm * nc + aj] = acc[r];
                    }
                }
            }
    }
}


// (The first-generation fused power-spectrum + tail kernels -- k_soap_ps_tail_fwd / _bwd behind pet_config_set("soap_fused", 1):
// features never stored, but 4.3 + 7.0 ms against 0.5 + 0.6 + 0.9 + 0.7 for the separate kernels -- were removed in round 6:
// the packed power spectrum halves the feature traffic at no cost in time.)

// dC[l][m][a] = sum_b (dF[l][a][b] + dF[l][b][a]) c[l][m][b]
__global__ __launch_bounds__(256) void k_soap_ps_bwd(SoapDims d, const float* __restrict__ Cf,
                                                     const float* __restrict__ dF, const int* __restrict__ lut,
                                                     float* __restrict__ dCf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int i = blockIdx.x;
    for (int k = threadIdx.x; k < d.NCOEF; k += 256) smem[k] = Cf[(size_t)i * d.NCOEF + k];
    __syncthreads();
    const float* dFi = dF + (size_t)i * d.S;
    for (int idx = threadIdx.x; idx < d.NCOEF; idx += 256) {
        int l = 0;
        while (idx >= d.coef_off[l + 1]) l++;
        const int nc = d.n_per_l[l] * d.C, q = idx - d.coef_off[l];
        const int m = q / nc, a = q % nc;
        const float* crow = smem + d.coef_off[l] + m * nc;
        const float* fb = dFi + d.feat_off[l];
        float s = 0.f;
        for (int b = 0; b < nc; b++) s += (fb[a * nc + b] + fb[b * nc + a]) * crow[b];
        dCf[(size_t)i * d.NCOEF + idx] = s;
    }
}


// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
void soap_ps_full(const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    const size_t lds = (size_t)4 * d.NCOEF * 4;  // one atom's coefficients per wave
    allow_big_lds(k_soap_ps_m<false>, lds);
    k_soap_ps_m<false><<<cdiv(N, 4), 256, lds, st>>>(d, w.Cf, g.sp, m.enc, w.feats, w.tail, N);
}

void launch_soap_ps(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    ProfScope ps("soap_ps", st, 2.0 * (double)N * d.S * (d.L + 1), (double)N * (d.NCOEF + (p.packed ? d.Sp : d.S)) * 4);
    switch (p.ps) {
    case SoapPlan::PowerSpectrum::MfmaPacked: {
        const size_t lds = (size_t)4 * (d.NCOEF + ((d.ncmax * (d.ncmax + 1) / 2 + 3) & ~3)) * 4;
        allow_big_lds(k_soap_ps_m<true>, lds);
        k_soap_ps_m<true><<<cdiv(N, 4), 256, lds, st>>>(d, w.Cf, g.sp, nullptr, w.feats, w.tail, N);
        break;
    }
    case SoapPlan::PowerSpectrum::Mfma:
        soap_ps_full(m, g, w, st);
        break;
    case SoapPlan::PowerSpectrum::Lut: {
        const size_t lds = (size_t)4 * d.NCOEF * 4;
        allow_big_lds(k_soap_ps_w, lds);
        k_soap_ps_w<<<cdiv(N, 4), 256, lds, st>>>(d, w.Cf, g.sp, m.enc, m.feat_lut, w.feats, w.tail, N);
        break;
    }
    case SoapPlan::PowerSpectrum::PerAtom:
        k_soap_ps<<<N, 256, (size_t)d.NCOEF * 4, st>>>(d, w.Cf, g.sp, m.enc, w.feats, w.tail);
        break;
    }
}

void launch_soap_ps_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    ProfScope ps("soap_ps_bwd", st, 4.0 * (double)N * d.S * (d.L + 1), (double)N * (2 * d.NCOEF + (p.packed ? d.Sp : d.S)) * 4);
    const size_t lds_row = (size_t)(d.NCOEF + (p.packed ? d.Sp : d.S)) * 4;  // the atom's coefficients and its dF row
    switch (p.ps) {
    case SoapPlan::PowerSpectrum::MfmaPacked:
        k_soap_ps_bwd_m<true><<<N, 256, lds_row, st>>>(d, w.Cf, w.dF, w.dCf);
        break;
    case SoapPlan::PowerSpectrum::Mfma:
        k_soap_ps_bwd_m<false><<<N, 256, lds_row, st>>>(d, w.Cf, w.dF, w.dCf);
        break;
    case SoapPlan::PowerSpectrum::Lut:
        k_soap_ps_bwd_s<<<N, 256, lds_row, st>>>(d, w.Cf, w.dF, m.out_lut, w.dCf);
        break;
    case SoapPlan::PowerSpectrum::PerAtom:
        k_soap_ps_bwd<<<N, 256, (size_t)d.NCOEF * 4, st>>>(d, w.Cf, w.dF, m.coef_lut, w.dCf);
        break;
    }
}

}  // namespace pet
