// SOAP-BPNN, LayerNorm + MLP tail and its adjoint -- per atom, stacked over all networks, or on
// species-sorted tiles after bucketing the atoms (k_sp_*) -- the folded weight forms soap_finalize prepares for them
// (k_soap_prep_*), the continuation kernels of deep tails, and their launchers:
//
//   e_i = w3 . silu(W2 silu(W1 LN(ps_i * enc[s_i])))                           model.py:553-595, 1204-1219
#include <type_traits>

#include "soap.h"

namespace pet {

// ---------------------------------------------------------------------------------------------
// a18: LayerNorm + MLP + last layer, one workgroup per atom. tail[i] = {mean, rstd, a1[H], a2[H]}
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_soap_tail(SoapDims d, const float* __restrict__ feats,
                                                   const int* __restrict__ sp, const SoapSet* __restrict__ sets,
                                                   float* __restrict__ tail, float* __restrict__ atomic) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                 // [S] normalised input
    float* part = xs + d.S;           // [256][H+1]
    float* red = part + 256 * (d.H + 1);  // [8]
    float* hs = red + 8;              // [2*H]
    const int i = blockIdx.x, tid = threadIdx.x;
    const SoapSet W = sets[d.legacy ? sp[i] : 0];
    const float* x = feats + (size_t)i * d.S;
    float mean = 0.f, rstd = 1.f;
    if (d.layernorm) {
        float s = 0.f;
        for (int k = tid; k < d.S; k += 256) s += x[k];
        mean = block_sum(s, red) / d.S;
        float v = 0.f;
        for (int k = tid; k < d.S; k += 256) { const float c = x[k] - mean; v += c * c; }
        rstd = rsqrtf(block_sum(v, red) / d.S + 1e-5f);
        for (int k = tid; k < d.S; k += 256) xs[k] = (x[k] - mean) * rstd * W.ln_w[k] + W.ln_b[k];
    } else {
        for (int k = tid; k < d.S; k += 256) xs[k] = x[k];
    }
    __syncthreads();
    float acc[MAXH];
#pragma unroll
    for (int j = 0; j < MAXH; j++) acc[j] = 0.f;
    for (int k = tid; k < d.S; k += 256) {
        const float xv = xs[k];
#pragma unroll
        for (int j = 0; j < MAXH; j++)
            if (j < d.H) acc[j] += W.W1[(size_t)j * d.S + k] * xv;
    }
#pragma unroll
    for (int j = 0; j < MAXH; j++)
        if (j < d.H) part[tid * (d.H + 1) + j] = acc[j];
    __syncthreads();
    if (tid < d.H) {
        float s = 0.f;
        for (int t = 0; t < 256; t++) s += part[t * (d.H + 1) + tid];
        hs[tid] = s;  // a1
    }
    __syncthreads();
    float a2 = 0.f;
    if (tid < d.H && d.NH > 1) {
        for (int q = 0; q < d.H; q++) a2 += W.W2[tid * d.H + q] * silu(hs[q]);
        hs[d.H + tid] = a2;
    }
    __syncthreads();
    if (tid < 64) {
        float e = 0.f;
        if (tid < d.H) e = W.w3[tid] * silu(d.NH > 1 ? hs[d.H + tid] : hs[tid]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (tid == 0) atomic[i] = e;
    }
    float* tl = tail + (size_t)i * (2 + 2 * d.H);
    if (tid == 0) { tl[0] = mean; tl[1] = rstd; }
    if (tid < 2 * d.H) tl[2 + tid] = hs[tid];
}

// ---- MFMA tail: 64 atoms per workgroup, first Linear of ALL sets as one [64 x Kp] x [Kp x NOUTP] GEMM ----
__global__ void k_soap_prep_wall(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int NOUTP, int Kp,
                                 float* __restrict__ wall) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)NOUTP * Kp) return;
    const int o = (int)(idx / Kp), k = (int)(idx % Kp);
    float v = 0.f;
    if (o < n_sets * d.H && k < d.S) {
        const SoapSet W = sets[o / d.H];
        v = W.W1[(size_t)(o % d.H) * d.S + k];
        if (d.layernorm) v *= W.ln_w[k];
    }
    wall[idx] = v;
}
__global__ void k_soap_prep_rows(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int NOUTP, int Kp,
                                 const float* __restrict__ wall, float* __restrict__ rs, float* __restrict__ bs) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= NOUTP) return;
    double s = 0.0, b = 0.0;
    if (o < n_sets * d.H) {
        const SoapSet W = sets[o / d.H];
        for (int k = 0; k < d.S; k++) {
            s += wall[(size_t)o * Kp + k];
            if (d.layernorm) b += (double)W.W1[(size_t)(o % d.H) * d.S + k] * W.ln_b[k];
        }
    }
    rs[o] = (float)s;
    bs[o] = (float)b;
}

// The first Linear over the packed (upper-triangle) feature layout, one network after the other: [n_sets * H][Kpp].
// diag2: the adjoint's copy -- its GEMM output is G[a][b] = dx[a][b] + dx[b][a], which on the diagonal is TWICE dx[a][a].
__global__ void k_soap_prep_wallp(SoapDims d, const SoapSet* __restrict__ sets, int n_sets, int Kpp, int diag2,
                                  float* __restrict__ wallp) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n_sets * d.H * Kpp) return;
    const int o = (int)(idx / Kpp), t = (int)(idx % Kpp);
    float v = 0.f;
    if (t < d.Sp) {
        int l = 0;
        while (t >= d.pfeat_off[l + 1]) l++;
        const int nc = d.n_per_l[l] * d.C;
        int q = t - d.pfeat_off[l], a = 0;
        while (q >= nc - a) { q -= nc - a; a++; }
        const int b = a + q;
        const SoapSet W = sets[o / d.H];
        const float* w1 = W.W1 + (size_t)(o % d.H) * d.S + d.feat_off[l];
        const float* lw = W.ln_w + d.feat_off[l];
        const int k1 = a * nc + b, k2 = b * nc + a;
        v = w1[k1] * (d.layernorm ? lw[k1] : 1.f);
        if (a != b) v += w1[k2] * (d.layernorm ? lw[k2] : 1.f);
        else if (diag2) v *= 2.f;
    }
    wallp[idx] = v;
}

template <int NT>
__global__ __launch_bounds__(NTHREADS) void k_soap_tail_fwd_mfma(SoapDims d, const float* __restrict__ feats,
                                                                 const int* __restrict__ sp,
                                                                 const SoapSet* __restrict__ sets,
                                                                 const float4* __restrict__ Wp, int Kp,
                                                                 const float* __restrict__ rs,
                                                                 const float* __restrict__ bs, float* __restrict__ tail,
                                                                 float* __restrict__ atomic, int N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NOUTP = 64 * NT, LDO = NOUTP + 1, LDA = lds_ld(128);
    float* As = smem;                    // [64][132], later out [64][NOUTP + 1]
    float* out = smem;
    float* a1s = smem + BM * (LDO > LDA ? LDO : LDA);  // [64][32] silu(a1)
    const WaveId w;
    const int row0 = blockIdx.x * BM;
    f32x16 acc[NT];
    acc_fill_bias<NT>(acc, nullptr, 0, w.lane);
    for (int kc = 0; kc < Kp / 128; kc++) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < BM * 32; idx += NTHREADS) {
            const int r = idx >> 5, c = idx & 31, col = 128 * kc + 4 * c;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < N && col < d.S) v = *reinterpret_cast<const float4*>(feats + (size_t)(row0 + r) * d.S + col);
            *reinterpret_cast<float4*>(As + r * LDA + 4 * c) = v;
        }
        __syncthreads();
        gemm_acc<128, NT>(As + w.rb * 32 * LDA, LDA, Wp, Kp / 8, 16 * kc, NT * w.ch, acc, w.lane);
    }
    __syncthreads();
    acc_foreach<NT>(acc, w.rb, 32 * NT * w.ch, w.lane, [&](int r, int c, float v) { out[r * LDO + c] = v; });
    __syncthreads();
    const int H = 32, TS = 2 + 2 * H;
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, atom = row0 + r;
        float a1 = 0.f;
        if (atom < N) {
            const int s = d.legacy ? sp[atom] : 0;
            const float mu = d.layernorm ? tail[(size_t)atom * TS] : 0.f;
            const float rstd = d.layernorm ? tail[(size_t)atom * TS + 1] : 1.f;
            a1 = rstd * (out[r * LDO + s * H + j] - mu * rs[s * H + j]) + bs[s * H + j];
            tail[(size_t)atom * TS + 2 + j] = a1;
        }
        a1s[r * H + j] = silu(a1);
    }
    __syncthreads();
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, atom = row0 + r;
        float e = 0.f;
        if (atom < N) {
            const SoapSet W = sets[d.legacy ? sp[atom] : 0];
            if (d.NH > 1) {
                float a2 = 0.f;
                for (int q = 0; q < H; q++) a2 += W.W2[j * H + q] * a1s[r * H + q];
                tail[(size_t)atom * TS + 2 + H + j] = a2;
                e = W.w3[j] * silu(a2);
            } else {
                e = W.w3[j] * a1s[r * H + j];
            }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (j == 0 && atom < N) atomic[atom] = e;
    }
}

template <int NT>
__global__ __launch_bounds__(NTHREADS) void k_soap_tail_bwd_mfma(SoapDims d, const float* __restrict__ feats,
                                                                 const int* __restrict__ sp,
                                                                 const SoapSet* __restrict__ sets,
                                                                 const float4* __restrict__ Wpb, int Kp,
                                                                 const float* __restrict__ rs,
                                                                 const float* __restrict__ bs,
                                                                 const float* __restrict__ enc,
                                                                 const float* __restrict__ tail,
                                                                 const float* __restrict__ gA, float* __restrict__ dF,
                                                                 int N, const float* __restrict__ da2x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NOUTP = 64 * NT, LDD = lds_ld(NOUTP);
    float* Ds = smem;                 // [64][NOUTP + 4] d a1, zero outside the atom's own set
    float* d2 = Ds + BM * LDD;        // [64][32] d a2
    float* st = d2 + BM * 32;         // [64][4] mean, rstd, m1, m2
    float* ot = st + BM * 4;          // [64][132] output tile staging: full-row (512 B) reads / writes below
    const WaveId w;
    const int row0 = blockIdx.x * BM;
    const int H = 32, TS = 2 + 2 * H;
    for (int idx = threadIdx.x; idx < BM * LDD; idx += NTHREADS) Ds[idx] = 0.f;
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, atom = row0 + r;
        float v = 0.f;
        if (atom < N && d.NH > 1) {
            const SoapSet W = sets[d.legacy ? sp[atom] : 0];
            v = da2x ? da2x[(size_t)atom * H + j] : gA[atom] * W.w3[j] * dsilu(tail[(size_t)atom * TS + 2 + H + j]);
        }
        d2[r * H + j] = v;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, atom = row0 + r;
        float da1 = 0.f, t1 = 0.f, t2 = 0.f;
        float mu = 0.f, rstd = 1.f;
        if (atom < N) {
            const int s = d.legacy ? sp[atom] : 0;
            const SoapSet W = sets[s];
            const float a1 = tail[(size_t)atom * TS + 2 + j];
            if (d.NH > 1) {
                float acc = 0.f;
                for (int q = 0; q < H; q++) acc += W.W2[q * H + j] * d2[r * H + q];
                da1 = acc * dsilu(a1);
            } else {
                da1 = gA[atom] * W.w3[j] * dsilu(a1);
            }
            Ds[r * LDD + s * H + j] = da1;
            if (d.layernorm) {
                mu = tail[(size_t)atom * TS];
                rstd = tail[(size_t)atom * TS + 1];
                const float rsj = rs[s * H + j];
                const float raw = (a1 - bs[s * H + j]) / rstd + mu * rsj;  // Wall_s[j] . x
                t1 = da1 * rsj;
                t2 = da1 * raw;
            }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { t1 += __shfl_xor(t1, o); t2 += __shfl_xor(t2, o); }
        if (j == 0) {
            st[r * 4] = mu; st[r * 4 + 1] = rstd;
            st[r * 4 + 2] = t1 / d.S;                        // m1 = mean(dxn gamma)
            st[r * 4 + 3] = rstd * (t2 - mu * t1) / d.S;     // m2 = mean(dxn gamma xhat)
        }
    }
    __syncthreads();
    for (int nblk = 0; nblk < Kp / 128; nblk++) {
        f32x16 acc[2];
        acc_fill_bias<2>(acc, nullptr, 0, w.lane);
        gemm_acc<NOUTP, 2>(Ds + w.rb * 32 * LDD, LDD, Wpb, NOUTP / 8, 0, 4 * nblk + 2 * w.ch, acc, w.lane);
        __syncthreads();  // the previous block's staging tile has been consumed
        acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) { ot[r * lds_ld(128) + c] = v; });
        __syncthreads();
        for (int idx = threadIdx.x; idx < BM * 32; idx += NTHREADS) {
            const int r = idx >> 5, c4 = idx & 31, k = 128 * nblk + 4 * c4, atom = row0 + r;
            if (atom >= N || k >= d.S) continue;
            float4 v = *reinterpret_cast<const float4*>(ot + r * lds_ld(128) + 4 * c4);
            if (d.layernorm) {
                const float4 x = *reinterpret_cast<const float4*>(feats + (size_t)atom * d.S + k);
                const float mu = st[r * 4], rs_ = st[r * 4 + 1], m1 = st[r * 4 + 2], m2 = st[r * 4 + 3];
                v.x = rs_ * (v.x - m1 - (x.x - mu) * rs_ * m2);
                v.y = rs_ * (v.y - m1 - (x.y - mu) * rs_ * m2);
                v.z = rs_ * (v.z - m1 - (x.z - mu) * rs_ * m2);
                v.w = rs_ * (v.w - m1 - (x.w - mu) * rs_ * m2);
            }
            if (enc) {
                const float4 e = *reinterpret_cast<const float4*>(enc + (size_t)sp[atom] * d.S + k);
                v.x *= e.x; v.y *= e.y; v.z *= e.z; v.w *= e.w;
            }
            *reinterpret_cast<float4*>(dF + (size_t)atom * d.S + k) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// a18, species-sorted tiles (pet_config_set("soap_sorted", 1), default): in legacy mode every atom uses ONE of the
// per-species networks, so the stacked GEMM above does n_species times the needed MFMA work. Here the atoms are
// bucketed by network once per forward (counting sort, k_sp_*), a 64-atom tile holds atoms of one network only and
// multiplies with that network's [32 x Kp] weight: one 32-column tile, the two column-half waves split K instead
// and their accumulators are summed through LDS. Per-atom results do not depend on tile mates, so the (atomic)
// order inside a bucket does not show in the output.
// ---------------------------------------------------------------------------------------------
// The bucket table and the k_sp_* kernels are sized by MS at compile time: the forward keeps MS = 8 (eight ballots per
// atom in k_sp_fill), the training pass of a model with more networks takes MS = 16. An atom of a network >= MS would
// index every array here out of range, so each host path checks n_sets <= MS before the first launch.
template <int MS>
__global__ void k_sp_count(const int* __restrict__ sp, int legacy, int N, SpInfoT<MS>* __restrict__ info) {
    __shared__ int hist[MS];
    if (threadIdx.x < MS) hist[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) atomicAdd(&hist[legacy ? sp[i] : 0], 1);
    __syncthreads();
    if (threadIdx.x < MS && hist[threadIdx.x]) atomicAdd(&info->count[threadIdx.x], hist[threadIdx.x]);
}
template <int MS>
__global__ void k_sp_scan(int n_sets, SpInfoT<MS>* __restrict__ info) {
    info->offs[0] = 0;
    info->tstart[0] = 0;
    for (int s = 0; s < n_sets; s++) {
        info->offs[s + 1] = info->offs[s] + info->count[s];
        info->tstart[s + 1] = info->tstart[s] + (info->count[s] + BM - 1) / BM;
        info->cursor[s] = 0;
    }
}
template <int MS>
__global__ __launch_bounds__(1024) void k_sp_fill(const int* __restrict__ sp, int legacy, int N, SpInfoT<MS>* __restrict__ info,
                                                   int* __restrict__ perm) {
    // one atomic per (workgroup of 1 024 atoms, network) instead of one per atom: 100 k atoms on 4 cursors serialised in
    // L2 (0.63 ms per atom, 0.08 ms per wave)
    __shared__ int wcount[MS][16], wbase[MS][16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = i < N ? (legacy ? sp[i] : 0) : -1;
    int rank = 0;
    for (int t = 0; t < MS; t++) {
        const unsigned long long m = __ballot(s == t);
        if (lane == 0) wcount[t][wave] = __popcll(m);
        if (s == t) rank = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (threadIdx.x < MS) {
        const int t = threadIdx.x;
        int tot = 0;
        for (int w = 0; w < 16; w++) { wbase[t][w] = tot; tot += wcount[t][w]; }
        const int base = tot ? atomicAdd(&info->cursor[t], tot) : 0;
        for (int w = 0; w < 16; w++) wbase[t][w] += base;
    }
    __syncthreads();
    if (s >= 0) perm[info->offs[s] + wbase[s][wave] + rank] = i;
}
// atoms bucketed by network into perm, on a table of MS networks; *offs = the table's offs[n_sets + 1] (device pointer)
template <int MS>
static int sp_bucket(const int* sp, int legacy, int N, int n_sets, void* info_, int* perm, const int** offs, hipStream_t st) {
    PET_REQUIRE(n_sets <= MS, PET_ERR_UNSUPPORTED, "more networks than the bucket table holds");
    SpInfoT<MS>* info = static_cast<SpInfoT<MS>*>(info_);
    PET_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(SpInfoT<MS>), st));
    k_sp_count<MS><<<cdiv(N, 256), 256, 0, st>>>(sp, legacy, N, info);
    k_sp_scan<MS><<<1, 1, 0, st>>>(n_sets, info);
    k_sp_fill<MS><<<cdiv(N, 1024), 1024, 0, st>>>(sp, legacy, N, info, perm);
    if (offs) *offs = info->offs;
    return PET_OK;
}
// tile -> (network, first slot in perm, number of atoms); false if the tile index is past the last bucket
__device__ __forceinline__ bool sp_tile(const SpInfo* __restrict__ info, int n_sets, int t, int& s, int& base, int& cnt) {
    if (t >= info->tstart[n_sets]) return false;
    s = 0;
    while (t >= info->tstart[s + 1]) s++;
    base = info->offs[s] + BM * (t - info->tstart[s]);
    cnt = min(BM, info->offs[s + 1] - base);
    return true;
}

__global__ __launch_bounds__(NTHREADS) void k_soap_tail_fwd_set(SoapDims d, const float* __restrict__ feats,
                                                                const int* __restrict__ perm,
                                                                const SpInfo* __restrict__ info, int n_sets,
                                                                const SoapSet* __restrict__ sets,
                                                                const float4* __restrict__ Wps, int Kp,
                                                                const float* __restrict__ rs,
                                                                const float* __restrict__ bs, float* __restrict__ tail,
                                                                float* __restrict__ atomic) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int H = 32, LDO = H + 1, LDA = lds_ld(128), TS = 2 + 2 * H;
    float* As = smem;                    // [64][132]; later the K-split partial sums [64][33] + out [64][33]
    float* a1s = smem + BM * LDA;        // [64][32] silu(a1)
    int* rows = reinterpret_cast<int*>(a1s + BM * H);  // [64] atom of each row, -1 beyond the bucket
    int sidx, base, cnt;
    if (!sp_tile(info, n_sets, blockIdx.x, sidx, base, cnt)) return;
    const WaveId w;
    if (threadIdx.x < BM) rows[threadIdx.x] = (int)threadIdx.x < cnt ? perm[base + threadIdx.x] : -1;
    const float4* Wp = Wps + (size_t)sidx * (Kp / 8) * 64;
    f32x16 acc[1];
    acc_fill_bias<1>(acc, nullptr, 0, w.lane);
    // this thread's 8 float4 of a chunk: rows r0 + 8 q (q = 0..7), column group c; the next chunk is requested
    // before the MFMAs of the current one, so its HBM latency hides behind them and the barriers
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    // the GEMM runs on CENTRED features (x - mean): a1 = rstd W~(x - mu) + W beta without the large, cancelling
    // terms W~x and mu rowsum(W~) of the stacked kernel
    int64_t rowoff[8];
    float rowmu[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int at = rows[r0 + 8 * q];
        rowoff[q] = at >= 0 ? (int64_t)at * d.S : -1;
        rowmu[q] = at >= 0 && d.layernorm ? tail[(size_t)at * TS] : 0.f;
    }
    float4 pre[8];
    auto fetch = [&](int kc) {
        const int col = 128 * kc + 4 * c;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            // raw values: the centring waits until the tile is written (a subtraction here makes the load's latency part of
            // this trip instead of hiding it behind the MFMAs)
            pre[q] = make_float4(rowmu[q], rowmu[q], rowmu[q], rowmu[q]);  // (x - mu = 0 in the padding)
            if (rowoff[q] >= 0 && col < d.S) pre[q] = *reinterpret_cast<const float4*>(feats + rowoff[q] + col);
        }
    };
    fetch(0);
    // The 4 544-term dot products are summed in fp32 only WITHIN a chunk (32 MFMA steps); the 36 chunk results are
    // added in fp64. A single fp32 accumulator over all 1 152 steps leaves a1 with ~3e-6 of rounding noise, which the
    // reverse pass turns into the same relative error of dE/dR (silu'(a1) and the LayerNorm adjoint's mean(dx xhat),
    // which is rebuilt from the saved a1): the worst force component of a 10 000-atom box then sat at 1.05e-5.
    double tot[16];
#pragma unroll
    for (int r = 0; r < 16; r++) tot[r] = 0.0;
    for (int kc = 0; kc < Kp / 128; kc++) {
        // this wave's eight weight fragments of the chunk (the column-half index splits K: 64 of the chunk's 128 k) are
        // requested together, ahead of the barriers: gemm_acc asks for one fragment per four MFMAs, i.e. eight dependent L2
        // round trips per chunk, which is what this kernel waited for (20 k cycles per chunk against 2 k of MFMA)
        float4 bw[8];
        {
            const float4* bp = Wp + ((size_t)16 * kc + 8 * w.ch) * 64 + w.lane;
#pragma unroll
            for (int kg = 0; kg < 8; kg++) bw[kg] = bp[kg * 64];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; q++)
            *reinterpret_cast<float4*>(As + (r0 + 8 * q) * LDA + 4 * c) =
                make_float4(pre[q].x - rowmu[q], pre[q].y - rowmu[q], pre[q].z - rowmu[q], pre[q].w - rowmu[q]);
        __syncthreads();
        if (kc + 1 < Kp / 128) fetch(kc + 1);
        acc_fill_bias<1>(acc, nullptr, 0, w.lane);
        {
            const float* arow = As + (w.rb * 32 + (w.lane & 31)) * LDA + 64 * w.ch + (w.lane >> 5) * 4;
#pragma unroll
            for (int kg = 0; kg < 8; kg++) {  // the same products in the same order as gemm_acc<64, 1>
                const float4 av = *reinterpret_cast<const float4*>(arow + kg * 8);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw[kg].x, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw[kg].y, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw[kg].z, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw[kg].w, acc[0], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) tot[r] += (double)acc[0][r];
    }
    __syncthreads();
    double* part = reinterpret_cast<double*>(smem);                  // [64][33] partial sums of the second K half
    float* out = smem + 2 * BM * LDO;                                 // [64][33]
    if (w.ch == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) part[(w.rb * 32 + acc_row(r, w.lane)) * LDO + (w.lane & 31)] = tot[r];
    }
    __syncthreads();
    if (w.ch == 0) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int idx = (w.rb * 32 + acc_row(r, w.lane)) * LDO + (w.lane & 31);
            out[idx] = (float)(tot[r] + part[idx]);
        }
    }
    __syncthreads();
    const SoapSet W = sets[sidx];
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, at = rows[r];
        float a1 = 0.f;
        if (at >= 0) {
            const float rstd = d.layernorm ? tail[(size_t)at * TS + 1] : 1.f;
            a1 = rstd * out[r * LDO + j] + bs[sidx * H + j];
            tail[(size_t)at * TS + 2 + j] = a1;
        }
        a1s[r * H + j] = silu(a1);
    }
    __syncthreads();
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, at = rows[r];
        float e = 0.f;
        if (at >= 0) {
            if (d.NH > 1) {
                float a2 = 0.f;
                for (int q = 0; q < H; q++) a2 += W.W2[j * H + q] * a1s[r * H + q];
                tail[(size_t)at * TS + 2 + H + j] = a2;
                e = W.w3[j] * silu(a2);
            } else {
                e = W.w3[j] * a1s[r * H + j];
            }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (j == 0 && at >= 0) atomic[at] = e;
    }
}

__global__ __launch_bounds__(NTHREADS) void k_soap_tail_bwd_set(SoapDims d, const float* __restrict__ feats,
                                                                const int* __restrict__ perm,
                                                                const SpInfo* __restrict__ info, int n_sets,
                                                                const int* __restrict__ sp,
                                                                const SoapSet* __restrict__ sets,
                                                                const float4* __restrict__ Wpbs, int Kp,
                                                                const float* __restrict__ rs,
                                                                const float* __restrict__ bs,
                                                                const float* __restrict__ enc,
                                                                const float* __restrict__ tail,
                                                                const float* __restrict__ gA, float* __restrict__ dF,
                                                                const float* __restrict__ da2x, int packed) {
    // packed != 0: feats / dF rows are the upper-triangle layout (SoapDims::Sp floats), Wpbs the packed weights with the
    // diagonal doubled; the output is G[a][b] = dx[a][b] + dx[b][a] = rstd (g'_t - 2 (m1 + xhat_t m2)): the two LayerNorm means
    // (over the FULL S-vector, as before) enter twice
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int H = 32, LDD = lds_ld(H), TS = 2 + 2 * H;
    const int SR = packed ? d.Sp : d.S;   // row pitch and length of feats / dF
    const float pm = packed ? 2.f : 1.f;
    float* Ds = smem;                 // [64][36] d a1
    float* d2 = Ds + BM * LDD;        // [64][32] d a2
    float* st = d2 + BM * H;          // [64][4] mean, rstd, m1, m2
    float* ot = st + BM * 4;          // [64][132] output tile staging
    int* rows = reinterpret_cast<int*>(ot + BM * lds_ld(128));  // [64]
    int sidx, base, cnt;
    if (!sp_tile(info, n_sets, blockIdx.x, sidx, base, cnt)) return;
    const WaveId w;
    if (threadIdx.x < BM) rows[threadIdx.x] = (int)threadIdx.x < cnt ? perm[base + threadIdx.x] : -1;
    const SoapSet W = sets[sidx];
    const float4* Wpb = Wpbs + (size_t)sidx * (Kp / 32) * 4 * 64;
    __syncthreads();
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, at = rows[r];
        float v = 0.f;
        if (at >= 0 && d.NH > 1)
            v = da2x ? da2x[(size_t)at * H + j] : gA[at] * W.w3[j] * dsilu(tail[(size_t)at * TS + 2 + H + j]);
        d2[r * H + j] = v;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < BM * H; item += NTHREADS) {
        const int r = item >> 5, j = item & 31, at = rows[r];
        float da1 = 0.f, t1 = 0.f, t2 = 0.f;
        float mu = 0.f, rstd = 1.f;
        if (at >= 0) {
            const float a1 = tail[(size_t)at * TS + 2 + j];
            if (d.NH > 1) {
                float acc = 0.f;
                for (int q = 0; q < H; q++) acc += W.W2[q * H + j] * d2[r * H + q];
                da1 = acc * dsilu(a1);
            } else {
                da1 = gA[at] * W.w3[j] * dsilu(a1);
            }
            if (d.layernorm) {
                mu = tail[(size_t)at * TS];
                rstd = tail[(size_t)at * TS + 1];
                t1 = da1 * rs[sidx * H + j];
                t2 = da1 * (a1 - bs[sidx * H + j]) / rstd;  // da1 * Wall_s[j] . (x - mu)
            }
        }
        Ds[r * LDD + j] = da1;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { t1 += __shfl_xor(t1, o); t2 += __shfl_xor(t2, o); }
        if (j == 0) {
            st[r * 4] = mu; st[r * 4 + 1] = rstd;
            st[r * 4 + 2] = pm * t1 / d.S;          // m1 = mean(dxn gamma)
            st[r * 4 + 3] = pm * rstd * t2 / d.S;   // m2 = mean(dxn gamma xhat)
        }
    }
    __syncthreads();
    // the feature values the LayerNorm adjoint needs are requested one block ahead (8 float4 per thread)
    const int c4 = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    int64_t rowoff[8];
#pragma unroll
    for (int q = 0; q < 8; q++) rowoff[q] = rows[r0 + 8 * q] >= 0 ? (int64_t)rows[r0 + 8 * q] * SR : -1;
    float4 xpre[8];
    auto fetch = [&](int nblk) {
        const int k = 128 * nblk + 4 * c4;
#pragma unroll
        for (int q = 0; q < 8; q++)
            xpre[q] = d.layernorm && rowoff[q] >= 0 && k < SR ? *reinterpret_cast<const float4*>(feats + rowoff[q] + k)
                                                             : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    fetch(0);
    for (int nblk = 0; nblk < Kp / 128; nblk++) {
        f32x16 acc[2];
        acc_fill_bias<2>(acc, nullptr, 0, w.lane);
        gemm_acc<H, 2>(Ds + w.rb * 32 * LDD, LDD, Wpb, H / 8, 0, 4 * nblk + 2 * w.ch, acc, w.lane);
        __syncthreads();  // the previous block's staging tile has been consumed
        acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) { ot[r * lds_ld(128) + c] = v; });
        __syncthreads();
        float4 xcur[8];
#pragma unroll
        for (int q = 0; q < 8; q++) xcur[q] = xpre[q];
        if (nblk + 1 < Kp / 128) fetch(nblk + 1);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int r = r0 + 8 * q, k = 128 * nblk + 4 * c4;
            const int at = rows[r];
            if (at < 0 || k >= SR) continue;
            float4 v = *reinterpret_cast<const float4*>(ot + r * lds_ld(128) + 4 * c4);
            if (d.layernorm) {
                const float4 x = xcur[q];
                const float mu = st[r * 4], rs_ = st[r * 4 + 1], m1 = st[r * 4 + 2], m2 = st[r * 4 + 3];
                v.x = rs_ * (v.x - m1 - (x.x - mu) * rs_ * m2);
                v.y = rs_ * (v.y - m1 - (x.y - mu) * rs_ * m2);
                v.z = rs_ * (v.z - m1 - (x.z - mu) * rs_ * m2);
                v.w = rs_ * (v.w - m1 - (x.w - mu) * rs_ * m2);
            }
            if (enc) {
                const float4 e = *reinterpret_cast<const float4*>(enc + (size_t)sp[at] * d.S + k);
                v.x *= e.x; v.y *= e.y; v.z *= e.z; v.w *= e.w;
            }
            *reinterpret_cast<float4*>(dF + (size_t)at * SR + k) = v;
        }
    }
}

// reverse of the tail: dF[i][k] = d e_i / d ps_i[k] * gA[i]
__global__ __launch_bounds__(256) void k_soap_tail_bwd(SoapDims d, const float* __restrict__ feats,
                                                       const int* __restrict__ sp, const SoapSet* __restrict__ sets,
                                                       const float* __restrict__ enc, const float* __restrict__ tail,
                                                       const float* __restrict__ gA, float* __restrict__ dF,
                                                       const float* __restrict__ da2x) {
    __shared__ float da1[MAXH], da2[MAXH], red[8];
    const int i = blockIdx.x, tid = threadIdx.x;
    const SoapSet W = sets[d.legacy ? sp[i] : 0];
    const float* tl = tail + (size_t)i * (2 + 2 * d.H);
    const float mean = tl[0], rstd = tl[1], g = gA[i];
    if (tid < d.H) {
        if (d.NH > 1) da2[tid] = da2x ? da2x[(size_t)i * d.H + tid] : g * W.w3[tid] * dsilu(tl[2 + d.H + tid]);
        else da1[tid] = g * W.w3[tid] * dsilu(tl[2 + tid]);
    }
    __syncthreads();
    if (tid < d.H && d.NH > 1) {
        float s = 0.f;
        for (int j = 0; j < d.H; j++) s += W.W2[j * d.H + tid] * da2[j];
        da1[tid] = s * dsilu(tl[2 + tid]);
    }
    __syncthreads();
    const float* x = feats + (size_t)i * d.S;
    // pass 1: dxn gamma and the two LayerNorm means
    float s1 = 0.f, s2 = 0.f;
    for (int k = tid; k < d.S; k += 256) {
        float dx = 0.f;
        for (int q = 0; q < d.H; q++) dx += W.W1[(size_t)q * d.S + k] * da1[q];
        if (d.layernorm) {
            dx *= W.ln_w[k];
            s1 += dx;
            s2 += dx * (x[k] - mean) * rstd;
        }
        dF[(size_t)i * d.S + k] = dx;
    }
    if (d.layernorm) {
        const float m1 = block_sum(s1, red) / d.S;
        const float m2 = block_sum(s2, red) / d.S;
        for (int k = tid; k < d.S; k += 256) {
            const float xh = (x[k] - mean) * rstd;
            dF[(size_t)i * d.S + k] = rstd * (dF[(size_t)i * d.S + k] - m1 - xh * m2);
        }
    }
    if (enc) {
        const float* e = enc + (size_t)sp[i] * d.S;
        for (int k = tid; k < d.S; k += 256) dF[(size_t)i * d.S + k] *= e[k];
    }
}

// Hidden layers beyond the second (num_hidden_layers > 2; the reference's MLPMap stacks Linear + SiLU per layer,
// soap_bpnn/model.py). Every tail kernel above keeps a1, a2 and the 4 544-wide first Linear, which is all of the work; one
// wave per atom continues from a2: a_{k+3} = Wh[k+1] silu(a_{k+2}) -> ext[atom][k][H], and replaces the atom's energy.
__global__ __launch_bounds__(256) void k_soap_tail_extra_fwd(SoapDims d, const int* __restrict__ sp,
                                                             const SoapSet* __restrict__ sets,
                                                             const float* __restrict__ tail, float* __restrict__ ext,
                                                             float* __restrict__ atomic, int N) {
    __shared__ float hs[4][MAXH];
    const int wave = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int at = blockIdx.x * 4 + wave;
    if (at >= N) return;  // whole waves leave; no workgroup barrier below
    const int H = d.H, TS = 2 + 2 * H, NX = d.NH - 2;
    const SoapSet* W = sets + (d.legacy ? sp[at] : 0);
    float a = j < H ? tail[(size_t)at * TS + 2 + H + j] : 0.f;
    for (int k = 0; k < NX; k++) {
        if (j < H) hs[wave][j] = silu(a);
        __builtin_amdgcn_wave_barrier();
        float s = 0.f;
        if (j < H) {
            const float* w = W->Wh[k + 1] + (size_t)j * H;
            for (int q = 0; q < H; q++) s += w[q] * hs[wave][q];
            ext[((size_t)at * NX + k) * H + j] = s;
        }
        a = s;
        __builtin_amdgcn_wave_barrier();
    }
    float e = j < H ? W->w3[j] * silu(a) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if (j == 0) atomic[at] = e;
}

// ... and its reverse down to d a2 [N, H], which the tail adjoints then start from instead of gA w3 silu'(a2)
__global__ __launch_bounds__(256) void k_soap_tail_extra_bwd(SoapDims d, const int* __restrict__ sp,
                                                             const SoapSet* __restrict__ sets,
                                                             const float* __restrict__ tail,
                                                             const float* __restrict__ ext, const float* __restrict__ gA,
                                                             float* __restrict__ da2, int N) {
    __shared__ float ds[4][MAXH];
    const int wave = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int at = blockIdx.x * 4 + wave;
    if (at >= N) return;
    const int H = d.H, TS = 2 + 2 * H, NX = d.NH - 2;
    const SoapSet* W = sets + (d.legacy ? sp[at] : 0);
    float da = j < H ? gA[at] * W->w3[j] * dsilu(ext[((size_t)at * NX + NX - 1) * H + j]) : 0.f;
    for (int k = NX - 1; k >= 0; k--) {  // through a_{k+3} = Wh[k+1] silu(a_{k+2})
        if (j < H) ds[wave][j] = da;
        __builtin_amdgcn_wave_barrier();
        float s = 0.f;
        if (j < H) {
            const float* w = W->Wh[k + 1];
            for (int q = 0; q < H; q++) s += w[(size_t)q * H + j] * ds[wave][q];
            const float aprev = k > 0 ? ext[((size_t)at * NX + k - 1) * H + j] : tail[(size_t)at * TS + 2 + H + j];
            s *= dsilu(aprev);
        }
        da = s;
        __builtin_amdgcn_wave_barrier();
    }
    if (j < H) da2[(size_t)at * H + j] = da;
}


// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int soap_bucket(bool wide, const int* sp, int legacy, int N, int n_sets, void* info, int* perm, const int** offs,
                hipStream_t st) {
    return wide ? sp_bucket<SP_TRAIN_MAXSETS>(sp, legacy, N, n_sets, info, perm, offs, st)
                : sp_bucket<SP_MAXSETS>(sp, legacy, N, n_sets, info, perm, offs, st);
}

// f(NT as a compile-time constant): the stacked kernels' instantiation for NT 64-column tiles (two networks each)
template <class F>
static void with_nt(int NT, F&& f) {
    switch (NT) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    }
}

int launch_soap_tail(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, float* atomic, hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    {
        ProfScope ps("soap_tail", st, 2.0 * (double)N * d.S * d.H, (double)N * (p.packed ? d.Sp : d.S) * 4);
        switch (p.tail) {
        case SoapPlan::Tail::Sorted: {
            PET_TRY(soap_bucket(false, g.sp, d.legacy, N, m.n_sets, w.info, w.perm, nullptr, st));
            const size_t lds = ((size_t)BM * lds_ld(128) + BM * 32 + BM) * 4;
            SoapDims dt = d;
            if (p.packed) dt.S = d.Sp;  // (the kernel uses S as the row pitch / length of the feature rows only)
            k_soap_tail_fwd_set<<<cdiv(N, BM) + m.n_sets, NTHREADS, lds, st>>>(
                dt, w.feats, w.perm, w.info, m.n_sets, m.sets, p.packed ? m.wallp_fwd_set : m.wall_fwd_set,
                p.packed ? m.Kpp : m.Kp, m.wall_rs, m.wall_b, w.tail, atomic);
            break;
        }
        case SoapPlan::Tail::Stacked: {
            const int lda = lds_ld(128);
            const size_t lds = ((size_t)BM * (m.NOUTP + 1 > lda ? m.NOUTP + 1 : lda) + BM * 32) * 4;
            with_nt(m.NT, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                allow_big_lds(k_soap_tail_fwd_mfma<NT>, lds);
                k_soap_tail_fwd_mfma<NT><<<cdiv(N, BM), NTHREADS, lds, st>>>(d, w.feats, g.sp, m.sets, m.wall_fwd, m.Kp,
                                                                            m.wall_rs, m.wall_b, w.tail, atomic, N);
            });
            break;
        }
        case SoapPlan::Tail::PerAtom: {
            const size_t lds = ((size_t)d.S + 256 * (d.H + 1) + 8 + 2 * d.H) * 4;
            allow_big_lds(k_soap_tail, lds);
            k_soap_tail<<<N, 256, lds, st>>>(d, w.feats, g.sp, m.sets, w.tail, atomic);
            break;
        }
        }
    }
    if (p.deep_tail) k_soap_tail_extra_fwd<<<cdiv(N, 4), 256, 0, st>>>(d, g.sp, m.sets, w.tail, w.tail_ext, atomic, N);
    return PET_OK;
}

void launch_soap_tail_bwd(const SoapPlan& p, const SoapModel& m, const Graph& g, const SoapWs& w, const float* gA,
                          hipStream_t st) {
    const SoapDims& d = m.d;
    const int N = (int)g.n_nodes;
    const float* da2x = nullptr;  // a deep tail: the adjoint of a2, from which the tail adjoints start instead of gA
    if (p.deep_tail) {
        k_soap_tail_extra_bwd<<<cdiv(N, 4), 256, 0, st>>>(d, g.sp, m.sets, w.tail, w.tail_ext, gA, w.da2, N);
        da2x = w.da2;
    }
    ProfScope ps("soap_tail_bwd", st, 2.0 * (double)N * d.S * d.H, (double)N * (p.packed ? d.Sp : d.S) * 8);
    switch (p.tail) {
    case SoapPlan::Tail::Sorted: {  // perm / info: filled by the forward pass on this workspace (soap_plan_backward asks its record)
        const size_t lds = ((size_t)BM * lds_ld(32) + BM * 32 + BM * 4 + BM * lds_ld(128) + BM) * 4;
        k_soap_tail_bwd_set<<<cdiv(N, BM) + m.n_sets, NTHREADS, lds, st>>>(
            d, w.feats, w.perm, w.info, m.n_sets, g.sp, m.sets, p.packed ? m.wallp_bwd_set : m.wall_bwd_set,
            p.packed ? m.Kpp : m.Kp, m.wall_rs, m.wall_b, m.enc, w.tail, gA, w.dF, da2x, p.packed ? 1 : 0);
        break;
    }
    case SoapPlan::Tail::Stacked: {
        const size_t lds = ((size_t)BM * lds_ld(m.NOUTP) + BM * 32 + BM * 4 + BM * lds_ld(128)) * 4;
        with_nt(m.NT, [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            allow_big_lds(k_soap_tail_bwd_mfma<NT>, lds);
            k_soap_tail_bwd_mfma<NT><<<cdiv(N, BM), NTHREADS, lds, st>>>(d, w.feats, g.sp, m.sets, m.wall_bwd, m.Kp, m.wall_rs,
                                                                        m.wall_b, m.enc, w.tail, gA, w.dF, N, da2x);
        });
        break;
    }
    case SoapPlan::Tail::PerAtom:
        k_soap_tail_bwd<<<N, 256, 0, st>>>(d, w.feats, g.sp, m.sets, m.enc, w.tail, gA, w.dF, da2x);
        break;
    }
}

}  // namespace pet
