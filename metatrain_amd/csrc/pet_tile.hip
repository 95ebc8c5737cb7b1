// The LDS-tile kernels of the tuned PET pass, both directions, and their launchers (pet_stages.h tile_*): 64-row tiles in LDS, fp32
// MFMA (f16x3 where a stage's rows are un-normalised and the weight was packed). The one fallback of every row stage, and the
// transformer layers of PostLN models and the residual featuriser. pet_fwd.hip has the token layout and the reference map.
//
// Every dense adjoint is a row-tile GEMM against the TRANSPOSED weight (Lin::bwd packs W^T in fragment order), so the same MFMA
// toolkit applies. Cross-atom terms are gathers, never float atomics.
#include "pet_stages.h"
#include "pet_tile.h"

namespace pet {

// ---------------------------------------------------------------------------------
// compress: a0 = [v,d] Wc^T + Tbl[species] (+ M W0c^T);  e = SiLU(a0) W2^T + b2
// ---------------------------------------------------------------------------------
template <bool FIRST>
__global__ __launch_bounds__(NTHREADS) void k_compress(const float4* __restrict__ geo,
                                                        const int* __restrict__ sp_nbr,
                                                        const float* __restrict__ wc,   // [D,4]
                                                        const float* __restrict__ tbl,  // [ns,D]
                                                        const float* __restrict__ Min,  // [E,D] (!FIRST)
                                                        WX w0c, WX w2,
                                                        const float* __restrict__ b2,
                                                        float* __restrict__ a0_out,  // [E,D] or null
                                                        float* __restrict__ Xout,    // [E,D]
                                                        int64_t E) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* S = smem;                 // [64][132]
    float* A = smem + BM * LD128;    // [64][132] (!FIRST)
    float4* geo_s = reinterpret_cast<float4*>(smem + (FIRST ? 1 : 2) * BM * LD128);  // [64]
    int* sp_s = reinterpret_cast<int*>(geo_s + BM);                                   // [64]
    float* rs = reinterpret_cast<float*>(sp_s + BM);  // [64][2] power-of-two row scales for the f16x3 GEMMs
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    if (threadIdx.x < BM) {
        int64_t p = row0 + threadIdx.x;
        geo_s[threadIdx.x] = p < E ? geo[p] : make_float4(0, 0, 0, 0);
        sp_s[threadIdx.x] = p < E ? sp_nbr[p] : 0;
    }
    if (!FIRST) load_rows_to_lds<128>(A, Min, row0, E, D);
    __syncthreads();
    if (!FIRST && w0c.h) {  // messages: un-normalised rows
        tile_row_scales<128>(A, LD128, rs);
        __syncthreads();
    }
    if (FIRST) {
        const int c = threadIdx.x & 127;
        const float4 wv = reinterpret_cast<const float4*>(wc)[c];
        for (int r = threadIdx.x >> 7; r < BM; r += 2) {
            float4 g = geo_s[r];
            float a = fmaf(g.w, wv.w, fmaf(g.z, wv.z, fmaf(g.y, wv.y, g.x * wv.x))) + tbl[sp_s[r] * D + c];
            if (a0_out && row0 + r < E) a0_out[(row0 + r) * D + c] = a;
            S[r * LD128 + c] = siluf_(a);
        }
    } else {
        f32x16 acc[2];
        const int col0 = 64 * w.ch;
        acc_fill_bias<2>(acc, nullptr, 0, w.lane);
        gemm_acc_x<128, 2>(A + w.rb * 32 * LD128, LD128, w0c, 16, 0, 2 * w.ch, acc, w.lane, w0c.h ? rs + 64 * w.rb : nullptr);
        // The geometry / species terms are added AFTER the GEMM. With them pre-filled into `acc` and live across
        // gemm_acc_x, a few (row, 16-column) groups of the result came out different from launch to launch
        // (same inputs, same weights; lanes 48..63 of one wave): not understood, avoided by this order.
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int c = col0 + 32 * t + (w.lane & 31);
            const float4 wv = reinterpret_cast<const float4*>(wc)[c];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = w.rb * 32 + acc_row(r, w.lane);
                float4 g = geo_s[row];
                acc[t][r] += fmaf(g.w, wv.w, fmaf(g.z, wv.z, fmaf(g.y, wv.y, g.x * wv.x))) + tbl[sp_s[row] * D + c];
            }
        }
        acc_foreach<2>(acc, w.rb, col0, w.lane, [&](int r, int c, float v) {
            if (a0_out && row0 + r < E) a0_out[(row0 + r) * D + c] = v;
            S[r * LD128 + c] = siluf_(v);
        });
    }
    __syncthreads();
    if (w2.h) {
        tile_row_scales<128>(S, LD128, rs);
        __syncthreads();
    }
    f32x16 acc2[2];
    acc_fill_bias<2>(acc2, b2, 64 * w.ch, w.lane);
    gemm_acc_x<128, 2>(S + w.rb * 32 * LD128, LD128, w2, 16, 0, 2 * w.ch, acc2, w.lane, w2.h ? rs + 64 * w.rb : nullptr);
    store_acc<2>(acc2, Xout, row0, E, D, w.rb, 64 * w.ch, w.lane);
}

// ---------------------------------------------------------------------------------
// centre contraction: X[E + i] = H[i] Wcc^T + b   (DN -> D)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_center(const float* __restrict__ H, WX wcc,
                                                      const float* __restrict__ bcc, float* __restrict__ Xc,
                                                      int64_t N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    float* rs = smem + BM * LD256;  // [64][2] power-of-two row scales: node features are un-normalised rows
    load_rows_to_lds<256>(smem, H, row0, N, DN);
    __syncthreads();
    if (wcc.h) {
        tile_row_scales<256>(smem, LD256, rs);
        __syncthreads();
    }
    f32x16 acc[2];
    acc_fill_bias<2>(acc, bcc, 64 * w.ch, w.lane);
    gemm_acc_x<256, 2>(smem + w.rb * 32 * LD256, LD256, wcc, 32, 0, 2 * w.ch, acc, w.lane, wcc.h ? rs + 64 * w.rb : nullptr);
    store_acc<2>(acc, Xc, row0, N, D, w.rb, 64 * w.ch, w.lane);
}

// ---------------------------------------------------------------------------------
// QKV = Norm(X) Win^T + b   (D -> 3D) over all E+N token rows; Norm = RMSNorm, LayerNorm (beta) or, for PostLN
// (transformer.py:243: attention on the raw tokens), nothing
// ---------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(NTHREADS) void k_qkv(const float* __restrict__ X, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta,
                                                   const float4* __restrict__ win, const float* __restrict__ bin,
                                                   float* __restrict__ QKV, int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(smem, X, row0, R, D);
    __syncthreads();
    if (NORM) {
        norm_rows_inplace<128>(smem, gamma, beta);
        __syncthreads();
    }
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        f32x16 acc[2];
        const int col0 = 128 * c + 64 * w.ch;
        acc_fill_bias<2>(acc, bin, col0, w.lane);
        gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, win, 16, 0, 4 * c + 2 * w.ch, acc, w.lane);
        store_acc<2>(acc, QKV, row0, R, 3 * D, w.rb, col0, w.lane);
    }
}

// ---------------------------------------------------------------------------------
// output_linear + edge residual:  rows < E: X1 = X + AO Wo^T + b ; rows >= E: OC = AO Wo^T + b
// POST (transformer.py:243-245): every token keeps its residual, X1 = X + AO Wo^T + b on all E+N rows
// ---------------------------------------------------------------------------------
template <bool POST>
__global__ __launch_bounds__(NTHREADS) void k_oproj(const float* __restrict__ AO, const float* __restrict__ X,
                                                     const float4* __restrict__ wo, const float* __restrict__ bo,
                                                     float* __restrict__ X1, float* __restrict__ OC, int64_t E,
                                                     int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(smem, AO, row0, R, D);
    __syncthreads();
    f32x16 acc[2];
    acc_fill_bias<2>(acc, bo, 64 * w.ch, w.lane);
    gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, wo, 16, 0, 2 * w.ch, acc, w.lane);
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const int64_t row = row0 + r;
        if (row < E || (POST && row < R)) X1[row * D + c] = X[row * D + c] + v;
        else if (row < R) OC[(row - E) * D + c] = v;
    });
}

// ---------------------------------------------------------------------------------
// edge MLP: X2 = X1 + SwiGLU_MLP(Norm(X1)); PostLN (NORM = false, transformer.py:246-247): X2 = X1 + SwiGLU_MLP(X1) on
// already-normalised tokens, centre rows included (E = the row count)
// ---------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(NTHREADS) void k_emlp(const float* __restrict__ X1, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta,
                                                    const float4* __restrict__ win, const float* __restrict__ bin,
                                                    const float4* __restrict__ wout, const float* __restrict__ bout,
                                                    float* __restrict__ VG, float* __restrict__ X2, int64_t E) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* A = smem;               // [64][132]
    float* U = smem + BM * LD128;  // [64][132]
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(A, X1, row0, E, D);
    __syncthreads();
    if (NORM) {
        norm_rows_inplace<128>(A, gamma, beta);
        __syncthreads();
    }
    f32x16 out[2];
    acc_fill_bias<2>(out, bout, 64 * w.ch, w.lane);
#pragma unroll 1
    for (int hc = 0; hc < DFF / 128; hc++) {
        f32x16 av[2], ag[2];
        const int hcol0 = 128 * hc + 64 * w.ch;
        acc_fill_bias<2>(av, bin, hcol0, w.lane);
        acc_fill_bias<2>(ag, bin, DFF + hcol0, w.lane);
        gemm_acc<128, 2>(A + w.rb * 32 * LD128, LD128, win, 16, 0, hcol0 / 32, av, w.lane);
        gemm_acc<128, 2>(A + w.rb * 32 * LD128, LD128, win, 16, 0, (DFF + hcol0) / 32, ag, w.lane);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = w.rb * 32 + acc_row(r, w.lane);
                const int cc = 64 * w.ch + 32 * t + (w.lane & 31);
                const float v = av[t][r], gte = ag[t][r];
                if (VG && row0 + rr < E) {
                    VG[(row0 + rr) * (2 * DFF) + 128 * hc + cc] = v;
                    VG[(row0 + rr) * (2 * DFF) + DFF + 128 * hc + cc] = gte;
                }
                U[rr * LD128 + cc] = v * sigmoidf_(gte);
            }
        }
        __syncthreads();
        gemm_acc<128, 2>(U + w.rb * 32 * LD128, LD128, wout, DFF / 8, 16 * hc, 2 * w.ch, out, w.lane);
    }
    acc_foreach<2>(out, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const int64_t row = row0 + r;
        if (row < E) X2[row * D + c] = X1[row * D + c] + v;
    });
}

// ---------------------------------------------------------------------------------
// PostLN: Y = Norm(S) row by row (transformer.py:245,247); rows < E go to Ye, rows >= E (the centre tokens) to Yc
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_rownorm(const float* __restrict__ S, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ Ye,
                                                       float* __restrict__ Yc, int64_t E, int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(smem, S, row0, R, D);
    __syncthreads();
    norm_rows_inplace<128>(smem, gamma, beta);
    __syncthreads();
    for (int idx = threadIdx.x; idx < BM * 32; idx += NTHREADS) {
        const int r = idx >> 5, c = idx & 31;
        const int64_t row = row0 + r;
        if (row >= R) continue;
        const float4 v = *reinterpret_cast<const float4*>(smem + r * LD128 + 4 * c);
        if (row < E) *reinterpret_cast<float4*>(Ye + row * D + 4 * c) = v;
        else *reinterpret_cast<float4*>(Yc + (row - E) * D + 4 * c) = v;
    }
}

// ---------------------------------------------------------------------------------
// residual featuriser (backend.py:621-647): Mout[p] = 0.5 (Min[p] + e[rev[p]]); layer 0: Min = edge_embedder[species]
// ---------------------------------------------------------------------------------
__global__ void k_resmix(const float* __restrict__ Min, const float* __restrict__ emb, const int* __restrict__ sp_nbr,
                         const float* __restrict__ XF, const int* __restrict__ rev, float* __restrict__ Mout, int64_t E) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * (D / 4)) return;
    const int64_t p = idx / (D / 4);
    const int c = (int)(idx % (D / 4));
    const float4 a = Min ? reinterpret_cast<const float4*>(Min)[idx]
                         : *reinterpret_cast<const float4*>(emb + (int64_t)sp_nbr[p] * D + 4 * c);
    const float4 b = *reinterpret_cast<const float4*>(XF + (int64_t)rev[p] * D + 4 * c);
    reinterpret_cast<float4*>(Mout)[idx] = make_float4(0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z),
                                                       0.5f * (a.w + b.w));
}

// ---------------------------------------------------------------------------------
// heads: y = w . SiLU(W2 SiLU(W0 x + b0) + b2) + b     (backend.py:171-217, 726-777)
// ---------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(NTHREADS) void k_head(const float* __restrict__ Xin, WX w0,
                                                    const float* __restrict__ b0, WX w2,
                                                    const float* __restrict__ b2, const float* __restrict__ wl,
                                                    float bl, const float* __restrict__ fc /* or null */,
                                                    float* __restrict__ ypred, float* __restrict__ yout,
                                                    int64_t R, float* __restrict__ hidden = nullptr, int ldh = 0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LDK = lds_ld(K);
    float* A = smem;              // [64][K+4]
    float* S = smem + BM * LDK;   // [64][132]
    float* rs = S + BM * LD128;   // [64][2] row scales: backbone features and the hidden rows are un-normalised
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<K>(A, Xin, row0, R, K);
    __syncthreads();
    if (w0.h) {
        tile_row_scales<K>(A, LDK, rs);
        __syncthreads();
    }
    f32x16 acc[2];
    acc_fill_bias<2>(acc, b0, 64 * w.ch, w.lane);
    gemm_acc_x<K, 2>(A + w.rb * 32 * LDK, LDK, w0, K / 8, 0, 2 * w.ch, acc, w.lane, w0.h ? rs + 64 * w.rb : nullptr);
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) { S[r * LD128 + c] = siluf_(v); });
    __syncthreads();
    if (w2.h) {
        tile_row_scales<128>(S, LD128, rs);
        __syncthreads();
    }
    acc_fill_bias<2>(acc, b2, 64 * w.ch, w.lane);
    gemm_acc_x<128, 2>(S + w.rb * 32 * LD128, LD128, w2, 16, 0, 2 * w.ch, acc, w.lane, w2.h ? rs + 64 * w.rb : nullptr);
    __syncthreads();
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const float a = siluf_(v);
        if (hidden && row0 + r < R) hidden[(row0 + r) * ldh + c] = a;  // last-layer features (pet_aux_outputs)
        S[r * LD128 + c] = a * wl[c];
    });
    __syncthreads();
    {
        const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
        float s = 0.f;
        for (int c = q * 4; c < 128; c += 16) {
            float4 v = *reinterpret_cast<float4*>(S + r * LD128 + c);
            s += v.x + v.y + v.z + v.w;
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (q == 0 && row0 + r < R) {
            const float y = s + bl;
            if (ypred) ypred[row0 + r] = y;
            yout[row0 + r] = fc ? y * fc[row0 + r] : y;
        }
    }
}

// ---------------------------------------------------------------------------------
// heads
// ---------------------------------------------------------------------------------
// GEN (pet_predict_backward: any number of properties, features given by the caller): the gradient w.r.t. the head's
// hidden row arrives as a per-atom row Gd[atom][DH] = sum_p gA[atom][p] Wl[p][:] (instead of gA[atom] * wl), and the
// cutoff-factor gradient is dfc = Gd[atom] . hidden + gb[atom] (gb = sum_p gA[atom][p] bl[p]) from the recomputed hidden row.
template <int K, bool EDGE, bool TRAIN, bool GEN = false>
__global__ __launch_bounds__(NTHREADS) void k_head_bwd(const float* __restrict__ Xin, WX w0f,
                                                        const float* __restrict__ b0, WX w2f,
                                                        const float* __restrict__ b2, WX w0b,
                                                        WX w2b, const float* __restrict__ wl,
                                                        const float* __restrict__ gA, const int* __restrict__ ctr,
                                                        const float* __restrict__ fc, const float* __restrict__ ypred,
                                                        float* __restrict__ dfc, float* __restrict__ dXout, int64_t R,
                                                        float* __restrict__ t_s1, float* __restrict__ t_da2,
                                                        float* __restrict__ t_da1, float* __restrict__ t_s2y,
                                                        const float* __restrict__ Gd = nullptr,
                                                        const float* __restrict__ gb = nullptr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LDK = lds_ld(K);
    float* A = smem;
    float* S = smem + BM * LDK;
    float* gy = S + BM * LD128;  // [64]
    float* rs = gy + BM;         // [64][2] power-of-two row scales of the adjoint tiles (f16x3 GEMMs)
    int* at = reinterpret_cast<int*>(rs + 2 * BM);  // [64] GEN: atom of the row (Gd / gb row index)
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<K>(A, Xin, row0, R, K);
    if (threadIdx.x < BM) {
        const int64_t row = row0 + threadIdx.x;
        float g = 0.f;
        if (row < R) {
            if (GEN) {
                g = EDGE ? fc[row] : 1.0f;
                at[threadIdx.x] = EDGE ? ctr[row] : (int)row;
            } else if (EDGE) {
                const float ga = gA[ctr[row]];
                g = ga * fc[row];
                dfc[row] = ga * ypred[row];  // d(y fc)/dfc
            } else {
                g = gA[row];
            }
        } else if (GEN) {
            at[threadIdx.x] = 0;
        }
        gy[threadIdx.x] = g;
    }
    __syncthreads();
    if (w0f.h) {  // the forward kernel's row scales (k_head): un-normalised backbone features and hidden rows
        tile_row_scales<K>(A, LDK, rs);
        __syncthreads();
    }
    f32x16 a1[2], acc[2];
    acc_fill_bias<2>(a1, b0, 64 * w.ch, w.lane);
    gemm_acc_x<K, 2>(A + w.rb * 32 * LDK, LDK, w0f, K / 8, 0, 2 * w.ch, a1, w.lane, w0f.h ? rs + 64 * w.rb : nullptr);
    acc_foreach<2>(a1, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const float s1 = siluf_(v);
        S[r * LD128 + c] = s1;
        if (TRAIN && row0 + r < R) t_s1[(row0 + r) * DH + c] = s1;
    });
    __syncthreads();
    if (w2f.h) {
        tile_row_scales<128>(S, LD128, rs);
        __syncthreads();
    }
    acc_fill_bias<2>(acc, b2, 64 * w.ch, w.lane);
    gemm_acc_x<128, 2>(S + w.rb * 32 * LD128, LD128, w2f, 16, 0, 2 * w.ch, acc, w.lane, w2f.h ? rs + 64 * w.rb : nullptr);
    __syncthreads();
    if (GEN && EDGE) {  // dfc[row] = Gd[atom] . silu(a2) + gb[atom]
        acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
            S[r * LD128 + c] = siluf_(v) * Gd[(int64_t)at[r] * DH + c];
        });
        __syncthreads();
        {
            const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
            float sum = 0.f;
            for (int c = q * 4; c < 128; c += 16) {
                const float4 v = *reinterpret_cast<float4*>(S + r * LD128 + c);
                sum += v.x + v.y + v.z + v.w;
            }
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            if (q == 0 && row0 + r < R) dfc[row0 + r] = sum + gb[at[r]];
        }
        __syncthreads();
    }
    // da2 = gy * wl * silu'(a2)
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const float d2 = gy[r] * (GEN ? Gd[(int64_t)at[r] * DH + c] : wl[c]) * silu_grad_(v);
        S[r * LD128 + c] = d2;
        if (TRAIN && row0 + r < R) {
            t_da2[(row0 + r) * DH + c] = d2;
            t_s2y[(row0 + r) * DH + c] = gy[r] * siluf_(v);
        }
    });
    __syncthreads();
    acc_fill_bias<2>(acc, nullptr, 0, w.lane);
    if (w2b.h) {
        tile_row_scales<128>(S, LD128, rs);
        __syncthreads();
    }
    gemm_acc_x<128, 2>(S + w.rb * 32 * LD128, LD128, w2b, 16, 0, 2 * w.ch, acc, w.lane,
                       w2b.h ? rs + 64 * w.rb : nullptr);  // ds1 = da2 W2
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int rr = w.rb * 32 + acc_row(r, w.lane), cc = 64 * w.ch + 32 * t + (w.lane & 31);
            const float d1 = acc[t][r] * silu_grad_(a1[t][r]);
            S[rr * LD128 + cc] = d1;  // da1
            if (TRAIN && row0 + rr < R) t_da1[(row0 + rr) * DH + cc] = d1;
        }
    __syncthreads();
    constexpr int NTO = K / 64;  // output columns K split over the two column halves
    f32x16 dx[NTO];
    acc_fill_bias<NTO>(dx, nullptr, 0, w.lane);
    if (w0b.h) {
        tile_row_scales<128>(S, LD128, rs);
        __syncthreads();
    }
    gemm_acc_x<128, NTO>(S + w.rb * 32 * LD128, LD128, w0b, 16, 0, NTO * w.ch, dx, w.lane,
                         w0b.h ? rs + 64 * w.rb : nullptr);  // dx = da1 W0
    acc_foreach<NTO>(dx, w.rb, (K / 2) * w.ch, w.lane, [&](int r, int c, float v) {
        if (row0 + r < R) dXout[(row0 + r) * K + c] = v;
    });
}

// dXF[p] = dM[p] + dcat[p][:D] + dcat[rev[p]][D:]   (inference graphs on one rank: formed inside k_comb_bwd_p2 / k_emlp_bwd_p2
// instead -- `dxf_fused` in backward())
__global__ void k_dxf(const float* __restrict__ dM, const float* __restrict__ dcat, const int* __restrict__ rev,
                      float* __restrict__ dX, int64_t E) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * (D / 4)) return;
    const int64_t p = idx / (D / 4);
    const int c = (int)(idx % (D / 4));
    float4 a = reinterpret_cast<const float4*>(dM)[idx];
    float4 b = *reinterpret_cast<const float4*>(dcat + p * (2 * D) + 4 * c);
    float4 d = *reinterpret_cast<const float4*>(dcat + (int64_t)rev[p] * (2 * D) + D + 4 * c);
    reinterpret_cast<float4*>(dX)[idx] = make_float4(a.x + b.x + d.x, a.y + b.y + d.y, a.z + b.z + d.z, a.w + b.w + d.w);
}

// ---------------------------------------------------------------------------------
// SwiGLU MLP adjoint (edge rows: K = 128, hidden 256; node rows: K = 256, hidden 512)
//   y = x + Wout (v * sig(g)),  [v; g] = Win RMSNorm(x)
//   dx = dy + RMSNorm^T( Win^T [du sig(g) ; du v sig'(g)] ),  du = Wout^T dy
// ---------------------------------------------------------------------------------
// NORM = false (PostLN, transformer.py:246-247: the MLP reads already-normalised tokens): dx = dy + Win^T [..]; ln: LayerNorm
template <int K, int HID, bool TRAIN, bool NORM = true>
__global__ __launch_bounds__(NTHREADS) void k_swiglu_bwd(const float* __restrict__ dY, const float* __restrict__ Xin,
                                                          const float* __restrict__ VG, const float* __restrict__ gamma,
                                                          const float4* __restrict__ woutb, const float4* __restrict__ winb,
                                                          float* __restrict__ dXout, int64_t R, float* __restrict__ t_dvg,
                                                          bool ln = false) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LDK = lds_ld(K);
    constexpr int NTO = K / 64;
    float* A = smem;              // [64][K+4]: dY tile, later w = gamma * dn
    float* U = smem + BM * LDK;   // [64][132]
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<K>(A, dY, row0, R, K);
    __syncthreads();
    f32x16 dn[NTO];
    acc_fill_bias<NTO>(dn, nullptr, 0, w.lane);
#pragma unroll 1
    for (int hc = 0; hc < HID / 128; hc++) {
        f32x16 du[2];
        acc_fill_bias<2>(du, nullptr, 0, w.lane);
        // du chunk = dY Wout[:, chunk]  (woutb: rows = hidden, k = K)
        gemm_acc<K, 2>(A + w.rb * 32 * LDK, LDK, woutb, K / 8, 0, 4 * hc + 2 * w.ch, du, w.lane);
        float sg[2][16], vv[2][16];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t row = row0 + w.rb * 32 + acc_row(r, w.lane);
                const int cc = 128 * hc + 64 * w.ch + 32 * t + (w.lane & 31);
                float v = 0.f, g = 0.f;
                if (row < R) {
                    v = VG[row * (2 * HID) + cc];
                    g = VG[row * (2 * HID) + HID + cc];
                }
                sg[t][r] = sigmoidf_(g);
                vv[t][r] = v;
            }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = w.rb * 32 + acc_row(r, w.lane), cc = 64 * w.ch + 32 * t + (w.lane & 31);
                const float dvv = du[t][r] * sg[t][r];
                U[rr * LD128 + cc] = dvv;  // dv
                if (TRAIN && row0 + rr < R) t_dvg[(row0 + rr) * (2 * HID) + 128 * hc + cc] = dvv;
            }
        __syncthreads();
        gemm_acc<128, NTO>(U + w.rb * 32 * LD128, LD128, winb, 2 * HID / 8, 16 * hc, NTO * w.ch, dn, w.lane);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = w.rb * 32 + acc_row(r, w.lane), cc = 64 * w.ch + 32 * t + (w.lane & 31);
                const float dgv = du[t][r] * vv[t][r] * sigmoid_grad_from(sg[t][r]);
                U[rr * LD128 + cc] = dgv;  // dg
                if (TRAIN && row0 + rr < R) t_dvg[(row0 + rr) * (2 * HID) + HID + 128 * hc + cc] = dgv;
            }
        __syncthreads();
        gemm_acc<128, NTO>(U + w.rb * 32 * LD128, LD128, winb, 2 * HID / 8, HID / 8 + 16 * hc, NTO * w.ch, dn, w.lane);
    }
    if (!NORM) {
        acc_foreach<NTO>(dn, w.rb, (K / 2) * w.ch, w.lane, [&](int r, int c, float v) {
            const int64_t row = row0 + r;
            if (row < R) dXout[row * K + c] = dY[row * K + c] + v;
        });
        return;
    }
    __syncthreads();  // everyone is done with the dY tile in A
    acc_foreach<NTO>(dn, w.rb, (K / 2) * w.ch, w.lane, [&](int r, int c, float v) { A[r * LDK + c] = v * gamma[c]; });
    __syncthreads();
    norm_bwd_rows<K>(A, Xin, row0, R, K, ln, [&](int r, int c, float4 dx) {
        const int64_t o = (row0 + r) * K + c;
        float4 dy = *reinterpret_cast<const float4*>(dY + o);
        *reinterpret_cast<float4*>(dXout + o) = make_float4(dy.x + dx.x, dy.y + dx.y, dy.z + dx.z, dy.w + dx.w);
    });
}

// ---------------------------------------------------------------------------------
// node chain adjoint, second half: dOC = dH1 Wce ; (dH_in = dH1 is finished by k_center_bwd)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_expand_bwd(const float* __restrict__ dH1, const float4* __restrict__ wceb,
                                                          float* __restrict__ dOC, int64_t N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<256>(smem, dH1, row0, N, DN);
    __syncthreads();
    f32x16 acc[2];
    acc_fill_bias<2>(acc, nullptr, 0, w.lane);
    gemm_acc<256, 2>(smem + w.rb * 32 * LD256, LD256, wceb, 32, 0, 2 * w.ch, acc, w.lane);
    __syncthreads();  // the dH1 tile is consumed: its memory stages the float4 row stores (tile.h wave_rows64)
    const int64_t wrow0 = row0 + 32 * w.rb;
    wave_rows64(acc, smem + w.wave * (32 * 64), w.lane, [&](int r, int cc, float4 v) {
        if (wrow0 + r < N) *reinterpret_cast<float4*>(dOC + (wrow0 + r) * D + 64 * w.ch + cc) = v;
    });
}

// dH_in = dH1 + dC Wcc   (centre contraction adjoint); DEEP (small graphs): eight weight blocks in flight
template <bool DEEP>
__global__ __launch_bounds__(NTHREADS) void k_center_bwd(const float* __restrict__ dC, const float* __restrict__ dH1,
                                                          const float4* __restrict__ wccb, float* __restrict__ dHin,
                                                          int64_t N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(smem, dC, row0, N, D);
    __syncthreads();
    f32x16 acc[4];
    acc_fill_bias<4>(acc, nullptr, 0, w.lane);
    if constexpr (DEEP) gemm_acc_deep<128, 4, 8>(smem + w.rb * 32 * LD128, LD128, wccb, 16, 0, 4 * w.ch, acc, w.lane);
    else gemm_acc<128, 4>(smem + w.rb * 32 * LD128, LD128, wccb, 16, 0, 4 * w.ch, acc, w.lane);
    __syncthreads();  // the dC tile is consumed: its memory stages float4 row traffic (tile.h wave_rows64)
    const int64_t wrow0 = row0 + 32 * w.rb;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const f32x16 pair[2] = {acc[2 * half], acc[2 * half + 1]};
        wave_rows64(pair, smem + w.wave * (32 * 64), w.lane, [&](int r, int cc, float4 v) {
            const int64_t row = wrow0 + r;
            if (row >= N) return;
            const int64_t o = row * DN + 128 * w.ch + 64 * half + cc;
            const float4 d1 = *reinterpret_cast<const float4*>(dH1 + o);
            *reinterpret_cast<float4*>(dHin + o) = make_float4(d1.x + v.x, d1.y + v.y, d1.z + v.z, d1.w + v.w);
        });
    }
}

// ---------------------------------------------------------------------------------
// output_linear adjoint: dAO = dOut Wo, rows < E from dX1, rows >= E from dOC
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_oproj_bwd(const float* __restrict__ dX1, const float* __restrict__ dOC,
                                                         const float4* __restrict__ wob, float* __restrict__ dAO,
                                                         int64_t E, int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    for (int idx = threadIdx.x; idx < BM * 32; idx += NTHREADS) {
        const int r = idx >> 5, c = idx & 31;
        const int64_t row = row0 + r;
        float4 v = make_float4(0, 0, 0, 0);
        if (row < E) v = *reinterpret_cast<const float4*>(dX1 + row * D + 4 * c);
        else if (row < R) v = *reinterpret_cast<const float4*>(dOC + (row - E) * D + 4 * c);
        *reinterpret_cast<float4*>(smem + r * LD128 + 4 * c) = v;
    }
    __syncthreads();
    f32x16 acc[2];
    acc_fill_bias<2>(acc, nullptr, 0, w.lane);
    gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, wob, 16, 0, 2 * w.ch, acc, w.lane);
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        if (row0 + r < R) dAO[(row0 + r) * D + c] = v;
    });
}

// ---------------------------------------------------------------------------------
// input_linear + RMSNorm adjoint: dXin = (rows<E ? dX1 : 0) + RMSNorm^T(dQKV Win)
// ---------------------------------------------------------------------------------
// POST (transformer.py:243-245): no norm in front of input_linear and every token row carries the residual gradient dX1
template <bool POST>
__global__ __launch_bounds__(NTHREADS) void k_qkv_bwd(const float* __restrict__ dQKV, const float* __restrict__ X,
                                                       const float* __restrict__ gamma, const float4* __restrict__ winb,
                                                       const float* __restrict__ dX1, float* __restrict__ dXin,
                                                       int64_t E, int64_t R, bool ln) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    f32x16 dn[2];
    acc_fill_bias<2>(dn, nullptr, 0, w.lane);
#pragma unroll 1
    for (int ks = 0; ks < 3; ks++) {
        __syncthreads();
        load_rows_to_lds<128>(smem, dQKV + 128 * ks, row0, R, 3 * D);
        __syncthreads();
        gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, winb, 48, 16 * ks, 2 * w.ch, dn, w.lane);
    }
    if (POST) {
        acc_foreach<2>(dn, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
            const int64_t row = row0 + r;
            if (row < R) dXin[row * D + c] = dX1[row * D + c] + v;
        });
        return;
    }
    __syncthreads();
    acc_foreach<2>(dn, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) { smem[r * LD128 + c] = v * gamma[c]; });
    __syncthreads();
    norm_bwd_rows<128>(smem, X, row0, R, D, ln, [&](int r, int c, float4 dx) {
        const int64_t row = row0 + r;
        if (row < E) {
            float4 d1 = *reinterpret_cast<const float4*>(dX1 + row * D + c);
            dx.x += d1.x; dx.y += d1.y; dx.z += d1.z; dx.w += d1.w;
        }
        *reinterpret_cast<float4*>(dXin + row * D + c) = dx;
    });
}

// ---------------------------------------------------------------------------------
// PostLN: adjoint of Y = Norm(S) (k_rownorm): rows < E of dY from dYe, rows >= E from dYc; dS on all E+N rows
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_rownorm_bwd(const float* __restrict__ dYe, const float* __restrict__ dYc,
                                                           const float* __restrict__ S, const float* __restrict__ gamma,
                                                           bool ln, float* __restrict__ dS, int64_t E, int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    for (int idx = threadIdx.x; idx < BM * 32; idx += NTHREADS) {
        const int r = idx >> 5, c = idx & 31;
        const int64_t row = row0 + r;
        float4 v = make_float4(0, 0, 0, 0);
        if (row < E) v = *reinterpret_cast<const float4*>(dYe + row * D + 4 * c);
        else if (row < R) v = *reinterpret_cast<const float4*>(dYc + (row - E) * D + 4 * c);
        const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * c);
        *reinterpret_cast<float4*>(smem + r * LD128 + 4 * c) = make_float4(v.x * g.x, v.y * g.y, v.z * g.z, v.w * g.w);
    }
    __syncthreads();
    norm_bwd_rows<128>(smem, S, row0, R, D, ln, [&](int r, int c, float4 dx) {
        *reinterpret_cast<float4*>(dS + (row0 + r) * D + c) = dx;
    });
}

// residual featuriser adjoint (k_resmix): Mout[p] = 0.5 (Min[p] + e[rev[p]]) with rev an involution, so
//   de[p] = ge[p] + 0.5 dMout[rev[p]],  dMin[p] = 0.5 dMout[p];  dMout == nullptr (last layer): de = ge, dMin = 0
__global__ void k_resmix_bwd(const float* __restrict__ ge, const float* __restrict__ dMout, const int* __restrict__ rev,
                             float* __restrict__ de, float* __restrict__ dMin, int64_t E) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * (D / 4)) return;
    const int64_t p = idx / (D / 4);
    const int c = (int)(idx % (D / 4));
    float4 a = ge ? reinterpret_cast<const float4*>(ge)[idx] : make_float4(0, 0, 0, 0);
    float4 mp = make_float4(0, 0, 0, 0);
    if (dMout) {
        const float4 b = *reinterpret_cast<const float4*>(dMout + (int64_t)rev[p] * D + 4 * c);
        a.x += 0.5f * b.x; a.y += 0.5f * b.y; a.z += 0.5f * b.z; a.w += 0.5f * b.w;
        const float4 q = reinterpret_cast<const float4*>(dMout)[idx];
        mp = make_float4(0.5f * q.x, 0.5f * q.y, 0.5f * q.z, 0.5f * q.w);
    }
    reinterpret_cast<float4*>(de)[idx] = a;
    reinterpret_cast<float4*>(dMin)[idx] = mp;
}

// ---------------------------------------------------------------------------------
// compress adjoint: da0 = (dE W2) * silu'(a0); dgeo += da0 Wc; dM = dMpass + da0 W0c
// ---------------------------------------------------------------------------------
template <bool FIRST, bool TRAIN>
__global__ __launch_bounds__(NTHREADS) void k_compress_bwd(const float* __restrict__ dXe, const float* __restrict__ a0,
                                                            const float4* __restrict__ w2b, const float* __restrict__ wct,
                                                            const float4* __restrict__ w0cb, float* __restrict__ dgeo,
                                                            float* __restrict__ dM /* in/out, !FIRST */, int64_t E,
                                                            float* __restrict__ t_da0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(smem, dXe, row0, E, D);
    __syncthreads();
    f32x16 acc[2];
    acc_fill_bias<2>(acc, nullptr, 0, w.lane);
    gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, w2b, 16, 0, 2 * w.ch, acc, w.lane);
    __syncthreads();
    acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
        const int64_t row = row0 + r;
        const float d0v = row < E ? v * silu_grad_(a0[row * D + c]) : 0.f;
        smem[r * LD128 + c] = d0v;
        if (TRAIN && row < E) t_da0[row * D + c] = d0v;
    });
    __syncthreads();
    {   // dgeo[row][k] += sum_c da0[row][c] * Wc[c][k]; 4 threads per row, thread q -> component q
        const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
        const float* wrow = wct + q * D;
        float s = 0.f;
        for (int c = 0; c < 128; c += 4) {
            float4 a = *reinterpret_cast<float4*>(smem + r * LD128 + c);
            float4 ww = *reinterpret_cast<const float4*>(wrow + c);
            s += a.x * ww.x + a.y * ww.y + a.z * ww.z + a.w * ww.w;
        }
        if (row0 + r < E) dgeo[(row0 + r) * 4 + q] += s;
    }
    if (!FIRST) {
        acc_fill_bias<2>(acc, nullptr, 0, w.lane);
        gemm_acc<128, 2>(smem + w.rb * 32 * LD128, LD128, w0cb, 16, 0, 2 * w.ch, acc, w.lane);
        acc_foreach<2>(acc, w.rb, 64 * w.ch, w.lane, [&](int r, int c, float v) {
            const int64_t row = row0 + r;
            if (row < E) dM[row * D + c] += v;
        });
    }
}

// ---------------------------------------------------------------------------------
// launchers (pet_stages.h): one 64-row tile per workgroup of NTHREADS; a kernel's dynamic LDS is stated here and nowhere else
// ---------------------------------------------------------------------------------
constexpr size_t tile_bytes(int K) { return K == 256 ? T256 : T128; }  // (T128 / T256: pet_tile.h)

// the opt-in above 64 KiB belongs to the instantiation that is launched, on the path that launches it (it is sticky per process:
// an opt-in made elsewhere would hide a missing one)
template <class Kern, class... Args>
static int launch_tile(Kern kern, int64_t rows, size_t lds, hipStream_t st, Args... args) {
    allow_big_lds(kern, lds);
    kern<<<cdiv(rows, BM), NTHREADS, lds, st>>>(args...);
    return PET_OK;
}
static inline int grid4(int64_t E) { return cdiv(E * (D / 4), 256); }  // one float4 of an edge row per thread

int tile_compress(bool first, const Graph& g, const GnnLayerW& G, const float* Min, float* a0_out, float* Xout, int64_t E,
                  hipStream_t st) {
    const size_t lds = (first ? 1 : 2) * T128 + BM * 20 + BM * 8;  // S (| message tile) | geometry, species | row scales
    if (first)
        return launch_tile(k_compress<true>, E, lds, st, g.geo, g.sp_nbr, G.wc, G.tbl, nullptr, WX(), wx_fwd(G.compress2),
                           G.compress2.b, a0_out, Xout, E);
    return launch_tile(k_compress<false>, E, lds, st, g.geo, g.sp_nbr, G.wc, G.tbl, Min, wx_fwd(G.compress0_msg),
                       wx_fwd(G.compress2), G.compress2.b, a0_out, Xout, E);
}

int tile_center(const Lin& cc, const float* H, float* Xc, int64_t N, hipStream_t st) {
    return launch_tile(k_center, N, T256 + BM * 8, st, H, wx_fwd(cc), cc.b, Xc, N);
}

int tile_qkv(bool post, const float* X, const float* gamma, const float* beta, const Lin& qkv, float* QKV, int64_t R, hipStream_t st) {
    if (post) return launch_tile(k_qkv<false>, R, T128, st, X, nullptr, nullptr, qkv.fwd, qkv.b, QKV, R);
    return launch_tile(k_qkv<true>, R, T128, st, X, gamma, beta, qkv.fwd, qkv.b, QKV, R);
}

int tile_oproj(bool post, const float* AO, const float* X, const Lin& out, float* X1, float* OC, int64_t E, int64_t R, hipStream_t st) {
    if (post) return launch_tile(k_oproj<true>, R, T128, st, AO, X, out.fwd, out.b, X1, nullptr, E, R);
    return launch_tile(k_oproj<false>, R, T128, st, AO, X, out.fwd, out.b, X1, OC, E, R);
}

int tile_emlp(bool norm, const float* X1, const float* gamma, const float* beta, const Lin& win, const Lin& wout, float* VG, float* X2,
              int64_t rows, hipStream_t st) {
    const size_t lds = 2 * T128;  // normalised rows | SwiGLU chunk
    if (norm) return launch_tile(k_emlp<true>, rows, lds, st, X1, gamma, beta, win.fwd, win.b, wout.fwd, wout.b, VG, X2, rows);
    return launch_tile(k_emlp<false>, rows, lds, st, X1, nullptr, nullptr, win.fwd, win.b, wout.fwd, wout.b, VG, X2, rows);
}

int tile_rownorm(const float* S, const float* gamma, const float* beta, float* Ye, float* Yc, int64_t E, int64_t R, hipStream_t st) {
    return launch_tile(k_rownorm, R, T128, st, S, gamma, beta, Ye, Yc, E, R);
}

int tile_resmix(const float* Min, const float* emb, const int* sp_nbr, const float* XF, const int* rev, float* Mout, int64_t E,
                hipStream_t st) {
    k_resmix<<<grid4(E), 256, 0, st>>>(Min, emb, sp_nbr, XF, rev, Mout, E);
    return PET_OK;
}

template <int K>
static int head_tile(const float* Xin, const Lin& w0, const Lin& w2, const float* wl, float bl, const float* fc, float* ypred,
                     float* yout, int64_t R, float* hidden, int ldh, hipStream_t st) {
    return launch_tile(k_head<K>, R, tile_bytes(K) + T128 + BM * 8, st, Xin, wx_fwd(w0), w0.b, wx_fwd(w2), w2.b, wl, bl, fc, ypred,
                       yout, R, hidden, ldh);
}
int tile_head(bool edge, const float* Xin, const Lin& w0, const Lin& w2, const float* wl, float bl, const float* fc, float* ypred,
              float* yout, int64_t R, float* hidden, int ldh, hipStream_t st) {
    return edge ? head_tile<128>(Xin, w0, w2, wl, bl, fc, ypred, yout, R, hidden, ldh, st)
                : head_tile<256>(Xin, w0, w2, wl, bl, fc, ypred, yout, R, hidden, ldh, st);
}

// ---- adjoints
template <int K, bool EDGE>
static int head_bwd_tile(const float* Xin, const Lin& w0, const Lin& w2, const float* wl, const float* gA, const int* ctr,
                         const float* fc, const float* ypred, float* dfc, float* dXout, int64_t R, float* t_s1, float* t_da2,
                         float* t_da1, float* t_s2y, const float* Gd, const float* gb, hipStream_t st) {
    const bool train = t_s1 != nullptr, gen = Gd != nullptr;
    const size_t lds = tile_bytes(K) + T128 + 768 + (gen ? BM * 4 : 0);  // A | S | gy, row scales (| the rows' atoms)
    auto go = [&](auto kern) {
        return launch_tile(kern, R, lds, st, Xin, wx_fwd(w0), w0.b, wx_fwd(w2), w2.b, wx_b(w0), wx_b(w2), wl, gA, ctr, fc, ypred, dfc,
                           dXout, R, t_s1, t_da2, t_da1, t_s2y, Gd, gb);
    };
    if (gen) return train ? go(k_head_bwd<K, EDGE, true, true>) : go(k_head_bwd<K, EDGE, false, true>);
    return train ? go(k_head_bwd<K, EDGE, true, false>) : go(k_head_bwd<K, EDGE, false, false>);
}
int tile_head_bwd(bool edge, const float* Xin, const Lin& w0, const Lin& w2, const float* wl, const float* gA, const int* ctr,
                  const float* fc, const float* ypred, float* dfc, float* dXout, int64_t R, float* t_s1, float* t_da2, float* t_da1,
                  float* t_s2y, const float* Gd, const float* gb, hipStream_t st) {
    return edge ? head_bwd_tile<128, true>(Xin, w0, w2, wl, gA, ctr, fc, ypred, dfc, dXout, R, t_s1, t_da2, t_da1, t_s2y, Gd, gb, st)
                : head_bwd_tile<256, false>(Xin, w0, w2, wl, gA, ctr, fc, ypred, dfc, dXout, R, t_s1, t_da2, t_da1, t_s2y, Gd, gb, st);
}

int tile_dxf(const float* dM, const float* dcat, const int* rev, float* dX, int64_t E, hipStream_t st) {
    k_dxf<<<grid4(E), 256, 0, st>>>(dM, dcat, rev, dX, E);
    return PET_OK;
}

// the SwiGLU adjoint of edge rows (K = 128, hidden DFF) and of node rows (K = 256, hidden DNF); norm = false: the PostLN form, which
// only edge-width rows have (no node-row instantiation of it exists)
template <int K, int HID>
static int swiglu_bwd_tile(bool norm, const float* dY, const float* Xin, const float* VG, const float* gamma, bool ln, const Lin& win,
                           const Lin& wout, float* dX, int64_t rows, float* t_dvg, hipStream_t st) {
    const size_t lds = tile_bytes(K) + T128;  // dY tile | dv / dg chunk
    if constexpr (K == 128) {
        if (!norm) return launch_tile(k_swiglu_bwd<K, HID, false, false>, rows, lds, st, dY, Xin, VG, gamma, wout.bwd, win.bwd, dX, rows, nullptr, ln);
    }
    if (t_dvg) return launch_tile(k_swiglu_bwd<K, HID, true, true>, rows, lds, st, dY, Xin, VG, gamma, wout.bwd, win.bwd, dX, rows, t_dvg, ln);
    return launch_tile(k_swiglu_bwd<K, HID, false, true>, rows, lds, st, dY, Xin, VG, gamma, wout.bwd, win.bwd, dX, rows, t_dvg, ln);
}
int tile_emlp_bwd(bool norm, const float* dY, const float* X1, const float* VG, const float* gamma, bool layer_norm, const Lin& win,
                  const Lin& wout, float* dX1, int64_t rows, float* t_dvg, hipStream_t st) {
    return swiglu_bwd_tile<128, DFF>(norm, dY, X1, VG, gamma, layer_norm, win, wout, dX1, rows, t_dvg, st);
}
int tile_node_bwd(const AttnLayerW& A, const float* dHn, const float* H1, const float* VGn, float* dH1, int64_t N, bool layer_norm,
                  float* t_dvg, hipStream_t st) {
    return swiglu_bwd_tile<256, DNF>(true, dHn, H1, VGn, A.g_center, layer_norm, A.cmlp_in, A.cmlp_out, dH1, N, t_dvg, st);
}

int tile_expand_bwd(const Lin& ce, const float* dH1, float* dOC, int64_t N, hipStream_t st) {
    return launch_tile(k_expand_bwd, N, T256, st, dH1, ce.bwd, dOC, N);
}

int tile_center_bwd(bool deep, const Lin& cc, const float* dC, const float* dH1, float* dHin, int64_t N, hipStream_t st) {
    if (deep) return launch_tile(k_center_bwd<true>, N, T128, st, dC, dH1, cc.bwd, dHin, N);
    return launch_tile(k_center_bwd<false>, N, T128, st, dC, dH1, cc.bwd, dHin, N);
}

int tile_oproj_bwd(const float* dX1, const float* dOC, const Lin& out, float* dAO, int64_t E, int64_t R, hipStream_t st) {
    return launch_tile(k_oproj_bwd, R, T128, st, dX1, dOC, out.bwd, dAO, E, R);
}

int tile_qkv_bwd(bool post, const float* dQKV, const float* X, const float* gamma, bool layer_norm, const Lin& qkv, const float* dX1,
                 float* dXin, int64_t E, int64_t R, hipStream_t st) {
    if (post) return launch_tile(k_qkv_bwd<true>, R, T128, st, dQKV, nullptr, nullptr, qkv.bwd, dX1, dXin, E, R, false);
    return launch_tile(k_qkv_bwd<false>, R, T128, st, dQKV, X, gamma, qkv.bwd, dX1, dXin, E, R, layer_norm);
}

int tile_rownorm_bwd(const float* dYe, const float* dYc, const float* S, const float* gamma, bool layer_norm, float* dS, int64_t E,
                     int64_t R, hipStream_t st) {
    return launch_tile(k_rownorm_bwd, R, T128, st, dYe, dYc, S, gamma, layer_norm, dS, E, R);
}

int tile_resmix_bwd(const float* ge, const float* dMout, const int* rev, float* de, float* dMin, int64_t E, hipStream_t st) {
    k_resmix_bwd<<<grid4(E), 256, 0, st>>>(ge, dMout, rev, de, dMin, E);
    return PET_OK;
}

int tile_compress_bwd(bool first, const float* dXe, const float* a0, const GnnLayerW& G, float* dgeo, float* dM, int64_t E,
                      float* t_da0, hipStream_t st) {
    auto go = [&](auto kern) {
        return launch_tile(kern, E, T128, st, dXe, a0, G.compress2.bwd, G.wct, first ? nullptr : G.compress0_msg.bwd, dgeo,
                           first ? nullptr : dM, E, t_da0);
    };
    if (first) return t_da0 ? go(k_compress_bwd<true, true>) : go(k_compress_bwd<true, false>);
    return t_da0 ? go(k_compress_bwd<false, true>) : go(k_compress_bwd<false, false>);
}

}  // namespace pet
