// What the LDS-tile unit (pet_tile.hip) and the node unit (pet_node.hip) share on top of tile.h: the row strides of their tiles, the
// operand forms of a Linear, the accumulator store and the norm adjoint on a tile.
#pragma once
#include "model.h"
#include "tile.h"

namespace pet {

constexpr int LD128 = lds_ld(128);
constexpr int LD256 = lds_ld(256);
constexpr size_t T128 = BM * LD128 * 4, T256 = BM * LD256 * 4;  // bytes of a [64][132] / [64][260] fp32 tile

// both operand forms of a Linear for the LDS-tile kernels (tile.h gemm_acc_x): fp16 planes when f16x3 is on and the weight was
// packed; fwd: x W^T, bwd: dy W
inline WX wx_fwd(const Lin& L) {
    WX w;
    w.f = L.fwd;
    if (L.fwd2) {
        const size_t n8 = (size_t)(L.n_out / 32) * (L.k_in / 16) * 64;
        w.h = reinterpret_cast<const f16x8_t*>(L.fwd2);
        w.l = w.h + n8;
    }
    return w;
}
inline WX wx_b(const Lin& L) {
    WX w;
    w.f = L.bwd;
    if (L.bwd2) {
        const size_t n8 = (size_t)(L.n_out / 32) * (L.k_in / 16) * 64;
        w.h = reinterpret_cast<const f16x8_t*>(L.bwd2);
        w.l = w.h + n8;
    }
    return w;
}

// store this wave's NT accumulator tiles to a row-major global array
template <int NT>
__device__ __forceinline__ void store_acc(f32x16 (&acc)[NT], float* __restrict__ G, int64_t row0,
                                          int64_t n_rows, int ld, int rb, int col0, int lane) {
    acc_foreach<NT>(acc, rb, col0, lane, [&](int r, int c, float v) {
        if (row0 + r < n_rows) G[(row0 + r) * ld + c] = v;
    });
}

__device__ __forceinline__ float sigmoid_grad_from(float s) { return s * (1.0f - s); }

// RMSNorm adjoint on a tile: W holds w = gamma * dn (LDS [64][K+4]); x rows come from
// global. dx = rstd * (w - xhat * mean(w * xhat)), xhat = x * rstd.
// calls f(row_in_tile, col, dx) for the 4-thread-per-row decomposition.
template <int K, int ROWS = BM, class F>
__device__ __forceinline__ void rmsnorm_bwd_rows(const float* Wt, const float* __restrict__ Xg, int64_t row0,
                                                 int64_t n_rows, int ldx, F f) {
    constexpr int LDW = lds_ld(K), TPR = NTHREADS / ROWS;
    const int r = threadIdx.x / TPR, q = threadIdx.x % TPR;
    const bool valid = row0 + r < n_rows;
    const float* xrow = Xg + (row0 + r) * ldx;
    float ss = 0.f, dot = 0.f;
    for (int c = q * 4; c < K; c += 4 * TPR) {
        float4 x = valid ? *reinterpret_cast<const float4*>(xrow + c) : make_float4(0, 0, 0, 0);
        float4 wv = *reinterpret_cast<const float4*>(Wt + r * LDW + c);
        ss += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
        dot += x.x * wv.x + x.y * wv.y + x.z * wv.z + x.w * wv.w;
    }
    ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); if (TPR == 8) ss += __shfl_xor(ss, 4);
    dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); if (TPR == 8) dot += __shfl_xor(dot, 4);
    const float rstd = rsqrtf(ss * (1.0f / K) + 1.1920928955078125e-07f);
    const float coef = dot * rstd * rstd * rstd * (1.0f / K);  // mean(w*xhat) * rstd / x-scale
    if (!valid) return;
    for (int c = q * 4; c < K; c += 4 * TPR) {
        float4 x = *reinterpret_cast<const float4*>(xrow + c);
        float4 wv = *reinterpret_cast<const float4*>(Wt + r * LDW + c);
        f(r, c, make_float4(rstd * wv.x - x.x * coef, rstd * wv.y - x.y * coef, rstd * wv.z - x.z * coef,
                            rstd * wv.w - x.w * coef));
    }
}

// The same with LayerNorm (ln): xhat = (x - mean) rstd, dx = rstd (w - mean(w) - xhat mean(w xhat)).
template <int K, int ROWS = BM, class F>
__device__ __forceinline__ void norm_bwd_rows(const float* Wt, const float* __restrict__ Xg, int64_t row0,
                                              int64_t n_rows, int ldx, bool ln, F f) {
    if (!ln) {
        rmsnorm_bwd_rows<K, ROWS>(Wt, Xg, row0, n_rows, ldx, f);
        return;
    }
    constexpr int LDW = lds_ld(K), TPR = NTHREADS / ROWS;
    const int r = threadIdx.x / TPR, q = threadIdx.x % TPR;
    const bool valid = row0 + r < n_rows;
    const float* xrow = Xg + (row0 + r) * ldx;
    float s = 0.f, sw = 0.f;
    for (int c = q * 4; c < K; c += 4 * TPR) {
        float4 x = valid ? *reinterpret_cast<const float4*>(xrow + c) : make_float4(0, 0, 0, 0);
        float4 wv = *reinterpret_cast<const float4*>(Wt + r * LDW + c);
        s += (x.x + x.y) + (x.z + x.w);
        sw += (wv.x + wv.y) + (wv.z + wv.w);
    }
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); if (TPR == 8) s += __shfl_xor(s, 4);
    sw += __shfl_xor(sw, 1); sw += __shfl_xor(sw, 2); if (TPR == 8) sw += __shfl_xor(sw, 4);
    const float mean = s * (1.0f / K), mw = sw * (1.0f / K);
    float ss = 0.f, dot = 0.f;
    for (int c = q * 4; c < K; c += 4 * TPR) {
        float4 x = valid ? *reinterpret_cast<const float4*>(xrow + c) : make_float4(0, 0, 0, 0);
        float4 wv = *reinterpret_cast<const float4*>(Wt + r * LDW + c);
        x.x -= mean; x.y -= mean; x.z -= mean; x.w -= mean;
        ss += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
        dot += x.x * wv.x + x.y * wv.y + x.z * wv.z + x.w * wv.w;
    }
    ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); if (TPR == 8) ss += __shfl_xor(ss, 4);
    dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); if (TPR == 8) dot += __shfl_xor(dot, 4);
    const float rstd = rsqrtf(ss * (1.0f / K) + 1e-5f);
    const float coef = dot * rstd * rstd * rstd * (1.0f / K);
    if (!valid) return;
    for (int c = q * 4; c < K; c += 4 * TPR) {
        float4 x = *reinterpret_cast<const float4*>(xrow + c);
        float4 wv = *reinterpret_cast<const float4*>(Wt + r * LDW + c);
        f(r, c, make_float4(rstd * (wv.x - mw) - (x.x - mean) * coef, rstd * (wv.y - mw) - (x.y - mean) * coef,
                            rstd * (wv.z - mw) - (x.z - mean) * coef, rstd * (wv.w - mw) - (x.w - mean) * coef));
    }
}

}  // namespace pet
