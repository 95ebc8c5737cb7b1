// The three node-row Linear layers around the attention block of large graphs on the row ring (rows_s.h):
//   k_center       X[E + i] = H[i] Wcc^T + b            (DN -> D;  transformer.py:211-214, centre contraction)
//   k_expand_bwd   dOC = dH1 Wce                        (DN -> D;  adjoint of the centre expansion, transformer.py:222)
//   k_center_bwd   dHin = dH1 + dC Wcc                  (D -> DN;  adjoint of the contraction)
// The LDS-tile kernels they replace (pet_fwd.hip / pet_bwd.hip; they keep serving small graphs and the training passes) run 64-row
// workgroups whose waves each stream their own weight blocks from L2, two in flight: 63 / 76 / 83 us per launch at 80 000 atoms for
// 25 us worth of HBM traffic, four launches of each per step on a node chain that the edge kernels do not overlap.
// Here a 256-wide row arrives as two 128-column halves through the wave's 16-KB tile; every row is scaled by its power of two
// first (node features and adjoints are un-normalised). Round 5.
#include "rows_s.h"

namespace pet {

// Y[N, NOUT] = X[N, KIN] W^T (+ bias) (+ addend rows), W as planes of 64 w in fragment order [tile][K block]
template <int KIN, int NOUT, bool ADD>
__global__ __launch_bounds__(256, 2) void k_rowlin_s(const float* __restrict__ X, W2 w, const float* __restrict__ bias,
                                                    const float* __restrict__ addend, float* __restrict__ Y, int64_t N) {
    constexpr int KB = KIN / 16, NT = NOUT / 32, NST = (NT / 2) * KB;
    RING_WAVE(N);
    auto req = [&](int g) {  // stage g: tile pair g / KB, K block g % KB; wave w brings tile 2 tp + (w >> 1), plane w & 1
        g = ring_clamp(g, NST);
        const unsigned dst = RING_SLOT_DST(ring_u, wave, g);
        const int tp = g / KB, kb = g % KB;
        ab_dma_piece((wave & 1) ? w.l : w.h, (2 * tp + (wave >> 1)) * KB + kb, lane16, dst);
    };
    // the rows: 128 columns at a time through the tile; the power-of-two scale is the whole row's
    float4 x[KIN / 8];
    {
        float4 xa[16];
        dma_tile128(X, row0, N, tile_u, L, KIN);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tile128_to_frag(xa, tile, L);
#pragma unroll
        for (int k = 0; k < 16; k++) x[k] = xa[k];
        if (KIN == 256) {
            // the reads must have RETURNED before the tile is requested again (an L2-warm LDS-DMA lands after 250-400 cycles, sooner
            // than sixteen queued ds_read_b128 of a busy CU are served; the copies above are no instructions, so nothing else waits)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            dma_tile128(X + 128, row0, N, tile_u, L, KIN);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            tile128_to_frag(xa, tile, L);
#pragma unroll
            for (int k = 0; k < 16; k++) x[(KIN == 256 ? 16 : 0) + k] = xa[k];
        }
    }
    req(0);
    req(1);
    req(2);
    float inv;
    f16x8 xh[KB], xl[KB];
    {
        float sc;
        inv = row_scale_pow2<KIN / 8>(x, sc);
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
            const float v8[8] = {x[2 * kb].x * ABS, x[2 * kb].y * ABS, x[2 * kb].z * ABS, x[2 * kb].w * ABS,
                                 x[2 * kb + 1].x * ABS, x[2 * kb + 1].y * ABS, x[2 * kb + 1].z * ABS, x[2 * kb + 1].w * ABS};
            ab_split8(v8, xh[kb], xl[kb]);
        }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = ab_zero();
    hs_gemm_r(acc, xh, xl, 0, req, ring, lane16);
    // ---- after the last stage: whole lines through the wave's tile, 128 columns at a time
    const float f = inv * ABQ_INV;
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int hf = 0; hf < NOUT / 128; hf++) {
        float4 y[16];
        hs_acc_rows<4>(y, acc + 4 * hf, f, bias, 128 * hf, L.h);
        auto out = [&](int r) { return live && row0 + r < N ? Y + (row0 + r) * NOUT + 128 * hf : nullptr; };
        if (ADD) {
            float4 old[16];
            request_rows_addend<16>(old, L, [&](int r) { return addend + (row0 + r < N ? row0 + r : N - 1) * NOUT + 128 * hf; });
            store_rows_lines_add<16>(y, old, reinterpret_cast<float*>(tile), L, out);
        } else {
            store_rows_lines<16>(y, reinterpret_cast<float*>(tile), L, out);
        }
    }
}

int center_s(const Lin& cc, const float* H, float* Xc, int64_t N, hipStream_t st) {  // X[E + i] = H[i] Wcc^T + b
    PET_REQUIRE_PLANES(cc.fwd2s, "centre contraction");
    launch_ring(k_rowlin_s<DN, D, false>, N, st, H, w2_planes(cc.fwd2s, D / 32, DN / 16), cc.b, nullptr, Xc, N);
    return PET_OK;
}
int expand_bwd_s(const Lin& ce, const float* dH1, float* dOC, int64_t N, hipStream_t st) {  // dOC = dH1 Wce
    PET_REQUIRE_PLANES(ce.bwd2s, "centre expansion adjoint");
    launch_ring(k_rowlin_s<DN, D, false>, N, st, dH1, w2_planes(ce.bwd2s, D / 32, DN / 16), nullptr, nullptr, dOC, N);
    return PET_OK;
}
int center_bwd_s(const Lin& cc, const float* dC, const float* dH1, float* dHin, int64_t N, hipStream_t st) {  // dHin = dH1 + dC Wcc
    PET_REQUIRE_PLANES(cc.bwd2s, "centre contraction adjoint");
    launch_ring(k_rowlin_s<D, DN, true>, N, st, dC, w2_planes(cc.bwd2s, DN / 32, D / 16), nullptr, dH1, dHin, N);
    return PET_OK;
}

}  // namespace pet
