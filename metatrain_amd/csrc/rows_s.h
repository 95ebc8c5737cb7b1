// The row ring: the one statement of the protocol of the row kernels that run as two desynchronised four-wave workgroups per
// CU and share ONE stream of weight fragments per workgroup ("the row ring's contract"). Included by
//   pet_emlp_s.hip (edge MLP, adjoint)   pet_head_s.hip (edge head, adjoint)   pet_compress_s.hip (compress adjoint)
//   pet_center_s.hip (node-row Linears)  pet_comb_s.hip / pet_comb_bwd_s.hip (combination stage, adjoint)
//   so_rows_s.hip (the row GEMMs of the second-order pass and of the ring node chain)
// Each of them keeps what is its own: which fragment stage g of its stream brings, its rows, its arithmetic, its epilogue,
// and the reason for every vmcnt count it passes to ring_stage_sync.
//
// LDS of a workgroup (RING_LDS_BYTES = 80 KB): four 16-KB row tiles, one per wave, then the ring of RING_NSLOT = 4 slots of
// RING_SLOT = 4 KB. A stage of the stream is four 1-KB fragments, one brought by each wave (LDS-DMA, ab_dma_piece) and all four
// read by every wave: two tiles x (h, l) of one-accumulator split-operand products (ablk.h), six MFMAs per wave and stage.
// Stage g lives in slot g mod 4 and is requested three stages ahead (k_emlp_s reads one stage ahead and requests four ahead:
// ablk.h ring_turn; the counts are the same). Past the end of its stream a wave requests the last stage again: identical bytes,
// and the count of requests in flight stays what the waits assume.
// THE INVARIANT: nothing but ring requests in the vmcnt queue between a tile's first and last stage, because vmcnt retires in
// order -- whatever else a wave sends to memory there (stores, row requests, scratch) is waited for with the fragment behind
// it. The kernels that do send something say how many operations, and pass that count to the sync.
#pragma once
#include "ablk.h"

namespace pet {

constexpr int RING_NW = 4;  // waves per workgroup (ablk.h: RING_SLOT, RING_NSLOT)
constexpr size_t RING_LDS_BYTES = RING_NW * 16384 + RING_NSLOT * RING_SLOT;

// What every ring kernel knows about its wave, as the first statement of the kernel (R: its row count): 32 rows from row0 (row:
// this lane's, clamped to the last one; valid: it exists and is this wave's to store), its 16-KB tile, the ring -- generic
// pointers for reads, the wave-uniform 32-bit LDS addresses for LDS-DMA destinations.
// THE DEAD-WAVE RULE: a wave whose tile lies past the last row runs along on the last tile -- same requests, same barriers, so
// the workgroup's stream and its vmcnt counts do not depend on the row count -- and stores nothing (live == false).
// (A macro, not a struct with a constructor: as members of a struct passed to the request functions the same values cost
// k_head_s and k_head_bwd_s three registers and moved the ring's LDS reads.)
#define RING_WAVE(R)                                                                              \
    extern __shared__ __attribute__((aligned(16))) char ring_smem[];                             \
    const RowLane L;                                                                              \
    const unsigned lane16 = (unsigned)L.lane * 16u;                                               \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                            \
    int64_t row0 = ((int64_t)blockIdx.x * RING_NW + wave) * WROWS;                                \
    const bool live = row0 < (R);                                                                 \
    if (!live) row0 = (((R) - 1) / WROWS) * WROWS;                                                \
    [[maybe_unused]] const int64_t row = row0 + L.r < (R) ? row0 + L.r : (R) - 1;                 \
    [[maybe_unused]] const bool valid = live && row0 + L.r < (R);                                 \
    char* tile = ring_smem + wave * 16384;                                                        \
    const char* ring = ring_smem + RING_NW * 16384;                                               \
    const unsigned tile_u = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)tile);            \
    const unsigned ring_u = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)ring)
// stage g lives in slot g mod 4: where wave `wave` requests its fragment to, and where a lane reads fragment 0 (fragment i at + 1024 i)
// (macros: as functions returning the address they moved the register allocation of k_comb_bwd_s and k_rowlin_s)
#define RING_SLOT_DST(ring_u, wave, g) ((ring_u) + (unsigned)((g) & (RING_NSLOT - 1)) * RING_SLOT + (wave) * 1024)
#define RING_SLOT_PTR(ring, g, lane16) ((ring) + ((g) & (RING_NSLOT - 1)) * RING_SLOT + (lane16))
// past the end of a stream of n stages: the last stage again (identical bytes; keeps vmcnt uniform)
__device__ __forceinline__ int ring_clamp(int g, int n) { return g < n ? g : n - 1; }
// the same for a stream of NC chunks of SPC stages, stage (hc, s) with s < 2 SPC (s past the chunk: the next chunk's stage)
template <int SPC, int NC>
__device__ __forceinline__ void ring_clamp_chunk(int& hc, int& s) {
    if (s >= SPC) { s -= SPC; hc += 1; }
    if (hc >= NC) { hc = NC - 1; s = SPC - 1; }
}

// The sync in front of a stage: this wave's fragment of the stage has landed -- everything but its fragments of the two stages
// requested after it, vmcnt(2) -- and its own LDS reads have returned, then the workgroup barrier: the stage is complete for
// everybody, and everybody is done with the stage before it (whose slot is requested next).
//   extra_in_flight   EXTRA vector-memory operations of this wave are younger than the fragment waited for and may stay in
//                     flight: vmcnt(2 + EXTRA)
//   drain             ... but not all EXTRA were issued (a partial tile skips store instructions): vmcnt(0)
// AB_ABL_NOBAR (timing ablation, results are wrong): no barrier.
template <int EXTRA = 0>
__device__ __forceinline__ void ring_stage_sync(bool extra_in_flight = false, bool drain = false) {
    if (extra_in_flight && drain) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else if (extra_in_flight) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 + EXTRA) : "memory");
    else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
#ifndef AB_ABL_NOBAR
    __syncthreads();
#endif
}

// a stage's six MFMAs: a0 += W[fragments 0, 1] . (x0h, x0l), a1 += W[fragments 2, 3] . (x1h, x1l)  (a0 and a1 may be one accumulator)
__device__ __forceinline__ void ring_stage_mfma(const char* slot, f32x16& a0, const f16x8& x0h, const f16x8& x0l, f32x16& a1,
                                                const f16x8& x1h, const f16x8& x1l) {
    const f16x8 w0h = *reinterpret_cast<const f16x8*>(slot);
    const f16x8 w0l = *reinterpret_cast<const f16x8*>(slot + 1024);
    AB_MFMA3(a0, w0h, w0l, x0h, x0l);
    const f16x8 w1h = *reinterpret_cast<const f16x8*>(slot + 2048);
    const f16x8 w1l = *reinterpret_cast<const f16x8*>(slot + 3072);
    AB_MFMA3(a1, w1h, w1l, x1h, x1l);
}

// a product of NT output tiles over KB K blocks: acc[t] += W[tile t] planes . x planes; stages g0 .. g0 + (NT / 2) KB - 1 of the
// stream (tile pair tp, K block kb: tiles 2 tp, 2 tp + 1 x (h, l)). req(g): this wave's request of stage g, clamped by the caller.
// lead (wave-uniform): LEAD vector-memory operations younger than the requests of the first three stages may stay in flight
// over those stages.
template <int LEAD = 0, int NT = 4, int KB = 8, class Req>
__device__ __forceinline__ void hs_gemm_r(f32x16 (&acc)[NT], const f16x8 (&xh)[KB], const f16x8 (&xl)[KB], int g0, Req req,
                                          const char* ring, unsigned lane16, bool lead = false) {
#pragma unroll
    for (int r = 0; r < (NT / 2) * KB; r++) {
        const int g = g0 + r, tp = r / KB, kb = r % KB;
        if (r < 3 && lead) ring_stage_sync<LEAD>(true);
        else ring_stage_sync();
        req(g + 3);
        ring_stage_mfma(RING_SLOT_PTR(ring, g, lane16), acc[2 * tp], xh[kb], xl[kb], acc[2 * tp + 1], xh[kb], xl[kb]);
    }
}
// planes of f x of a row fragment of KB K blocks (f = 64, times whatever scales the row)
template <int KB>
__device__ __forceinline__ void hs_planes(const float4 (&x)[2 * KB], f16x8 (&xh)[KB], f16x8 (&xl)[KB], float f = ABS) {
#pragma unroll
    for (int kb = 0; kb < KB; kb++) {
        const float v8[8] = {x[2 * kb].x * f, x[2 * kb].y * f, x[2 * kb].z * f, x[2 * kb].w * f,
                             x[2 * kb + 1].x * f, x[2 * kb + 1].y * f, x[2 * kb + 1].z * f, x[2 * kb + 1].w * f};
        ab_split8(v8, xh[kb], xl[kb]);
    }
}
// the value of a 128-vector at the feature of accumulator register 4 j + i of tile t, read through the SCALAR cache (wave-uniform
// addresses, both halves of the column group, selected by lane half: a vector load would queue behind the ring requests)
__device__ __forceinline__ float hs_vec(const float* __restrict__ v, int t, int j, int i, int h) {
    const float lo = v[32 * t + 8 * j + i], hi = v[32 * t + 8 * j + 4 + i];
    return h ? hi : lo;
}
// the same for a vector whose address changes inside a stage loop (v + 32 hc): the compiler makes VECTOR loads of those, which queue
// behind the ring requests and drain the ring when they are waited for; ablk.h ab_sload keeps them in the scalar cache
__device__ __forceinline__ float hs_vec_s(const float* __restrict__ v, int t, int j, int i, int h) {
    const float lo = ab_sload(v + 32 * t + 8 * j + i), hi = ab_sload(v + 32 * t + 8 * j + 4 + i);
    return h ? hi : lo;
}
// NT accumulator tiles times f (+ a bias vector from bias + off, hs_vec) as a row fragment: y[4 t + j] = columns 32 t + 8 j + 4 h .. + 3
template <int NT>
__device__ __forceinline__ void hs_acc_rows(float4 (&y)[4 * NT], const f32x16* acc, float f, const float* __restrict__ bias = nullptr,
                                            int off = 0, int h = 0) {
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x16& a = acc[t];
            y[4 * t + j] = make_float4(a[4 * j] * f, a[4 * j + 1] * f, a[4 * j + 2] * f, a[4 * j + 3] * f);
            if (bias) {
                y[4 * t + j].x += hs_vec(bias + off, t, j, 0, h); y[4 * t + j].y += hs_vec(bias + off, t, j, 1, h);
                y[4 * t + j].z += hs_vec(bias + off, t, j, 2, h); y[4 * t + j].w += hs_vec(bias + off, t, j, 3, h);
            }
        }
}

// whole rows of a [32 x 128] fp32 block (leading dimension ld) into a wave's tile: trr.h dma_tile128 with the addresses as one
// wave-uniform base (the block's first row) + a 32-bit lane offset. The 64-bit row addresses of trr.h's form, sixteen per call
// site, were kept across the stage loops in spilled registers -- scratch loads inside the ring's vmcnt window.
__device__ __forceinline__ void ring_dma_rows(const float* __restrict__ X, int64_t r0, int64_t R, int ld, unsigned lds_base,
                                              const RowLane& L) {
    const float* base = X + r0 * ld;
    const int rmax = (int)(R - 1 - r0 < 31 ? R - 1 - r0 : 31);  // rows past the end: the last one again
    const int hi = L.lane >> 5, c = L.lane & 31;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int r = 2 * j + hi, rr = r < rmax ? r : rmax;
        const unsigned off = ((unsigned)rr * (unsigned)ld + 4u * (unsigned)(c ^ (r & 15))) * 4u;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(off), "s"(base), "s"(lds_base + j * 1024) : "memory");
    }
}

// host side: the planes of a layer's packed matrix (fwd2s or bwd2s: the same number of fragments either way)
inline W2 lin_planes(const void* planes, const Lin& l) { return w2_planes(planes, l.n_out / 32, l.k_in / 16); }
// one workgroup of 256 threads per 128 rows, the ring's LDS
template <class... P, class... A>
inline void launch_ring(void (*kern)(P...), int64_t rows, hipStream_t st, A... args) {
    allow_big_lds(kern, RING_LDS_BYTES);
    kern<<<cdiv(rows, RING_NW * WROWS), 256, RING_LDS_BYTES, st>>>(static_cast<P>(args)...);
}

}  // namespace pet
