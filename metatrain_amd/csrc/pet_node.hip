// The node update of the tuned PET pass (transformer.py:222-227: center_expansion, center_mlp) and its adjoint as fused kernels,
// and the two entries (pet_stages.h node_fwd / node_bwd) that launch whichever form the plan chose (pet_plan.h Node); the ring
// form's three row GEMMs are in pet_node_s.hip, the LDS-tile adjoint (k_swiglu_bwd<256>) is in pet_tile.hip.
#include "pet_stages.h"
#include "pet_tile.h"

namespace pet {

// ---------------------------------------------------------------------------------
// node update: h1 = h + OC Wce^T + b ; h2 = h1 + SwiGLU_MLP(RMSNorm(h1))
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void k_node(const float* __restrict__ H, const float* __restrict__ OC,
                                                    WX wce, const float* __restrict__ bce,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, WX win,
                                                    const float* __restrict__ bin, WX wout,
                                                    const float* __restrict__ bout,
                                                    float* __restrict__ H1, float* __restrict__ VGn,
                                                    float* __restrict__ Hn, int64_t N) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Hs = smem;               // [64][260]
    float* U = smem + BM * LD256;   // [64][132] (OC tile, then SwiGLU hidden chunk)
    float* rs = U + BM * LD128;     // [64][2] row scales of the OC tile (un-normalised attention output)
    const WaveId w;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    load_rows_to_lds<128>(U, OC, row0, N, D);
    __syncthreads();
    if (wce.h) {
        tile_row_scales<128>(U, LD128, rs);
        __syncthreads();
    }
#pragma unroll 1
    for (int c = 0; c < 2; c++) {  // 256 output columns in two chunks of 128
        f32x16 acc[2];
        const int col0 = 128 * c + 64 * w.ch;
        acc_fill_bias<2>(acc, bce, col0, w.lane);
        gemm_acc_x<128, 2>(U + w.rb * 32 * LD128, LD128, wce, 16, 0, 4 * c + 2 * w.ch, acc, w.lane,
                           wce.h ? rs + 64 * w.rb : nullptr);
        acc_foreach<2>(acc, w.rb, col0, w.lane, [&](int r, int cc, float v) {
            const int64_t row = row0 + r;
            float h1 = v + (row < N ? H[row * DN + cc] : 0.f);
            Hs[r * LD256 + cc] = h1;
            if (row < N) H1[row * DN + cc] = h1;
        });
    }
    __syncthreads();
    norm_rows_inplace<256>(Hs, gamma, beta);
    __syncthreads();
    f32x16 out[4];  // this wave: 32 rows x 128 columns (128 * ch ..)
    acc_fill_bias<4>(out, bout, 128 * w.ch, w.lane);
#pragma unroll 1
    for (int hc = 0; hc < DNF / 128; hc++) {
        f32x16 av[2], ag[2];
        const int hcol0 = 128 * hc + 64 * w.ch;  // hidden columns of this wave
        acc_fill_bias<2>(av, bin, hcol0, w.lane);
        acc_fill_bias<2>(ag, bin, DNF + hcol0, w.lane);
        gemm_acc_x<256, 2>(Hs + w.rb * 32 * LD256, LD256, win, 32, 0, hcol0 / 32, av, w.lane);
        gemm_acc_x<256, 2>(Hs + w.rb * 32 * LD256, LD256, win, 32, 0, (DNF + hcol0) / 32, ag, w.lane);
        __syncthreads();  // previous chunk's readers of U are done
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = w.rb * 32 + acc_row(r, w.lane);
                const int cc = 64 * w.ch + 32 * t + (w.lane & 31);
                const float v = av[t][r], gte = ag[t][r];
                if (VGn && row0 + rr < N) {
                    VGn[(row0 + rr) * (2 * DNF) + 128 * hc + cc] = v;
                    VGn[(row0 + rr) * (2 * DNF) + DNF + 128 * hc + cc] = gte;
                }
                U[rr * LD128 + cc] = v * sigmoidf_(gte);  // transformer.py:42-43: value * sigmoid(gate)
            }
        }
        __syncthreads();
        gemm_acc_x<128, 4>(U + w.rb * 32 * LD128, LD128, wout, DNF / 8, 16 * hc, 4 * w.ch, out, w.lane);
    }
    acc_foreach<4>(out, w.rb, 128 * w.ch, w.lane, [&](int r, int c, float v) {
        const int64_t row = row0 + r;
        if (row < N) Hn[row * DN + c] = H1[row * DN + c] + v;
    });
}

// The same stage with the memory side rebuilt (k_node spends more than half of its time outside the GEMMs: one float
// per lane to and from global memory at one workgroup per CU): the H rows arrive as a coalesced tile, h1 leaves as one,
// the SwiGLU pre-activations and the result leave through wave-private staging tiles as float4 rows (tile.h
// wave_rows64); and the normalised rows are split ONCE into fp16 planes (gemm_acc_hs) for the 16 column-chunk GEMMs of
// the centre MLP's first Linear. LDS: [ h tile fp32 -> (SwiGLU chunk | 4 staging tiles) ][ OC tile -> planes ][ scales ].
// RB = 2: 64 rows per workgroup, waves = 2 row blocks x 2 column halves (1 workgroup per CU: 133 KB of LDS). RB = 1: 32 rows,
// the four waves own a quarter of the columns each and two workgroups share a CU (67 KB): half the dependent chain per
// wave and a second workgroup to fill its stalls -- the node chain sits on the critical path of a small box (one
// k_node2 per attention layer between the output projection and the next layer's centre tokens).
// SPLIT (RB = 1, graphs of at most 128 row tiles): the four 128-unit chunks of the hidden layer go to four workgroups
// (blockIdx.y) -- a workgroup of a small graph is alone on its CU and its time is the round trips of the 1.8 MB of weights it
// streams (bytes in flight / latency = 25 GB/s per CU), so four CUs per row tile stream a quarter each. Every workgroup
// forms h1 and its planes, runs its chunk and leaves a partial [32 x 256] output in Pp; the one that arrives last at the
// tile's counter (fence + atomic, the counter resets itself) adds bias and partials in chunk order -- the order of the
// unsplit accumulation, so the same bits whoever is last -- and finishes (Hn, the next layer's centre tokens).
template <int RB, bool SPLIT = false>
__global__ __launch_bounds__(NTHREADS) void k_node2(const float* __restrict__ H, const float* __restrict__ OC,
                                                     WX wce, const float* __restrict__ bce,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, WX win,
                                                     const float* __restrict__ bin, WX wout,
                                                     const float* __restrict__ bout,
                                                     float* __restrict__ H1, float* __restrict__ VGn,
                                                     float* __restrict__ Hn, int64_t N, WX wcn,
                                                     const float* __restrict__ bcn, float* __restrict__ Xcn,
                                                     float* __restrict__ Pp, int* __restrict__ cnt) {
    static_assert(!SPLIT || RB == 1, "the hidden-chunk split is built for the 32-row workgroups");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWS = 32 * RB, NCH = 4 / RB;      // rows per workgroup, column groups
    constexpr int WC = 256 / NCH, HC = 128 / NCH;    // output columns / hidden columns (per 128-chunk) of one wave
    constexpr int NTH = HC / 32, NTO = WC / 32;
    constexpr int XD = RB == 1 ? 8 : 2;  // weight blocks in flight in the products that split their A operand on the fly
    constexpr int LDH = plane_ld(256);
    float* Hs = smem;                                                  // [ROWS][260] h, then h1, then dead
    float* U = smem;                                                   // [ROWS][132] SwiGLU chunk (aliases Hs)
    float* stage = smem + ROWS * LD128;                                // 4 staging tiles (behind U, inside Hs)
    _Float16* Ph = reinterpret_cast<_Float16*>(smem + ROWS * LD256);   // [ROWS][264] high pieces of Norm(h1)
    _Float16* Pl = Ph + ROWS * LDH;                                    // [ROWS][264] low pieces
    float* OCs = smem + ROWS * LD256;                                  // [ROWS][132] OC tile (before the planes exist)
    float* rs = smem + ROWS * LD256 + ROWS * LDH;                      // [ROWS][2] row scales of the OC tile
    const WaveIdT<RB> w;
    float* my_stage = stage + w.wave * (RB == 2 ? 32 * 64 : 32 * 32);
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    load_rows_to_lds<128, ROWS>(OCs, OC, row0, N, D);
    load_rows_to_lds<256, ROWS>(Hs, H, row0, N, DN);
    __syncthreads();
    tile_row_scales<128, ROWS>(OCs, LD128, rs);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < RB; c++) {  // this wave's WC output columns in groups of 64
        f32x16 acc[2];
        const int col0 = 64 * (NCH * c + w.ch);
        acc_fill_bias<2>(acc, bce, col0, w.lane);
        gemm_acc_x<128, 2, XD>(OCs + w.rb * 32 * LD128, LD128, wce, 16, 0, col0 / 32, acc, w.lane, rs + 64 * w.rb);
        acc_foreach<2>(acc, w.rb, col0, w.lane, [&](int r, int cc, float v) { Hs[r * LD256 + cc] += v; });  // h1 = h + ...
    }
    __syncthreads();
    if constexpr (SPLIT) {  // (read again by whichever workgroup finishes the tile)
        if (blockIdx.y == 0) store_rows_from_lds_agent<256, ROWS>(Hs, H1, row0, N, DN);
    } else store_rows_from_lds<256, ROWS>(Hs, H1, row0, N, DN);
    __syncthreads();
    norm_rows_inplace<256, ROWS>(Hs, gamma, beta);
    __syncthreads();
    split_tile_planes<256, ROWS>(Hs, LD256, Ph, Pl);
    __syncthreads();  // Hs is dead from here on: U and the staging tiles reuse its memory
    f32x16 out[NTO];  // this wave: 32 rows x WC columns (WC * ch ..)
    acc_fill_bias<NTO>(out, SPLIT ? nullptr : bout, WC * w.ch, w.lane);
    const int64_t wrow0 = row0 + 32 * w.rb;  // first row of this wave's block
    const int hc_lo = SPLIT ? (int)blockIdx.y : 0, hc_hi = SPLIT ? (int)blockIdx.y + 1 : DNF / 128;
#pragma unroll 1
    for (int hc = hc_lo; hc < hc_hi; hc++) {
        f32x16 av[NTH], ag[NTH];
        const int hcol0 = 128 * hc + HC * w.ch;  // hidden columns of this wave
        acc_fill_bias<NTH>(av, bin, hcol0, w.lane);
        acc_fill_bias<NTH>(ag, bin, DNF + hcol0, w.lane);
        XRing<NTO, 8> ro;  // RB == 1: this chunk's K = 128 operand of the output product, requested before the hidden products
        const bool ring = RB == 1 && wout.h != nullptr;
        if (ring) xring_request(ro, wout, DNF / 8, 16 * hc, NTO * w.ch, w.lane);
        if constexpr (RB == 1) {  // value and gate tile in ONE product (one exposed round trip instead of two); same MFMA order per tile
            f32x16 vg[2] = {av[0], ag[0]};
            gemm_acc_hs<256, 2, 4>(Ph + w.rb * 32 * LDH, Pl + w.rb * 32 * LDH, LDH, win, 32, 0, hcol0 / 32, vg, w.lane, DNF / 32);
            av[0] = vg[0];
            ag[0] = vg[1];
        } else {
        gemm_acc_hs<256, NTH, 8>(Ph + w.rb * 32 * LDH, Pl + w.rb * 32 * LDH, LDH, win, 32, 0, hcol0 / 32, av, w.lane);
        gemm_acc_hs<256, NTH, 8>(Ph + w.rb * 32 * LDH, Pl + w.rb * 32 * LDH, LDH, win, 32, 0, (DNF + hcol0) / 32, ag, w.lane);
        }
        if (VGn) {  // saved for the adjoint: [value | gate] pre-activations, whole float4 rows
            if constexpr (RB == 2) {
                wave_rows64(av, my_stage, w.lane, [&](int r, int cc, float4 v) {
                    if (wrow0 + r < N) *reinterpret_cast<float4*>(VGn + (wrow0 + r) * (2 * DNF) + hcol0 + cc) = v;
                });
                wave_rows64(ag, my_stage, w.lane, [&](int r, int cc, float4 v) {
                    if (wrow0 + r < N) *reinterpret_cast<float4*>(VGn + (wrow0 + r) * (2 * DNF) + DNF + hcol0 + cc) = v;
                });
            } else {
                wave_rows32(av[0], my_stage, w.lane, [&](int r, int cc, float4 v) {
                    if (wrow0 + r < N) *reinterpret_cast<float4*>(VGn + (wrow0 + r) * (2 * DNF) + hcol0 + cc) = v;
                });
                wave_rows32(ag[0], my_stage, w.lane, [&](int r, int cc, float4 v) {
                    if (wrow0 + r < N) *reinterpret_cast<float4*>(VGn + (wrow0 + r) * (2 * DNF) + DNF + hcol0 + cc) = v;
                });
            }
        }
        __syncthreads();  // previous chunk's readers of U are done
#pragma unroll
        for (int t = 0; t < NTH; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)  // transformer.py:42-43: value * sigmoid(gate)
                U[(w.rb * 32 + acc_row(r, w.lane)) * LD128 + HC * w.ch + 32 * t + (w.lane & 31)] = av[t][r] * sigmoidf_(ag[t][r]);
        __syncthreads();
        if (ring) gemm_acc_x_ring<NTO, 8>(U + w.rb * 32 * LD128, LD128, ro, out, w.lane);
        else gemm_acc_x<128, NTO, XD>(U + w.rb * 32 * LD128, LD128, wout, DNF / 8, 16 * hc, NTO * w.ch, out, w.lane);
    }
    // Xcn: the NEXT attention layer's centre tokens = center_contraction(Hn) (transformer.py:211-214) from the Hn tile while
    // it is on chip (k_center's arithmetic: power-of-two row scales, the same GEMM) -- one launch and one stream hand-over
    // less per layer on the critical path of a small box
    float* Hn_s = smem + ROWS * LD256;  // [ROWS][260]: over the planes, which nobody reads after the last hidden chunk
    if constexpr (SPLIT) {
        __shared__ int last_arrival;
        const size_t prows = (size_t)gridDim.x * ROWS;  // rows of one partial (whole tiles)
#pragma unroll
        for (int t = 0; t < NTO; t++)
            wave_rows32(out[t], my_stage, w.lane, [&](int r, int cc, float4 v) {
                st4_agent(Pp + ((size_t)blockIdx.y * prows + (wrow0 + r)) * DN + WC * w.ch + 32 * t + cc, v);
            });
        // the partial (and h1) went out as device-coherent stores: once they are acknowledged (the workgroup-scope release
        // waits for that) the workgroup may be counted -- no L2 write-back fence, which costs 10+ us with a step's dirty lines
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        if (threadIdx.x == 0) {
            const int old = atomicAdd(&cnt[blockIdx.x], 1);
            last_arrival = old == (int)gridDim.y - 1;
            if (last_arrival) cnt[blockIdx.x] = 0;  // ready for the next launch on this stream
        }
        __syncthreads();
        if (!last_arrival) return;
        // Consumer side of the hand-over: an agent-scope ACQUIRE (buffer_inv, no write-back) orders the loads below after the
        // counter update this workgroup saw. Producer side: the partials are relaxed agent-scope atomic stores (write-through
        // to the device-coherent level) that the workgroup-scope release above has waited for (s_waitcnt vmcnt(0)); an
        // agent-scope RELEASE would add the L2 write-back of every dirty line of the step (10+ us) for
        // data that already went through. That part relies on gfx950's write-through behaviour of sc1 stores rather than on
        // the formal memory model; tests/test_gpu_stress.py (node_split_stress) runs the hand-over 200 x and demands
        // bit-identical results.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // every load of the reduction in flight before the first sum (8 positions x (4 partials + h1) per thread)
        constexpr int IT = ROWS * (DN / 4) / NTHREADS, NCHK = DNF / 128;
        float4 pk[IT][NCHK], h1v[IT];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int idx = threadIdx.x + it * NTHREADS, r = idx / (DN / 4), c = 4 * (idx % (DN / 4));
#pragma unroll
            for (int k = 0; k < NCHK; k++) pk[it][k] = ld4_agent(Pp + ((size_t)k * prows + row0 + r) * DN + c);
            h1v[it] = ld4_agent(H1 + (row0 + r < N ? row0 + r : N - 1) * DN + c);
        }
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int idx = threadIdx.x + it * NTHREADS, r = idx / (DN / 4), c = 4 * (idx % (DN / 4));
            float4 sum = *reinterpret_cast<const float4*>(bout + c);
#pragma unroll
            for (int k = 0; k < NCHK; k++)  // ((((b + chunk 0) + chunk 1) + chunk 2) + chunk 3): the unsplit order
                sum = make_float4(sum.x + pk[it][k].x, sum.y + pk[it][k].y, sum.z + pk[it][k].z, sum.w + pk[it][k].w);
            const int64_t row = row0 + r;
            float4 hn = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < N) {
                hn = make_float4(h1v[it].x + sum.x, h1v[it].y + sum.y, h1v[it].z + sum.z, h1v[it].w + sum.w);
                *reinterpret_cast<float4*>(Hn + row * DN + c) = hn;
            }
            if (Xcn) *reinterpret_cast<float4*>(Hn_s + r * LD256 + c) = hn;
        }
    } else {
    if (Xcn) __syncthreads();
    auto add_h1 = [&](int col) {  // Hn = h1 + MLP
        return [&, col](int r, int cc, float4 v) {
            const int64_t row = wrow0 + r;
            float4 hn = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < N) {
                const int64_t o = row * DN + col + cc;
                const float4 h1 = *reinterpret_cast<const float4*>(H1 + o);
                hn = make_float4(h1.x + v.x, h1.y + v.y, h1.z + v.z, h1.w + v.w);
                *reinterpret_cast<float4*>(Hn + o) = hn;
            }
            if (Xcn) *reinterpret_cast<float4*>(Hn_s + (w.rb * 32 + r) * LD256 + col + cc) = hn;
        };
    };
    if constexpr (RB == 2) {
#pragma unroll
        for (int half = 0; half < 2; half++) {  // this wave's 128 columns in two groups of 64
            const f32x16 pair[2] = {out[2 * half], out[2 * half + 1]};
            wave_rows64(pair, my_stage, w.lane, add_h1(WC * w.ch + 64 * half));
        }
    } else {
#pragma unroll
        for (int t = 0; t < NTO; t++) wave_rows32(out[t], my_stage, w.lane, add_h1(WC * w.ch + 32 * t));
    }
    }
    if (Xcn) {
        constexpr int NTC = RB;  // 128 centre-token columns over the NCH column groups
        __syncthreads();
        tile_row_scales<256, ROWS>(Hn_s, LD256, rs);
        __syncthreads();
        f32x16 cacc[NTC];
        acc_fill_bias<NTC>(cacc, bcn, 32 * NTC * w.ch, w.lane);
        gemm_acc_x<256, NTC, XD>(Hn_s + w.rb * 32 * LD256, LD256, wcn, 32, 0, NTC * w.ch, cacc, w.lane, rs + 64 * w.rb);
        store_acc<NTC>(cacc, Xcn, row0, N, D, w.rb, 32 * NTC * w.ch, w.lane);
    }
}

// k_node2w: the 64-row node update of large graphs with every weight block requested ONCE per workgroup. k_node2<2> runs
// (row block, column half) waves, so two waves stream the same weights (phase timings at 80 000 atoms, us per launch: tile
// loads 60, expansion + norm + planes 73, hidden products 234 for 50 us of MFMA work, U exchange + output product 167,
// epilogue 57). Here a wave owns a column quarter for BOTH 32-row blocks (tile.h gemm_acc_hs_rb2 / gemm_acc_x_ring_rb2): the
// value and gate tiles of a hidden chunk in one product, the K = 128 operand of the output product requested behind the
// barriers. 0.52 -> 0.455 ms per launch: the rest is the exposed latency of each phase at one workgroup per CU (133 KB of
// LDS). Same LDS layout and the same MFMA order per output element as k_node2<2> (the A/B kernel of rounds 3 - 5; its forward instantiation is no longer launched).
__global__ __launch_bounds__(NTHREADS) void k_node2w(const float* __restrict__ H, const float* __restrict__ OC,
                                                      WX wce, const float* __restrict__ bce,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, WX win,
                                                      const float* __restrict__ bin, WX wout,
                                                      const float* __restrict__ bout,
                                                      float* __restrict__ H1, float* __restrict__ VGn,
                                                      float* __restrict__ Hn, int64_t N, WX wcn,
                                                      const float* __restrict__ bcn, float* __restrict__ Xcn) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWS = 64, LDH = plane_ld(256);
    float* Hs = smem;                                                  // [64][260] h, then h1, then dead
    float* U = smem;                                                   // [64][132] SwiGLU chunk (aliases Hs)
    float* stage = smem + ROWS * LD128;                                // 4 staging tiles [32][32] (behind U, inside Hs)
    _Float16* Ph = reinterpret_cast<_Float16*>(smem + ROWS * LD256);   // [64][264] high pieces of Norm(h1)
    _Float16* Pl = Ph + ROWS * LDH;
    float* OCs = smem + ROWS * LD256;                                  // [64][132] OC tile (before the planes exist)
    float* rs = smem + ROWS * LD256 + ROWS * LDH;                      // [64][2] row scales
    const int lane = threadIdx.x & 63, ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // column quarter
    float* my_stage = stage + ch * (32 * 32);
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    load_rows_to_lds<128, ROWS>(OCs, OC, row0, N, D);
    load_rows_to_lds<256, ROWS>(Hs, H, row0, N, DN);
    __syncthreads();
    tile_row_scales<128, ROWS>(OCs, LD128, rs);
    __syncthreads();
    {   // h1 = h + center_expansion(OC): this wave's 64 columns, both row blocks
        XRing<2, 8> rc;
        xring_request(rc, wce, 16, 0, 2 * ch, lane);
        f32x16 acc[4];
        f32x16 b2[2];
        acc_fill_bias<2>(b2, bce, 64 * ch, lane);
        acc[0] = acc[2] = b2[0];
        acc[1] = acc[3] = b2[1];
        gemm_acc_x_ring_rb2<2, 8>(OCs, LD128, rc, acc, lane, 32 * LD128, rs);
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    Hs[(rb * 32 + acc_row(r, lane)) * LD256 + 64 * ch + 32 * t + (lane & 31)] += acc[rb * 2 + t][r];
    }
    __syncthreads();
    store_rows_from_lds<256, ROWS>(Hs, H1, row0, N, DN);
    __syncthreads();
    norm_rows_inplace<256, ROWS>(Hs, gamma, beta);
    __syncthreads();
    split_tile_planes<256, ROWS>(Hs, LD256, Ph, Pl);
    __syncthreads();  // Hs is dead from here on: U and the staging tiles reuse its memory
    f32x16 out[4];  // [row block][2 tiles]: 64 rows x this wave's 64 columns
    {
        f32x16 b2[2];
        acc_fill_bias<2>(b2, bout, 64 * ch, lane);
        out[0] = out[2] = b2[0];
        out[1] = out[3] = b2[1];
    }
#pragma unroll 1
    for (int hc = 0; hc < DNF / 128; hc++) {
        const int hcol0 = 128 * hc + 32 * ch;  // this wave's 32 hidden units of the chunk
        f32x16 vg[4];  // [row block][value, gate]
        {
            f32x16 bv[1], bg[1];
            acc_fill_bias<1>(bv, bin, hcol0, lane);
            acc_fill_bias<1>(bg, bin, DNF + hcol0, lane);
            vg[0] = vg[2] = bv[0];
            vg[1] = vg[3] = bg[0];
        }
        gemm_acc_hs_rb2<256, 2, 4>(Ph, Pl, LDH, win, 32, 0, hcol0 / 32, vg, lane, DNF / 32, 32 * LDH);
        if (VGn) {  // saved for the adjoint: [value | gate] pre-activations, whole float4 rows
#pragma unroll
            for (int rb = 0; rb < 2; rb++)
#pragma unroll
                for (int q = 0; q < 2; q++)
                    wave_rows32(vg[rb * 2 + q], my_stage, lane, [&](int r, int cc, float4 v) {
                        const int64_t row = row0 + 32 * rb + r;
                        if (row < N) *reinterpret_cast<float4*>(VGn + row * (2 * DNF) + q * DNF + hcol0 + cc) = v;
                    });
        }
        XRing<2, 8> ro;  // the K = 128 operand of the output product: requested here, it arrives behind the barriers
        xring_request(ro, wout, DNF / 8, 16 * hc, 2 * ch, lane);
        __syncthreads();  // previous chunk's readers of U are done
#pragma unroll
        for (int rb = 0; rb < 2; rb++)
#pragma unroll
            for (int r = 0; r < 16; r++)  // transformer.py:42-43: value * sigmoid(gate)
                U[(rb * 32 + acc_row(r, lane)) * LD128 + 32 * ch + (lane & 31)] = vg[rb * 2][r] * sigmoidf_(vg[rb * 2 + 1][r]);
        __syncthreads();
        gemm_acc_x_ring_rb2<2, 8>(U, LD128, ro, out, lane, 32 * LD128);
    }
    float* Hn_s = smem + ROWS * LD256;  // [64][260]: over the planes, which nobody reads after the last hidden chunk
    if (Xcn) __syncthreads();
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int t = 0; t < 2; t++)
            wave_rows32(out[rb * 2 + t], my_stage, lane, [&](int r, int cc, float4 v) {  // Hn = h1 + MLP
                const int64_t row = row0 + 32 * rb + r;
                const int col = 64 * ch + 32 * t;
                float4 hn = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < N) {
                    const int64_t o = row * DN + col + cc;
                    const float4 h1 = *reinterpret_cast<const float4*>(H1 + o);
                    hn = make_float4(h1.x + v.x, h1.y + v.y, h1.z + v.z, h1.w + v.w);
                    *reinterpret_cast<float4*>(Hn + o) = hn;
                }
                if (Xcn) *reinterpret_cast<float4*>(Hn_s + (rb * 32 + r) * LD256 + col + cc) = hn;
            });
    if (Xcn) {  // the next attention layer's centre tokens (k_node2): this wave's 32 of the 128 columns, both row blocks
        __syncthreads();
        tile_row_scales<256, ROWS>(Hn_s, LD256, rs);
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 2; rb++) {
            f32x16 cacc[1];
            acc_fill_bias<1>(cacc, bcn, 32 * ch, lane);
            gemm_acc_x<256, 1, 8>(Hn_s + rb * 32 * LD256, LD256, wcn, 32, 0, ch, cacc, lane, rs + 64 * rb);
            store_acc<1>(cacc, Xcn, row0, N, D, rb, 32 * ch, lane);
        }
    }
}

// The node-row instance (K = 256, hidden 512) rebuilt like k_node2 (above): the dY tile is scaled per row by a
// power of two (adjoint rows have any magnitude) and split ONCE into fp16 planes for the four du chunk GEMMs, all products
// on the 16-bit matrix cores (the fp32-MFMA form above spends 46 % of its time in the matrix pipe: 64 cycles per 2 k),
// everything between the two scalings stays in scaled units; the saved pre-activations arrive as float4 rows through
// wave-private staging tiles. Inference only (no weight-gradient exports).
// SPLIT (RB = 1): the hidden chunks of a row tile on four workgroups as in k_node2 -- partial dn tiles through Pp (device-
// coherent stores / loads), the workgroup that arrives last at the tile's counter sums them in chunk order (deterministic;
// not the bits of the unsplit accumulation, whose chunks interleave their two products) and runs the epilogue.
template <int RB, bool SPLIT = false>  // 32 RB rows per workgroup (see k_node2)
__global__ __launch_bounds__(NTHREADS) void k_node_bwd2(const float* __restrict__ dY, const float* __restrict__ Xin,
                                                         const float* __restrict__ VG, const float* __restrict__ gamma,
                                                         WX woutb, WX winb, float* __restrict__ dXout, int64_t R, bool ln,
                                                         const float4* __restrict__ wceb, float* __restrict__ dOC,
                                                         float* __restrict__ Pp, int* __restrict__ cnt) {
    static_assert(!SPLIT || RB == 1, "the hidden-chunk split is built for the 32-row workgroups");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int K = 256, HID = DNF, LDK = lds_ld(K), LDH = plane_ld(K);
    constexpr int ROWS = 32 * RB, NCH = 4 / RB, WC = 256 / NCH, HC = 128 / NCH, NTH = HC / 32, NTO = WC / 32;
    constexpr int XD = RB == 1 ? 8 : 2;  // weight blocks in flight (tile.h gemm_acc_x)
    float* A = smem;                                                 // [ROWS][260] dY tile; at the end w = gamma * dn
    float* U = smem;                                                 // [ROWS][132] dv / dg chunk (aliases A while A is dead)
    float* stage = smem + ROWS * LD128;                              // 4 staging tiles (behind U, inside A)
    _Float16* Ph = reinterpret_cast<_Float16*>(smem + ROWS * LDK);   // [ROWS][264] planes of the scaled dY rows
    _Float16* Pl = Ph + ROWS * LDH;
    float* rs = smem + ROWS * LDK + ROWS * LDH;                      // [ROWS][2] scale, inverse
    const WaveIdT<RB> w;
    constexpr int SW = RB == 2 ? 64 : 32;                            // staging tile width
    float* my_stage = stage + w.wave * (32 * SW);
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int64_t wrow0 = row0 + 32 * w.rb;
    load_rows_to_lds<K, ROWS>(A, dY, row0, R, K);
    __syncthreads();
    tile_row_scales<K, ROWS>(A, LDK, rs);
    __syncthreads();
    split_tile_planes_scaled<K, ROWS>(A, LDK, rs, Ph, Pl);
    __syncthreads();  // A is dead until the epilogue
    f32x16 dn[NTO];
    acc_fill_bias<NTO>(dn, nullptr, 0, w.lane);
    const int hc_lo = SPLIT ? (int)blockIdx.y : 0, hc_hi = SPLIT ? (int)blockIdx.y + 1 : HID / 128;
#pragma unroll 1
    for (int hc = hc_lo; hc < hc_hi; hc++) {
        f32x16 du[NTH];
        acc_fill_bias<NTH>(du, nullptr, 0, w.lane);
        const int hcol0 = 128 * hc + HC * w.ch;
        // RB == 1 (small graphs, one wave per SIMD, every product starts with an exposed round trip): the K = 128 operands of
        // this chunk's two dn products and its saved [v | g] rows are requested around the du product instead of after it
        XRing<NTO, 8> r1, r2;
        const bool ring = RB == 1 && winb.h != nullptr;
        float4 vpre[4], gpre[4];
        if constexpr (RB == 1) {
            if (ring) xring_request(r1, winb, 2 * HID / 8, 16 * hc, NTO * w.ch, w.lane);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t rr = wrow0 + 8 * j + (w.lane >> 3);
                const float* p = VG + (rr < R ? rr : R - 1) * (2 * HID) + hcol0 + 4 * (w.lane & 7);
                vpre[j] = *reinterpret_cast<const float4*>(p);
                gpre[j] = *reinterpret_cast<const float4*>(p + HID);
                if (rr >= R) vpre[j] = gpre[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        gemm_acc_hs<K, NTH, (RB == 1 ? 4 : 8)>(Ph + w.rb * 32 * LDH, Pl + w.rb * 32 * LDH, LDH, woutb, K / 8, 0, hcol0 / 32, du, w.lane);
        if (ring) xring_request(r2, winb, 2 * HID / 8, HID / 8 + 16 * hc, NTO * w.ch, w.lane);
        float sg[NTH][16], vv[NTH][16];
        auto vg_rows = [&](int off) {
            return [&, off](int r, int cc, float4& v) {
                if constexpr (RB == 1) {
                    v = off ? gpre[r >> 3] : vpre[r >> 3];  // r = 8 j + (lane >> 3), cc = 4 (lane & 7): the mapping of the request
                } else
                v = wrow0 + r < R ? *reinterpret_cast<const float4*>(VG + (wrow0 + r) * (2 * HID) + off + hcol0 + cc)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            };
        };
        if constexpr (RB == 2) wave_load_rows64(my_stage, w.lane, vg_rows(0));
        else wave_load_rows32(my_stage, w.lane, vg_rows(0));
#pragma unroll
        for (int t = 0; t < NTH; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) vv[t][r] = my_stage[acc_row(r, w.lane) * SW + 32 * t + (w.lane & 31)];
        __builtin_amdgcn_wave_barrier();
        if constexpr (RB == 2) wave_load_rows64(my_stage, w.lane, vg_rows(HID));
        else wave_load_rows32(my_stage, w.lane, vg_rows(HID));
#pragma unroll
        for (int t = 0; t < NTH; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) sg[t][r] = sigmoidf_(my_stage[acc_row(r, w.lane) * SW + 32 * t + (w.lane & 31)]);
        __builtin_amdgcn_wave_barrier();
        __syncthreads();  // the previous chunk's readers of U are done
#pragma unroll
        for (int t = 0; t < NTH; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                U[(w.rb * 32 + acc_row(r, w.lane)) * LD128 + HC * w.ch + 32 * t + (w.lane & 31)] = du[t][r] * sg[t][r];  // dv
        __syncthreads();
        if (ring) gemm_acc_x_ring<NTO, 8>(U + w.rb * 32 * LD128, LD128, r1, dn, w.lane);
        else gemm_acc_x<128, NTO, XD>(U + w.rb * 32 * LD128, LD128, winb, 2 * HID / 8, 16 * hc, NTO * w.ch, dn, w.lane);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NTH; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                U[(w.rb * 32 + acc_row(r, w.lane)) * LD128 + HC * w.ch + 32 * t + (w.lane & 31)] =
                    du[t][r] * vv[t][r] * sigmoid_grad_from(sg[t][r]);  // dg
        __syncthreads();
        if (ring) gemm_acc_x_ring<NTO, 8>(U + w.rb * 32 * LD128, LD128, r2, dn, w.lane);
        else gemm_acc_x<128, NTO, XD>(U + w.rb * 32 * LD128, LD128, winb, 2 * HID / 8, HID / 8 + 16 * hc, NTO * w.ch, dn, w.lane);
    }
    __syncthreads();  // everyone is done with U: A takes w = gamma * dn (back in true units)
    if constexpr (SPLIT) {
        __shared__ int last_arrival;
        constexpr int NCHK = HID / 128, IT = ROWS * (K / 4) / NTHREADS;
        const size_t prows = (size_t)gridDim.x * ROWS;
#pragma unroll
        for (int t = 0; t < NTO; t++)
            wave_rows32(dn[t], my_stage, w.lane, [&](int r, int cc, float4 v) {
                st4_agent(Pp + ((size_t)blockIdx.y * prows + (wrow0 + r)) * K + WC * w.ch + 32 * t + cc, v);
            });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the coherent stores are acknowledged (k_node2)
        __syncthreads();
        if (threadIdx.x == 0) {
            const int old = atomicAdd(&cnt[blockIdx.x], 1);
            last_arrival = old == NCHK - 1;
            if (last_arrival) cnt[blockIdx.x] = 0;
        }
        __syncthreads();
        if (!last_arrival) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // consumer side of the hand-over (see k_node2)
        float4 pk[IT][NCHK];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int idx = threadIdx.x + it * NTHREADS, r = idx / (K / 4), c = 4 * (idx % (K / 4));
#pragma unroll
            for (int k = 0; k < NCHK; k++) pk[it][k] = ld4_agent(Pp + ((size_t)k * prows + row0 + r) * K + c);
        }
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int idx = threadIdx.x + it * NTHREADS, r = idx / (K / 4), c = 4 * (idx % (K / 4));
            float4 sum = pk[it][0];
#pragma unroll
            for (int k = 1; k < NCHK; k++)
                sum = make_float4(sum.x + pk[it][k].x, sum.y + pk[it][k].y, sum.z + pk[it][k].z, sum.w + pk[it][k].w);
            const float sc = rs[2 * r + 1];
            const float4 ga = *reinterpret_cast<const float4*>(gamma + c);
            *reinterpret_cast<float4*>(A + r * LDK + c) = make_float4(sum.x * sc * ga.x, sum.y * sc * ga.y, sum.z * sc * ga.z, sum.w * sc * ga.w);
        }
    } else
    acc_foreach<NTO>(dn, w.rb, WC * w.ch, w.lane, [&](int r, int c, float v) { A[r * LDK + c] = v * rs[2 * r + 1] * gamma[c]; });
    __syncthreads();
    // dOC = dH1 Wce (k_expand_bwd's GEMM) from the dH1 tile while it is on chip, when the caller passes dOC: one launch less
    // on the critical path of a small box. The tile goes over the planes, which nobody reads any more.
    float* T = smem + ROWS * LDK;  // [ROWS][260]
    if (dOC) {
        for (int idx = threadIdx.x; idx < ROWS * (K / 4); idx += NTHREADS)  // rows past the end stay zero
            *reinterpret_cast<float4*>(T + (idx / (K / 4)) * LDK + 4 * (idx % (K / 4))) = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
    }
    norm_bwd_rows<K, ROWS>(A, Xin, row0, R, K, ln, [&](int r, int c, float4 dx) {
        const int64_t o = (row0 + r) * K + c;
        const float4 dy = *reinterpret_cast<const float4*>(dY + o);
        const float4 v = make_float4(dy.x + dx.x, dy.y + dx.y, dy.z + dx.z, dy.w + dx.w);
        *reinterpret_cast<float4*>(dXout + o) = v;
        if (dOC) *reinterpret_cast<float4*>(T + r * LDK + c) = v;
    });
    if (dOC) {
        constexpr int NTC = RB;  // 128 columns over the NCH column groups
        __syncthreads();
        f32x16 acc[NTC];
        acc_fill_bias<NTC>(acc, nullptr, 0, w.lane);
        if constexpr (RB == 1) gemm_acc_deep<256, NTC, 8>(T + w.rb * 32 * LDK, LDK, wceb, 32, 0, NTC * w.ch, acc, w.lane);
        else gemm_acc<256, NTC>(T + w.rb * 32 * LDK, LDK, wceb, 32, 0, NTC * w.ch, acc, w.lane);
        acc_foreach<NTC>(acc, w.rb, 32 * NTC * w.ch, w.lane, [&](int r, int c, float v) {
            if (row0 + r < R) dOC[(row0 + r) * D + c] = v;
        });
    }
}


// ---------------------------------------------------------------------------------
// the two entries (pet_stages.h)
// ---------------------------------------------------------------------------------
// dynamic LDS of k_node2 / k_node2w / k_node_bwd2 on `rows` rows: [ row tile fp32 ][ two fp16 planes ][ row scales ]
static constexpr size_t node_lds(int rows) { return (size_t)rows * LD256 * 4 + (size_t)2 * rows * plane_ld(256) * 2 + rows * 8; }

// Split: the partials of the DNF / 128 hidden chunks ([chunk][whole 32-row tiles][DN]) at the front of `scratch`, the tiles' arrival
// counters behind them; the counters are zeroed once per pass, on the stream of the first launch, and reset themselves
static int split_counters(float* scratch, int nt32, bool& cnt_zeroed, hipStream_t st, int*& cnt) {
    cnt = reinterpret_cast<int*>(scratch + (size_t)(DNF / 128) * nt32 * 32 * DN);
    if (!cnt_zeroed) PET_HIP_CHECK(hipMemsetAsync(cnt, 0, nt32 * sizeof(int), st));
    cnt_zeroed = true;
    return PET_OK;
}

int node_fwd(Node form, const AttnLayerW& A, const float* H, const float* OC, float* H1, float* VGn, float* Hn, const Lin* cc_next,
             float* Xcn, float* scratch, bool& cnt_zeroed, int64_t N, hipStream_t st) {
    if (form == Node::Ring) return node_fwd_s(A, H, OC, H1, VGn, Hn, scratch, N, st);  // three ring GEMMs beside the edge MLP
    const WX wce = wx_fwd(A.ce), wci = wx_fwd(A.cmlp_in), wco = wx_fwd(A.cmlp_out);
    const WX wcn = cc_next ? wx_fwd(*cc_next) : WX();  // the next layer's centre tokens in the same launch
    const float* bcn = cc_next ? cc_next->b : nullptr;
    const int nt32 = cdiv(N, 32);
    switch (form) {
    case Node::Split: {  // the hidden chunks of a row tile on four workgroups
        int* cnt;
        PET_TRY(split_counters(scratch, nt32, cnt_zeroed, st, cnt));
        allow_big_lds(k_node2<1, true>, node_lds(32));
        k_node2<1, true><<<dim3(nt32, DNF / 128), NTHREADS, node_lds(32), st>>>(
            H, OC, wce, A.ce.b, A.g_center, A.b_center, wci, A.cmlp_in.b, wco, A.cmlp_out.b, H1, VGn, Hn, N, wcn, bcn, Xcn, scratch, cnt);
        break;
    }
    case Node::Rows32:
        allow_big_lds(k_node2<1>, node_lds(32));
        k_node2<1><<<nt32, NTHREADS, node_lds(32), st>>>(H, OC, wce, A.ce.b, A.g_center, A.b_center, wci, A.cmlp_in.b, wco,
                                                        A.cmlp_out.b, H1, VGn, Hn, N, wcn, bcn, Xcn, nullptr, nullptr);
        break;
    case Node::Rows64:
        allow_big_lds(k_node2w, node_lds(64));
        k_node2w<<<cdiv(N, 64), NTHREADS, node_lds(64), st>>>(H, OC, wce, A.ce.b, A.g_center, A.b_center, wci, A.cmlp_in.b, wco,
                                                             A.cmlp_out.b, H1, VGn, Hn, N, wcn, bcn, Xcn);
        break;
    case Node::LdsTile: {  // (no centre tokens)
        const size_t lds = T256 + T128 + BM * 8;  // h tile | OC tile, SwiGLU chunk | row scales
        allow_big_lds(k_node, lds);
        k_node<<<cdiv(N, BM), NTHREADS, lds, st>>>(H, OC, wce, A.ce.b, A.g_center, A.b_center, wci, A.cmlp_in.b, wco, A.cmlp_out.b,
                                                   H1, VGn, Hn, N);
        break;
    }
    case Node::Ring: break;  // (served above)
    }
    return PET_OK;
}

int node_bwd(Node form, const AttnLayerW& A, const float* dHn, const float* H1, const float* VGn, float* dH1, float* dOC,
             float* scratch, bool& cnt_zeroed, int64_t N, bool layer_norm, float* t_dvg, hipStream_t st) {
    if (form == Node::Ring) return node_bwd_s(A, dHn, H1, VGn, dH1, scratch, N, layer_norm, st);  // two ring GEMMs beside the edge kernels
    if (form == Node::LdsTile) return tile_node_bwd(A, dHn, H1, VGn, dH1, N, layer_norm, t_dvg, st);
    const WX wob = wx_b(A.cmlp_out), wib = wx_b(A.cmlp_in);
    const int nt32 = cdiv(N, 32);
    switch (form) {
    case Node::Split: {  // four workgroups per row tile; the expansion adjoint in the same launch
        int* cnt;
        PET_TRY(split_counters(scratch, nt32, cnt_zeroed, st, cnt));
        allow_big_lds(k_node_bwd2<1, true>, node_lds(32));
        k_node_bwd2<1, true><<<dim3(nt32, DNF / 128), NTHREADS, node_lds(32), st>>>(dHn, H1, VGn, A.g_center, wob, wib, dH1, N,
                                                                                   layer_norm, A.ce.bwd, dOC, scratch, cnt);
        break;
    }
    case Node::Rows32:  // the expansion adjoint in the same launch
        allow_big_lds(k_node_bwd2<1>, node_lds(32));
        k_node_bwd2<1><<<nt32, NTHREADS, node_lds(32), st>>>(dHn, H1, VGn, A.g_center, wob, wib, dH1, N, layer_norm, A.ce.bwd, dOC,
                                                            nullptr, nullptr);
        break;
    case Node::Rows64:
        allow_big_lds(k_node_bwd2<2>, node_lds(64));
        k_node_bwd2<2><<<cdiv(N, 64), NTHREADS, node_lds(64), st>>>(dHn, H1, VGn, A.g_center, wob, wib, dH1, N, layer_norm, nullptr,
                                                                   nullptr, nullptr, nullptr);
        break;
    case Node::Ring: case Node::LdsTile: break;  // (served above)
    }
    return PET_OK;
}

}  // namespace pet
