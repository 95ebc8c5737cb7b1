// SOAP-BPNN Hessian-vector product: H u = d/dR <u, dE/dR>, and with a cell direction
// d/d(R, cell) of  J = <u, dE/dR> + <u_cell, dE/dcell> = sum_i e'_i,  e'_i the tangent of the atomic energies along
// v'_p = u_j - u_i + shift_p . u_cell. The reference gets this from torch's double backward; here it is the
// forward-over-reverse sweep of the training pass (soap_train.hip) with gA = 0 and tangent seed 1, carried one stage
// further than training needs: from the joint adjoints of the expansion coefficients,
//     nu_c = dJ/dc,  lambda_c = dJ/dc',      c = sum_p B(v_p) w,   c' = sum_p (grad B(v_p) . v'_p) w,   B = Y_lm(v / r) R_n(r) fc(r),
// to the pair vectors,
//     dJ/dv_p = sum_{lm n a} w_a(species of j) [ nu_c grad B + lambda_c (grad grad B) v'_p ]                  (k_soap_expand_hvp)
// and then through the shared geometry adjoint (k_pos_grad / k_cell_grad). No weight gradient is formed and no gradient slot
// is read or written. Per-atom workgroups like the training pass: correctness first, nothing here runs on the matrix core.
#include "soap.h"

namespace pet {

// (nu_y, lambda_y) = W1^T (abar_1, adbar_1) of the atom's own network, times the LayerNorm weight: the adjoints of xhat and
// xhat' (y = gamma xhat + beta, y' = gamma xhat'), so that the shared LayerNorm reverse runs with gamma = 1 for every row
// whichever network the row belongs to (k_soap_ybar of the training pass serves legacy = False, one network, only)
__global__ __launch_bounds__(256) void k_soap_ybar_hvp(SoapDims d, const int* __restrict__ sp,
                                                       const SoapSet* __restrict__ sets, const float* __restrict__ pack,
                                                       float* __restrict__ NY, float* __restrict__ LY) {
    __shared__ float ab[2 * MAXH];
    const int i = blockIdx.x, H = d.H, PK = soap_pack_size(H, d.NH);
    const float* pk = pack + (size_t)i * PK + 4;
    if ((int)threadIdx.x < H) { ab[threadIdx.x] = pk[threadIdx.x]; ab[MAXH + threadIdx.x] = pk[H + threadIdx.x]; }
    __syncthreads();
    const SoapSet W = sets[d.legacy ? sp[i] : 0];
    for (int k = threadIdx.x; k < d.S; k += 256) {
        float a = 0.f, b = 0.f;
        for (int j = 0; j < H; j++) {
            const float w = W.W1[(size_t)j * d.S + k];
            a += w * ab[j];
            b += w * ab[MAXH + j];
        }
        const float g = d.layernorm ? W.ln_w[k] : 1.f;
        NY[(size_t)i * d.S + k] = g * a;
        LY[(size_t)i * d.S + k] = g * b;
    }
}

__global__ void k_soap_fill(float* __restrict__ x, float v, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) x[k] = v;
}

// x = p enc[species], x' = p' enc: (nu_p, lambda_p) = (nu_x, lambda_x) enc. The training pass's k_soap_enc_rev without its
// sums for d enc.
__global__ void k_soap_enc_scale(const int* __restrict__ sp, const float* __restrict__ enc, float* __restrict__ NX,
                                 float* __restrict__ LX, int64_t N, int S) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * S) return;
    const float e = enc[(size_t)sp[idx / S] * S + idx % S];
    NX[idx] *= e;
    LX[idx] *= e;
}

// dv[p] = dJ/dv_p for every pair p of atom i. With s = u . v', u' = (v' - u s) / r, G = grad Y, G' = (grad grad Y) v',
// Y' = G . v', (R0, R1, R2) = (R fc, (R fc)', (R fc)'') and, per pair and lm, the sums over the radial functions n of l and
// the species channels a
//     N_n = sum_a w_a nu_c[lm n a],  M_n = sum_a w_a lambda_c[lm n a],
//     A = sum_n N_n R0_n,  A1 = sum_n N_n R1_n,  B0 = sum_n M_n R0_n,  B1 = sum_n M_n R1_n,  B2 = sum_n M_n R2_n:
//     dv = sum_lm [ G (A + s B1) + G' B0 + u (Y A1 + Y' B1 + Y s B2) + u' Y B1 ]
// (grad B = G R0 + Y R1 u;  (grad grad B) v' = G' R0 + Y' R1 u + G R1 s + Y (R2 s u + R1 u')).
// One workgroup per atom, pairs in chunks of PC; thread (pair, lm) forms the lm term in place of G, then thread
// (pair, x | y | z) adds the terms in lm order: a fixed order, no floating-point atomics.
__global__ __launch_bounds__(256) void k_soap_expand_hvp(SoapDims d, const float4* __restrict__ geo,
                                                         const float4* __restrict__ vdot,
                                                         const int* __restrict__ rowptr, const int* __restrict__ sp_nbr,
                                                         const float* __restrict__ table, const float* __restrict__ curv,
                                                         const float* __restrict__ shn, const float* __restrict__ spw,
                                                         const float* __restrict__ NC, const float* __restrict__ LC,
                                                         float4* __restrict__ dv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ys = smem;                     // [PC][NLM]
    float* Yd = Ys + PC * d.NLM;          // [PC][NLM]
    float* Gs = Yd + PC * d.NLM;          // [PC][3][NLM] G, then the lm terms of dv
    float* Gd = Gs + PC * 3 * d.NLM;      // [PC][3][NLM]
    float* R0 = Gd + PC * 3 * d.NLM;      // [PC][F]
    float* R1 = R0 + PC * d.F;            // [PC][F]
    float* R2 = R1 + PC * d.F;            // [PC][F]
    float* us = R2 + PC * d.F;            // [PC][16] u(3), r, 1/r, fc, fc', fc'', v'(3) (then dv), s, u'(3), (1/r)'
    float* ncs = us + PC * 16;            // [NCOEF] nu_c of this atom
    float* lcs = ncs + d.NCOEF;           // [NCOEF] lambda_c
    int* sps = reinterpret_cast<int*>(lcs + d.NCOEF);   // [PC]
    const int i = blockIdx.x, tid = threadIdx.x;
    const int p0 = rowptr[i], p1 = rowptr[i + 1];
    for (int k = tid; k < d.NCOEF; k += 256) {
        ncs[k] = NC[(size_t)i * d.NCOEF + k];
        lcs[k] = LC[(size_t)i * d.NCOEF + k];
    }
    for (int base = p0; base < p1; base += PC) {
        const int npc = min(PC, p1 - base);
        __syncthreads();
        if (tid < npc) {
            const float4 g = geo[base + tid], t = vdot[base + tid];
            const float r = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
            const float ir = r > 0.f ? 1.0f / r : 0.f;
            float* u = us + tid * 16;
            u[0] = g.x * ir; u[1] = g.y * ir; u[2] = g.z * ir; u[3] = r; u[4] = ir;
            float dfc;
            u[5] = shifted_cosine(r, d.rc, d.width, &dfc);
            u[6] = dfc;
            u[7] = shifted_cosine_dd(r, d.rc, d.width);
            u[8] = t.x; u[9] = t.y; u[10] = t.z;
            const float s = u[0] * t.x + u[1] * t.y + u[2] * t.z;
            u[11] = s;
            u[12] = (t.x - u[0] * s) * ir; u[13] = (t.y - u[1] * s) * ir; u[14] = (t.z - u[2] * s) * ir;
            u[15] = -s * ir * ir;
            sps[tid] = sp_nbr[base + tid];
        }
        __syncthreads();
        for (int idx = tid; idx < npc * (d.L + 1); idx += 256) {
            const int pp = idx / (d.L + 1), mm = idx % (d.L + 1);
            const float* u = us + pp * 16;
            float* G = Gs + pp * 3 * d.NLM;
            float* Gt = Gd + pp * 3 * d.NLM;
            sh_chain2(u[0], u[1], u[2], u[12], u[13], u[14], mm, d.L, shn, Ys + pp * d.NLM, Yd + pp * d.NLM, G, G + d.NLM,
                      G + 2 * d.NLM, Gt, Gt + d.NLM, Gt + 2 * d.NLM, u[4], u[15]);
        }
        for (int idx = tid; idx < npc * d.F; idx += 256) {
            const int pp = idx / d.F, f = idx % d.F;
            const float* u = us + pp * 16;
            radial_two(d, table, curv, f, u[3], u[5], u[6], u[7], R0 + idx, R1 + idx, R2 + idx);
        }
        __syncthreads();
        for (int idx = tid; idx < npc * d.NLM; idx += 256) {
            const int pp = idx / d.NLM, lm = idx % d.NLM;
            int l = 0;
            while ((l + 1) * (l + 1) <= lm) l++;
            const int nl = d.n_per_l[l], cb = d.coef_off[l] + (lm - l * l) * nl * d.C;
            const float* w = spw + (size_t)sps[pp] * d.C;
            const float* r0 = R0 + pp * d.F + d.rad_off[l];
            const float* r1 = R1 + pp * d.F + d.rad_off[l];
            const float* r2 = R2 + pp * d.F + d.rad_off[l];
            float A = 0.f, A1 = 0.f, B0 = 0.f, B1 = 0.f, B2 = 0.f;
            for (int n = 0; n < nl; n++) {
                float Nn = 0.f, Mn = 0.f;
                for (int a = 0; a < d.C; a++) {
                    Nn += w[a] * ncs[cb + n * d.C + a];
                    Mn += w[a] * lcs[cb + n * d.C + a];
                }
                A += Nn * r0[n]; A1 += Nn * r1[n];
                B0 += Mn * r0[n]; B1 += Mn * r1[n]; B2 += Mn * r2[n];
            }
            const float* u = us + pp * 16;
            const float s = u[11], y = Ys[idx], yd = Yd[idx];
            const float cg = A + s * B1, cu = y * A1 + yd * B1 + y * s * B2, ct = y * B1;
            float* G = Gs + pp * 3 * d.NLM + lm;
            const float* Gt = Gd + pp * 3 * d.NLM + lm;
#pragma unroll
            for (int k = 0; k < 3; k++) G[k * d.NLM] = G[k * d.NLM] * cg + Gt[k * d.NLM] * B0 + u[k] * cu + u[12 + k] * ct;
        }
        __syncthreads();
        if (tid < npc * 3) {
            const int pp = tid / 3, k = tid % 3;
            const float* G = Gs + (pp * 3 + k) * d.NLM;
            float s = 0.f;
            for (int lm = 0; lm < d.NLM; lm++) s += G[lm];
            us[pp * 16 + 8 + k] = s;
        }
        __syncthreads();
        if (tid < npc) dv[base + tid] = make_float4(us[tid * 16 + 8], us[tid * 16 + 9], us[tid * 16 + 10], 0.f);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The product's own workspace: the tangent sweep's buffers and the front-of-the-tail adjoints (NY .. LC), which the training
// workspace carves for legacy = False models only and the product needs for both.
struct SoapHvpWs {
    float4 *vd, *dv;
    float *Cd, *xd, *pack, *NY, *LY, *NX, *LX, *NC, *LC, *ones, *edot;
    size_t bytes;
};
static void carve_soap_hvp(const SoapDims& d, int64_t N, int64_t E, void* base, SoapHvpWs& w) {
    Carver c(base);
    const int64_t Na = N > 0 ? N : 1, Ea = E > 0 ? E : 1;
    w.vd = c.take<float4>(Ea);
    w.dv = c.take<float4>(Ea);
    w.Cd = c.take<float>(Na * d.NCOEF);
    w.xd = c.take<float>(Na * d.S);
    w.pack = c.take<float>(Na * soap_pack_size(d.H, d.NH));
    w.NY = c.take<float>(Na * d.S); w.LY = c.take<float>(Na * d.S);
    w.NX = c.take<float>(d.layernorm ? Na * d.S : 1); w.LX = c.take<float>(d.layernorm ? Na * d.S : 1);
    w.NC = c.take<float>(Na * d.NCOEF); w.LC = c.take<float>(Na * d.NCOEF);
    w.ones = c.take<float>(d.S);
    w.edot = c.take<float>(Na);
    w.bytes = c.off;
}

int64_t soap_hvp_ws_bytes(const SoapModel& m, int64_t n_nodes, int64_t n_edges) {
    SoapHvpWs w;
    carve_soap_hvp(m.d, n_nodes, n_edges, nullptr, w);
    return (int64_t)w.bytes;
}

// hvp_pos [N,3] = dJ/dR; hvp_cell [S,3,3] (null: not asked for) = dJ/dcell; tangent_atomic [N] (null: not asked for) = e'_i.
// `ws` is the workspace soap_forward ran on: the expansion coefficients and the power spectrum are read from it.
int soap_hvp(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, void* hws, int64_t hws_bytes, const float* u,
             const float* ucell, float* hvp_pos, float* hvp_cell, float* tangent_atomic, hipStream_t st) {
    const SoapDims& d = m.d;
    PET_REQUIRE(m.curv != nullptr, PET_ERR_ARGUMENT,
                "soap_model_set_radial_curvature has not been called: the Hessian-vector product needs the curvature table "
                "of the radial spline");
    PET_REQUIRE(d.H <= MAXH && d.NH <= MAXNH, PET_ERR_UNSUPPORTED, "tail size outside the compiled limits (MAXH / MAXNH)");
    PET_REQUIRE(!ucell || g.shift, PET_ERR_ARGUMENT, "d_u_cell: a cell tangent needs a pet_graph_build handle (cell shifts)");
    PET_REQUIRE(!hvp_cell || g.shift || g.n_edges == 0, PET_ERR_ARGUMENT,
                "d_hvp_cells: a cell result needs a pet_graph_build handle (cell shifts)");
    const size_t lds_hvp = ((size_t)PC * (8 * d.NLM + 3 * d.F + 16 + 1) + 2 * d.NCOEF) * 4;
    PET_REQUIRE(lds_hvp <= 160 * 1024, PET_ERR_UNSUPPORTED,
                "SOAP basis too large for the Hessian-vector product: k_soap_expand_hvp needs more than 160 KB of LDS");
    SoapWs w;
    carve_soap(d, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "soap workspace too small");
    SoapHvpWs t;
    carve_soap_hvp(d, g.n_nodes, g.n_edges, hws, t);
    PET_REQUIRE((int64_t)t.bytes <= hws_bytes, PET_ERR_ARGUMENT, "soap Hessian-vector workspace too small");
    const int N = (int)g.n_nodes;
    if (N == 0) return PET_OK;
    Graph::FwdRecord* rec = g.fwd_record(ws);
    SoapTrainPlan plan;
    PET_TRY(soap_plan_train(m, rec, plan));
    if (g.n_edges == 0) {   // no pair: every e_i is a constant. Nothing that indexes pairs is launched.
        PET_HIP_CHECK(hipMemsetAsync(hvp_pos, 0, (size_t)N * 3 * 4, st));
        if (hvp_cell) PET_HIP_CHECK(hipMemsetAsync(hvp_cell, 0, (size_t)g.n_systems * 9 * 4, st));
        if (tangent_atomic) PET_HIP_CHECK(hipMemsetAsync(tangent_atomic, 0, (size_t)N * 4, st));
        return PET_OK;
    }
    if (plan.rebuild_full) {  // behind a packed inference forward: the full power spectrum from the coefficients, as in training
        soap_ps_full(m, g, w, st);
        rec->soap_plan.packed = false;
        rec->soap_plan.ps = SoapPlan::PowerSpectrum::Mfma;
    }
    // 1. tangent sweep
    k_edge_tangent<<<cdiv(g.n_edges, 256), 256, 0, st>>>(u, g.ctr, g.nbr, g.shift, g.sys, ucell, t.vd, g.n_edges);
    {
        const size_t lds = (size_t)PC * (5 * d.NLM + 2 * d.F + 12 + 1) * 4;
        allow_big_lds(k_soap_expand_jvp, lds);
        k_soap_expand_jvp<<<N, 256, lds, st>>>(d, g.geo, t.vd, g.rowptr, g.sp_nbr, m.table, m.shnorm, m.coef_lut, m.species_w,
                                               t.Cd);
    }
    const size_t lds2 = (size_t)2 * d.NCOEF * 4;
    allow_big_lds(k_soap_ps_jvp, lds2);
    k_soap_ps_jvp<<<N, 256, lds2, st>>>(d, w.Cf, t.Cd, g.sp, m.enc, m.feat_lut, t.xd);
    // 2. the tail's primal + tangent forward and joint reverse: seeds (gA, e'bar) = (0, 1)
    k_soap_tail_train<<<N, 256, 0, st>>>(d, w.feats, t.xd, g.sp, m.sets, nullptr, 1.f, t.pack,
                                         tangent_atomic ? tangent_atomic : t.edot);
    // 3. first Linear, 4. LayerNorm (second order), 5. encoding
    k_soap_ybar_hvp<<<N, 256, 0, st>>>(d, g.sp, m.sets, t.pack, t.NY, t.LY);
    float *NX = t.NY, *LX = t.LY;
    if (d.layernorm) {
        k_soap_fill<<<cdiv(d.S, 256), 256, 0, st>>>(t.ones, 1.f, d.S);
        PET_TRY(norm_rev_rows(w.feats, t.xd, t.ones, 1, 1e-5f, t.NY, t.LY, t.NX, t.LX, N, d.S, st));
        NX = t.NX; LX = t.LX;
    }
    if (m.enc) k_soap_enc_scale<<<cdiv((int64_t)N * d.S, 256), 256, 0, st>>>(g.sp, m.enc, NX, LX, N, d.S);
    // 6. power spectrum, 7. expansion, 8. / 9. geometry
    allow_big_lds(k_soap_ps_rev2, lds2);
    k_soap_ps_rev2<<<N, 256, lds2, st>>>(d, w.Cf, t.Cd, NX, LX, t.NC, t.LC);
    allow_big_lds(k_soap_expand_hvp, lds_hvp);
    k_soap_expand_hvp<<<N, 256, lds_hvp, st>>>(d, g.geo, t.vd, g.rowptr, g.sp_nbr, m.table, m.curv, m.shnorm, m.species_w,
                                               t.NC, t.LC, t.dv);
    k_pos_grad<<<cdiv(N, 16), 256, 0, st>>>(t.dv, g.rowptr, g.rev, hvp_pos, N);
    if (hvp_cell)
        k_cell_grad<<<(int)g.n_systems, 256, 0, st>>>(t.dv, g.shift, g.ctr, g.sys, g.rowptr, hvp_cell, N, g.n_edges, 0);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace pet
