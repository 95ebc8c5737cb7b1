// PET reverse pass (dL/dR) on gfx950. Hand-written adjoint of every stage of pet_fwd.hip's driver;
// replaces torch.autograd.grad(E, positions) of utils/output_gradient.py:34-40 for the
// inference / force path (activation gradients only, no weight gradients).
//
// Every dense adjoint is a row-tile GEMM against the TRANSPOSED weight (Lin::bwd packs
// W^T in fragment order), so the same MFMA toolkit applies. Cross-atom terms are
// gathers, never float atomics:
//   * ji message gather   e_rev[p] = e[rev[p]]  ->  de[p] += dcat_hi[rev[p]]   (rev is an involution)
//   * dE/dR_a = sum_{p in row a} (dv[rev[p]] - dv[p])                          (v_p = r_j - r_i + S.cell)
// so the result is deterministic run to run.
// The stage adjoints and their launchers: pet_tile.hip (LDS-tile family), pet_node.hip, pet_attn.hip and the pipelined / ring /
// fused-block files (pet_stages.h declares them by stage). This file: the three drivers (heads, features, geometry), the geometry
// adjoint's kernels, the multi-target head paths and the entry points of the ABI.
#include "common.h"
#include "cutoff.h"
#include "model.h"
#include "pet_stages.h"
#include "pet_ws.h"
#include "train.h"

namespace pet {

// ---------------------------------------------------------------------------------
// geometry adjoint
// ---------------------------------------------------------------------------------
// key-bias adjoint -> cutoff-factor gradient: bias = log(clamp(fc, 1e-15)), so the gradient
// passes only where fc >= 1e-15 (transformer.py:109-110); heads and layers are summed here.
// dbias_l: one head-major slice [NHEAD, E] per attention layer, each written once by that layer's adjoint
__global__ void k_dfc_attn(const float* __restrict__ fc, const float* __restrict__ dbias_l, int slices,
                           float* __restrict__ dfc_attn, int64_t E, int hstep) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    float dbias = 0.f;
    for (int h = 0; h < slices * NHEAD; h += hstep) dbias += dbias_l[(int64_t)h * E + p];
    const float f = fc[p];
    dfc_attn[p] = f >= 1e-15f ? dbias / f : 0.f;
}
int dfc_attn(const float* fc, const float* dbias_l, int slices, float* dfc, int64_t E, int hstep, hipStream_t st) {
    k_dfc_attn<<<cdiv(E, 256), 256, 0, st>>>(fc, dbias_l, slices, dfc, E, hstep);
    return PET_OK;
}

// dgeo = d/d(vx,vy,vz,dist), dfc_a + dfc_b = d/d(cutoff factor)  ->  d/d(edge vector)
__global__ void k_geom_bwd(const float4* __restrict__ geo, const float* __restrict__ d0,
                           const float* __restrict__ dgeo, const float* __restrict__ dfc_a,
                           const float* __restrict__ dfc_b, float4* __restrict__ dv, int64_t E, float cutoff,
                           float width, int fn, const float* __restrict__ pc, float* __restrict__ gc) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const float4 g = geo[p];
    const float4 dg = reinterpret_cast<const float4*>(dgeo)[p];
    const float dfc_t = (dfc_a ? dfc_a[p] : 0.f) + (dfc_b ? dfc_b[p] : 0.f);
    // adaptive cutoff: fc = f(d - c) with the pair cutoff c, so df/dc = -df/dd
    const float dd0 = dfc_t * cutoff_deriv_dev(d0[p], pc ? pc[p] : cutoff, width, fn);
    if (gc) gc[p] = -dd0;
    const float nrm = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    const float c_dist = dg.w / g.w;                    // d sqrt(v.v + 1e-15) / dv = v / dist
    const float c_d0 = nrm > 0.f ? dd0 / nrm : 0.f;     // d |v| / dv = v / |v|
    const float c = c_dist + c_d0;
    dv[p] = make_float4(dg.x + c * g.x, dg.y + c * g.y, dg.z + c * g.z, 0.f);
}

// dE/dR_a = sum_{p in row a} (dv[rev[p]] - dv[p]); one 16-lane group per atom
__global__ void k_pos_grad(const float4* __restrict__ dv, const int* __restrict__ rowptr, const int* __restrict__ rev,
                           float* __restrict__ gpos, int N) {
    const int gid = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const int a = gid < N ? gid : N - 1;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int p = rowptr[a] + l; p < rowptr[a + 1]; p += 16) {
        const float4 m = dv[p], q = dv[rev[p]];
        x += q.x - m.x; y += q.y - m.y; z += q.z - m.z;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        x += __shfl_xor(x, o); y += __shfl_xor(y, o); z += __shfl_xor(z, o);
    }
    if (l == 0 && gid < N) {
        gpos[3 * gid] = x; gpos[3 * gid + 1] = y; gpos[3 * gid + 2] = z;
    }
}

// ---- adaptive cutoff adjoint (adaptive_cutoff.py:196-229: the implicit-function step carries the gradient)
// g_r[i] = dL/d r_i = sum over kept edges touching i of dL/dc / 2 = 1/2 sum_{p in row i} (gc[p] + gc[rev p])
__global__ void k_adapt_gr(const float* __restrict__ gc, const int* __restrict__ rowptr, const int* __restrict__ rev,
                           float* __restrict__ gr, int N) {
    const int gid = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const int a = gid < N ? gid : N - 1;
    float s = 0.f;
    for (int p = rowptr[a] + l; p < rowptr[a + 1]; p += 16) s += gc[p] + gc[rev[p]];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && gid < N) gr[gid] = 0.5f * s;
}
// every input edge q of atom i (all-edge CSR): d r_i / d d_q = -(d bump(d_q; r, w)/d d_q) / dn_root,
// d bump / d d = -(d bump / d r); the edge vector gets (v / |v|) times that
__global__ void k_adapt_dv(const int* __restrict__ rowptr0, const int* __restrict__ perm0,
                           const float4* __restrict__ vin, const float* __restrict__ gr,
                           const float* __restrict__ r_newton, const float* __restrict__ inv_dn,
                           float4* __restrict__ dvA, int N, float w) {
    const int gid = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    if (gid >= N) return;
    const float coef = gr[gid] * inv_dn[gid], r = r_newton[gid];
    for (int q = rowptr0[gid] + l; q < rowptr0[gid + 1]; q += 16) {
        const float4 v = vin[perm0[q]];
        // d r_adapt / d d_q = -(d bump/d d)(d_q; r) * inv_dn  (bump derivative w.r.t. d, bump taper = BUMP)
        const float dd = -coef * cutoff_deriv_dev(v.w, r, w, PET_CUTOFF_BUMP);
        const float nrm = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
        const float c = nrm > 0.f ? dd / nrm : 0.f;
        dvA[q] = make_float4(c * v.x, c * v.y, c * v.z, 0.f);
    }
}
// "grid" method: r_i = sum_k p_k w_k(n_i1 .. n_iK), n_ik = sum_q bump(d_q; p_k, w): every input edge q of atom i gets
//   d r_i / d d_q = sum_k (d r_i / d n_ik) (d bump / d d)(d_q; p_k, w)   with the per-atom row drdn of k_adaptive_grid
__global__ void k_adapt_dv_grid(const int* __restrict__ rowptr0, const int* __restrict__ perm0,
                                const float4* __restrict__ vin, const float* __restrict__ gr,
                                const float* __restrict__ drdn, float4* __restrict__ dvA, int N, float w, int K,
                                float pmin, float dp) {
    __shared__ float s_c[16][GRID_MAX_PROBES];
    const int grp = threadIdx.x >> 4;
    const int gid = blockIdx.x * (blockDim.x / 16) + grp;
    const int l = threadIdx.x & 15;
    const int a = gid < N ? gid : N - 1;
    for (int k = l; k < K; k += 16) s_c[grp][k] = gr[a] * drdn[(int64_t)a * GRID_MAX_PROBES + k];
    __syncthreads();
    if (gid >= N) return;
    for (int q = rowptr0[gid] + l; q < rowptr0[gid + 1]; q += 16) {
        const float4 v = vin[perm0[q]];
        float dd = 0.f;
        for (int k = 0; k < K; k++) dd += s_c[grp][k] * cutoff_deriv_dev(v.w, pmin + (float)k * dp, w, PET_CUTOFF_BUMP);
        const float nrm = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
        const float c = nrm > 0.f ? dd / nrm : 0.f;
        dvA[q] = make_float4(c * v.x, c * v.y, c * v.z, 0.f);
    }
}
// gpos[a] += sum_{q in row0 a} (dvA[rev0 q] - dvA[q])
__global__ void k_pos_grad_acc(const float4* __restrict__ dv, const int* __restrict__ rowptr,
                               const int* __restrict__ rev, float* __restrict__ gpos, int N) {
    const int gid = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const int a = gid < N ? gid : N - 1;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int p = rowptr[a] + l; p < rowptr[a + 1]; p += 16) {
        const float4 m = dv[p];
        const int rp = rev[p];
        const float4 q = rp >= 0 ? dv[rp] : make_float4(0.f, 0.f, 0.f, 0.f);
        x += q.x - m.x; y += q.y - m.y; z += q.z - m.z;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        x += __shfl_xor(x, o); y += __shfl_xor(y, o); z += __shfl_xor(z, o);
    }
    if (l == 0 && gid < N) {
        gpos[3 * gid] += x; gpos[3 * gid + 1] += y; gpos[3 * gid + 2] += z;
    }
}

// dE/dcell[s][a][k] = sum_{edges of system s} S_a dv_k (structures.py:212-219); one block per system
__global__ void k_cell_grad(const float4* __restrict__ dv, const int* __restrict__ shift, const int* __restrict__ ctr,
                            const int* __restrict__ sys, const int* __restrict__ rowptr, float* __restrict__ gcell,
                            int N, int64_t E, int accumulate) {
    // systems are contiguous atom ranges; find this system's atom range by scanning sys[] boundaries
    const int s = blockIdx.x;
    __shared__ double red[9][256];  // fp64 sums: a system's edges with a shift are a signed sum with heavy cancellation
    __shared__ int range[2];
    if (threadIdx.x == 0) {
        int lo = 0, hi = N;
        // lower bound of s and of s+1 in the sorted sys[] array
        int a = 0, b = N;
        while (a < b) { int m = (a + b) >> 1; if (sys[m] < s) a = m + 1; else b = m; }
        lo = a; b = N;
        while (a < b) { int m = (a + b) >> 1; if (sys[m] < s + 1) a = m + 1; else b = m; }
        hi = a;
        range[0] = rowptr[lo];
        range[1] = rowptr[hi];
    }
    __syncthreads();
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = 0.0;
    for (int p = range[0] + threadIdx.x; p < range[1]; p += blockDim.x) {
        const int ia = shift[3 * p], ib = shift[3 * p + 1], ic = shift[3 * p + 2];
        if ((ia | ib | ic) == 0) continue;  // most edges stay inside the cell
        const float4 d = dv[p];
        const double sa = ia, sb = ib, sc = ic, dx = d.x, dy = d.y, dz = d.z;
        acc[0] += sa * dx; acc[1] += sa * dy; acc[2] += sa * dz;
        acc[3] += sb * dx; acc[4] += sb * dy; acc[5] += sb * dz;
        acc[6] += sc * dx; acc[7] += sc * dy; acc[8] += sc * dz;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 9; k++) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 9)
        gcell[9 * s + threadIdx.x] = (accumulate ? gcell[9 * s + threadIdx.x] : 0.f) + (float)red[threadIdx.x][0];
}

// ---------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------
// (pet_graph_build refuses a list with an edge that has no (j, i, -S) partner, so the reverse pass needs no check
//  and no host synchronisation of its own.)
// Stage P: adjoint of PETBackend.predict. seeds gA [N] -> w.dH [N,DN], w.dM [E,D], w.dfc [E]
int backward_predict(const Model& m, const Graph& g, Workspace& w, const float* gA, hipStream_t st,
                     Trainer* tr = nullptr) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    const double fE = (double)E, fN = (double)N;
    const GnnBufs& last = w.gnn.back();
    StagePlan plan;  // (no record: what this stage reads, the heads' inputs, every forward leaves behind)
    PET_TRY(plan_backward(m, g, nullptr, tr != nullptr, plan));
    if (E > 0) {
        ProfScope ps("head_edge_bwd", st, fE * 2.0 * (D * DH + DH * DH + DH));
        switch (plan.head_edge) {
        case Rows::Ring: PET_TRY(head_edge_bwd_s(m, last.Mout, gA, g.ctr, g.fc, w.ypred_e, w.dfc, w.dM, E, st)); break;
        case Rows::Pipelined:
            PET_TRY(trr_head_edge_bwd(m, last.Mout, gA, g.ctr, g.fc, w.ypred_e, w.dfc, w.dM, E, tr ? w.hs1 : nullptr,
                                      tr ? w.hda2 : nullptr, tr ? w.hda1 : nullptr, tr ? w.hs2y : nullptr, st));
            break;
        case Rows::LdsTile:
            PET_TRY(tile_head_bwd(true, last.Mout, m.eh0, m.eh2, m.ell_w, gA, g.ctr, g.fc, w.ypred_e, w.dfc, w.dM, E,
                                  tr ? w.hs1 : nullptr, tr ? w.hda2 : nullptr, tr ? w.hda1 : nullptr, tr ? w.hs2y : nullptr, nullptr,
                                  nullptr, st));
            break;
        }
        if (tr) tr->heads(true, last.Mout, D, E, gA);
    }
    {
        SideStream ss = side_stream();
        ss.enabled = plan.side_heads;
        const hipStream_t s2 = ss.stream(st);
        ss.fork(st);
        {
            ProfScope ps("head_node_bwd", s2, fN * 2.0 * (DN * DH + DH * DH + DH));
            PET_TRY(tile_head_bwd(false, last.Hout, m.nh0, m.nh2, m.nll_w, gA, nullptr, nullptr, nullptr, nullptr, w.dH, N,
                                  tr ? w.hs1 : nullptr, tr ? w.hda2 : nullptr, tr ? w.hda1 : nullptr, tr ? w.hs2y : nullptr, nullptr,
                                  nullptr, s2));
            if (tr) tr->heads(false, last.Hout, DN, N, gA);
        }
        ss.join(st);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// Stage F: adjoint of PETBackend.calculate_features. (w.dH, w.dM) -> w.dgeo [E,4], w.dbias [E]
// Residual featuriser: one (node, edge) gradient pair per readout layer in g_node / g_edge (null entries = zero) instead
// of the seeds in w.dH / w.dM.
int backward_features(const Model& m, const Graph& g, Workspace& w, hipStream_t st, Trainer* tr = nullptr,
                      const float* const* g_node = nullptr, const float* const* g_edge = nullptr) {
    const int64_t N = g.n_nodes, E = g.n_edges, R = E + N;
    if (E == 0) return PET_OK;
    const int nt = attn_tiles(g);
    PET_REQUIRE(nt <= 8, PET_ERR_UNSUPPORTED, "more than 127 neighbours per atom is not supported yet");
    const bool post = m.post_ln(), res = m.residual(), ln = m.layer_norm();
    PET_REQUIRE(!tr || m.trainable(), PET_ERR_UNSUPPORTED,
                "training is built for transformer_type=PreLN, featurizer_type=feedforward only");
    const int nxm = ln ? 5 : 1;  // weight-gradient row source: LayerNorm-hat / RMSNorm-hat of the saved input
    PET_REQUIRE(!res || (g_node && g_edge), PET_ERR_ARGUMENT,
                "residual featuriser: the reverse pass starts from one gradient pair per readout layer "
                "(pet_backward_features_layers)");
    const float scale = 1.0f / (sqrtf((float)HD) * m.h.attention_temperature);
    const double fE = (double)E, fN = (double)N, fR = (double)R;
    // which kernel serves every stage below: decided here, once, from what the forward of this workspace left behind; an adjoint
    // that the switches no longer allow to follow that forward is refused before anything is launched (pet_plan.hip)
    StagePlan plan;
    PET_TRY(plan_backward(m, g, w.base ? g.fwd_record(w.base) : nullptr, tr != nullptr, plan));
    bool node_cnt_zeroed = false;  // k_node_bwd2 SPLIT: arrival counters zeroed once per adjoint, then they reset themselves
    const bool dxf_fused = plan.dxf_fused;
    PET_HIP_CHECK(hipMemsetAsync(w.dgeo, 0, E * 4 * sizeof(float), st));
    float* dH = w.dH;
    float* dH_alt = w.dH2;
    float* dX = w.dX;
    float* dX_alt = w.dX2;
    float* dM = w.dM;      // gradient w.r.t. the messages leaving the layer below the one being processed
    float* dM_alt = w.dM2;
    bool have_dM = !res;   // residual: no message gradient enters the last layer
    // node-feature adjoint chain on the side stream: it only meets the edge chain at output_linear^T
    // (needs dOC) and at the centre rows of the token gradient (k_center_bwd)
    SideStream ss = side_stream();
    ss.enabled = plan.side;
    const hipStream_t s2 = ss.stream(st);
    ss.fork(st);  // the seeds in w.dH / w.dM were produced on the main stream
    for (int gi = m.h.num_gnn_layers - 1; gi >= 0; gi--) {
        const GnnLayerW& G = m.gnn[gi];
        const GnnBufs& B = w.gnn[gi];
        const GnnPlan& P = plan.gnn[gi];
        // dH is the adjoint of the node features LEAVING this layer, where the system embedding was added (training:
        // the side stream is off, so dH is complete on this stream)
        if (tr) tr->cond_accumulate(dH, gi == m.h.num_gnn_layers - 1);
        if (res) {
            // backend.py:621-647: this layer's features were read out (seeds g_node / g_edge), its edge features were
            // averaged into the next layer's messages, and its node features started from a fresh embedding
            if (g_node[gi]) PET_HIP_CHECK(hipMemcpyAsync(dH, g_node[gi], N * DN * sizeof(float), hipMemcpyDeviceToDevice, st));
            else PET_HIP_CHECK(hipMemsetAsync(dH, 0, N * DN * sizeof(float), st));
            ProfScope ps("comb_bwd", st, 0.0, fE * 4.0 * 4 * D);
            PET_TRY(tile_resmix_bwd(g_edge[gi], have_dM ? dM : nullptr, g.rev, dX, dM_alt, E, st));
            std::swap(dM, dM_alt);
            have_dM = true;
        } else {
            {
                ProfScope ps("comb_bwd", st, fE * 2.0 * (2 * D * 2 * D + 2 * D * D), fE * 4.0 * (3 * D + 2 * D + 2 * D));  // dM, e, e[rev], CA in; dcat out
                if (P.comb == Rows::Ring)
                    PET_TRY(comb_bwd_s(dM, B.XF, g.rev, B.LNS, B.CA, G.comb0_g, G.comb2, w.dcat, E, dxf_fused, st));
                else
                    PET_TRY(trr_comb_bwd(dM, B.XF, g, G, B.LNS, B.CA, w.dcat, E, tr ? w.dCA : nullptr, st, dxf_fused));
                if (tr) {
                    const std::string gs = std::to_string(gi);
                    tr->linear("combination_mlps." + gs + ".2", D, 2 * D, {dM, nullptr, 0, D},
                               {B.CA, 2 * D, 0, nullptr, nullptr}, 3, E);
                    tr->linear_after_norm("combination_mlps." + gs + ".0", G.comb0.w, 2 * D, 2 * D,
                                          {w.dCA, nullptr, 0, 2 * D}, {B.XF, D, 0, g.rev, B.LNS}, 4, E,
                                          "combination_norms." + gs + ".weight", G.ln_g,
                                          "combination_norms." + gs + ".bias", G.ln_b);
                }
            }
            if (!dxf_fused) {
                ProfScope ps("dxf", st, 0.0);
                PET_TRY(tile_dxf(dM, w.dcat, g.rev, dX, E, st));
            }
            if (g.x_fn) {   // one box over several ranks: the adjoints on ghost rows go home to their owners
                int rc = exchange_backward(g, dX, gi, st);
                if (rc) return rc;
            }
        }
        for (int a = m.h.num_attention_layers - 1; a >= 0; a--) {
            const AttnLayerW& A = G.attn[a];
            const AttnBufs& Ab = B.attn[a];
            const LayerPlan& Q = P.layers[a];
            const bool trr_l = Q.attn != Attn::LdsTile;  // (the pipelined QKV / projection adjoints and edge-MLP adjoint go together)
            const std::string lp = "gnn_layers." + std::to_string(gi) + ".trans.layers." + std::to_string(a);
            // dX (edge rows) = grad wrt the edge MLP output; dH = grad wrt Hn
            {
                ProfScope ps("node_bwd", s2, fN * 2.0 * (D * DN + DN * 2 * DNF + DNF * DN));
                // scratch: the attention-output temporary of the forward pass, which no adjoint kernel touches
                PET_TRY(node_bwd(Q.node, A, dH, Ab.H1, Ab.VGn, dH_alt, w.dOC, w.AO, node_cnt_zeroed, N, ln, tr ? w.dVGn : nullptr, s2));
                if (Q.expand == Center::Ring) PET_TRY(expand_bwd_s(A.ce, dH_alt, w.dOC, N, s2));
                else if (Q.expand == Center::LdsTile) PET_TRY(tile_expand_bwd(A.ce, dH_alt, w.dOC, N, s2));
                if (tr) {
                    tr->linear(lp + ".center_mlp.w_out", DN, DNF, {dH, nullptr, 0, DN},
                               {Ab.VGn, 2 * DNF, DNF, nullptr, nullptr}, 2, N);
                    tr->linear_after_norm(lp + ".center_mlp.w_in", A.cmlp_in.w, 2 * DNF, DN,
                                          {w.dVGn, nullptr, 0, 2 * DNF}, {Ab.H1, DN, 0, nullptr, nullptr}, nxm, N,
                                          lp + ".norm_center_features.weight", A.g_center,
                                          ln ? lp + ".norm_center_features.bias" : std::string(), ln ? A.b_center : nullptr);
                    tr->linear(lp + ".center_expansion", DN, D, {dH_alt, nullptr, 0, DN},
                               {Ab.OC, D, 0, nullptr, nullptr}, 0, N);
                }
            }
            if (post) {
                // transformer.py:245-247 backwards on every token: norm_mlp^T of [dX edge rows ; dOC], the MLP residual
                // block on normalised tokens, norm_attention^T; dX_alt = gradient of (tokens + attention output)
                ProfScope ps("emlp_bwd", st, fR * 2.0 * (D * 2 * DFF + DFF * D));
                PET_TRY(tile_rownorm_bwd(dX, w.dOC, Ab.S2, A.g_mlp, ln, dX_alt, E, R, st));
                PET_TRY(tile_emlp_bwd(false, dX_alt, nullptr, Ab.VG, nullptr, false, A.mlp_in, A.mlp_out, dX, R, nullptr, st));
                PET_TRY(tile_rownorm_bwd(dX, dX + E * D, Ab.X1, A.g_attn, ln, dX_alt, E, R, st));
            } else {
                ProfScope ps("emlp_bwd", st, fE * 2.0 * (D * 2 * DFF + DFF * D), fE * 4.0 * (3 * D + (Q.emlp_saved ? 2 * DFF : 0)));  // dY, X1 (and the saved VG) in; dX1 out
                // dxf_fused, last attention layer: dXF[p] = (dM[p] + dcat[p][:D]) + dcat[rev[p]][D:] -- the bracket left the
                // combination adjoint in dcat's first half, the gather is made while the kernel reads its tile
                const bool gat = dxf_fused && a == m.h.num_attention_layers - 1;
                switch (Q.emlp) {
                case Rows::Ring:  // the forward of this workspace did not save [v; g]: recomputed
                    PET_TRY(emlp_bwd_s(gat ? w.dcat : dX, Ab.X1, ln, A.mlp_in_g, A.mlp_out, dX_alt, E, st, gat ? 2 * D : D,
                                       gat ? w.dcat + D : nullptr, gat ? g.rev : nullptr));
                    break;
                case Rows::Pipelined:
                    if (gat)
                        trr_emlp_bwd(w.dcat, Ab.X1, Ab.VG, A.g_mlp, ln ? A.b_mlp : nullptr, A.mlp_in, A.mlp_out, dX_alt, E, st,
                                     nullptr, 2 * D, w.dcat + D, g.rev);
                    else
                        trr_emlp_bwd(dX, Ab.X1, Ab.VG, A.g_mlp, ln ? A.b_mlp : nullptr, A.mlp_in, A.mlp_out, dX_alt, E, st,
                                     tr ? w.dVG : nullptr);
                    break;
                case Rows::LdsTile:
                    PET_TRY(tile_emlp_bwd(true, dX, Ab.X1, Ab.VG, A.g_mlp, ln, A.mlp_in, A.mlp_out, dX_alt, E, tr ? w.dVG : nullptr, st));
                    break;
                }
                if (tr) {
                    tr->linear(lp + ".mlp.w_out", D, DFF, {dX, nullptr, 0, D}, {Ab.VG, 2 * DFF, DFF, nullptr, nullptr},
                               2, E);
                    tr->linear_after_norm(lp + ".mlp.w_in", A.mlp_in.w, 2 * DFF, D, {w.dVG, nullptr, 0, 2 * DFF},
                                          {Ab.X1, D, 0, nullptr, nullptr}, nxm, E, lp + ".norm_mlp.weight", A.g_mlp,
                                          ln ? lp + ".norm_mlp.bias" : std::string(), ln ? A.b_mlp : nullptr);
                }
            }
            ss.join(st);  // dOC ready
            // dX_alt (edge rows) = dX1, dH_alt = dH1; PostLN: dX_alt holds all E+N rows of d(tokens + attention output)
            const float* dOCr = post ? dX_alt + E * D : w.dOC;
            // the per-atom fused adjoint (pet_ablk.hip): Q, K, V recomputed from X, only dX and the key-bias gradient leave
            if (Q.attn == Attn::Fused) {
                ProfScope ps("attn_blk_bwd", st, fR * 2.0 * D * 4 * D + 2.0 * 4.0 * D * g_sum_t2(g), fR * 4.0 * 3 * D);  // algorithmic: the adjoint's own products (the Q, K, V recomputation is this design's choice, not counted); X, dX1 in; dX out
                // (the key-bias reduction below assumes every layer took the same form: the plan gives all of them one)
                PET_TRY(ablk_bwd(m, g, A, Ab.X, dX_alt, w.dOC, dX,
                                 w.dbias_l + ((int64_t)gi * m.h.num_attention_layers + a) * NHEAD * E, scale, st));
            } else {
            {
                ProfScope ps("oproj_bwd", st, fR * 2.0 * D * D, fR * 4.0 * 2 * D);  // dX1 (| dOC) in; dAO out
                if (trr_l) trr_oproj_bwd(dX_alt, w.dOC, A.out, w.dAO, E, R, st);
                else PET_TRY(tile_oproj_bwd(dX_alt, dOCr, A.out, w.dAO, E, R, st));
                if (tr)
                    tr->linear(lp + ".attention.output_linear", D, D, {dX_alt, w.dOC, E, D},
                               {Ab.AO, D, 0, nullptr, nullptr}, 0, R);
            }
            {
                ProfScope ps("attn_bwd", st, 2.0 * 4.0 * D * g_sum_t2(g), fR * 4.0 * (3 * D + D + 3 * D));
                float* dbias_h = w.dbias_l + ((int64_t)gi * m.h.num_attention_layers + a) * NHEAD * E;
                PET_TRY(attn_bwd(nt, plan.attn_preload, Ab.QKV, w.dAO, g, w.dQKV, dbias_h, scale, st));
            }
            if (tr)
                tr->linear_after_norm(lp + ".attention.input_linear", A.qkv.w, 3 * D, D, {w.dQKV, nullptr, 0, 3 * D},
                                      {Ab.X, D, 0, nullptr, nullptr}, nxm, R, lp + ".norm_attention.weight", A.g_attn,
                                      ln ? lp + ".norm_attention.bias" : std::string(), ln ? A.b_attn : nullptr);
            {
                ProfScope ps("qkv_bwd", st, fR * 2.0 * D * 3 * D, fR * 4.0 * (3 * D + 3 * D));  // dQKV, X, dX1 in; dX out
                if (trr_l) trr_qkv_bwd(w.dQKV, Ab.X, A.g_attn, ln, A.qkv, dX_alt, dX, E, R, st);
                else PET_TRY(tile_qkv_bwd(post, w.dQKV, Ab.X, A.g_attn, ln, A.qkv, dX_alt, dX, E, R, st));
            }
            }
            ss.fork(st);  // centre rows of dX ready
            {
                ProfScope ps("center_bwd", s2, fN * 2.0 * DN * D);
                if (Q.center == Center::Ring) PET_TRY(center_bwd_s(A.cc, dX + E * D, dH_alt, dH, N, s2));
                else PET_TRY(tile_center_bwd(plan.center_bwd_deep, A.cc, dX + E * D, dH_alt, dH, N, s2));
                if (tr)
                    tr->linear(lp + ".center_contraction", D, DN, {dX + E * D, nullptr, 0, D},
                               {Ab.H, DN, 0, nullptr, nullptr}, 0, N);
            }
            // now dX (edge rows) = grad wrt this layer's input edge tokens, dH = grad wrt its input h
        }
        {
            ProfScope ps("compress_bwd", st, fE * 2.0 * (D * D * (gi == 0 ? 3 : 4) + 4 * D));
            if (P.compress == Rows::Ring) PET_TRY(compress_bwd_s(gi == 0, dX, B.a0, G, w.dgeo, dM, E, st));
            else if (P.compress == Rows::Pipelined)
                PET_TRY(trr_compress_bwd(gi == 0, dX, B.a0, G, w.dgeo, dM, E, tr ? w.da0 : nullptr, st));
            else
                PET_TRY(tile_compress_bwd(gi == 0, dX, B.a0, G, w.dgeo, dM, E, tr ? w.da0 : nullptr, st));
            if (tr) {
                const std::string pre = "gnn_layers." + std::to_string(gi);
                tr->linear(pre + ".compress.2", D, D, {dX, nullptr, 0, D}, {B.a0, D, 0, nullptr, nullptr}, 3, E);
                tr->compress0(gi, w.da0, gi > 0 ? w.gnn[gi - 1].Mout : nullptr);
            }
        }
        // dM now holds d/dMout of layer gi-1 (pass-through + compress adjoint)
    }
    ss.join(st);
    if (tr) {
        tr->embeddings(dH, dM);
        tr->cond_finish();
        if (tr->err) return tr->err;
    }
    // fused adjoint: one slice per attention layer (the head sum), at the place of the layer's first head slice
    PET_TRY(dfc_attn(g.fc, w.dbias_l, m.h.num_gnn_layers * m.h.num_attention_layers, w.dbias, E, plan.dbias_stride, st));
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// Stage G: adjoint of PETBackend.preprocess. (dgeo [E,4], dfc_a + dfc_b [E]) -> dL/dR, dL/dcell
int backward_geometry(const Model& m, const Graph& g, Workspace& w, const float* dgeo, const float* dfc_a,
                      const float* dfc_b, float* gpos, float* gcell, hipStream_t st) {
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (E == 0) {  // isolated atoms: no position dependence at all
        PET_HIP_CHECK(hipMemsetAsync(gpos, 0, N * 3 * sizeof(float), st));
        if (gcell) PET_HIP_CHECK(hipMemsetAsync(gcell, 0, g.n_systems * 9 * sizeof(float), st));
        return PET_OK;
    }
    k_geom_bwd<<<cdiv(E, 256), 256, 0, st>>>(g.geo, g.d0, dgeo, dfc_a, dfc_b, reinterpret_cast<float4*>(w.dv), E,
                                             m.h.cutoff, m.h.cutoff_width, m.h.cutoff_function,
                                             g.adaptive ? g.pc : nullptr, g.adaptive ? g.ad_gc : nullptr);
    k_pos_grad<<<cdiv(N, 16), 256, 0, st>>>(reinterpret_cast<const float4*>(w.dv), g.rowptr, g.rev, gpos, (int)N);
    if (gcell)
        k_cell_grad<<<(int)g.n_systems, 256, 0, st>>>(reinterpret_cast<const float4*>(w.dv), g.shift, g.ctr, g.sys,
                                                      g.rowptr, gcell, (int)N, E, 0);
    if (g.adaptive) {
        k_adapt_gr<<<cdiv(N, 16), 256, 0, st>>>(g.ad_gc, g.rowptr, g.rev, g.ad_gr, (int)N);
        if (g.grid_probes > 0)
            k_adapt_dv_grid<<<cdiv(N, 16), 256, 0, st>>>(g.rowptr0, g.perm0, g.vin, g.ad_gr, g.grid_drdn, g.ad_dv, (int)N,
                                                         m.h.cutoff_width_adaptive, g.grid_probes, 0.5f,
                                                         m.h.cutoff_width_adaptive / 4.0f);
        else
        k_adapt_dv<<<cdiv(N, 16), 256, 0, st>>>(g.rowptr0, g.perm0, g.vin, g.ad_gr, g.r_newton, g.inv_dn, g.ad_dv,
                                                (int)N, m.h.cutoff_width_adaptive);
        k_pos_grad_acc<<<cdiv(N, 16), 256, 0, st>>>(g.ad_dv, g.rowptr0, g.rev0, gpos, (int)N);
        if (gcell)  // the adaptive term reaches the cell through the shift vectors of ALL input edges
            k_cell_grad<<<(int)g.n_systems, 256, 0, st>>>(g.ad_dv, g.shift0, g.ctr, g.sys, g.rowptr0, gcell, (int)N,
                                                          g.n_edges_in, 1);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// Gn[i][c] = sum_p gA[i][p] Wn[p][c], Ge likewise with We, gb[i] = sum_p gA[i][p] be[p]
__global__ void k_last_bwd(const float* __restrict__ gA, const float* __restrict__ nw, const float* __restrict__ ew,
                           const float* __restrict__ eb, int P, float* __restrict__ Gn, float* __restrict__ Ge,
                           float* __restrict__ gbv, int n, int accumulate = 0) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n * DH) return;
    const int i = (int)(idx / DH), c = (int)(idx % DH);
    float a = 0.f, b = 0.f, s = 0.f;
    for (int p = 0; p < P; p++) {
        const float gv = gA[(int64_t)i * P + p];
        a = fmaf(gv, nw[(int64_t)p * DH + c], a);
        b = fmaf(gv, ew[(int64_t)p * DH + c], b);
        s = fmaf(gv, eb[p], s);
    }
    Gn[idx] = accumulate ? Gn[idx] + a : a;  // accumulate: the blocks of one target share its heads
    Ge[idx] = accumulate ? Ge[idx] + b : b;
    if (c == 0) gbv[i] = accumulate ? gbv[i] + s : s;
}

// adjoint of predict() (pet_fwd.hip) for the features the caller passes in
int predict_backward(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                     const float* edge_feat, const float* fc, const float* gA, float* g_node, float* g_edge, float* g_fc,
                     float* scratch, hipStream_t st) {
    if (m.generic()) return gen_predict_backward(m, g, H, Lw, node_feat, edge_feat, fc, gA, g_node, g_edge, g_fc, st);
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (N == 0) return PET_OK;
    float* Gn = scratch;
    float* Ge = scratch + N * DH;
    float* gbv = Ge + N * DH;
    if (!fc) fc = g.fc;
    k_last_bwd<<<cdiv(N * DH, 256), 256, 0, st>>>(gA, Lw.nw, Lw.ew, Lw.eb, Lw.P, Gn, Ge, gbv, (int)N);
    PET_TRY(tile_head_bwd(false, node_feat, H.nh0, H.nh2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g_node, N, nullptr,
                          nullptr, nullptr, nullptr, Gn, gbv, st));
    if (E > 0)
        PET_TRY(tile_head_bwd(true, edge_feat, H.eh0, H.eh2, nullptr, nullptr, g.ctr, fc, nullptr, g_fc, g_edge, E, nullptr, nullptr,
                              nullptr, nullptr, Ge, gbv, st));
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// extra targets of a training step (non-conservative forces / stress, several blocks or properties): their predictions
// and adjoints read the features pet_forward(save_for_backward = 2) left in the training workspace (last.Hout /
// last.Mout), so a step runs ONE backbone forward and ONE backbone reverse sweep for all of its targets.
// ---------------------------------------------------------------------------------------------
// dst += src, float4 granularity
__global__ void k_add_seed(float4* __restrict__ dst, const float4* __restrict__ src, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = dst[i], b = src[i];
    dst[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
static void add_seed(float* dst, const float* src, int64_t n, hipStream_t st) {
    if (n > 0) k_add_seed<<<cdiv(n / 4, 256), 256, 0, st>>>(reinterpret_cast<float4*>(dst), reinterpret_cast<const float4*>(src), n / 4);
}

// the step runs on the size-generic training pass (other sizes, PostLN, residual, a dense atom, no edge): its forward left
// a generic workspace, read by gen_train_predict / gen_train_predict_backward
static int train_on_generic(const Model& m, const Graph& g, const void* ws, bool& gen) {
    gen = train_generic_for(m, g) || generic_workspace(g, ws);
    PET_REQUIRE(!gen || generic_workspace(g, ws), PET_ERR_ARGUMENT,
                "pet_forward with save_for_backward = 2 has not run on this workspace");
    return PET_OK;
}

static int train_workspace(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, Workspace& w) {
    PET_REQUIRE(layer == 0, PET_ERR_ARGUMENT, "the feedforward featuriser has one readout layer (0)");
    carve_workspace(m, g.n_nodes, g.n_edges, ws, w, true);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small for training");
    return PET_OK;
}

int train_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H, const LastW& Lw,
                  float* atomic, hipStream_t st) {
    bool gen;
    int rc = train_on_generic(m, g, ws, gen);
    if (rc) return rc;
    if (gen) return gen_train_predict(m, g, ws, ws_bytes, layer, H, Lw, atomic, st);
    Workspace w;
    rc = train_workspace(m, g, ws, ws_bytes, layer, w);
    if (rc || g.n_nodes == 0) return rc;
    PoolBuf scratch;
    PET_HIP_CHECK(scratch.alloc((size_t)predict_scratch_floats(g.n_nodes, g.n_edges) * sizeof(float), st));
    const GnnBufs& last = w.gnn.back();
    return predict(m, g, H, Lw, last.Hout, last.Mout, nullptr, atomic, nullptr, nullptr, scratch.as<float>(), st);
}

// dL/dtheta of one target's heads and of the last layers of `n_blocks` of its blocks (seeds gA[b] [N, P_b]) ADDED to the
// gradient slots; the adjoints of the heads' inputs ADDED to seed_node [N, DN] / seed_edge [E, D] (either may be NULL).
// The head MLPs run once per (target, layer): their hidden adjoint is the sum over the blocks (k_last_bwd).
int train_predict_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const std::string& target, int layer,
                           const HeadW& H, int n_blocks, const char* const* blocks, const LastW* const* Lw,
                           const float* const* gA, float* seed_node, float* seed_edge, hipStream_t st) {
    bool gen;
    int rc = train_on_generic(m, g, ws, gen);
    if (rc) return rc;
    if (gen) return gen_train_predict_backward(m, g, ws, ws_bytes, layer, H, n_blocks, Lw, gA, seed_node, seed_edge, st);
    Workspace w;
    rc = train_workspace(m, g, ws, ws_bytes, layer, w);
    if (rc || g.n_nodes == 0 || n_blocks == 0) return rc;
    PET_REQUIRE(m.grad_flat, PET_ERR_ARGUMENT, "pet_model_zero_grad has not been called");
    const int64_t N = g.n_nodes, E = g.n_edges;
    auto al = [](int64_t n) { return (n + 63) & ~(int64_t)63; };
    const int64_t nX = N * DN > E * D ? N * DN : E * D;
    PoolBuf scratch;  // Gn, Ge [N, DH] | gb [N] | input adjoint rows | dfc [E] (not wanted: fc has no parameter)
    PET_HIP_CHECK(scratch.alloc((size_t)(2 * al(N * DH) + al(N) + al(nX) + al(E)) * sizeof(float), st));
    float* Gn = scratch.as<float>();
    float* Ge = Gn + al(N * DH);
    float* gbv = Ge + al(N * DH);
    float* dX = gbv + al(N);
    float* dfc = dX + al(nX);
    for (int b = 0; b < n_blocks; b++)
        k_last_bwd<<<cdiv(N * DH, 256), 256, 0, st>>>(gA[b], Lw[b]->nw, Lw[b]->ew, Lw[b]->eb, Lw[b]->P, Gn, Ge, gbv, (int)N,
                                                       b > 0);
    Trainer tr{m, g, w, m.grad_flat, st};
    const std::string tl = target + "." + std::to_string(layer);
    const GnnBufs& last = w.gnn.back();
    {
        ProfScope ps("extra_head_node_bwd", st, (double)N * 2.0 * (DN * DH + 2 * DH * DH));
        PET_TRY(tile_head_bwd(false, last.Hout, H.nh0, H.nh2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dX, N, w.hs1,
                              w.hda2, w.hda1, w.hs2y, Gn, gbv, st));
        tr.head_linears("node_heads." + tl, last.Hout, DN, N);
        for (int b = 0; b < n_blocks; b++) tr.last_layer(false, "node_last_layers." + tl + "." + blocks[b], gA[b], Lw[b]->P, N);
        if (seed_node) add_seed(seed_node, dX, N * DN, st);
    }
    if (E > 0) {
        ProfScope ps("extra_head_edge_bwd", st, (double)E * 2.0 * (D * DH + 2 * DH * DH));
        PET_TRY(tile_head_bwd(true, last.Mout, H.eh0, H.eh2, nullptr, nullptr, g.ctr, g.fc, nullptr, dfc, dX, E, w.hs1, w.hda2,
                              w.hda1, w.hs2y, Ge, gbv, st));
        tr.head_linears("edge_heads." + tl, last.Mout, D, E);
        for (int b = 0; b < n_blocks; b++) tr.last_layer(true, "edge_last_layers." + tl + "." + blocks[b], gA[b], Lw[b]->P, E);
        if (seed_edge) add_seed(seed_edge, dX, E * D, st);
    }
    PET_HIP_CHECK(hipGetLastError());
    return tr.err;
}

#define PET_CARVE(w)                                                                      \
    Workspace w;                                                                          \
    carve_workspace(m, g.n_nodes, g.n_edges, ws, w);                                      \
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small")

static int d2d(void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes) PET_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return PET_OK;
}

int backward_predict_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA,
                         float* g_node, float* g_edge, float* g_fc, hipStream_t st) {
    if (use_generic(m, g) || generic_workspace(g, ws)) return gen_backward_predict(m, g, ws, ws_bytes, gA, g_node, g_edge, g_fc, st);
    PET_CARVE(w);
    if (g.n_nodes == 0) return PET_OK;
    int rc;
    if ((rc = backward_predict(m, g, w, gA, st))) return rc;
    if (g_node && (rc = d2d(g_node, w.dH, g.n_nodes * DN * sizeof(float), st))) return rc;
    if (g_edge && (rc = d2d(g_edge, w.dM, g.n_edges * D * sizeof(float), st))) return rc;
    if (g_fc && (rc = d2d(g_fc, w.dfc, g.n_edges * sizeof(float), st))) return rc;
    return PET_OK;
}

int backward_features_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_node,
                          const float* g_edge, float* g_geo, float* g_fc, hipStream_t st) {
    if (use_generic(m, g) || generic_workspace(g, ws)) return gen_backward_features(m, g, ws, ws_bytes, &g_node, &g_edge, 1, g_geo, g_fc, st);
    PET_CARVE(w);
    if (g.n_nodes == 0) return PET_OK;
    int rc;
    if ((rc = d2d(w.dH, g_node, g.n_nodes * DN * sizeof(float), st))) return rc;
    if ((rc = d2d(w.dM, g_edge, g.n_edges * D * sizeof(float), st))) return rc;
    if ((rc = backward_features(m, g, w, st))) return rc;
    if ((rc = d2d(g_geo, w.dgeo, g.n_edges * 4 * sizeof(float), st))) return rc;
    if ((rc = d2d(g_fc, w.dbias, g.n_edges * sizeof(float), st))) return rc;
    return PET_OK;
}

int backward_features_layers_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* const* g_node,
                                 const float* const* g_edge, int n_layers, float* g_geo, float* g_fc, hipStream_t st) {
    if (use_generic(m, g) || generic_workspace(g, ws)) return gen_backward_features(m, g, ws, ws_bytes, g_node, g_edge, n_layers, g_geo, g_fc, st);
    PET_CARVE(w);
    PET_REQUIRE(n_layers == m.num_readout_layers(), PET_ERR_ARGUMENT,
                "expected one gradient pair per readout layer (" + std::to_string(m.num_readout_layers()) + ")");
    if (g.n_nodes == 0) return PET_OK;
    int rc;
    if (!m.residual()) {
        if (g_node[0]) { if ((rc = d2d(w.dH, g_node[0], g.n_nodes * DN * sizeof(float), st))) return rc; }
        else PET_HIP_CHECK(hipMemsetAsync(w.dH, 0, g.n_nodes * DN * sizeof(float), st));
        if (g_edge[0]) { if ((rc = d2d(w.dM, g_edge[0], g.n_edges * D * sizeof(float), st))) return rc; }
        else if (g.n_edges) PET_HIP_CHECK(hipMemsetAsync(w.dM, 0, g.n_edges * D * sizeof(float), st));
        if ((rc = backward_features(m, g, w, st))) return rc;
    } else if ((rc = backward_features(m, g, w, st, nullptr, g_node, g_edge))) return rc;
    if ((rc = d2d(g_geo, w.dgeo, g.n_edges * 4 * sizeof(float), st))) return rc;
    if ((rc = d2d(g_fc, w.dbias, g.n_edges * sizeof(float), st))) return rc;
    return PET_OK;
}

int backward_geometry_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_geo,
                          const float* g_fc, float* gpos, float* gcell, hipStream_t st) {
    if (use_generic(m, g) || generic_workspace(g, ws)) return gen_backward_geometry(m, g, ws, ws_bytes, g_geo, g_fc, gpos, gcell, st);
    PET_CARVE(w);
    if (g.n_nodes == 0) return PET_OK;
    return backward_geometry(m, g, w, g_geo, g_fc, nullptr, gpos, gcell, st);
}

// preprocess^T on its own: only the d/d(edge vector) buffer is needed, not a forward workspace
int geometry_backward(const Model& m, const Graph& g, const float* g_geo, const float* g_fc, float* gpos, float* gcell,
                      float* scratch, hipStream_t st) {
    Workspace w;
    w.dv = scratch;
    if (g.n_nodes == 0) return PET_OK;
    return backward_geometry(m, g, w, g_geo, g_fc, nullptr, gpos, gcell, st);
}

// shared by the size-generic path (gen.hip): only the d/d(edge vector) buffer is needed
int backward_geometry_generic(const Model& m, const Graph& g, float* dv_scratch, const float* dgeo, const float* dfc_a,
                              const float* dfc_b, float* gpos, float* gcell, hipStream_t st) {
    Workspace w;
    w.dv = dv_scratch;
    return backward_geometry(m, g, w, dgeo, dfc_a, dfc_b, gpos, gcell, st);
}

int backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* gpos,
             float* gcell, hipStream_t st) {
    if (use_generic(m, g) || generic_workspace(g, ws)) return gen_backward(m, g, ws, ws_bytes, gA, gpos, gcell, st);
    Workspace w;
    carve_workspace(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small");
    if (g.n_nodes == 0) return PET_OK;
    int rc;
    if (g.n_edges > 0) {
        if ((rc = backward_predict(m, g, w, gA, st))) return rc;
        if ((rc = backward_features(m, g, w, st))) return rc;
    }
    return backward_geometry(m, g, w, w.dgeo, w.dfc, w.dbias, gpos, gcell, st);
}

// Training reverse pass (energy term): dL/dtheta accumulated into the model's flat gradient
// buffer for the seeds gA = dL/d(atomic prediction), plus dL/dR (and dL/dcell) when requested.
// Needs a forward run with save_for_backward = 2 on a training workspace.
// seed_node / seed_edge [n_seed] (NULL entries = 0): feature adjoints of further targets (train_predict_backward), added
// where the fused head's adjoint enters the backbone; gA may then be NULL (no fused target in the loss).
int backward_train(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* gpos,
                   float* gcell, hipStream_t st, const float* const* seed_node, const float* const* seed_edge, int n_seed) {
    const float* sn = n_seed > 0 && seed_node ? seed_node[0] : nullptr;
    const float* se = n_seed > 0 && seed_edge ? seed_edge[0] : nullptr;
    // other sizes, PostLN, residual, and any graph with an atom of more than 127 neighbours: the first-order terms alone = the
    // size-generic second-order pass without a tangent
    if (train_generic_for(m, g)) {
        PET_REQUIRE(generic_workspace(g, ws), PET_ERR_ARGUMENT, "pet_forward with save_for_backward = 2 has not run on this workspace");
        PET_REQUIRE(n_seed == 0 || n_seed == m.num_readout_layers(), PET_ERR_ARGUMENT, "expected one seed pair per readout layer");
        bool seeded = false;
        for (int l = 0; l < n_seed; l++) seeded = seeded || (seed_node && seed_node[l]) || (seed_edge && seed_edge[l]);
        PET_REQUIRE(!(gpos || gcell) || !seeded, PET_ERR_UNSUPPORTED,
                    "d_grad_positions / d_grad_cells with feature seeds: the further targets' cutoff-factor adjoint is not "
                    "carried; ask for the parameter gradients only");
        PET_REQUIRE(gA || !(gpos || gcell), PET_ERR_ARGUMENT, "d_grad_positions needs d_grad_atomic (the fused target's seeds)");
        // (the energy-only step has no second-order workspace of its own in the ABI: the dual activations come from the
        // stream's pool and go back to it on every exit)
        const int64_t n2 = gen_train_workspace_bytes(m, g.n_nodes, g.n_edges);
        PoolBuf ws2_pool;
        PET_HIP_CHECK(ws2_pool.alloc((size_t)n2, st));
        void* ws2 = ws2_pool.p;
        int rc = gen_train2(m, g, ws2, n2, nullptr, gA, nullptr, nullptr, nullptr, st, seed_node, seed_edge, n_seed);
        if (!rc && gpos) rc = gen_backward(m, g, ws, ws_bytes, gA, gpos, gcell, st);
        return rc;
    }
    PET_REQUIRE(m.grad_flat, PET_ERR_ARGUMENT, "pet_model_zero_grad has not been called");
    Workspace w;
    carve_workspace(m, g.n_nodes, g.n_edges, ws, w, true);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small for training");
    if (g.n_nodes == 0) return PET_OK;
    PET_REQUIRE(g.n_edges > 0, PET_ERR_UNSUPPORTED, "training on a batch without any edge is not supported");
    PET_REQUIRE(n_seed == 0 || n_seed == m.num_readout_layers(), PET_ERR_ARGUMENT, "expected one seed pair per readout layer");
    // the seeds carry the further targets' feature adjoints only, not their cutoff-factor adjoint (d fc / dR): dL/dR and
    // dL/dcell of such a loss would be incomplete
    PET_REQUIRE(!(gpos || gcell) || !(sn || se), PET_ERR_UNSUPPORTED,
                "d_grad_positions / d_grad_cells with feature seeds: the further targets' cutoff-factor adjoint is not "
                "carried; ask for the parameter gradients only");
    Trainer tr{m, g, w, m.grad_flat, st};
    int rc;
    if (gA) {
        PET_REQUIRE(m.has_fused_head, PET_ERR_ARGUMENT, "d_grad_atomic needs the fused single-property target");
        if ((rc = backward_predict(m, g, w, gA, st, &tr))) return rc;
    } else {
        PET_HIP_CHECK(hipMemsetAsync(w.dH, 0, g.n_nodes * DN * sizeof(float), st));
        PET_HIP_CHECK(hipMemsetAsync(w.dM, 0, g.n_edges * D * sizeof(float), st));
        PET_HIP_CHECK(hipMemsetAsync(w.dfc, 0, g.n_edges * sizeof(float), st));
    }
    if (sn) add_seed(w.dH, sn, g.n_nodes * DN, st);
    if (se) add_seed(w.dM, se, g.n_edges * D, st);
    if (!gpos && !tr.backbone_live()) return tr.err;  // only heads / last layers train
    if ((rc = backward_features(m, g, w, st, &tr))) return rc;
    if (tr.err) return tr.err;
    if (gpos) return backward_geometry(m, g, w, w.dgeo, w.dfc, w.dbias, gpos, gcell, st);
    return PET_OK;
}

}  // namespace pet
