// Size-generic PET path: forward + hand-written reverse pass (dE/dR) for ANY (d_pet, d_node, d_feedforward, d_head,
// num_heads) -- the reference is size-generic (pet/documentation.py:196-213; its own architecture suites run at
// d_pet = 1, pet/tests/test_basic.py:22-32) while the tuned kernels of pet_fwd / pet_trr / pet_attn / pet_comb are ONE
// compiled instantiation (128 / 256 / 256 / 128 / 8). A model of any other size runs here, behind the same C ABI:
//
//   * every Linear is one GEMM kernel over the RAW torch weights [n_out, k_in] on the fp32 matrix core (k_gen_lin:
//     v_mfma_f32_32x32x2_f32, 64 x 64 output tiles, K chunks of 32 through LDS, run-time bounds everywhere), the adjoint
//     dX = dY W is the same kernel with swapped strides;
//   * norms / SwiGLU / SiLU are row kernels with a run-time width (one wave per row);
//   * attention is one wave per (atom, head): a lane is (query | key, 16-feature slice) -- queries for the forward and dQ, keys
//     for dK, dV and the key-bias gradient -- and walks the other index with an online soft-max, so any head dimension up
//     to 128 and ANY number of neighbours is served (no 16-token tiles); dot products are xor-shuffle sums over the slices:
//     fixed summation order, bit-reproducible;
//   * d_node == d_pet follows transformer.py:189-201: no centre contraction / expansion / centre MLP, the node features
//     leaving a layer ARE the centre token;
//   * all architecture switches of the tuned path: RMSNorm / LayerNorm, PreLN / PostLN, feedforward / residual featuriser,
//     SwiGLU / SiLU (tied halves), system conditioning, bump / cosine / adaptive cutoffs (graph side, shared).
// Correctness-first: fp32 products throughout (no split operands, no tuned tiles); rates in DESIGN.md section 1.
// Training on this path: gen_train.hip.
#include <string>
#include <vector>

#include "gen_walk.h"

namespace pet {

int attn_tiles(const Graph& g);
int backward_geometry_generic(const Model& m, const Graph& g, float* dv_scratch, const float* dgeo, const float* dfc_a,
                              const float* dfc_b, float* gpos, float* gcell, hipStream_t st);  // pet_bwd.hip


int64_t gen_workspace_bytes(const Model& m, int64_t N, int64_t E) {
    GWs w;
    gen_carve(m, N, E, nullptr, w);
    return (int64_t)w.bytes;
}

// ---------------------------------------------------------------------------------------------
// the primal pass of gen_walk.h on a forward workspace: inference and its reverse (dE/d geometry)
// ---------------------------------------------------------------------------------------------
namespace {
struct Infer : Ops {
    GWs& w;
    Roles<float*> s;
    const float* geo;
    const float* const* g_node = nullptr;   // reverse: the read-out adjoints per layer (null = zero) and the two sinks
    const float* const* g_edge = nullptr;
    float *g_geo = nullptr, *g_fc = nullptr;
    Infer(const Model& m_, const Graph& g_, hipStream_t st_, GWs& w_)
        : Ops(m_, g_, st_), w(w_), geo(reinterpret_cast<const float*>(g_.geo)) {
        s.normed = w.tE1; s.OUT = w.tE2; s.act = w.tE3; s.nNormed = w.tN1; s.nAct = w.tN2;
        s.dAO = w.tE1; s.dOUT = w.tE2; s.dXin = w.tE3; s.dVG = w.tE4;
        s.dH1 = w.tN1; s.nA = w.tN2; s.nB = w.tN3; s.dTOKo = w.tN3;
        // s.re / s.nRe stay null: only the recompute hooks and the weight gradients read them, and this pass has neither.
        // A hook that becomes non-empty here needs them carved first.
    }
    void attn(const GAttn& A) const {
        attn_dispatch(d.HD, [&](auto hdm) {
            k_gen_attn_fwd<decltype(hdm)::value><<<dim3((unsigned)N, (unsigned)d.NH), 64, 0, st>>>(
                A.QKV, g.rowptr, g.fc, A.AO, A.LSE, E, d.D, d.NH, d.HD, scale);
        });
    }
    void add_cond(float* H) const { k_gen_add_cond<<<g1(N * d.DN), 256, 0, st>>>(H, w.cond, g.sys, g.cond_sys, N, d.DN); }
    void attn_rev(const GAttn& A, const float* dAO) const {
        attn_dispatch(d.HD, [&](auto hdm) {
            constexpr int HDM = decltype(hdm)::value;
            k_gen_attn_bwd_q<HDM><<<dim3((unsigned)N, (unsigned)d.NH), 64, 0, st>>>(
                A.QKV, A.AO, dAO, A.LSE, g.rowptr, g.fc, w.dQKV, w.DELTA, E, d.D, d.NH, d.HD, scale);
            k_gen_attn_bwd_k<HDM><<<dim3((unsigned)N, (unsigned)d.NH), 64, 0, st>>>(
                A.QKV, dAO, A.LSE, w.DELTA, g.rowptr, g.fc, w.dQKV, w.dbias_h, E, d.D, d.NH, d.HD, scale);
        });
    }
    void key_bias_sink(bool) const { if (E > 0) k_gen_dfc<<<g1(E), 256, 0, st>>>(w.dbias_h, g.fc, g_fc, E, d.NH); }
    void geo_sink(const float* dTOK, int kin, const Lin& eemb, bool) const { lin.bwd(dTOK, kin, eemb, g_geo, 4, E, true); }
    void cond_accum(const float*, bool) const {}
    void seed(int l, float* dH, float* dE) const {
        if (g_node[l]) copy(g_node[l], dH, N, d.DN); else zero(dH, N * d.DN);
        if (g_edge[l]) copy(g_edge[l], dE, E, d.D); else zero(dE, E * d.D);
    }
};
}  // namespace

// ---------------------------------------------------------------------------------------------
// predict (a function of the features it is given) and its adjoint
// ---------------------------------------------------------------------------------------------
int gen_predict(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                const float* edge_feat, const float* fc, float* atomic, float* node_hidden, float* edge_hidden,
                hipStream_t st) {
    Ops o(m, g, st);
    const int64_t N = o.N, E = o.E;
    if (N == 0) return PET_OK;
    const int DH = o.d.DH, P = Lw.P;
    if (!fc) fc = g.fc;
    // (the caller's scratch is sized for the compiled instantiation: this path takes its own from the stream's pool)
    const int64_t need = 4 * (N + E + 2) * (int64_t)DH + (N + E + 2) * (int64_t)P;
    float* scratch = nullptr;
    PoolBuf scratch_pool;
    PET_HIP_CHECK(scratch_pool.alloc((size_t)need * sizeof(float), st));
    scratch = scratch_pool.as<float>();
    float* a1n = scratch; float* s1n = a1n + N * DH; float* a2n = s1n + N * DH; float* s2n = a2n + N * DH;
    float* a1e = s2n + N * DH; float* s1e = a1e + E * DH; float* a2e = s1e + E * DH; float* s2e = a2e + E * DH;
    float* np = s2e + E * DH; float* ep = np + N * P;
    gen_head(o, H.nh0, H.nh2, node_feat, o.d.DN, N, a1n, s1n, a2n, s2n);
    Lin ln; ln.w = Lw.nw; ln.b = Lw.nb; ln.n_out = P; ln.k_in = DH;
    o.lin.fwd(s2n, DH, ln, np, P, N);
    if (E > 0) {
        gen_head(o, H.eh0, H.eh2, edge_feat, o.d.D, E, a1e, s1e, a2e, s2e);
        Lin le; le.w = Lw.ew; le.b = Lw.eb; le.n_out = P; le.k_in = DH;
        o.lin.fwd(s2e, DH, le, ep, P, E);
    }
    k_gen_atom_sum<<<g1(N * P), 256, 0, st>>>(np, ep, fc, g.rowptr, atomic, N, P);
    if (node_hidden) o.copy(s2n, node_hidden, N, DH);
    if (edge_hidden && E > 0) o.copy(s2e, edge_hidden, E, DH);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int gen_predict_backward(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                         const float* edge_feat, const float* fc, const float* gA, float* g_node, float* g_edge, float* g_fc,
                         hipStream_t st) {
    Ops o(m, g, st);
    const int64_t N = o.N, E = o.E;
    if (N == 0) return PET_OK;
    const int DH = o.d.DH, P = Lw.P;
    if (!fc) fc = g.fc;
    const int64_t M = N > E ? N : E;
    float* scratch = nullptr;
    PoolBuf scratch_pool;
    PET_HIP_CHECK(scratch_pool.alloc((size_t)(4 * M * DH + 2 * M * P) * sizeof(float), st));
    scratch = scratch_pool.as<float>();
    float* a1 = scratch; float* s1 = a1 + M * DH; float* a2 = s1 + M * DH; float* s2 = a2 + M * DH;
    float* pr = s2 + M * DH; float* dpr = pr + M * P;
    // node branch (recomputed from the features: nothing is read from a forward workspace)
    gen_head(o, H.nh0, H.nh2, node_feat, o.d.DN, N, a1, s1, a2, s2);
    Lin ln; ln.w = Lw.nw; ln.b = Lw.nb; ln.n_out = P; ln.k_in = DH;
    o.lin.bwd(gA, P, ln, s2, DH, N);                                                   // d s2
    k_gen_silu_bwd<<<g1(N * DH), 256, 0, st>>>(a2, s2, s2, N * DH);                    // d a2
    o.lin.bwd(s2, DH, H.nh2, s1, DH, N);                                               // d s1
    k_gen_silu_bwd<<<g1(N * DH), 256, 0, st>>>(a1, s1, s1, N * DH);                    // d a1
    o.lin.bwd(s1, DH, H.nh0, g_node, o.d.DN, N);
    if (E > 0) {
        gen_head(o, H.eh0, H.eh2, edge_feat, o.d.D, E, a1, s1, a2, s2);
        Lin le; le.w = Lw.ew; le.b = Lw.eb; le.n_out = P; le.k_in = DH;
        o.lin.fwd(s2, DH, le, pr, P, E);
        k_gen_edge_seed<<<g1(E), 256, 0, st>>>(gA, g.ctr, fc, pr, dpr, g_fc, 0, E, P);
        o.lin.bwd(dpr, P, le, s2, DH, E);
        k_gen_silu_bwd<<<g1(E * DH), 256, 0, st>>>(a2, s2, s2, E * DH);
        o.lin.bwd(s2, DH, H.eh2, s1, DH, E);
        k_gen_silu_bwd<<<g1(E * DH), 256, 0, st>>>(a1, s1, s1, E * DH);
        o.lin.bwd(s1, DH, H.eh0, g_edge, o.d.D, E);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int gen_aux_outputs(const Model& m, const Graph& g, const float* node_feat, const float* edge_feat, float* feature,
                    float* last_layer, float* scratch, hipStream_t st) {
    Ops o(m, g, st);
    const int64_t N = o.N, E = o.E;
    const GD& d = o.d;
    if (N == 0) return PET_OK;
    if (feature) {
        o.axpby(1.f, node_feat, d.DN, 0.f, nullptr, 0, nullptr, feature, d.DN + d.D, false, N, d.DN);
        k_gen_edge_sum<<<g1(N * d.D), 256, 0, st>>>(edge_feat, g.fc, g.rowptr, feature + d.DN, d.DN + d.D, N, d.D);
    }
    if (last_layer) {
        PET_REQUIRE(m.has_fused_head, PET_ERR_ARGUMENT, "last-layer features need the fused target's heads");
        const int64_t M = N > E ? N : E;
        (void)scratch;  // sized for the compiled instantiation: this path takes its temporaries from the stream's pool
        PoolBuf tmp_pool;
        PET_HIP_CHECK(tmp_pool.alloc((size_t)4 * M * d.DH * sizeof(float), st));
        float* tmp = tmp_pool.as<float>();
        float* b1 = tmp; float* b2 = b1 + M * d.DH; float* b3 = b2 + M * d.DH; float* b4 = b3 + M * d.DH;
        gen_head(o, m.nh0, m.nh2, node_feat, d.DN, N, b1, b2, b3, b4);
        o.axpby(1.f, b4, d.DH, 0.f, nullptr, 0, nullptr, last_layer, 2 * d.DH, false, N, d.DH);
        if (E > 0) {
            gen_head(o, m.eh0, m.eh2, edge_feat, d.D, E, b1, b2, b3, b4);
            k_gen_edge_sum<<<g1(N * d.DH), 256, 0, st>>>(b4, g.fc, g.rowptr, last_layer + d.DH, 2 * d.DH, N, d.DH);
        } else
            o.axpby(0.f, b4, d.DH, 0.f, nullptr, 0, nullptr, last_layer + d.DH, 2 * d.DH, false, N, d.DH);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// forward (backend.py:496-649)
// ---------------------------------------------------------------------------------------------
int gen_forward_layers(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int, float* atomic,
                       float* const* node_feats, float* const* edge_feats, int n_layers, hipStream_t st) {
    // (no `save` switch: everything the reverse passes need is kept anyway; the training pass, gen_train.hip, recomputes)
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT,
                "forward workspace too small for the size-generic path (other model sizes, or an atom with more than 127 "
                "neighbours): size it with pet_forward_workspace_bytes_for(model, graph)");
    const bool res = m.residual();
    PET_REQUIRE(res ? (n_layers == m.h.num_gnn_layers || (n_layers == 1 && !node_feats[0] && !edge_feats[0])) : n_layers == 1,
                PET_ERR_ARGUMENT, "expected one feature pair per readout layer");
    Infer p(m, g, st, w);
    const int64_t N = p.N, E = p.E;
    if (N == 0) return PET_OK;
    const int D = p.d.D, DN = p.d.DN;
    if (m.h.system_conditioning) {
        PET_REQUIRE(g.cond_charge && g.n_cond_systems >= 1 && g.n_cond_systems <= N, PET_ERR_ARGUMENT,
                    "system_conditioning: call pet_graph_set_conditioning (charge, spin multiplicity, system indices) first");
        k_gen_system_cond<<<(int)g.n_cond_systems, 128, 3 * DN * sizeof(float), st>>>(
            g.cond_charge, g.cond_spin, m.cond_qe, m.cond_se, m.cond_w0, m.cond_b0, m.cond_w2, m.cond_b2, w.cond,
            m.h.max_charge, DN);
    }
    gen_walk_forward(p, w);
    const GGnn& last = w.gnn.back();
    if (atomic) {
        // the fused single-property target; with the residual featuriser the sum over the readout layers (backend.py:468-481)
        const int NR = m.num_readout_layers();
        PoolBuf tmp_pool;
        if (NR > 1) PET_HIP_CHECK(tmp_pool.alloc((size_t)N * sizeof(float), st));
        float* tmp = tmp_pool.as<float>();
        for (int l = 0; l < NR; l++) {
            const HeadW* H;
            const LastW* Lw;
            int rc = fused_heads(m, l, H, Lw, "pet_forward with d_atomic needs the fused single-property target (of every readout "
                                              "layer); use pet_predict for other heads");
            if (rc) return rc;
            const GGnn& Bl = res ? w.gnn[l] : last;
            rc = gen_predict(m, g, *H, *Lw, Bl.Hout, res ? Bl.XF : Bl.Mout, g.fc, l == 0 ? atomic : tmp, nullptr, nullptr, st);
            if (rc) return rc;
            if (l > 0) p.add(tmp, atomic, N, 1);
        }
    }
    for (int l = 0; l < n_layers; l++) {
        const GGnn& Bl = res ? w.gnn[l] : last;
        if (node_feats[l])
            PET_HIP_CHECK(hipMemcpyAsync(node_feats[l], Bl.Hout, N * DN * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (edge_feats[l] && E > 0)
            PET_HIP_CHECK(hipMemcpyAsync(edge_feats[l], res ? Bl.XF : Bl.Mout, E * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// reverse pass of the features: (dL/d node features, dL/d edge features) of every readout layer -> dL/d geometry [E,4],
// dL/d cutoff factors [E] (the attention key biases)
// ---------------------------------------------------------------------------------------------
int gen_backward_features(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* const* g_node,
                          const float* const* g_edge, int n_layers, float* g_geo, float* g_fc, hipStream_t st) {
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small");
    PET_REQUIRE(n_layers == m.num_readout_layers(), PET_ERR_ARGUMENT, "expected one gradient pair per readout layer");
    Infer p(m, g, st, w);
    if (p.N == 0) return PET_OK;
    p.g_node = g_node; p.g_edge = g_edge; p.g_geo = g_geo; p.g_fc = g_fc;
    p.zero(g_geo, p.E * 4);
    p.zero(g_fc, p.E);
    gen_walk_reverse(p, w);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// staged pieces the C ABI exposes (features and their adjoints live in the workspace between the calls)
int gen_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* gpos, float* gcell,
                 hipStream_t st) {
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small");
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (N == 0) return PET_OK;
    const GD d = dims_of(m);
    const int NR = m.num_readout_layers();
    const bool res = m.residual();
    const int64_t Ea = E > 0 ? E : 1;
    float* buf = nullptr;   // per readout layer: d node features, d edge features; then d fc (heads, summed), scratch d fc, d geo, d fc (attention)
    const size_t per = (size_t)N * d.DN + (size_t)Ea * d.D;
    PoolBuf buf_pool;
    PET_HIP_CHECK(buf_pool.alloc((per * NR + (size_t)Ea * 7) * sizeof(float), st));
    buf = buf_pool.as<float>();
    float* gfh = buf + per * NR;
    float* gft = gfh + Ea;
    float* ggeo = gft + Ea;
    float* gfc = ggeo + Ea * 4;
    std::vector<const float*> gnp(NR), gep(NR);
    int rc = PET_OK;
    for (int l = 0; l < NR && !rc; l++) {
        const HeadW* H;
        const LastW* Lw;
        if ((rc = fused_heads(m, l, H, Lw, "pet_backward needs the fused single-property target (of every readout layer)"))) return rc;
        const GGnn& Bl = res ? w.gnn[l] : w.gnn.back();
        float* gn = buf + per * l;
        float* ge = gn + (size_t)N * d.DN;
        gnp[l] = gn; gep[l] = ge;
        rc = gen_predict_backward(m, g, *H, *Lw, Bl.Hout, res ? Bl.XF : Bl.Mout, g.fc, gA, gn, ge, l == 0 ? gfh : gft, st);
        if (!rc && l > 0 && E > 0) { Ops o(m, g, st); o.add(gft, gfh, E, 1); }
    }
    if (!rc) rc = gen_backward_features(m, g, ws, ws_bytes, gnp.data(), gep.data(), NR, ggeo, gfc, st);
    // the two cutoff-factor gradients (heads, attention key biases) are added by the geometry kernel
    if (!rc) rc = backward_geometry_generic(m, g, w.dv, ggeo, E > 0 ? gfh : nullptr, E > 0 ? gfc : nullptr, gpos, gcell, st);
    return rc;
}

// staged adjoint of the fused head on the features the forward left in the workspace (pet_backward_predict)
int gen_backward_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* g_node,
                         float* g_edge, float* g_fc, hipStream_t st) {
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small");
    PET_REQUIRE(!m.residual() && m.has_fused_head, PET_ERR_ARGUMENT, "pet_backward_predict needs the fused single-property target");
    if (g.n_nodes == 0) return PET_OK;
    const GD d = dims_of(m);
    HeadW H; H.nh0 = m.nh0; H.nh2 = m.nh2; H.eh0 = m.eh0; H.eh2 = m.eh2;
    const GGnn& last = w.gnn.back();
    const int64_t Ea = g.n_edges > 0 ? g.n_edges : 1;
    float* tmp = nullptr;   // outputs the caller did not ask for
    PoolBuf tmp_pool;
    PET_HIP_CHECK(tmp_pool.alloc((size_t)(g.n_nodes * d.DN + Ea * d.D + Ea) * sizeof(float), st));
    tmp = tmp_pool.as<float>();
    int rc = gen_predict_backward(m, g, H, m.lasts.at("@|0|@"), last.Hout, last.Mout, g.fc, gA, g_node ? g_node : tmp,
                                  g_edge ? g_edge : tmp + g.n_nodes * d.DN, g_fc ? g_fc : tmp + g.n_nodes * d.DN + Ea * d.D, st);
    return rc;
}

// prediction of one (target, readout layer, block) of a training step from the features the forward left in the workspace
// (pet_train_predict): the readout layer's node features, and its edge features -- the last layer's messages, or with the
// residual featuriser the layer's own edge tokens
int gen_train_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H, const LastW& Lw,
                      float* atomic, hipStream_t st) {
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small for training");
    PET_REQUIRE(layer >= 0 && layer < m.num_readout_layers(), PET_ERR_ARGUMENT, "readout layer out of range");
    if (g.n_nodes == 0) return PET_OK;
    const bool res = m.residual();
    const GGnn& Bl = res ? w.gnn[layer] : w.gnn.back();
    return gen_predict(m, g, H, Lw, Bl.Hout, res ? Bl.XF : Bl.Mout, g.fc, atomic, nullptr, nullptr, st);
}

int gen_backward_geometry(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_geo, const float* g_fc,
                          float* gpos, float* gcell, hipStream_t st) {
    GWs w;
    gen_carve(m, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "workspace too small");
    if (g.n_nodes == 0) return PET_OK;
    return backward_geometry_generic(m, g, w.dv, g_geo, g_fc, nullptr, gpos, gcell, st);
}

}  // namespace pet
