// The plan of the tuned first-order pass (pet_plan.h): every policy of every stage, forward and adjoint, in this file.
#include "pet_plan.h"

#include "common.h"
#include "model.h"

namespace pet {

// ---- policy ----------------------------------------------------------------------------------------------------------
// (the ring kernels' row policy: switches.h ring_serves)
// the node chain's Linear layers as k_rowlin_s: large graphs (below, the 32-row node kernels fuse two of the three), or forced
static bool ring_center_serves(int64_t N) {
    return ring_serves((int64_t)1 << 40) && (N >= NODE_ROWS32_MAX_ATOMS || switches().emlp_s_rows < EMLP_S_MIN_ROWS);
}
// the forward leaves [v; g] unsaved and the ring adjoint recomputes it
static bool emlp_recompute_on(const Lin& win, const Lin& wout, int64_t E) {
    return ring_serves(E) && win.fwd2s && wout.fwd2s && wout.bwd2s;
}
// whether this graph's attention layers run the fused block
static bool ablk_serves(const Graph& g) {
    if (g.bucket_start[5] > g.bucket_start[4]) return false;  // an atom of more than 64 tokens
    if (!g.tiles_planned) return false;                       // a small graph built before the block was forced
    if (switches().attn_fused & 4) return true;
    // A tile is one wave's serial chain (40 us forward, 100 us adjoint): below a few waves per SIMD the launch costs that
    // latency whatever its size, and the three row-parallel kernels are quicker (one box, three-kernel / fused ms per step:
    // 1 000 atoms 1.69 / 2.18, 3 000: 2.96 / 3.29, 5 000: 4.16 / 4.08, 10 000: 7.30 / 6.72; ABLK_MIN_TILES). Many
    // 64-slot tiles (the adjoint's instantiation for them spills): likewise.
    return g.n_tiles1 >= ABLK_MIN_TILES && (int64_t)g.n_tiles2 * 20 <= g.n_nodes;
}
static bool ablk_bwd_on(const Graph& g) { return (switches().attn_fused & 2) && ablk_serves(g); }
// k_node2 / k_node_bwd2: 64 rows per workgroup on large graphs (node_planes = 2 forces 32, the tests' route to those kernels);
// the 32-row form split over four workgroups when the tiles are few and the partial outputs with the tiles' arrival counters
// fit the scratch buffer of `cap` floats
static Node node_planes_form(int64_t N, size_t cap) {
    if (switches().node_planes != 2 && N > NODE_ROWS32_MAX_ATOMS) return Node::Rows64;
    const int nt32 = cdiv(N, 32);
    const size_t p_floats = (size_t)(DNF / 128) * nt32 * 32 * DN;
    return switches().node_split && nt32 <= NODE_SPLIT_MAX_TILES && p_floats + nt32 <= cap ? Node::Split : Node::Rows32;
}

bool StagePlan::unsaved_attn() const {
    for (const GnnPlan& G : gnn)
        for (const LayerPlan& A : G.layers)
            if (A.attn == Attn::Fused) return true;
    return false;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
StagePlan plan_forward(const Model& m, const Graph& g, int save) {
    const Switches& sw = switches();
    const int64_t N = g.n_nodes, E = g.n_edges, R = E + N;
    const int L = m.h.num_gnn_layers, AL = m.h.num_attention_layers;
    StagePlan p;
    p.gnn.assign(L, GnnPlan{Rows::LdsTile, Rows::Pipelined, std::vector<LayerPlan>(AL)});
    const bool trr = use_trr();
    const bool trr_l = trr && m.plain_layers();  // the TRR transformer-layer kernels are PreLN (RMSNorm or LayerNorm)
    const bool conditioned = m.h.system_conditioning != 0, res = m.residual();
    p.attn_preload = trr;
    p.side = p.side_heads = side_stream().enabled && !m.post_ln();  // PostLN: the node update needs the MLP output of the centre token, one chain
    // Training keeps the three-kernel attention (its second-order pass reads the saved QKV and AO); a forward whose adjoint
    // could not run fused keeps it too
    const bool fused_ok = trr_l && save != 2 && E > 0 && (save == 0 || ablk_bwd_on(g)) && (sw.attn_fused & 1) && ablk_serves(g);
    const bool center_ring = save != 2 && ring_center_serves(N);
    for (int gi = 0; gi < L; gi++) {
        const GnnLayerW& G = m.gnn[gi];
        GnnPlan& P = p.gnn[gi];
        if (trr && (sw.trr_compress & 1) && G.compress2.fwd2 && (gi == 0 || G.compress0_msg.fwd2) && E > 0) P.compress = Rows::Pipelined;
        if (G.comb0.fwd2 && G.comb2.fwd2 && ring_serves(E) && G.comb0_g.fwd2s && G.comb2.fwd2s) P.comb = Rows::Ring;
        for (int a = 0; a < AL; a++) {
            const AttnLayerW& A = G.attn[a];
            LayerPlan& Q = P.layers[a];
            Q.attn = fused_ok && A.qkv.fwd2s && A.out.fwd2s ? Attn::Fused : trr_l ? Attn::Pipelined : Attn::LdsTile;
            if (trr_l) {
                Q.emlp = ring_serves(E) && A.mlp_in.fwd2s && A.mlp_out.fwd2s ? Rows::Ring : Rows::Pipelined;
                // [v; g] is stored for the adjoint unless none follows or the adjoint recomputes it
                Q.emlp_saved = save != 0 && !(save == 1 && emlp_recompute_on(A.mlp_in, A.mlp_out, E));
            } else {
                Q.emlp_saved = save != 0;
            }
            // large graphs: three ring GEMMs that can run BESIDE the edge MLP; their scratch lives in dQKV (R * 3 D floats),
            // which only the adjoint uses -- as do the partial outputs of the split form
            if (sw.node_planes && (size_t)N * DNF <= (size_t)R * 3 * D && ring_serves(N) && A.ce.fwd2s && A.cmlp_in.fwd2s &&
                A.cmlp_out.fwd2s && N > 0)
                Q.node = Node::Ring;
            else if (sw.node_planes && A.cmlp_in.fwd2 && A.ce.fwd2 && A.cmlp_out.fwd2)
                Q.node = node_planes_form(N, (size_t)R * 3 * D);
            // the centre tokens of the NEXT layer in the node kernel's launch when they are center_contraction(Hn) as it leaves
            // that kernel: not behind the conditioning add, not into a residual GNN layer (its own embedding), f16x3 weights,
            // 32-row kernels (large graphs: k_center is quicker)
            if (a + 1 < AL || gi + 1 < L) {
                const AttnLayerW& An = a + 1 < AL ? G.attn[a + 1] : m.gnn[gi + 1].attn[0];
                LayerPlan& Qn = a + 1 < AL ? P.layers[a + 1] : p.gnn[gi + 1].layers[0];
                const bool by_node = (Q.node == Node::Split || Q.node == Node::Rows32) && sw.center_fused &&
                                     !(a + 1 == AL && (conditioned || res)) && An.cc.fwd2;
                Qn.center = by_node ? Center::ByNode : center_ring && An.cc.fwd2s ? Center::Ring : Center::LdsTile;
            }
        }
    }
    if (L > 0 && AL > 0 && center_ring && m.gnn[0].attn[0].cc.fwd2s) p.gnn[0].layers[0].center = Center::Ring;
    if (trr && (sw.trr_compress & 2) && m.eh0.fwd2 && m.eh2.fwd2)
        p.head_edge = ring_serves(E) && m.eh0.fwd2s && m.eh2.fwd2s ? Rows::Ring : Rows::Pipelined;
    return p;
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------
int plan_backward(const Model& m, const Graph& g, const FwdRecord* rec, bool tr, StagePlan& p) {
    const Switches& sw = switches();
    const int64_t N = g.n_nodes, E = g.n_edges, R = E + N;
    const int L = m.h.num_gnn_layers, AL = m.h.num_attention_layers;
    p = StagePlan();
    p.gnn.assign(L, GnnPlan{Rows::LdsTile, Rows::Pipelined, std::vector<LayerPlan>(AL)});
    const bool trr = use_trr();
    const bool trr_l = trr && m.plain_layers();
    const bool res = m.residual();
    const bool enabled = side_stream().enabled;
    p.attn_preload = trr;
    p.side_heads = enabled && !tr;  // training: the weight-gradient scratch is shared, one stream
    p.side = enabled && !(tr || m.post_ln() || res);
    if (trr && (sw.trr_compress & 2) && m.eh0.fwd2 && m.eh2.fwd2 && m.eh0.bwd2 && m.eh2.bwd2)
        p.head_edge = !tr && ring_serves(E) && m.eh0.fwd2s && m.eh2.fwd2s && m.eh0.bwd2s && m.eh2.bwd2s ? Rows::Ring : Rows::Pipelined;
    if (L == 0 || AL == 0) return PET_OK;
    const bool fused_attn = trr_l && !tr && ablk_bwd_on(g) && m.gnn[0].attn[0].qkv.bwd2s;
    // a forward that kept nothing (save_for_backward = 0) wrote neither [v; g] nor the compress pre-activations: no adjoint
    // can follow it, whatever the switches say
    PET_REQUIRE(!rec || rec->save != 0, PET_ERR_ARGUMENT,
                "the last forward into this workspace ran with save_for_backward = 0: nothing was kept for an adjoint");
    // the forward that filled this workspace decided by itself whether Q, K, V were written: if it ran the fused block, the
    // three-kernel adjoint would read buffers nobody wrote (a switch flipped between the two calls) -- refuse
    PET_REQUIRE(!(rec && rec->plan.unsaved_attn()) || fused_attn, PET_ERR_ARGUMENT,
                "the forward of this workspace ran the fused attention block (Q, K, V not saved) but the adjoint is "
                "configured for the three-kernel form: pet_config_set changed between forward and backward");
    const bool rec_layers = rec && (int)rec->plan.gnn.size() == L;  // (a record of the size-generic path has no layers)
    // k_dxf folded into its producer and its consumer (pet_config_set("dxf_fused", 0): the separate kernel)
    p.dxf_fused = trr_l && !tr && !res && !g.x_fn && AL >= 1 && sw.dxf_fused;
    p.dbias_stride = fused_attn ? NHEAD : 1;
    p.center_bwd_deep = N <= CENTER_BWD_DEEP_MAX_ATOMS;
    const bool center_ring = !tr && ring_center_serves(N);
    for (int gi = 0; gi < L; gi++) {
        const GnnLayerW& G = m.gnn[gi];
        GnnPlan& P = p.gnn[gi];
        if (!tr && ring_serves(E) && G.comb0_g.bwd2s && G.comb2.bwd2s && G.comb0_g.b) P.comb = Rows::Ring;
        if (trr && (sw.trr_compress & 1) && G.compress2.bwd2 && G.wc2 && (gi == 0 || G.compress0_msg.bwd2) && E > 0)
            P.compress = !tr && ring_serves(E) && G.compress2.bwd2s && G.wc2s && (gi == 0 || G.compress0_msg.bwd2s) ? Rows::Ring : Rows::Pipelined;
        for (int a = 0; a < AL; a++) {
            const AttnLayerW& A = G.attn[a];
            LayerPlan& Q = P.layers[a];
            // large graphs: two ring GEMMs beside the edge kernels; scratch (and the split form's partials): the attention-output
            // temporary of the forward pass (R * D floats), which no adjoint kernel touches
            if (!tr && sw.node_planes && (size_t)N * 3 * DNF <= (size_t)R * D && ring_serves(N) && A.cmlp_in.bwd2s &&
                A.cmlp_out.bwd2s && N > 0)
                Q.node = Node::Ring;
            else if (!tr && sw.node_planes && A.cmlp_out.bwd2 && A.cmlp_in.bwd2)
                Q.node = node_planes_form(N, (size_t)R * D);
            // (the 32-row kernels form the expansion adjoint in the same launch)
            Q.expand = Q.node == Node::Split || Q.node == Node::Rows32 ? Center::ByNode : center_ring && A.ce.bwd2s ? Center::Ring : Center::LdsTile;
            Q.center = center_ring && A.cc.bwd2s ? Center::Ring : Center::LdsTile;
            // the forward of this workspace did not save [v; g] (its record says so; without a record -- a graph handle made
            // anew for the adjoint call -- the forward followed the same switches as this call does)
            const bool recompute = rec ? rec_layers && !rec->plan.gnn[gi].layers[a].emlp_saved
                                       : !tr && trr_l && emlp_recompute_on(A.mlp_in, A.mlp_out, E);
            Q.emlp_saved = !recompute;
            Q.emlp = recompute ? Rows::Ring : trr_l ? Rows::Pipelined : Rows::LdsTile;
            PET_REQUIRE(!recompute || (!tr && trr_l && sw.emlp_s && A.mlp_in_g.fwd2s && A.mlp_in_g.bwd2s && A.mlp_out.bwd2s),
                        PET_ERR_ARGUMENT, "the forward of this workspace did not save the edge MLP's pre-activations "
                        "and the recomputing adjoint is switched off: pet_config_set changed between forward and backward");
            // (one form for every layer: the key-bias reduction assumes it; ablk_bwd refuses a layer whose weights are not packed)
            Q.attn = fused_attn ? Attn::Fused : trr_l ? Attn::Pipelined : Attn::LdsTile;
        }
    }
    return PET_OK;
}

}  // namespace pet
