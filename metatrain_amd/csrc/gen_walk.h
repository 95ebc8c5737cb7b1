// The PET architecture on the size-generic path, stated once per direction: the forward walk and the reverse walk over the
// GNN and attention layers (backend.py:496-649, transformer.py:189-247), for every pass of gen.hip and gen_train.hip.
//
// A walk is a template over a PASS object `p` and the pass' workspace `w`. The pass supplies the value type V -- one array
// (`float*`, Ops / Infer in gen.hip) or a (primal, tangent) pair, for an adjoint (nu, lambda) (`D2`, TOps in gen_train.hip)
// -- the operations on V (linf / linb, norm / norm_rev, silu / silu_rev, swiglu / swiglu_rev, axpby, copy, zero, embed,
// attn / attn_rev, add_cond), the scratch buffers by role (p.s, a Roles<V>), and the hooks only some passes have, each
// an empty inline function elsewhere so that a pass without it launches nothing:
//   wgrad, embed_grad        weight / table gradients (dual training); norm parameters ride on norm_rev
//   re_norm, re_silu, re_swiglu   the operand of a weight gradient, recomputed where the adjoint is about to overwrite it
//   geo_sink, key_bias_sink  where the adjoints of geo = (v, d) and of the attention key bias go: g_geo / g_fc
//                            (inference), the taps of the Hessian-vector mode, nowhere (training)
//   cond_accum               the conditioning embedding's adjoint (dual training)
//   seed                     the read-out adjoints entering layer l
// Every operation skips zero rows: a batch without an edge (E == 0) walks the node path with no guard here.
// `w` holds the saved activations (w.gnn[gi].attn[a], H0, M0) and the adjoints the reverse walk carries between layers:
// dH (node features entering the next stage), dM (messages leaving layer gi), dX / dX2, dQKV.
#pragma once
#include "gen_common.h"

namespace pet {

namespace {

template <class P, class WS>
static void gen_walk_forward(P& p, WS& w) {
    using V = typename P::V;
    const Model& m = p.m;
    const Graph& g = p.g;
    const GD& d = p.d;
    const Roles<V>& s = p.s;
    const int64_t N = p.N, E = p.E, R = p.R;
    const int D = d.D, DN = d.DN, L = m.h.num_gnn_layers, AL = m.h.num_attention_layers;
    const bool post = m.post_ln(), res = m.residual();
    p.embed(g.sp, m.node_emb, w.H0, DN, N, DN);
    p.embed(g.sp_nbr, m.edge_emb, w.M0, D, E, D);
    V Min = w.M0;
    for (int gi = 0; gi < L; gi++) {
        const GnnLayerW& G = m.gnn[gi];
        auto& B = w.gnn[gi];
        if (res && gi > 0) p.embed(g.sp, m.node_embs[gi], B.Hin, DN, N, DN);
        // tokens = [edge_embedder([v, d]) ; (gi > 0: neighbor_embedder[species]) ; message] -> compress (transformer.py:499-521)
        const int kin = (gi == 0 ? 2 : 3) * D;
        p.linf(p.geo, 4, G.eemb, B.TOK, kin, E);
        if (gi > 0) p.embed(g.sp_nbr, G.nbr_emb, off(B.TOK, D), kin, E, D);
        p.axpby(1.f, Min, D, 0.f, V(), 0, nullptr, off(B.TOK, kin - D), kin, false, E, D);
        p.linf(B.TOK, kin, G.c0, B.a0, D, E);
        p.silu(B.a0, s.OUT, E * D);
        p.linf(s.OUT, D, G.compress2, B.attn[0].X, D, E);
        for (int a = 0; a < AL; a++) {
            const AttnLayerW& A = G.attn[a];
            auto& Ab = B.attn[a];
            const V Xnext = (a + 1 < AL) ? B.attn[a + 1].X : B.XF;
            // centre token (transformer.py:210-214)
            if (d.expanded) p.linf(Ab.H, DN, A.cc, off(Ab.X, E * D), D, N);
            else p.copy(Ab.H, off(Ab.X, E * D), N, D);
            V Xatt = Ab.X;
            if (!post) { p.norm(Ab.X, A.g_attn, A.b_attn, s.normed, R, D); Xatt = s.normed; }
            p.linf(Xatt, D, A.qkv, Ab.QKV, 3 * D, R);
            p.attn(Ab);
            p.linf(Ab.AO, D, A.out, s.OUT, D, R);   // output_linear of every token
            if (!post) {
                p.copy(off(s.OUT, E * D), Ab.TOKo, N, D);
                // edges: residual + MLP (transformer.py:229-232)
                p.axpby(1.f, Ab.X, D, 1.f, s.OUT, D, nullptr, Ab.X1, D, false, E, D);
                gen_ffn(p, Ab.X1, true, A.g_mlp, A.b_mlp, A.mlp_in, A.mlp_out, Ab.VG, Ab.X1, Xnext, s.normed, s.act, E, D, d.DFF);
            } else {
                // transformer.py:245-247 on every token: S1 = tokens + attention; T1 = norm(S1); S2 = T1 + MLP(T1); T2 = norm(S2)
                p.axpby(1.f, Ab.X, D, 1.f, s.OUT, D, nullptr, Ab.X1, D, false, R, D);
                p.norm(Ab.X1, A.g_attn, A.b_attn, Ab.T1, R, D);
                gen_ffn(p, Ab.T1, false, nullptr, nullptr, A.mlp_in, A.mlp_out, Ab.VG, Ab.T1, Ab.S2, s.normed, s.act, R, D, d.DFF);
                p.norm(Ab.S2, A.g_mlp, A.b_mlp, s.normed, R, D);
                p.copy(s.normed, Xnext, E, D);
                p.copy(off(s.normed, E * D), Ab.TOKo, N, D);
            }
            // node update (transformer.py:221-227)
            if (d.expanded) {
                p.copy(Ab.H, Ab.H1, N, DN);
                p.linf(Ab.TOKo, D, A.ce, Ab.H1, DN, N, true);
                gen_ffn(p, Ab.H1, true, A.g_center, A.b_center, A.cmlp_in, A.cmlp_out, Ab.VGn, Ab.H1, Ab.Hn, s.nNormed, s.nAct, N, DN, d.DNF);
            } else
                p.copy(Ab.TOKo, Ab.Hn, N, DN);
        }
        // backend.py:543-545: added to the node features LEAVING the layer; no tangent, it does not move with the positions
        if (m.h.system_conditioning) p.add_cond(B.Hout);
        if (res) {
            if (gi + 1 < L) p.axpby(0.5f, Min, D, 0.5f, B.XF, D, g.rev, B.Mout, D, false, E, D);   // backend.py:640-647
        } else {
            // backend.py:559-575: m = m + e + MLP(LayerNorm([e ; e[rev]]))
            const V CAT = s.normed;
            p.axpby(1.f, B.XF, D, 0.f, V(), 0, nullptr, CAT, 2 * D, false, E, D);
            p.axpby(0.f, V(), 0, 1.f, B.XF, D, g.rev, off(CAT, D), 2 * D, false, E, D);
            p.norm(CAT, G.ln_g, G.ln_b, s.OUT, E, 2 * D, 1, 1e-5f);
            p.linf(s.OUT, 2 * D, G.comb0, B.CA, 2 * D, E);
            p.silu(B.CA, s.act, E * 2 * D);
            p.axpby(1.f, Min, D, 1.f, B.XF, D, nullptr, B.Mout, D, false, E, D);
            p.linf(s.act, 2 * D, G.comb2, B.Mout, D, E, true);
        }
        Min = B.Mout;
    }
}

// Two adjoints live across the layers: w.dH and w.dM. Within a layer dXF is the adjoint of the edge tokens leaving the
// transformer ([E][D]; its rows E.. are scratch) and dMin that of the incoming messages.
template <class P, class WS>
static void gen_walk_reverse(P& p, WS& w) {
    using V = typename P::V;
    const Model& m = p.m;
    const Graph& g = p.g;
    const GD& d = p.d;
    const Roles<V>& s = p.s;
    const int64_t N = p.N, E = p.E, R = p.R;
    const int D = d.D, DN = d.DN, L = m.h.num_gnn_layers, AL = m.h.num_attention_layers;
    const bool post = m.post_ln(), res = m.residual();
    const V dXF = w.dX, dMin = w.dX2;
    if (res) p.zero(w.dM, E * D);   // the last layer's messages are never read
    else p.seed(0, w.dH, w.dM);
    for (int gi = L - 1; gi >= 0; gi--) {
        const GnnLayerW& G = m.gnn[gi];
        auto& B = w.gnn[gi];
        if (res) {
            // readout of this layer + (gi + 1 < L) the averaged messages: Mout = 0.5 (Min + XF[rev])
            p.seed(gi, w.dH, dXF);
            if (gi + 1 < L) {
                p.axpby(0.f, V(), 0, 0.5f, w.dM, D, g.rev, dXF, D, true, E, D);   // rev is an involution
                p.axpby(0.5f, w.dM, D, 0.f, V(), 0, nullptr, dMin, D, false, E, D);
            } else
                p.zero(dMin, E * D);
        } else {
            // Mout = Min + XF + comb2(silu(comb0(LN([XF ; XF[rev]]))))
            const V CAT = s.dAO, dS = s.dOUT, dCN = s.dVG;
            p.axpby(1.f, B.XF, D, 0.f, V(), 0, nullptr, CAT, 2 * D, false, E, D);
            p.axpby(0.f, V(), 0, 1.f, B.XF, D, g.rev, off(CAT, D), 2 * D, false, E, D);
            p.re_silu(B.CA, dS, E * 2 * D);                                    // input of comb2
            p.wgrad(G.comb2, w.dM, D, dS, 2 * D, E);
            p.linb(w.dM, D, G.comb2, dS, 2 * D, E);                            // of silu(CA)
            p.silu_rev(B.CA, dS, E * 2 * D);
            p.re_norm(CAT, G.ln_g, G.ln_b, dCN, E, 2 * D, 1, 1e-5f);           // input of comb0
            p.wgrad(G.comb0, dS, 2 * D, dCN, 2 * D, E);
            p.linb(dS, 2 * D, G.comb0, dCN, 2 * D, E);                         // of LN(CAT)
            const V dCAT = dS;
            p.norm_rev(CAT, G.ln_g, G.ln_b, dCN, dCAT, false, s.re, E, 2 * D, 1, 1e-5f);
            // dXF = dM + dCAT[:, :D] + dCAT[rev][:, D:]
            p.copy(w.dM, dXF, E, D);
            p.axpby(1.f, dCAT, 2 * D, 1.f, off(dCAT, D), 2 * D, g.rev, dXF, D, true, E, D);
            p.copy(w.dM, dMin, E, D);
        }
        p.cond_accum(w.dH, gi == L - 1);
        // transformer layers, last to first
        for (int a = AL - 1; a >= 0; a--) {
            const AttnLayerW& A = G.attn[a];
            auto& Ab = B.attn[a];
            // ---- node update: dH (of Hn) -> dTOKo [N][D] and dH (of H entering the layer)
            if (d.expanded) {
                // Hn = H1 + cmlp(norm(H1)); H1 = H + ce(TOKo)   (s.dTOKo may be the FFN's last temporary: it is written after)
                p.copy(w.dH, s.dH1, N, DN);
                gen_ffn_rev(p, Ab.H1, true, A.g_center, A.b_center, A.cmlp_in, A.cmlp_out, Ab.VGn, w.dH, s.dH1, true, s.nA, s.nB,
                            s.nRe, N, DN, d.DNF);
                p.wgrad(A.ce, s.dH1, DN, Ab.TOKo, D, N);
                p.linb(s.dH1, DN, A.ce, s.dTOKo, D, N);
                p.copy(s.dH1, w.dH, N, DN);   // through the residual H1 = H + ...
            } else {
                p.copy(w.dH, s.dTOKo, N, D);
                p.zero(w.dH, N * DN);
            }
            // ---- dOUT: adjoint entering output_linear; dXin: adjoint of the tokens ENTERING the layer, both [R][D]
            const V dOUT = s.dOUT, dXin = s.dXin;
            if (!post) {
                // edges: X2 = X1 + mlp(norm(X1)); X1 = X + OUT_e; the centre token has no residual
                p.copy(dXF, dXin, E, D);
                gen_ffn_rev(p, Ab.X1, true, A.g_mlp, A.b_mlp, A.mlp_in, A.mlp_out, Ab.VG, dXF, dXin, true, s.dAO, s.dVG, s.re, E, D,
                            d.DFF);
                p.copy(dXin, dOUT, E, D);
                p.copy(s.dTOKo, off(dOUT, E * D), N, D);
                p.zero(off(dXin, E * D), N * D);
            } else {
                // T2 = norm_mlp(S2) [edges -> next tokens, centre -> TOKo]; S2 = T1 + mlp(T1); T1 = norm_attn(S1); S1 = X + OUT
                const V dT2 = s.dAO, dS2 = dOUT, dT1 = dXin, dS1 = s.dAO;
                p.copy(dXF, dT2, E, D);
                p.copy(s.dTOKo, off(dT2, E * D), N, D);
                p.norm_rev(Ab.S2, A.g_mlp, A.b_mlp, dT2, dS2, false, s.dVG, R, D);
                p.copy(dS2, dT1, R, D);
                gen_ffn_rev(p, Ab.T1, false, nullptr, nullptr, A.mlp_in, A.mlp_out, Ab.VG, dS2, dT1, true, s.dAO, s.dVG, s.re, R, D,
                            d.DFF);
                p.norm_rev(Ab.X1, A.g_attn, A.b_attn, dT1, dS1, false, s.dVG, R, D);
                p.copy(dS1, dOUT, R, D);
                p.copy(dS1, dXin, R, D);
            }
            // ---- output_linear, attention, input_linear
            p.wgrad(A.out, dOUT, D, Ab.AO, D, R);
            p.linb(dOUT, D, A.out, s.dAO, D, R);
            p.attn_rev(Ab, s.dAO);   // -> w.dQKV
            p.key_bias_sink(gi == L - 1 && a == AL - 1);
            if (!post) {
                const V Xn = s.dAO, dXn = dOUT;
                p.re_norm(Ab.X, A.g_attn, A.b_attn, Xn, R, D);   // input of input_linear
                p.wgrad(A.qkv, w.dQKV, 3 * D, Xn, D, R);
                p.linb(w.dQKV, 3 * D, A.qkv, dXn, D, R);
                p.norm_rev(Ab.X, A.g_attn, A.b_attn, dXn, dXin, true, s.dVG, R, D);
            } else {
                p.wgrad(A.qkv, w.dQKV, 3 * D, Ab.X, D, R);
                p.linb(w.dQKV, 3 * D, A.qkv, dXin, D, R, true);
            }
            // ---- split the token adjoint: edges -> dXF of the previous layer, centre -> dH through center_contraction
            p.copy(dXin, dXF, E, D);
            if (d.expanded) {
                p.wgrad(A.cc, off(dXin, E * D), D, Ab.H, DN, N);
                p.linb(off(dXin, E * D), D, A.cc, w.dH, DN, N, true);
            } else
                p.axpby(1.f, off(dXin, E * D), D, 0.f, V(), 0, nullptr, w.dH, DN, true, N, DN);
        }
        // ---- compress: X0 = c2(silu(a0)), a0 = c0 [EE ; (nbr emb) ; Min]
        const int kin = (gi == 0 ? 2 : 3) * D;
        const V dS = s.dAO, dTOK = s.dOUT;
        p.re_silu(B.a0, dS, E * D);
        p.wgrad(G.compress2, dXF, D, dS, D, E);
        p.linb(dXF, D, G.compress2, dS, D, E);
        p.silu_rev(B.a0, dS, E * D);
        p.wgrad(G.c0, dS, D, B.TOK, kin, E);
        p.linb(dS, D, G.c0, dTOK, kin, E);
        p.wgrad(G.eemb, dTOK, kin, p.geo, 4, E);
        p.geo_sink(dTOK, kin, G.eemb, gi == L - 1);   // through edge_embedder([v, d])
        if (gi > 0) p.embed_grad(g.sp_nbr, off(dTOK, D), kin, E, D, G.nbr_emb);
        p.axpby(1.f, off(dTOK, kin - D), kin, 0.f, V(), 0, nullptr, dMin, D, true, E, D);
        p.copy(dMin, w.dM, E, D);   // adjoint of the previous layer's messages
        // node features entering the layer: an embedding per layer (residual) or the previous layer's output
        if (res || gi == 0) {
            p.embed_grad(g.sp, w.dH, DN, N, DN, m.node_embs[res ? gi : 0]);
            if (res) p.zero(w.dH, N * DN);
        }
    }
    p.embed_grad(g.sp_nbr, w.dM, D, E, D, m.edge_emb);   // the first layer's messages are the neighbour embedding
}

}  // namespace

}  // namespace pet
