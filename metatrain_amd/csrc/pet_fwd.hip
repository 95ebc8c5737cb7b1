// PET forward on gfx950: fused row-tile kernels (fp32 MFMA) + per-atom attention.
//
// Token layout: one buffer X[(E+N), D]; rows 0..E-1 are the edges in CSR order
// (edge p belongs to atom ctr[p], rows rowptr[i]..rowptr[i+1]-1), rows E..E+N-1
// are the centre tokens. The reference pads every atom to max_neighbors and runs
// [N, M+1, D] batches (pet/modules/transformer.py:463-562); here there are no pads.
//
// Reference map:
//   k_compress   transformer.py:499-521 (edge_embedder, neighbor_embedder, compress MLP)
//   k_center     transformer.py:211-214 (center_contraction)
//   k_qkv        transformer.py:216-218 + 103-107 (norm_attention, input_linear)
//   k_attn_fwd   transformer.py:108-151 / 565-589 (softmax(QK^T/sqrt(hd)/tau + log fc) V)
//   k_oproj      transformer.py:151 + 229 (output_linear, edge residual)
//   k_node       transformer.py:222-227 (center_expansion, center_mlp)
//   k_emlp       transformer.py:230-232 (edge SwiGLU MLP)
//   (combination stage backend.py:559-575: k_comb_p2 in pet_comb.hip)
//   k_head_*     backend.py:651-687, 726-777 (heads, last layers, cutoff-weighted sum)
// The kernels of these stages and their launchers: pet_tile.hip (LDS-tile family), pet_node.hip, pet_attn.hip and the pipelined /
// ring / fused-block files; pet_stages.h declares the launchers by stage. This file: the driver, and the embedding, conditioning,
// exchange and read-out kernels around it.
#include "common.h"
#include "model.h"
#include "pet_stages.h"
#include "pet_ws.h"
#include "tile.h"

namespace pet {

// ---------------------------------------------------------------------------------
// node embedding lookup
// ---------------------------------------------------------------------------------
__global__ void k_node_embed(const int* __restrict__ sp, const float* __restrict__ emb,
                             float* __restrict__ H, int n) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
    if (idx >= (int64_t)n * (DN / 4)) return;
    int i = (int)(idx / (DN / 4)), c = (int)(idx % (DN / 4));
    reinterpret_cast<float4*>(H)[idx] = reinterpret_cast<const float4*>(emb + (size_t)sp[i] * DN)[c];
}
static void node_embed(const int* sp, const float* emb, float* H, int64_t N, hipStream_t st) {
    k_node_embed<<<cdiv(N * (DN / 4), 256), 256, 0, st>>>(sp, emb, H, (int)N);
}

// ---------------------------------------------------------------------------------
// system conditioning (conditioning.py:82-100): cond[s] = W2 silu(W0 [emb_q[charge_s + max_charge] ; emb_m[mult_s - 1]] + b0) + b2,
// one 256-thread block per SYSTEM (a handful of rows: plain fp32 dot products), then h_i += cond[system of i] after every
// GNN layer (backend.py:543-545, :628-629)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(DN) void k_system_cond(const int64_t* __restrict__ charge, const int64_t* __restrict__ spin,
                                                   const float* __restrict__ emb_q, const float* __restrict__ emb_m,
                                                   const float* __restrict__ w0, const float* __restrict__ b0,
                                                   const float* __restrict__ w2, const float* __restrict__ b2,
                                                   float* __restrict__ cond, int max_charge, int max_spin) {
    __shared__ float x[2 * DN], hid[DN];
    const int s = blockIdx.x, t = threadIdx.x;
    int q = (int)charge[s] + max_charge, mi = (int)spin[s] - 1;
    q = q < 0 ? 0 : (q > 2 * max_charge ? 2 * max_charge : q);  // the caller validates (conditioning.py:54-80); stay in bounds
    mi = mi < 0 ? 0 : (mi > max_spin - 1 ? max_spin - 1 : mi);
    x[t] = emb_q[(size_t)q * DN + t];
    x[DN + t] = emb_m[(size_t)mi * DN + t];
    __syncthreads();
    float a = b0[t];
    for (int k = 0; k < 2 * DN; k++) a = fmaf(w0[(size_t)t * 2 * DN + k], x[k], a);
    hid[t] = siluf_(a);
    __syncthreads();
    float o = b2[t];
    for (int k = 0; k < DN; k++) o = fmaf(w2[(size_t)t * DN + k], hid[k], o);
    cond[(size_t)s * DN + t] = o;
}
__global__ void k_add_cond(float* __restrict__ H, const float* __restrict__ cond, const int* __restrict__ sys32,
                           const int64_t* __restrict__ sys64, int n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
    if (idx >= (int64_t)n * (DN / 4)) return;
    const int i = (int)(idx / (DN / 4)), c = (int)(idx % (DN / 4));
    const int64_t s = sys64 ? sys64[i] : (int64_t)sys32[i];
    float4 h = reinterpret_cast<float4*>(H)[idx];
    const float4 a = reinterpret_cast<const float4*>(cond + s * DN)[c];
    h.x += a.x; h.y += a.y; h.z += a.z; h.w += a.w;
    reinterpret_cast<float4*>(H)[idx] = h;
}
static void system_cond(const Model& m, const Graph& g, float* cond, hipStream_t st) {
    k_system_cond<<<(int)g.n_cond_systems, DN, 0, st>>>(g.cond_charge, g.cond_spin, m.cond_qe, m.cond_se, m.cond_w0, m.cond_b0,
                                                         m.cond_w2, m.cond_b2, cond, m.h.max_charge, m.h.max_spin_multiplicity);
}
static void add_cond(float* H, const float* cond, const Graph& g, int64_t N, hipStream_t st) {
    k_add_cond<<<cdiv(N * (DN / 4), 256), 256, 0, st>>>(H, cond, g.sys, g.cond_sys, (int)N);
}

// atomic[i] = ynode[i] + sum_{edges of i} ye   (backend.py:768-772, 476)
__global__ void k_atom_sum(const float* __restrict__ ynode, const float* __restrict__ ye,
                           const int* __restrict__ rowptr, float* __restrict__ atomic, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) s += ye[p];
    atomic[i] = ynode[i] + s;
}
static void atom_sum(const float* ynode, const float* ye, const int* rowptr, float* atomic, int64_t N, hipStream_t st) {
    k_atom_sum<<<cdiv(N, 256), 256, 0, st>>>(ynode, ye, rowptr, atomic, (int)N);
}

// out[i][c] = sum_{edges p of i} fc[p] X[p][c], c < 128: one wave per atom, two columns per lane
// (the cutoff-weighted edge sums of pet/model.py:753 and :797-799)
__global__ void k_edge_sum_fc(const float* __restrict__ X, const float* __restrict__ fc, const int* __restrict__ rowptr,
                              float* __restrict__ out, int ldo, int n) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    float2 s = make_float2(0.f, 0.f);
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) {
        const float f = fc[p];
        const float2 x = *reinterpret_cast<const float2*>(X + (int64_t)p * D + 2 * lane);
        s.x = fmaf(f, x.x, s.x);
        s.y = fmaf(f, x.y, s.y);
    }
    *reinterpret_cast<float2*>(out + (int64_t)i * ldo + 2 * lane) = s;
}
__global__ void k_copy_rows(const float* __restrict__ X, int w, float* __restrict__ out, int ldo, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * w) return;
    out[(idx / w) * ldo + idx % w] = X[idx];
}

// ---------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------
// ---- per-layer exchange of edge tokens (one box over several ranks): staging kernels around the caller's collective
__global__ void k_rows_gather(const float* __restrict__ X, const int* __restrict__ rows, int64_t n, float* __restrict__ buf) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one float4 per thread, D / 4 per row
    if (idx >= n * (D / 4)) return;
    const int64_t r = idx / (D / 4);
    const int c = (int)(idx % (D / 4));
    reinterpret_cast<float4*>(buf)[idx] = reinterpret_cast<const float4*>(X + (int64_t)rows[r] * D)[c];
}
// mode 0: X[rows] = buf; 1: X[rows] += buf; 2: X[rows] = 0
__global__ void k_rows_scatter(const float* __restrict__ buf, const int* __restrict__ rows, int64_t n, float* __restrict__ X,
                               int mode) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * (D / 4)) return;
    const int64_t r = idx / (D / 4);
    const int c = (int)(idx % (D / 4));
    float4* dst = reinterpret_cast<float4*>(X + (int64_t)rows[r] * D) + c;
    if (mode == 2) { *dst = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float4 v = reinterpret_cast<const float4*>(buf)[idx];
    if (mode == 0) *dst = v;
    else { float4 o = *dst; o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w; *dst = o; }
}
// forward: XF[ghost rows] <- the owners' XF[export rows]   (before the combination stage reads e[rev])
int exchange_forward(const Graph& g, float* XF, int layer, hipStream_t st) {
    if (!g.x_fn) return PET_OK;
    if (g.n_export > 0)
        k_rows_gather<<<cdiv(g.n_export * (D / 4), 256), 256, 0, st>>>(XF, g.x_export, g.n_export, g.x_export_buf);
    PET_REQUIRE(g.x_fn(g.x_user, 0, layer) == 0, PET_ERR_ARGUMENT, "the exchange callback failed (forward)");
    if (g.n_ghost > 0)
        k_rows_scatter<<<cdiv(g.n_ghost * (D / 4), 256), 256, 0, st>>>(g.x_ghost_buf, g.x_ghost, g.n_ghost, XF, 0);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}
// reverse: the adjoint that landed on ghost rows belongs to their owners: send it, zero it here, add what arrives to the
// export rows
int exchange_backward(const Graph& g, float* dXF, int layer, hipStream_t st) {
    if (!g.x_fn) return PET_OK;
    if (g.n_ghost > 0) {
        k_rows_gather<<<cdiv(g.n_ghost * (D / 4), 256), 256, 0, st>>>(dXF, g.x_ghost, g.n_ghost, g.x_ghost_buf);
        k_rows_scatter<<<cdiv(g.n_ghost * (D / 4), 256), 256, 0, st>>>(nullptr, g.x_ghost, g.n_ghost, dXF, 2);
    }
    PET_REQUIRE(g.x_fn(g.x_user, 1, layer) == 0, PET_ERR_ARGUMENT, "the exchange callback failed (reverse)");
    if (g.n_export > 0)
        k_rows_scatter<<<cdiv(g.n_export * (D / 4), 256), 256, 0, st>>>(g.x_export_buf, g.x_export, g.n_export, dXF, 1);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int64_t forward_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges, bool train) {
    if (m.generic() || (train && train_generic(m))) return gen_workspace_bytes(m, n_nodes, n_edges);  // gen.hip
    Workspace w;
    carve_workspace(m, n_nodes, n_edges, nullptr, w, train);
    return (int64_t)w.bytes;
}

int attn_tiles(const Graph& g) { return (g.max_nbr + 1 + 15) / 16; }
bool use_generic(const Model& m, const Graph& g) { return m.generic() || attn_tiles(g) > 8; }
// Which layout the last forward of THIS graph left in a workspace: a training forward of a PostLN / residual model of the
// compiled size runs on the size-generic path while its inference forward runs on the tuned kernels, and the adjoint calls
// must follow. Recorded on the graph handle (host side, the caller owns its lifetime): no process-global table, and an
// adjoint call on a workspace this graph's forward has not written falls back to what (model, graph) say.
bool generic_workspace(const Graph& g, const void* ws) {
    const Graph::FwdRecord* r = g.fwd_record(ws);
    return r && r->generic;
}
static Graph::FwdRecord& note_workspace(const Graph& g, const void* ws, bool generic) {
    Graph::FwdRecord& r = g.fwd_record_new(ws);
    r.generic = generic;
    return r;
}

// sum_i (n_i + 1)^2 estimated from the mean neighbour count (exact value is not needed on the hot path)
double g_sum_t2(const Graph& g) {
    if (g.n_nodes == 0) return 0.0;
    const double t = (double)g.n_edges / (double)g.n_nodes + 1.0;
    return (double)g.n_nodes * t * t;
}

int forward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int save, float* atomic,
            float* node_feat, float* edge_feat, hipStream_t st) {
    PET_REQUIRE(!m.residual() || (!node_feat && !edge_feat), PET_ERR_ARGUMENT,
                "residual featuriser: one feature pair per GNN layer, use pet_forward_layers");
    return forward_layers(m, g, ws, ws_bytes, save, atomic, &node_feat, &edge_feat, 1, st);
}

// node_feats / edge_feats: n_layers = num_readout_layers() output pointers each (entries may be null)
int forward_layers(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int save, float* atomic,
                   float* const* node_feats, float* const* edge_feats, int n_layers, hipStream_t st) {
    const bool gen = use_generic(m, g) || (save == 2 && train_generic_for(m, g));
    PET_REQUIRE(!(gen && g.x_fn), PET_ERR_UNSUPPORTED, "the per-layer exchange is built for the tuned path (default model size)");
    Graph::FwdRecord& fwd_rec = note_workspace(g, ws, gen);
    fwd_rec.save = save;
    if (gen) return gen_forward_layers(m, g, ws, ws_bytes, save, atomic, node_feats, edge_feats, n_layers, st);
    if (int rcl = graph_attention_lists(g, st)) return rcl;
    Workspace w;
    carve_workspace(m, g.n_nodes, g.n_edges, ws, w, save == 2);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "forward workspace too small");
    const bool post = m.post_ln(), res = m.residual();
    PET_REQUIRE(res ? (n_layers == m.h.num_gnn_layers || (n_layers == 1 && !node_feats[0] && !edge_feats[0])) : n_layers == 1,
                PET_ERR_ARGUMENT, "expected one feature pair per readout layer (" + std::to_string(m.num_readout_layers()) + ")");
    PET_REQUIRE(!(atomic && res), PET_ERR_UNSUPPORTED,
                "the fused head reads one readout layer; with the residual featuriser use pet_forward_layers and "
                "pet_predict per readout layer");
    PET_REQUIRE(save != 2 || m.trainable(), PET_ERR_UNSUPPORTED,
                "training is built for transformer_type=PreLN, featurizer_type=feedforward only");
    const int64_t N = g.n_nodes, E = g.n_edges, R = E + N;
    if (N == 0) return PET_OK;
    const int nt = attn_tiles(g);
    const float scale = 1.0f / (sqrtf((float)HD) * m.h.attention_temperature);
    const double fE = (double)E, fN = (double)N, fR = (double)R;
    // which kernel serves every stage below: decided here, once (pet_plan.hip); the adjoint of this workspace follows it
    const StagePlan& plan = fwd_rec.plan = plan_forward(m, g, save);
    // attention: 4 T^2 d FLOPs per atom per layer; T^2 summed on the host side of the graph
    const double attn_flops = 4.0 * D * g_sum_t2(g);
    const int L = m.h.num_gnn_layers, AL = m.h.num_attention_layers;
    SideStream ss = side_stream();
    ss.enabled = plan.side;
    const hipStream_t s2 = ss.stream(st);  // node-feature chain
    bool side_busy = false;
    auto launch_center = [&](int gi, int a) -> int {
        const AttnLayerW& A = m.gnn[gi].attn[a];
        AttnBufs& Ab = w.gnn[gi].attn[a];
        if (a == 0 && res && gi > 0)  // backend.py:617: every GNN layer starts from its own node embedding
            node_embed(g.sp, m.node_embs[gi], w.gnn[gi].Hin, N, s2);
        ProfScope ps("center", s2, fN * 2.0 * DN * D);
        if (plan.gnn[gi].layers[a].center == Center::Ring) return center_s(A.cc, Ab.H, Ab.X + E * D, N, s2);
        return tile_center(A.cc, Ab.H, Ab.X + E * D, N, s2);
    };
    node_embed(g.sp, m.node_emb, w.H0, N, st);
    const bool conditioned = m.h.system_conditioning != 0;
    if (conditioned) {
        PET_REQUIRE(g.cond_charge && g.n_cond_systems >= 1 && g.n_cond_systems <= N, PET_ERR_ARGUMENT,
                    "system_conditioning: call pet_graph_set_conditioning (charge, spin multiplicity, system indices) first");
        system_cond(m, g, w.cond, st);
    }
    ss.fork(st);
    PET_TRY(launch_center(0, 0));
    side_busy = true;
    bool node_cnt_zeroed = false;  // k_node2 SPLIT: the arrival counters are zeroed once per forward, then reset themselves
    for (int gi = 0; gi < L; gi++) {
        const GnnLayerW& G = m.gnn[gi];
        GnnBufs& B = w.gnn[gi];
        const GnnPlan& P = plan.gnn[gi];
        const float* Min = gi == 0 ? nullptr : w.gnn[gi - 1].Mout;
        if (E > 0) {
            ProfScope ps("compress", st, fE * 2.0 * (D * D * (gi == 0 ? 3 : 4) + 4 * D));
            if (P.compress == Rows::Pipelined)  // (save = 0, no adjoint follows: the pre-activation is not stored)
                PET_TRY(trr_compress(gi == 0, g, G, Min, save == 0 ? nullptr : B.a0, B.attn[0].X, E, st));
            else
                PET_TRY(tile_compress(gi == 0, g, G, Min, B.a0, B.attn[0].X, E, st));
        }
        for (int a = 0; a < AL; a++) {
            const AttnLayerW& A = G.attn[a];
            AttnBufs& Ab = B.attn[a];
            const LayerPlan& Q = P.layers[a];
            float* Xnext = (a + 1 < AL) ? B.attn[a + 1].X : B.XF;
            if (side_busy) {  // the centre rows of this layer's tokens come from the node chain
                ss.join(st);
                side_busy = false;
            }
            const bool trr_l = Q.attn == Attn::Pipelined;
            if (Q.attn == Attn::Fused) {
                // the per-atom fused block (pet_ablk.hip): QKV, attention output and nothing else of this stage reach HBM
                ProfScope ps("attn_blk", st, fR * 2.0 * D * 4 * D + attn_flops, fR * 4.0 * 2 * D);  // X in; X1 | OC out
                PET_TRY(ablk_fwd(m, g, A, Ab.X, Ab.X1, Ab.OC, scale, st));
            } else {
            {
                ProfScope ps("qkv", st, fR * 2.0 * D * 3 * D, fR * 4.0 * (D + 3 * D));  // X in, QKV out
                if (trr_l) trr_qkv(Ab.X, A.g_attn, m.layer_norm() ? A.b_attn : nullptr, A.qkv, Ab.QKV, R, st);
                else PET_TRY(tile_qkv(post, Ab.X, A.g_attn, A.b_attn, A.qkv, Ab.QKV, R, st));
            }
            {
                ProfScope ps("attn_fwd", st, attn_flops, fR * 4.0 * (3 * D + D));
                PET_TRY(attn_fwd(nt, plan.attn_preload, Ab.QKV, g, Ab.AO, scale, st));
            }
            {
                ProfScope ps("oproj", st, fR * 2.0 * D * D, fR * 4.0 * 3 * D);  // AO, X in; X1 (| OC) out
                if (trr_l) trr_oproj(Ab.AO, Ab.X, A.out, Ab.X1, Ab.OC, E, R, st);
                else PET_TRY(tile_oproj(post, Ab.AO, Ab.X, A.out, Ab.X1, Ab.OC, E, R, st));
            }
            }
            if (post) {
                // transformer.py:245-247 on every token (edges and centre): norm_attention, + MLP, norm_mlp; the edge rows
                // of the result are the next layer's tokens, the centre row feeds center_expansion
                ProfScope ps("emlp", st, fR * 2.0 * (D * 2 * DFF + DFF * D));
                PET_TRY(tile_rownorm(Ab.X1, A.g_attn, A.b_attn, w.T1, w.T1 + E * D, E, R, st));
                PET_TRY(tile_emlp(false, w.T1, nullptr, nullptr, A.mlp_in, A.mlp_out, Ab.VG, Ab.S2, R, st));
                PET_TRY(tile_rownorm(Ab.S2, A.g_mlp, A.b_mlp, Xnext, Ab.OC, E, R, st));
            }
            // node chain (side stream): node update of this layer, then the centre token of the next
            ss.fork(st);
            const bool has_next = a + 1 < AL || gi + 1 < L;
            const AttnLayerW* An = !has_next ? nullptr : a + 1 < AL ? &G.attn[a + 1] : &m.gnn[gi + 1].attn[0];
            AttnBufs* Abn = !has_next ? nullptr : a + 1 < AL ? &B.attn[a + 1] : &w.gnn[gi + 1].attn[0];
            const bool center_done = has_next && (a + 1 < AL ? P.layers[a + 1] : plan.gnn[gi + 1].layers[0]).center == Center::ByNode;
            {
                ProfScope ps("node", s2, fN * 2.0 * (D * DN + DN * 2 * DNF + DNF * DN));
                // the next layer's centre tokens in the same launch: center_contraction(Hn) as it leaves this kernel
                PET_REQUIRE(!center_done || Abn->H == Ab.Hn, PET_ERR_ARGUMENT,
                            "node update: the next layer does not start from this layer's node features");
                // scratch in dQKV, which only the adjoint uses
                PET_TRY(node_fwd(Q.node, A, Ab.H, Ab.OC, Ab.H1, Ab.VGn, Ab.Hn, center_done ? &An->cc : nullptr,
                                 center_done ? Abn->X + E * D : nullptr, w.dQKV, node_cnt_zeroed, N, s2));
            }
            if (a + 1 == AL && conditioned)  // backend.py:543-545: the node features LEAVING the GNN layer
                add_cond(Ab.Hn, w.cond, g, N, s2);
            if (has_next && !center_done) PET_TRY(a + 1 < AL ? launch_center(gi, a + 1) : launch_center(gi + 1, 0));
            side_busy = true;
            if (E > 0 && !post) {
                ProfScope ps("emlp", st, fE * 2.0 * (D * 2 * DFF + DFF * D), fE * 4.0 * (2 * D + (Q.emlp_saved ? 2 * DFF : 0)));  // X1 in; X2 (and VG, when it is saved) out
                float* vg = Q.emlp_saved ? Ab.VG : nullptr;  // [v; g]: not stored when no adjoint follows or the adjoint recomputes it
                const float* beta = m.layer_norm() ? A.b_mlp : nullptr;
                switch (Q.emlp) {
                case Rows::Ring: PET_TRY(emlp_s(Ab.X1, A.g_mlp, beta, A.mlp_in, A.mlp_out, vg, Xnext, E, st)); break;
                case Rows::Pipelined: trr_emlp(Ab.X1, A.g_mlp, beta, A.mlp_in, A.mlp_out, vg, Xnext, E, st); break;
                case Rows::LdsTile: PET_TRY(tile_emlp(true, Ab.X1, A.g_mlp, A.b_mlp, A.mlp_in, A.mlp_out, Ab.VG, Xnext, E, st)); break;
                }
            }
        }
        if (g.x_fn) {   // one box over several ranks: the transformer outputs of foreign centres arrive from their owners
            PET_REQUIRE(m.plain() && save != 2, PET_ERR_UNSUPPORTED,
                        "the per-layer exchange is built for PreLN + feedforward models, inference and forces");
            int rc = exchange_forward(g, B.XF, gi, st);
            if (rc) return rc;
        }
        if (E > 0 && res) {
            if (gi + 1 < L) {  // the messages of the next layer (backend.py:640-647); the last layer's are never read
                ProfScope ps("comb", st, 0.0, fE * 4.0 * 3 * D);
                PET_TRY(tile_resmix(Min, m.edge_emb, g.sp_nbr, B.XF, g.rev, B.Mout, E, st));
            }
        } else if (E > 0) {
            ProfScope ps("comb", st, fE * 2.0 * (2 * D * 2 * D + 2 * D * D), fE * 4.0 * (3 * D + 2 * D + D));  // e, e[rev], M in; CA, M out
            // (no LDS-tile form: the software-pipelined kernel of pet_comb.hip is the fallback of this stage)
            if (P.comb == Rows::Ring)
                PET_TRY(comb_s(gi == 0, B.XF, g.rev, G.comb0_g, G.comb2, Min, m.edge_emb, g.sp_nbr, B.CA, B.LNS, B.Mout, E, st));
            else
                PET_TRY(trr_comb(gi == 0, B.XF, g, G, Min, m.edge_emb, B.CA, B.LNS, B.Mout, E, st));
        }
    }
    const GnnBufs& last = w.gnn.back();
    if (atomic) {
        PET_REQUIRE(m.has_fused_head, PET_ERR_ARGUMENT,
                    "pet_forward with d_atomic needs the fused single-property target (keys 'node_heads.@...'); use "
                    "pet_predict for other heads");
    }
    if (atomic) {
        ProfScope ps("head_node", s2, fN * 2.0 * (DN * DH + DH * DH + DH));
        PET_TRY(tile_head(false, last.Hout, m.nh0, m.nh2, m.nll_w, m.nll_b, nullptr, nullptr, w.ynode, N, nullptr, 0, s2));
    }
    if (atomic && E > 0) {
        ProfScope ps("head_edge", st, fE * 2.0 * (D * DH + DH * DH + DH));
        switch (plan.head_edge) {
        case Rows::Ring: PET_TRY(head_edge_s(m, last.Mout, g.fc, w.ypred_e, w.ye, E, st)); break;
        case Rows::Pipelined: PET_TRY(trr_head_edge(m, last.Mout, g.fc, w.ypred_e, w.ye, E, st)); break;
        case Rows::LdsTile:
            PET_TRY(tile_head(true, last.Mout, m.eh0, m.eh2, m.ell_w, m.ell_b, g.fc, w.ypred_e, w.ye, E, nullptr, 0, st));
            break;
        }
    }
    ss.join(st);
    if (atomic) atom_sum(w.ynode, w.ye, g.rowptr, atomic, N, st);
    for (int l = 0; l < n_layers; l++) {  // backend.py:585-586 / :621-625: (node, edge) features of every readout layer
        const GnnBufs& Bl = res ? w.gnn[l] : last;
        if (node_feats[l])
            PET_HIP_CHECK(hipMemcpyAsync(node_feats[l], Bl.Hout, N * DN * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (edge_feats[l] && E > 0)
            PET_HIP_CHECK(hipMemcpyAsync(edge_feats[l], res ? Bl.XF : Bl.Mout, E * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// Auxiliary per-atom outputs (pet/model.py:730-875) from the backbone features pet_forward returned:
//   feature    [N, DN + D]  = [ node features | sum_e fc_e edge features ]
//   last_layer [N, 2 DH]    = [ node-head hidden | sum_e fc_e edge-head hidden ]   (the inputs of the last Linear)
// scratch: E DH + max(E, N) floats, needed for last_layer
int aux_outputs(const Model& m, const Graph& g, const float* node_feat, const float* edge_feat, float* feature,
                float* last_layer, float* scratch, hipStream_t st) {
    if (m.generic()) return gen_aux_outputs(m, g, node_feat, edge_feat, feature, last_layer, scratch, st);
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (N == 0) return PET_OK;
    if (feature) {
        k_copy_rows<<<cdiv(N * DN, 256), 256, 0, st>>>(node_feat, DN, feature, DN + D, N);
        k_edge_sum_fc<<<cdiv(N, 4), 256, 0, st>>>(edge_feat, g.fc, g.rowptr, feature + DN, DN + D, (int)N);
    }
    if (last_layer) {
        PET_REQUIRE(scratch, PET_ERR_ARGUMENT, "last-layer features need the scratch buffer");
        float* hid_e = scratch;             // [E, DH] edge-head hidden rows
        float* ytmp = scratch + E * DH;     // [max(E, N)] the heads' scalar predictions, not wanted here
        PET_TRY(tile_head(false, node_feat, m.nh0, m.nh2, m.nll_w, m.nll_b, nullptr, nullptr, ytmp, N, last_layer, 2 * DH, st));
        if (E > 0) PET_TRY(tile_head(true, edge_feat, m.eh0, m.eh2, m.ell_w, m.ell_b, nullptr, nullptr, ytmp, E, hid_e, DH, st));
        k_edge_sum_fc<<<cdiv(N, 4), 256, 0, st>>>(hid_e, g.fc, g.rowptr, last_layer + DH, 2 * DH, (int)N);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

// ---------------------------------------------------------------------------------
// PETBackend.predict as a function of its arguments (backend.py:420-494): heads of ONE (target, readout layer) on the
// GIVEN node / edge features, the last layers of ONE block with P properties, cutoff-weighted edge sum:
//   atomic[i][p] = Wn[p] . hn_i + bn[p] + We[p] . (sum_e fc_e he_e) + be[p] sum_e fc_e        (backend.py:726-777)
// (the edge sum commutes with the last Linear, so it is taken on the 128 hidden columns once, not on P outputs).
// ---------------------------------------------------------------------------------
__global__ void k_fc_sum(const float* __restrict__ fc, const int* __restrict__ rowptr, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) s += fc[p];
    out[i] = s;
}
// one wave per atom: lane l owns hidden columns 2 l, 2 l + 1 of both halves; P outputs by wave reductions
__global__ void k_last_layers(const float* __restrict__ hn, const float* __restrict__ hes, const float* __restrict__ csum,
                              const float* __restrict__ nw, const float* __restrict__ nb, const float* __restrict__ ew,
                              const float* __restrict__ eb, int P, float* __restrict__ atomic, int n) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float2 a = *reinterpret_cast<const float2*>(hn + (int64_t)i * DH + 2 * lane);
    const float2 b = *reinterpret_cast<const float2*>(hes + (int64_t)i * DH + 2 * lane);
    const float cs = csum[i];
    for (int p = 0; p < P; p++) {
        const float2 wn = *reinterpret_cast<const float2*>(nw + (int64_t)p * DH + 2 * lane);
        const float2 we = *reinterpret_cast<const float2*>(ew + (int64_t)p * DH + 2 * lane);
        float v = a.x * wn.x + a.y * wn.y + b.x * we.x + b.y * we.y;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) atomic[(int64_t)i * P + p] = v + nb[p] + eb[p] * cs;
    }
}

// floats: node hidden [N, DH] | edge hidden [E, DH] | edge sums [N, DH] | fc sums [N] | scalar scratch [max(E, N)]
// (+ the adjoint's per-atom rows Gn, Ge [N, DH] each and gb [N])
int64_t predict_scratch_floats(int64_t N, int64_t E) {
    const int64_t Na = N > 0 ? N : 1, Ea = E > 0 ? E : 1;
    return 4 * Na * DH + Ea * DH + 2 * Na + (Ea > Na ? Ea : Na) + 1024;
}

int predict(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat, const float* edge_feat,
            const float* fc, float* atomic, float* node_hidden, float* edge_hidden, float* scratch, hipStream_t st) {
    if (m.generic()) return gen_predict(m, g, H, Lw, node_feat, edge_feat, fc, atomic, node_hidden, edge_hidden, st);
    const int64_t N = g.n_nodes, E = g.n_edges;
    if (N == 0) return PET_OK;
    const int64_t Ea = E > 0 ? E : 1;
    float* hid_n = node_hidden ? node_hidden : scratch;
    float* hid_e = edge_hidden ? edge_hidden : scratch + N * DH;
    float* sums = scratch + N * DH + Ea * DH;
    float* csum = sums + N * DH;
    float* ytmp = csum + N;
    if (!fc) fc = g.fc;
    // the heads' own dot-product output is not wanted here (P properties follow): any DH-vector serves as `wl`
    PET_TRY(tile_head(false, node_feat, H.nh0, H.nh2, Lw.nw, 0.f, nullptr, nullptr, ytmp, N, hid_n, DH, st));
    if (E > 0) PET_TRY(tile_head(true, edge_feat, H.eh0, H.eh2, Lw.ew, 0.f, nullptr, nullptr, ytmp, E, hid_e, DH, st));
    k_edge_sum_fc<<<cdiv(N, 4), 256, 0, st>>>(hid_e, fc, g.rowptr, sums, DH, (int)N);
    k_fc_sum<<<cdiv(N, 256), 256, 0, st>>>(fc, g.rowptr, csum, (int)N);
    k_last_layers<<<cdiv(N, 4), 256, 0, st>>>(hid_n, sums, csum, Lw.nw, Lw.nb, Lw.ew, Lw.eb, Lw.P, atomic, (int)N);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace pet
