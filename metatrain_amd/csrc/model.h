// Device-resident PET weights: raw copies keyed by the reference state-dict names
//  plus the packed / derived forms the kernels consume.
#pragma once
#include <cmath>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "common.h"
#include "switches.h"

namespace pet {

// compiled instantiation (pet/documentation.py:159-259 defaults)
constexpr int D = 128;        // d_pet
constexpr int DN = 256;       // d_node
constexpr int DFF = 256;      // d_feedforward (edge SwiGLU hidden; w_in has 2*DFF outputs)
constexpr int DNF = 2 * DN;   // node SwiGLU hidden (transformer.py:188-190: 2 * dim_node_features)
constexpr int DH = 128;       // d_head
constexpr int NHEAD = 8;
constexpr int HD = D / NHEAD; // 16
constexpr int MAX_SPECIES = 128;

// y = x W^T + b with W [n_out, k_in] (torch Linear). fwd: packed for x W^T;
// bwd: packed W^T for dx = dy W.
struct Lin {
    const float* w = nullptr;  // raw [n_out, k_in]
    const float* b = nullptr;  // raw [n_out]
    float4* fwd = nullptr;
    float4* bwd = nullptr;
    void* fwd2 = nullptr;  // f16x3 operands (trr.h): two fp16 planes, fragment order
    void* bwd2 = nullptr;
    void* fwd2s = nullptr;  // the same planes with the low piece scaled by 64 (single-accumulator products, pet_ablk.hip)
    void* bwd2s = nullptr;
    int n_out = 0, k_in = 0;
};

struct AttnLayerW {
    Lin qkv, out, mlp_in, mlp_out, cc, ce, cmlp_in, cmlp_out;
    Lin qkv_g;     // qkv with norm_attention folded in (k_ablk_bwd)
    Lin mlp_in_g;  // mlp_in with norm_mlp folded in: W diag(gamma), b + W beta (k_emlp_bwd_s works on the un-scaled normalised rows)
    const float *g_attn = nullptr, *g_mlp = nullptr, *g_center = nullptr;
    const float *b_attn = nullptr, *b_mlp = nullptr, *b_center = nullptr;  // LayerNorm biases (nullptr: RMSNorm)
};

struct GnnLayerW {
    std::vector<AttnLayerW> attn;
    Lin compress2;      // [D, D]
    Lin compress0_msg;  // columns of compress.0 that multiply the incoming message (g >= 1)
    float* wc = nullptr;   // [D, 4]  compress.0[:, :D] @ edge_embedder.weight  (4 -> D composite)
    float* wct = nullptr;  // [4, D]  transpose, for the backward dot products
    float* wcp = nullptr;  // [32, D] wct padded with zero rows to one MFMA tile
    void* wc2 = nullptr;   // f16x3 planes of wcp in fragment order (dgeo = da0 Wc as a 32-wide GEMM tile, pet_trr.hip)
    void* wc2s = nullptr;  // the same as planes of 64 w (single-accumulator products, pet_compress_s.hip)
    float* tbl = nullptr;  // [n_species, D] species part of compress.0 (+ all biases)
    Lin comb0, comb2;
    Lin comb0_g;  // comb0 with the combination LayerNorm's weight and bias folded in (k_comb_s, pet_comb_s.hip)
    const float *ln_g = nullptr, *ln_b = nullptr;
    // raw forms for the size-generic path (gen.hip): edge_embedder (4 -> d_pet), compress.0 as uploaded, neighbor_embedder
    Lin eemb, c0;
    const float* nbr_emb = nullptr;
};

// Heads of one (target, readout layer): node_heads.<t>.<l>.{0,2}, edge_heads.<t>.<l>.{0,2} (backend.py:171-217);
// last layers of one (target, readout layer, block): [P, DH] weights + [P] biases, node and edge (P = properties).
struct HeadW {
    Lin nh0, nh2, eh0, eh2;
};
struct LastW {
    const float *nw = nullptr, *nb = nullptr, *ew = nullptr, *eb = nullptr;
    int P = 0;
};

// the tuned kernels are ONE instantiation; every other size runs on the generic path (gen.hip)
inline bool compiled_size(const pet_hypers_t& h) {
    return h.d_pet == D && h.d_node == DN && h.d_feedforward == DFF && h.d_head == DH && h.num_heads == NHEAD;
}

// probe cutoffs of adaptive_cutoff_method = "grid": the count the caller made in double from the hypers as written
// (pet_hypers_t::adaptive_grid_probes), else the same formula on the float32 fields
inline int grid_probes_from_floats(const pet_hypers_t& h) {
    const double k = std::ceil(((double)h.cutoff - 0.5) / ((double)h.cutoff_width_adaptive / 4.0));
    return k < 0.0 ? 0 : k > 1e9 ? 1000000000 : (int)k;  // (far outside what is served either way)
}
inline int grid_probe_count(const pet_hypers_t& h) {
    return h.adaptive_grid_probes > 0 ? h.adaptive_grid_probes : grid_probes_from_floats(h);
}

// A LoRA adapter on one Linear "<lin>" (keys <lin>.linear.{weight,bias}, <lin>.lora_A.weight [r, k_in],
// <lin>.lora_B.weight [n_out, r]): the kernels read W_eff = W + scaling B A, folded by finalize; the reverse passes write
// dL/dW_eff into `dw` (a slice of Model::lora_grad) and lora_project() turns it into the A / B (and W) gradients.
struct LoraW {
    float scaling = 0.f;
    bool has_scaling = false;
    int rank = 0, n_out = 0, k_in = 0;
    const float *w = nullptr, *a = nullptr, *b = nullptr;  // raw base weight, A, B
    float* w_eff = nullptr;
    int64_t dw_off = 0;  // offset of dL/dW_eff in Model::lora_grad
};

struct Model {
    pet_hypers_t h;
    bool generic() const { return !compiled_size(h); }
    std::map<std::string, std::pair<float*, int64_t>> raw;  // device copies
    int* species_table = nullptr;
    int species_table_len = 0;
    std::vector<GnnLayerW> gnn;
    const float* node_emb = nullptr;  // [ns, DN]  node_embedders.0
    std::vector<const float*> node_embs;  // node_embedders.<l>: one per GNN layer for the residual featuriser, else [0]
    // architecture variants (pet_hypers_t): the TRR kernels serve RMSNorm + PreLN transformer layers only
    bool layer_norm() const { return h.normalization == PET_NORM_LAYER; }
    bool post_ln() const { return h.transformer_type == PET_POST_LN; }
    bool residual() const { return h.featurizer_type == PET_FEATURIZER_RESIDUAL; }
    bool plain_layers() const { return !post_ln(); }  // PreLN (either norm): what the TRR transformer-layer kernels serve
    bool plain() const { return plain_layers() && !residual(); }
    bool trainable() const { return !post_ln() && !residual(); }  // RMSNorm or LayerNorm, PreLN, feedforward featuriser
    int num_readout_layers() const { return residual() ? h.num_gnn_layers : 1; }
    const float* edge_emb = nullptr;  // [ns, D]
    // system conditioning (conditioning.py:38-52): embeddings [2 max_charge + 1, DN], [max_spin, DN]; project.0 [DN, 2 DN],
    // project.2 [DN, DN] as raw torch Linear weights (a per-SYSTEM MLP: a few rows, evaluated by one small kernel)
    const float *cond_qe = nullptr, *cond_se = nullptr, *cond_w0 = nullptr, *cond_b0 = nullptr, *cond_w2 = nullptr,
                *cond_b2 = nullptr;
    // the FUSED target (keys with "@" for target and block: pet_forward / the native training step): one property
    bool has_fused_head = false;
    Lin nh0, nh2, eh0, eh2;
    const float *nll_w = nullptr, *ell_w = nullptr;  // [DH]
    float nll_b = 0.f, ell_b = 0.f;
    // every head uploaded (the fused one included, under "@"), for pet_predict: key "<target>|<layer>" / "...|<block>"
    std::map<std::string, HeadW> heads;
    std::map<std::string, LastW> lasts;
    std::vector<void*> owned;  // device allocations to free
    std::map<std::string, std::pair<void*, size_t>> named;  // derived buffers, reused across finalize calls
    bool finalized = false;
    int64_t n_params = 0;
    // training (row a16): one flat gradient buffer, parameter `key` at grad_off[key] (upload order)
    std::map<std::string, int64_t> grad_off;
    float* grad_flat = nullptr;
    float* adam_m = nullptr;   // first / second moments, same layout as grad_flat
    float* adam_v = nullptr;
    float** seg_ptr = nullptr; // device table: parameter storage of segment i
    int64_t* seg_off = nullptr;  // device table: first flat index of segment i (n_seg + 1 entries)
    int n_seg = 0;
    // per segment: its key, the optimizer steps it has sat out (frozen while the others stepped: its own step count is the
    // step handed to adam_step minus this), and the (bc1, bc2_sqrt) table a step with such a segment live hands to k_adam
    std::vector<std::string> seg_keys;
    std::vector<int64_t> seg_idle;
    std::vector<float> seg_bc_host;
    float* seg_bc = nullptr;
    float* opt_scalars = nullptr;  // [4] sum of squares, clip coefficient
    // tied parameters (activation = "SiLU": w_in held as [W; W]): (flat offset, half length) pairs
    std::vector<int64_t> ties;
    bool ties_dirty = false;
    int64_t* d_ties = nullptr;
    uint8_t* d_dup = nullptr;  // [n_params] 1 on the second copy of a tied parameter
    int64_t max_tie_half = 0;
    // fine-tuning: LoRA adapters keyed by "<lin>", parameters frozen by pet_model_set_trainable
    std::map<std::string, LoraW> lora;
    float* lora_grad = nullptr;  // dL/dW_eff of every adapted Linear, cleared by every reverse entry point
    int64_t lora_floats = 0;
    std::set<std::string> lora_folded;  // adapters finalize has folded (each must meet its Linear)
    std::set<std::string> frozen;
    bool frozen_dirty = false;
    uint8_t* d_frozen = nullptr;  // [n_params] 1 on a frozen parameter's entries
    int64_t frozen_mask_n = 0;    // n_params the mask was built for
    bool is_frozen(const std::string& key) const { return !frozen.empty() && frozen.count(key) > 0; }
    // the adapter whose W_eff stands for "<lin>.weight" (nullptr: not adapted)
    const LoraW* adapter(const std::string& lin) const {
        if (lora.empty()) return nullptr;
        auto it = lora.find(lin);
        return it == lora.end() ? nullptr : &it->second;
    }
};

// some parameter outside the heads and last layers takes a gradient (false: a reverse pass may stop at the heads)
inline bool backbone_trainable(const Model& m) {
    if (m.frozen.empty()) return true;
    for (const auto& kv : m.grad_off) {
        const std::string& k = kv.first;
        const bool head = k.rfind("node_heads.", 0) == 0 || k.rfind("edge_heads.", 0) == 0 ||
                          k.rfind("node_last_layers.", 0) == 0 || k.rfind("edge_last_layers.", 0) == 0;
        if (!head && !m.is_frozen(k)) return true;
    }
    return false;
}

// lora.hip: the fold W_eff = W + s B A (finalize), the gradient projection of the reverse entry points, frozen slots
int lora_register(Model& m, const std::string& key);  // pet_model_set_param: placement check of an injected key
int lora_set_scaling(Model& m, const std::string& lin, float scaling);
// finalize: the weight and bias every raw read of Linear "<lin>" goes through (W_eff and <lin>.linear.bias when adapted)
int lora_resolve(Model& m, const std::string& lin, int n_out, int k_in, const float** w, const float** b, hipStream_t st);
int lora_check_all_folded(const Model& m, const std::set<std::string>& folded);
int lora_begin(Model& m, hipStream_t st);                           // reverse entry: clear dL/dW_eff
int lora_end(Model& m, hipStream_t st);                             // reverse exit: project, clear frozen slots
int set_trainable(Model& m, const std::string& key, bool trainable);
const uint8_t* frozen_mask(Model& m, hipStream_t st);  // nullptr: nothing frozen

// abi.hip
int dev_alloc(Model& m, void** p, size_t bytes);
int finalize(Model& m, hipStream_t st);

// optim.hip: fused clip_grad_norm_ + Adam/AdamW over the flat gradient buffer, then re-pack
int adam_step(Model& m, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
              int64_t step, float* d_grad_norm, hipStream_t st);

int tie_halves(Model& m, const std::string& key);
int optimizer_state(Model& m, float* d_m, float* d_v, int64_t numel, int direction, hipStream_t st);
int optimizer_idle_steps(Model& m, int64_t* counts, int64_t n, int direction, hipStream_t st);

// graph.hip
// na + nb <= MAILBOX_INTS - 1 device integers (two sources, either may be empty) to `out` on the host, ordered after
// everything issued on `st` so far: a one-wave kernel into the calling thread's pinned mailbox, which the host polls
constexpr int MAILBOX_INTS = 64;
int read_back(const int* d_a, int na, const int* d_b, int nb, int* out, hipStream_t st);
int64_t graph_workspace_bytes(int64_t n_nodes, int64_t e0);
int graph_attention_lists(const Graph& g, hipStream_t st);  // graph.hip: lazily, for a graph built before pet_model_finalize
int graph_build(const Model& m, const float* pos, const float* cells, const int* centers,
                const int* neighbors, const int* shifts, const int* species, const int* sys,
                int64_t n_nodes, int64_t e0, int64_t n_systems, void* ws, int64_t ws_bytes,
                Graph& g, hipStream_t st);
int graph_check_reverse(Graph& g, hipStream_t st);
int64_t graph_from_batch_workspace_bytes(int64_t n_nodes, int64_t max_nbr);
int graph_from_batch(const int64_t* el_nodes, const int64_t* el_nbr, const float* ev, const float* ed, const uint8_t* mask,
                     const int64_t* rni, const float* cf, int64_t n_nodes, int64_t max_nbr, void* ws, int64_t ws_bytes,
                     Graph& g, hipStream_t st);
int graph_export(const Graph& g, float cutoff, int64_t* el_nodes, int64_t* el_nbr, float* ev,
                 float* ed, uint8_t* mask, int64_t* rni, float* cf, float* stats, int64_t* centers,
                 int64_t* neighbors, int64_t* slot, int64_t* shifts, hipStream_t st);
int sum_over_atoms(const Graph& g, const float* atomic, float* out, hipStream_t st);

// nl.hip
int64_t nl_workspace_bytes(int64_t n_atoms);
int64_t nl_batch_workspace_bytes(int64_t n_atoms, int64_t n_systems);
int nl_build_batch(const float* d_pos, const float* h_cells, const int* h_pbc, const int64_t* h_first_atom, int64_t n_sys,
                   float cutoff, void* ws, int* d_pairs, float* d_vectors, int64_t capacity, int64_t* n_pairs,
                   hipStream_t st);
int nl_build(const float* d_pos, const float* h_cell, const int* h_pbc, int64_t n, float cutoff,
             void* ws, int* d_pairs, float* d_vectors, int64_t capacity, int64_t* n_pairs,
             hipStream_t st);

// A graph with an atom of more than 127 neighbours (attention tiles of 16 tokens, at most 8 per atom in the tuned kernels)
// runs on the size-generic path too, whatever the model size: its attention walks keys one by one, without a tile limit.
bool use_generic(const Model& m, const Graph& g);  // pet_fwd.hip

// gen.hip: the size-generic path (any d_pet / d_node / d_feedforward / d_head / num_heads; inference + dE/dR)
int64_t gen_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges);
int gen_forward_layers(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int save, float* atomic,
                       float* const* node_feats, float* const* edge_feats, int n_layers, hipStream_t st);
int gen_backward_features(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* const* g_node,
                          const float* const* g_edge, int n_layers, float* g_geo, float* g_fc, hipStream_t st);
int gen_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* gpos, float* gcell,
                 hipStream_t st);
int gen_predict(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                const float* edge_feat, const float* fc, float* atomic, float* node_hidden, float* edge_hidden,
                hipStream_t st);
int gen_predict_backward(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                         const float* edge_feat, const float* fc, const float* gA, float* g_node, float* g_edge, float* g_fc,
                         hipStream_t st);
int gen_aux_outputs(const Model& m, const Graph& g, const float* node_feat, const float* edge_feat, float* feature,
                    float* last_layer, float* scratch, hipStream_t st);
int gen_backward_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* g_node,
                         float* g_edge, float* g_fc, hipStream_t st);
int gen_backward_geometry(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_geo, const float* g_fc,
                          float* gpos, float* gcell, hipStream_t st);
// gen_train.hip: the size-generic TRAINING pass (forward-over-reverse on dual activations, any size / PostLN / residual)
int64_t gen_train_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges);
int norm_rev_rows(const float* Xp, const float* Xt, const float* gamma, int ln, float eps, const float* NYp, const float* NYt,
                  float* NXp, float* NXt, int64_t R, int W, hipStream_t st);
// Hessian-vector mode of gen_train2 (gen_hvp): no parameter gradients, the adjoints that reach the geometry are kept instead
struct HvpTaps {
    float *ngeo, *lgeo;   // (nu, lambda) of geo = (v, d) [E, 4], summed over the GNN layers
    float *sb, *sdb;      // one attention layer's key-bias adjoints per head [NH][E]
    float *db, *dbd;      // ... summed over heads and layers [E]: adjoints of b = log max(fc, 1e-15) and of b'
    float *dfc, *dfcd;    // adjoints of fc and fc' from the atom sums of the readout layers [E]
    float* dv;            // result: dJ/d(edge vector) [E, 4], last slot zero
};
// seed_node / seed_edge [n_seed] (n_seed = 0 or num_readout_layers(); NULL entries = 0): first-order feature adjoints of
// further targets, added to the nu half of every readout layer's adjoint. lA and nA both NULL: no fused target in the loss
// The long-range stage of gen_train2: the featuriser between the backbone and the heads, on a planned
// handle the caller has checked against the graph (long_range.h: lr_check). `ws` holds what gen_train.hip's lr_carve lays out: the
// operator's workspace at d_node channels (lr_workspace_bytes; with `ucell` its cell form), then the stage's dual rows; it lies
// ws_offset bytes into the d_workspace of the entry point (what a P3M handle's transform hook counts its offsets from).
// rbar [N, 3] (Hessian-vector mode only) receives the operator's own share of dJ/dR; ucell [S, 3, 3] is the operator's cell
// tangent (pet_backward_train2_long_range_cell; the backbone's is gen_train2's ucell).
struct LrStage {
    const pet_ewald_t* e;
    const float* pos;
    void* ws;
    int64_t ws_bytes;
    float* rbar;
    int64_t ws_offset;
    const float* ucell = nullptr;
};
int gen_train2(const Model& m, const Graph& g, void* ws2, int64_t ws2_bytes, const float* lA, const float* nA, const float* u,
               const float* ucell, float* tangent_atomic, hipStream_t st, const float* const* seed_node = nullptr,
               const float* const* seed_edge = nullptr, int n_seed = 0, const HvpTaps* hv = nullptr,
               const LrStage* lr = nullptr);
// The long-range forms of pet_backward_train2 and pet_hessian_vector (abi.hip checks and refuses; these carve and run), on ONE
// workspace whose layout LrSweep states for all three: the training sweep, the same with a cell tangent ucell [S, 3, 3]
// beside u (either may be null, not both: the stress term of a loss) and the Hessian-vector product.
enum LrSweep { LR_TRAIN, LR_TRAIN_CELL, LR_HVP };
int64_t lr_sweep_workspace_bytes(const Model& m, const pet_ewald_t* e, int64_t n_nodes, int64_t n_edges, LrSweep form);
// (without ucell the sweep is the one without a cell tangent, launch for launch, on either workspace)
int gen_train2_lr(const Model& m, const Graph& g, const pet_ewald_t* e, const float* pos, void* ws, int64_t ws_bytes,
                  const float* lA, const float* nA, const float* u, const float* ucell, float* tangent_atomic, hipStream_t st);
int gen_hvp_lr(const Model& m, const Graph& g, const pet_ewald_t* e, const float* pos, void* ws, int64_t ws_bytes,
               const float* lA, const float* u, float* hvp_pos, float* tangent_atomic, hipStream_t st);
// Hessian-vector product of the fused single-property target on the size-generic dual pass (pet_hessian_vector)
int64_t gen_hvp_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges);
int gen_hvp(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* lA, const float* u, const float* ucell,
            float* hvp_pos, float* hvp_cell, float* tangent_atomic, hipStream_t st);
// further targets of a training step on a size-generic training workspace (train_predict / train_predict_backward)
int gen_train_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H, const LastW& Lw,
                      float* atomic, hipStream_t st);
int gen_train_predict_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H,
                               int n_blocks, const LastW* const* Lw, const float* const* gA, float* seed_node,
                               float* seed_edge, hipStream_t st);
// a model whose TRAINING runs on the size-generic path: other sizes, PostLN layers, the residual featuriser
inline bool train_generic(const Model& m) { return m.generic() || !m.trainable(); }
// ... and for a built graph: an atom of more than 127 neighbours, or NO edge at all (a batch of isolated atoms -- reference
// structures of a dataset -- trains the node path alone; the tuned passes launch over E rows)
inline bool train_generic_for(const Model& m, const Graph& g) { return train_generic(m) || use_generic(m, g) || g.n_edges == 0; }
// the workspace `ws` was last filled by a size-generic forward (pet_fwd.hip keeps the record): its adjoints must follow
bool generic_workspace(const Graph& g, const void* ws);
int backward_geometry_generic(const Model& m, const Graph& g, float* dv_scratch, const float* dgeo, const float* dfc_a,
                              const float* dfc_b, float* gpos, float* gcell, hipStream_t st);

// pet_fwd.hip / pet_bwd.hip
int64_t forward_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges, bool train = false);
int forward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int save, float* atomic,
            float* node_feat, float* edge_feat, hipStream_t st);
int forward_layers(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int save, float* atomic,
                   float* const* node_feats, float* const* edge_feats, int n_layers, hipStream_t st);
int backward_features_layers_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* const* g_node,
                                 const float* const* g_edge, int n_layers, float* g_geo, float* g_fc, hipStream_t st);
int backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* grad_atomic,
             float* grad_pos, float* grad_cells, hipStream_t st);
int64_t predict_scratch_floats(int64_t n_nodes, int64_t n_edges);
int predict(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat, const float* edge_feat,
            const float* fc, float* atomic, float* node_hidden, float* edge_hidden, float* scratch, hipStream_t st);
int predict_backward(const Model& m, const Graph& g, const HeadW& H, const LastW& Lw, const float* node_feat,
                     const float* edge_feat, const float* fc, const float* grad_atomic, float* g_node, float* g_edge,
                     float* g_fc, float* scratch, hipStream_t st);
int aux_outputs(const Model& m, const Graph& g, const float* node_feat, const float* edge_feat, float* feature,
                float* last_layer, float* scratch, hipStream_t st);
int backward_train(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* grad_atomic,
                   float* grad_pos, float* grad_cells, hipStream_t st, const float* const* seed_node = nullptr,
                   const float* const* seed_edge = nullptr, int n_seed = 0);
// extra targets of a training step, from the features the training forward left in `ws` (pet_train_predict*)
int train_predict(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, int layer, const HeadW& H, const LastW& Lw,
                  float* atomic, hipStream_t st);
int train_predict_backward(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const std::string& target, int layer,
                           const HeadW& H, int n_blocks, const char* const* blocks, const LastW* const* Lw,
                           const float* const* gA, float* seed_node, float* seed_edge, hipStream_t st);
// llpr.hip: last-layer features of every readout layer and the four LLPR kernels (pet_hip.h, pet_llpr_*)
int llpr_features(const Model& m, const Graph& g, const char* target, const char* block, const float* const* node_feats,
                  const float* const* edge_feats, int n_layers, float* atomic, float* llf, hipStream_t st);
int llpr_rows(const float* llf, int64_t N, int F, const int* sysidx, int64_t S, const uint8_t* mask, int mean, float* rows,
              hipStream_t st);
int llpr_covariance_accumulate(const float* X, int64_t R, int F, double* C, hipStream_t st);
int llpr_covariance_finalize(double* C, int F, hipStream_t st);
int llpr_variance(const float* X, int64_t R, int F, const float* M, float alpha, float* sigma, hipStream_t st);
int llpr_ensemble(const float* X, int64_t R, int F, const float* W, int K, int P, const float* pred, float* Y, hipStream_t st);
// so.hip: second-order (force-loss) reverse pass
int64_t so_workspace_bytes(const Model& m, int64_t n_nodes, int64_t n_edges);
// tangents of (edge vector, distance), cutoff factor and key bias along (u, ucell), adaptive cutoffs ('solver') included
int geometry_tangent(const Model& m, const Graph& g, const float* u, const float* ucell, float* Tgeo, float* Tfc, float* Tkb,
                     hipStream_t st);
int backward_train2(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, void* ws2, int64_t ws2_bytes,
                    const float* lambda_atomic, const float* nu_atomic, const float* u, float* tangent_atomic,
                    hipStream_t st, const float* u_cell = nullptr, const float* const* seed_node = nullptr,
                    const float* const* seed_edge = nullptr, int n_seed = 0);
int backward_predict_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* grad_atomic,
                         float* g_node, float* g_edge, float* g_fc, hipStream_t st);
int backward_features_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_node,
                          const float* g_edge, float* g_geo, float* g_fc, hipStream_t st);
int geometry_backward(const Model& m, const Graph& g, const float* g_geo, const float* g_fc, float* gpos, float* gcell,
                      float* scratch, hipStream_t st);
int backward_geometry_abi(const Model& m, const Graph& g, void* ws, int64_t ws_bytes, const float* g_geo,
                          const float* g_fc, float* grad_pos, float* grad_cells, hipStream_t st);

// ---- the stage launchers of the tuned first-order pass are declared in pet_stages.h. Which of them serves a stage is the plan's decision
// (pet_plan.h).
bool use_trr();  // abi.hip: pet_config_set("trr") / PET_HIP_TRR (0 selects the LDS-tile kernels)
void ablk_prof_dump();  // debugging aid: per-phase cycle sums of the fused kernels (library built with -DAB_PROFILE)
// so_rows_s.hip: the generic row GEMM of the training passes with a workgroup-shared weight ring; false = not served (planes
// missing, a shape it does not tile, or fewer rows than the ring kernels' threshold)
bool rowgemm_s(hipStream_t st, const float* X, int K, const float* cs, const void* planes, const float* bias, float* Y, int n_out,
               int64_t R, bool acc);
// the same with an addend A (may be Y) and, for K == 256, a RMSNorm (norm 1) / LayerNorm (2) of the rows in front (weight cs, bias cb)
bool rowgemm_s_ex(hipStream_t st, const float* X, int K, const float* cs, const void* planes, const float* bias, const float* A,
                  float* Y, int n_out, int64_t R, int norm, const float* cb);
bool rowgemm_s_swiglu_bwd(hipStream_t st, const float* X, const void* planes, const float* VG, float* dVG, int hid, int64_t R);
bool rowgemm_s_norm_bwd(hipStream_t st, const float* X, int K, const void* planes, const float* xn, const float* gamma, int ln,
                        const float* dres, float* out, int64_t R);

// second-order attention on MFMA (training pass); false if the tile count is not served
bool attn_jvp_mfma(int nt, const float* QKV, const float* QKVd, const Graph& g, const float* Tkb, float* AOd,
                   float scale, hipStream_t st);
bool attn_rev_mfma(int nt, const float* QKV, const float* QKVd, const Graph& g, const float* Tkb, const float* LO,
                   const float* NO, float* lQKV, float* nQKV, float scale, hipStream_t st);

// abi.hip: a second HIP stream for the node-feature chain, which is independent of the edge chain
// between output_linear and the next attention layer (PET_HIP_SIDE=0 runs everything on one stream)
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t to_side = nullptr, to_main = nullptr;
    bool enabled = false;
    hipStream_t stream(hipStream_t main) const { return enabled ? s : main; }
    void fork(hipStream_t main) const;  // side waits for everything issued on main so far
    void join(hipStream_t main) const;  // main waits for everything issued on side so far
};
const SideStream& side_stream();

// profiling (abi.hip)
struct ProfScope {
    ProfScope(const char* name, hipStream_t st, double flops, double bytes = 0.0);
    ~ProfScope();
    const char* name;
    hipStream_t st;
    double flops;
    double bytes = 0.0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

}  // namespace pet

// opaque handle behind pet_graph_t (shared by abi.hip and soap.hip)
struct pet_graph {
    pet::Graph g;
    float cutoff;
    bool strict = false;  // built by a model with nl_is_strict (long_range.enable): every pair inside the cutoff is kept
};
