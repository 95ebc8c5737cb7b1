// The stage launchers of the tuned first-order PET pass (default model size), grouped by stage. The drivers (pet_fwd.hip
// forward_layers, pet_bwd.hip backward_predict / backward_features) carve, plan (pet_plan.h) and call one of these per arm of a
// stage's switch; a launcher sits next to its kernels and owns their grid, their dynamic-LDS size, the opt-in above 64 KiB of the
// instantiation it launches, and the operand forms and template choice. Families:
//   tile_*   pet_tile.hip: LDS-tile kernels on fp32 MFMA (the one fallback of every row stage; PostLN and the residual featuriser)
//   trr_*    pet_trr.hip, pet_comb.hip, pet_comb_bwd.hip: software-pipelined register-resident row kernels on f16x3 planes
//   *_s      pet_emlp_s.hip, pet_head_s.hip, pet_compress_s.hip, pet_comb_s.hip, pet_comb_bwd_s.hip, pet_center_s.hip,
//            pet_node_s.hip: the same stages (inference) with a workgroup-shared weight ring, two workgroups per CU
//   ablk_*   pet_ablk.hip: the per-atom fused attention block
//   node_*   pet_node.hip: the node update in every form of the plan's Node
//   attn_*   pet_attn.hip: the three-kernel attention
// Conventions: beta is the LayerNorm bias of the layer's norm, nullptr = RMSNorm; t_* are the operands the weight-gradient GEMMs
// need (training), nullptr otherwise -- a launcher picks the TRAIN instantiation of its kernel from whether they are given. A
// launcher returns an error only when it is called without the weight planes of its kernel.
#pragma once
#include "model.h"
#include "pet_plan.h"

namespace pet {

// ---- what the drivers share (pet_fwd.hip)
int attn_tiles(const Graph& g);    // 16-token tiles of the graph's largest atom
double g_sum_t2(const Graph& g);   // sum_i (n_i + 1)^2, for the attention FLOP figures
int exchange_forward(const Graph& g, float* XF, int layer, hipStream_t st);
int exchange_backward(const Graph& g, float* dXF, int layer, hipStream_t st);

// ---- compress: a0 = [v, d] Wc^T + Tbl[species] (+ M W0c^T); e = SiLU(a0) W2^T + b2
int tile_compress(bool first, const Graph& g, const GnnLayerW& G, const float* Min, float* a0_out, float* Xout, int64_t E,
                  hipStream_t st);
int trr_compress(bool first, const Graph& g, const GnnLayerW& G, const float* Min, float* a0_out, float* Xout, int64_t E,
                 hipStream_t st);
int tile_compress_bwd(bool first, const float* dXe, const float* a0, const GnnLayerW& G, float* dgeo, float* dM, int64_t E,
                      float* t_da0, hipStream_t st);
int trr_compress_bwd(bool first, const float* dXe, const float* a0, const GnnLayerW& G, float* dgeo, float* dM, int64_t E,
                     float* t_da0, hipStream_t st);
int compress_bwd_s(bool first, const float* dXe, const float* a0, const GnnLayerW& G, float* dgeo, float* dM, int64_t E, hipStream_t st);

// ---- centre contraction X[E + i] = H[i] Wcc^T + b, its adjoint dHin = dH1 + dC Wcc (deep: eight weight blocks in flight), and
// the expansion adjoint dOC = dH1 Wce
int tile_center(const Lin& cc, const float* H, float* Xc, int64_t N, hipStream_t st);
int center_s(const Lin& cc, const float* H, float* Xc, int64_t N, hipStream_t st);
int tile_center_bwd(bool deep, const Lin& cc, const float* dC, const float* dH1, float* dHin, int64_t N, hipStream_t st);
int center_bwd_s(const Lin& cc, const float* dC, const float* dH1, float* dHin, int64_t N, hipStream_t st);
int tile_expand_bwd(const Lin& ce, const float* dH1, float* dOC, int64_t N, hipStream_t st);
int expand_bwd_s(const Lin& ce, const float* dH1, float* dOC, int64_t N, hipStream_t st);

// ---- attention, three kernels: input_linear, softmax(QK^T + log fc) V, output_linear. post (PostLN): no norm in front of
// input_linear, every token row keeps its residual
int tile_qkv(bool post, const float* X, const float* gamma, const float* beta, const Lin& qkv, float* QKV, int64_t R, hipStream_t st);
void trr_qkv(const float* X, const float* gamma, const float* beta, const Lin& qkv, float* QKV, int64_t R, hipStream_t st);
int tile_qkv_bwd(bool post, const float* dQKV, const float* X, const float* gamma, bool layer_norm, const Lin& qkv, const float* dX1,
                 float* dXin, int64_t E, int64_t R, hipStream_t st);
void trr_qkv_bwd(const float* dQKV, const float* X, const float* gamma, bool layer_norm, const Lin& qkv, const float* dX1,
                 float* dXin, int64_t E, int64_t R, hipStream_t st);
// preload: the variants that serve at most four tiles where they can (the plan's attn_preload); nt = attn_tiles(g)
int attn_fwd(int nt, bool preload, const float* QKV, const Graph& g, float* AO, float scale, hipStream_t st);
int attn_bwd(int nt, bool preload, const float* QKV, const float* dAO, const Graph& g, float* dQKV, float* dbias_h, float scale,
             hipStream_t st);
int tile_oproj(bool post, const float* AO, const float* X, const Lin& out, float* X1, float* OC, int64_t E, int64_t R, hipStream_t st);
void trr_oproj(const float* AO, const float* X, const Lin& out, float* X1, float* OC, int64_t E, int64_t R, hipStream_t st);
int tile_oproj_bwd(const float* dX1, const float* dOC, const Lin& out, float* dAO, int64_t E, int64_t R, hipStream_t st);
void trr_oproj_bwd(const float* dX1, const float* dOC, const Lin& out, float* dAO, int64_t E, int64_t R, hipStream_t st);
// ... and in one kernel per atom (norm -> QKV -> attention -> output projection, the adjoint recomputing Q, K, V)
int ablk_fwd(const Model& m, const Graph& g, const AttnLayerW& A, const float* X, float* X1, float* OC, float scale, hipStream_t st);
int ablk_bwd(const Model& m, const Graph& g, const AttnLayerW& A, const float* X, const float* dX1, const float* dOC, float* dXin,
             float* dbias, float scale, hipStream_t st);
// key-bias adjoint of every attention layer -> cutoff-factor gradient (pet_bwd.hip)
int dfc_attn(const float* fc, const float* dbias_l, int slices, float* dfc, int64_t E, int hstep, hipStream_t st);

// ---- node update h1 = h + OC Wce^T + b, h2 = h1 + SwiGLU_MLP(Norm(h1)) in the form the plan chose. cc_next / Xcn: the next attention
// layer's centre tokens written by the same launch (the forms that can; nullptr otherwise). scratch: a buffer no kernel of the
// direction reads -- the Split form's partial outputs and, behind them, its arrival counters, which are zeroed once per pass
// (cnt_zeroed, the driver's) and then reset themselves; the Ring form's temporary
int node_fwd(Node form, const AttnLayerW& A, const float* H, const float* OC, float* H1, float* VGn, float* Hn, const Lin* cc_next,
             float* Xcn, float* scratch, bool& cnt_zeroed, int64_t N, hipStream_t st);
// dOC: the expansion adjoint, written by the forms that have it in the same launch (Split, Rows32)
int node_bwd(Node form, const AttnLayerW& A, const float* dHn, const float* H1, const float* VGn, float* dH1, float* dOC,
             float* scratch, bool& cnt_zeroed, int64_t N, bool layer_norm, float* t_dvg, hipStream_t st);
int tile_node_bwd(const AttnLayerW& A, const float* dHn, const float* H1, const float* VGn, float* dH1, int64_t N, bool layer_norm,
                  float* t_dvg, hipStream_t st);
int node_fwd_s(const AttnLayerW& A, const float* H, const float* OC, float* H1, float* VGn, float* Hn, float* tmp, int64_t N,
               hipStream_t st);
int node_bwd_s(const AttnLayerW& A, const float* dHn, const float* H1, const float* VGn, float* dH1, float* tmp, int64_t N, bool ln,
               hipStream_t st);

// ---- edge MLP X2 = X1 + SwiGLU_MLP(Norm(X1)); norm = false (PostLN): on already-normalised tokens. emlp_bwd_s recomputes [v; g]
int tile_emlp(bool norm, const float* X1, const float* gamma, const float* beta, const Lin& win, const Lin& wout, float* VG, float* X2,
              int64_t rows, hipStream_t st);
void trr_emlp(const float* X1, const float* gamma, const float* beta, const Lin& win, const Lin& wout, float* VG, float* X2,
              int64_t E, hipStream_t st);
int emlp_s(const float* X1, const float* gamma, const float* beta, const Lin& win, const Lin& wout, float* VG, float* X2,
           int64_t E, hipStream_t st);
int tile_emlp_bwd(bool norm, const float* dY, const float* X1, const float* VG, const float* gamma, bool layer_norm, const Lin& win,
                  const Lin& wout, float* dX1, int64_t rows, float* t_dvg, hipStream_t st);
void trr_emlp_bwd(const float* dY, const float* X1, const float* VG, const float* gamma, const float* beta, const Lin& win,
                  const Lin& wout, float* dX1, int64_t E, hipStream_t st, float* t_dvg = nullptr, int ldy = 128,
                  const float* dY2 = nullptr, const int* rev2 = nullptr);  // dY2: dY = dY[p] + dY2[rev2[p]], rows of ldy floats
int emlp_bwd_s(const float* dY, const float* X1, bool ln, const Lin& win_g, const Lin& wout, float* dX1, int64_t E,
               hipStream_t st, int ldy, const float* dY2, const int* rev2);
// PostLN: Y = Norm(S) row by row, rows < E to Ye, the centre rows to Yc; and its adjoint
int tile_rownorm(const float* S, const float* gamma, const float* beta, float* Ye, float* Yc, int64_t E, int64_t R, hipStream_t st);
int tile_rownorm_bwd(const float* dYe, const float* dYc, const float* S, const float* gamma, bool layer_norm, float* dS, int64_t E,
                     int64_t R, hipStream_t st);

// ---- combination stage and its adjoint (no LDS-tile form). add_dm: dcat[p][:D] += dM[p]
int trr_comb(bool first, const float* XF, const Graph& g, const GnnLayerW& G, const float* Min, const float* edge_emb, float* CA,
             float* LNS, float* Mout, int64_t E, hipStream_t st);
int comb_s(bool first, const float* XF, const int* rev, const Lin& c0g, const Lin& c2, const float* Min, const float* edge_emb,
           const int* sp_nbr, float* CA, float* LNS, float* Mout, int64_t E, hipStream_t st);
int trr_comb_bwd(const float* dM, const float* XF, const Graph& g, const GnnLayerW& G, const float* LNS, const float* CA,
                 float* dcat, int64_t E, float* t_da, hipStream_t st, bool add_dm = false);
int comb_bwd_s(const float* dM, const float* XF, const int* rev, const float* LNS, const float* CA, const Lin& c0g, const Lin& c2,
               float* dcat, int64_t E, bool add_dm, hipStream_t st);
// dXF[p] = dM[p] + dcat[p][:D] + dcat[rev[p]][D:] by a launch of its own
int tile_dxf(const float* dM, const float* dcat, const int* rev, float* dX, int64_t E, hipStream_t st);
// ... and in its place with the residual featuriser: Mout[p] = 0.5 (Min[p] + e[rev[p]]) (Min = nullptr: the edge embedding), and its adjoint
int tile_resmix(const float* Min, const float* emb, const int* sp_nbr, const float* XF, const int* rev, float* Mout, int64_t E,
                hipStream_t st);
int tile_resmix_bwd(const float* ge, const float* dMout, const int* rev, float* de, float* dMin, int64_t E, hipStream_t st);

// ---- heads y = w . SiLU(W2 SiLU(W0 x + b0) + b2) + b on node rows (K = 256) or edge rows (edge: K = 128, yout = fc y). hidden: the
// last-layer features, rows of ldh floats (or nullptr)
int tile_head(bool edge, const float* Xin, const Lin& w0, const Lin& w2, const float* wl, float bl, const float* fc, float* ypred,
              float* yout, int64_t R, float* hidden, int ldh, hipStream_t st);
int trr_head_edge(const Model& m, const float* Xin, const float* fc, float* ypred, float* yout, int64_t E, hipStream_t st);
int head_edge_s(const Model& m, const float* Xin, const float* fc, float* ypred, float* yout, int64_t E, hipStream_t st);
// Gd / gb given: the adjoint for any number of properties (k_head_bwd's GEN form)
int tile_head_bwd(bool edge, const float* Xin, const Lin& w0, const Lin& w2, const float* wl, const float* gA, const int* ctr,
                  const float* fc, const float* ypred, float* dfc, float* dXout, int64_t R, float* t_s1, float* t_da2, float* t_da1,
                  float* t_s2y, const float* Gd, const float* gb, hipStream_t st);
int trr_head_edge_bwd(const Model& m, const float* Xin, const float* gA, const int* ctr, const float* fc, const float* ypred,
                      float* dfc, float* dXout, int64_t E, float* t_s1, float* t_da2, float* t_da1, float* t_s2y, hipStream_t st);
int head_edge_bwd_s(const Model& m, const float* Xin, const float* gA, const int* ctr, const float* fc, const float* ypred,
                    float* dfc, float* dXout, int64_t E, hipStream_t st);

}  // namespace pet
