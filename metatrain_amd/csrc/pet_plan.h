// Which kernel serves every stage of the tuned first-order pass (default model size), decided once per call in one place:
// plan_forward / plan_backward (pet_plan.hip) are the only code of that pass that reads switches() to choose a kernel, compares
// a row, atom or tile count with a policy threshold, or asks whether a weight has the planes a kernel family needs. The drivers
// (pet_fwd.hip forward_layers, pet_bwd.hip backward_predict / backward_features) switch on the plan and call one launcher per arm;
// the launchers (pet_stages.h, each next to its kernels) launch: grid, dynamic LDS, opt-in, operand forms, template choice.
// DESIGN.md 4.7 has the table (stage x condition -> kernel, forward and adjoint).
#pragma once
#include <stdint.h>

#include <vector>

namespace pet {

// emlp_s = 1: the shared-ring edge kernels from this many edge rows on (the measured crossover -- 1 000 atoms, 19 k rows:
// the pipelined kernels 2 % ahead; 2 000 atoms, 38 k rows: the shared-ring ones 1 % ahead); v > 1 sets the row count itself
constexpr int64_t EMLP_S_MIN_ROWS = 28672;
// graphs of at least this many 32-slot attention tiles (about 4 700 atoms at 19 neighbours) take the fused per-atom block:
// measured crossover of one box, graph + forward + dE/dR, fused against three-kernel form -- 3 000 atoms 3.29 / 2.96 ms,
// 5 000: 4.08 / 4.16, 7 000: 5.21 / 5.51, 10 000: 6.72 / 7.30 (round 5, k_ablk_fwd4 and the VGPR-form adjoint)
constexpr int ABLK_MIN_TILES = 3840;
// the node chain's Linear layers take the ring form (k_rowlin_s) from this many atoms on; up to as many, k_node2 / k_node_bwd2 work
// on 32 rows per workgroup (measured: 1 000 / 3 000 / 10 000 atoms gain 14 / 8 / 2 %, 80 000 lose 8 % of the stage), beyond on 64
constexpr int64_t NODE_ROWS32_MAX_ATOMS = 16384;
constexpr int NODE_SPLIT_MAX_TILES = 128;         // k_node2<1, true> / k_node_bwd2<1, true>: at most this many 32-row tiles
constexpr int64_t CENTER_BWD_DEEP_MAX_ATOMS = 4096;  // k_center_bwd<DEEP>

// the kernel families of a row stage: LDS-tile kernels (pet_tile.hip; the one fallback, and the transformer layers
// of PostLN models), software-pipelined register-resident kernels on f16x3 planes (pet_trr.hip, pet_comb*.hip), kernels with a
// workgroup-shared weight ring, two workgroups per CU (pet_*_s.hip)
enum class Rows : uint8_t { LdsTile, Pipelined, Ring };
// attention layer: QKV / attention / projection as three kernels with Q, K, V in HBM (the two GEMMs of either family), or the
// per-atom fused block (pet_ablk.hip), which stores none of them
enum class Attn : uint8_t { LdsTile, Pipelined, Fused };
// node update and its adjoint: k_node / k_swiglu_bwd; k_node2w / k_node_bwd2<2> (64 rows); k_node2<1> / k_node_bwd2<1> (32 rows);
// the same with a row tile's hidden chunks on four workgroups; three ring row GEMMs beside the edge kernels (pet_node_s.hip)
enum class Node : uint8_t { LdsTile, Rows64, Rows32, Split, Ring };
// centre contraction (and, in an adjoint plan, the expansion adjoint): k_center / k_center_bwd / k_expand_bwd, k_rowlin_s, or
// written by the node kernel of the layer before (forward: center_fused) / of the same layer (adjoint: the 32-row kernels)
enum class Center : uint8_t { LdsTile, Ring, ByNode };

struct LayerPlan {  // one attention layer
    Attn attn = Attn::LdsTile;
    Rows emlp = Rows::LdsTile;
    bool emlp_saved = true;  // forward: [v; g] is stored; adjoint: it is read (false: recomputed by the ring adjoint)
    Node node = Node::LdsTile;
    Center center = Center::LdsTile;  // forward: this layer's centre tokens; adjoint: the contraction's adjoint
    Center expand = Center::LdsTile;  // adjoint only: the expansion's adjoint
};
struct GnnPlan {  // one GNN layer
    Rows compress = Rows::LdsTile;
    Rows comb = Rows::Pipelined;  // (no LDS-tile form; the residual featuriser has k_resmix in this place)
    std::vector<LayerPlan> layers;
};
// A forward plan names the forward kernels, an adjoint plan their adjoints. The forward's plan stays with its workspace
// (FwdRecord, common.h): the adjoint follows what it left unsaved.
struct StagePlan {
    std::vector<GnnPlan> gnn;
    Rows head_edge = Rows::LdsTile;
    bool side = false;        // the node chain of the layers on the second stream
    bool side_heads = false;  // ... and the node head
    bool dxf_fused = false;   // adjoint: dXF formed by the combination adjoint and the last edge-MLP adjoint, not by k_dxf
    bool center_bwd_deep = false;
    bool attn_preload = false;  // three-kernel attention: the preload variants of k_attn_fwd / k_attn_bwd where they serve the tile count
    int dbias_stride = 1;     // adjoint: slices per attention layer that k_dfc_attn skips (the fused adjoint writes the head sum)
    bool unsaved_attn() const;  // some layer ran the fused block: Q, K, V and the attention output were not written
};

struct Model;
struct Graph;
struct FwdRecord;
// (after graph_attention_lists: the fused block's policy reads the graph's tile counts)
StagePlan plan_forward(const Model& m, const Graph& g, int save);
// rec: what the forward left in the workspace (nullptr: a graph handle made anew for the adjoint -- the plan is derived as the
// forward's would be); refuses an adjoint that the switches no longer allow to follow that forward
int plan_backward(const Model& m, const Graph& g, const FwdRecord* rec, bool train, StagePlan& plan);

}  // namespace pet
