/*
 * pet_hip.h -- C ABI of libpet_hip.so: the MI355X (gfx950) hot path of metatrain's PET.
 *
 * Drop-in boundary: the plain-tensor L1 API of the reference,
 *   PETBackend.preprocess          src/metatrain/pet/modules/backend.py:238-342
 *   PETBackend.calculate_features  src/metatrain/pet/modules/backend.py:344-418
 *   PETBackend.predict             src/metatrain/pet/modules/backend.py:420-494
 *   compute_gradient (dE/dR)       src/metatrain/utils/output_gradient.py:7-63
 *   vesin.ase_neighbor_list        src/metatrain/utils/neighbor_lists.py:131-135
 * The reference is pure Python on torch; a maintainer binds this library with the
 * ctypes stub shown in INTEGRATION.md (or torch.ops via a thin TORCH_LIBRARY shim).
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory owned by the caller (e.g. a torch
 *     tensor's data_ptr()); the library never frees or retains it beyond the call,
 *     except for workspaces which the caller keeps alive while handles refer to them;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - all calls return PET_OK (0) or a negative error code; pet_last_error() returns
 *     a thread-local human-readable message for the last failure;
 *   - float data is fp32, indices are int32 unless stated otherwise;
 *   - no torch types, no host-side allocation of device memory on the hot path.
 */
#ifndef PET_HIP_H
#define PET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PET_OK 0
#define PET_ERR_HIP -1          /* a HIP runtime call failed                        */
#define PET_ERR_UNSUPPORTED -2  /* hypers outside the compiled kernel instantiation */
#define PET_ERR_ARGUMENT -3     /* bad argument / missing parameter / short buffer  */
#define PET_ERR_GRAPH -4        /* neighbour list is not a full list (no ji for ij) */

#define PET_CUTOFF_COSINE 0
#define PET_CUTOFF_BUMP 1

#define PET_NORM_RMS 0
#define PET_NORM_LAYER 1
#define PET_PRE_LN 0
#define PET_POST_LN 1
#define PET_FEATURIZER_FEEDFORWARD 0
#define PET_FEATURIZER_RESIDUAL 1
#define PET_ADAPTIVE_SOLVER 0
#define PET_ADAPTIVE_GRID 1

/* Mirrors the subset of ModelHypers that shapes the hot path
 * (src/metatrain/pet/documentation.py:159-259). */
typedef struct pet_hypers {
    float cutoff;            /* 4.5   */
    float cutoff_width;      /* 0.5   */
    int32_t cutoff_function; /* PET_CUTOFF_BUMP */
    int32_t d_pet;           /* 128   */
    int32_t d_head;          /* 128   */
    int32_t d_node;          /* 256   */
    int32_t d_feedforward;   /* 256   */
    int32_t num_heads;       /* 8     */
    int32_t num_attention_layers; /* 2 */
    int32_t num_gnn_layers;       /* 2 */
    float attention_temperature;  /* 1.0 */
    int32_t nl_is_strict;    /* = long_range.enable (backend.py:38); 0 => filter d <= cutoff */
    int32_t n_species;       /* len(atomic_types) */
    int32_t max_atomic_number; /* species_to_species_index has max+1 entries */
    float num_neighbors_adaptive; /* target neighbour count of the adaptive cutoff ("solver" method,
                                     pet/modules/adaptive_cutoff.py:110-229); <= 0: fixed cutoff */
    float cutoff_width_adaptive;  /* taper width of the adaptive-cutoff probe */
    /* the architecture variants older checkpoints use (pet/checkpoints.py:190-205 upgrades them to
     * LayerNorm + PostLN + residual); all 0 = the current defaults */
    int32_t normalization;    /* PET_NORM_RMS | PET_NORM_LAYER (transformer.py:170-176; LayerNorm: eps 1e-5, weight + bias) */
    int32_t transformer_type; /* PET_PRE_LN (transformer.py:203-234) | PET_POST_LN (transformer.py:236-262) */
    int32_t featurizer_type;  /* PET_FEATURIZER_FEEDFORWARD (backend.py:496-587) | PET_FEATURIZER_RESIDUAL (backend.py:589-649) */
    int32_t adaptive_cutoff_method; /* PET_ADAPTIVE_SOLVER (adaptive_cutoff.py:110-229) | PET_ADAPTIVE_GRID (:232-395, legacy) */
    int32_t system_conditioning;    /* 1: charge / spin-multiplicity embedding added to the node features leaving every
                                       GNN layer (conditioning.py, backend.py:121-130,517-545); needs pet_graph_set_conditioning */
    int32_t max_charge;             /* charges in [-max_charge, max_charge]   (10) */
    int32_t max_spin_multiplicity;  /* multiplicities in [1, max]             (10) */
    int32_t adaptive_grid_probes;   /* PET_ADAPTIVE_GRID: the number of probe cutoffs, len(torch.arange(0.5, cutoff,
                                       cutoff_width_adaptive / 4)) = ceil((cutoff - 0.5) / (cutoff_width_adaptive / 4)),
                                       counted by the caller IN DOUBLE from the hypers as the user wrote them: the float
                                       fields above hold 0.64 or 0.32 rounded down, and the same formula on them counts one
                                       probe too many (cutoff 4.5: 26 for 25, 51 for 50). 0: counted here from the float
                                       fields (callers from before the field existed). 2 .. 64 probes are built; any other
                                       count is PET_ERR_UNSUPPORTED at pet_model_create */
} pet_hypers_t;

typedef struct pet_model pet_model_t; /* packed weights on the device */
typedef struct pet_graph pet_graph_t; /* CSR edge graph living in a caller workspace */

/* ---- library ------------------------------------------------------------------ */
const char* pet_last_error(void);
const char* pet_version(void);
/* 1 if the default hypers instantiation (d_pet=128, d_node=256, d_ff=256, d_head=128,
 * heads=8) matches `h`, else 0. */
int pet_hypers_supported(const pet_hypers_t* h);

/* ---- model: owns device copies of the weights in MFMA fragment order ----------- */
int pet_model_create(const pet_hypers_t* h, pet_model_t** out);
void pet_model_destroy(pet_model_t* m);
/* Upload one tensor of the reference state dict (SURVEY §8(b) key schema, e.g.
 * "gnn_layers.0.trans.layers.1.mlp.w_in.weight"). `d_data` is a device pointer to
 * `numel` contiguous fp32 values (int64 values for "species_to_species_index").
 * The FUSED target (what pet_forward / the native training step evaluate; one property) is
 * uploaded with its target and block names replaced by "@" ("node_heads.@.0.0.weight" ...,
 * "node_last_layers.@.0.@.weight"); any further heads / last layers (other targets, blocks with
 * P > 1 properties, other readout layers) are uploaded under their own names and served by
 * pet_predict.
 * activation = "SiLU" (transformer.py:32-49): upload every "...w_in.weight" / "...w_in.bias" as the tensor stacked on
 * itself ([W; W], [b; b]): with equal value and gate halves the SwiGLU stage computes silu(W x + b) exactly; the
 * gradient of W is the sum of the two halves' gradients (metatrain_amd/runtime.py does both). */
int pet_model_set_param(pet_model_t* m, const char* key, const void* d_data,
                        int64_t numel, void* stream);
/* Pack / precompute derived tables once all parameters are set. */
int pet_model_finalize(pet_model_t* m, void* stream);
int64_t pet_model_num_params(const pet_model_t* m);

/* ---- neighbour list (replaces vesin at utils/neighbor_lists.py:131-135) --------- */
/* Full periodic neighbour list of ONE system within `cutoff` (strict: |D| < cutoff).
 * Two-call protocol: pass d_pairs = NULL to count; then allocate n_pairs rows.
 *   d_positions [n,3] fp32, h_cell[9] row-major lattice (host), h_pbc[3] (host)
 *   d_pairs     [n_pairs,5] int32 rows (i, j, Sa, Sb, Sc), grouped by i (CSR order)
 *   d_vectors   [n_pairs,3] fp32 D = r_j - r_i + S.cell   (may be NULL)
 *   d_workspace: pet_nl_workspace_bytes(n) bytes. */
int64_t pet_nl_workspace_bytes(int64_t n_atoms);
int pet_nl_build(const float* d_positions, const float* h_cell, const int32_t* h_pbc,
                 int64_t n_atoms, float cutoff, void* d_workspace, int32_t* d_pairs,
                 float* d_vectors, int64_t capacity, int64_t* n_pairs, void* stream);

/* All systems of a batch in one set of launches (what the reference does per system inside DataLoader workers,
 * utils/neighbor_lists.py:13-46): positions concatenated, system s owning atoms h_first_atom[s] .. h_first_atom[s+1]-1,
 * h_cells [S,9] / h_pbc [S,3] on the host. Pairs carry GLOBAL atom indices (the offsets concatenate_structures adds,
 * structures.py:81-85), grouped by centre. d_pairs = NULL counts only. With d_pairs: one call does everything when
 * `capacity` suffices; otherwise PET_ERR_ARGUMENT and *n_pairs tells the size to retry with. One device->host
 * read-back per call (two when a system has an open boundary: its bounding box). */
int64_t pet_nl_batch_workspace_bytes(int64_t n_atoms, int64_t n_systems);
int pet_nl_build_batch(const float* d_positions, const float* h_cells, const int32_t* h_pbc, const int64_t* h_first_atom,
                       int64_t n_systems, float cutoff, void* d_workspace, int32_t* d_pairs, float* d_vectors,
                       int64_t capacity, int64_t* n_pairs, void* stream);

/* ---- preprocess (replaces PETBackend.preprocess, backend.py:238) --------------- */
int64_t pet_graph_workspace_bytes(int64_t n_nodes, int64_t n_edges_in);
/* Builds edge vectors, the non-strict filter, cutoff factors, the CSR (= NEF slot)
 * order and the ij->ji map.  Inputs as in compute_batch_tensors
 * (pet/modules/structures.py:115-131): d_positions [N,3], d_cells [S,3,3],
 * d_centers/d_neighbors [E] int32 (global atom indices), d_cell_shifts [E,3] int32,
 * d_species [N] int32 atomic numbers, d_system_indices [N] int32.
 * ONE device->host read-back (kept edges, max neighbours, validation counters) happens
 * here, like the reference's int(torch.max(num_neighbors)) (structures.py:292); nothing
 * downstream (forward, reverse passes) synchronises with the host. The read-back is a one-wave
 * kernel into a pinned mailbox that the calling thread polls (under 10 us against 27 us for
 * hipMemcpyAsync + hipStreamSynchronize: it sits on the critical path of a small box's MD step).
 * A list that arrives ordered by centre with nothing to drop skips the radix sort: the first build
 * of a process asks the device, later builds assume what the build before them found and verify
 * it with the read-back above (a wrong guess costs a second build, never a wrong graph).
 * Errors: PET_ERR_GRAPH if a kept edge (i, j, S) has no partner (j, i, -S) -- every consumer
 * gathers through the ij->ji map, the reference's get_corresponding_edges (nef.py:88-166)
 * has the same precondition; PET_ERR_ARGUMENT for indices outside [0, N), atomic numbers
 * outside the model's atomic_types, or system_indices that are not non-decreasing runs
 * inside [0, n_systems). */
int pet_graph_build(const pet_model_t* m, const float* d_positions, const float* d_cells,
                    const int32_t* d_centers, const int32_t* d_neighbors,
                    const int32_t* d_cell_shifts, const int32_t* d_species,
                    const int32_t* d_system_indices, int64_t n_nodes, int64_t n_edges_in,
                    int64_t n_systems, void* d_workspace, int64_t workspace_bytes,
                    pet_graph_t** out, void* stream);
void pet_graph_destroy(pet_graph_t* g);
int64_t pet_graph_num_edges(const pet_graph_t* g);     /* kept edges E            */
int32_t pet_graph_max_neighbors(const pet_graph_t* g); /* M of the NEF grid       */
/* The 12 batch_data tensors of backend.py:328-341 in the reference's padded NEF
 * layout (pads replicate kept edge 0). int64 where the reference
 * has int64, uint8 for the bool mask. Any output pointer may be NULL. */
int pet_graph_export_batch(const pet_graph_t* g,
                           int64_t* d_element_indices_nodes,     /* [N]     */
                           int64_t* d_element_indices_neighbors, /* [N,M]   */
                           float* d_edge_vectors,                /* [N,M,3] */
                           float* d_edge_distances,              /* [N,M]   */
                           uint8_t* d_padding_mask,              /* [N,M]   */
                           int64_t* d_reverse_neighbor_index,    /* [N,M]   */
                           float* d_cutoff_factors,              /* [N,M]   */
                           float* d_atomic_cutoffs_stats,        /* [N]     */
                           int64_t* d_centers,                   /* [E]     */
                           int64_t* d_neighbors,                 /* [E]     */
                           int64_t* d_nef_to_edges_neighbor,     /* [E]     */
                           int64_t* d_cell_shifts,               /* [E,3]   */
                           void* stream);
/* CSR views for callers that want the unpadded layout (device pointers into the
 * graph workspace): rowptr [N+1], ctr/nbr/rev [E] int32. */
int pet_graph_csr(const pet_graph_t* g, const int32_t** d_rowptr, const int32_t** d_ctr,
                  const int32_t** d_nbr, const int32_t** d_rev);

/* ONE box over several GPUs with a per-layer exchange (not in the reference, which leaves large systems to the MD engine's
 * domain decomposition, pet/model.py:1004-1017). A rank's graph holds its OWNED centres with all
 * their edges plus, for every foreign neighbour j of an owned atom i, the reverse edge (j -> i) as a "ghost" row. After the
 * transformer layers of each GNN layer the library gathers the "export" rows (owned centre, foreign neighbour) of the edge
 * tokens into d_export_buf, calls fn(user, 0, layer) -- the caller's all-to-all, which must fill d_ghost_buf with the
 * owners' rows, stream-ordered on the call's stream -- and scatters d_ghost_buf into the ghost rows before the combination
 * stage reads e[reversed] (backend.py:559-575). In the reverse pass the adjoints that land on ghost rows are gathered into
 * d_ghost_buf, zeroed locally, fn(user, 1, layer) carries them home and d_export_buf is ADDED to the export rows. Halo
 * atoms need no complete neighbourhood: one cutoff of halo instead of (layers + 1). Buffers [n, d_pet] fp32; row lists are
 * CSR rows of this graph (pet_graph_csr). Default model size, PreLN + feedforward, inference + forces. fn == NULL: off. */
typedef int (*pet_exchange_fn)(void* user, int direction, int layer);
int pet_graph_set_exchange(pet_graph_t* g, const int32_t* d_export_rows, int64_t n_export, const int32_t* d_ghost_rows,
                           int64_t n_ghost, float* d_export_buf, float* d_ghost_buf, pet_exchange_fn fn, void* user);
/* system_conditioning (backend.py:375-378: batch_data["charge"], ["spin_multiplicity"], ["system_indices"]): per-system
 * total charge and spin multiplicity (2S + 1) for the forward passes on this graph handle. d_system_indices [N] may be
 * NULL for a pet_graph_build handle (it has them); the three device arrays must stay alive while the handle is used.
 * Values outside [-max_charge, max_charge] / [1, max_spin_multiplicity] are the caller's to reject (conditioning.py:54-80
 * does it on the host); the kernels clamp them.
 * Training (pet_backward_train / pet_backward_train2) sums the node-feature adjoints per system for the conditioning
 * parameters: the system indices must then be non-decreasing (what concatenate_structures produces). */
int pet_graph_set_conditioning(pet_graph_t* g, const int64_t* d_charge, const int64_t* d_spin_multiplicity,
                               const int64_t* d_system_indices, int64_t n_systems);

/* ---- features + predict + gradient -------------------------------------------- */
/* Activation workspace for one forward (+ saved tensors for the backward). */
int64_t pet_forward_workspace_bytes(const pet_model_t* m, int64_t n_nodes, int64_t n_edges);
/* The same for a built graph. The tuned kernels are one compiled model size (d_pet=128, d_node=256, d_feedforward=256,
 * d_head=128, num_heads=8) with at most 127 neighbours per atom; every other model size (the reference is size-generic,
 * pet/documentation.py:196-213; d_node == d_pet follows transformer.py:189-201) AND any graph with a denser atom (the
 * reference pads to any max(num_neighbors), pet/modules/structures.py:292-294) runs on a size-generic path with its own,
 * larger workspace layout. pet_forward_workspace_bytes answers for the model alone; a caller that may meet dense graphs
 * sizes the workspace with this function. Training of other sizes / PostLN / residual models runs on that path too
 * (pet_train_workspace_bytes answers for the model, pet_train_workspace_bytes_for / pet_train2_workspace_bytes_for for a
 * built graph: a model of the compiled size trains on a graph with a denser atom through that path as well). */
int64_t pet_forward_workspace_bytes_for(const pet_model_t* m, const pet_graph_t* g);
/* calculate_features + predict for the fused target (the heads uploaded under the name "@", one property):
 *   d_atomic [N]       per-atom prediction (node + sum of cutoff-weighted edge terms); NULL = features only
 *   d_node_features [N,d_node] / d_edge_features [E,d_pet] (CSR rows): optional copies
 *   of the backbone features (backend.py:585-586) -- may be NULL.
 * save_for_backward != 0 keeps what pet_backward needs in the workspace. */
int pet_forward(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                int64_t workspace_bytes, int save_for_backward, float* d_atomic,
                float* d_node_features, float* d_edge_features, void* stream);

/* ---- the three PETBackend calls as functions of their arguments ---------------------------------
 * pet_graph_build + pet_graph_export_batch is preprocess (backend.py:238). The two calls below take a
 * batch_data dictionary as the reference's calculate_features / predict do (backend.py:344, :420): a graph handle
 * made FROM the padded NEF tensors, whoever produced them -- this library's preprocess, the reference's, or a caller
 * that edited them in between (pet/tests/test_backend.py:122-150 is the executable spec).
 *   d_element_indices_nodes [N] i64, d_element_indices_neighbors [N,M] i64, d_edge_vectors [N,M,3] f32,
 *   d_edge_distances [N,M] f32, d_padding_mask [N,M] u8, d_reverse_neighbor_index [N,M] i64, d_cutoff_factors [N,M] f32.
 * Real slots are a prefix of each row (nef.py:63-85); CSR row of (i, slot) = rowptr[i] + slot. The handle holds
 * what features / heads and their adjoints read (rowptr, ctr, nbr, rev, species, geometry, cutoff factors); it has
 * no positions, so the geometry adjoint needs the pet_graph_build handle. One device->host read-back.
 * predict only reads the row structure and the cutoff factors: every pointer except d_padding_mask and
 * d_cutoff_factors may be NULL for a handle that is only passed to pet_predict / pet_predict_backward. */
int64_t pet_graph_from_batch_workspace_bytes(int64_t n_nodes, int64_t max_neighbors);
int pet_graph_from_batch(const int64_t* d_element_indices_nodes, const int64_t* d_element_indices_neighbors,
                         const float* d_edge_vectors, const float* d_edge_distances, const uint8_t* d_padding_mask,
                         const int64_t* d_reverse_neighbor_index, const float* d_cutoff_factors, int64_t n_nodes,
                         int64_t max_neighbors, void* d_workspace, int64_t workspace_bytes, pet_graph_t** out,
                         void* stream);
/* calculate_features alone: pet_forward with d_atomic = NULL (no heads), d_node_features / d_edge_features out.
 *
 * predict (backend.py:420-494) for ONE (target, readout layer, block) on the features the caller passes:
 *   heads node_heads.<target>.<layer> / edge_heads.<target>.<layer> (backend.py:651-687), last layers
 *   node_last_layers.<target>.<layer>.<block> / edge_... with P properties (:689-777), edge predictions weighted by the
 *   cutoff factor and summed per atom (:762-772), node + edge (:468-476). Summing over readout layers and blocks is
 *   the caller's loop, as in the reference.
 *   target / block: the names the heads were uploaded with ("@" for the fused target of pet_forward);
 *   d_node_features [N, d_node], d_edge_features [E, d_pet] (CSR rows), d_cutoff_factors [E] (NULL = the graph's),
 *   d_atomic [N, P] out; d_node_hidden [N, d_head] / d_edge_hidden [E, d_head] optional outs: the last-layer features
 *   predict returns as its 2nd / 3rd value; d_scratch: pet_predict_scratch_floats(N, E) floats. */
int32_t pet_model_block_properties(const pet_model_t* m, const char* target, int32_t readout_layer, const char* block);
int64_t pet_predict_scratch_floats(int64_t n_nodes, int64_t n_edges);
int pet_predict(const pet_model_t* m, const pet_graph_t* g, const char* target, int32_t readout_layer, const char* block,
                const float* d_node_features, const float* d_edge_features, const float* d_cutoff_factors,
                float* d_atomic, float* d_node_hidden, float* d_edge_hidden, float* d_scratch, void* stream);
/* Its adjoint, from the same inputs (the head MLPs are recomputed; nothing is read from a forward workspace):
 *   d_grad_atomic [N, P] -> d_grad_node_features [N, d_node], d_grad_edge_features [E, d_pet], d_grad_cutoff [E]. */
int pet_predict_backward(const pet_model_t* m, const pet_graph_t* g, const char* target, int32_t readout_layer,
                         const char* block, const float* d_node_features, const float* d_edge_features,
                         const float* d_cutoff_factors, const float* d_grad_atomic, float* d_grad_node_features,
                         float* d_grad_edge_features, float* d_grad_cutoff, float* d_scratch, void* stream);

/* Auxiliary per-atom outputs of pet/model.py:730-875 ("feature" and "mtt::aux::<target>_last_layer_features"),
 * from the backbone features pet_forward returned (same graph):
 *   d_feature [N, d_node + d_pet]          = [ node features | sum over edges of cutoff_factor * edge features ]
 *                                            (model.py:750-755; feedforward featuriser: the last GNN layer)
 *   d_last_layer_features [N, 2 * d_head]  = [ node-head hidden | sum over edges of cutoff_factor * edge-head hidden ]
 *                                            (model.py:795-812): the inputs of the target's last Linear layers
 * Either may be NULL. d_scratch: n_edges * d_head + max(n_edges, n_nodes) floats, needed for d_last_layer_features. */
int pet_aux_outputs(const pet_model_t* m, const pet_graph_t* g, const float* d_node_features,
                    const float* d_edge_features, float* d_feature, float* d_last_layer_features, float* d_scratch,
                    void* stream);
/* Reverse pass of the last pet_forward on (m, g, workspace):
 *   d_grad_atomic [N] = dL/d(atomic prediction) (ones => L = total energy),
 *   d_grad_positions [N,3] = dL/dR  (what compute_gradient returns; force = -grad),
 *   d_grad_cells [S,3,3] = dL/dcell through the S.cell term (may be NULL). */
int pet_backward(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                 int64_t workspace_bytes, const float* d_grad_atomic,
                 float* d_grad_positions, float* d_grad_cells, void* stream);
/* The same reverse pass split at the three PETBackend calls, so that torch autograd can chain
 * preprocess -> calculate_features -> predict as three nodes (pet/tests/test_backend.py takes
 * autograd.grad of the summed prediction w.r.t. positions and a strain tensor). Edge-shaped
 * gradients are CSR rows (row p = slot p - rowptr[ctr[p]] of atom ctr[p]).
 *   predict^T   : d_grad_atomic [N] -> d_grad_node_features [N,d_node], d_grad_edge_features
 *                 [E,d_pet], d_grad_cutoff [E] (through the cutoff weight of backend.py:768-772)
 *   features^T  : (d_grad_node_features, d_grad_edge_features) -> d_grad_geometry [E,4] =
 *                 d/d(vx,vy,vz,dist) and d_grad_cutoff [E] (through the attention key bias)
 *   preprocess^T: (d_grad_geometry, d_grad_cutoff) -> d_grad_positions [N,3], d_grad_cells */
int pet_backward_predict(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                         int64_t workspace_bytes, const float* d_grad_atomic,
                         float* d_grad_node_features, float* d_grad_edge_features,
                         float* d_grad_cutoff, void* stream);
int pet_backward_features(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                          int64_t workspace_bytes, const float* d_grad_node_features,
                          const float* d_grad_edge_features, float* d_grad_geometry,
                          float* d_grad_cutoff, void* stream);
int pet_backward_geometry(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                          int64_t workspace_bytes, const float* d_grad_geometry,
                          const float* d_grad_cutoff, float* d_grad_positions, float* d_grad_cells,
                          void* stream);

/* Every readout layer at once (backend.py:93-119: the residual featuriser reads out the features of EVERY GNN layer,
 * the feedforward one only the last: pet_model_num_readout_layers = num_gnn_layers or 1).
 *   pet_forward_layers: h_node_features[l] -> device [N,d_node], h_edge_features[l] -> device [E,d_pet] (CSR rows), two
 *     HOST arrays of n_layers device pointers (calculate_features' two lists, backend.py:344-418); no heads.
 *   pet_backward_features_layers: its adjoint for one gradient per returned tensor (NULL entries = zero). */
int32_t pet_model_num_readout_layers(const pet_model_t* m);
int pet_forward_layers(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                       int save_for_backward, float* const* h_node_features, float* const* h_edge_features,
                       int32_t n_layers, void* stream);
int pet_backward_features_layers(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                                 const float* const* h_grad_node_features, const float* const* h_grad_edge_features,
                                 int32_t n_layers, float* d_grad_geometry, float* d_grad_cutoff, void* stream);

/* preprocess^T without a forward workspace (the autograd node of preprocess on its own):
 * d_scratch: 4 * n_edges floats. Needs the pet_graph_build handle (positions, shifts). */
int pet_geometry_backward(const pet_model_t* m, const pet_graph_t* g, const float* d_grad_geometry,
                          const float* d_grad_cutoff, float* d_grad_positions, float* d_grad_cells, float* d_scratch,
                          void* stream);

/* ---- training step (trainer.py:391-480) ---------------- */
/* Served architectures: transformer_type = PreLN with the feed-forward featuriser; normalization RMSNorm or LayerNorm,
 * activation SwiGLU or SiLU, system conditioning on or off. PostLN / residual models: PET_ERR_UNSUPPORTED from
 * pet_forward(save_for_backward = 2) and from the two training reverse passes. */
/* The model owns one gradient slot per uploaded parameter (same numel, fp32).
 * pet_model_zero_grad allocates (first call) and clears them -- optimizer.zero_grad(). */
int pet_model_zero_grad(pet_model_t* m, void* stream);
/* Copy the accumulated gradient of parameter `key` (same key as pet_model_set_param) into d_dst. */
int pet_model_get_grad(const pet_model_t* m, const char* key, float* d_dst, int64_t numel,
                       void* stream);
/* Current value of parameter `key` (after optimizer steps). */
int pet_model_get_param(const pet_model_t* m, const char* key, float* d_dst, int64_t numel,
                        void* stream);
/* The gradient slots as ONE flat fp32 buffer of pet_model_num_params elements (upload order):
 * direction 0 copies it out to d_flat, 1 copies d_flat back in. This is the bucket the RCCL
 * gradient all-reduce runs on (torch DDP's role, pet/trainer.py:344-345): 11.6 MB, one collective. */
int pet_model_flat_grad(pet_model_t* m, float* d_flat, int64_t numel, int direction, void* stream);
/* clip_grad_norm_(max_grad_norm; <= 0: off) + torch.optim.Adam (weight_decay < 0) or AdamW
 * (weight_decay >= 0) on every parameter, `step` counted from 1 (pet/trainer.py:367-376,463-467),
 * then re-packs the weights. d_grad_norm (device, may be NULL) receives the pre-clip total norm.
 * `step` is the step count of a parameter that has taken part in every step. torch counts per parameter and only the
 * steps in which it has a .grad, so the model keeps, per parameter, the number of calls it sat out frozen
 * (pet_model_set_trainable) and gives it the bias correction of `step` minus that number: a parameter turned on after k
 * steps starts at step 1, one that skipped a step lags one behind. */
int pet_adam_step(pet_model_t* m, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float max_grad_norm, int64_t step, float* d_grad_norm, void* stream);
/* Adam's first / second moments as two flat fp32 buffers of pet_model_num_params elements in upload order (the layout
 * of pet_model_flat_grad): direction 0 copies them out, 1 copies them in. With the step counter this is the
 * optimizer_state_dict a checkpoint keeps (pet/trainer.py:697-717, trainer checkpoint v15). */
int pet_optimizer_state(pet_model_t* m, float* d_m, float* d_v, int64_t numel, int direction, void* stream);
/* The third part of that state: per uploaded float parameter, in upload order, the number of pet_adam_step calls it sat
 * out frozen (HOST array `counts` of `n` = number of such parameters; direction 0 copies out, 1 copies in). A model that
 * was never told starts with zeros: every parameter takes the bias correction of `step`. */
int pet_optimizer_idle_steps(pet_model_t* m, int64_t* counts, int64_t n, int direction, void* stream);
/* Declare parameter `key` (uploaded as a tensor stacked on itself, see pet_model_set_param) TIED: pet_adam_step sums
 * the gradient slots of its two halves, counts the parameter once in the clipping norm and gives both halves the same
 * update, so that they stay equal. */
int pet_model_tie_halves(pet_model_t* m, const char* key);
/* ---- fine-tuning (pet/modules/finetuning.py) ---- */
/* LoRA adapters. pet_model_set_param accepts the keys of a LoRA-injected Linear "<lin>" = gnn_layers.<g>.trans.layers.<a>.
 * {attention.input_linear, attention.output_linear, mlp.w_in, mlp.w_out, center_mlp.w_in, center_mlp.w_out,
 * center_contraction, center_expansion}: <lin>.linear.weight / .linear.bias (the base Linear), <lin>.lora_A.weight [r, k_in]
 * and <lin>.lora_B.weight [n_out, r], rank r in 1 .. 64. They are ordinary parameters (gradient slots, Adam moments, places
 * in the flat buffers, upload order). Adapter keys elsewhere: PET_ERR_UNSUPPORTED naming the key. The scale s = alpha / rank
 * is not in the state dict: pet_model_set_lora_scaling(m, "<lin>", s). pet_model_finalize folds W_eff = W + s B A (fp64,
 * deterministic) and builds every packed form from it (PET_ERR_ARGUMENT: no scaling, or A / B do not fit the base Linear;
 * PET_ERR_UNSUPPORTED: a larger rank, or an adapter on a tied w_in -- activation = "SiLU"); the training reverse passes
 * give lora_A dL/dA = s B^T dL/dW_eff and lora_B dL/dB = s dL/dW_eff A^T. pet_model_get_param("<lin>.linear.weight")
 * is the base W. */
int pet_model_set_lora_scaling(pet_model_t* m, const char* lin, float scaling);
/* Frozen parameters (requires_grad = False; default: everything trainable). A frozen parameter's gradient slot stays zero
 * after the training reverse passes, it is left out of the clipping norm, and pet_adam_step leaves it and its moments
 * untouched (torch's optimizers skip a parameter without .grad). The weight-gradient work of frozen parameters is skipped. */
int pet_model_set_trainable(pet_model_t* m, const char* key, int trainable);
/* Workspace for pet_forward(save_for_backward = 2) + pet_backward_train. */
int64_t pet_train_workspace_bytes(const pet_model_t* m, int64_t n_nodes, int64_t n_edges);
int64_t pet_train_workspace_bytes_for(const pet_model_t* m, const pet_graph_t* g);   /* graph-aware (dense atoms) */
/* Reverse pass of loss.backward() for L with dL/d(atomic prediction) = d_grad_atomic [N]:
 * accumulates dL/dtheta into the model's gradient slots; d_grad_positions [N,3] (and d_grad_cells)
 * may be NULL. Needs pet_forward(save_for_backward = 2) on a training workspace. */
int pet_backward_train(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                       int64_t workspace_bytes, const float* d_grad_atomic,
                       float* d_grad_positions, float* d_grad_cells, void* stream);
/* Second-order reverse pass for losses on dE/dR (forces), i.e. what loss.backward() does through the
 * create_graph=True gradient of evaluate_model(is_training=True) (pet/trainer.py:417-462):
 *   d_lambda_atomic [N]  seeds the force pass used (grad_outputs of autograd.grad: ones),
 *   d_nu_atomic [N]      dL/d(atomic prediction) of the energy term (may be NULL = 0),
 *   d_u [N,3]            dL/d(dE/dR),
 *   d_tangent_atomic [N] optional out: directional derivative of every atomic prediction along dR = u.
 * Accumulates dL/dtheta into the gradient slots. Needs pet_forward(save_for_backward = 2) on a
 * training workspace plus a second workspace of pet_train2_workspace_bytes. */
int64_t pet_train2_workspace_bytes(const pet_model_t* m, int64_t n_nodes, int64_t n_edges);
int64_t pet_train2_workspace_bytes_for(const pet_model_t* m, const pet_graph_t* g);  /* graph-aware (dense atoms) */
int pet_backward_train2(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                        int64_t workspace_bytes, void* d_workspace2, int64_t workspace2_bytes,
                        const float* d_lambda_atomic, const float* d_nu_atomic, const float* d_u,
                        float* d_tangent_atomic, void* stream);
/* The same with a tangent of the CELLS as well (a stress / strain-gradient term in the loss, utils/evaluate_model.py:
 * 305-321: positions @ strain, cell @ strain under create_graph): the sweep runs along (dR, dcell) = (d_u [N,3],
 * d_u_cell [S,3,3]) with u = dL/d(dE/dR), u_cell = dL/d(dE/dcell); d_u_cell = NULL is pet_backward_train2. */
int pet_backward_train2_cell(const pet_model_t* m, const pet_graph_t* g, void* d_workspace,
                             int64_t workspace_bytes, void* d_workspace2, int64_t workspace2_bytes,
                             const float* d_lambda_atomic, const float* d_nu_atomic, const float* d_u,
                             const float* d_u_cell, float* d_tangent_atomic, void* stream);
/* ---- further targets of a training step (non-conservative forces / stress, several blocks or properties) --------------
 * A step trains every target from ONE pet_forward(save_for_backward = 2) and ONE backbone reverse sweep:
 *   1. pet_train_predict: the prediction of one (target, readout layer, block) from the features that forward left in
 *      the training workspace (no second backbone forward): d_atomic [N, P] out. target / block as in pet_predict.
 *   2. pet_train_predict_backward: for the seeds d_grad_atomic[b] = dL/d(prediction of blocks[b]) [N, P_b] of some blocks
 *      of one target, ADDS dL/dtheta of the target's heads (recomputed once for all its blocks) and of those blocks' last
 *      layers to the gradient slots, and ADDS the adjoints of the heads' inputs to d_seed_node_features [N, d_node] and
 *      d_seed_edge_features [E, d_pet] (CSR rows; either may be NULL). Frozen parameters get no gradient (the tuned
 *      pass skips them; the size-generic pass clears their slots when the seeded call of step 3 returns).
 *   3. pet_backward_train_seeded / pet_backward_train2_seeded: pet_backward_train / pet_backward_train2_cell with the
 *      summed seeds of step 2 (h_seed_*_features: host arrays of n_layers device pointers, one per readout layer, NULL
 *      entries = 0; n_layers = 0: none) added where the fused head's adjoint enters the backbone (the second-order pass:
 *      its first-order adjoint only; these targets do not enter dE/dR). pet_backward_train_seeded takes
 *      d_grad_atomic = NULL when the loss has no fused target (a model loaded without one trains this way). The seeds
 *      carry no cutoff-factor adjoint, so pet_backward_train_seeded refuses d_grad_positions / d_grad_cells with seeds.
 * Every model and graph that trains: the tuned pass, and the size-generic pass (other sizes, PostLN, the residual
 * featuriser, an atom with more than 127 neighbours, a batch without any edge). readout_layer < the model's number of
 * readout layers (pet_model_num_readout_layers; the residual featuriser has one per GNN layer): the prediction of a block
 * is the SUM over the readout layers of pet_train_predict, so one dL/d(prediction) seeds every layer, step 2 runs once per
 * layer into that layer's seed pair, and step 3 takes n_layers = the number of readout layers (any other count but 0 is
 * PET_ERR_ARGUMENT). pet_backward_train / pet_backward_train2_cell are the seeded calls with no seed. */
int pet_train_predict(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                      const char* target, int32_t readout_layer, const char* block, float* d_atomic, void* stream);
int pet_train_predict_backward(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                               const char* target, int32_t readout_layer, int32_t n_blocks, const char* const* blocks,
                               const float* const* d_grad_atomic, float* d_seed_node_features,
                               float* d_seed_edge_features, void* stream);
int pet_backward_train_seeded(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                              const float* d_grad_atomic, float* d_grad_positions, float* d_grad_cells,
                              const float* const* h_seed_node_features, const float* const* h_seed_edge_features,
                              int32_t n_layers, void* stream);
int pet_backward_train2_seeded(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                               void* d_workspace2, int64_t workspace2_bytes, const float* d_lambda_atomic,
                               const float* d_nu_atomic, const float* d_u, const float* d_u_cell, float* d_tangent_atomic,
                               const float* const* h_seed_node_features, const float* const* h_seed_edge_features,
                               int32_t n_layers, void* stream);
/* ---- Hessian-vector products of the fused single-property target (second derivatives w.r.t. positions and cells) ------
 * With e_i the per-atom predictions and e'_i = d/d eps e_i(R + eps u, cell + eps u_cell):
 *   d_hvp_positions [N,3] = grad_R    sum_i lambda_i e'_i      (lambda = ones: H u of the total energy, H = d2E/dR dR,
 *   d_hvp_cells [S,3,3]   = grad_cell sum_i lambda_i e'_i       and its mixed position / cell blocks),
 *   d_tangent_atomic [N]  = e'_i  (so that sum_i lambda_i e'_i = <u, dE_lambda/dR> + <u_cell, dE_lambda/dcell>).
 * d_lambda_atomic NULL = ones; d_u_cell, d_hvp_cells and d_tangent_atomic may be NULL (a cell direction or a cell result
 * needs a pet_graph_build handle, for the cell shifts). No pet_forward and no pet_model_zero_grad is needed, and no
 * gradient slot is touched: the call evaluates the model itself, as a dual (primal, tangent) forward along (u, u_cell)
 * and a joint reverse sweep down to the geometry. It runs on the SIZE-GENERIC kernels of the training pass for every
 * model and graph that pass serves -- every size (the default size included: there is no tuned Hessian-vector path),
 * PreLN / PostLN, both featurisers, both normalisations, system conditioning, any number of neighbours per atom -- in
 * fp32 FMA with fixed summation orders and no float atomics (the same bits run to run).
 * PET_ERR_UNSUPPORTED: an adaptive-cutoff model (the second-order implicit derivative of the cutoff solver is not built)
 * and a graph with a per-layer exchange (pet_graph_set_exchange). A batch without edges and empty systems give zeros.
 * The ZBL term (pet_zbl_*) is not part of it: pet_zbl_hessian_vector is the same product of the pair term, and the two add
 * (the network's after the scaler's factor, the pair term's as it is). */
int64_t pet_hvp_workspace_bytes_for(const pet_model_t* m, const pet_graph_t* g);
int pet_hessian_vector(const pet_model_t* m, const pet_graph_t* g, void* d_workspace, int64_t workspace_bytes,
                       const float* d_lambda_atomic, const float* d_u, const float* d_u_cell, float* d_hvp_positions,
                       float* d_hvp_cells, float* d_tangent_atomic, void* stream);
/* Per-system sum (utils/sum_over_atoms.py:10-48): d_out[S] = sum_{atoms of s} d_atomic. */
int pet_sum_over_atoms(const pet_graph_t* g, const float* d_atomic, float* d_out, void* stream);

/* ---- LLPR: last-layer prediction rigidity (llpr/model.py) ------------------------------------------------------
 * Uncertainties and last-layer ensembles from the last-layer features (LLF) of one target. F = 2 L d_head with
 * L = pet_model_num_readout_layers (pet/model.py:118-120); every entry point below checks F against the model.
 * All products are fp32 MFMA, every sum has a fixed order: results are the same bits run to run. Arguments are checked
 * on the host before any launch: NULL buffers, a wrong F, R <= 0 or K P above PET_LLPR_MAX_ENSEMBLE give PET_ERR_ARGUMENT.
 *
 * pet_llpr_features: per-atom LLF [N, F] of (target, block) -- the names the heads were uploaded with, "@" for the
 *   fused target -- from the features of every readout layer (pet_forward / pet_forward_layers outputs, two HOST arrays
 *   of n_layers device pointers). Columns node0 | edge0 | node1 | edge1 | ... (the concatenation of
 *   last_layer_parameter_names, pet/model.py:788-875, 1064-1072); each edge part is the cutoff-weighted sum over the
 *   atom's edges. d_atomic [N, P] optional out: the target's prediction, summed over readout layers (backend.py:468-476).
 * pet_llpr_rows: d_rows [S, F] = per-system sums of d_llf [N, F] over the atoms whose d_mask [N] byte is non-zero (NULL =
 *   all; selected_atoms), divided by the system's atom count when mean != 0 (covariance rows, llpr/model.py:898-908).
 *   d_system_indices [N] int32: non-decreasing runs inside [0, S), as pet_graph_build requires.
 * pet_llpr_covariance_accumulate: d_cov [F, F] fp64 += X^T X for X = d_x [R, F] (llpr/model.py:912). Only the upper
 *   triangle (by 64-column tiles) is accumulated: call pet_llpr_covariance_finalize once after the last batch to mirror it.
 * pet_llpr_variance: d_sigma [R] = alpha sqrt(|M x_r|^2) with d_inv_cholesky M = L^-1 [F, F] lower triangular, zeros
 *   above the diagonal (llpr/model.py:427-436: solve_triangular(L, x) then the sum of squares; alpha: the multiplier).
 * pet_llpr_ensemble: d_out [R, K P] = X W^T with d_weights W [K P, F] (llpr_ensemble_layers.<target>.weight, member-major
 *   index k P + p, llpr/model.py:1125-1138), then, when d_prediction [R, P] is given, re-centred on it:
 *   out - mean_k out + prediction (llpr/model.py:578-587). */
#define PET_LLPR_MAX_ENSEMBLE 16384
int64_t pet_llpr_feature_size(const pet_model_t* m);
int pet_llpr_features(const pet_model_t* m, const pet_graph_t* g, const char* target, const char* block,
                      const float* const* h_node_features, const float* const* h_edge_features, int32_t n_layers,
                      float* d_atomic, float* d_llf, void* stream);
int pet_llpr_rows(const pet_model_t* m, int64_t F, const float* d_llf, int64_t n_atoms, const int32_t* d_system_indices,
                  int64_t n_systems, const uint8_t* d_mask, int mean, float* d_rows, void* stream);
int pet_llpr_covariance_accumulate(const pet_model_t* m, int64_t F, const float* d_x, int64_t R, double* d_cov,
                                   void* stream);
int pet_llpr_covariance_finalize(const pet_model_t* m, int64_t F, double* d_cov, void* stream);
int pet_llpr_variance(const pet_model_t* m, int64_t F, const float* d_x, int64_t R, const float* d_inv_cholesky,
                      float alpha, float* d_sigma, void* stream);
int pet_llpr_ensemble(const pet_model_t* m, int64_t F, const float* d_x, int64_t R, const float* d_weights, int32_t K,
                      int32_t P, const float* d_prediction, float* d_out, void* stream);

/* ---- ZBL short-range repulsion (utils/additive/zbl.py): the additive model of `zbl: true` ----------------------------
 * e(r) = 1/2 [E(r) + A/3 r^3 + B/4 r^4 + C] for r <= rc = rad(Zi) + rad(Zj), else 0, E(r) = K Zi Zj / r * phi(r / a)
 * (LAMMPS pair_style zbl with inner cutoff 0; eV and Angstrom). Per-atom energies a_i = sum over the CSR row of atom i.
 * The pair term is evaluated in fp64, rows are summed in edge order in fp64, outputs are fp32; no atomics: every result
 * is the same bits run to run, and a system gives the same bits alone as inside a batch.
 *   pet_zbl_create: h_atomic_types [n_types] = the atomic_types of the model that builds the graphs, in the same order
 *     (the graph's species indices index it); h_covalent_radii [n_types] in Angstrom. Builds the [n_types, n_types, 6]
 *     fp64 table (rc, 1/a, K Zi Zj, A, B, C) on the host. Neither it nor pet_zbl_pair_table needs a GPU.
 *   pet_zbl_cutoff: 2 * the largest radius = the range a neighbour list must cover (full list).
 *   pet_zbl_forward: d_atomic [N]. pet_zbl_backward: d_grad_atomic [N] = dL/d(a_i), NULL = ones;
 *     d_grad_positions [N,3] = dL/dR; d_grad_cells [S,3,3] = dL/dcell through the S.cell term (may be NULL);
 *     d_grad_strain [S,3,3] = dE/d(strain) = R^T dE/dR + cell^T dE/dcell formed directly from the edge vectors (may be
 *     NULL; unit weights only: PET_ERR_ARGUMENT together with d_grad_atomic). The pair terms are recomputed: nothing is
 *     kept between the two calls. d_workspace: pet_zbl_workspace_bytes(N, S) bytes, needed for either 3x3 output.
 *   pet_zbl_hessian_vector: the second derivatives of E_lambda = sum_i lambda_i a_i along (u [N,3], u_cell [S,3,3]), in the
 *     convention of pet_hessian_vector. With D = R_j - R_i + S . cell_s and D' = u_j - u_i + S . u_cell_s per edge,
 *       q = D . D',  f = e'(r) / r,  t = f D' + ((e''(r) - f) / r^2) q D                    (the tangent of f D)
 *       E''(r) = K Zi Zj (phi''/r - 2 phi'/r^2 + 2 phi/r^3),  e'' = 1/2 (E'' + 2 A r + 3 B r^2) for r <= rc, 0 beyond,
 *       d_hvp_positions [N,3]: (H u)_k = -sum_{row k} (lambda_k + lambda_nbr) t        (row-local: the list is full)
 *       d_hvp_cells [S,3,3]:   (H u)_ab =  sum_{edges of the system} lambda_i S_a t_b   (may be NULL)
 *       d_tangent_atomic [N]:  e'_i = sum_{row i} f q = d/d(lambda_i) of the contracted gradient (may be NULL)
 *     d_lambda_atomic NULL = ones, d_u_cell NULL = zero. e', e'', D', q and t are fp64 (S . u_cell too), rows are summed as in
 *     the other two launches. An edge from an atom to its own image contributes to the cell block and the tangent only (it
 *     depends on no position). d_workspace: pet_zbl_workspace_bytes(N, S) bytes, needed for d_hvp_cells only. NULL z, g,
 *     d_u or d_hvp_positions: PET_ERR_ARGUMENT. Third derivatives are not built.
 * The launches run on the caller's stream without a synchronisation, with one exception: the FIRST launch on a device
 * uploads the table and the radii (two allocations kept until pet_zbl_destroy, two blocking copies that have completed
 * before any thread or stream can see the entry), so it must not sit inside a stream capture. Later ones allocate nothing.
 * PET_ERR_ARGUMENT: a graph whose cutoff is below pet_zbl_cutoff, a graph built under an adaptive cutoff (it drops edges
 * inside the range), a pet_graph_from_batch handle (no shifts / system indices). */
typedef struct pet_zbl pet_zbl_t;
int pet_zbl_create(const int32_t* h_atomic_types, const double* h_covalent_radii, int32_t n_types, pet_zbl_t** out);
void pet_zbl_destroy(pet_zbl_t* z);
double pet_zbl_cutoff(const pet_zbl_t* z);
int pet_zbl_pair_table(const pet_zbl_t* z, double* h_out);
int64_t pet_zbl_workspace_bytes(int64_t n_nodes, int64_t n_systems);
int pet_zbl_forward(const pet_zbl_t* z, const pet_graph_t* g, float* d_atomic, void* stream);
int pet_zbl_backward(const pet_zbl_t* z, const pet_graph_t* g, const float* d_grad_atomic, float* d_grad_positions,
                     float* d_grad_cells, float* d_grad_strain, void* d_workspace, int64_t workspace_bytes, void* stream);
int pet_zbl_hessian_vector(const pet_zbl_t* z, const pet_graph_t* g, const float* d_lambda_atomic, const float* d_u,
                           const float* d_u_cell, float* d_hvp_positions, float* d_hvp_cells, float* d_tangent_atomic,
                           void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Long-range (Ewald) features of `long_range: {enable: true}` (utils/long_range.py:108-195, pet/model.py:505-518) ---------
 * A periodic Coulomb sum over C channels of per-atom "charges" q [N, C], with its adjoints. torch-pme is not part of the
 * reference tree: the operator is fixed HERE by definition (DESIGN section 18 holds the same convention table) and pinned to
 * an independent fp64 oracle; parity with torch-pme is NOT pinned.
 *   sigma = smearing, R = the model cutoff (exclusion radius), lambda = kspace_resolution, Omega = |det cell|, a = sqrt(2) sigma,
 *   f(d) = (1 + cos(pi d / R)) / 2 for d < R, else 0,   G(k) = 4 pi exp(-sigma^2 k^2 / 2) / k^2,   P = 1/2 (prefactor).
 * Periodic system (all three pbc):
 *   V_i = P [ (1/Omega) sum_{k != 0, |k| <= 2 pi / lambda} G(k) Re(e^{-i k.r_i} S(k)) - q_i sqrt(2/pi)/sigma
 *             - (2 pi sigma^2 / Omega) sum_j q_j - sum_{edges (i -> j, S) of the graph} q_j w(d) ],
 *   S(k) = sum_j q_j e^{i k.r_j},  w(d) = erf(d/a) f(d) / d,  k over the reciprocal lattice 2 pi n cell^{-T} (a sphere).
 * Non-periodic system (no pbc): V_i = P sum_{j != i} q_j K(d_ij) over ALL pairs of the system, K(d) = (1 - f(d)) / d.
 * Mixed pbc: PET_ERR_UNSUPPORTED from pet_ewald_plan.
 * Adjoints, for L with dL/dV = g [N, C] (the operator is symmetric in (i, j): the neighbour list is full):
 *   dL/dq = the operator applied to g.
 *   With T(k) = sum_i g_i e^{i k.r_i}, c_ik = cos k.r_i, s_ik = sin k.r_i (per channel, summed over channels below):
 *   k-space:   F_i = (P/Omega) sum_k G k [ g_i (c_ik Im S - s_ik Re S) + q_i (c_ik Im T - s_ik Re T) ],  dL/dR_i += F_i
 *              Z_k = Re(conj(T) S);  dL/dcell_bc += -sum_i s_ib F_ic          (s_i = r_i cell^{-1}: the phases through k)
 *                                  + (P/Omega) sum_k G Z_k [ (sigma^2 + 2/k^2) (cell^{-T} k)_b k_c - (cell^{-T})_bc ]
 *   background: dL/dcell_bc += (2 pi sigma^2 P / Omega) (sum_i g_i).(sum_j q_j) (cell^{-T})_bc
 *   exclusion: per edge p = (i -> j, S), D = r_j - r_i + S.cell, B_p = g_i.q_j, B'_p = g_j.q_i, w' = dw/dd:
 *              dL/dR_i += P sum_{row i, j != i} w'(d) (B_p + B'_p) D/d,   dL/dcell_ab += -P sum_p w'(d) B_p S_a D_b / d
 *              (an edge from an atom to its own image moves with the cell only)
 *   non-periodic: dL/dR_i = -P sum_{j != i} K'(d) (g_i.q_j + g_j.q_i) (r_j - r_i)/d.
 * Kernels (csrc/ewald.hip; the local terms, shared with P3M mode, in csrc/long_range.h): structure factors, the gather back to atoms and the all-pairs sum are GEMMs on the fp32 matrix
 * core (v_mfma_f32_32x32x2_f32) with one operand GENERATED in registers -- phases as products of per-axis tables
 * e^{2 pi i n s_a}, built in fp64 from fractional coordinates and rounded once; cos(k.r) of a large fp32 argument is never
 * formed. Sums over atoms and over k run in fixed-order chunks relative to the system's first atom / first k-vector, the
 * exclusion term is a CSR row sum; no float atomics: the same bits run to run, and a system gives the same bits alone as
 * inside a batch.
 *   pet_ewald_create(smearing, kspace_resolution, cutoff).
 *   pet_ewald_kvectors_host: the k-set of one cell, host fp64, no GPU: returns the count and fills h_out [count, 3] when
 *     capacity suffices (h_out may be NULL to count); -1 for a singular cell.
 *   pet_ewald_plan: h_cells [S,3,3] fp64, h_pbc [S,3], h_first_atom [S+1] on the host. Builds the per-system k lists in fp64
 *     and uploads them (allocations kept until the next plan / destroy; blocking host-to-device copies, no read-back). The
 *     plan is valid while the cells and the batch layout do not change (every step of fixed-cell MD). Not inside a capture.
 *   pet_ewald_num_kvectors: k-vectors of system s (0 for a non-periodic one); the kernels walk one of every pair (k, -k).
 *   pet_ewald_potential: d_positions [N,3], d_charges [N,C] -> d_potential [N,C], any C >= 1.
 *   pet_ewald_backward: d_grad_potential [N,C] -> d_grad_charges [N,C], d_grad_positions [N,3], d_grad_cells [S,3,3] (may be
 *     NULL): dL/dcell at fixed Cartesian positions. Nothing is kept between the two calls.
 *   d_workspace: pet_ewald_workspace_bytes(e, C) bytes (after the plan). No host synchronisation after the plan.
 * Second derivatives (pet_ewald_second). Per system V = A(r) q with A symmetric, Phi(r; g, q) = sum_c g_c^T A q_c,
 * and the adjoint above returns gq = A g, gpos = grad_r Phi. For cotangents u_q [N, C] of gq and u_r [N, 3] of gpos,
 *   Psi = <u_q, A g> + <u_r, grad_r Phi(r; g, q)>, and the call returns
 *   d_out_grad_potential = dPsi/dg = A u_q + (D_u A) q,     d_out_charges = dPsi/dq = (D_u A) g,
 *   d_out_positions      = dPsi/dr = grad_r Phi(r; u_q, g) + H_Phi(r; g, q) u_r,
 *   D_u A = sum_i u_r,i . grad_{r_i} A (the directional derivative of A along u_r), H_Phi the position Hessian of Phi.
 *   The same outputs serve forward mode: d/dt (A q) = A q' + (D_r' A) q is d_out_grad_potential with u_q = q', u_r = r'.
 *   With e_ij = u_j - u_i, n = D / d and M_phi = phi''(d) n n^T + (phi'(d) / d) (I - n n^T):
 *   k-space (half the k-set, w = 2 G / Omega, c, s = cos, sin k.r_i, S'_X = w sum_j X_j e^{i k.r_j},
 *            S'_{uX} = w sum_j (k.u_j) X_j e^{i k.r_j}):
 *     (D_u A X)_i = -P sum_k [ (c Im S'_{uX} - s Re S'_{uX}) - (k.u_i) (c Im S'_X - s Re S'_X) ]
 *     (H u)_i     =  P sum_k k { g_i . [ (c Re S'_{uq} + s Im S'_{uq}) - (k.u_i) (c Re S'_q + s Im S'_q) ]
 *                              + q_i . [ the same with g in place of q ] }
 *     (self and background do not depend on r: they enter through A u_q alone)
 *   exclusion, edge p = (i -> j, S), phi = w:  (D_u A X)_i = -P sum_{row i} w'(d) (n.e) X_j,
 *     (H u)_i = P sum_{row i, j != i} (B_p + B'_p) M_w e          (an edge to an atom's own image has e = 0)
 *   non-periodic, phi = K, all pairs j != i:  (D_u A X)_i = P sum_j K'(d) (n.e) X_j,
 *     (H u)_i = -P sum_j (g_i.q_j + g_j.q_i) M_K e                (f = 0 beyond R: f'' jumps at d = R)
 *   grad_r Phi(r; u_q, g) is the first-order position adjoint with (g, q) := (u_q, g), from the same kernels.
 *   d_u_charges / d_u_positions may each be NULL (zero; that part's work is skipped), both NULL: PET_ERR_ARGUMENT. All three
 *   outputs are written in full. d_workspace: pet_ewald_second_workspace_bytes(e, C) bytes (-1 without a plan, on a P3M-mode
 *   handle, for C < 1). No atoms: PET_OK, nothing touched. Nothing is kept between calls, no host synchronisation, same bits run
 *   to run and alone as inside a batch. No cell tangent is taken and no cell result returned (mixed position / cell second
 *   derivatives are not built); a P3M-mode handle: PET_ERR_ARGUMENT (the mesh operator's are pet_p3m_second's, below).
 * PET_ERR_ARGUMENT: a pet_graph_from_batch handle, a graph built under an adaptive cutoff (it drops edges inside R), a graph
 * of a model without nl_is_strict, a graph whose cutoff, atom or system count differ from the plan's.
 * PET_ERR_UNSUPPORTED: mixed pbc; a cell with more than PET_EWALD_MAX_INDEX reciprocal indices along an axis. */
#define PET_EWALD_MAX_INDEX 63
typedef struct pet_ewald pet_ewald_t;
int pet_ewald_create(double smearing, double kspace_resolution, double cutoff, pet_ewald_t** out);
void pet_ewald_destroy(pet_ewald_t* e);
int64_t pet_ewald_kvectors_host(const double* h_cell, double kspace_resolution, double* h_out, int64_t capacity);
int pet_ewald_plan(pet_ewald_t* e, const double* h_cells, const int32_t* h_pbc, const int64_t* h_first_atom,
                   int64_t n_systems);
int64_t pet_ewald_num_kvectors(const pet_ewald_t* e, int64_t system);
int64_t pet_ewald_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_ewald_potential(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                        int32_t n_channels, float* d_potential, void* d_workspace, int64_t workspace_bytes, void* stream);
int pet_ewald_backward(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                       const float* d_grad_potential, int32_t n_channels, float* d_grad_charges, float* d_grad_positions,
                       float* d_grad_cells, void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t pet_ewald_second_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_ewald_second(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                     const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions,
                     int32_t n_channels, float* d_out_charges, float* d_out_grad_potential, float* d_out_positions,
                     void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Long-range PET: the force-loss training sweep and Hessian-vector products -----------------------
 * The long-range forms of pet_backward_train2 and pet_hessian_vector for a long_range.enable model: the size-generic dual
 * pass (for EVERY model size, the default included, as pet_hessian_vector) with the featuriser between the backbone and the
 * heads,  x = sum_l h_l / sqrt(L),  q = charges_map(x),  V = A(r) q,  y = out_projection(V),  m_l = (h_l + y) / sqrt(2),  the
 * node heads reading m_l. `e` is a planned handle for the batch of `g` (Ewald mode, or P3M mode with a transform hook: below); d_positions [N,3] the positions the graph
 * was built from. The six featuriser tensors are read from the MODEL's parameter table, under the reference's keys
 * long_range_featurizer.{charges_map,out_projection.0,out_projection.2}.{weight,bias} (pet_model_set_param; each d_node x
 * d_node / d_node), and their gradients go to their slots: clipping, Adam, pet_model_set_trainable and the flat gradient
 * cover them like any other parameter. A missing tensor: PET_ERR_ARGUMENT naming the key.
 *   pet_backward_train2_long_range: ADDS dJ/dtheta, J = sum_i (nu_i e_i + lambda_i e'_i), e'_i = d/d eps e_i(R + eps u), to the
 *     gradient slots (pet_model_zero_grad first); d_tangent_atomic [N] (may be NULL) receives e'_i. d_u NULL: first order
 *     (an energy-only loss), d_nu_atomic is then required and d_lambda_atomic ignored; with d_u, d_lambda_atomic is
 *     required and d_nu_atomic may be NULL. Needs no forward pass before it.
 *   pet_hessian_vector_long_range: d_hvp_positions [N,3] = grad_R sum_i lambda_i e'_i (d_lambda_atomic NULL = ones: H u of the
 *     total energy), d_tangent_atomic [N] (may be NULL) = e'_i. Touches no gradient slot.
 *   d_workspace: ONE buffer of pet_train2_long_range_workspace_bytes / pet_hvp_long_range_workspace_bytes (-1 for what the
 *     entry point itself refuses). A batch WITHOUT ANY EDGE is computed like any other: open systems interact through the
 *     operator beyond the cutoff, so it has forces, a Hessian and featuriser gradients.
 * Neither takes a cell tangent, seeds of further targets or returns a cell result: they have no such argument (a stress
 * loss needs the operator's cell tangents, which are not built). Same bits run to run (no float atomics).
 * PET_ERR_UNSUPPORTED: a P3M-mode handle without a transform hook (pet_p3m_set_transform); an adaptive-cutoff model or graph; a graph with a per-layer exchange.
 * PET_ERR_ARGUMENT: a handle without a plan or planned for another batch (atom / system counts, cutoff, device), a
 * pet_graph_from_batch handle, a model without the fused single-property target, a workspace that is too small. */
int64_t pet_train2_long_range_workspace_bytes(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e);
int pet_backward_train2_long_range(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e, const float* d_positions,
                                   void* d_workspace, int64_t workspace_bytes, const float* d_lambda_atomic,
                                   const float* d_nu_atomic, const float* d_u, float* d_tangent_atomic, void* stream);
int64_t pet_hvp_long_range_workspace_bytes(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e);
int pet_hessian_vector_long_range(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e, const float* d_positions,
                                  void* d_workspace, int64_t workspace_bytes, const float* d_lambda_atomic, const float* d_u,
                                  float* d_hvp_positions, float* d_tangent_atomic, void* stream);

/* ---- P3M evaluation of the same operator (utils/long_range.py:71-79,153-170) ------------------------------------------------
 * The reference takes its Ewald branch only under `use_ewald and training`: every evaluation of a periodic long-range model
 * goes through torch-pme's P3MCalculator (mesh_spacing = kspace_resolution, interpolation_nodes). This block is a second
 * implementation of the RECIPROCAL-SPACE sum of the block above; self, background, exclusion and the open all-pairs sum are
 * the same kernels. torch-pme is not part of the reference tree: the mesh operator too is fixed HERE by definition (DESIGN
 * section 19 and metatrain_amd.long_range.P3M_CONVENTIONS hold the same table) and pinned to an independent fp64 oracle
 * (tests/_p3m_oracle.py); parity with torch-pme is NOT pinned.
 *   h = kspace_resolution, p = interpolation_nodes in 1..5, N_a = the smallest power of two >= |cell row a| / h (at least 1),
 *   u = s N with s = r cell^{-1} wrapped to [0, 1), W(x) = M_p(x + p/2) the order-p charge-assignment function (centred
 *   cardinal B-spline), separable over the fractional axes. Nodes: odd p around floor(u + 1/2), offsets -(p-1)/2 .. (p-1)/2;
 *   even p around floor(u), offsets -(p/2-1) .. p/2; indices mod N_a (with N_a < p several nodes fold onto one point and add).
 *   G^(n) = sum_m U_m^2 G(|k_{n+mN}|) / (sum_m U_m^2)^2, G^(0) = 0, U_m = prod_a sinc^p((n_a + m_a N_a) / N_a), m in {-2..2}^3,
 *   n_a in [-N_a/2, N_a/2), k_nu = 2 pi nu cell^{-T}.
 *   Phi = (1/Omega) sum_n G^(n) rho^(n) e^{2 pi i n.j/N} (unnormalised transforms both ways: G^/Omega is the whole filter).
 *   Periodic system: V_i = P [ sum_nodes W_i(node) Phi(node) - self - background - exclusion ]; open systems as above.
 * Adjoints, for dL/dV = g: dL/dq = the operator applied to g. With Phi_q, Phi_g the mesh potentials of q and g and q^, g^ their
 * unfiltered half spectra (per channel, summed over channels):
 *   F_i = P sum_nodes grad_r W_i(node) [ g_i Phi_q + q_i Phi_g ](node),  dW/dr_b = sum_a N_a (cell^{-1})_{ba} dW/du_a,
 *   dL/dcell_bc += -sum_i s_ib F_ic + P sum_n w_n Re(conj(g^_n) q^_n) d(G^_n/Omega)/dcell_bc,  w_n = 1 on the planes n_z = 0 and
 *   n_z = N_z/2 of the half spectrum, 2 elsewhere; the derivative alias term by alias term with the bracket of the block above.
 * The transforms are the CALLER's (torch.fft.rfftn / irfftn(norm="forward") over the last three axes, fp32, same stream): this
 * library links no FFT. Layout, CHANNEL-FIRST: mesh of system s = [C, N_x, N_y, N_z] floats at offset mesh_off_s * C of the
 * packed buffer, half spectrum [C, N_x, N_y, N_z/2 + 1] complex at spec_off_s * C; systems in batch order; non-periodic and
 * empty systems have none (pet_p3m_mesh_shape gives 0 0 0).
 *   pet_ewald_set_p3m(e, p): before pet_ewald_plan, which then builds mesh descriptors and G^/Omega (k_p3m_influence, fp64 ->
 *     fp32; one device synchronisation) instead of k lists. On such a handle pet_ewald_potential / _backward /
 *     _workspace_bytes / _num_kvectors fail (PET_ERR_ARGUMENT / -1), and pet_p3m_* fail on an Ewald-mode handle.
 *   pet_p3m_mesh_shape_host / pet_p3m_influence_host: host fp64, no GPU: N[3] of one cell (0, or -1 for a singular cell), and
 *     G^/Omega on the half spectrum [N_x, N_y, N_z/2 + 1] (returns the count; fills h_out when capacity suffices).
 *   pet_p3m_spread: bins the atoms (k_p3m_bin_*: weights in fp64 from wrapped fractional coordinates, rounded once; stable
 *     counting sort by stencil origin) and spreads d_charges [N, C] to d_mesh. The weights and bins stay in the workspace:
 *     pet_p3m_finish and pet_p3m_backward read them, so they follow a pet_p3m_spread of the same positions.
 *   pet_p3m_filter: d_spectrum *= G^/Omega in place.   pet_p3m_finish: gather of d_mesh_potential, open pairs, self,
 *     background, exclusion -> d_out [N, C].   pet_p3m_backward: d_grad_positions [N, 3] and d_grad_cells [S, 3, 3] (may be
 *     NULL, then the spectra may be too) from the mesh potentials and UNFILTERED spectra of q and g: mesh, exclusion and
 *     open-system parts.
 * PET_ERR_UNSUPPORTED: a mesh axis above PET_P3M_MAX_AXIS; mixed pbc. No float atomics; fixed orders (csrc/p3m.hip, and
 * csrc/long_range.h for the terms both modes launch). */
#define PET_P3M_MAX_AXIS 512
int pet_ewald_set_p3m(pet_ewald_t* e, int32_t interpolation_nodes);
int pet_p3m_mesh_shape_host(const double* h_cell, double spacing, int32_t* out);
int64_t pet_p3m_influence_host(const double* h_cell, double smearing, double spacing, int32_t interpolation_nodes,
                               double* h_out, int64_t capacity);
int pet_p3m_mesh_shape(const pet_ewald_t* e, int64_t system, int32_t* out);
int64_t pet_p3m_mesh_elements(const pet_ewald_t* e, int64_t n_channels);
int64_t pet_p3m_spectrum_elements(const pet_ewald_t* e, int64_t n_channels);
int64_t pet_p3m_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_p3m_spread(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                   int32_t n_channels, float* d_mesh, void* d_workspace, int64_t workspace_bytes, void* stream);
int pet_p3m_filter(const pet_ewald_t* e, int32_t n_channels, void* d_spectrum, void* stream);
int pet_p3m_finish(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                   int32_t n_channels, const float* d_mesh_potential, float* d_out, void* d_workspace, int64_t workspace_bytes,
                   void* stream);
int pet_p3m_backward(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                     const float* d_grad_potential, int32_t n_channels, const float* d_phi_q, const float* d_phi_g,
                     const void* d_spec_q, const void* d_spec_g, float* d_grad_positions, float* d_grad_cells,
                     void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Second derivatives of the mesh operator, and P3M in the dual pass ---------------------------------
 * pet_p3m_second is pet_ewald_second (same arguments, same three results, same contract) on a P3M-mode handle. Positions
 * enter the mesh sum A_mesh = W^T K W (W the spread, K = irfftn . (G^/Omega) . rfftn) through W alone: with the per-atom
 * direction du_i = N (.) (u_r,i cell^{-1}) in mesh units and the tangent weight (D_u W)_i = sum_a (d_a W) du_a,
 *   (D_u A) x = (D_u W)^T K W x + W^T K (D_u W) x,
 *   H_Phi(g, q) u_r = per atom sum_c sum_nodes [ (grad grad W . du)(g phi_q + q phi_g) + grad W (g phi_dq + q phi_dg) ],
 *   phi_x = K W x, phi_dx = K (D_u W) x; d^2W/du^2 = M_{p-2}(x) - 2 M_{p-2}(x-1) + M_{p-2}(x-2) (fp64, rounded once).
 * The self, background, exclusion and open-system terms are the kernels pet_ewald_second launches. A NULL result is not
 * formed and what serves it alone is skipped (all three NULL: PET_ERR_ARGUMENT). Pairs of transforms per call, both
 * cotangents given: d_out_grad_potential alone 2, d_out_charges alone 2, d_out_positions or all three 4.
 * The library links no FFT: the transforms inside the call are the caller's, through a HOOK. pet_p3m_set_transform(e, fn,
 * user) (fn NULL removes it; it survives pet_ewald_plan): fn(user, inverse, mesh_byte_offset, spectrum_byte_offset, C) runs
 * rfftn (inverse = 0) or irfftn with norm = "forward" (inverse = 1) of the plan's packed channel-first meshes (layout of the
 * block above) between a mesh buffer and a half-spectrum buffer at those byte offsets (multiples of 256) of the d_workspace
 * of the entry point that is running, on the stream that entry point was given. It is called on the host while the entry
 * point enqueues its launches and must not synchronise; non-zero fails the entry point with PET_ERR_ARGUMENT naming the hook.
 * The hook is the opt-in: with one, pet_backward_train2_long_range / pet_hessian_vector_long_range and their workspace
 * functions take a P3M-mode handle (their single workspace then holds four meshes and a half spectrum at d_node channels);
 * without one they refuse it as before, and pet_p3m_second returns PET_ERR_ARGUMENT naming pet_p3m_set_transform.
 * pet_p3m_second_workspace_bytes: -1 without a plan, on an Ewald-mode handle, for C < 1. pet_ewald_second* refuse a
 * P3M-mode handle as before. No cell tangent and no cell result. No float atomics; same bits run to run and alone as in a batch. */
typedef int (*pet_p3m_transform_fn)(void* user, int32_t inverse, int64_t mesh_byte_offset, int64_t spectrum_byte_offset,
                                    int32_t n_channels);
int pet_p3m_set_transform(pet_ewald_t* e, pet_p3m_transform_fn fn, void* user);
int64_t pet_p3m_second_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_p3m_second(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                   const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions, int32_t n_channels,
                   float* d_out_charges, float* d_out_grad_potential, float* d_out_positions, void* d_workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- Cell tangents of the second-order operation: the stress term of a loss ----------------------------
 * With a cotangent u_c [S, 3, 3] of dL/dcell (what pet_ewald_backward returns, at fixed Cartesian positions) beside u_q and u_r,
 *   Psi = <u_q, A g> + <u_r, grad_r Phi> + <u_c, grad_cell Phi>, and pet_ewald_second_cell / pet_p3m_second_cell return
 *   d_out_grad_potential = A u_q + (D A) q,   d_out_charges = (D A) g,   D A = d/dt A(r + t u_r, cell + t u_c) at t = 0,
 * the plan's k-index set and mesh shape held fixed (as the first-order dL/dcell holds them). These two feed parameter
 * gradients; the position and cell results (mixed and second cell derivatives) are not built and have no argument here.
 * Per periodic system U = cell^{-1} u_c and u'_i = u_r,i - r_i U (fp64, rounded once): fractional coordinates move by
 * u' cell^{-1} alone, so every phase k.r and every mesh stencil moves as under the position direction u'. With k = 2 pi n cell^{-T}:
 *   (D A) X = (D_{u'} A) X                                          the position tangent of the blocks above, k / the mesh fixed
 *           + P sum_k w_k f_k Re(e^{-i k.r_i} S_X(k)),  f_k = (sigma^2 + 2/k^2)(k U k^T) - tr U      (Ewald: the weights)
 *             P3M: W^T K' W X, K' the filter sum_bc d(G^/Omega)/dcell_bc u_c,bc in place of G^/Omega
 *           + P (2 pi sigma^2 / Omega) tr U sum_j X_j                                                 (background)
 *           - P sum_{row i} w'(d) (n.dD) X_j,  dD = u_j - u_i + S u_c, edges to an atom's own image included   (exclusion)
 * Ewald: f_k S'_X is folded into the weighted structure factor S'_{u'X} before the one tangent gather (k_ew_wdot): no gather is
 * added. P3M: K' W X shares the forward transform of K W X and is added to the spectrum of the mesh the tangent gather reads
 * before that one's inverse transform: no transform is added. HOOK CALLS per pet_p3m_second_cell call with d_u_cells: 4 per
 * result formed (two pairs), 8 for both, whichever of u_q / u_r are given; without d_u_cells those of pet_p3m_second without
 * d_out_positions. Rows of d_u_cells that belong to open systems are ignored (u' = u_r there).
 * Arguments of pet_*_second plus d_u_cells, without d_out_positions. Any of the three cotangents may be NULL (zero), all
 * three: PET_ERR_ARGUMENT. A NULL result is not formed; both NULL: PET_ERR_ARGUMENT. d_u_cells NULL: the launches and bits of
 * pet_*_second with d_out_positions NULL. *_second_cell_workspace_bytes: -1 without a plan, on the other mode's handle, for
 * C < 1 (the second-order workspace, then u' [N, 3]; P3M: also K' per half-spectrum point and one more half spectrum).
 * pet_p3m_second_cell needs the transform hook. Same bits run to run and alone as in a batch; no float atomics.
 *   pet_backward_train2_long_range_cell: pet_backward_train2_long_range with d_u_cell [S, 3, 3] = dL/d(dE/dcell) beside d_u:
 *     e'_i = d/d eps e_i(R + eps u, cell + eps u_cell). Either direction may be NULL when the other is given (d_lambda_atomic is
 *     then required); d_u_cell NULL: the launches and bits of pet_backward_train2_long_range. Both handle modes; the refusals
 *     of that entry point, and PET_ERR_ARGUMENT for a graph without cell shifts (the backbone's cell tangent needs them).
 *     pet_hessian_vector_long_range takes no cell direction. */
int64_t pet_ewald_second_cell_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_ewald_second_cell(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                          const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions,
                          const float* d_u_cells, int32_t n_channels, float* d_out_charges, float* d_out_grad_potential,
                          void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t pet_p3m_second_cell_workspace_bytes(const pet_ewald_t* e, int64_t n_channels);
int pet_p3m_second_cell(const pet_ewald_t* e, const pet_graph_t* g, const float* d_positions, const float* d_charges,
                        const float* d_grad_potential, const float* d_u_charges, const float* d_u_positions,
                        const float* d_u_cells, int32_t n_channels, float* d_out_charges, float* d_out_grad_potential,
                        void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t pet_train2_long_range_cell_workspace_bytes(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e);
int pet_backward_train2_long_range_cell(const pet_model_t* m, const pet_graph_t* g, const pet_ewald_t* e,
                                        const float* d_positions, void* d_workspace, int64_t workspace_bytes,
                                        const float* d_lambda_atomic, const float* d_nu_atomic, const float* d_u,
                                        const float* d_u_cell, float* d_tangent_atomic, void* stream);

/* ---- Rotational augmentation (utils/augmentation.py:O3Augmenter; pet/trainer.py:187-193, 288-303) -------------------------
 * A random element of O(3) per system of a collated batch, drawn and applied on the device. A rigid transformation of
 * positions and cell leaves fractional coordinates alone, so the batch's (center, neighbor, cell_shift) list stays valid:
 * nothing here touches it, and no neighbour search is needed after the call.
 *   pet_o3_draw replaces augmentation.py:57-71 (random_transformations, the +-identity draw of lines 58-63): d_matrices
 *     [n_systems,3,3], one thread per system. Philox-4x32-10 on the counter block (counter low, counter high, system ordinal,
 *     0) under the 64-bit `key`: a system's matrix is a function of (key, counter, ordinal) alone -- not of the grid, of
 *     n_systems or of earlier calls. PET_O3_GROUP_O3: a Haar-uniform rotation from Shoemake's unit quaternion, negated with
 *     probability 1/2 by an independent bit. PET_O3_GROUP_INVERSIONS: +-identity from that same bit. fp64 arithmetic, the
 *     nine entries rounded to fp32 once.
 *   pet_o3_apply replaces augmentation.py:97-124 (transform_systems, transform_tensormap for Cartesian targets): up to
 *     PET_O3_MAX_ARRAYS arrays in one launch, each OUT OF PLACE (dst != src; the sources are the cached batch). Row r of an
 *     array uses the matrix of system system_of_row[r], or of system r when system_of_row is NULL (then rows <= n_systems).
 *     PET_O3_VECTOR: rows [3, P], P innermost, out[a,p] = sum_b R[a,b] x[b,p] (positions, forces, gradients; cells as [3 S]
 *     lattice-vector rows with system_of_row[r] = r / 3). PET_O3_TENSOR2: rows [3, 3, P], out = R T R^T per property
 *     (stress, strain gradients). fp32. Scalars are not passed at all. A NaN anywhere in a vector or tensor makes that whole
 *     output vector or tensor NaN (a partly known vector cannot be rotated), and only that one; a zero row stays exactly
 *     zero. A system index outside [0, n_systems) is not followed: that row comes out NaN.
 * No atomics, no allocation, no host read-back, no synchronisation: results are the same bits run to run.
 * PET_ERR_ARGUMENT: an unknown group or kind, n_arrays above PET_O3_MAX_ARRAYS, a negative count, dst == src. */
#define PET_O3_GROUP_O3 0
#define PET_O3_GROUP_INVERSIONS 1
#define PET_O3_VECTOR 0
#define PET_O3_TENSOR2 1
#define PET_O3_MAX_ARRAYS 8
typedef struct pet_o3_array {
    const float* src;             /* device, rows x (3 or 9) x n_properties */
    float* dst;                   /* device, same shape */
    int64_t rows;
    const int32_t* system_of_row; /* device [rows], or NULL: row r belongs to system r */
    int32_t n_properties;         /* P, the innermost dimension */
    int32_t kind;                 /* PET_O3_VECTOR or PET_O3_TENSOR2 */
} pet_o3_array_t;
int pet_o3_draw(uint64_t key, uint64_t counter, int32_t group, int64_t n_systems, float* d_matrices, void* stream);
int pet_o3_apply(const float* d_matrices, int64_t n_systems, int32_t n_arrays, const pet_o3_array_t* h_arrays, void* stream);

/* ---- Rotational augmentation of spherical targets (utils/augmentation.py:158-180, 97-124; utils/testing/output.py:940-944) ---
 * Targets that are blocks of irreducible representations of O(3), {o3_lambda = l, o3_sigma = +-1}: rows [2l+1, P], P innermost.
 * With positions x' = O x, Q = det(O) O the proper part, a block transforms as t'[m] = f sum_m' D^l(Q)[m,m'] t[m'], f = 1 for a
 * proper O and o3_sigma (-1)^l for an improper one. D^l is defined by Y_l(Q u) = D^l(Q) Y_l(u) with the orthonormal real
 * spherical harmonics in the order m = -l..l WITHOUT the Condon-Shortley phase (metatensor / sphericart):
 * Y_1 = sqrt(3/4pi) (y, z, x), Y_2 = (sqrt(15/4pi) xy, sqrt(15/4pi) yz, sqrt(5/16pi) (3z^2 - 1), sqrt(15/4pi) xz,
 * sqrt(15/16pi) (x^2 - y^2)).
 *   pet_o3_wigner replaces augmentation.py:158-180 (the Wigner-D cache the reference sizes from its targets and fills on the
 *     host through Euler angles): from d_matrices [n_systems,3,3] fp32 (what pet_o3_draw wrote, or the caller's own) it writes
 *     d_parity [n_systems] fp32, the sign of the fp64 determinant as +-1, and d_wigner [n_systems, W(l_max)] fp32 with
 *     W(L) = (L+1)(2L+1)(2L+3)/3: for l = 0..l_max the block D^l(Q) row-major [2l+1, 2l+1], block l at offset l (4 l^2 - 1) / 3.
 *     The Ivanic-Ruedenberg recursion (D^l from D^(l-1) and D^1; every entry a polynomial of degree l in the entries of Q, so
 *     a slightly non-orthogonal matrix gives a slightly non-orthogonal D), fp64 arithmetic, every entry rounded to fp32 once.
 *     A matrix that is exactly +-identity gives exactly the identity blocks. A NaN or an infinity in a matrix makes that
 *     system's whole table and its parity NaN, and no other system's. One workgroup per system.
 *   pet_o3_apply_spherical replaces augmentation.py:97-124 (transform_tensormap for spherical targets): up to
 *     PET_O3_MAX_ARRAYS arrays in one launch, each OUT OF PLACE (dst != src). Rows and system_of_row as in pet_o3_apply.
 *     out[m,p] = f sum_m' D^l[m,m'] x[m',p] in fp32 fused multiply-adds over ALL m': a NaN anywhere in a (row, p) multiplet
 *     makes that whole multiplet NaN, and only that one; a zero multiplet stays exactly zero; under +-identity the output is
 *     exactly +-input. A system index outside [0, n_systems) is not followed: that row comes out NaN. o3_lambda = 0 with
 *     o3_sigma = -1 (a pseudoscalar) multiplies by det; invariants (0, +1) need not be passed at all.
 * No atomics, no allocation, no host read-back, no synchronisation: results are the same bits run to run, whatever the grid.
 * PET_ERR_ARGUMENT: l_max or o3_lambda outside [0, PET_O3_MAX_L], o3_lambda above l_max, o3_sigma not +-1, a negative count,
 * n_arrays above PET_O3_MAX_ARRAYS, dst == src, more rows than systems without system_of_row. Empty inputs launch nothing. */
#define PET_O3_MAX_L 8
typedef struct pet_o3_spherical_array {
    const float* src;             /* device, rows x (2 o3_lambda + 1) x n_properties */
    float* dst;                   /* device, same shape */
    int64_t rows;
    const int32_t* system_of_row; /* device [rows], or NULL: row r belongs to system r */
    int32_t n_properties;         /* P, the innermost dimension */
    int32_t o3_lambda;            /* l in [0, PET_O3_MAX_L], at most the table's l_max */
    int32_t o3_sigma;             /* +1, or -1: the block changes sign under inversion relative to (-1)^l */
} pet_o3_spherical_array_t;
int pet_o3_wigner(const float* d_matrices, int64_t n_systems, int32_t l_max, float* d_wigner, float* d_parity, void* stream);
int pet_o3_apply_spherical(const float* d_wigner, const float* d_parity, int32_t l_max, int64_t n_systems, int32_t n_arrays,
                           const pet_o3_spherical_array_t* h_arrays, void* stream);

/* ---- Composition baselines and target scales (composition/_base_composition.py; scaler/_base_scaler.py) ----------------------
 * What the reference fits on the training set before the first optimizer step, from the plain tensors of a collated batch:
 * species [N] i32 (atomic numbers), system_indices [N] i32 (non-decreasing, in [0, n_systems)) and targets. No model or graph
 * handle: fitting happens before a model exists. Atomic numbers go through d_type_index [max_z + 1] i32 (-1: not a model
 * type). Targets are fp32 or fp64 (`*_is_f64`), rows [n_values] with n_values = components x properties, properties innermost.
 *   pet_species_counts replaces _base_composition.py:_compute_X_per_structure: d_counts [S, T] i32, the atoms of every type in
 *     every system, and d_n_atoms [S] i32. One wave per system.
 *   pet_composition_accumulate replaces _base_composition.py:306-322. per_atom = 0, Y [S, n_values]: XTX [T, T] += sum_s c_s c_s^T
 *     (int64, exact), XTY [T, n_values] += sum_s c_s y_s^T (fp64; a NaN spreads as in tensordot). per_atom = 1, Y [N, n_values]:
 *     the diagonal of XTX += the types' atom counts, XTY[t] += sum of y_i over the atoms of type t (a NaN stays inside its type).
 *   pet_target_moments replaces _base_scaler.py:_compute_N_and_Y2 (:308-370) on the residual r that utils/additive/remove.py,
 *     utils/per_atom.py:average_by_num_atoms and (for n_out > 1) the scaler's own remove=True would have built; no residual
 *     tensor is materialised. per_atom = 0: r = (y - sum_t c_t w[t,:]) / n_atoms (divide_by_n_atoms = 0: the target is one of
 *     per_structure_targets), one output row. per_atom = 1: r = y_i - w[type_i,:], one output row per type. r /= d_scale[row]
 *     (fp64, NULL: 1). d_weights [T, n_values] fp64 or NULL (no baseline). n_out = 1: d_n [rows] i64 += number of non-NaN
 *     entries, d_y2 [rows] fp64 += sum r^2 (accumulate, :372-429). n_out = n_properties: the same per property, [rows, n_out],
 *     summed over rows and components (accumulate_per_property, :459-491).
 *   pet_targets_remove replaces the per-step remove_additive + scaler(remove=True, per-target scales): arrays[0] is the target,
 *     per_atom = 0: out[s,p] = (y[s,p] - sum_t counts[s,t] w[t,p]) / scale[0]; per_atom = 1: out[i,p] = (y[i,p] - w[type_i,p]) /
 *     scale[type_i]. arrays[1..] (per_atom = 0 only) are its gradient arrays (dE/dR [N,3], strain gradients [S,3,3]): divided by
 *     scale[0] only (_base_scaler.py:726-751; the baseline does not depend on positions). One launch, out of place, fp64
 *     arithmetic, rounded to fp32 once on the store. NaN stays NaN.
 * Determinism: every sum is over chunks of 256 rows in ascending order (stage one, partials in the workspace), then over the
 * chunks in ascending order (stage two), in fp64 or exact integers; no floating-point atomics; accumulators are += across
 * calls. Workspace: pet_baseline_workspace_bytes(rows, T, n_values) bytes.
 * *d_error (i32, zeroed by the caller) |= 1 when an atom's species is no model type (the host raises, _base_composition.py:
 * 247-254; such an atom is counted nowhere and its row of pet_targets_remove comes out NaN), |= 2 when system_indices leave
 * [0, n_systems). PET_ERR_ARGUMENT: null or negative arguments, n_out not dividing n_values, a workspace too small, dst == src. */
#define PET_TARGET_MAX_ARRAYS 4
typedef struct pet_target_array {
    const void* src;  /* device, rows x width, fp32 or fp64 */
    float* dst;       /* device, rows x width */
    int64_t rows;
    int32_t width;    /* values per row */
    int32_t is_f64;   /* 1: src is fp64 */
} pet_target_array_t;
int64_t pet_baseline_workspace_bytes(int64_t n_rows, int32_t n_types, int32_t n_values);
int pet_species_counts(const int32_t* d_species, const int32_t* d_system_indices, int64_t n_atoms, int64_t n_systems,
                       const int32_t* d_type_index, int32_t max_z, int32_t n_types, int32_t* d_counts, int32_t* d_n_atoms,
                       int32_t* d_error, void* stream);
int pet_composition_accumulate(int32_t per_atom, const void* d_y, int32_t y_is_f64, int64_t n_rows, int32_t n_values,
                               const int32_t* d_counts, const int32_t* d_species, const int32_t* d_type_index, int32_t max_z,
                               int32_t n_types, int64_t* d_xtx, double* d_xty, int32_t* d_error, void* d_workspace,
                               int64_t workspace_bytes, void* stream);
int pet_target_moments(int32_t per_atom, const void* d_y, int32_t y_is_f64, int64_t n_rows, int32_t n_values, int32_t n_out,
                       const int32_t* d_counts, const int32_t* d_n_atoms, int32_t divide_by_n_atoms, const int32_t* d_species,
                       const int32_t* d_type_index, int32_t max_z, int32_t n_types, const double* d_weights,
                       const double* d_scale, int64_t* d_n, double* d_y2, int32_t* d_error, void* d_workspace,
                       int64_t workspace_bytes, void* stream);
int pet_targets_remove(int32_t per_atom, int32_t n_arrays, const pet_target_array_t* h_arrays, const int32_t* d_counts,
                       const int32_t* d_species, const int32_t* d_type_index, int32_t max_z, int32_t n_types,
                       const double* d_weights, const double* d_scale, int32_t* d_error, void* stream);

/* ---- Pointwise training losses (utils/loss.py; utils/per_atom.py; utils/metrics.py) -------------------------------------------
 * What the reference's trainer forms per target and per gradient from its `loss` hyper (pet/documentation.py:368, utils/loss.py:
 * 144-217 compute_flattened with torch.nn.MSELoss / L1Loss / HuberLoss, :247-279 the masked forms): the loss value, its
 * derivative with respect to the prediction (the seed of a reverse pass) and the sums of utils/metrics.py's RMSEAccumulator /
 * MAEAccumulator. One TERM is one prediction array against one target array, both [rows, width] fp32, row-major.
 *   Residual: d = p rs[row] cs[col mod n_col_scale] - t rs[row]. d_row_scale [rows] fp64 or NULL carries 1 / n_atoms (utils/
 *     per_atom.py average_by_num_atoms: prediction AND target), d_col_scale [n_col_scale] fp64 or NULL (then n_col_scale = 0) the
 *     per-property scales of scaler.apply_scales (predictions only); properties are the innermost axis of a row. d, l, l' and
 *     every sum are fp64.
 *   Validity: an entry counts when its target is not NaN (utils/loss.py:203-207) and, with d_mask [rows, width] u8, its mask byte
 *     is non-zero (:187-194). An invalid entry adds to no sum or count; its seed is exactly 0. A NaN prediction at a valid entry
 *     spreads to the loss, as in torch.
 *   Kinds: PET_LOSS_MSE l = d^2, l' = 2 d; PET_LOSS_MAE l = |d|, l' = sign(d) with sign(0) = 0; PET_LOSS_HUBER l = d^2 / 2 for |d|
 *     <= delta, else delta (|d| - delta / 2), l' = d or delta sign(d). delta is read for PET_LOSS_HUBER only.
 *   pet_loss_count adds the term's number of valid entries to *d_count (i64; an integer atomic, exact in any order).
 *   pet_loss_pointwise: D = *d_count for PET_LOSS_MEAN -- read on the device, no host count -- and 1 for PET_LOSS_SUM (d_count
 *     may then be NULL). *d_loss += weight sum l(d) / D; d_seed[row, col] = weight l'(d) rs[row] cs[col] / D, rounded to fp32
 *     once on the store (NULL: the evaluation form, no seeds); *d_stats += that loss, sum d^2, sum |d| and the valid count.
 *     d_loss or d_stats may be NULL. D = 0 (no valid entry in the whole step): loss 0 and seeds 0 (utils/loss.py:209-215).
 *     A one-batch step is count, then pointwise; a micro-batched step counts every micro-batch first.
 * Determinism: sums go over chunks of 256 rows (a fixed tree inside the chunk) into the workspace, then over the chunks in
 * ascending order, in fp64; a term of one chunk is one launch; no floating-point atomics; two identical calls give the same
 * bits; accumulators are += across calls. No host read-back, no synchronisation. Workspace: pet_loss_workspace_bytes.
 * PET_ERR_ARGUMENT: null or negative arguments, a workspace too small, d_seed == d_pred, n_col_scale not dividing width, an
 * unknown kind or reduction, delta <= 0 for PET_LOSS_HUBER, PET_LOSS_MEAN without d_count. */
#define PET_LOSS_MSE 0
#define PET_LOSS_MAE 1
#define PET_LOSS_HUBER 2
#define PET_LOSS_MEAN 0
#define PET_LOSS_SUM 1
typedef struct pet_loss_stats {
    double loss;    /* sum over calls of weight sum l(d) / D */
    double sum_sq;  /* sum d^2 */
    double sum_abs; /* sum |d| */
    int64_t count;  /* valid entries */
} pet_loss_stats_t;
int64_t pet_loss_workspace_bytes(int64_t rows, int32_t width);
int pet_loss_count(const float* d_target, const uint8_t* d_mask, int64_t rows, int32_t width, int64_t* d_count, void* stream);
int pet_loss_pointwise(const float* d_pred, const float* d_target, const uint8_t* d_mask, const double* d_row_scale,
                       const double* d_col_scale, int32_t n_col_scale, int64_t rows, int32_t width, int32_t kind, double delta,
                       double weight, int32_t reduction, const int64_t* d_count, float* d_seed, double* d_loss,
                       pet_loss_stats_t* d_stats, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- profiling hooks used by bench.py ------------------------------------------ */
/* When enabled, every kernel launch of pet_forward/pet_backward is bracketed with HIP
 * events on the launch stream; pet_profile_report fills name / total ms / calls / algorithmic
 * FLOPs / algorithmic HBM bytes per stage. */
int pet_profile_enable(int on);
/* Restrict the event bracketing to one stage name (e.g. "emlp_bwd"); NULL or "" = all. */
int pet_profile_select(const char* stage);
int pet_profile_reset(void);
int pet_profile_report(int max_entries, char (*names)[64], double* total_ms, int64_t* calls,
                       double* flops, double* bytes, int* n_entries);
/* Runtime switches used by tests / the benchmark (every setting meets the same parity bar). Which kernel serves a stage of the
 * tuned pass under them is decided in one place, csrc/pet_plan.hip; DESIGN.md section 4.7 has every condition as one table.
 *   "side_stream" 1 = node-feature chain on a second HIP stream (default); that stream is created one priority level below the
 *                 caller's (environment PET_HIP_SIDE_PRIO = same | high overrides; PET_HIP_SIDE = 0 disables the stream)
 *   "trr"         1 = transposed register-resident row kernels on f16x3 split-operand products (default; environment
 *                 PET_HIP_TRR = 0 makes 0 the default); 0 = the LDS-tile kernels for the transformer layers (the one fallback
 *                 generation, also the transformer-layer path of PostLN models). The combination stage has one implementation
 *                 (the software-pipelined TRR kernel).
 *   "attn_fused"  bits: 1 = the per-atom fused attention block in the forward (norm -> QKV -> soft-max attention -> output
 *                 projection in one kernel; Q, K, V and the attention output never reach HBM; csrc/pet_ablk.hip), 2 = its
 *                 adjoint (recomputes Q, K, V from the layer input), 4 = whatever the graph's size; default 3: large graphs only
 *                 (at least 3 840 attention tiles). 0 = the three-kernel form everywhere. A forward that ran the block saved no
 *                 Q, K, V: switching its adjoint off in between makes pet_backward fail (PET_ERR_ARGUMENT).
 *   "emlp_s"      the edge MLP and its adjoint -- and, in inference, the edge head and its adjoint (csrc/pet_head_s.hip), the compress
 *                 adjoint (pet_compress_s.hip), the combination stage and its adjoint (pet_comb_s.hip, pet_comb_bwd_s.hip), from
 *                 16 384 atoms on the node-row Linear layers around the attention block (pet_center_s.hip), and in training the
 *                 generic GEMMs of the second-order pass (so_rows_s.hip) -- as two desynchronised four-wave workgroups per CU on one-accumulator products
 *                 with a workgroup-shared weight ring (csrc/pet_emlp_s.hip, rows_s.h; the adjoint RECOMPUTES the SwiGLU pre-activations, so an inference forward does not
 *                 store them): 1 = for graphs of at least 28 672 edge rows (default), v > 1 = from v rows on, 0 = never
 *                 (the one-wave-per-SIMD pipelined kernels everywhere). A forward that ran without saving can only be followed
 *                 by the recomputing adjoint: flipping the switch in between makes pet_backward fail (PET_ERR_ARGUMENT).
 *   "trr_compress" bit mask of f16x3 TRR kernels replacing LDS-tile ones: 1 compress (+adjoint), 2 edge head (+adjoint);
 *                  default 3; 0 = LDS-tile kernels
 *   "node_planes" 1 = node-row kernels k_node2 / k_node2w / k_node_bwd2 (coalesced tiles, fp16 planes; default), 0 = k_node /
 *                 k_swiglu_bwd; 2 forces 32 rows per workgroup (by default up to 16 384 atoms)
 *   "so_trr"      1 = generic training GEMMs with K = 128 or n_out = 128 as TRR kernels (default); 0 = LDS-tile k_gemm_h
 *   "soap_ps_mfma" 1 = SOAP-BPNN power spectrum and its adjoint on the fp32 matrix core (default); 0 = the VALU kernels
 *   "node_split"  1 = graphs of at most 4 096 atoms: the node update and its adjoint run the four hidden chunks of a 32-row
 *                 tile on four workgroups (partials through a temporary, the last arrival finishes the tile) -- default;
 *                 0 = one workgroup per tile
 *   "center_fused" 1 = the node-update kernel also writes the next attention layer's centre tokens (default); 0 = k_center
 *   "sorted_shortcut" 1 = pet_graph_build skips the radix sort of the edges when the neighbour list is already ordered by centre
 *                 with no edge to drop (the first build asks the device, later ones assume the previous build's answer and verify
 *                 it with the build's one read-back; default); 0 = always sort
 *   "dxf_fused"   1 = inference adjoint on one rank: dXF[p] = dM[p] + dcat[p][:D] + dcat[rev[p]][D:] formed inside the
 *                 combination adjoint (first two terms) and the edge-MLP adjoint (the gather) -- default; 0 = k_dxf launch
 *   "train_bf16"  1 = the GEMMs of the second-order pass and the weight-gradient GEMMs keep ONE 16-bit MFMA term per product
 *                 (fp16 / bf16 high planes, fp32 accumulation: BASELINE configs[2]'s "bf16 MFMA MLPs"; gradients within
 *                 ~1e-3, NOT the 1e-5 parity mode; 20-step loss curve in tests/test_gpu_train.py); default 0
 *   "wgrad_bf16"  1 = weight-gradient GEMMs of the training passes as bf16x3 split-operand products (default); 0 = fp32 MFMA
 *   "so_f16x3"    1 = generic GEMMs of the second-order (training) pass as f16x3 (default); 0 = fp32 MFMA
 *   "soap_mfma"   1 = SOAP-BPNN LayerNorm + MLP tail on MFMA (default); 0 = per-atom tail kernels
 *   "soap_packed" 1 = SOAP-BPNN inference (legacy / per-species networks) stores the upper triangle of every power-spectrum block
 *                 only (p_l[a][b] = p_l[b][a]: 2 360 instead of 4 544 floats per atom for the default basis), LayerNorm statistics
 *                 weighted and the first Linear folded accordingly -- default; 0 = the full [N][S] layout (what the feature output,
 *                 the Alchemical centre encoding and the training pass use in any case)
 *   "soap_sorted" 1 = SOAP-BPNN tail GEMM on species-sorted atom tiles, one network per tile (default); 0 = all networks stacked
 *   "soap_pair"   1 = SOAP expansion one wave per atom, its adjoint one lane per pair (default); 0 = first generation
 *   "attn_fused_prof" an action, not a switch (the value is ignored): prints and clears the per-phase cycle sums of the fused
 *                 attention kernels in a library built with -DAB_PROFILE, does nothing otherwise
 *   (removed in round 4 with the kernels they selected: "emlp_pipe", "emlp_bwd_pipe", "comb_pipe", "comb_bwd_pipe",
 *   "emlp_recompute", "line_stores", "lds_w"; in round 6: "attn_lds" with the two staged-adjoint instantiations only it reached,
 *   "tile_f16x3" (the fp32 fallback of the LDS-tile kernels remains for weights without fp16 planes), "soap_fused" with the
 *   first-generation fused SOAP kernels, the A/B value 3 of "node_planes" with its kernel)
 * Unknown keys return PET_ERR_ARGUMENT. */
int pet_config_set(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* PET_HIP_H */
