// The runtime switches of pet_config_set: one field per key, its default here. include/pet_hip.h describes every key;
// abi.hip holds the one instance and the key table that writes it. Everything else reads it through switches().
#pragma once
#include <stdint.h>

#include "pet_plan.h"  // EMLP_S_MIN_ROWS

namespace pet {

struct Switches {
    int side_stream = -1;  // -1: the environment decides (abi.hip side_stream())
    int trr = -1;          // -1: PET_HIP_TRR, read on first use (abi.hip use_trr())
    int attn_fused = 3;    // bit mask
    int emlp_s = 1;
    int64_t emlp_s_rows = EMLP_S_MIN_ROWS;  // set together with emlp_s
    int trr_compress = 3;  // bit mask
    int node_planes = 1;   // 0, 1 or 2
    int so_trr = 1;
    int soap_ps_mfma = 1;
    int node_split = 1;
    int center_fused = 1;
    int sorted_shortcut = 1;
    int dxf_fused = 1;
    int train_bf16 = 0;
    int wgrad_bf16 = 1;
    int so_f16x3 = 1;
    int soap_mfma = 1;
    int soap_packed = 1;
    int soap_sorted = 1;
    int soap_pair = 1;
};

const Switches& switches();

// the row policy of the ring kernels (rows_s.h), first-order plan and second-order GEMMs alike: pet_config_set("emlp_s", v) serves
// row counts from emlp_s_rows on (v > 1: the tests force small graphs through)
inline bool ring_serves(int64_t rows) { return switches().emlp_s && rows >= switches().emlp_s_rows; }

}  // namespace pet
