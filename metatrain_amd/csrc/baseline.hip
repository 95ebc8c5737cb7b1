// Composition baselines and target scales (composition/_base_composition.py, scaler/_base_scaler.py, utils/additive/remove.py):
// what the reference fits on the training set before the first optimizer step, accumulated on the device from the plain tensors
// of a collated batch, and the per-step transform that takes both out of the targets.
//   pet_species_counts          counts [S, T] and n_atoms [S]: _compute_X_per_structure, one wave per system
//   pet_composition_accumulate  XTX [T, T] += X^T X (int64, exact), XTY [T, P] += X^T Y (fp64)
//   pet_target_moments          N (int64, non-NaN entries) and Y2 = sum r^2 (fp64) of the residual r, formed on the fly
//   pet_targets_remove          out = (y - baseline) / scale, fp64 inside, rounded to fp32 once; gradient arrays in the same launch
// Arithmetic. Targets come in as fp32 or fp64 and are widened on load; every product, difference, quotient and sum is fp64, and
// only pet_targets_remove rounds, once, on its store. A raw energy of -1e5 eV has an fp32 ulp of 8e-3 eV: the baseline has to come
// off before any rounding.
// Reductions. Rows (systems or atoms) are cut into chunks of BL_CHUNK. Stage one: one workgroup per chunk, one thread per output
// element, the chunk's rows summed in ascending order into a partial in the workspace. Stage two: one thread per output element
// sums the partials in ascending chunk order and adds the total to the accumulator. No floating-point atomics, no dependence on
// the grid: two runs give the same bits. (The error flag is set with an integer atomicOr, whose result does not depend on order.)
// Species go through type_index [max_z + 1] (-1: not a model type). An atom whose species is outside [0, max_z] or maps to -1 sets
// *d_error and is counted nowhere; the host raises (_base_composition.py:247-254).
#include <cmath>

#include "common.h"

namespace pet {

namespace {

constexpr int BL_BLOCK = 256;
constexpr int BL_CHUNK = 256;  // rows per partial

__device__ inline double bl_load(const void* p, int64_t i, int f64) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

__device__ inline int bl_type(const int32_t* __restrict__ type_index, int max_z, int z) {
    return (z >= 0 && z <= max_z) ? type_index[z] : -1;
}

// first index in [0, n) with a[i] >= v (a non-decreasing)
__device__ inline int64_t bl_lower_bound(const int32_t* __restrict__ a, int64_t n, int v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per system: lane l owns the counters of types l, l + 64, ...; the system's atoms go by in slices of 64, and the
// number of atoms of a type in a slice is the population count of a ballot
__global__ __launch_bounds__(64) void k_species_counts(const int32_t* __restrict__ species, const int32_t* __restrict__ sysidx,
                                                       int64_t N, int S, const int32_t* __restrict__ type_index, int max_z, int T,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ n_atoms,
                                                       int32_t* __restrict__ error) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int64_t first = bl_lower_bound(sysidx, N, s), last = bl_lower_bound(sysidx, N, s + 1);
    if (lane == 0) n_atoms[s] = (int32_t)(last - first);
    if (s == 0 && lane == 0 && (sysidx[0] < 0 || sysidx[N - 1] >= S)) atomicOr(error, 2);  // atoms that belong to no system
    for (int tb = 0; tb < T; tb += 64) {
        int32_t mine = 0;
        for (int64_t base = first; base < last; base += 64) {
            const int64_t i = base + lane;
            const int t = i < last ? bl_type(type_index, max_z, species[i]) : -2;
            if (t == -1 && tb == 0) atomicOr(error, 1);
            const int tn = T - tb < 64 ? T - tb : 64;
            for (int k = 0; k < tn; k++) {
                const unsigned long long m = __ballot(t == tb + k);
                if (lane == k) mine += __popcll(m);
            }
        }
        if (tb + lane < T) counts[(int64_t)s * T + tb + lane] = mine;
    }
}

// stage one of pet_composition_accumulate. Partials per chunk: XTX [T, TX] int64, then (after all chunks' XTX) XTY [T, P] fp64;
// TX = T (per structure: c c^T) or 1 (per atom: the type's count, the diagonal).
template <bool PER_ATOM>
__global__ __launch_bounds__(BL_BLOCK) void k_comp_partial(const void* __restrict__ Y, int y_f64, int64_t rows, int T, int P,
                                                            const int32_t* __restrict__ counts, const int32_t* __restrict__ species,
                                                            const int32_t* __restrict__ type_index, int max_z,
                                                            int64_t* __restrict__ part_xtx, double* __restrict__ part_xty,
                                                            int32_t* __restrict__ error) {
    const int64_t chunk = blockIdx.x, r0 = chunk * BL_CHUNK, r1 = r0 + BL_CHUNK < rows ? r0 + BL_CHUNK : rows;
    const int TX = PER_ATOM ? 1 : T, W = TX + P;
    for (int o = threadIdx.x; o < T * W; o += BL_BLOCK) {
        const int t = o / W, j = o - t * W;
        if (j < TX) {
            int64_t acc = 0;
            for (int64_t r = r0; r < r1; r++) {
                if (PER_ATOM) {
                    const int tr = bl_type(type_index, max_z, species[r]);
                    if (tr < 0 && t == 0) atomicOr(error, 1);
                    acc += tr == t;
                } else {
                    acc += (int64_t)counts[r * T + t] * (int64_t)counts[r * T + j];
                }
            }
            part_xtx[(chunk * T + t) * TX + j] = acc;
        } else {
            const int p = j - TX;
            double acc = 0.0;
            for (int64_t r = r0; r < r1; r++) {
                const double y = bl_load(Y, r * P + p, y_f64);
                if (PER_ATOM) {  // a select, not a product with the one-hot row: a NaN stays inside its own type (:315-322)
                    if (bl_type(type_index, max_z, species[r]) == t) acc += y;
                } else {
                    acc = fma((double)counts[r * T + t], y, acc);  // tensordot (:314): 0 x NaN is NaN there too
                }
            }
            part_xty[(chunk * T + t) * P + p] = acc;
        }
    }
}

// stage two: element o of XTX [T, TX] (written to the diagonal of [T, T] when TX = 1) and of XTY [T, P]
__global__ __launch_bounds__(BL_BLOCK) void k_comp_final(int64_t n_chunks, int T, int TX, int P, const int64_t* __restrict__ part_xtx,
                                                         const double* __restrict__ part_xty, int64_t* __restrict__ xtx,
                                                         double* __restrict__ xty) {
    const int o = blockIdx.x * BL_BLOCK + threadIdx.x;
    const int nx = T * TX;
    if (o < nx) {
        int64_t acc = 0;
        for (int64_t c = 0; c < n_chunks; c++) acc += part_xtx[c * nx + o];
        xtx[TX == 1 ? (int64_t)o * T + o : o] += acc;
    } else if (o < nx + T * P) {
        const int e = o - nx;
        double acc = 0.0;
        for (int64_t c = 0; c < n_chunks; c++) acc += part_xty[c * T * P + e];
        xty[e] += acc;
    }
}

// the residual of one entry: per structure (y - sum_t c_t w[t,p]) / n_atoms, per atom y - w[type,p]; w == NULL: no baseline
__device__ inline double bl_residual_structure(double y, const int32_t* __restrict__ c, const double* __restrict__ w, int T, int P, int p) {
    if (w) {
        double base = 0.0;
        for (int t = 0; t < T; t++) base = fma((double)c[t], w[t * P + p], base);
        y -= base;
    }
    return y;
}

// stage one of pet_target_moments. Partials [chunk, R, P, 2] fp64: (sum r^2, number of non-NaN entries; at most BL_CHUNK, exact);
// R = 1 (per structure) or T (per atom)
template <bool PER_ATOM>
__global__ __launch_bounds__(BL_BLOCK) void k_moments_partial(const void* __restrict__ Y, int y_f64, int64_t rows, int T, int P,
                                                               const int32_t* __restrict__ counts, const int32_t* __restrict__ n_atoms,
                                                               int divide, const int32_t* __restrict__ species,
                                                               const int32_t* __restrict__ type_index, int max_z,
                                                               const double* __restrict__ w, const double* __restrict__ scale,
                                                               double* __restrict__ part, int32_t* __restrict__ error) {
    const int64_t chunk = blockIdx.x, r0 = chunk * BL_CHUNK, r1 = r0 + BL_CHUNK < rows ? r0 + BL_CHUNK : rows;
    const int R = PER_ATOM ? T : 1;
    for (int o = threadIdx.x; o < R * P; o += BL_BLOCK) {
        const int t = o / P, p = o - t * P;
        const double sc = scale ? scale[t] : 1.0;
        double y2 = 0.0, n = 0.0;
        for (int64_t r = r0; r < r1; r++) {
            double y;
            if (PER_ATOM) {
                const int tr = bl_type(type_index, max_z, species[r]);
                if (tr < 0 && o == 0) atomicOr(error, 1);
                if (tr != t) continue;
                y = bl_load(Y, r * P + p, y_f64);
                if (w) y -= w[t * P + p];
            } else {
                y = bl_residual_structure(bl_load(Y, r * P + p, y_f64), counts + r * T, w, T, P, p);
                if (divide) y /= (double)n_atoms[r];
            }
            if (y != y) continue;  // the NaN mask of _compute_N_and_Y2 (:308-316)
            y /= sc;
            y2 = fma(y, y, y2);
            n += 1.0;
        }
        part[((chunk * R + t) * P + p) * 2] = y2;
        part[((chunk * R + t) * P + p) * 2 + 1] = n;
    }
}

// stage two: output (t, q), q < Q; Q = 1 sums all P columns, Q = n_properties sums the columns c * Q + q (the components)
__global__ __launch_bounds__(BL_BLOCK) void k_moments_final(int64_t n_chunks, int R, int P, int Q, const double* __restrict__ part,
                                                            int64_t* __restrict__ Nacc, double* __restrict__ Y2acc) {
    const int o = blockIdx.x * BL_BLOCK + threadIdx.x;
    if (o >= R * Q) return;
    const int t = o / Q, q = o - t * Q;
    double y2 = 0.0;
    int64_t n = 0;
    for (int64_t c = 0; c < n_chunks; c++)
        for (int p = q; p < P; p += Q) {
            const double* e = part + ((c * R + t) * P + p) * 2;
            y2 += e[0];
            n += (int64_t)e[1];
        }
    Y2acc[o] += y2;
    Nacc[o] += n;
}

struct RemoveBatch {
    pet_target_array_t a[PET_TARGET_MAX_ARRAYS];  // a[0]: the values, a[1..]: gradient arrays
    int first_block[PET_TARGET_MAX_ARRAYS + 1];
    int n;
};

__global__ __launch_bounds__(BL_BLOCK) void k_targets_remove(RemoveBatch b, int per_atom, int T, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ species,
                                                             const int32_t* __restrict__ type_index, int max_z,
                                                             const double* __restrict__ w, const double* __restrict__ scale,
                                                             int32_t* __restrict__ error) {
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.first_block[k + 1]) k++;
    const pet_target_array_t d = b.a[k];
    const int64_t P = d.width;
    const int64_t e = (int64_t)(blockIdx.x - b.first_block[k]) * BL_BLOCK + threadIdx.x;
    if (e >= d.rows * P) return;
    double y = bl_load(d.src, e, d.is_f64);
    if (k > 0) {  // a gradient array: the baseline does not depend on positions or strain (_base_scaler.py:726-751)
        d.dst[e] = (float)(scale ? y / scale[0] : y);
        return;
    }
    const int64_t r = e / P;
    const int p = (int)(e - r * P);
    if (per_atom) {
        const int t = bl_type(type_index, max_z, species[r]);
        if (t < 0) {
            atomicOr(error, 1);
            d.dst[e] = NAN;
            return;
        }
        if (w) y -= w[t * P + p];
        if (scale) y /= scale[t];
    } else {
        y = bl_residual_structure(y, counts + r * T, w, T, (int)P, p);
        if (scale) y /= scale[0];
    }
    d.dst[e] = (float)y;
}

int check_types(int64_t n_types, int64_t max_z, const void* d_type_index) {
    PET_REQUIRE(n_types >= 1 && n_types <= 4096, PET_ERR_ARGUMENT, "n_types outside [1, 4096]");
    PET_REQUIRE(max_z >= 0 && max_z < (1 << 20) && d_type_index, PET_ERR_ARGUMENT, "type_index missing or max_z out of range");
    return PET_OK;
}

}  // namespace

}  // namespace pet

using namespace pet;

extern "C" {

int64_t pet_baseline_workspace_bytes(int64_t n_rows, int32_t n_types, int32_t n_values) {
    if (n_rows < 0 || n_types < 1 || n_values < 0) return -1;
    const int64_t chunks = (n_rows + BL_CHUNK - 1) / BL_CHUNK;
    const int64_t T = n_types, P = n_values;
    const int64_t comp = T * (T + P), mom = T * P * 2;
    return 8 * chunks * (comp > mom ? comp : mom) + 8;
}

int pet_species_counts(const int32_t* d_species, const int32_t* d_system_indices, int64_t n_atoms, int64_t n_systems,
                       const int32_t* d_type_index, int32_t max_z, int32_t n_types, int32_t* d_counts, int32_t* d_n_atoms,
                       int32_t* d_error, void* stream) {
    if (int rc = check_types(n_types, max_z, d_type_index)) return rc;
    PET_REQUIRE(n_atoms >= 0 && n_systems >= 0 && n_systems <= INT32_MAX, PET_ERR_ARGUMENT, "negative count or too many systems");
    if (n_systems == 0) {
        PET_REQUIRE(n_atoms == 0, PET_ERR_ARGUMENT, "atoms but no systems");
        return PET_OK;
    }
    PET_REQUIRE(d_counts && d_n_atoms && d_error, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(n_atoms > 0 && d_species && d_system_indices, PET_ERR_ARGUMENT, "systems but no atoms");
    k_species_counts<<<(unsigned)n_systems, 64, 0, (hipStream_t)stream>>>(d_species, d_system_indices, n_atoms, (int)n_systems,
                                                                         d_type_index, max_z, n_types, d_counts, d_n_atoms, d_error);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_composition_accumulate(int32_t per_atom, const void* d_y, int32_t y_is_f64, int64_t n_rows, int32_t n_values,
                               const int32_t* d_counts, const int32_t* d_species, const int32_t* d_type_index, int32_t max_z,
                               int32_t n_types, int64_t* d_xtx, double* d_xty, int32_t* d_error, void* d_workspace,
                               int64_t workspace_bytes, void* stream) {
    if (int rc = check_types(n_types, max_z, d_type_index)) return rc;
    PET_REQUIRE(n_rows >= 0 && n_values >= 1, PET_ERR_ARGUMENT, "negative row count or no values per row");
    if (n_rows == 0) return PET_OK;
    PET_REQUIRE(d_y && d_xtx && d_xty && d_error && (per_atom ? (const void*)d_species : (const void*)d_counts), PET_ERR_ARGUMENT,
                "null argument");
    PET_REQUIRE((int64_t)n_types * (n_types + n_values) <= INT32_MAX / 2, PET_ERR_ARGUMENT, "too many types x values");
    PET_REQUIRE(d_workspace && workspace_bytes >= pet_baseline_workspace_bytes(n_rows, n_types, n_values), PET_ERR_ARGUMENT,
                "workspace too small (pet_baseline_workspace_bytes)");
    const int64_t chunks = (n_rows + BL_CHUNK - 1) / BL_CHUNK;
    PET_REQUIRE(chunks <= INT32_MAX, PET_ERR_ARGUMENT, "too many rows");
    const int T = n_types, P = n_values, TX = per_atom ? 1 : T;
    int64_t* part_xtx = (int64_t*)d_workspace;
    double* part_xty = (double*)d_workspace + chunks * T * TX;
    hipStream_t st = (hipStream_t)stream;
    if (per_atom)
        k_comp_partial<true><<<(unsigned)chunks, BL_BLOCK, 0, st>>>(d_y, y_is_f64, n_rows, T, P, d_counts, d_species, d_type_index,
                                                                   max_z, part_xtx, part_xty, d_error);
    else
        k_comp_partial<false><<<(unsigned)chunks, BL_BLOCK, 0, st>>>(d_y, y_is_f64, n_rows, T, P, d_counts, d_species, d_type_index,
                                                                    max_z, part_xtx, part_xty, d_error);
    PET_HIP_CHECK(hipGetLastError());
    k_comp_final<<<cdiv((int64_t)T * (TX + P), BL_BLOCK), BL_BLOCK, 0, st>>>(chunks, T, TX, P, part_xtx, part_xty, d_xtx, d_xty);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_target_moments(int32_t per_atom, const void* d_y, int32_t y_is_f64, int64_t n_rows, int32_t n_values, int32_t n_out,
                       const int32_t* d_counts, const int32_t* d_n_atoms, int32_t divide_by_n_atoms, const int32_t* d_species,
                       const int32_t* d_type_index, int32_t max_z, int32_t n_types, const double* d_weights,
                       const double* d_scale, int64_t* d_n, double* d_y2, int32_t* d_error, void* d_workspace,
                       int64_t workspace_bytes, void* stream) {
    if (int rc = check_types(n_types, max_z, d_type_index)) return rc;
    PET_REQUIRE(n_rows >= 0 && n_values >= 1, PET_ERR_ARGUMENT, "negative row count or no values per row");
    PET_REQUIRE(n_out >= 1 && n_values % n_out == 0, PET_ERR_ARGUMENT,
                "n_out must be 1 or the number of properties, which divides the values per row");
    if (n_rows == 0) return PET_OK;
    PET_REQUIRE(d_y && d_n && d_y2 && d_error, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(per_atom ? d_species != nullptr : (d_n_atoms != nullptr || !divide_by_n_atoms) && (d_counts != nullptr || !d_weights),
                PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE((int64_t)n_types * n_values <= INT32_MAX / 4, PET_ERR_ARGUMENT, "too many types x values");
    PET_REQUIRE(d_workspace && workspace_bytes >= pet_baseline_workspace_bytes(n_rows, n_types, n_values), PET_ERR_ARGUMENT,
                "workspace too small (pet_baseline_workspace_bytes)");
    const int64_t chunks = (n_rows + BL_CHUNK - 1) / BL_CHUNK;
    PET_REQUIRE(chunks <= INT32_MAX, PET_ERR_ARGUMENT, "too many rows");
    const int T = n_types, P = n_values, R = per_atom ? T : 1;
    double* part = (double*)d_workspace;
    hipStream_t st = (hipStream_t)stream;
    if (per_atom)
        k_moments_partial<true><<<(unsigned)chunks, BL_BLOCK, 0, st>>>(d_y, y_is_f64, n_rows, T, P, d_counts, d_n_atoms, 0, d_species,
                                                                      d_type_index, max_z, d_weights, d_scale, part, d_error);
    else
        k_moments_partial<false><<<(unsigned)chunks, BL_BLOCK, 0, st>>>(d_y, y_is_f64, n_rows, T, P, d_counts, d_n_atoms,
                                                                       divide_by_n_atoms, d_species, d_type_index, max_z, d_weights,
                                                                       d_scale, part, d_error);
    PET_HIP_CHECK(hipGetLastError());
    k_moments_final<<<cdiv((int64_t)R * n_out, BL_BLOCK), BL_BLOCK, 0, st>>>(chunks, R, P, n_out, part, d_n, d_y2);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_targets_remove(int32_t per_atom, int32_t n_arrays, const pet_target_array_t* h_arrays, const int32_t* d_counts,
                       const int32_t* d_species, const int32_t* d_type_index, int32_t max_z, int32_t n_types,
                       const double* d_weights, const double* d_scale, int32_t* d_error, void* stream) {
    if (int rc = check_types(n_types, max_z, d_type_index)) return rc;
    PET_REQUIRE(n_arrays >= 1 && n_arrays <= PET_TARGET_MAX_ARRAYS && h_arrays, PET_ERR_ARGUMENT,
                "n_arrays outside [1, " + std::to_string(PET_TARGET_MAX_ARRAYS) + "]");
    PET_REQUIRE(!per_atom || n_arrays == 1, PET_ERR_ARGUMENT, "gradient arrays go with a per-structure target only");
    PET_REQUIRE(d_error, PET_ERR_ARGUMENT, "null argument");
    RemoveBatch b{};
    int64_t blocks = 0;
    for (int i = 0; i < n_arrays; i++) {
        const pet_target_array_t& d = h_arrays[i];
        const std::string which = "array " + std::to_string(i) + ": ";
        PET_REQUIRE(d.rows >= 0 && d.width >= 1, PET_ERR_ARGUMENT, which + "negative row count or no values per row");
        const int64_t threads = d.rows * (int64_t)d.width;
        if (i == 0) {
            PET_REQUIRE((int64_t)n_types * d.width <= INT32_MAX, PET_ERR_ARGUMENT, which + "too many types x values");
            PET_REQUIRE(threads == 0 || (per_atom ? d_species != nullptr : (d_counts != nullptr || !d_weights)), PET_ERR_ARGUMENT,
                        which + "null argument");
        }
        PET_REQUIRE(threads == 0 || (d.src && d.dst && d.src != (const void*)d.dst), PET_ERR_ARGUMENT,
                    which + "null argument, or dst == src (the transform is out of place)");
        b.a[b.n] = d;
        b.first_block[b.n] = (int)blocks;
        blocks += (threads + BL_BLOCK - 1) / BL_BLOCK;
        PET_REQUIRE(blocks <= INT32_MAX, PET_ERR_ARGUMENT, "too many values in one call");
        b.n++;
    }
    b.first_block[b.n] = (int)blocks;
    if (blocks == 0) return PET_OK;
    k_targets_remove<<<(unsigned)blocks, BL_BLOCK, 0, (hipStream_t)stream>>>(b, per_atom, n_types, d_counts, d_species, d_type_index,
                                                                           max_z, d_weights, d_scale, d_error);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // extern "C"
