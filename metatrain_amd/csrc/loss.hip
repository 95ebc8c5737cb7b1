// Pointwise training losses (utils/loss.py: BaseTensorMapLoss.compute_flattened with torch.nn.MSELoss / L1Loss / HuberLoss, and
// their masked forms): the loss value, dL/d(prediction) and the sums the reference's RMSE / MAE accumulators keep (utils/
// metrics.py), for one TERM -- one prediction array against one target array, both [rows, width] fp32 row-major.
//   pet_loss_count      *d_count (int64) += the term's number of valid entries
//   pet_loss_pointwise  residuals, loss, seeds and statistics; the denominator of a "mean" is read from *d_count on the device
// Residual. d = p rs[row] cs[col % n_cs] - t rs[row]: rs (optional, fp64) is the 1 / n_atoms of utils/per_atom.py, applied to
// prediction AND target; cs (optional, fp64) are the per-property scales of scaler.apply_scales, predictions only; properties are
// the innermost axis of a row. fp32 operands are widened on load and d, l(d), l'(d) and every sum are fp64; only the seed is
// rounded, once, on its store.
// Validity. An entry counts when its target is not NaN (utils/loss.py:203-207) and its mask byte (optional) is non-zero (:187-194).
// An invalid entry adds nothing to any sum and gets the seed 0. A NaN prediction at a valid entry spreads, as in torch.
// Reductions, as in baseline.hip. Rows are cut into chunks of LS_CHUNK. Stage one: one workgroup per chunk; thread t takes the
// chunk's entries t, t + 256, ... in ascending order, the 64 lanes of a wave are summed by a shuffle tree and the four waves in
// ascending order: the chunk's partial in the workspace. Stage two: one thread per statistic sums the partials in ascending
// chunk order and adds to the accumulators. A term of one chunk (energies, strain gradients) does both in its one workgroup: one
// launch. The tree has a fixed shape and nothing depends on the grid or on timing: no floating-point atomics, two identical
// calls give the same bits. (pet_loss_count adds integers atomically: exact in any order.)
#include <cmath>

#include "common.h"

namespace pet {

namespace {

constexpr int LS_BLOCK = 256;
constexpr int LS_CHUNK = 256;  // rows per partial
constexpr int LS_STATS = 4;    // sum l(d), sum d^2, sum |d|, valid entries
constexpr int LS_WAVES = LS_BLOCK / 64;

__device__ inline bool ls_valid(const float* __restrict__ target, const uint8_t* __restrict__ mask, int64_t e) {
    const float t = target[e];
    return t == t && (!mask || mask[e] != 0);
}

__device__ inline double ls_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum
}

__global__ __launch_bounds__(LS_BLOCK) void k_loss_count(const float* __restrict__ target, const uint8_t* __restrict__ mask, int64_t n,
                                                         unsigned long long* __restrict__ count) {
    __shared__ unsigned int s_n[LS_WAVES];
    unsigned int mine = 0;
    for (int64_t e = (int64_t)blockIdx.x * LS_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * LS_BLOCK)
        mine += ls_valid(target, mask, e);
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < LS_WAVES; w++) total += s_n[w];
        if (total) atomicAdd(count, total);
    }
}

struct LossArgs {
    const float* pred;
    const float* target;
    const uint8_t* mask;
    const double* rs;
    const double* cs;
    int n_cs;
    int64_t rows;
    int width;
    int kind;
    double delta, weight;
    const int64_t* count;  // NULL: reduction = sum
    float* seed;
    double* part;          // [chunks, LS_STATS]
    double* loss;          // += (either may be NULL)
    pet_loss_stats_t* stats;
};

// adds the totals of one term to the accumulators; weight * (sum l(d) / D): the order of torch's mean, then the weight
__device__ inline void ls_accumulate(const LossArgs& a, const double* t, int64_t D) {
    const double l = D > 0 ? a.weight * (t[0] / (double)D) : 0.0;
    if (a.loss) *a.loss += l;
    if (a.stats) {
        a.stats->loss += l;
        a.stats->sum_sq += t[1];
        a.stats->sum_abs += t[2];
        a.stats->count += (int64_t)t[3];
    }
}

template <bool SINGLE>
__global__ __launch_bounds__(LS_BLOCK) void k_loss_pointwise(LossArgs a) {
    __shared__ double s_part[LS_WAVES][LS_STATS];
    const int64_t chunk = blockIdx.x;
    const int64_t e0 = chunk * LS_CHUNK * a.width;
    const int64_t e1 = (chunk + 1) * LS_CHUNK < a.rows ? (chunk + 1) * LS_CHUNK * a.width : a.rows * a.width;
    const int64_t D = a.count ? *a.count : 1;
    const double scale = D > 0 ? a.weight / (double)D : 0.0;  // no valid entry in the whole step: loss 0, seeds 0 (:209-215)
    double acc[LS_STATS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = e0 + threadIdx.x; e < e1; e += LS_BLOCK) {
        if (!ls_valid(a.target, a.mask, e)) {
            if (a.seed) a.seed[e] = 0.0f;
            continue;
        }
        const int64_t r = e / a.width;
        const int c = (int)(e - r * a.width);
        const double rs = a.rs ? a.rs[r] : 1.0;
        const double cs = a.cs ? a.cs[c % a.n_cs] : 1.0;
        const double d = (double)a.pred[e] * rs * cs - (double)a.target[e] * rs;
        const double ad = fabs(d);
        double l, dl;
        if (a.kind == PET_LOSS_MSE) {
            l = d * d;
            dl = 2.0 * d;
        } else if (a.kind == PET_LOSS_MAE) {
            l = ad;
            dl = d != d ? d : (double)((d > 0.0) - (d < 0.0));
        } else if (ad <= a.delta) {
            l = 0.5 * d * d;
            dl = d;
        } else {
            l = a.delta * (ad - 0.5 * a.delta);
            dl = d != d ? d : (d > 0.0 ? a.delta : -a.delta);
        }
        acc[0] += l;
        acc[1] = fma(d, d, acc[1]);
        acc[2] += ad;
        acc[3] += 1.0;
        if (a.seed) a.seed[e] = (float)(scale * dl * rs * cs);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < LS_STATS; k++) {
        const double v = ls_wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[LS_STATS];
        for (int k = 0; k < LS_STATS; k++) {
            t[k] = s_part[0][k];
            for (int w = 1; w < LS_WAVES; w++) t[k] += s_part[w][k];
        }
        if (SINGLE) {
            ls_accumulate(a, t, D);
        } else {
            for (int k = 0; k < LS_STATS; k++) a.part[chunk * LS_STATS + k] = t[k];
        }
    }
}

__global__ __launch_bounds__(64) void k_loss_final(LossArgs a, int64_t n_chunks) {
    __shared__ double s_t[LS_STATS];
    const int k = threadIdx.x;
    if (k < LS_STATS) {
        double t = 0.0;
        for (int64_t c = 0; c < n_chunks; c++) t += a.part[c * LS_STATS + k];
        s_t[k] = t;
    }
    __syncthreads();
    if (k == 0) {
        ls_accumulate(a, s_t, a.count ? *a.count : 1);
    }
}

}  // namespace

}  // namespace pet

using namespace pet;

extern "C" {

int64_t pet_loss_workspace_bytes(int64_t rows, int32_t width) {
    if (rows < 0 || width < 1) return -1;
    const int64_t chunks = (rows + LS_CHUNK - 1) / LS_CHUNK;
    return 8 * LS_STATS * chunks + 8;
}

int pet_loss_count(const float* d_target, const uint8_t* d_mask, int64_t rows, int32_t width, int64_t* d_count, void* stream) {
    PET_REQUIRE(rows >= 0 && width >= 1, PET_ERR_ARGUMENT, "negative row count or no values per row");
    PET_REQUIRE(d_count, PET_ERR_ARGUMENT, "null argument");
    if (rows == 0) return PET_OK;
    PET_REQUIRE(d_target, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(rows <= (INT64_MAX >> 1) / width, PET_ERR_ARGUMENT, "too many values");
    const int64_t n = rows * width;
    const int64_t blocks = (n + LS_BLOCK - 1) / LS_BLOCK;
    k_loss_count<<<(unsigned)(blocks < 1024 ? blocks : 1024), LS_BLOCK, 0, (hipStream_t)stream>>>(d_target, d_mask, n,
                                                                                                (unsigned long long*)d_count);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int pet_loss_pointwise(const float* d_pred, const float* d_target, const uint8_t* d_mask, const double* d_row_scale,
                       const double* d_col_scale, int32_t n_col_scale, int64_t rows, int32_t width, int32_t kind, double delta,
                       double weight, int32_t reduction, const int64_t* d_count, float* d_seed, double* d_loss,
                       pet_loss_stats_t* d_stats, void* d_workspace, int64_t workspace_bytes, void* stream) {
    PET_REQUIRE(rows >= 0 && width >= 1, PET_ERR_ARGUMENT, "negative row count or no values per row");
    PET_REQUIRE(kind == PET_LOSS_MSE || kind == PET_LOSS_MAE || kind == PET_LOSS_HUBER, PET_ERR_ARGUMENT,
                "unknown loss kind " + std::to_string(kind));
    PET_REQUIRE(reduction == PET_LOSS_MEAN || reduction == PET_LOSS_SUM, PET_ERR_ARGUMENT,
                "unknown reduction " + std::to_string(reduction));
    PET_REQUIRE(kind != PET_LOSS_HUBER || delta > 0.0, PET_ERR_ARGUMENT, "the Huber delta must be positive");  // (NaN fails too)
    PET_REQUIRE(weight == weight, PET_ERR_ARGUMENT, "the weight is NaN");
    PET_REQUIRE(reduction != PET_LOSS_MEAN || d_count, PET_ERR_ARGUMENT, "reduction = mean reads its denominator from d_count");
    if (d_col_scale)
        PET_REQUIRE(n_col_scale >= 1 && width % n_col_scale == 0, PET_ERR_ARGUMENT,
                    "the number of column scales must divide the values per row");
    else
        PET_REQUIRE(n_col_scale == 0, PET_ERR_ARGUMENT, "column scales counted but not given");
    if (rows == 0) return PET_OK;
    PET_REQUIRE(d_pred && d_target, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(d_seed != d_pred, PET_ERR_ARGUMENT, "seed == pred (the seeds are written out of place)");
    PET_REQUIRE(rows <= (INT64_MAX >> 1) / width, PET_ERR_ARGUMENT, "too many values");
    const int64_t chunks = (rows + LS_CHUNK - 1) / LS_CHUNK;
    PET_REQUIRE(chunks <= INT32_MAX, PET_ERR_ARGUMENT, "too many rows");
    PET_REQUIRE(d_workspace && workspace_bytes >= pet_loss_workspace_bytes(rows, width), PET_ERR_ARGUMENT,
                "workspace too small (pet_loss_workspace_bytes)");
    LossArgs a{d_pred, d_target, d_mask, d_row_scale, d_col_scale, d_col_scale ? n_col_scale : 1, rows, width, kind, delta, weight,
               reduction == PET_LOSS_MEAN ? d_count : nullptr, d_seed, (double*)d_workspace, d_loss, d_stats};
    hipStream_t st = (hipStream_t)stream;
    if (chunks == 1) {
        k_loss_pointwise<true><<<1, LS_BLOCK, 0, st>>>(a);
        PET_HIP_CHECK(hipGetLastError());
        return PET_OK;
    }
    k_loss_pointwise<false><<<(unsigned)chunks, LS_BLOCK, 0, st>>>(a);
    PET_HIP_CHECK(hipGetLastError());
    k_loss_final<<<1, 64, 0, st>>>(a, chunks);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // extern "C"
