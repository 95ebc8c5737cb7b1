// Last-layer features of the SOAP-BPNN tail for LLPR (llpr/model.py; soap_bpnn/model.py:347-351, 664-697), and the soap_*
// entries of the four LLPR kernels of llpr.hip, which take a feature width F and know nothing about the model in front.
//
//   x_i = silu(a_q[i])  [H]     a_q the pre-activation of native tail layer q = NH - back (back = 0: the input of the last
//                               layer, the reference's last-layer features; back = 1: one layer below, which is the `feature`
//                               output of a model whose mlp head runs as the tail's last layer)
//   legacy = False:  LLF [N, H] = x
//   legacy = True:   LLF [N, ns H], x_i in columns [s_i H, (s_i + 1) H), every other column 0   (keys_to_properties("center_type"))
//
// Every tail kernel leaves tail[i] = {mean, rstd, a1[H], a2[H]} and, beyond two layers, tail_ext[i][NH - 2][H] in the forward's
// workspace (soap_tail.hip), whichever form of the tail ran and whichever layout the power spectrum had: nothing is recomputed.
#include "soap.h"

namespace pet {

// One thread per V consecutive output columns, threads consecutive along F: the [N, F] array is written once, whole, in
// order, zeros included (the wave-per-atom mapping of k_soap_tail_extra_fwd would leave 3 lanes in 4 idle at H = 16 and
// write F / H separate runs per atom). V = 4 when H % 4 == 0: a group of four columns then lies inside the atom's block or
// outside it, and rows of F floats keep 16-byte alignment. The source rows start 8 bytes into a tail record, so they are
// read as scalars; they are one eighth (legacy, eight species) to all of the traffic and stay coalesced.
template <int V>
__global__ __launch_bounds__(256) void k_soap_llpr_features(const float* __restrict__ src, int64_t stride, int H, int F,
                                                            int legacy, const int* __restrict__ sp, int64_t N,
                                                            float* __restrict__ llf) {
    const int per = F / V;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N * per) return;
    const int64_t i = t / per;
    const int c = (int)(t - i * per) * V;
    const int c0 = legacy ? sp[i] * H : 0;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; k++) v[k] = 0.f;
    if (c >= c0 && c < c0 + H) {
        const float* a = src + i * stride + (c - c0);
#pragma unroll
        for (int k = 0; k < V; k++) v[k] = silu(a[k]);
    }
    if constexpr (V == 4) reinterpret_cast<float4*>(llf)[t] = make_float4(v[0], v[1], v[2], v[3]);
    else llf[t] = v[0];
}

int soap_llpr_feats(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, int back, float* llf, hipStream_t st) {
    const SoapDims& d = m.d;
    const int64_t N = g.n_nodes;
    PET_REQUIRE(back == 0 || back == 1, PET_ERR_ARGUMENT, "layer = " + std::to_string(back) + ": 0 (the last layer's input) or 1 (the layer below)");
    PET_REQUIRE(d.NH - back >= 1, PET_ERR_ARGUMENT, "layer = 1 on a tail of one layer: there is no hidden layer below the last one");
    SoapWs w;
    carve_soap(d, N, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT,
                "soap workspace too small: " + std::to_string(ws_bytes) + " bytes, this graph needs " + std::to_string(w.bytes));
    PET_REQUIRE(g.fwd_record(ws) != nullptr, PET_ERR_ARGUMENT,
                "no soap_forward of this graph into this workspace (never run, or pushed out by forwards into four other "
                "workspaces): the last-layer features are read from what the forward left there");
    const int H = d.H, F = soap_llpr_width(d), q = d.NH - back;
    const float* src = q == 1 ? w.tail + 2 : q == 2 ? w.tail + 2 + H : w.tail_ext + (size_t)(q - 3) * H;
    const int64_t stride = q <= 2 ? 2 + 2 * H : (int64_t)(d.NH - 2) * H;
    if (H % 4 == 0)
        k_soap_llpr_features<4><<<cdiv(N * (F / 4), 256), 256, 0, st>>>(src, stride, H, F, d.legacy, g.sp, N, llf);
    else
        k_soap_llpr_features<1><<<cdiv(N * F, 256), 256, 0, st>>>(src, stride, H, F, d.legacy, g.sp, N, llf);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace pet

using namespace pet;

static int soap_llpr_check_f(const soap_model_t* sm, int64_t F) {
    PET_REQUIRE(sm, PET_ERR_ARGUMENT, "null model");
    PET_REQUIRE(F == soap_llpr_feature_size(sm), PET_ERR_ARGUMENT,
                "F = " + std::to_string(F) + " is not this model's last-layer feature size " +
                    std::to_string(soap_llpr_feature_size(sm)) + " (num_neurons_per_layer, times n_species when legacy)");
    return PET_OK;
}

extern "C" {

int64_t soap_llpr_feature_size(const soap_model_t* sm) { return sm ? soap_llpr_width(sm->m.d) : -1; }

int soap_llpr_features(const soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                       int32_t layer, float* d_llf, void* stream) {
    PET_REQUIRE(sm && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(sm->m.finalized, PET_ERR_ARGUMENT, "soap_model_finalize has not been called");
    if (pg->g.n_nodes == 0) return PET_OK;  // an empty batch: nothing to write, and its forward left no record
    PET_REQUIRE(d_workspace && d_llf, PET_ERR_ARGUMENT, "null argument");
    return soap_llpr_feats(sm->m, pg->g, d_workspace, workspace_bytes, layer, d_llf, (hipStream_t)stream);
}

// the arguments and checks of the pet_llpr_* entries (abi.hip), F checked against this model
int soap_llpr_rows(const soap_model_t* sm, int64_t F, const float* d_llf, int64_t n_atoms, const int32_t* d_system_indices,
                   int64_t n_systems, const uint8_t* d_mask, int mean, float* d_rows, void* stream) {
    if (int rc = soap_llpr_check_f(sm, F)) return rc;
    PET_REQUIRE(n_atoms >= 0 && n_systems > 0, PET_ERR_ARGUMENT, "n_atoms < 0 or n_systems <= 0");
    PET_REQUIRE(d_rows && (n_atoms == 0 || (d_llf && d_system_indices)), PET_ERR_ARGUMENT, "null argument");
    return llpr_rows(d_llf, n_atoms, (int)F, d_system_indices, n_systems, d_mask, mean, d_rows, (hipStream_t)stream);
}

int soap_llpr_covariance_accumulate(const soap_model_t* sm, int64_t F, const float* d_x, int64_t R, double* d_cov,
                                    void* stream) {
    if (int rc = soap_llpr_check_f(sm, F)) return rc;
    PET_REQUIRE(R > 0, PET_ERR_ARGUMENT, "R <= 0 rows");
    PET_REQUIRE(d_x && d_cov, PET_ERR_ARGUMENT, "null argument");
    return llpr_covariance_accumulate(d_x, R, (int)F, d_cov, (hipStream_t)stream);
}

int soap_llpr_covariance_finalize(const soap_model_t* sm, int64_t F, double* d_cov, void* stream) {
    if (int rc = soap_llpr_check_f(sm, F)) return rc;
    PET_REQUIRE(d_cov, PET_ERR_ARGUMENT, "null argument");
    return llpr_covariance_finalize(d_cov, (int)F, (hipStream_t)stream);
}

int soap_llpr_variance(const soap_model_t* sm, int64_t F, const float* d_x, int64_t R, const float* d_inv_cholesky,
                       float alpha, float* d_sigma, void* stream) {
    if (int rc = soap_llpr_check_f(sm, F)) return rc;
    PET_REQUIRE(R > 0, PET_ERR_ARGUMENT, "R <= 0 rows");
    PET_REQUIRE(d_x && d_inv_cholesky && d_sigma, PET_ERR_ARGUMENT, "null argument");
    return llpr_variance(d_x, R, (int)F, d_inv_cholesky, alpha, d_sigma, (hipStream_t)stream);
}

int soap_llpr_ensemble(const soap_model_t* sm, int64_t F, const float* d_x, int64_t R, const float* d_weights, int32_t K,
                       int32_t P, const float* d_prediction, float* d_out, void* stream) {
    if (int rc = soap_llpr_check_f(sm, F)) return rc;
    PET_REQUIRE(R > 0, PET_ERR_ARGUMENT, "R <= 0 rows");
    PET_REQUIRE(K > 0 && P > 0 && (int64_t)K * P <= PET_LLPR_MAX_ENSEMBLE, PET_ERR_ARGUMENT,
                "K P = " + std::to_string((int64_t)K * P) + " outside [1, " + std::to_string(PET_LLPR_MAX_ENSEMBLE) + "]");
    PET_REQUIRE(d_x && d_weights && d_out, PET_ERR_ARGUMENT, "null argument");
    return llpr_ensemble(d_x, R, (int)F, d_weights, K, P, d_prediction, d_out, (hipStream_t)stream);
}

}  // extern "C"
