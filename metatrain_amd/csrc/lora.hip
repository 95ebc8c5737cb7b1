// Fine-tuning support: LoRA adapters (pet/modules/finetuning.py LoRALinear: y = x W^T + b + s (x A^T) B^T) and frozen
// parameters.
//   inference: finalize folds W_eff = W + s B A once per Linear (fp64, fixed order); every packed / folded form of the
//              Linear is built from W_eff, so the forward kernels are the ones of a plain model;
//   training:  the reverse passes write dL/dW_eff of an adapted Linear into Model::lora_grad (Trainer::gp, TOps::slot);
//              lora_end projects it: dA += s B^T dW_eff, dB += s dW_eff A^T, dW += dW_eff (W trainable);
//   frozen:    a frozen parameter's slot is cleared at the end of every reverse entry point, the clipping norm and
//              Adam skip its entries (optim.hip).
#include <algorithm>
#include <map>
#include <vector>

#include "common.h"
#include "model.h"

namespace pet {

// W_eff[n][k] = W[n][k] + s sum_j B[n][j] A[j][k]; the sum in j order, fp64, one rounding
__global__ void k_lora_fold(const float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ B, double s,
                            int n_out, int k_in, int r, float* __restrict__ Weff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_out * k_in) return;
    const int n = (int)(i / k_in), k = (int)(i % k_in);
    double acc = 0.0;
    for (int j = 0; j < r; j++) acc += (double)B[(size_t)n * r + j] * (double)A[(size_t)j * k_in + k];
    Weff[i] = (float)((double)W[i] + s * acc);
}

// dA[j][k] += s sum_n B[n][j] G[n][k]  (n ascending),  dB[n][j] += s sum_k G[n][k] A[j][k]  (k ascending),
// dW[i] += G[i]; fp64 sums, one thread per output (deterministic). Null destinations are frozen: skipped.
__global__ void k_lora_project(const float* __restrict__ G, const float* __restrict__ A, const float* __restrict__ B,
                               double s, int n_out, int k_in, int r, float* __restrict__ dA, float* __restrict__ dB,
                               float* __restrict__ dW) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t na = (int64_t)r * k_in, nb = (int64_t)n_out * r, nw = (int64_t)n_out * k_in;
    if (i < na) {
        if (!dA) return;
        const int j = (int)(i / k_in), k = (int)(i % k_in);
        double acc = 0.0;
        for (int n = 0; n < n_out; n++) acc += (double)B[(size_t)n * r + j] * (double)G[(size_t)n * k_in + k];
        dA[i] += (float)(s * acc);
    } else if (i < na + nb) {
        if (!dB) return;
        const int64_t t = i - na;
        const int n = (int)(t / r), j = (int)(t % r);
        double acc = 0.0;
        for (int k = 0; k < k_in; k++) acc += (double)G[(size_t)n * k_in + k] * (double)A[(size_t)j * k_in + k];
        dB[t] += (float)(s * acc);
    } else if (i < na + nb + nw) {
        if (!dW) return;
        const int64_t t = i - na - nb;
        dW[t] += G[t];
    }
}

__global__ void k_clear_masked(float* __restrict__ g, const uint8_t* __restrict__ mask, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && mask[i]) g[i] = 0.f;
}

// the Linears an adapter may sit on (transformer.py: one transformer layer's attention, MLPs and node projections)
static const char* const LORA_PLACES[] = {"attention.input_linear", "attention.output_linear", "mlp.w_in", "mlp.w_out",
                                          "center_mlp.w_in", "center_mlp.w_out", "center_contraction", "center_expansion"};
static const char* const LORA_SUFFIXES[] = {".linear.weight", ".linear.bias", ".lora_A.weight", ".lora_B.weight"};

static bool ends_with(const std::string& s, const std::string& t) {
    return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}
static bool all_digits(const std::string& s) {
    if (s.empty()) return false;
    for (char c : s)
        if (c < '0' || c > '9') return false;
    return true;
}
// "<lin>" is gnn_layers.<g>.trans.layers.<a>.<place>
static bool served_place(const std::string& lin) {
    const std::string p0 = "gnn_layers.";
    if (lin.rfind(p0, 0) != 0) return false;
    size_t a = p0.size(), b = lin.find('.', a);
    if (b == std::string::npos || !all_digits(lin.substr(a, b - a))) return false;
    const std::string p1 = ".trans.layers.";
    if (lin.compare(b, p1.size(), p1) != 0) return false;
    a = b + p1.size();
    b = lin.find('.', a);
    if (b == std::string::npos || !all_digits(lin.substr(a, b - a))) return false;
    const std::string place = lin.substr(b + 1);
    for (const char* p : LORA_PLACES)
        if (place == p) return true;
    return false;
}

// the adapter suffix of an injected key, or -1 for an ordinary key
static int injected_suffix(const std::string& key) {
    const bool head = key.rfind("node_last_layers.", 0) == 0 || key.rfind("edge_last_layers.", 0) == 0;
    for (int i = 0; i < 4; i++)
        if (ends_with(key, LORA_SUFFIXES[i]) && (i >= 2 || !head)) return i;
    if (key.find(".lora_") != std::string::npos) return 4;  // an adapter tensor of another kind
    return -1;
}

int lora_register(Model& m, const std::string& key) {
    const int sfx = injected_suffix(key);
    if (sfx < 0) return PET_OK;
    const std::string lin = sfx < 4 ? key.substr(0, key.size() - std::string(LORA_SUFFIXES[sfx]).size()) : key;
    PET_REQUIRE(sfx < 4 && served_place(lin), PET_ERR_UNSUPPORTED,
                "LoRA adapter key '" + key + "' is not served: adapters go on attention.input_linear / output_linear, "
                "mlp.w_in / w_out, center_mlp.w_in / w_out, center_contraction / center_expansion of a transformer layer");
    m.lora[lin];  // registered; shapes, rank and scaling are checked by finalize
    return PET_OK;
}

int lora_set_scaling(Model& m, const std::string& lin, float scaling) {
    PET_REQUIRE(served_place(lin), PET_ERR_UNSUPPORTED, "LoRA adapter on '" + lin + "' is not served");
    LoraW& L = m.lora[lin];
    L.scaling = scaling;
    L.has_scaling = true;
    m.finalized = false;
    return PET_OK;
}

int lora_resolve(Model& m, const std::string& lin, int n_out, int k_in, const float** w, const float** b, hipStream_t st) {
    *w = *b = nullptr;
    auto it = m.lora.find(lin);
    if (it == m.lora.end()) return PET_OK;
    LoraW& L = it->second;
    auto raw = [&](const char* sfx, int64_t* numel) -> const float* {
        auto r = m.raw.find(lin + sfx);
        if (r == m.raw.end()) return nullptr;
        *numel = r->second.second;
        return r->second.first;
    };
    int64_t nw = 0, nbias = 0, na = 0, nb = 0;
    const float *W = raw(".linear.weight", &nw), *bias = raw(".linear.bias", &nbias), *A = raw(".lora_A.weight", &na),
                *B = raw(".lora_B.weight", &nb);
    PET_REQUIRE(W && bias && A && B, PET_ERR_ARGUMENT,
                "LoRA adapter '" + lin + "' needs .linear.weight, .linear.bias, .lora_A.weight and .lora_B.weight");
    PET_REQUIRE(nw == (int64_t)n_out * k_in && nbias == n_out, PET_ERR_ARGUMENT,
                "LoRA adapter '" + lin + "': the base Linear has " + std::to_string(nw) + " weights, expected " +
                    std::to_string((int64_t)n_out * k_in));
    const int r = (int)(na / k_in);
    PET_REQUIRE(na % k_in == 0 && (int64_t)n_out * r == nb, PET_ERR_ARGUMENT,
                "LoRA adapter '" + lin + "': lora_A [r, " + std::to_string(k_in) + "] and lora_B [" + std::to_string(n_out) +
                    ", r] do not fit the base Linear (" + std::to_string(na) + " and " + std::to_string(nb) + " elements)");
    PET_REQUIRE(r >= 1 && r <= 64, PET_ERR_UNSUPPORTED,
                "LoRA adapter '" + lin + ".lora_A.weight': rank " + std::to_string(r) + " is not served (1 .. 64)");
    PET_REQUIRE(L.has_scaling, PET_ERR_ARGUMENT, "LoRA adapter '" + lin + "' has no scaling (pet_model_set_lora_scaling)");
    if (!L.w_eff) {  // once per adapter: its shape is that of the base weight, which cannot change size
        int rc = dev_alloc(m, (void**)&L.w_eff, (size_t)nw * sizeof(float));
        if (rc) return rc;
    }
    L.rank = r; L.n_out = n_out; L.k_in = k_in;
    L.w = W; L.a = A; L.b = B;
    k_lora_fold<<<cdiv(nw, 256), 256, 0, st>>>(W, A, B, (double)L.scaling, n_out, k_in, r, L.w_eff);
    PET_HIP_CHECK(hipGetLastError());
    *w = L.w_eff;
    *b = bias;
    return PET_OK;
}

int lora_check_all_folded(const Model& m, const std::set<std::string>& folded) {
    for (const auto& kv : m.lora)
        PET_REQUIRE(folded.count(kv.first), PET_ERR_UNSUPPORTED,
                    "LoRA adapter '" + kv.first + "' is on a Linear this model does not have");
    return PET_OK;
}

// a device buffer of the model replaced by a larger one (the old one is freed)
static int regrow(Model& m, void** p, size_t bytes) {
    if (*p) {
        PET_HIP_CHECK(hipFree(*p));
        m.owned.erase(std::find(m.owned.begin(), m.owned.end(), *p));
        *p = nullptr;
    }
    return dev_alloc(m, p, bytes);
}

int lora_begin(Model& m, hipStream_t st) {
    if (m.lora.empty()) return PET_OK;
    int64_t total = 0;
    for (auto& kv : m.lora) {
        kv.second.dw_off = total;
        total += (int64_t)kv.second.n_out * kv.second.k_in;
    }
    if (total > m.lora_floats) {  // (more adapters than at the last call)
        int rc = regrow(m, (void**)&m.lora_grad, (size_t)total * sizeof(float));
        if (rc) return rc;
        m.lora_floats = total;
    }
    PET_HIP_CHECK(hipMemsetAsync(m.lora_grad, 0, (size_t)total * sizeof(float), st));
    return PET_OK;
}

static int ensure_frozen_mask(Model& m, hipStream_t st) {
    if (!m.frozen_dirty && m.frozen_mask_n == m.n_params) return PET_OK;
    if (m.frozen_mask_n != m.n_params) {  // parameters were uploaded since: the mask covers the whole flat layout
        int rc = regrow(m, (void**)&m.d_frozen, (size_t)m.n_params);
        if (rc) return rc;
        m.frozen_mask_n = m.n_params;
    }
    std::vector<uint8_t> mask((size_t)m.n_params, 0);
    for (const auto& k : m.frozen) {
        const int64_t off = m.grad_off.at(k), n = m.raw.at(k).second;
        std::fill(mask.begin() + off, mask.begin() + off + n, (uint8_t)1);
    }
    PET_HIP_CHECK(hipMemcpyAsync(m.d_frozen, mask.data(), mask.size(), hipMemcpyHostToDevice, st));
    PET_HIP_CHECK(hipStreamSynchronize(st));
    m.frozen_dirty = false;
    return PET_OK;
}

const uint8_t* frozen_mask(Model& m, hipStream_t st) {
    if (m.frozen.empty()) return nullptr;
    return ensure_frozen_mask(m, st) == PET_OK ? m.d_frozen : nullptr;
}

int lora_end(Model& m, hipStream_t st) {
    for (const auto& kv : m.lora) {
        const LoraW& L = kv.second;
        auto slot = [&](const char* sfx) -> float* {
            const std::string k = kv.first + sfx;
            return m.is_frozen(k) ? nullptr : m.grad_flat + m.grad_off.at(k);
        };
        const int64_t n = (int64_t)L.rank * L.k_in + (int64_t)L.n_out * L.rank + (int64_t)L.n_out * L.k_in;
        k_lora_project<<<cdiv(n, 256), 256, 0, st>>>(m.lora_grad + L.dw_off, L.a, L.b, (double)L.scaling, L.n_out, L.k_in,
                                                     L.rank, slot(".lora_A.weight"), slot(".lora_B.weight"),
                                                     slot(".linear.weight"));
    }
    if (!m.frozen.empty()) {
        int rc;
        if ((rc = ensure_frozen_mask(m, st))) return rc;
        k_clear_masked<<<cdiv(m.n_params, 256), 256, 0, st>>>(m.grad_flat, m.d_frozen, m.n_params);
    }
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

int set_trainable(Model& m, const std::string& key, bool trainable) {
    PET_REQUIRE(m.grad_off.count(key), PET_ERR_ARGUMENT, "unknown parameter '" + key + "'");
    const bool was = m.frozen.count(key) > 0;
    if (trainable == !was) return PET_OK;
    if (trainable) m.frozen.erase(key);
    else m.frozen.insert(key);
    m.frozen_dirty = true;
    return PET_OK;
}

}  // namespace pet
