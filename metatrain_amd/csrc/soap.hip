// SOAP-BPNN hot path for gfx950: spherical expansion, power spectrum,
// LayerNorm + MLP tail, and the hand-written reverse pass for dE/dR. See include/soap_hip.h.
//
//   c[i][l][m][n][a] = sum_{p in row i} Y_lm(r_p / |r_p|) R_nl(|r_p|) fc(|r_p|) w_a(species of neighbour)   (a17, spex)
//   ps[i][l][(n a), (n' a')] = sum_m c[i][l][m][n a] c[i][l][m][n' a']        power_spectrum.py:125-136
//   e_i = w3 . silu(W2 silu(W1 LN(ps_i * enc[s_i])))                           model.py:553-595, 1204-1219
//
// This file: the model (soap_finalize), the plan (soap_plan.h: which kernel serves each stage), the two drivers and the
// extern "C" entries. The stages and their launchers: soap_expand.hip, soap_ps.hip, soap_tail.hip; training: soap_train.hip;
// Hessian-vector product: soap_hvp.hip.
#include "soap.h"

namespace pet {

// ---------------------------------------------------------------------------------------------
// the model
// ---------------------------------------------------------------------------------------------
static int soap_get(const SoapModel& m, const std::string& key, int64_t numel, const float** out) {
    auto it = m.raw.find(key);
    PET_REQUIRE(it != m.raw.end(), PET_ERR_ARGUMENT, "missing parameter '" + key + "'");
    PET_REQUIRE(it->second.second == numel, PET_ERR_ARGUMENT, "parameter '" + key + "' has the wrong size");
    *out = it->second.first;
    return PET_OK;
}

int soap_finalize(SoapModel& m, hipStream_t st) {
    const SoapDims& d = m.d;
    PET_REQUIRE(m.table != nullptr, PET_ERR_ARGUMENT, "soap_model_set_radial_table has not been called");
    int rc;
    // normalisation of the real spherical harmonics: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) [* sqrt 2]
    std::vector<float> shn((d.L + 1) * (d.L + 1), 0.f);
    for (int l = 0; l <= d.L; l++)
        for (int mm = 0; mm <= l; mm++) {
            double f = (2 * l + 1) / (4.0 * M_PI);
            for (int k = l - mm + 1; k <= l + mm; k++) f /= k;
            shn[l * (d.L + 1) + mm] = (float)(sqrt(f) * (mm > 0 ? sqrt(2.0) : 1.0));
        }
    std::vector<int> clut(d.NCOEF), ilut(d.ITEMS);
    int idx = 0, it = 0;
    for (int l = 0; l <= d.L; l++)
        for (int mi = 0; mi < 2 * l + 1; mi++)
            for (int n = 0; n < d.n_per_l[l]; n++) {
                const int lm = l * l + mi, rn = d.rad_off[l] + n;
                ilut[it++] = lm | (rn << 8) | (idx << 16);
                for (int a = 0; a < d.C; a++) clut[idx++] = lm | (rn << 8) | (a << 16);
            }
    std::vector<int2> flut(d.S), olut(d.NCOEF);
    for (int l = 0; l <= d.L; l++) {
        const int nc = d.n_per_l[l] * d.C, M = 2 * l + 1;
        for (int a = 0; a < nc; a++)
            for (int b = 0; b < nc; b++)
                flut[d.feat_off[l] + a * nc + b] = make_int2(d.coef_off[l] + a, (d.coef_off[l] + b) | (M << 16) | (nc << 24));
        for (int mi = 0; mi < M; mi++)
            for (int a = 0; a < nc; a++)
                olut[d.coef_off[l] + mi * nc + a] = make_int2(d.feat_off[l] + a, (d.coef_off[l] + mi * nc) | (nc << 16));
    }
    if (!m.shnorm) {
        if ((rc = salloc(m, (void**)&m.feat_lut, flut.size() * sizeof(int2)))) return rc;
        if ((rc = salloc(m, (void**)&m.out_lut, olut.size() * sizeof(int2)))) return rc;
        if ((rc = salloc(m, (void**)&m.shnorm, shn.size() * 4))) return rc;
        if ((rc = salloc(m, (void**)&m.coef_lut, clut.size() * 4))) return rc;
        if ((rc = salloc(m, (void**)&m.item_lut, ilut.size() * 4))) return rc;
        if ((rc = salloc(m, (void**)&m.species_w, (size_t)d.ns * d.C * 4))) return rc;
        if ((rc = salloc(m, (void**)&m.sets, sizeof(SoapSet) * m.n_sets))) return rc;
    }
    PET_HIP_CHECK(hipMemcpyAsync(m.shnorm, shn.data(), shn.size() * 4, hipMemcpyHostToDevice, st));
    PET_HIP_CHECK(hipMemcpyAsync(m.coef_lut, clut.data(), clut.size() * 4, hipMemcpyHostToDevice, st));
    PET_HIP_CHECK(hipMemcpyAsync(m.item_lut, ilut.data(), ilut.size() * 4, hipMemcpyHostToDevice, st));
    PET_HIP_CHECK(hipMemcpyAsync(m.feat_lut, flut.data(), flut.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    PET_HIP_CHECK(hipMemcpyAsync(m.out_lut, olut.data(), olut.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    if (d.legacy) {
        std::vector<float> eye((size_t)d.ns * d.C, 0.f);
        for (int s = 0; s < d.ns; s++) eye[s * d.C + s] = 1.f;
        PET_HIP_CHECK(hipMemcpyAsync(m.species_w, eye.data(), eye.size() * 4, hipMemcpyHostToDevice, st));
        m.enc = nullptr;
    } else {
        const float* emb;
        if ((rc = soap_get(m, "species_embedding.weight", (int64_t)d.ns * d.C, &emb))) return rc;
        PET_HIP_CHECK(hipMemcpyAsync(m.species_w, emb, (size_t)d.ns * d.C * 4, hipMemcpyDeviceToDevice, st));
        if ((rc = soap_get(m, "center_encoding.weight", (int64_t)d.ns * d.S, &m.enc))) return rc;
    }
    std::vector<SoapSet> sets(m.n_sets);
    for (int s = 0; s < m.n_sets; s++) {
        const std::string ss = std::to_string(s);
        if (d.layernorm) {
            if ((rc = soap_get(m, "layernorm." + ss + ".weight", d.S, &sets[s].ln_w))) return rc;
            if ((rc = soap_get(m, "layernorm." + ss + ".bias", d.S, &sets[s].ln_b))) return rc;
        }
        if ((rc = soap_get(m, "bpnn." + ss + ".0.weight", (int64_t)d.H * d.S, &sets[s].W1))) return rc;
        for (int k = 1; k < d.NH; k++)
            if ((rc = soap_get(m, "bpnn." + ss + "." + std::to_string(2 * k) + ".weight", (int64_t)d.H * d.H,
                               &sets[s].Wh[k - 1])))
                return rc;
        sets[s].W2 = sets[s].Wh[0];
        if ((rc = soap_get(m, "last_layers.energy." + ss + ".weight", d.H, &sets[s].w3))) return rc;
    }
    PET_HIP_CHECK(hipMemcpyAsync(m.sets, sets.data(), sizeof(SoapSet) * m.n_sets, hipMemcpyHostToDevice, st));
    // stacked first Linear for the MFMA tail
    m.NT = 0;
    if (d.H == 32 && m.n_sets <= 8 && d.S % 4 == 0) {
        const int NT = (m.n_sets + 1) / 2, NOUTP = 64 * NT, Kp = (d.S + 127) / 128 * 128;
        if (!m.wall || m.NOUTP != NOUTP || m.Kp != Kp) {
            const size_t n4 = (size_t)NOUTP * Kp / 4;
            if ((rc = salloc(m, (void**)&m.wall, (size_t)NOUTP * Kp * 4))) return rc;
            if ((rc = salloc(m, (void**)&m.wall_fwd, n4 * sizeof(float4)))) return rc;
            if ((rc = salloc(m, (void**)&m.wall_bwd, n4 * sizeof(float4)))) return rc;
            if ((rc = salloc(m, (void**)&m.wall_rs, NOUTP * 4))) return rc;
            if ((rc = salloc(m, (void**)&m.wall_b, NOUTP * 4))) return rc;
        }
        m.NT = NT; m.NOUTP = NOUTP; m.Kp = Kp;
        const size_t n4 = (size_t)NOUTP * Kp / 4;
        k_soap_prep_wall<<<cdiv((int64_t)NOUTP * Kp, 256), 256, 0, st>>>(d, m.sets, m.n_sets, NOUTP, Kp, m.wall);
        k_soap_prep_rows<<<cdiv(NOUTP, 64), 64, 0, st>>>(d, m.sets, m.n_sets, NOUTP, Kp, m.wall, m.wall_rs, m.wall_b);
        k_pack<<<cdiv(n4, 256), 256, 0, st>>>(m.wall, Kp, 1, NOUTP, Kp, m.wall_fwd);   // x W^T: tiles over NOUTP
        k_pack<<<cdiv(n4, 256), 256, 0, st>>>(m.wall, 1, Kp, Kp, NOUTP, m.wall_bwd);   // dy W: tiles over Kp
        {   // the same weights network by network, for the species-sorted tiles
            const size_t per = (size_t)(Kp / 8) * 64;  // float4 per network, both orientations
            if (!m.wall_fwd_set) {
                if ((rc = salloc(m, (void**)&m.wall_fwd_set, m.n_sets * per * sizeof(float4)))) return rc;
                if ((rc = salloc(m, (void**)&m.wall_bwd_set, m.n_sets * per * sizeof(float4)))) return rc;
            }
            for (int sset = 0; sset < m.n_sets; sset++) {
                const float* ws = m.wall + (size_t)sset * d.H * Kp;
                k_pack<<<cdiv(per, 256), 256, 0, st>>>(ws, Kp, 1, d.H, Kp, m.wall_fwd_set + sset * per);
                k_pack<<<cdiv(per, 256), 256, 0, st>>>(ws, 1, Kp, Kp, d.H, m.wall_bwd_set + sset * per);
            }
        }
        if (d.ncmax <= 32 && d.Sp % 4 == 0) {  // packed power spectrum: the networks' first Linear over the upper-triangle layout
            const int Kpp = (d.Sp + 127) / 128 * 128;
            const size_t per = (size_t)(Kpp / 8) * 64, nw = (size_t)m.n_sets * d.H * Kpp;
            if (!m.wallp || m.Kpp != Kpp) {
                if ((rc = salloc(m, (void**)&m.wallp, nw * 4))) return rc;
                if ((rc = salloc(m, (void**)&m.wallpb, nw * 4))) return rc;
                if ((rc = salloc(m, (void**)&m.wallp_fwd_set, m.n_sets * per * sizeof(float4)))) return rc;
                if ((rc = salloc(m, (void**)&m.wallp_bwd_set, m.n_sets * per * sizeof(float4)))) return rc;
            }
            m.Kpp = Kpp;
            k_soap_prep_wallp<<<cdiv((int64_t)nw, 256), 256, 0, st>>>(d, m.sets, m.n_sets, Kpp, 0, m.wallp);
            k_soap_prep_wallp<<<cdiv((int64_t)nw, 256), 256, 0, st>>>(d, m.sets, m.n_sets, Kpp, 1, m.wallpb);
            for (int sset = 0; sset < m.n_sets; sset++) {
                k_pack<<<cdiv(per, 256), 256, 0, st>>>(m.wallp + (size_t)sset * d.H * Kpp, Kpp, 1, d.H, Kpp,
                                                        m.wallp_fwd_set + sset * per);
                k_pack<<<cdiv(per, 256), 256, 0, st>>>(m.wallpb + (size_t)sset * d.H * Kpp, 1, Kpp, Kpp, d.H,
                                                        m.wallp_bwd_set + sset * per);
            }
        }
        PET_HIP_CHECK(hipGetLastError());
    }
    PET_HIP_CHECK(hipStreamSynchronize(st));  // host vectors go out of scope
    m.finalized = true;
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// the plan (soap_plan.h): every condition of the pass, once
// ---------------------------------------------------------------------------------------------
// the wave-per-atom expansion and its lane-per-pair adjoint: four species channels as one float4, items and table indices
// inside their packed fields
static bool soap_pair_ok(const SoapDims& d) {
    return switches().soap_pair && d.C == 4 && d.ITEMS <= 64 * MAXI && d.NLM <= 255 && d.F <= 255 && d.NCOEF < 32768;
}
// the species-sorted tail tiles: the per-network weight planes exist and the networks fit the forward's bucket table
static bool soap_sorted_ok(const SoapModel& m) {
    return switches().soap_sorted && switches().soap_mfma && m.NT > 0 && m.wall_fwd_set != nullptr && m.n_sets <= SP_MAXSETS;
}
static bool soap_packed_ok(const SoapModel& m) {
    for (int l = 0; l <= m.d.L; l++) {  // every block's triangle an even number of floats (k_soap_ps_m<true> stores 8 bytes per lane)
        const int nc = m.d.n_per_l[l] * m.d.C;
        if ((nc * (nc + 1) / 2) % 2) return false;
    }
    const Switches& sw = switches();
    return sw.soap_packed && sw.soap_pair && sw.soap_ps_mfma && m.enc == nullptr && m.wallp_fwd_set != nullptr &&
           m.d.ncmax <= 32 && (size_t)(m.d.NCOEF + m.d.Sp) * 4 <= 64 * 1024;
}
static SoapPlan::Tail soap_tail_form(const SoapModel& m) {  // the same conditions serve the tail and its adjoint
    if (soap_sorted_ok(m)) return SoapPlan::Tail::Sorted;
    return m.NT > 0 && switches().soap_mfma ? SoapPlan::Tail::Stacked : SoapPlan::Tail::PerAtom;
}
// soap_bwd / soap_train_grads without a record of the workspace's forward (Graph::FwdRecord: the last four workspaces)
static constexpr const char* SOAP_NO_FORWARD =
    "no soap_forward of this graph into this workspace (never run, or pushed out by forwards into four other workspaces)";

SoapPlan soap_plan_forward(const SoapModel& m, const Graph&, bool want_features) {
    using PS = SoapPlan::PowerSpectrum;
    const SoapDims& d = m.d;
    const Switches& sw = switches();
    SoapPlan p;
    p.expand = soap_pair_ok(d) ? SoapPlan::Expand::Wave : SoapPlan::Expand::PerAtom;
    p.wide_l = d.L > 6;
    p.tail = soap_tail_form(m);
    p.bucketed = p.tail == SoapPlan::Tail::Sorted;
    p.deep_tail = d.NH > 2;
    // the packed layout: read by the sorted tail alone, and never handed out (a caller's features are the full layout)
    p.packed = p.tail == SoapPlan::Tail::Sorted && soap_packed_ok(m) && !want_features;
    p.ps = p.packed                                               ? PS::MfmaPacked
           : sw.soap_pair && sw.soap_ps_mfma && d.ncmax <= 32      ? PS::Mfma  // an l block inside one 32 x 32 tile
           : sw.soap_pair && d.ncmax < 128 && d.NCOEF < 65536      ? PS::Lut   // the table's packed fields
                                                                   : PS::PerAtom;
    return p;
}

int soap_plan_backward(const SoapModel& m, const Graph&, const FwdRecord* rec, SoapPlan& p) {
    using PS = SoapPlan::PowerSpectrum;
    const SoapDims& d = m.d;
    const Switches& sw = switches();
    PET_REQUIRE(rec, PET_ERR_ARGUMENT, SOAP_NO_FORWARD);
    p = SoapPlan();
    p.packed = rec->soap_plan.packed;  // what the forward into this workspace stored
    PET_REQUIRE(!p.packed || (soap_sorted_ok(m) && soap_packed_ok(m)), PET_ERR_ARGUMENT,
                "the forward of this workspace stored the packed power spectrum but the adjoint is configured for the full "
                "layout: pet_config_set changed between soap_forward and soap_backward");
    p.tail = soap_tail_form(m);
    // (the other direction needs no refusal: every tail form leaves {mean, rstd, a1, a2} per atom in the same place, so the
    // stacked and per-atom adjoints follow a forward that bucketed)
    PET_REQUIRE(p.tail != SoapPlan::Tail::Sorted || rec->soap_plan.bucketed, PET_ERR_ARGUMENT,
                "the forward of this workspace did not bucket the atoms by network but the adjoint is configured for the "
                "species-sorted tail: pet_config_set(\"soap_sorted\" / \"soap_mfma\") changed between soap_forward and "
                "soap_backward");
    p.deep_tail = d.NH > 2;
    // the adjoint's own conditions: a staged dF row of whole float4 beside the atom's coefficients in 64 KB of LDS
    const bool row_fits = d.S % 4 == 0 && (size_t)(d.NCOEF + d.S) * 4 <= 64 * 1024;
    p.ps = p.packed                                            ? PS::MfmaPacked
           : sw.soap_pair && sw.soap_ps_mfma && row_fits        ? PS::Mfma
           : sw.soap_pair && row_fits && d.NCOEF < 65536        ? PS::Lut
                                                                : PS::PerAtom;
    p.expand = soap_pair_ok(d) ? SoapPlan::Expand::Wave : SoapPlan::Expand::PerAtom;
    p.wide_l = d.L > 6;
    p.lds_rows = d.NCOEF % 4 == 0 ? 16 * 1024 : 0;  // float4 rows, or none staged
    return PET_OK;
}

int soap_plan_train(const SoapModel& m, const FwdRecord* rec, SoapTrainPlan& t) {
    PET_REQUIRE(rec, PET_ERR_ARGUMENT, SOAP_NO_FORWARD);
    t.rebuild_full = rec->soap_plan.packed;
    t.wide_table = m.n_sets > SP_MAXSETS;
    return PET_OK;
}

// ---------------------------------------------------------------------------------------------
// the drivers: carve, plan, launch
// ---------------------------------------------------------------------------------------------
static int soap_fwd(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, float* atomic, float* features,
                    hipStream_t st) {
    SoapWs w;
    carve_soap(m.d, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "soap workspace too small");
    const int N = (int)g.n_nodes;
    if (N == 0) return PET_OK;
    const SoapPlan p = soap_plan_forward(m, g, features != nullptr);
    launch_soap_expand(p, m, g, w, st);
    g.fwd_record_new(ws).soap_plan = p;  // soap_bwd and the training pass follow what this forward stores
    launch_soap_ps(p, m, g, w, st);
    PET_TRY(launch_soap_tail(p, m, g, w, atomic, st));
    if (features)
        PET_HIP_CHECK(hipMemcpyAsync(features, w.feats, (size_t)N * m.d.S * 4, hipMemcpyDeviceToDevice, st));
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

static int soap_bwd(const SoapModel& m, const Graph& g, void* ws, int64_t ws_bytes, const float* gA, float* gpos,
                    float* gcell, hipStream_t st) {
    SoapWs w;
    carve_soap(m.d, g.n_nodes, g.n_edges, ws, w);
    PET_REQUIRE((int64_t)w.bytes <= ws_bytes, PET_ERR_ARGUMENT, "soap workspace too small");
    const int N = (int)g.n_nodes;
    if (N == 0) return PET_OK;
    SoapPlan p;
    PET_TRY(soap_plan_backward(m, g, g.fwd_record(ws), p));  // (refusals first: nothing is launched or cleared behind one)
    if (g.n_edges == 0) {
        PET_HIP_CHECK(hipMemsetAsync(gpos, 0, (size_t)N * 3 * 4, st));
        if (gcell) PET_HIP_CHECK(hipMemsetAsync(gcell, 0, g.n_systems * 9 * 4, st));
        return PET_OK;
    }
    launch_soap_tail_bwd(p, m, g, w, gA, st);
    launch_soap_ps_bwd(p, m, g, w, st);
    launch_soap_expand_bwd(p, m, g, w, st);
    k_pos_grad<<<cdiv(N, 16), 256, 0, st>>>(reinterpret_cast<const float4*>(w.dv), g.rowptr, g.rev, gpos, N);
    if (gcell)
        k_cell_grad<<<(int)g.n_systems, 256, 0, st>>>(reinterpret_cast<const float4*>(w.dv), g.shift, g.ctr, g.sys,
                                                      g.rowptr, gcell, N, g.n_edges, 0);
    PET_HIP_CHECK(hipGetLastError());
    return PET_OK;
}

}  // namespace pet

using namespace pet;

extern "C" {

int soap_model_create(const soap_hypers_t* h, soap_model_t** out) {
    PET_REQUIRE(h && out, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(h->max_angular >= 0 && h->max_angular <= SOAP_MAX_L, PET_ERR_UNSUPPORTED, "max_angular out of range");
    PET_REQUIRE(h->num_neurons_per_layer >= 1 && h->num_neurons_per_layer <= MAXH, PET_ERR_UNSUPPORTED,
                "num_neurons_per_layer > 64 is not built");
    PET_REQUIRE(h->num_hidden_layers >= 1 && h->num_hidden_layers <= MAXNH, PET_ERR_UNSUPPORTED,
                "num_hidden_layers must be 1 .. 8");
    PET_REQUIRE(h->n_species >= 1 && h->n_channels >= 1 && h->n_channels <= 255, PET_ERR_ARGUMENT, "bad species counts");
    PET_REQUIRE(!h->legacy || h->n_channels == h->n_species, PET_ERR_ARGUMENT,
                "legacy (Orthogonal species): n_channels must equal n_species");
    soap_model_t* sm = new soap_model_t();
    SoapModel& m = sm->m;
    m.h = *h;
    SoapDims& d = m.d;
    memset(&d, 0, sizeof(d));
    d.L = h->max_angular; d.C = h->n_channels; d.ns = h->n_species; d.legacy = h->legacy; d.layernorm = h->layernorm;
    d.H = h->num_neurons_per_layer; d.NH = h->num_hidden_layers; d.rc = h->cutoff; d.width = h->cutoff_width;
    d.NLM = (d.L + 1) * (d.L + 1);
    int f = 0, co = 0, fo = 0, items = 0, pfo = 0;
    for (int l = 0; l <= d.L; l++) {
        const int n = h->n_per_l[l];
        if (n < 0 || n > 64) { delete sm; set_error("bad n_per_l"); return PET_ERR_ARGUMENT; }
        d.n_per_l[l] = n; d.rad_off[l] = f; d.coef_off[l] = co; d.feat_off[l] = fo;
        if (n * d.C > d.ncmax) d.ncmax = n * d.C;
        d.pfeat_off[l] = pfo;
        f += n; co += (2 * l + 1) * n * d.C; fo += (n * d.C) * (n * d.C); items += (2 * l + 1) * n;
        pfo += (n * d.C) * (n * d.C + 1) / 2;
    }
    d.coef_off[d.L + 1] = co; d.feat_off[d.L + 1] = fo; d.pfeat_off[d.L + 1] = pfo; d.Sp = pfo;
    d.F = f; d.NCOEF = co; d.S = fo; d.ITEMS = items;
    m.n_sets = h->legacy ? h->n_species : 1;
    if (d.F > 255 || d.NLM > 255 || d.NCOEF > 256 * MAXK || d.NCOEF >= 65536) {
        delete sm;
        set_error("SOAP basis too large for the compiled limits");
        return PET_ERR_UNSUPPORTED;
    }
    *out = sm;
    return PET_OK;
}

void soap_model_destroy(soap_model_t* sm) {
    if (!sm) return;
    for (void* p : sm->m.owned) (void)hipFree(p);
    delete sm;
}

int64_t soap_model_feature_size(const soap_model_t* sm) { return sm ? sm->m.d.S : -1; }

int soap_model_set_radial_table(soap_model_t* sm, const float* d_table, int32_t n_grid, void* stream) {
    PET_REQUIRE(sm && d_table && n_grid >= 4, PET_ERR_ARGUMENT, "bad argument");
    SoapModel& m = sm->m;
    const size_t bytes = (size_t)n_grid * m.d.F * 4 * sizeof(float);
    int rc = salloc(m, (void**)&m.table, bytes);
    if (rc) return rc;
    PET_HIP_CHECK(hipMemcpyAsync(m.table, d_table, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    m.d.n_grid = n_grid;
    m.d.inv_h = (float)(n_grid - 1) / m.d.rc;
    m.curv = nullptr;  // the curvature slopes belong to the table they were formed from
    m.finalized = false;
    return PET_OK;
}

int soap_model_set_radial_curvature(soap_model_t* sm, const float* d_table, int32_t n_grid, void* stream) {
    PET_REQUIRE(sm && d_table, PET_ERR_ARGUMENT, "bad argument");
    SoapModel& m = sm->m;
    PET_REQUIRE(m.table != nullptr && n_grid == m.d.n_grid, PET_ERR_ARGUMENT,
                "the curvature table follows soap_model_set_radial_table, on the same grid");
    const size_t bytes = (size_t)n_grid * m.d.F * 2 * sizeof(float);
    m.curv = nullptr;
    int rc = salloc(m, (void**)&m.curv, bytes);
    if (rc) return rc;
    PET_HIP_CHECK(hipMemcpyAsync(m.curv, d_table, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PET_OK;
}

int soap_model_set_param(soap_model_t* sm, const char* key, const float* d_data, int64_t numel, void* stream) {
    PET_REQUIRE(sm && key && d_data && numel > 0, PET_ERR_ARGUMENT, "bad argument");
    SoapModel& m = sm->m;
    float* p;
    auto it = m.raw.find(key);
    if (it != m.raw.end() && it->second.second == numel) {
        p = it->second.first;
    } else {
        int rc = salloc(m, (void**)&p, numel * sizeof(float));
        if (rc) return rc;
        m.raw[key] = {p, numel};
    }
    PET_HIP_CHECK(hipMemcpyAsync(p, d_data, numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    m.finalized = false;
    return PET_OK;
}

int soap_model_finalize(soap_model_t* sm, void* stream) {
    PET_REQUIRE(sm, PET_ERR_ARGUMENT, "null model");
    return soap_finalize(sm->m, (hipStream_t)stream);
}

int64_t soap_workspace_bytes(const soap_model_t* sm, int64_t n_nodes, int64_t n_edges) {
    if (!sm) return -1;
    SoapWs w;
    carve_soap(sm->m.d, n_nodes, n_edges, nullptr, w);
    return (int64_t)w.bytes;
}

int soap_forward(const soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                 float* d_atomic, float* d_features, void* stream) {
    PET_REQUIRE(sm && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(sm->m.finalized, PET_ERR_ARGUMENT, "soap_model_finalize has not been called");
    if (pg->g.n_nodes == 0) return PET_OK;   // an empty system: nothing to write (zero-sized buffers may be null)
    PET_REQUIRE(d_workspace && d_atomic, PET_ERR_ARGUMENT, "null argument");
    return soap_fwd(sm->m, pg->g, d_workspace, workspace_bytes, d_atomic, d_features, (hipStream_t)stream);
}

int soap_backward(const soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                  const float* d_grad_atomic, float* d_grad_positions, float* d_grad_cells, void* stream) {
    PET_REQUIRE(sm && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(sm->m.finalized, PET_ERR_ARGUMENT, "soap_model_finalize has not been called");
    if (pg->g.n_nodes == 0) return PET_OK;
    PET_REQUIRE(d_workspace && d_grad_atomic && d_grad_positions, PET_ERR_ARGUMENT, "null argument");
    return soap_bwd(sm->m, pg->g, d_workspace, workspace_bytes, d_grad_atomic, d_grad_positions, d_grad_cells,
                    (hipStream_t)stream);
}

int soap_model_zero_grad(soap_model_t* sm, void* stream) {
    PET_REQUIRE(sm, PET_ERR_ARGUMENT, "null model");
    return soap_zero_grad(sm->m, (hipStream_t)stream);
}

int64_t soap_train_workspace_bytes(const soap_model_t* sm, int64_t n_nodes, int64_t n_edges) {
    if (!sm) return -1;
    return soap_train_ws_bytes(sm->m, n_nodes, n_edges);
}

int soap_train_gradients_cell(soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                              void* d_train_workspace, int64_t train_workspace_bytes, const float* d_grad_atomic,
                              const float* d_u, const float* d_u_cell, float* d_tangent_atomic, void* stream) {
    PET_REQUIRE(sm && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(sm->m.finalized, PET_ERR_ARGUMENT, "soap_model_finalize has not been called");
    if (pg->g.n_nodes == 0) return PET_OK;
    PET_REQUIRE(d_workspace && d_train_workspace && d_grad_atomic && d_tangent_atomic, PET_ERR_ARGUMENT, "null argument");
    return soap_train_grads(sm->m, pg->g, d_workspace, workspace_bytes, d_train_workspace, train_workspace_bytes,
                            d_grad_atomic, d_u, d_u_cell, d_tangent_atomic, (hipStream_t)stream);
}

int soap_train_gradients(soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                         void* d_train_workspace, int64_t train_workspace_bytes, const float* d_grad_atomic,
                         const float* d_u, float* d_tangent_atomic, void* stream) {
    return soap_train_gradients_cell(sm, pg, d_workspace, workspace_bytes, d_train_workspace, train_workspace_bytes,
                                     d_grad_atomic, d_u, nullptr, d_tangent_atomic, stream);
}

int64_t soap_hvp_workspace_bytes(const soap_model_t* sm, int64_t n_nodes, int64_t n_edges) {
    if (!sm) return -1;
    return soap_hvp_ws_bytes(sm->m, n_nodes, n_edges);
}

int soap_hessian_vector(const soap_model_t* sm, const pet_graph_t* pg, void* d_workspace, int64_t workspace_bytes,
                        void* d_hvp_workspace, int64_t hvp_workspace_bytes, const float* d_u, const float* d_u_cell,
                        float* d_hvp_positions, float* d_hvp_cells, float* d_tangent_atomic, void* stream) {
    PET_REQUIRE(sm && pg, PET_ERR_ARGUMENT, "null argument");
    PET_REQUIRE(sm->m.finalized, PET_ERR_ARGUMENT, "soap_model_finalize has not been called");
    if (pg->g.n_nodes == 0) return PET_OK;
    PET_REQUIRE(d_workspace && d_hvp_workspace && d_u && d_hvp_positions, PET_ERR_ARGUMENT, "null argument");
    return soap_hvp(sm->m, pg->g, d_workspace, workspace_bytes, d_hvp_workspace, hvp_workspace_bytes, d_u, d_u_cell,
                    d_hvp_positions, d_hvp_cells, d_tangent_atomic, (hipStream_t)stream);
}

static int soap_copy_out(const std::map<std::string, std::pair<float*, int64_t>>& table, const char* key, float* d_out,
                         int64_t numel, void* stream) {
    auto it = table.find(key);
    PET_REQUIRE(it != table.end(), PET_ERR_ARGUMENT, std::string("no entry '") + key + "'");
    PET_REQUIRE(it->second.second == numel, PET_ERR_ARGUMENT, std::string("'") + key + "' has another size");
    PET_HIP_CHECK(hipMemcpyAsync(d_out, it->second.first, numel * sizeof(float), hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
    return PET_OK;
}

int soap_model_get_grad(const soap_model_t* sm, const char* key, float* d_out, int64_t numel, void* stream) {
    PET_REQUIRE(sm && key && d_out, PET_ERR_ARGUMENT, "null argument");
    return soap_copy_out(sm->m.grad, key, d_out, numel, stream);
}

int soap_model_get_param(const soap_model_t* sm, const char* key, float* d_out, int64_t numel, void* stream) {
    PET_REQUIRE(sm && key && d_out, PET_ERR_ARGUMENT, "null argument");
    return soap_copy_out(sm->m.raw, key, d_out, numel, stream);
}

int soap_adam_step(soap_model_t* sm, float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
    PET_REQUIRE(sm, PET_ERR_ARGUMENT, "null model");
    return soap_adam(sm->m, lr, beta1, beta2, eps, step, (hipStream_t)stream);
}


}  // extern "C"
