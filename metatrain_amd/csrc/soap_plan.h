// Which kernel serves every stage of the SOAP-BPNN pass, decided once per call in one place: soap_plan_forward /
// soap_plan_backward / soap_plan_train (soap.hip) are the only code of that pass that reads switches(), compares a SoapDims
// field with a limit, or asks whether a weight form exists (m.NT, wall_fwd_set, wallp_fwd_set, m.enc). The drivers (soap.hip
// soap_fwd / soap_bwd, soap_train.hip soap_train_grads) switch on the plan; the launchers (soap_expand.hip, soap_ps.hip,
// soap_tail.hip) compute the LDS size and launch. DESIGN.md 4.6 has the table (stage x condition -> kernel, forward and adjoint).
#pragma once
#include <stdint.h>

namespace pet {

// A forward plan names the forward kernels, an adjoint plan their adjoints. The forward's plan stays with its workspace
// (FwdRecord, common.h): the adjoint and the training pass follow the layout it stored and the tables it filled, or refuse.
struct SoapPlan {
    // spherical expansion: one workgroup per atom, any number of species channels (k_soap_expand; adjoint k_soap_expand_bwd),
    // or one wave per atom with four channels (k_soap_expand_w<6 | MAXL>; adjoint one lane per pair, k_soap_expand_bwd_p)
    enum class Expand : uint8_t { PerAtom, Wave };
    // power spectrum: one workgroup per atom (k_soap_ps; adjoint k_soap_ps_bwd), one wave per atom on a feature table
    // (k_soap_ps_w; adjoint k_soap_ps_bwd_s on a staged dF row), on the matrix core in the full layout (k_soap_ps_m<false>;
    // adjoint k_soap_ps_bwd_m<false>) or storing the upper triangles only (k_soap_ps_m<true>; adjoint k_soap_ps_bwd_m<true>)
    enum class PowerSpectrum : uint8_t { PerAtom, Lut, Mfma, MfmaPacked };
    // LayerNorm + MLP tail: one workgroup per atom (k_soap_tail; adjoint k_soap_tail_bwd), 64 atoms against the first Linear
    // of all networks stacked (k_soap_tail_fwd_mfma<NT>; adjoint k_soap_tail_bwd_mfma<NT>), or 64 atoms of ONE network
    // against that network's weight after bucketing the atoms (k_sp_*, k_soap_tail_fwd_set; adjoint k_soap_tail_bwd_set,
    // which reads the forward's buckets)
    enum class Tail : uint8_t { PerAtom, Stacked, Sorted };

    Expand expand = Expand::PerAtom;
    PowerSpectrum ps = PowerSpectrum::PerAtom;
    Tail tail = Tail::PerAtom;
    bool packed = false;     // the feature buffer holds the packed power spectrum (forward: it stores it; adjoint: it reads it)
    bool bucketed = false;   // forward only: it filled perm / info of the workspace (the atoms bucketed by network)
    bool wide_l = false;     // max_angular > 6: the MAXL instantiation of the wave expansion and its adjoint
    bool deep_tail = false;  // num_hidden_layers > 2: the continuation kernels k_soap_tail_extra_fwd / _bwd run beside the tail
    int lds_rows = 0;        // adjoint only: LDS floats in which k_soap_expand_bwd_p stages its centres' rows (16 * 1024 or 0)
};

// the training pass's two choices
struct SoapTrainPlan {
    bool rebuild_full = false;  // the forward stored the packed layout: the full one is rebuilt first (k_soap_ps_m<false>)
    bool wide_table = false;    // more networks than the forward's bucket table holds: the 16-network table
};

struct SoapModel;
struct Graph;
struct FwdRecord;
SoapPlan soap_plan_forward(const SoapModel& m, const Graph& g, bool want_features);
// rec: what the forward left in the workspace (required). Refuses, before anything is launched, an adjoint that the switches
// no longer allow to follow that forward: a packed feature buffer in front of a full-layout adjoint, and a sorted tail adjoint
// behind a forward that did not bucket the atoms.
int soap_plan_backward(const SoapModel& m, const Graph& g, const FwdRecord* rec, SoapPlan& plan);
int soap_plan_train(const SoapModel& m, const FwdRecord* rec, SoapTrainPlan& plan);

}  // namespace pet
