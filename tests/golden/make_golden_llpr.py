"""Fixture of the LLPR tests -> ``pet_llpr.npz``.

* Per-atom last-layer features of every readout layer, as the reference PET assembles them for
  ``mtt::aux::energy_last_layer_features`` (pet/model.py:788-875: node part, then the cutoff-weighted sum of the edge part, per
  readout layer), from the reference ``PETBackend`` imported as ``make_golden`` does, in fp64:
  default hypers on the ``batch_two_systems`` and ``pet_default_box64`` inputs, the residual featuriser on the
  ``pet_variant_residual_box64`` inputs (synthetic parameters, seed 0, one energy property).
* The three calibration multipliers of the reference's ``llpr/calibration.py`` (loaded by path; it imports only ``math``,
  ``typing`` and ``torch``, plus scipy for the CRPS root) on fixed seeded residual / sigma arrays.

    python tests/golden/make_golden_llpr.py        (needs the reference checkout next to make_golden's)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402


def _llf_case(PETBackend, hyp, g):
    be, _ = mg._reference_backend(PETBackend, hyp, torch.float64)
    be = be.eval()
    t = lambda k: torch.tensor(g[k])  # noqa: E731
    pos, cells = t("in_positions").double(), t("in_cells").double()
    sysidx = t("in_system_indices").long()
    batch = be.preprocess(pos, t("in_centers").long(), t("in_neighbors").long(), t("in_species").long(), cells,
                          t("in_cell_shifts").long(), sysidx, 1.0)
    with torch.no_grad():
        nf, ef = be.calculate_features(batch)
        pred, node_ll, edge_ll = be.predict(nf, ef, batch, cells, sysidx, ["energy"])
    cf = batch["cutoff_factors"][:, :, None]
    parts = []
    for a, b in zip(node_ll["energy"], edge_ll["energy"]):
        parts += [a, (b * cf).sum(1)]
    return torch.cat(parts, dim=1).numpy(), pred["energy"][0].numpy()


def _calibration():
    path = os.path.join(mg.REF, "llpr", "calibration.py")
    spec = importlib.util.spec_from_file_location("reference_llpr_calibration", path)
    cal = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cal)
    rng = np.random.default_rng(7)
    sigma = rng.uniform(0.5, 2.0, size=(400, 2))
    residuals = rng.normal(size=(400, 2)) * sigma * np.array([1.7, 0.6])
    out = {"cal_residuals": residuals, "cal_sigma": sigma}
    for method in ("squared_residuals", "absolute_residuals", "crps"):
        c = cal.GaussianCRPSCalibrator() if method == "crps" else cal.RatioCalibrator(method=method)
        for lo in range(0, 400, 100):  # four batches, as calibrate() feeds them
            c.update(uncertainty_name="u", residuals=torch.tensor(residuals[lo:lo + 100]),
                     uncertainties=torch.tensor(sigma[lo:lo + 100]))
        out[f"cal_{method}"] = c.finalize()["u"].numpy()
        print(method, out[f"cal_{method}"])
    return out


def main():
    from oracle import pet as opet

    PETBackend = mg.import_reference_backend()
    torch.set_num_threads(8)
    store = {}
    for tag, fname, delta in (("two_systems", "batch_two_systems.npz", {}),
                              ("box64", "pet_default_box64.npz", {}),
                              ("residual_box64", "pet_variant_residual_box64.npz", {"featurizer_type": "residual"})):
        g = dict(np.load(os.path.join(HERE, fname)))
        hyp = dict(opet.DEFAULT_HYPERS, **delta)
        llf, atomic = _llf_case(PETBackend, hyp, g)
        store[f"llf_{tag}"] = llf.astype(np.float32)
        store[f"atomic_{tag}"] = atomic
        print(tag, llf.shape, float(np.abs(llf).max()))
    store.update(_calibration())
    np.savez_compressed(os.path.join(HERE, "pet_llpr.npz"), **store)


if __name__ == "__main__":
    main()
