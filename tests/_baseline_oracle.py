"""fp64 numpy restatement of the reference's composition model and scaler, written from the reference's lines alone (not from
metatrain_amd/baseline.py): what the tests of the baseline / scale path compare against. The reference's own classes are built
on metatensor TensorMaps; here a block is its values array ``[samples, components..., properties]``.

    composition/_base_composition.py   229-322 accumulate, 324-367 fixed weights, 369-467 fit, 713-742 _solve_linear_system
    scaler/_base_scaler.py             287-370 _compute_N_and_Y2, 372-429 accumulate, 431-491 accumulate_per_property,
                                       493-538 fit, 540-617 fit_per_property, 619-751 forward (remove=True)
    scaler/trainer.py                  174-186 additive models removed, average_by_num_atoms, then accumulate
    utils/additive/remove.py           123-143 target - additive contribution
    utils/per_atom.py                  30-37 per-structure values / n_atoms unless named in per_structure_targets
"""
import numpy as np


def type_indices(atomic_types, species):
    """Position of every atom's species in ``atomic_types``; unexpected types raise (_base_composition.py:247-254)."""
    atomic_types = np.asarray(atomic_types)
    species = np.asarray(species)
    if not np.all(np.isin(species, atomic_types)):
        raise ValueError(f"system contains unexpected atom types. Expected atomic types: {atomic_types}, found: {np.unique(species)}")
    return np.argmax(species[:, None] == atomic_types[None, :], axis=1)


def one_hot(atomic_types, species):
    """_compute_X_per_atom: ``[N, T]``."""
    return (np.asarray(species)[:, None] == np.asarray(atomic_types)[None, :]).astype(np.int64)


def counts_per_structure(atomic_types, species, system_indices, n_systems):
    """_compute_X_per_structure: ``[S, T]`` counts, and the atoms per system."""
    type_indices(atomic_types, species)
    X = np.zeros((n_systems, len(atomic_types)), dtype=np.int64)
    np.add.at(X, np.asarray(system_indices), one_hot(atomic_types, species))
    return X, X.sum(axis=1)


def composition_accumulate(per_atom, X, Y):
    """One batch's (XTX, XTY), :306-322. ``X``: counts [S, T] or one-hot [N, T]; ``Y [rows, ...]``."""
    Y = np.asarray(Y, dtype=np.float64)
    XTX = X.T @ X
    if not per_atom:
        XTY = np.tensordot(X.astype(np.float64), Y, axes=([0], [0]))
    else:
        XTY = np.zeros((X.shape[1],) + Y.shape[1:])
        np.add.at(XTY, np.argmax(X, axis=1), Y)  # scatter_add: a NaN stays inside its type
    return XTX, XTY


def solve_linear_system(XTX, XTY):
    """:713-742."""
    XTX = np.asarray(XTX, dtype=np.float64)
    regularizer = 1e-14 * float(np.mean(np.abs(np.diag(XTX))))
    flat = np.asarray(XTY, dtype=np.float64).reshape(XTY.shape[0], -1)
    return np.linalg.solve(XTX + regularizer * np.eye(XTX.shape[1]), flat).reshape(XTY.shape)


def sanitize_fixed_weights(atomic_types, weights, target_name="target"):
    """:352-365."""
    atomic_types = [int(z) for z in atomic_types]
    if isinstance(weights, float):
        return {z: float(weights) for z in atomic_types}
    missing = set(atomic_types) - set(weights)
    if missing:
        raise ValueError(f"Fixed weights for target '{target_name}' are missing the following atomic types: {missing}")
    return weights


def composition_fit(atomic_types, per_atom, XTX, XTY, fixed=None):
    """Weights ``[T, ...]`` of one block, :392-453."""
    XTX = np.asarray(XTX, dtype=np.float64)
    XTY = np.asarray(XTY, dtype=np.float64)
    if fixed is not None:
        fixed = sanitize_fixed_weights(atomic_types, fixed)
        return np.stack([np.full(XTY.shape[1:], fixed[int(z)]) for z in atomic_types])
    if np.all(XTX == 0):
        return np.zeros_like(XTY)
    if not per_atom:
        return solve_linear_system(XTX, XTY)
    counts = np.diag(XTX).reshape((-1,) + (1,) * (XTY.ndim - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts == 0, np.zeros_like(XTY), XTY / counts)


def residual(per_atom, Y, weights, X, n_atoms=None, divide=True):
    """The target the scaler sees: composition removed (remove.py:123-143, the composition's prediction is X @ w), then
    per-structure values divided by the atom count (per_atom.py:30-37). ``weights`` None: no baseline."""
    r = np.array(Y, dtype=np.float64)
    if weights is not None:
        r = r - np.tensordot(X.astype(np.float64), np.asarray(weights, dtype=np.float64), axes=([1], [0]))
    if not per_atom and divide:
        r = r / np.asarray(n_atoms, dtype=np.float64).reshape((-1,) + (1,) * (r.ndim - 1))
    return r


def n_and_y2(per_atom, r, per_property, type_index=None, n_types=None):
    """_compute_N_and_Y2 of one block (:297-368): rows 1 (per structure) or T (per atom); columns 1 or n_properties."""
    r = np.array(r, dtype=np.float64)
    mask = ~np.isnan(r)
    r[np.isnan(r)] = 0.0
    axes = tuple(range(0, r.ndim - 1)) if per_property else tuple(range(0, r.ndim))
    if not per_atom:
        return mask.sum(axis=axes).reshape(1, -1), np.sum((r * mask) ** 2, axis=axes).reshape(1, -1)
    N, Y2 = [], []
    for t in range(n_types):
        sel = np.asarray(type_index) == t
        N.append(mask[sel].sum(axis=axes).reshape(-1))
        Y2.append(np.sum((r[sel] * mask[sel]) ** 2, axis=axes).reshape(-1))
    return np.stack(N), np.stack(Y2)


def scaler_fit(N, Y2):
    """:521-538: sqrt(Y2 / N), NaN -> 1."""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (np.asarray(Y2, dtype=np.float64) / np.asarray(N)) ** 0.5
    return np.where(np.isnan(s), 1.0, s)


def full_scales(per_target, per_property):
    """:599-607."""
    s = np.asarray(per_target, dtype=np.float64) * np.asarray(per_property, dtype=np.float64)
    return np.where(np.isnan(s), 1.0, s)


def remove_scale(per_atom, r, scale, type_index=None):
    """forward(remove=True, use_per_target_scales=True), :712-751 and the per-atom branch: values / scale (of the atom's type)."""
    r = np.asarray(r, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if not per_atom:
        return r / scale[0]
    return r / scale[np.asarray(type_index)].reshape((-1,) + (1,) * (r.ndim - 1))
