"""fp64 numpy oracle of the real Wigner-D matrices, sharing no code (and no method) with ``csrc/wigner.h``.

Convention: ``Y_l(Q u) = D^l(Q) Y_l(u)`` with the orthonormal real spherical harmonics written out in
:func:`real_harmonics` -- order ``m = -l..l``, NO Condon-Shortley phase, ``Y_1 = sqrt(3/4pi) (y, z, x)`` -- so that with
positions ``x' = Q x`` a block transforms as ``t'[m] = sum_m' D^l[m,m'] t[m']``.

Method: ``D^l(Q)`` is the least-squares solution of ``Y_l(u_k) D^T = Y_l(Q u_k)`` over 400 fixed random unit vectors, ``Q``
first projected to the nearest rotation (``U V^T`` of its SVD); the two sides are evaluated in numpy's extended precision and
the fp64 solve is refined twice on the extended residual. The harmonics are polynomials evaluated by the standard
three-term recurrence in ``z`` times ``Re / Im (x + i y)^m``; nothing here builds ``D`` from ``D^(l-1)``.
"""
import math

import numpy as np

L_MAX = 8
N_SAMPLES = 400
P_YZX = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])  # (x, y, z) -> (y, z, x)


def offset(l: int) -> int:
    """Where block ``l`` starts in a table ``[W]``."""
    return l * (4 * l * l - 1) // 3


def width(l_max: int) -> int:
    return (l_max + 1) * (2 * l_max + 1) * (2 * l_max + 3) // 3


def real_harmonics(l: int, u: np.ndarray) -> np.ndarray:
    """``Y_l`` at the vectors ``u [K,3]`` as ``[K, 2l+1]``: homogeneous polynomials of degree ``l`` for unit vectors (the
    radial factor is NOT divided out: callers pass unit vectors, or mean the solid harmonic ``|u|^l Y_l(u / |u|)`` only when
    they normalise themselves)."""
    u = np.asarray(u)
    u = u if u.dtype == np.longdouble else u.astype(np.float64)  # (the fit below evaluates in extended precision)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    out = np.empty((u.shape[0], 2 * l + 1), dtype=u.dtype)
    xy = (x + 1j * y)
    for m in range(l + 1):
        # q_l^m(z) = P_l^m(z) / (1 - z^2)^(m/2) without the Condon-Shortley phase: q_m^m = (2m-1)!!
        q_prev, q = np.zeros_like(z), np.full_like(z, float(np.prod(np.arange(2 * m - 1, 0, -2))) if m else 1.0)
        for k in range(m + 1, l + 1):
            q_prev, q = q, ((2 * k - 1) * z * q - (k + m - 1) * q_prev) / (k - m)
        norm = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
        e = xy ** m
        if m == 0:
            out[:, l] = norm * q
        else:
            out[:, l + m] = math.sqrt(2.0) * norm * q * e.real
            out[:, l - m] = math.sqrt(2.0) * norm * q * e.imag
    return out


def solid_harmonics(l: int, r: np.ndarray) -> np.ndarray:
    """``|r|^l Y_l(r / |r|)`` for any vectors ``r [K,3]`` (zero vectors give zero for ``l > 0``): equivariant in ``r``."""
    r = np.asarray(r, dtype=np.float64)
    norm = np.linalg.norm(r, axis=1)
    safe = np.where(norm > 0, norm, 1.0)
    y = real_harmonics(l, r / safe[:, None]) * (norm ** l)[:, None]
    if l > 0:
        y[norm == 0] = 0.0
    return y


def _samples() -> np.ndarray:
    v = np.random.default_rng(20240).standard_normal((N_SAMPLES, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


SAMPLES = _samples()


def nearest_rotation(q: np.ndarray) -> np.ndarray:
    """The orthogonal polar factor ``U V^T`` of ``q`` (its determinant must be positive)."""
    u, _, vt = np.linalg.svd(np.asarray(q, dtype=np.float64))
    r = u @ vt
    assert np.linalg.det(r) > 0, "not a proper matrix"
    return r


def wigner_d(l: int, q: np.ndarray) -> np.ndarray:
    """``D^l`` ``[2l+1, 2l+1]`` of the rotation nearest to ``q``."""
    r = nearest_rotation(q)
    # both sides in extended precision, the solve in fp64 with two steps of iterative refinement on the extended residual: the
    # solution is then the least-squares one to about an fp64 rounding per entry, whatever LAPACK's own error
    wide = SAMPLES.astype(np.longdouble)
    a = real_harmonics(l, wide)
    b = real_harmonics(l, wide @ r.T.astype(np.longdouble))
    a64 = a.astype(np.float64)
    dt = np.zeros((2 * l + 1, 2 * l + 1), dtype=np.longdouble)
    for _ in range(3):
        step, *_ = np.linalg.lstsq(a64, (b - a @ dt).astype(np.float64), rcond=None)
        dt = dt + step
    return dt.T.astype(np.float64)


def condition_number(l: int) -> float:
    return float(np.linalg.cond(real_harmonics(l, SAMPLES)))


def table(o: np.ndarray, l_max: int):
    """``(table [W(l_max)], det)`` of one matrix of O(3): ``det`` the sign of its determinant, the table that of the proper
    part ``det * o``, blocks row-major one after the other."""
    o = np.asarray(o, dtype=np.float64)
    det = -1.0 if np.linalg.det(o) < 0 else 1.0
    return np.concatenate([wigner_d(l, det * o).reshape(-1) for l in range(l_max + 1)]), det


def symmetric_traceless_to_l2(t: np.ndarray) -> np.ndarray:
    """The five ``l = 2`` components of a symmetric traceless ``T [3,3]`` (an orthonormal map up to one common factor)."""
    s2, s6 = math.sqrt(2.0), math.sqrt(6.0)
    return np.array([s2 * t[0, 1], s2 * t[1, 2], (2 * t[2, 2] - t[0, 0] - t[1, 1]) / s6, s2 * t[0, 2], (t[0, 0] - t[1, 1]) / s2])
