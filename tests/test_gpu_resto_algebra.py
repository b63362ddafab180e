"""Device tests of the small dense routines of the restoration phase (mpc-verde_amd/csrc/resto.h):
chol_small / chol_solve_small, resto_chol and resto_transform, for NX = 3, 4 and 6, through the
harness tests/hip/resto_check.hip, which calls the very functions recover() calls, one thread per case.

Reference: the definitions S = D^-1 + P, Pt = D^-1 - D^-1 S^-1 D^-1, pt = D^-1 S^-1 p, x = S^-1 b in
exact rational arithmetic, rounded once (tests/helpers/resto_ref.py; tests/test_resto_cpu.py checks
that side).  Classes, 300 draws each per NX at fixed seeds, D log-uniform and P = Q diag(ev) Q^T:
"P huge" (D in 1e-6..1e2, ev in 1e4..1e12), "balanced" (both in 1e-2..1e2), "D^-1 huge" (D in
1e-9..1e-5, ev in 1e-2..1e2), and the regular edges (P = 0 off the diagonal, P exactly singular).
Broken cases: the NX-th pivot of S exactly 0 and exactly -2^-40 (ok false, every output finite:
chol_small goes on with sqrt(fmax(d, 1e-300))), a NaN in P (ok false).

Tolerance, as tests/test_gpu_scan.py: per class, NX and quantity, 64 times the worst error of the
float64 restatement of the device algorithm against the exact reference over that class, measured in
the test; each quantity normalised by max(1e-300, max |reference|) of its case; the factor pays for
the device's fma contraction.  The L factor is compared through L L^T against S.  D^-1 is a single
IEEE division on both sides, so its tolerance is 0.

Measured on one MI355X (device's worst error over NX = 3 / 4 / 6, and its largest ratio to the
restatement's worst of the same class and NX):

class       Pt                           pt               x = S^-1 b       L L^T
P huge      7.3e-10 / 4.2e-10 / 1.9e-10  1.2e-9  (1.35)   1.7e-9  (1.39)   2.4e-16 (1.01)
            (1.61)
balanced    4.8e-13 / 1.7e-13 / 7.6e-14  3.8e-14 (1.34)   4.8e-14 (1.12)   4.5e-16 (1.00)
            (1.00)
D^-1 huge   2.1e-6 / 8.8e-7 / 3.7e-7     5.4e-16 (1.00)   6.9e-16 (1.00)   5.6e-16 (1.00)
            (1.00)
edges       5.5e-13 (1.00)               5.1e-15 (0.81)   2.3e-14 (2.84)   3.4e-16 (1.00)

D^-1 is bit for bit the reference's.  The largest ratio anywhere is 2.84 (edges, NX = 6, x), 22
times under the tolerance; on the class the comment of resto_transform did not mention, "D^-1
huge", device and restatement lose the same 6 to 7 digits of Pt.  Every broken case reports false
with finite outputs, and its factor equals the restatement's bit for bit.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resto_ref as rr  # noqa: E402

LIB = os.path.join(ROOT, "tests", "hip", "libresto_check.so")
FACTOR = 64.0


def device(nx, D, P, p):
    """The three kernels on the cases (D (c, nx), P (c, nx, nx) symmetric, p (c, nx)): dict of L0, x
    (chol_small + chol_solve_small on the float64 S = P + 1 / D), Di, L (resto_chol), Pt, pt
    (resto_transform) and the three verdicts."""
    import torch

    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (make -C tests/hip)")
    lib = ctypes.CDLL(LIB)
    lib.resto_check.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    c, npk = len(D), nx * (nx + 1) // 2
    with np.errstate(all="ignore"):
        S = P + (1.0 / D)[:, :, None] * np.eye(nx)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
    dD, dS, dP, dp = up(D), up(S), up(rr.pack(P)), up(p)
    assert dS.numel() == c * nx * nx and dP.numel() == c * npk and dD.numel() == dp.numel() == c * nx
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    outs, oks = [], []
    for which, (d_, m_, v_) in enumerate(((None, dS, dp), (dD, dP, None), (dD, dP, dp))):
        n_out = lib.resto_check_out_size(which, nx)
        assert n_out == (nx * nx + nx, nx + nx * nx, npk + nx)[which]
        out = torch.full((c, n_out), np.nan, dtype=torch.float64, device="cuda")
        ok = torch.full((c,), -1, dtype=torch.int32, device="cuda")
        rc = lib.resto_check(which, nx, c, ptr(d_) if d_ is not None else None, ptr(m_),
                             ptr(v_) if v_ is not None else None, ptr(out), ptr(ok))
        assert rc == 0, (which, nx, rc)
        outs.append(out.cpu().numpy())
        oks.append(ok.cpu().numpy())
        assert set(np.unique(oks[-1])) <= {0, 1}
    o0, o1, o2 = outs
    return dict(L0=o0[:, :nx * nx].reshape(c, nx, nx), x=o0[:, nx * nx:], Di=o1[:, :nx],
                L=o1[:, nx:].reshape(c, nx, nx), Pt=rr.unpack(o2[:, :npk], nx), pt=o2[:, npk:],
                ok=[o.astype(bool) for o in oks])


@pytest.mark.parametrize("nx", rr.NXS)
@pytest.mark.parametrize("cls", list(rr.CLASSES) + ["edges"])
def test_device_algebra_against_the_exact_reference(cls, nx):
    (D, P, p), ex, rs, worst = rr.class_case(cls, nx)
    got = device(nx, D, P, p)
    assert all(np.all(ok) for ok in got["ok"])
    # the factors are lower triangular with a positive diagonal
    for L in (got["L0"], got["L"]):
        assert np.all(np.triu(L, 1) == 0.0) and np.all(np.einsum("cii->ci", L) > 0.0)
    err = rr.errors(got, ex)
    for k, e in err.items():
        ratio = e.max() / worst[k] if worst[k] > 0 else (0.0 if e.max() == 0 else np.inf)
        print(f"{cls} NX={nx} {k}: device worst {e.max():.2e}, restatement worst {worst[k]:.2e}, ratio {ratio:.2f}, "
              f"tolerance {FACTOR * worst[k]:.2e}")
    for k, e in err.items():
        assert e.max() <= FACTOR * worst[k], (cls, nx, k, int(np.argmax(e)), e.max(), worst[k])


@pytest.mark.parametrize("nx", rr.NXS)
def test_device_algebra_on_broken_cases(nx):
    """Pivot exactly 0, exactly -2^-40, a NaN in P: every verdict false.  With a finite S the
    factorisation goes on: every output finite, the last pivot's entry sqrt(1e-300), and -- the
    construction being exact in any order of operations -- the factor equal to the restatement's."""
    D, P, p, kind = rr.broken_cases(nx)
    got = device(nx, D, P, p)
    for ok in got["ok"]:
        assert not ok.any(), (nx, np.flatnonzero(ok))
    fin = kind < 2
    for k in ("L0", "x", "Di", "L", "Pt", "pt"):
        assert np.all(np.isfinite(got[k][fin])), (nx, k)
    _, _, L, _ = rr.resto_chol(D, P)
    for k in ("L0", "L"):
        assert np.all(got[k][fin, nx - 1, nx - 1] == 1e-150)
        assert np.array_equal(got[k][fin], L[fin]), (nx, k)
