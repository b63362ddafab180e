"""CPU: the algebra of the sensitivities to x0 (tests/helpers/sens_ref.py) and the C ABI's two entry points.

The sensitivity kernel (csrc/sens.h) runs one Riccati sweep on H + Sigma and a prefix product of the
closed-loop maps.  Here the recursion is restated in NumPy and checked against itself in long double
(the yardstick E_ref of the GPU tests) and against the active-set sensitivities it approaches as the
barrier term of the active variables grows."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sens_ref as sr  # noqa: E402

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_sens_x0", "mpcx_sens_x0_dev")


def test_float64_recursion_against_long_double():
    """The float64 recursion against the long-double one on random LQ stages of the shapes
    LQ_SHAPES, Sigma in {1, 1e4, 1e9} on a random 40 % of the inputs.  Its worst relative error is
    the yardstick E_ref (measured: 6.1e-16).  Bound: a sweep is at most 50 stages of a few products
    of matrices of order <= 7, each entry a sum of <= 7 rounded terms, backward and forward; errors
    add at worst linearly, 2 x 50 x 7 x 7 roundings ~ 2^13 eps, with the stages' conditioning (H's
    eigenvalues in [0.5, ~5], |A| <= 0.95) inside another factor 2^7."""
    e = sr.e_ref()
    print(f"E_ref = {e:.3e}")
    assert 0.0 < e <= 2.0 ** 20 * np.finfo(np.float64).eps


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES)))
def test_stage_zero_rows(seed, shape):
    """dX_0/dx0 is the identity exactly and dU_0/dx0 is K_0 = -Huu'^-1 (Hux_0 + B_0^T P_1 A_0): not zero."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    dw, ok = sr.riccati_sens(A, B, H, np.zeros((N + 1, nx + nu)))
    assert ok
    assert np.array_equal(dw[:nx], np.eye(nx))
    assert np.min(np.max(np.abs(dw[sr.iu_w(nx, nu, 0)]), axis=1)) > 1e-3
    # against the dense KKT solve without a barrier term (nothing active): the same linear system
    ref = sr.active_set_sens(A, B, H, np.zeros(dw.shape[0], bool))
    assert sr.rel_err(dw, ref) <= 1e-11  # (the CPU check of the algebra: 1e-11 or better for Sigma <= 1e4)


# worst |riccati (Sigma = 1e10 on the active inputs, 1e-9 elsewhere) - active set| over LQ_SHAPES, measured
GAP_1E10 = 2.62e-9


def test_barrier_recursion_approaches_the_active_set():
    """(a) with Sigma = 1e10 on the inputs classed active and 1e-9 on the others against (b), the
    active-set reference.  Measured per shape (max absolute difference, entries of order 1 to 1.7):
    (3,2,5) 2.1e-10, (3,2,20) 1.2e-9, (4,1,50) 1.7e-9, (5,1,50) 9.4e-10, (4,2,12) 2.6e-9 -- worst
    2.62e-9; at Sigma = 1e6 the same cases give 1.2e-6 to 2.6e-5, so the gap goes like 1/Sigma: a
    property of the barrier term, not of the code.  Asserted: 16 x the worst measured value.  The rows
    of the active inputs are within the same distance of zero."""
    worst = 0.0
    for seed, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
        A, B, H = sr.random_lq(nx, nu, N, seed)
        m = sr.random_input_mask(nx, nu, N, seed)
        Sig = np.where(m, 1e10, 1e-9)
        Sig[:, :nx] = 0.0
        Sig[N, nx:] = 0.0
        dw, ok = sr.riccati_sens(A, B, H, Sig)
        assert ok
        act = np.zeros(dw.shape[0], bool)
        for k in range(N):
            act[sr.iu_w(nx, nu, k)] = m[k, nx:]
        assert act.any()
        ref = sr.active_set_sens(A, B, H, act)
        gap = float(np.max(np.abs(dw - ref)))
        print(f"{(nx, nu, N)}: |riccati - active set| = {gap:.3e}, active rows {np.max(np.abs(dw[act])):.3e}")
        worst = max(worst, gap)
        assert np.max(np.abs(dw[act])) <= 16 * GAP_1E10
    assert worst <= 16 * GAP_1E10


def test_refinement_on_an_unstable_open_loop():
    """The kernel's refinement step restated (helpers/sens_ref.py refined_sens) on the move-blocked
    cart-pole QP's tables (N = 50, 45 blocked stages: P_k = Q + A^T P_{k+1} A over an open loop of
    spectral radius 1.05), no barrier term.  Bound: 64 x E_ref, the GPU tests' own.  Measured against
    the long-double recursion: float64 recursion 3.9e-13 (misses the bound: why the step exists);
    after one step with long-double residuals 1.3e-16; after one step with float64 residuals
    7.7e-14 (misses it: why the kernel sums the residuals in twice the working precision).  On the
    stable random stages the step changes nothing of note (both sides of it meet the bound)."""
    from mpcx import lti

    lin = lti.inverted_pendulum_qp(N=50)
    A, B, H = sr.linear_operands(lin)
    Sig = np.zeros((lin.N + 1, lin.nx + lin.nu))
    ref, ok = sr.riccati_sens(A, B, H, Sig, np.longdouble)
    assert ok
    before, after = sr.refined_sens(A, B, H, Sig)
    plain = sr.refined_sens(A, B, H, Sig, resid_dtype=np.float64)[1]
    tol = 64.0 * sr.e_ref()
    print(f"cart-pole QP: before {sr.rel_err(before, ref):.3e}, after {sr.rel_err(after, ref):.3e}, "
          f"float64 residuals {sr.rel_err(plain, ref):.3e} (tolerance {tol:.3e})")
    assert np.array_equal(after[:lin.nx], np.eye(lin.nx))
    assert sr.rel_err(after, ref) <= tol
    for seed, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
        A, B, H = sr.random_lq(nx, nu, N, seed)
        Sig = np.where(sr.random_input_mask(nx, nu, N, seed), 1e9, 0.0)
        ref, _ = sr.riccati_sens(A, B, H, Sig, np.longdouble)
        before, after = sr.refined_sens(A, B, H, Sig)
        assert sr.rel_err(before, ref) <= tol and sr.rel_err(after, ref) <= tol


def test_classification():
    """classify(): class (i) = on the bound with a multiplier, class (ii) = no multiplier; anything else fails."""
    nx = 2
    w = np.array([0.0, 0.0, 1.0 - 1e-9, 0.3, 0.3, 0.2, 0.1, 0.1])
    lb = np.array([-1e20, -1e20, -1.0, -1e20, -1e20, -1.0, -1e20, -1e20])
    ub = -lb
    lam = np.array([0.0, 0.0, 0.5, 0.0, 0.0, 1e-9, 0.0, 0.0])
    act, ok = sr.classify(w, lam, lb, ub, nx)
    assert ok and act.tolist() == [False, False, True, False, False, False, False, False]
    lam[5] = 1e-4  # neither active nor without a multiplier
    assert not sr.classify(w, lam, lb, ub, nx)[1]
    Sig = sr.sigma_of(w, lam, lb, ub, nx, 1)
    assert Sig.shape == (3, 3) and Sig[0, 2] == 0.5 / (1.0 - w[2]) and Sig[1, 2] == 1e-4 / (1.0 - w[5])
    assert not Sig[:, :2].any() and Sig[2, 2] == 0.0  # no state is bounded, node N has no input


# ------------------------------------------------------------------------------------------
# the C ABI: both entry points are declared and exported
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mpc-verde_amd")], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_the_sensitivity_entry_points():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*int\s+(mpcx_\w+)\s*\(", src, re.M))
    for s in SYMBOLS:
        assert s in declared, s
    # the header states what is computed: the formula, the barrier-problem caveat, K0's place in dw_dx0
    for text in ("Phi_{k+1} = (A_k + B_k K_k) Phi_k", "BARRIER problem", "rows nx..nx+nu of dw_dx0"):
        assert text in src, text


def test_library_exports_the_sensitivity_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(rf"\bT {s}$", out, re.M), s


def test_python_binding_lists_the_entry_points():
    import mpcx

    for s in SYMBOLS:
        assert s in mpcx._lib.EXPORTS
    assert callable(mpcx.Solver.sens_x0)
