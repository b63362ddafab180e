"""CPU: the algebra of the directional sensitivities to the parameter row (tests/helpers/sens_p_ref.py)
and the C ABI's two entry points.

The kernel (csrc/sens.h sens_p_kernel) solves the KKT system of the sensitivities to x0 with the
right-hand side of a parameter direction: an affine Riccati recursion and one refinement step.  Here
the recursion is restated in NumPy and checked against a dense solve of the same system, against the
x0 recursion it contains, against itself in long double (the yardstick of the GPU tests) and against
the parametric active-set reference."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_sens_p", "mpcx_sens_p_dev")
EPS = float(np.finfo(np.float64).eps)
CASES = [(s, shape, sg) for s, shape in enumerate(sr.LQ_SHAPES) for sg in sr.LQ_SIGMAS]


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_recursion_against_the_dense_kkt_solve(seed, shape, sigma):
    """The affine recursion (float64) against the dense solve of the same KKT system, seeded normal r,
    d and dx0 (d non-zero here: no supported model has one, the code path does).  The dense side is
    LU with partial pivoting on the row-equilibrated matrix, backward stable, so its own forward error
    is at most ~cond x eps x |dw|; the recursion's is the yardstick's.  Bound: 16 x cond x eps x
    max(1, |dw|_max), cond the 2-norm condition number of the equilibrated matrix (22 to 340 on
    these shapes).  Measured: at most 2.6e-14 absolute, 1/130 of the bound or less."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    r, d, dx0 = sp.random_rhs(nx, nu, N, seed)
    d = np.random.default_rng(seed + 3000).normal(size=d.shape)
    Sig = np.where(sr.random_input_mask(nx, nu, N, seed), sigma, 0.0)
    got, ok = sp.affine_sens(A, B, H, Sig, r, d, dx0)
    ref, cond = sp.dense_kkt_sens(A, B, H, Sig, r, d, dx0)
    assert ok
    err = float(np.max(np.abs(got - ref)))
    tol = 16.0 * cond * EPS * max(1.0, float(np.max(np.abs(ref))))
    print(f"{shape} Sigma {sigma:g}: |recursion - dense| {err:.3e}, cond {cond:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert np.array_equal(got[:nx], dx0)


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES)))
def test_x0_directions_are_the_x0_recursion(seed, shape):
    """With r = 0, d = 0 and dX_0 = I the recursion is sens_ref.riccati_sens: in long double the two
    differ by the association of the forward products only.  Bound: 2^20 long-double roundings, the
    count of test_sens_cpu.py test_float64_recursion_against_long_double."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    LD = np.longdouble
    for sg in sr.LQ_SIGMAS:
        Sig = np.where(sr.random_input_mask(nx, nu, N, seed), sg, 0.0)
        got, ok = sp.affine_sens(A, B, H, Sig, np.zeros((N, nx + nu, nx)), np.zeros((N, nx, nx)), np.eye(nx), LD)
        ref, _ = sr.riccati_sens(A, B, H, Sig, LD)
        assert ok
        assert sr.rel_err(got, ref) <= 2.0 ** 20 * float(np.finfo(LD).eps)
    zero, _ = sp.affine_sens(A, B, H, Sig, np.zeros((N, nx + nu, 1)), np.zeros((N, nx, 1)), np.zeros((nx, 1)))
    assert not zero.any()


def test_float64_recursion_against_long_double():
    """The yardstick e_ref_p of the GPU tests, computed as sens_ref.e_ref (measured: 1.9e-15); the bound
    is that test's count of roundings."""
    e = sp.e_ref_p()
    print(f"e_ref_p = {e:.3e}")
    assert 0.0 < e <= 2.0 ** 20 * EPS


def test_barrier_recursion_approaches_the_parametric_active_set():
    """(a) with Sigma = 1e10 on the inputs classed active and 1e-9 on the others against (c), the
    parametric active-set reference, seeded normal r and dx0.  The gap is the barrier term's own, 1/Sigma
    times the solution's scale (test_sens_cpu.py measured 2.62e-9 for the x0 directions, entries of order
    1); here the right-hand sides are normal over every stage and the entries reach 3.5: measured 2.5e-9
    to 8.0e-9.  Asserted: 16 x GAP_1E10 of that test x max(1, |dw|_max); the rows of the active inputs are
    within it of zero."""
    GAP_1E10 = 2.62e-9  # tests/test_sens_cpu.py: the same stages and Sigma, x0 directions
    for seed, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
        A, B, H = sr.random_lq(nx, nu, N, seed)
        r, d, dx0 = sp.random_rhs(nx, nu, N, seed)
        m = sr.random_input_mask(nx, nu, N, seed)
        Sig = np.where(m, 1e10, 1e-9)
        Sig[:, :nx] = 0.0
        Sig[N, nx:] = 0.0
        dw, ok = sp.affine_sens(A, B, H, Sig, r, d, dx0)
        assert ok
        act = np.zeros(dw.shape[0], bool)
        for k in range(N):
            act[sr.iu_w(nx, nu, k)] = m[k, nx:]
        ref = sp.active_set_sens_p(A, B, H, act, r, d, dx0)
        gap, scale = float(np.max(np.abs(dw - ref))), max(1.0, float(np.max(np.abs(ref))))
        print(f"{(nx, nu, N)}: |recursion - active set| = {gap:.3e}, |dw|_max {scale:.2f}")
        assert gap <= 16 * GAP_1E10 * scale and np.max(np.abs(dw[act])) <= 16 * GAP_1E10 * scale
        # with nothing active and no r it is sens_ref's active-set reference
        none = np.zeros(dw.shape[0], bool)
        assert np.allclose(sp.active_set_sens_p(A, B, H, none, 0 * r, d, np.eye(nx)),
                           sr.active_set_sens(A, B, H, none), rtol=0, atol=1e-11)


def test_refinement_with_right_hand_sides_on_an_unstable_open_loop():
    """The kernel's refinement step restated with right-hand sides (helpers/sens_p_ref.py refined_sens_p)
    on the move-blocked cart-pole QP's tables (N = 50; test_sens_cpu.py's case), no barrier term, nx
    seeded directions over the whole parameter row.  Bound: 64 x e_ref_p, the GPU tests' own.  Measured
    against the long-double recursion: float64 recursion 6.7e-14 (half the bound of 1.2e-13: these
    directions excite the unstable mode less than the x0 columns, whose 3.9e-13 is in the same system),
    after one step with long-double residuals 1.2e-16, with float64 residuals 3.6e-14."""
    from mpcx import lti

    lin = lti.inverted_pendulum_qp(N=50)
    A, B, H = sr.linear_operands(lin)
    Sig = np.zeros((lin.N + 1, lin.nx + lin.nu))
    dP = np.random.default_rng(7).normal(size=(lin.nx, lin.n_p))
    r, d, dx0 = sp.linear_rhs(lin, dP)
    ref, ok = sp.affine_sens(A, B, H, Sig, r, d, dx0, np.longdouble)
    assert ok
    before, after = sp.refined_sens_p(A, B, H, Sig, r, d, dx0)
    plain = sp.refined_sens_p(A, B, H, Sig, r, d, dx0, resid_dtype=np.float64)[1]
    tol = 64.0 * sp.e_ref_p()
    print(f"cart-pole QP: before {sr.rel_err(before, ref):.3e}, after {sr.rel_err(after, ref):.3e}, "
          f"float64 residuals {sr.rel_err(plain, ref):.3e} (tolerance {tol:.3e})")
    assert np.array_equal(after[:lin.nx], dx0)
    assert sr.rel_err(after, ref) <= tol
    for seed, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
        A, B, H = sr.random_lq(nx, nu, N, seed)
        r, d, dx0 = sp.random_rhs(nx, nu, N, seed)
        Sig = np.where(sr.random_input_mask(nx, nu, N, seed), 1e9, 0.0)
        ref, _ = sp.affine_sens(A, B, H, Sig, r, d, dx0, np.longdouble)
        before, after = sp.refined_sens_p(A, B, H, Sig, r, d, dx0)
        assert sr.rel_err(before, ref) <= tol and sr.rel_err(after, ref) <= tol


# ------------------------------------------------------------------------------------------
# the C ABI: both entry points are declared and exported
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mpc-verde_amd")], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_the_entry_points():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*int\s+(mpcx_\w+)\s*\(", src, re.M))
    for s in SYMBOLS:
        assert s in declared, s
    # the header states what is computed: the right-hand side, the recursion, the layouts, the refusals
    for text in ("r_k = d(grad_{z_k} l_k)/dp . dp", "kf_k = -Huu'_k^-1 gu", "B x n_w x m", "MPCX_MODEL_PATH_BICYCLE (its"):
        assert text in src, text


def test_library_exports_the_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(rf"\bT {s}$", out, re.M), s


def test_python_binding_lists_the_entry_points():
    import mpcx
    from mpcx.device import DeviceLoop

    for s in SYMBOLS:
        assert s in mpcx._lib.EXPORTS
    assert callable(mpcx.Solver.sens_p) and callable(mpcx.Solver.sens_xref) and callable(DeviceLoop.sens_p)
