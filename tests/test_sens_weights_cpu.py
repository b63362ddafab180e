"""CPU: the algebra of the sensitivities to the cost weights (tests/helpers/sens_weights_ref.py) and the C
ABI's new entry points.

The kernels (csrc/sens.h sens_wt_kernel, sens_wt_vjp_kernel) solve the KKT system of the parameter
sensitivities with the right-hand side r_k = d(grad_z q_k)/d(weights) . dwt_k on every stage, d = 0, dX_0 = 0.
Here that recursion is restated in NumPy with sens_p_ref's factors and sweeps and checked against the dense
KKT solve, against central differences of a fixed-mu barrier LQ solve under perturbed stage Hessians (signs
and the factor 2), the reverse formulas through the dot-product identity (the factor 2 on the packed
off-diagonals), and the tracking-cost property: scaling the whole objective moves nothing."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sens_bounds_ref as sb  # noqa: E402
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402
import sens_vjp_ref as sv  # noqa: E402
import sens_weights_ref as sw  # noqa: E402

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_weight_dims", "mpcx_set_weights", "mpcx_sens_weights", "mpcx_sens_weights_dev",
           "mpcx_sens_weights_vjp", "mpcx_sens_weights_vjp_dev")
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
CASES = [(s, shape, sg) for s, shape in enumerate(sr.LQ_SHAPES) for sg in sr.LQ_SIGMAS]


def problem(seed, shape, sigma):
    """Random LQ stages with Sigma on a seeded 40 % of the inputs and on two states (sens_bounds_ref's mask)."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    lo, up = sb.random_bound_mask(nx, nu, N, seed)
    return A, B, H, sb.stage_sigma(np.where(lo | up, sigma, 0.0), nx, nu)


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_recursion_against_the_dense_kkt_solve(seed, shape, sigma):
    """1. The recursion with the weight right-hand sides (nx seeded packed per-stage directions at seeded
    residuals) against the dense solve of the same system, float64: 16 x cond x eps x max(1, |dw|_max),
    test_sens_p_cpu.py's rule, held against the recursion after the kernel's refinement round (a Sigma of 1e9
    on a state: tests/test_sens_bounds_cpu.py records why).  dX_0 = 0 exactly."""
    nx, nu, N = shape
    A, B, H, Sig = problem(seed, shape, sigma)
    r = sw.packed_rhs(sw.random_packed(nx, nu, N, seed), sw.random_residuals(nx, nu, N, seed))
    plain, ok = sw.weights_sens(A, B, H, Sig, r)
    assert ok and not plain[:nx].any()
    before, dw = sw.refined_weights_sens(A, B, H, Sig, r)
    assert np.array_equal(before, plain) and not dw[:nx].any()
    d, dx0 = sw._zeros(A, r.shape[2], np.float64)
    ref, cond = sp.dense_kkt_sens(A, B, H, Sig, r, d, dx0)
    tol = 16.0 * cond * EPS * max(1.0, float(np.max(np.abs(ref))))
    e0, e1 = float(np.max(np.abs(plain - ref))), float(np.max(np.abs(dw - ref)))
    print(f"{shape} Sigma {sigma:g}: |sweeps - dense| {e0:.3e}, |refined - dense| {e1:.3e}, cond {cond:.3e}, bound {tol:.3e}")
    assert e1 <= tol
    assert np.max(np.abs(dw)) > 1e-3


def test_yardsticks():
    """e_ref_w and e_ref_wvjp, the GPU tests' yardsticks, computed as sens_bounds_ref.e_ref_b is; the bound is
    test_sens_cpu.py's count of roundings."""
    e, ev = sw.e_ref_w(), sw.e_ref_wvjp()
    print(f"e_ref_w = {e:.3e}, e_ref_wvjp = {ev:.3e}")
    assert 0.0 < e <= 2.0 ** 20 * EPS and 0.0 < ev <= 2.0 ** 20 * EPS


def test_right_hand_sides():
    """A diagonal direction is the packed one with zero off-diagonals, forward and reverse, bit for bit."""
    nx, nu, N = 3, 2, 4
    nz = nx + nu
    rng = np.random.default_rng(5)
    e, dwt, zt = rng.normal(size=(N, nz)), rng.normal(size=(2, N, nz)), rng.normal(size=(N, nz, 2))
    iu = np.triu_indices(nz)
    dWp = np.zeros((2, N, nz * (nz + 1) // 2))
    dWp[:, :, iu[0] == iu[1]] = dwt
    assert np.array_equal(sw.packed_rhs(dWp, e), sw.diag_rhs(dwt, e))
    assert np.array_equal(sw.packed_vjp(zt, e)[:, :, iu[0] == iu[1]], sw.diag_vjp(zt, e))
    assert np.array_equal(sw.unpack_sym(dWp, nz), np.swapaxes(sw.unpack_sym(dWp, nz), -1, -2))


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES))[:3])
def test_against_central_differences_of_a_barrier_solve(seed, shape):
    """2. Signs and the factor 2 against the problem itself: a fixed-mu (1e-3) barrier LQ problem with one-sided
    bounds (tests/test_sens_bounds_cpu.py's: the multiplier split is exact), its stage Hessians H_k = 2 W_k
    perturbed along 2 dW_k with dW_k seeded symmetric: column 0 one direction per stage, column 1 the same
    direction at every stage.  r_k = 2 dW_k z_k (zero reference; the linear term c has no weight).  Central
    differences at h = 1e-4 and h / 2; asserted is |dw - FD(h/2)| <= spread + 1e-7."""
    nx, nu, N = shape
    nz = nx + nu
    A, B, H = sr.random_lq(nx, nu, N, seed)
    lo, up = sb.random_bound_mask(nx, nu, N, seed)
    rng = np.random.default_rng(seed + 6000)
    nw = nx + nz * N
    c, x0 = rng.normal(size=nw), rng.normal(size=nx)
    mu = 1e-3
    w_unc, _, res = sb.barrier_lq(A, B, H, c, x0, np.full(nw, -1e20), np.full(nw, 1e20), mu, np.zeros(nw))
    assert res <= 1e-11
    off = rng.choice([-0.05, 0.3], size=nw)
    lb = np.where(lo, w_unc - off, -1e20)
    ub = np.where(up, w_unc + off, 1e20)
    start = np.where(lo, np.maximum(w_unc, lb + 0.1), np.where(up, np.minimum(w_unc, ub - 0.1), w_unc))
    w, lam_x, res = sb.barrier_lq(A, B, H, c, x0, lb, ub, mu, start)
    assert res <= 1e-11, res
    assert np.sum(np.abs(lam_x) > 1e-2) >= 2
    Sig = sr.sigma_of(w, lam_x, lb, ub, nx, nu)
    dWp = sw.random_packed(nx, nu, N, seed, m=2)
    dWp[1] = dWp[1, 0]  # the stage-uniform column
    z = np.stack([np.concatenate([w[sr.ix_w(nx, nu, k)], w[sr.iu_w(nx, nu, k)]]) for k in range(N)])
    dw, ok = sw.weights_sens(A, B, H, Sig, sw.packed_rhs(dWp, z))
    assert ok
    dH = 2.0 * sw.unpack_sym(dWp, nz)  # (2, N, nz, nz)
    fd = {}
    for h in (1e-4, 5e-5):
        cols = []
        for j in range(2):
            side = []
            for sgn in (1.0, -1.0):
                wl, _, res = sb.barrier_lq(A, B, H + sgn * h * dH[j], c, x0, lb, ub, mu, w)
                assert res <= 1e-11
                side.append(wl)
            cols.append((side[0] - side[1]) / (2 * h))
        fd[h] = np.stack(cols, axis=1)
    spread = float(np.max(np.abs(fd[1e-4] - fd[5e-5])))
    err = float(np.max(np.abs(dw - fd[5e-5])))
    print(f"{shape}: |dw| {np.abs(dw).max():.3g}, FD spread {spread:.3e}, |dw - FD| {err:.3e}")
    assert err <= spread + 1e-7
    assert np.min(np.max(np.abs(dw), axis=0)) > 1e-3  # both columns move the solution


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_dot_product_identity(seed, shape, sigma):
    """3. <g, dw> = sum_k <gW_k, dW_k> for the forward dw and the reverse formulas' packed rows, each after the
    kernel's refinement round, nx seeded packed per-stage directions (off-diagonals included: a factor 1 in
    place of 2 on a < b fails this) and nx seeded cotangents, in float64 (residuals in long double) and long
    double: relative to the sum of the absolute terms of both sides, 2^20 roundings (test_sens_vjp_cpu.py's
    bound).  The diagonal formulas the same way."""
    nx, nu, N = shape
    A, B, H, Sig = problem(seed, shape, sigma)
    g = sv.random_cotangent(nx, nu, N, seed)
    for dt, bound in ((np.float64, 2.0 ** 20 * EPS), (LD, 2.0 ** 20 * float(np.finfo(LD).eps))):
        e = np.asarray(sw.random_residuals(nx, nu, N, seed), dt)
        dWp = np.asarray(sw.random_packed(nx, nu, N, seed), dt)
        dwt = dWp[:, :, :nx + nu]
        zt = sw.refined_adjoint_z(A, B, H, Sig, g, LD, dt)
        gd = np.asarray(g, dt)
        for name, r, gk, d in (("packed", sw.packed_rhs(dWp, e), sw.packed_vjp(zt, e), dWp),
                               ("diagonal", sw.diag_rhs(dwt, e), sw.diag_vjp(zt, e), dwt)):
            dw = sw.refined_weights_sens(A, B, H, Sig, r, LD, dt)[1]
            lhs = gd.T @ dw
            rhs = np.einsum("ckn,dkn->cd", gk, d)
            mag = np.abs(gd).T @ np.abs(dw) + np.einsum("ckn,dkn->cd", np.abs(gk), np.abs(d))
            viol = float(np.max(np.abs(lhs - rhs) / mag))
            print(f"{shape} Sigma {sigma:g} {name}: identity violation {viol:.3e} in {np.dtype(dt).name}")
            assert viol <= bound
        half = sw.packed_vjp(zt, e).copy()  # the wrong formula (no factor 2 on a < b) is told apart
        iu = np.triu_indices(nx + nu)
        half[:, :, iu[0] != iu[1]] *= 0.5
        assert np.max(np.abs(gd.T @ sw.refined_weights_sens(A, B, H, Sig, sw.packed_rhs(dWp, e), LD, dt)[1]
                             - np.einsum("ckn,dkn->cd", half, dWp))) > 1e-3


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES)))
def test_tracking_cost_scaling_moves_nothing(seed, shape):
    """4. No bounds (Sigma = 0) and the cost sum_k (z_k - zr_k)^T W_k (z_k - zr_k): the direction dW = W scales the
    whole objective, so dw = 0: |dw| <= 64 e_ref_w max|w|.  The optimum w comes from the recursion in long
    double (r_k = -2 W_k zr_k, dX_0 = x0), so that the right-hand side 2 W_k (z_k - zr_k), the cost's own
    gradient, is the exact one rounded once."""
    nx, nu, N = shape
    nz = nx + nu
    A, B, H = sr.random_lq(nx, nu, N, seed)
    W = H / 2.0
    rng = np.random.default_rng(seed + 9000)
    zr, x0 = rng.normal(size=(N, nz)), rng.normal(size=nx)
    Sig = np.zeros((N + 1, nz))
    lin_term = -2.0 * np.einsum("kij,kj->ki", np.asarray(W, LD), np.asarray(zr, LD))[:, :, None]
    w, ok = sp.affine_sens(A, B, H, Sig, lin_term, np.zeros((N, nx, 1)), x0[:, None], LD)
    assert ok
    w = w[:, 0]
    z = np.stack([np.concatenate([w[sr.ix_w(nx, nu, k)], w[sr.iu_w(nx, nu, k)]]) for k in range(N)])
    iu = np.triu_indices(nz)
    Wp = W[:, iu[0], iu[1]][None]  # (1, N, nh): dW = W
    r = np.asarray(sw.packed_rhs(np.asarray(Wp, LD), z - np.asarray(zr, LD)), np.float64)
    dw, ok = sw.weights_sens(A, B, H, Sig, r)
    assert ok
    tol = 64.0 * sw.e_ref_w() * float(np.max(np.abs(w)))
    print(f"{shape}: |w| {float(np.max(np.abs(w))):.3g}, |r| {np.abs(r).max():.3g}, |dw| {np.abs(dw).max():.3e} "
          f"(tolerance {tol:.3e})")
    assert np.max(np.abs(dw)) <= tol
    # another direction does move the solution
    other, _ = sw.weights_sens(A, B, H, Sig, sw.packed_rhs(sw.random_packed(nx, nu, N, seed, m=1), np.asarray(z - zr, np.float64)))
    assert np.max(np.abs(other)) > 1e-3


def test_exact_properties_of_the_restatement():
    """A zero direction gives zeros, a zero cotangent zero gradient rows."""
    shape = sr.LQ_SHAPES[1]
    nx, nu, N = shape
    A, B, H, Sig = problem(1, shape, 1e4)
    e = sw.random_residuals(nx, nu, N, 1)
    assert not sw.weights_sens(A, B, H, Sig, sw.packed_rhs(0.0 * sw.random_packed(nx, nu, N, 1), e))[0].any()
    zt, _ = sw.adjoint_z(A, B, H, Sig, np.zeros((nx + (nx + nu) * N, 2)))
    assert not sw.packed_vjp(zt, e).any() and not sw.diag_vjp(zt, e).any()


# ------------------------------------------------------------------------------------------
# 5. the C ABI: the entry points are declared and exported
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
    # the header states the right-hand sides, the reverse formulas and the identity
    for text in ("r_{k,i} = 2 dW_{k,i} e_{k,i}", "r_k = 2 dW_k (z_k - zr_k)", "gWk_k[a,b] = 2 (z~_a e_b + z~_b e_a)",
                 "<g, dw> = sum_{k<N} z~_k^T r_k", "B x m x (per_stage ? N : 1) x n_wt"):
        assert text in src, text


def test_library_exports_the_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(rf"\bT {s}$", out, re.M), s


def test_python_binding_lists_the_entry_points():
    import mpcx
    from mpcx.autograd import MPCWeightsFunction
    from mpcx.device import DeviceLoop

    for s in SYMBOLS:
        assert s in mpcx._lib.EXPORTS
    assert callable(mpcx.Solver.sens_weights) and callable(mpcx.Solver.sens_weights_vjp)
    assert callable(mpcx.Solver.set_weights)
    assert callable(DeviceLoop.sens_weights) and callable(DeviceLoop.sens_weights_vjp)
    assert callable(MPCWeightsFunction.apply)
