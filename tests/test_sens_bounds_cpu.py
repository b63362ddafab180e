"""CPU: the algebra of the sensitivities to the box bounds (tests/helpers/sens_bounds_ref.py) and the C
ABI's four entry points.

The kernels (csrc/sens.h sens_bnd_kernel, sens_bnd_vjp_kernel) solve the KKT system of the parameter
sensitivities with the right-hand side r_i = -(sigL_i dlb_i + sigU_i dub_i) on every bounded variable, the
X rows of node N included.  Here that recursion is restated in NumPy with sens_p_ref's factors and sweeps
and checked against the dense KKT solve, through one step of the kernel's refinement, against central
differences of a fixed-mu barrier LQ solve (signs and the node-N term), against the active-set
reference, and the reverse formulas through the dot-product identity."""
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

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_sens_bounds", "mpcx_sens_bounds_dev", "mpcx_sens_bounds_vjp", "mpcx_sens_bounds_vjp_dev")
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
CASES = [(s, shape, sg) for s, shape in enumerate(sr.LQ_SHAPES) for sg in sr.LQ_SIGMAS]


def problem(seed, shape, sigma):
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    lo, up = sb.random_bound_mask(nx, nu, N, seed)
    assert (lo | up)[sr.ix_w(nx, nu, N)].any() and (lo | up)[sr.iu_w(nx, nu, 0)[0]:].any()
    return A, B, H, np.where(lo, sigma, 0.0), np.where(up, sigma, 0.0)


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_recursion_against_the_dense_kkt_solve(seed, shape, sigma):
    """The recursion with the bound right-hand sides, rq_N included (node N's state 0 is bounded in every
    case), against the dense solve (b) of the same system, float64.  The dense side is LU with partial
    pivoting on the row-equilibrated matrix, so its forward error is at most ~cond x eps x |dw|: bound
    16 x cond x eps x max(1, |dw|_max), test_sens_p_cpu.py's rule.  Held against it is the recursion after
    the kernel's refinement round (c): a Sigma of 1e9 on a state makes Huu' = R + B^T P B ill-conditioned
    where the KKT system is not (cond 1e2), and the sweeps alone are then off by up to 2e-7 -- printed, and
    asserted only to be no better than the refined result needs: the round is what the kernel relies on."""
    nx, nu, N = shape
    A, B, H, sL, sU = problem(seed, shape, sigma)
    dlb, dub = sb.random_directions(nx, nu, N, seed)
    plain, ok = sb.bounds_sens(A, B, H, sL, sU, dlb, dub)
    assert ok and not plain[:nx].any()
    before, dw = sb.refined_bounds_sens(A, B, H, sL, sU, dlb, dub)
    assert np.array_equal(before, plain) and not dw[:nx].any()
    ref, cond = sb.dense_kkt_bounds(A, B, H, sL, sU, dlb, dub)
    tol = 16.0 * cond * EPS * max(1.0, float(np.max(np.abs(ref))))
    e0, e1 = float(np.max(np.abs(plain - ref))), float(np.max(np.abs(dw - ref)))
    print(f"{shape} Sigma {sigma:g}: |sweeps - dense| {e0:.3e}, |refined - dense| {e1:.3e}, cond {cond:.3e}, bound {tol:.3e}")
    assert e1 <= tol
    # without node N's right-hand side the result is another one: the term is not optional
    at_n = np.zeros_like(sL, bool)
    at_n[sr.ix_w(nx, nu, N)] = True
    cut, _ = sb.bounds_sens(A, B, H, sL, sU, np.where(at_n[:, None], 0.0, dlb), np.where(at_n[:, None], 0.0, dub))
    assert np.max(np.abs(cut - plain)) > 1e-3


def test_yardsticks():
    """e_ref_b and e_ref_bvjp, the GPU tests' yardsticks, computed as sens_p_ref.e_ref_p is; the bound is
    test_sens_cpu.py's count of roundings."""
    e, ev = sb.e_ref_b(), sb.e_ref_bvjp()
    print(f"e_ref_b = {e:.3e}, e_ref_bvjp = {ev:.3e}")
    assert 0.0 < e <= 2.0 ** 20 * EPS and 0.0 < ev <= 2.0 ** 20 * EPS


def test_refinement_restated():
    """One round of the kernel's refinement restated with the bound right-hand sides (helper (c)) on the
    move-blocked cart-pole QP's tables (test_sens_p_cpu.py's case: an unstable open loop), a Sigma of 1e6 on
    a seeded third of the inputs and on state 0 of node N, nx seeded directions, against both rounds in long
    double (helpers' ``reference``): after the round within 64 x e_ref_b, the GPU tests' own tolerance, and
    no worse than before.  The same on the random stages with Sigma = 1e9 on inputs AND states, where the
    sweeps alone miss the tolerance by orders of magnitude (printed) and the plain long-double recursion is
    itself off by up to 6e-11: why the GPU tests' reference restates both rounds."""
    from mpcx import lti

    lin = lti.inverted_pendulum_qp(N=50)
    A, B, H = sr.linear_operands(lin)
    nx, nu, N = lin.nx, lin.nu, lin.N
    rng = np.random.default_rng(21)
    lo = np.zeros(lin.n_w_ms, bool)
    for k in range(N):
        lo[sr.iu_w(nx, nu, k)] = rng.random(nu) < 0.33
    lo[sr.ix_w(nx, nu, N)[0]] = True
    side = rng.random(lin.n_w_ms) < 0.5
    sL, sU = np.where(lo & side, 1e6, 0.0), np.where(lo & ~side, 1e6, 0.0)
    dlb, dub = sb.random_directions(nx, nu, N, 21)
    ref = sb.reference(A, B, H, sL, sU, dlb, dub)
    before, after = sb.refined_bounds_sens(A, B, H, sL, sU, dlb, dub)
    tol = 64.0 * sb.e_ref_b()
    e0, e1 = sr.rel_err(before, ref), sr.rel_err(after, ref)
    print(f"cart-pole QP: float64 solve {e0:.3e}, after one round {e1:.3e} (tolerance {tol:.3e})")
    assert e1 <= tol and e1 <= e0
    for seed, shape in enumerate(sr.LQ_SHAPES):
        A, B, H, sL, sU = problem(seed, shape, 1e9)
        dlb, dub = sb.random_directions(*shape, seed)
        ref = sb.reference(A, B, H, sL, sU, dlb, dub)
        plain_ld, _ = sb.bounds_sens(A, B, H, sL, sU, dlb, dub, LD)
        before, after = sb.refined_bounds_sens(A, B, H, sL, sU, dlb, dub)
        e0, e1 = sr.rel_err(before, ref), sr.rel_err(after, ref)
        print(f"{shape} Sigma 1e9: float64 solve {e0:.3e}, after one round {e1:.3e}, plain long double "
              f"{sr.rel_err(plain_ld, ref):.3e} (tolerance {tol:.3e})")
        assert e1 <= tol


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES))[:3])
def test_against_central_differences_of_a_barrier_solve(seed, shape):
    """Signs and the node-N term against the problem itself: a fixed-mu (1e-3) barrier LQ problem with
    ONE-SIDED bounds (each bounded variable has a lower or an upper bound, never both), so the one-sided
    multiplier split is exact and the recursion's dw is the derivative of the barrier solution w(lb, ub)
    itself.  Bounds sit around the unconstrained solution so that some are active (multiplier O(0.1..1))
    and some not, on inputs, on states of inner nodes and on state 0 of node N.  Central differences along
    two seeded directions (dlb, dub) at h = 1e-4 and h / 2: their truncation error is O(h^2), so the finer
    one is within spread / 3 of the derivative; asserted is |dw - FD(h/2)| <= spread + 1e-7 (the floor: the
    Newton solves' residual 1e-12 over 2 h = 1e-4, times the conditioning, 10)."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    lo, up = sb.random_bound_mask(nx, nu, N, seed)
    rng = np.random.default_rng(seed + 6000)
    nw = nx + (nx + nu) * N
    c, x0 = rng.normal(size=nw), rng.normal(size=nx)
    inf_l, inf_u = np.full(nw, -1e20), np.full(nw, 1e20)
    mu = 1e-3
    w_unc, _, res = sb.barrier_lq(A, B, H, c, x0, inf_l, inf_u, mu, np.zeros(nw))
    assert res <= 1e-11
    off = rng.choice([-0.05, 0.3], size=nw)  # the bound cuts 0.05 into the free solution, or lies 0.3 off it
    lb = np.where(lo, w_unc - off, -1e20)
    ub = np.where(up, w_unc + off, 1e20)
    start = np.where(lo, np.maximum(w_unc, lb + 0.1), np.where(up, np.minimum(w_unc, ub - 0.1), w_unc))
    w, lam_x, res = sb.barrier_lq(A, B, H, c, x0, lb, ub, mu, start)
    assert res <= 1e-11, res
    assert np.sum(np.abs(lam_x) > 1e-2) >= 2 and np.sum((np.abs(lam_x) > 0) & (np.abs(lam_x) < 1e-2)) >= 1
    sL, sU = sb.split_sigma(w, lam_x, lb, ub, nx)
    assert not np.any((sL > 0) & (sU > 0))
    dlb, dub = sb.random_directions(nx, nu, N, seed, m=2)
    dlb[:, 1], dub[:, 1] = 1.0, -1.0  # the uniform tightening
    dw, ok = sb.bounds_sens(A, B, H, sL, sU, dlb, dub)
    assert ok
    fd = {}
    for h in (1e-4, 5e-5):
        cols = []
        for j in range(2):
            side = []
            for sgn in (1.0, -1.0):
                wl, _, res = sb.barrier_lq(A, B, H, c, x0, np.where(lo, lb + sgn * h * dlb[:, j], lb),
                                           np.where(up, ub + sgn * h * dub[:, j], ub), mu, w)
                assert res <= 1e-11
                side.append(wl)
            cols.append((side[0] - side[1]) / (2 * h))
        fd[h] = np.stack(cols, axis=1)
    spread = float(np.max(np.abs(fd[1e-4] - fd[5e-5])))
    err = float(np.max(np.abs(dw - fd[5e-5])))
    print(f"{shape}: |dw| {np.abs(dw).max():.3g}, FD spread {spread:.3e}, |dw - FD| {err:.3e}")
    assert err <= spread + 1e-7
    assert np.max(np.abs(dw[sr.ix_w(nx, nu, N)])) > 1e-3  # node N moves with its bound


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_dot_product_identity(seed, shape, sigma):
    """<g, dw> = <g_lb, dlb> + <g_ub, dub> for the forward dw and the reverse formulas' (g_lb, g_ub), each
    after the kernel's refinement round (helper (c); the sweeps alone carry the ill-conditioning of Huu'
    under a state's Sigma of 1e9 into both sides), states bounded at an inner node and at node N, nx seeded
    directions and cotangents, in float64 (residuals in long double) and long double: relative to the sum of
    the absolute terms of both sides, 2^20 roundings (test_sens_vjp_cpu.py's bound)."""
    nx, nu, N = shape
    A, B, H, sL, sU = problem(seed, shape, sigma)
    dlb, dub = sb.random_directions(nx, nu, N, seed)
    g = sv.random_cotangent(nx, nu, N, seed)
    for dt, bound in ((np.float64, 2.0 ** 20 * EPS), (LD, 2.0 ** 20 * float(np.finfo(LD).eps))):
        dw = sb.refined_bounds_sens(A, B, H, sL, sU, dlb, dub, LD, dt)[1]
        gl, gu = sb.refined_bounds_vjp(A, B, H, sL, sU, g, LD, dt)
        assert not gl[:nx].any() and not gu[:nx].any()
        assert not gl[sL == 0].any() and not gu[sU == 0].any()
        gd, dl, du = np.asarray(g, dt), np.asarray(dlb, dt), np.asarray(dub, dt)
        lhs, rhs = gd.T @ dw, gl.T @ dl + gu.T @ du
        mag = np.abs(gd).T @ np.abs(dw) + np.abs(gl).T @ np.abs(dl) + np.abs(gu).T @ np.abs(du)
        viol = float(np.max(np.abs(lhs - rhs) / mag))
        print(f"{shape} Sigma {sigma:g}: identity violation {viol:.3e} in {np.dtype(dt).name}")
        assert viol <= bound


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES)))
def test_active_set_limit(seed, shape):
    """At Sigma = 1e9 the barrier sensitivities are the active-set ones to O(1 / Sigma): the variables with a
    Sigma move with their bound, dw_i = dbound_i, the rest solves the reduced KKT system (helper (d)).
    Tolerance: 1 / Sigma times (1 + |H|_max) (1 + |dw|_max) cond of the reduced system -- the first-order
    effect of the dropped term H_aa + ... against Sigma."""
    nx, nu, N = shape
    A, B, H, sL, sU = problem(seed, shape, 1e9)
    dlb, dub = sb.random_directions(nx, nu, N, seed)
    dw, _ = sb.bounds_sens(A, B, H, sL, sU, dlb, dub, LD)
    act = (sL + sU) > 0
    dbound = np.where((sL > 0)[:, None], dlb, dub)
    ref = sb.active_set_bounds(A, B, H, act, dbound)
    err = float(np.max(np.abs(np.asarray(dw, np.float64) - ref)))
    tol = 1e-9 * (1.0 + float(np.max(np.abs(H)))) * (1.0 + float(np.max(np.abs(ref)))) * 1e3
    print(f"{shape}: barrier (Sigma 1e9) against the active-set reference {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    assert np.max(np.abs(ref[act] - dbound[act])) == 0.0


def test_exact_properties_of_the_restatement():
    """Zero directions give zeros; directions on X_0's rows and on unbounded variables change nothing."""
    shape = sr.LQ_SHAPES[1]
    nx, nu, N = shape
    A, B, H, sL, sU = problem(1, shape, 1e4)
    dlb, dub = sb.random_directions(nx, nu, N, 1)
    z = np.zeros_like(dlb)
    assert not sb.bounds_sens(A, B, H, sL, sU, z, z)[0].any()
    dw, _ = sb.bounds_sens(A, B, H, sL, sU, dlb, dub)
    dl2, du2 = np.where((sL > 0)[:, None], dlb, 7.0), np.where((sU > 0)[:, None], dub, -3.0)
    assert np.array_equal(sb.bounds_sens(A, B, H, sL, sU, dl2, du2)[0], dw)
    gl, gu, _ = sb.bounds_vjp(A, B, H, sL, sU, z)
    assert not gl.any() and not gu.any()


# ------------------------------------------------------------------------------------------
# the C ABI: the entry points are declared and exported
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
    # the header states the right-hand side, the one-sided split, the reverse formulas and the identity
    for text in ("r_i = -(sigL_i dlbw_i + sigU_i dubw_i)", "ONE-SIDED split", "glbw_i = -sigL_i z~_i",
                 "<g, dw> = <glbw, dlbw> + <gubw, dubw>", "the X rows of node N included"):
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
    assert callable(mpcx.Solver.sens_bounds) and callable(mpcx.Solver.sens_bounds_vjp)
    assert callable(DeviceLoop.sens_bounds) and callable(DeviceLoop.sens_bounds_vjp)
