"""CPU: the algebra of the adjoint sensitivities (tests/helpers/sens_vjp_ref.py) and the C ABI's two
entry points.

The kernel (csrc/sens.h sens_vjp_kernel) solves the symmetric KKT system of the parameter
sensitivities with the cotangent as right-hand side and contracts the result with the model's
reference tangent.  Here the adjoint is restated in NumPy with the forward restatement's own factors and
sweeps and checked to be the transpose of the Jacobian that the forward recursion and the dense KKT
solve produce column by column, against itself in long double (the yardstick of the GPU tests), and
through one step of the kernel's refinement on the cart-pole QP's tables."""
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
import sens_vjp_ref as sv  # noqa: E402

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_sens_vjp", "mpcx_sens_vjp_dev")
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
CASES = [(s, shape, sg) for s, shape in enumerate(sr.LQ_SHAPES) for sg in sr.LQ_SIGMAS]


def unit_rhs(nx, nu, N):
    """(r, d, dx0) with one column per entry of (dx0, r_0..r_{N-1}, d_0..d_{N-1}): the identity, in the
    order of sens_vjp_ref.stack"""
    nz = nx + nu
    n_in = nx + N * nz + N * nx
    r, d, dx0 = np.zeros((N, nz, n_in)), np.zeros((N, nx, n_in)), np.zeros((nx, n_in))
    dx0[np.arange(nx), np.arange(nx)] = 1.0
    for k in range(N):
        r[k, np.arange(nz), nx + nz * k + np.arange(nz)] = 1.0
        d[k, np.arange(nx), nx + N * nz + nx * k + np.arange(nx)] = 1.0
    return r, d, dx0


@pytest.mark.parametrize("seed, shape, sigma", CASES)
def test_adjoint_is_the_transposed_jacobian(seed, shape, sigma):
    """The Jacobian J of dw with respect to (dx0, r, d), one column per entry, from the forward
    recursion (sens_p_ref.affine_sens) and from the dense KKT solve (dense_kkt_sens); the adjoint's
    stacked result (lam~_0, z~_k, lam~_{k+1}) for nx seeded cotangents g is J^T g, and with seeded r,
    d != 0 and dx0 the identity <g, dw> = lam~_0^T dx0 + sum (z~^T r + lam~^T d) holds.
    Float64.  Bounds: against the recursion's J 2^20 roundings (test_sens_cpu.py's count; both sides are
    the same factors' sweeps) of the sum of the absolute terms of each inner product; against the dense J
    16 x cond x eps (test_sens_p_cpu.py's rule for the dense side, whose error is normwise) of
    |J|_max |g|_1; the identity relative to the sum of the absolute terms of <g, dw>.
    Measured: identity 4.7e-16 at most (2.0e-19 in long double), against the recursion's J 6.2e-15 at most,
    against the dense J 2.1e-16 at most (bound 7.7e-14 to 1.2e-12)."""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    Sig = np.where(sr.random_input_mask(nx, nu, N, seed), sigma, 0.0)
    g = sv.random_cotangent(nx, nu, N, seed)
    lam0, zt, lamn, ok = sv.adjoint_sens(A, B, H, Sig, g)
    assert ok
    adj = sv.stack(lam0, zt, lamn)                      # (n_in, m)
    ur, ud, ux = unit_rhs(nx, nu, N)
    Jr, _ = sp.affine_sens(A, B, H, Sig, ur, ud, ux)    # (n_w, n_in)
    Jd, cond = sp.dense_kkt_sens(A, B, H, Sig, ur, ud, ux)
    for J, bound, what in ((Jr, 2.0 ** 20 * EPS, "recursion"), (Jd, 16.0 * cond * EPS, "dense")):
        ref = J.T @ g
        # the recursion's J has the adjoint's exact zeros: componentwise; the dense one's error is normwise
        mag = np.abs(J).T @ np.abs(g) if J is Jr else np.max(np.abs(J)) * np.sum(np.abs(g), axis=0)[None, :]
        err = float(np.max(np.abs(adj - ref) / np.maximum(mag, 1e-300)))
        print(f"{shape} Sigma {sigma:g}: adjoint against the {what} Jacobian's transpose {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    r, d, dx0 = sp.random_rhs(nx, nu, N, seed)
    d = np.random.default_rng(seed + 3000).normal(size=d.shape)
    for dt, bound in ((np.float64, 2.0 ** 20 * EPS), (LD, 2.0 ** 20 * float(np.finfo(LD).eps))):
        dw, _ = sp.affine_sens(A, B, H, Sig, r, d, dx0, dt)
        l0, z, ln, _ = sv.adjoint_sens(A, B, H, Sig, g, dt)
        lhs = np.asarray(g, dt).T @ dw
        rhs = sv.contract(l0, z, ln, np.asarray(r, dt), np.asarray(d, dt), np.asarray(dx0, dt))
        viol = float(np.max(np.abs(lhs - rhs) / (np.abs(np.asarray(g, dt)).T @ np.abs(dw))))
        print(f"{shape} Sigma {sigma:g}: identity violation {viol:.3e} in {np.dtype(dt).name}")
        assert viol <= bound


def test_exact_properties_of_the_restatement():
    """A zero cotangent gives zeros; a cotangent on the X_0 rows alone gives lam~_0 = gX_0 bit for bit and
    zeros elsewhere (X~_0 = 0 is held, so nothing propagates)."""
    nx, nu, N = sr.LQ_SHAPES[1]
    A, B, H = sr.random_lq(nx, nu, N, 1)
    Sig = np.where(sr.random_input_mask(nx, nu, N, 1), 1e4, 0.0)
    g = np.zeros((nx + (nx + nu) * N, 2))
    lam0, zt, lamn, _ = sv.adjoint_sens(A, B, H, Sig, g)
    assert not lam0.any() and not zt.any() and not lamn.any()
    g[:nx] = np.random.default_rng(5).normal(size=(nx, 2))
    lam0, zt, lamn, _ = sv.adjoint_sens(A, B, H, Sig, g)
    assert np.array_equal(lam0, g[:nx]) and not zt.any() and not lamn.any()


def test_float64_restatement_against_long_double():
    """The yardstick e_ref_vjp of the GPU tests, computed as sens_p_ref.e_ref_p (measured: 3.7e-15); the
    bound is test_sens_cpu.py's count of roundings."""
    e = sv.e_ref_vjp()
    print(f"e_ref_vjp = {e:.3e}")
    assert 0.0 < e <= 2.0 ** 20 * EPS


def test_linear_gradient_row_is_the_transposed_forward_map():
    """helper (c) on a LinearOCP: <g, sens_p's dw(dP)> = <gP, dP> with sens_p_ref.linear_rhs as the forward
    map from seeded dP, long double; bound 2^20 roundings of the terms.  Measured 3.5e-17."""
    from mpcx import lti

    lin = lti.inverted_pendulum_qp(N=50)
    A, B, H = sr.linear_operands(lin)
    Sig = np.zeros((lin.N + 1, lin.nx + lin.nu))
    rng = np.random.default_rng(12)
    dP, g = rng.normal(size=(3, lin.n_p)), rng.normal(size=(lin.n_w_ms, 2))
    dw, _ = sp.affine_sens(A, B, H, Sig, *sp.linear_rhs(lin, dP), LD)
    lam0, zt, _, _ = sv.adjoint_sens(A, B, H, Sig, g, LD)
    gP = sv.linear_vjp(lin, lam0, zt)
    lhs, rhs = np.asarray(g, LD).T @ dw, gP @ np.asarray(dP, LD).T
    viol = float(np.max(np.abs(lhs - rhs) / (np.abs(g).T @ np.abs(dw))))
    print(f"cart-pole QP: <g, dw> against <gP, dP>: {viol:.3e}")
    assert viol <= 2.0 ** 20 * float(np.finfo(LD).eps)


def test_refinement_on_an_unstable_open_loop():
    """The kernel's refinement round restated for the adjoint (helpers/sens_vjp_ref.py refined_adjoint) on
    the move-blocked cart-pole QP's tables (N = 50; test_sens_p_cpu.py's case), no barrier term, nx seeded
    normal cotangents over the whole of w, against the long-double restatement.  Asserted after the
    round, bound 64 x e_ref_vjp (the GPU tests' own, 2.3e-13): the gradient row (helper (c)) and the part of
    the result it is made of, (lam~_0, z~).  Measured, relative to max(1, |entry|):
                                   (lam~_0, z~)   gradient row   lam~_{k+1} (costates up to 1e5)
      float64 solve, no round        8.8e-13        8.8e-13         2.4e-12
      one round, long-double resid.  1.9e-16        1.9e-16         1.9e-13
      one round, float64 residuals   5.9e-14        5.9e-14         5.3e-13
    so the round is needed -- the solve alone misses the bound by a factor of 4 -- and with residuals in
    twice the working precision it reaches the last bit (float64 residuals stop a factor of 4 inside the
    bound), as for sens_p.  The costates lam~_{k+1}, which enter the row only
    through D_k (zero for every supported model), keep the rounding of P_k X~_k + p~_k, large terms that
    cancel; they are printed, not asserted.  On the random stages the round changes nothing that the
    bound sees."""
    from mpcx import lti

    lin = lti.inverted_pendulum_qp(N=50)
    A, B, H = sr.linear_operands(lin)
    Sig = np.zeros((lin.N + 1, lin.nx + lin.nu))
    g = np.random.default_rng(7).normal(size=(lin.n_w_ms, lin.nx))
    ref = sv.adjoint_sens(A, B, H, Sig, g, LD)
    assert ref[3]
    before, after = sv.refined_adjoint(A, B, H, Sig, g)
    plain = sv.refined_adjoint(A, B, H, Sig, g, resid_dtype=np.float64)[1]
    tol = 64.0 * sv.e_ref_vjp()
    used = lambda v: np.concatenate([v[0], v[1].reshape(-1, v[1].shape[2])])  # noqa: E731
    e = [sr.rel_err(used(v), used(ref)) for v in (before, after, plain)]
    row = [sr.rel_err(sv.linear_vjp(lin, v[0], v[1]), sv.linear_vjp(lin, ref[0], ref[1])) for v in (before, after, plain)]
    co = [sr.rel_err(v[2], ref[2]) for v in (before, after, plain)]
    for name, a, b, c in zip(("float64 solve", "after one round", "float64 residuals"), e, row, co):
        print(f"cart-pole QP, {name}: (lam0, z) {a:.3e}, gradient row {b:.3e}, costates {c:.3e} (tolerance {tol:.3e})")
    assert e[1] <= tol and row[1] <= tol
    assert e[1] < e[0] and row[1] < row[0]
    for seed, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
        A, B, H = sr.random_lq(nx, nu, N, seed)
        g = sv.random_cotangent(nx, nu, N, seed)
        Sig = np.where(sr.random_input_mask(nx, nu, N, seed), 1e9, 0.0)
        ref = sv.stack(*sv.adjoint_sens(A, B, H, Sig, g, LD)[:3])
        before, after = sv.refined_adjoint(A, B, H, Sig, g)
        assert sr.rel_err(sv.stack(*before), ref) <= tol and sr.rel_err(sv.stack(*after), ref) <= tol


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
    # the header states the identity, the gradient row of both layouts and the refusals
    for text in ("<g, dw> = lam~_0^T dx0 + sum_{k<N} ( z~_k^T r_k + lam~_{k+1}^T d_k )",
                 "gzr_k = G_k^T z~_k + D_k^T lam~_{k+1}", "gP[nx : 2 nx] = sum_k gzr_k[:nx]", "B x m x n_p"):
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
    assert callable(mpcx.Solver.sens_vjp) and callable(mpcx.Solver.gain_p) and callable(DeviceLoop.sens_vjp)
    # import mpcx stays free of torch (mpcx.autograd, like mpcx.device, is imported on demand)
    code = "import sys, mpcx; assert 'torch' not in sys.modules and not hasattr(mpcx, 'autograd')"
    pkg = os.path.join(ROOT, "mpc-verde_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
