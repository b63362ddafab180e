"""CPU: the extended-precision reference of the ODE models' stage derivatives
(tests/helpers/stage_derivs_ref.py) against the existing oracles (complex steps and central differences
in float64), against 50-digit finite differences in mpmath, and the float64-vs-long-double yardstick
E64 in which tests/test_gpu_stage_derivs.py measures the device.
"""
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stage_derivs_ref as sd  # noqa: E402

EPS = 2.0 ** -52
needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="long double is not the x87 80-bit format")

# (model, steer, M): every M of the GPU cases
ORACLE_CASES = [("kin_bicycle", "bicycle", 1), ("kin_bicycle", "bicycle", 3), ("cartpole", "bicycle", 1),
                ("cartpole", "bicycle", 2), ("dyn_bicycle", "bicycle", 1), ("dyn_bicycle", "bicycle", 4),
                ("dyn_bicycle", "bicycle", 5), ("path_bicycle", "bicycle", 1), ("path_bicycle", "as_written", 1),
                ("path_bicycle", "bicycle", 2)]


def _oracle(model, steer, M):
    T, _, Q, R, par = sd.constants(model, steer)
    nx, nu = sd.NXU[model]
    ocp = types.SimpleNamespace(model=model, N=1, T=T, M=M, Q=Q, R=R, par=par, param="x0_stageref",
                                u_lb=(-1.0,) * nu, u_ub=(1.0,) * nu, x_lb=(-np.inf,) * nx, x_ub=(np.inf,) * nx)
    if model == "path_bicycle":
        from path_bicycle_ref import PathProblem

        return PathProblem(ocp)
    from oracle import ode_ref

    return ode_ref.Problem(ocp)


def _rel(got, ref):
    """Worst over the points of max |got - ref| / max |ref| of each point's block."""
    ref = np.asarray(ref, np.longdouble).reshape(len(ref), -1)
    got = np.asarray(got, np.longdouble).reshape(ref.shape)
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)))


@needs_longdouble
@pytest.mark.parametrize("model,steer,M", ORACLE_CASES)
def test_first_derivatives_match_complex_step(model, steer, M):
    """A, B against the oracles' complex-step Jacobians (oracle/ode_ref.py Problem.jac,
    helpers/path_bicycle_ref.py PathProblem.jac), grad q against PathProblem.grad_l (complex step)
    or 2 W (z - zr), F and q against the oracles' values, at the 256 points of the GPU test.

    A complex step is the same map evaluated once in float64 (complex) arithmetic: "exact to
    rounding", and the rounding of a float64 evaluation of this map is what E64 measures.  So the
    bound is the GPU test's: max(16 E64, 4 * 2^-52) per block.  Measured: the oracles differ from the
    reference by 0.04 to 0.11 of that bound in every block of the ten cases, i.e. by E64 itself
    (3.5e-16 in xf, up to 1.1e-15 in A of the 6-state bicycle at M = 4, 1.6e-14 at M = 1): their
    float64 evaluation and the reference's float64 run round alike."""
    pr = _oracle(model, steer, M)
    Z, lam, zr = sd.points(model)
    ref = sd.reference(model, M, steer, 1.0, 1)
    E = sd.yardstick(model, M, steer, 1.0, 1)
    nx = sd.NXU[model][0]
    if model == "path_bicycle":
        xf, q, J, g = pr.F(Z, zr), pr.l(Z, zr), pr.jac(Z, zr), pr.grad_l(Z, zr)
    else:
        xf, q, J = pr.F(Z[:, :nx], Z[:, nx:]), pr.l(Z, zr), pr.jac(Z)
        g = 2 * pr.W * (Z - zr)
    got = {"xf": xf, "q": q, "A": J[:, :, :nx], "B": J[:, :, nx:], "g": g}
    err = sd.block_errors(got, ref, blocks=tuple(got))
    for name, e in err.items():
        tol = max(16 * E[name], 4 * EPS)
        print(f"{model} {steer} M={M} {name}: oracle - reference {e:.2e}, E64 {E[name]:.2e}, bound {tol:.2e} ({e / tol:.2f})")
        assert e <= tol, name


@needs_longdouble
@pytest.mark.parametrize("model,M", [(m, M) for m, s, M in ORACLE_CASES if m != "path_bicycle"])
def test_hessian_matches_central_differences(model, M):
    """The Hessian of lam^T F (the reference at fs = 0: no cost part) against oracle/ode_ref.py
    Problem.hess_lam: central differences, step d = 1e-5, of complex-step gradients.

    The oracle's documented accuracy is its step's truncation plus the gradients' rounding over d.
    Both are taken from the oracle itself, per point, in absolute terms:
    * truncation: c d^2, so hess_lam(2 d) - hess_lam(d) = 3 c d^2; admitted 2 x a third of that
      difference's largest entry (the factor 2 for the next order and for taking one norm);
    * rounding: a complex-step gradient lam^T J is good to the rounding of J, which the first test
      bounds by 16 max(E64, 4 * 2^-52) of the point's largest |J|, times sum |lam_r|, over d.
    Measured, relative to each point's largest entry (and the worst ratio of a point's error to its
    bound): kinematic bicycle 3.5e-9 (0.44), cart-pole 3.9e-9 (0.30), 6-state bicycle M = 4 1.0e-9
    (0.29), M = 5 5.4e-10 (0.01), M = 1 1.2e-6 (0.50; one RK4 substep of 0.05 s is outside the
    stability region at vx = 2.5, so the higher derivatives the truncation carries are large)."""
    pr = _oracle(model, "bicycle", M)
    Z, lam, _ = sd.points(model)
    nz = Z.shape[1]
    ref = sd.reference(model, M, "bicycle", 0.0, 1)
    E = sd.yardstick(model, M, "bicycle", 1.0, 1)  # A, B do not depend on fs
    d = 1e-5
    pack = lambda H: np.stack([H[:, i, j] for i in range(nz) for j in range(i, nz)], axis=1)  # noqa: E731 (symix order)
    H1, H2 = pack(pr.hess_lam(Z, lam, delta=d)), pack(pr.hess_lam(Z, lam, delta=2 * d))
    trunc = np.max(np.abs(H2 - H1), axis=1) / 3
    Jmax = np.maximum(np.abs(ref["A"]).max(axis=(1, 2)), np.abs(ref["B"]).max(axis=(1, 2))).astype(np.float64)
    rnd = 16 * max(E["A"], E["B"], 4 * EPS) * Jmax * np.abs(lam).sum(axis=1) / d
    err = np.max(np.abs(H1 - ref["H"]), axis=1).astype(np.float64)
    ratio = float(np.max(err / (2 * trunc + rnd)))
    print(f"{model} M={M}: hess_lam - reference {_rel(H1, ref['H']):.2e}, worst error / bound {ratio:.2f}")
    assert ratio <= 1.0


MP_BOUND = {"kin_bicycle": 8 * 5.42e-20, "dyn_bicycle": 8 * 3.01e-19, "cartpole": 8 * 1.06e-19, "path_bicycle": 8 * 1.08e-19}


@needs_longdouble
@pytest.mark.parametrize("model,steer,M", [("kin_bicycle", "bicycle", 1), ("dyn_bicycle", "bicycle", 4),
                                           ("cartpole", "bicycle", 1), ("path_bicycle", "bicycle", 1),
                                           ("path_bicycle", "as_written", 2)])
def test_hyper_dual_algebra_matches_mpmath(model, steer, M):
    """The long-double hyper-dual run against central differences in 50-digit arithmetic of the same
    model functions, at 3 points per model, fs = 0.37: second differences of lam^T F + fs q for H,
    first differences of F and fs q for A, B and g.  The differences share the model's equations with
    the reference but none of the hyper-dual algebra, the seeding or the packing.

    Step 1e-13: truncation h^2 / 12 * (fourth derivative) ~ 1e-27 * (ratio <= 1e2), rounding
    4e-50 |Phi| / h^2 ~ 4e-24 |Phi|: both far below the long double's 2^-64 = 5.4e-20.

    Measured, relative to each point's largest entry of the block (H / A, B / g): kinematic bicycle
    7.0e-21 / 5.4e-20 / 7.9e-21, 6-state bicycle 3.0e-19 / 1.8e-19 / 0, cart-pole 5.1e-20 / 1.1e-19 /
    8.4e-20, path-frame bicycle 6.8e-20 / 1.1e-19 / 3.5e-20 (as written, M = 2: 6.2e-20 / 5.4e-20 /
    3.5e-20) -- one or two units of the long double's last place.  Asserted at 8 x each model's
    largest of the three (MP_BOUND)."""
    mp = pytest.importorskip("mpmath")
    T, _, Q, R, par = sd.constants(model, steer)
    nx, nu = sd.NXU[model]
    nz = nx + nu
    Z, lam, zr = (a[:3] for a in sd.points(model))
    fs = 0.37
    ref = sd.stage_derivs(model, Z, lam, zr, fs, T, M, Q, R, par)
    with mp.workdps(50):
        f = lambda v: mp.mpf(float(v))  # noqa: E731 (a float64 is an exact mpf)
        mpar, W, h = [f(p) for p in par], [f(w) for w in Q + R], mp.mpf(10) ** -13
        ld = lambda v: np.longdouble(mp.nstr(v, 30))  # noqa: E731
        worst = {"H": 0.0, "AB": 0.0, "g": 0.0}
        for p in range(3):
            z0, row, lm = [f(v) for v in Z[p]], [f(v) for v in zr[p]], [f(v) for v in lam[p]]

            def at(*steps):
                z = list(z0)
                for i, s in steps:
                    z[i] = z[i] + s * h
                return sd.interval(model, z, row, mpar, f(T), M), f(fs) * sd.stage_cost(model, z, row, W, mpar)

            def phi(*steps):
                xf, q = at(*steps)
                return q + sum(l * x for l, x in zip(lm, xf))

            H = np.zeros(nz * (nz + 1) // 2, np.longdouble)
            J = np.zeros((nx, nz), np.longdouble)
            g = np.zeros(nz, np.longdouble)
            p0 = phi()
            for i in range(nz):
                (xp, qp), (xm, qm) = at((i, 1)), at((i, -1))
                g[i] = ld((qp - qm) / (2 * h))
                for r in range(nx):
                    J[r, i] = ld((xp[r] - xm[r]) / (2 * h))
                H[sd.symix(i, i, nz)] = ld((phi((i, 1)) - 2 * p0 + phi((i, -1))) / (h * h))
                for j in range(i + 1, nz):
                    d2 = phi((i, 1), (j, 1)) - phi((i, 1), (j, -1)) - phi((i, -1), (j, 1)) + phi((i, -1), (j, -1))
                    H[sd.symix(i, j, nz)] = ld(d2 / (4 * h * h))
            Jr = np.concatenate([ref["A"][p], ref["B"][p]], axis=1)
            worst["H"] = max(worst["H"], _rel(ref["H"][p][None], H[None]))
            worst["AB"] = max(worst["AB"], _rel(Jr[None], J[None]))
            worst["g"] = max(worst["g"], _rel(ref["g"][p][None], g[None]))
    print(f"{model} {steer} M={M}: long double - mpmath H {worst['H']:.2e}, A/B {worst['AB']:.2e}, g {worst['g']:.2e}")
    assert max(worst.values()) <= MP_BOUND[model]


@needs_longdouble
def test_float64_yardstick_of_every_gpu_case():
    """E64 of every case of tests/test_gpu_stage_derivs.py: the reference's own algorithm in float64
    against its long-double run, per block, relative to each point's largest entry of the block.
    Printed (pytest -s) as the table the GPU test's docstring records.  The GPU test admits
    16 E64; that a wrong term cannot hide there needs 16 E64 far below 1e-3, asserted here as
    16 E64 <= 1e-9.  Worst per block over the cases with a stable step: xf 3.5e-16, q 4.7e-16,
    A 6.2e-16, B 4.9e-16, g 3.5e-16, H 2.6e-15 (cart-pole); the 6-state bicycle with one substep
    (M = 1, outside RK4's stability region at small vx) has xf 8.2e-15, A 1.5e-14, B 1.6e-14, H 2.3e-14."""
    seen = {}
    for (cid, model, M, _cache, _which, steer), fs, lay, _k, _id in sd.grid():
        key = (model, M, steer, fs, lay)
        if key not in seen:
            seen[key] = sd.yardstick(*key)
            print(f"E64 {model:12s} {steer:10s} M={M} fs={fs} layout={lay}: "
                  + " ".join(f"{b} {seen[key][b]:.1e}" for b in sd.BLOCKS))
    assert len(seen) == 34
    for key, E in seen.items():
        for b, e in E.items():
            assert np.isfinite(e) and 16 * e <= 1e-9, (key, b, e)
