"""GPU tests of the sensitivities of the MPC solution to the model (mpcx_sens_model[_vjp][_dev], mpcx_set_par,
mpcx_model_dims, Solver.sens_model / sens_model_vjp / set_par, DeviceLoop.sens_model / sens_model_vjp, mpcx.autograd
with par=; csrc/sens.h sens_mdl_kernel, sens_mdl_vjp_kernel).

References: tests/helpers/sens_model_ref.py -- the kernels' two rounds restated in long double from the GPU's own
point, the tangent by hyper-dual numbers over np.longdouble with the constants seeded (closed form for the linear
tables) -- central differences of the solver itself through set_par for the ODE models, and the project's forward mode
for the reverse one through the dot-product identity <g, dw> = sum_k <gThk_k, dTh_k>.  Cases are those of
tests/test_gpu_sens.py (their constructors and cached solves are imported)."""
import ctypes
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_model_ref as sm  # noqa: E402
import sens_nonlinear_ref as sn  # noqa: E402
import sens_ref as sr  # noqa: E402
from test_gpu_sens import LINEAR_CASES, NONLINEAR_CASES, REF_OPTS, linear_case, linear_problem, nonlinear_problem  # noqa: E402

LD = np.longdouble
ODE_CASES = tuple(n for n in NONLINEAR_CASES if not n.startswith("unicycle"))
ALL_CASES = LINEAR_CASES + ODE_CASES


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def point_of(r, rows=slice(None)):
    return {k: r[k][rows] for k in ("w", "lam_g", "lam_x")}


# ------------------------------------------------------------------------------------------
# the cases: solved once, shared, never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(ocp, P, solver, solve result, [(long-double point, float64 point)] per instance).  Linear cases: the solves of
    tests/test_gpu_sens.py; ODE cases: a solver at tol = 1e-10 (the finite differences need it)."""
    import mpcx

    if name in LINEAR_CASES:
        ocp, P, r, _, solver = linear_case(name)
        lb, ub = sr.ocp_bounds(ocp)
        pts = [tuple(sm.LinearPoint(ocp, P[b], point_of(r, b), lb, ub, b, dt) for dt in (LD, np.float64))
               for b in range(P.shape[0])]
    else:
        ocp, P, opts = nonlinear_problem(name)
        solver = mpcx.nlpsol(name + "_mdl", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
        r = solver.solve_batch(P)
        assert np.all(r["status"] <= 1), (name, r["status"])
        lb, ub = sr.ocp_bounds(ocp)
        pts = list(zip(sn.points(ocp, P, r, lb, ub, LD), sn.points(ocp, P, r, lb, ub, np.float64)))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ocp, P, solver, r, pts


def linear_split(ocp, d):
    """(dA, dB, dc) of rows (..., n_th) of a linear model in the problem's own (x, u)"""
    nx, nu = ocp.nx, ocp.nu
    return (d[..., :nx * nx].reshape(d.shape[:-1] + (nx, nx)), d[..., nx * nx:nx * nx + nx * nu].reshape(d.shape[:-1] + (nx, nu)),
            d[..., nx * nx + nx * nu:])


def forward(solver, P, r, d):
    """Solver.sens_model for rows d in the reference's layout (B, m[, N], n_th), or (B, n_th)"""
    if solver.ocp.model == "linear":
        dA, dB, dc = linear_split(solver.ocp, d)
        return solver.sens_model(P, r, dA=dA, dB=dB, dc=dc)
    return solver.sens_model(P, r, dpar=d)


def reverse(solver, P, r, g):
    """(per-stage rows (B, m, N, n_th) in the reference's layout, Solver.sens_model_vjp's result)"""
    v = solver.sens_model_vjp(P, r, g)
    if solver.ocp.model != "linear":
        return v["gpark"], v
    B, m, N = v["gAk"].shape[:3]
    return np.concatenate([v["gAk"].reshape(B, m, N, -1), v["gBk"].reshape(B, m, N, -1), v["gck"]], axis=3), v


def seeded(name, ocp, P, m=None):
    """(dth (B, m, N, n_th) per-stage directions relative to each constant's size, gw (B, m, n_w) seeded normal)"""
    B, m = P.shape[0], ocp.nx if m is None else m
    n_w = ocp.nx + (ocp.nx + ocp.nu) * ocp.N
    seed = 1300 + 10 * ALL_CASES.index(name)
    dth = np.stack([sm.relative_directions(ocp, m, seed + b) for b in range(B)])
    return dth, np.random.default_rng(seed + 7).normal(size=(B, m, n_w))


@functools.lru_cache(maxsize=None)
def measured(name):
    """Both calls of a case and their references: (dth, gw, dw, gthk, result of the reverse call, E64 forward, E64
    reverse, long-double references per instance)"""
    ocp, P, solver, r, pts = case(name)
    dth, gw = seeded(name, ocp, P)
    s = forward(solver, P, r, dth)
    gk, v = reverse(solver, P, r, gw)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0), (s["flag"], v["flag"])
    Ef = Er = 0.0
    refs = []
    for b, (pt, pt64) in enumerate(pts):
        sol = point_of(r, b)
        ef, rf, ok = sm.e64("model", pt, pt64, sol, dth[b])
        er, rr, ok2 = sm.e64("model_vjp", pt, pt64, sol, gw[b])
        assert ok and ok2, (name, b, "the reference's factors are not regular")
        Ef, Er = max(Ef, ef), max(Er, er)
        refs.append((rf, rr))
    return dth, gw, s["dw"], gk, v, Ef, Er, refs


# ------------------------------------------------------------------------------------------
# 1. every case against the long-double restatement at the same point
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_against_the_restatement(mpcx, name):
    """1. Forward and reverse kernels against the long-double reference at the GPU's own point: nx seeded per-stage
    directions (relative to each constant's size) and nx seeded cotangents; tolerance 64 x E64(case, call) relative to
    max(1, |entry|), E64 from the reference alone (its float64 pipeline against its long-double one at this point).
    The reverse call's stack is (gThk, their stage sum).  A shared row (per_stage = 0) against the same reference with
    the row repeated.  dX_0 = 0 exactly.  Linear cases: gA, gB, gc are the stages' rows summed per table through the
    schedule.  Measured on one MI355X, forward / reverse (E64 of each in parentheses): padded_dint_N8 7.0e-16
    (9.2e-16) / 6.6e-16 (1.7e-15), lin4x2_N12 5.3e-16 (1.0e-15) / 1.1e-15 (1.5e-15), cartpole_qp_N50 1.9e-14 (2.1e-14) /
    1.1e-13 (1.1e-13), ltv_N40 4.4e-15 (2.8e-15) / 3.2e-15 (3.9e-15), kin_bicycle_N10 4.7e-17 (8.6e-17) / 1.3e-16
    (2.4e-16), cartpole_N20 6.5e-15 (1.3e-14) / 1.1e-14 (2.9e-14), path_bicycle_N20 2.6e-17 (3.3e-17) / 2.1e-16
    (4.9e-16), dyn_bicycle_N10 3.4e-16 (3.4e-16) / 2.0e-16 (2.0e-16): the kernels are at the reference's own float64
    rounding."""
    ocp, P, solver, r, pts = case(name)
    dth, gw, dw, gk, v, Ef, Er, refs = measured(name)
    B, nx, N = P.shape[0], ocp.nx, ocp.N
    lin = ocp.model == "linear"
    assert dw.shape == (B, nx + (nx + ocp.nu) * N, nx) and gk.shape == dth.shape
    wf = wr = ws = 0.0
    for b in range(B):
        rf, rr = refs[b]
        n_k = gk[b].size
        wf = max(wf, sr.rel_err(np.ravel(dw[b]), rf))
        wr = max(wr, sr.rel_err(np.ravel(gk[b]), rr[:n_k]))
        if not lin:  # the kernel's own stage sum (gsum) against the reference's
            ws = max(ws, sr.rel_err(np.ravel(v["gpar"][b]), rr[n_k:]))
        assert not dw[b, :nx].any()
    # a row shared by the stages
    shared = np.ascontiguousarray(dth[:, :, 0])
    s1 = forward(solver, P, r, shared)
    we = 0.0
    for b, (pt, pt64) in enumerate(pts):
        rep = np.ascontiguousarray(np.broadcast_to(shared[b][:, None], dth[b].shape))
        e, ref, _ = sm.e64("model", pt, pt64, point_of(r, b), rep)
        we = max(we, sr.rel_err(np.ravel(s1["dw"][b]), ref) / max(e, 1e-300))
    print(f"{name}: |dw| {np.abs(dw).max():.3g}, |gThk| {np.abs(gk).max():.3g}; against the long-double reference: forward "
          f"{wf:.3e} (E64 {Ef:.2e}, bound {64 * Ef:.2e}), reverse {wr:.3e} (E64 {Er:.2e}, bound {64 * Er:.2e}), stage sum "
          f"{ws:.3e}; shared row: error / its E64 {we:.2f}")
    assert Ef <= 1e-12 and Er <= 1e-12
    assert wf <= 64.0 * Ef and wr <= 64.0 * Er and ws <= 64.0 * Er and we <= 64.0
    assert np.abs(dw).max() > 1e-3 and np.abs(gk).max() > 1e-3
    if lin:
        tab = np.asarray(ocp.tab)
        tab = np.broadcast_to(tab[None, :] if tab.ndim == 1 else tab, (B, N))
        for key, kk in (("gA", "gAk"), ("gB", "gBk"), ("gc", "gck")):
            ref = np.zeros_like(v[key])
            for b in range(B):
                for k in range(N):
                    ref[b, :, tab[b, k]] += v[kk][b, :, k]
            assert v[key].shape[:3] == (B, nx, ocp.n_tab) and np.allclose(v[key], ref, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------
# 2. reverse against forward: the dot-product identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_dot_product_identity(mpcx, name):
    """2. <g, dw> = sum_k <gThk_k, dTh_k> with dw the project's own sens_model at the same point, per-stage seeded
    directions, within 64 E64(forward) sum |g| max(1, |dw|) + 64 E64(reverse) sum max(1, |gThk|) |dTh| (the form of
    tests/test_gpu_sens_weights.py's identity_gap with this case's yardsticks).  Pins the sign and the costate
    convention: lam~_{k+1} pairs with stage k's defect.  Measured on one MI355X, worst gap / bound: 5.2e-7
    (dyn_bicycle_N10) to 1.5e-3 (kin_bicycle_N10)."""
    dth, gw, dw, gk, _, Ef, Er, _ = measured(name)
    lhs = np.einsum("bci,bij->bcj", gw, dw)
    rhs = np.einsum("bckn,bjkn->bcj", gk, dth)
    big = lambda a: np.maximum(1.0, np.abs(a))  # noqa: E731
    bound = (64.0 * Ef * np.einsum("bci,bij->bcj", np.abs(gw), big(dw))
             + 64.0 * Er * np.einsum("bckn,bjkn->bcj", big(gk), np.abs(dth)))
    gap = np.abs(lhs - rhs)
    print(f"{name}: worst identity gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)


# ------------------------------------------------------------------------------------------
# 3. ODE models against central differences of the solver itself through set_par
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ODE_CASES)
def test_against_finite_differences(mpcx, name):
    """3. dw against central differences of solves after set_par(par +- h dpar), warm-started from the nominal
    solution, at h = 1e-3 and 1e-4 with the directions relative to each constant: column 0 dpar = par xi with xi
    seeded normal, column 1 the first constant alone.  Solver at tol = 1e-10.  Tolerance 4 x the spread of the two
    estimates + 1e-6 against their mean; every instance kept has spread <= 1e-3 max(1, max|dw|); the seeded column
    moves by more than 1e-3.  An instance whose active set changes under +- h is left out, at most one per case
    (printed).  Measured on one MI355X, worst instance of each case (spread, |GPU - FD|): kin_bicycle_N10 1.5e-7,
    7.5e-8; cartpole_N20 9.8e-6, 5.0e-6 (|dw| 31); path_bicycle_N20 1.1e-7, 5.6e-8; dyn_bicycle_N10 2.2e-7, 1.1e-7.  No
    instance is left out."""
    ocp, P, solver, nom, _ = case(name)
    B, nx, n_th = P.shape[0], ocp.nx, sm.n_th_of(ocp)
    par = np.array(ocp.par, float)[:n_th]
    rng = np.random.default_rng(1400 + ODE_CASES.index(name))
    dpar = np.stack([par * rng.normal(size=n_th), par * (np.arange(n_th) == 0)])
    s = solver.sens_model(P, nom, dpar=np.tile(dpar, (B, 1, 1)))
    assert np.all(s["flag"] == 0), s["flag"]
    lb, ub = sr.ocp_bounds(ocp)
    act0, same = [], np.ones(B, bool)
    for b in range(B):
        a, ok = sr.classify(nom["w"][b], nom["lam_x"][b], lb, ub, nx)
        assert ok, (name, b, "the nominal solution is not strictly complementary")
        act0.append(a)
    fd = {}
    try:
        for h in (1e-3, 1e-4):
            d = np.zeros((B, nom["w"].shape[1], 2))
            for j in range(2):
                side = []
                for sgn in (1.0, -1.0):
                    solver.set_par(par + sgn * h * dpar[j])
                    r = solver.solve_batch(P, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                    for b in range(B):
                        a, ok = sr.classify(r["w"][b], r["lam_x"][b], lb, ub, nx)
                        same[b] &= bool(r["status"][b] <= 1 and ok and np.array_equal(a, act0[b]))
                    side.append(r["w"])
                d[:, :, j] = (side[0] - side[1]) / (2 * h)
            fd[h] = d
    finally:
        solver.set_par(par)
    print(f"{name}: instances left out (active set changes): {np.flatnonzero(~same)}")
    assert np.count_nonzero(~same) <= 1, (name, np.flatnonzero(~same))
    top_seeded = 0.0
    for b in np.flatnonzero(same):
        spread = float(np.max(np.abs(fd[1e-3][b] - fd[1e-4][b])))
        err = float(np.max(np.abs(s["dw"][b] - 0.5 * (fd[1e-3][b] + fd[1e-4][b]))))
        top = float(np.max(np.abs(s["dw"][b])))
        print(f"{name} b={b}: {int(act0[b].sum())} active, FD spread {spread:.3e}, |GPU - FD| {err:.3e}, |dw| {top:.3g} "
              f"(seeded column {np.max(np.abs(s['dw'][b, :, 0])):.3g})")
        assert spread <= 1e-3 * max(1.0, top), (name, b, "the yardstick itself is too wide")
        assert err <= 4.0 * spread + 1e-6, (name, b)
        top_seeded = max(top_seeded, float(np.max(np.abs(s["dw"][b, :, 0]))))
    assert top_seeded > 1e-3, (name, "the seeded direction must move the solution")


# ------------------------------------------------------------------------------------------
# 4. exactness and independence
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40", "kin_bicycle_N10", "path_bicycle_N20", "dyn_bicycle_N10"])
def test_exact_properties(mpcx, name):
    """4. Zero directions / cotangents give exact zeros; column c of an (nx + 1)-column call (two launches) = that
    column alone; an instance alone (B = 1) = inside its batch; a stage-uniform direction passed per stage gives the
    bits of the shared row."""
    ocp, P, solver, r, _ = case(name)
    lin = ocp.model == "linear"
    B, n_w = r["w"].shape
    nx, N, n_th = ocp.nx, ocp.N, sm.n_th_of(ocp)
    m = nx + 1
    d = np.ascontiguousarray(seeded(name, ocp, P, m)[0][:, :, 0])  # (B, m, n_th): shared rows
    g = np.random.default_rng(44).normal(size=(B, m, n_w))
    keys = ("gAk", "gBk", "gck", "gA", "gB", "gc") if lin else ("gpark", "gpar")
    s, v = forward(solver, P, r, d), solver.sens_model_vjp(P, r, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    assert s["dw"].shape == (B, n_w, m) and not s["dw"][:, :nx].any()
    assert all(np.all(np.isfinite(v[k])) for k in keys)
    assert np.all(forward(solver, P, r, np.zeros((B, 2, n_th)))["dw"] == 0.0)
    vz = solver.sens_model_vjp(P, r, np.zeros((B, 2, n_w)))
    assert all(np.all(vz[k] == 0.0) for k in keys)
    per_stage = np.ascontiguousarray(np.broadcast_to(d[:, :, None, :], (B, m, N, n_th)))
    assert bits(forward(solver, P, r, per_stage)["dw"]) == bits(s["dw"])
    first = forward(solver, P, r, d[:, :nx]), solver.sens_model_vjp(P, r, g[:, :nx])
    assert bits(first[0]["dw"]) == bits(s["dw"][:, :, :nx])
    assert all(bits(first[1][k]) == bits(v[k][:, :nx]) for k in keys)
    for c in range(m):
        one = forward(solver, P, r, d[:, c])  # a single direction
        assert one["dw"].shape == (B, n_w, 1) and bits(one["dw"][:, :, 0]) == bits(s["dw"][:, :, c]), c
        one = solver.sens_model_vjp(P, r, g[:, c])
        assert all(bits(one[k][:, 0]) == bits(v[k][:, c]) for k in keys), c
    # (a schedule per instance, ltv_N40: a batch of one reads the first row, so instance 0 is the one alone)
    for b in [0] if (lin and np.asarray(ocp.tab).ndim == 2) else range(B):
        pt = point_of(r, slice(b, b + 1))
        solo = forward(solver, P[b:b + 1], pt, d[b:b + 1, :nx])
        assert bits(solo["dw"][0]) == bits(first[0]["dw"][b]) and solo["flag"][0] == 0, b
        solo = solver.sens_model_vjp(P[b:b + 1], pt, g[b:b + 1, :nx])
        assert all(bits(solo[k][0]) == bits(first[1][k][b]) for k in keys), b
    with pytest.raises(ValueError):
        solver.sens_model(P, r)
    with pytest.raises(ValueError):
        solver.sens_model(P, r, dpar=np.zeros((B, n_th)), dA=np.zeros((B, nx, nx)))
    with pytest.raises(ValueError):
        solver.sens_model_vjp(P, r, np.zeros((B, 2, n_w + 1)))


# ------------------------------------------------------------------------------------------
# 5. set_par
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kin_bicycle_N10", "path_bicycle_N20"])
def test_set_par_equals_a_new_handle(mpcx, name):
    """5. A solve and both sensitivity calls after set_par(par') equal, bit for bit, the same on a solver created with
    par'; a refused call (NaN, inf, the path-frame bicycle's L = 0) leaves the constants as they were."""
    ocp, P, opts = nonlinear_problem(name)
    n_th = sm.n_th_of(ocp)
    par2 = tuple(float(v) for v in np.array(ocp.par, float) * (1.0 + 0.07 * np.arange(1, n_th + 1)))
    a = mpcx.nlpsol(name + "_sp_a", "mi355x", ocp, {"ipopt": opts})
    b = mpcx.nlpsol(name + "_sp_b", "mi355x", dataclasses.replace(ocp, par=par2), {"ipopt": opts})
    assert a._h.model_dims() == n_th
    before = a.solve_batch(P)
    a.set_par(par2)
    assert tuple(a.ocp.par) == par2
    for bad in ((float("nan"),) + par2[1:], (float("inf"),) + par2[1:]):
        with pytest.raises(mpcx._lib.MpcxError, match="finite"):
            a.set_par(bad)
    if name == "path_bicycle_N20":
        for L in (0.0, -1.0):
            with pytest.raises(mpcx._lib.MpcxError, match="must be > 0"):
                a.set_par((L,) + par2[1:])
    with pytest.raises(ValueError):
        a.set_par(par2 + (1.0,))
    assert tuple(a.ocp.par) == par2 and tuple(a._h.spec.par)[:n_th] == par2
    ra, rb = a.solve_batch(P), b.solve_batch(P)
    assert np.all(rb["status"] <= 1)
    for k in ("w", "lam_g", "lam_x", "f", "iters", "status"):
        assert bits(ra[k]) == bits(rb[k]), k
    assert bits(ra["w"]) != bits(before["w"])
    g = np.random.default_rng(7).normal(size=(P.shape[0], 2, ra["w"].shape[1]))
    d = np.random.default_rng(8).normal(size=(P.shape[0], 2, n_th)) * np.array(par2)
    assert bits(a.sens_model(P, ra, dpar=d)["dw"]) == bits(b.sens_model(P, rb, dpar=d)["dw"])
    va, vb = a.sens_model_vjp(P, ra, g), b.sens_model_vjp(P, rb, g)
    assert all(bits(va[k]) == bits(vb[k]) for k in ("gpar", "gpark"))


def test_set_par_refuses_linear_and_unicycle(mpcx):
    lib = mpcx._lib.load()
    buf = np.ones(8)
    lin, P, r, _, solver = linear_case("lin4x2_N12")
    with pytest.raises(ValueError):
        solver.set_par(np.ones(3))
    assert lib.mpcx_set_par(solver._h.ptr, mpcx._lib.dptr(buf)) == -1 and "tables" in lib.mpcx_last_error().decode()
    assert bits(solver.solve_batch(P)["w"]) == bits(r["w"])
    n = ctypes.c_int32()
    assert lib.mpcx_model_dims(solver._h.ptr, ctypes.byref(n)) == 0 and n.value == 16 + 8 + 4  # LinearModel<4,2>
    uni = mpcx.nlpsol("uni_sp", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    with pytest.raises(ValueError):
        uni.set_par(())
    assert lib.mpcx_set_par(uni._h.ptr, mpcx._lib.dptr(buf)) == -1 and "no model constants" in lib.mpcx_last_error().decode()
    assert lib.mpcx_model_dims(uni._h.ptr, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.mpcx_set_par(None, None) == -1 and lib.mpcx_set_par(uni._h.ptr, None) == -1
    assert lib.mpcx_model_dims(None, None) == -1


# ------------------------------------------------------------------------------------------
# 6. the device loop
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole_N20", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """6. DeviceLoop.sens_model / sens_model_vjp after solve() against the host calls on the loop's tensors copied
    back, bit for bit; every entry of preallocated outputs is written (pre-filled with 7); the point= override on a
    saved copy gives the same bits after the loop has moved on."""
    import torch
    from mpcx.device import DeviceLoop

    lin = name in LINEAR_CASES
    if lin:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name + "_ml", "mi355x", ocp, {"ipopt": {"max_iter": 300}})
    else:
        ocp, P, opts = nonlinear_problem(name)
        solver = mpcx.nlpsol(name + "_ml", "mi355x", ocp, {"ipopt": opts})
    pd = solver._pad
    B, m, N = P.shape[0], ocp.nx, ocp.N
    d, g = seeded(name, ocp, P)
    loop = DeviceLoop(solver, P, device="cuda:0")
    n_th = solver._h.model_dims()
    dk, gk_in = d, g
    if pd is not None:  # the kernel's padded layout
        dk = solver._model_rows(B, None, *linear_split(ocp, d))
        gk_in = pd.scatter(g.reshape(B * m, -1), pd.w_idx, pd.n_w_pad).reshape(B, m, -1)
    assert dk.shape == (B, m, N, n_th)
    d_d, d_g = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (dk, gk_in))
    loop.solve()
    nwk = loop.w.shape[1]
    full = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda:0")  # noqa: E731
    gk_out, gs_out, dw_out = full(B, m, N, n_th), full(B, m, n_th), full(B, nwk, m)
    dw, flag = loop.sens_model(d_d, dw_out=dw_out)
    gk, gs, vflag = loop.sens_model_vjp(d_g, gThk_out=gk_out, gTh_out=gs_out)
    none_k, gs_only, _ = loop.sens_model_vjp(d_g, per_stage=False)
    uni = loop.sens_model(d_d[:, :, 0].contiguous())[0], loop.sens_model(d_d[:, :, :1].expand(B, m, N, n_th).contiguous())[0]
    saved = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    torch.cuda.synchronize()
    assert dw is dw_out and gk is gk_out and gs is gs_out and none_k is None
    assert not bool((dw == 7.0).any()) and not bool((gk == 7.0).any()) and not bool((gs == 7.0).any())
    assert bits(gs_only.cpu().numpy()) == bits(gs.cpu().numpy())
    assert bits(uni[0].cpu().numpy()) == bits(uni[1].cpu().numpy())
    host = {k_: t.cpu().numpy() for k_, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
    dw_np, gk_np, gs_np = dw.cpu().numpy(), gk.cpu().numpy(), gs.cpu().numpy()
    if pd is not None:
        host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                "lam_x": host["lam_x"][:, pd.w_idx]}
        dw_np = dw_np[:, pd.w_idx]
    s = forward(solver, host["P"], host, d)
    hk, v = reverse(solver, host["P"], host, g)
    if lin:
        knx, nu, nx = solver._model_dims()[0], ocp.nu, ocp.nx
        gA = gk_np[..., :knx * knx].reshape(B, m, N, knx, knx)[..., :nx, :nx]
        gB = gk_np[..., knx * knx:knx * knx + knx * nu].reshape(B, m, N, knx, nu)[..., :nx, :]
        gc = gk_np[..., knx * knx + knx * nu:][..., :nx]
        assert bits(gA) == bits(v["gAk"]) and bits(gB) == bits(v["gBk"]) and bits(gc) == bits(v["gck"])
    else:
        assert bits(gk_np) == bits(hk) and bits(gs_np) == bits(v["gpar"])
    assert np.all(s["flag"] == 0) and bits(flag.cpu().numpy()) == bits(s["flag"]) == bits(vflag.cpu().numpy())
    assert bits(dw_np) == bits(s["dw"])
    loop.step()  # the resident point moves on
    loop.solve()
    again = loop.sens_model(d_d, point=saved)[0], loop.sens_model_vjp(d_g, point=saved)[0]
    moved = loop.sens_model(d_d)[0]
    torch.cuda.synchronize()
    assert bits(again[0].cpu().numpy()) == bits(dw.cpu().numpy()) and bits(again[1].cpu().numpy()) == bits(gk.cpu().numpy())
    assert bits(moved.cpu().numpy()) != bits(dw.cpu().numpy())
    with pytest.raises(ValueError):
        loop.sens_model_vjp(d_g, gTh_out=gs_out[:, :1])
    with pytest.raises(ValueError):
        loop.sens_model(torch.zeros((B, loop._knx + 1, n_th), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        loop.sens_model(d_d[..., :-1].contiguous())


# ------------------------------------------------------------------------------------------
# 7. irregular instances: ordinary statuses, nothing faults
# ------------------------------------------------------------------------------------------
def assert_only_irregular(s, v, bad, regular=None):
    keys = ("gAk", "gBk", "gck", "gA", "gB", "gc")
    for b in range(s["flag"].shape[0]):
        if b == bad:
            assert s["flag"][b] == 1 and v["flag"][b] == 1
            assert np.all(np.isnan(s["dw"][b])) and all(np.all(np.isnan(v[k][b])) for k in keys)
        else:
            assert s["flag"][b] == 0 and v["flag"][b] == 0
            assert np.all(np.isfinite(s["dw"][b])) and all(np.all(np.isfinite(v[k][b])) for k in keys)
            if regular is not None:  # the neighbours keep their bits
                assert bits(s["dw"][b]) == bits(regular[0]["dw"][b]), b
                assert bits(v["gAk"][b]) == bits(regular[1]["gAk"][b]), b


def test_variable_on_its_bound_is_flagged(mpcx):
    """7. U_3 of instance 2 placed on its upper bound (tests/test_gpu_sens_weights.py's case)"""
    lin, P, solver, r, _ = case("padded_dint_N8")
    dth, gw = seeded("padded_dint_N8", lin, P)
    good = forward(solver, P, r, dth), solver.sens_model_vjp(P, r, gw)
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0
    pt = {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}
    assert_only_irregular(forward(solver, P, pt, dth), solver.sens_model_vjp(P, pt, gw), 2, good)


def test_indefinite_stage_is_flagged(mpcx):
    """7. A negative input weight on the last stage of instance 1 of 3 (tests/test_gpu_sens_weights.py's case)."""
    from mpcx import lti

    rng = np.random.default_rng(11)
    nx, nu, N, B = 4, 1, 20, 3
    A = np.eye(nx) + 0.05 * rng.normal(size=(nx, nx))
    Bm = rng.normal(size=(nx, nu)) + 1.0
    W = np.zeros((2, nx + nu, nx + nu))
    W[:, :nx, :nx] = 5.0 * np.eye(nx)
    W[0, nx, nx] = 0.5
    W[1, nx, nx] = -0.05
    tab = np.zeros((B, N), np.int32)
    tab[1, -1] = 1
    lin = lti.LinearOCP(N=N, A=np.stack([A, A]), B=np.stack([Bm, Bm]), W=W, tab=tab, u_lb=(-1.0,), u_ub=(1.0,))
    solver = mpcx.nlpsol("indef_mdl", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    d, g = rng.normal(size=(B, 2, nx * nx + nx * nu + nx)), rng.normal(size=(B, 2, lin.n_w_ms))
    assert_only_irregular(forward(solver, P, point, d), solver.sens_model_vjp(P, point, g), 1)


# ------------------------------------------------------------------------------------------
# 8. refusals: MPCX_EINVAL with a message, nothing launched
# ------------------------------------------------------------------------------------------
def test_refusals(mpcx):
    """8. m = 0 and m = nx + 1, N = 64, the unicycle (n_th = 0), null pointers, B < 1, a null handle, on all four
    entry points; both outputs of the reverse mode null."""
    import torch
    from mpcx import _lib, ode

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, vjp, B=2, m=1, n_null=()):
        h = solver._h
        n, mm, N = max(B, 1), max(m, 1), solver.ocp.N
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w)),
               np.zeros((n, mm, max(h.n_w, N * 8))), np.full((n, mm, N, 8), 7.0), np.full((n, h.n_w, mm), 7.0)]
        a = [None if i in n_null else _lib.dptr(x) for i, x in enumerate(arr)]
        if vjp:  # gw = arr[4]; gThk = arr[5]; gTh = arr[6] (larger than needed)
            rc = lib.mpcx_sens_model_vjp(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], m, a[5], a[6], None)
        else:  # dTh = arr[4] (per stage); dw = arr[6]
            rc = lib.mpcx_sens_model(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], 1, m, a[6], None)
        assert rc != 0 and np.all(arr[5] == 7.0) and np.all(arr[6] == 7.0)
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok_mdl", "mi355x", ode.kinematic_bicycle_tracking(N=10), {"ipopt": {"max_iter": 500}})
    long = mpcx.nlpsol("n64_mdl", "mi355x", ode.kinematic_bicycle_tracking(N=64), {"ipopt": {"max_iter": 500}})
    uni = mpcx.nlpsol("uni_mdl", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    buf = torch.zeros(2 * long._h.n_w * 4, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, vjp, B=2, m=1, lam_g=p, a=p, b=p, c=p):
        if vjp:
            rc = lib.mpcx_sens_model_vjp_dev(h.ptr if h else None, B, p, p, lam_g, p, a, m, b, c, None, None)
        else:
            rc = lib.mpcx_sens_model_dev(h.ptr if h else None, B, p, p, lam_g, p, a, 1, m, b, None, None)
        return rc, lib.mpcx_last_error().decode()

    for vjp in (False, True):
        who = "sens_model_vjp" if vjp else "sens_model:"
        for call, ok, n64, un in ((host_call, solver, long, uni), (dev_call, solver._h, long._h, uni._h)):
            for m in (0, 4):
                rc, msg = call(ok, vjp, m=m)
                assert rc == EINVAL and "between 1 and nx" in msg and who in msg, (m, msg)
            for B in (0, -3):
                rc, msg = call(ok, vjp, B=B)
                assert rc == EINVAL and "B must be >= 1" in msg
            rc, msg = call(n64, vjp)
            assert rc == EINVAL and "N >= 64" in msg
            rc, msg = call(un, vjp)
            assert rc == EINVAL and "n_th = 0" in msg and who in msg
        for i in (0, 1, 2, 3, 4) + (() if vjp else (6,)):  # P, w, lam_g, lam_x, the directions / cotangents, dw
            rc, msg = host_call(solver, vjp, n_null=(i,))
            assert rc == EINVAL and "required" in msg, i
        if vjp:  # one of the two outputs is enough, none is refused
            rc, msg = host_call(solver, True, n_null=(5, 6))
            assert rc == EINVAL and "required" in msg
            rc, msg = dev_call(solver._h, True, b=None, c=None)
            assert rc == EINVAL and "required" in msg
        for kw in ({"lam_g": None}, {"a": None}) + (() if vjp else ({"b": None},)):
            rc, msg = dev_call(solver._h, vjp, **kw)
            assert rc == EINVAL and "required" in msg, kw
        rc, msg = dev_call(None, vjp)
        assert rc == EINVAL and "null handle" in msg
    with pytest.raises(ValueError):
        uni.sens_model(np.zeros((1, 6)), {}, dpar=np.zeros((1, 1)))
    with pytest.raises(ValueError):
        uni.sens_model_vjp(np.zeros((1, 6)), {}, np.zeros((1, 53)))
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched


# ------------------------------------------------------------------------------------------
# 9. autograd
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kin_bicycle_N10", "path_bicycle_N20"])
def test_autograd_par(mpcx, name):
    """9. solve_differentiable(loop, P, par=): par.grad of an imitation loss on U_0 against central differences of the
    loss through set_par (h = 1e-3 and 1e-4 relative to each constant, solver at tol = 1e-10; tolerance 4 x spread +
    1e-6 against the mean, spread <= 1e-3 max(1, |gradient|_max)).  The kinematic bicycle with P requiring a gradient
    too; the path-frame bicycle, which has no sens_vjp, with par.grad alone.  The backward differentiates at the
    forward's constants also after set_par has changed the solver's, and puts the changed ones back."""
    import torch
    from mpcx.autograd import MPCParFunction, solve_differentiable
    from mpcx.device import DeviceLoop

    ocp, P0, opts = nonlinear_problem(name)
    solver = mpcx.nlpsol(name + "_ag_p", "mi355x", ocp, {"ipopt": dict(opts, tol=1e-10)})
    B, nx, nu, n_th = P0.shape[0], ocp.nx, ocp.nu, sm.n_th_of(ocp)
    par0 = np.array(ocp.par, float)[:n_th]
    with_P = name == "kin_bicycle_N10"
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device="cuda:0", requires_grad=grad)  # noqa: E731
    u_np = np.random.default_rng(19).uniform(-0.5, 0.5, (B, nu)) * np.array(ocp.u_ub)
    u_t = t64(u_np)
    loss_np = lambda w: 0.5 * float(np.sum((w[:, nx:nx + nu] - u_np) ** 2))  # noqa: E731
    grads = []
    for change in (False, True):
        loop = DeviceLoop(solver, P0, device="cuda:0")
        P, par = t64(P0, with_P), t64(par0, True)
        w = solve_differentiable(loop, P, par=par)
        assert w.shape == (B, loop.w.shape[1]) and type(w.grad_fn).__name__ == MPCParFunction.__name__ + "Backward"
        point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
        gw = torch.zeros((B, 1, w.shape[1]), dtype=torch.float64, device="cuda:0")
        gw[:, 0, nx:nx + nu] = (w[:, nx:nx + nu] - u_t).detach()
        _, direct, flag = loop.sens_model_vjp(gw, point=point, per_stage=False)
        gP = loop.sens_vjp(gw, point=point)[0] if with_P else None
        other = tuple(1.3 * par0)
        if change:  # other constants after the forward: the backward must not use them
            solver.set_par(other)
            loop.solve()
        (0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
        torch.cuda.synchronize()
        assert int(flag.sum()) == 0
        if change:
            assert tuple(solver.ocp.par) == other
        assert bits(par.grad.cpu().numpy()) == bits(direct[:, 0].sum(dim=0).cpu().numpy())
        if with_P:
            assert bits(P.grad.cpu().numpy()) == bits(gP[:, 0].cpu().numpy())
        else:
            assert P.grad is None
        grads.append(par.grad.cpu().numpy())
        solver.set_par(par0)
    assert bits(grads[0]) == bits(grads[1])
    grad = grads[0]
    nom = solver.solve_batch(P0)
    fd = {}
    for h in (1e-3, 1e-4):
        row = []
        for i in range(n_th):
            val = []
            for sgn in (1.0, -1.0):
                moved = par0.copy()
                moved[i] += sgn * h * par0[i]
                solver.set_par(moved)
                r = solver.solve_batch(P0, w0=nom["w"], lam_g0=nom["lam_g"], lam_x0=nom["lam_x"])
                assert np.all(r["status"] <= 1)
                val.append(loss_np(r["w"]))
            row.append((val[0] - val[1]) / (2 * h * par0[i]))
        fd[h] = np.array(row)
    solver.set_par(par0)
    spread = float(np.max(np.abs(fd[1e-3] - fd[1e-4])))
    err = float(np.max(np.abs(grad - 0.5 * (fd[1e-3] + fd[1e-4]))))
    print(f"{name}: gradient {grad}, FD {0.5 * (fd[1e-3] + fd[1e-4])}, spread {spread:.3e}, |autograd - FD| {err:.3e}")
    assert spread <= 1e-3 * max(1.0, float(np.max(np.abs(grad))))
    assert err <= 4.0 * spread + 1e-6
    assert np.max(np.abs(grad)) > 1e-3
    loop = DeviceLoop(solver, P0, device="cuda:0")
    par = t64(par0, True)
    solve_differentiable(loop, t64(P0), irregular="zero", par=par).sum().backward()
    assert bool(torch.isfinite(par.grad).all())
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), par=par, Q=t64(np.ones(nx)), R=t64(np.ones(nu)))
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), par=par[:-1] if n_th > 1 else torch.cat([par, par]))
    with pytest.raises(ValueError):
        solve_differentiable(loop, t64(P0), par=par.to(torch.float32))


def test_autograd_par_refuses_a_linear_model(mpcx):
    import torch
    from mpcx.autograd import solve_differentiable
    from mpcx.device import DeviceLoop

    lin, P = linear_problem("lin4x2_N12")
    solver = mpcx.nlpsol("ag_p_lin", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    loop = DeviceLoop(solver, P, device="cuda:0")
    par = torch.ones(28, dtype=torch.float64, device="cuda:0", requires_grad=True)
    with pytest.raises(ValueError, match="sens_model_vjp"):
        solve_differentiable(loop, loop.P.clone(), par=par)
