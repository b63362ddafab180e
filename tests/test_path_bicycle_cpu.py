"""CPU: the path-frame kinematic bicycle MPC (model 7) -- the C ABI's default spec, the Python
builders, the stage rows against the recorded rows of ``Trajectory Tracking/test2.py:79-99``
(tests/golden/test2_parameter_rows.json) and against the rules as per-index formulas, and the NumPy reference (tests/helpers/path_bicycle_ref.py)
against finite differences and against the kinematic bicycle of oracle/ode_ref.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mpc-verde_amd")], check=True)
    return ctypes.CDLL(LIB)


def _csv():
    import pandas as pd

    g = pd.read_csv(os.path.join(ROOT, "tests", "golden", "lane_change.csv"))
    return np.asarray(g.x, float), np.asarray(g.y, float), np.asarray(g.uref, float)


@pytest.mark.parametrize("N", [20, 7])
def test_default_spec_is_the_script(lib, N):
    from mpcx import _lib

    M = _lib.MODEL_PATH_BICYCLE
    hdr = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    assert f"MPCX_MODEL_PATH_BICYCLE = {M}" in hdr and M == 7
    s = _lib.Spec()
    assert lib.mpcx_default_spec(ctypes.byref(s), M, N) == 0
    assert (s.model, s.nx, s.nu, s.N, s.M) == (M, 4, 2, N, 1)
    assert (s.cost, s.param_layout) == (_lib.COST_NODE, _lib.P_X0_STAGEREF)
    assert s.T == 0.05
    n1 = N + 1
    assert list(s.Q)[:4] == [1.75 / n1, 2.5 / n1, 2.5 / n1, 0.0]
    assert list(s.R)[:2] == [0.0, 0.4 / n1]
    assert list(s.par)[:4] == [3.5, 1.0, 1.0 / 3.5, 10.0 / n1]  # bicycle form tan(delta) / L
    assert (s.lbu[0], s.ubu[0], s.lbu[1], s.ubu[1]) == (-0.1225, 0.1225, -2.0, 2.0)
    assert (s.lbx[3], s.ubx[3]) == (-0.384, 0.384)
    assert all(s.lbx[i] == -1e20 and s.ubx[i] == 1e20 for i in range(3))
    for bad in (6, 8):  # 6 stays unassigned
        assert lib.mpcx_default_spec(ctypes.byref(s), bad, N) != 0


def test_create_refuses_invalid_specs_before_any_device_call(lib):
    """L > 0, par finite and the stage-row layout are checked with the other arguments, before the
    device is looked for: MPCX_EINVAL (-1) with a message, on a machine with or without a GPU."""
    from mpcx import _lib

    lib.mpcx_last_error.restype = ctypes.c_char_p

    def refused(edit):
        s = _lib.Spec()
        assert lib.mpcx_default_spec(ctypes.byref(s), _lib.MODEL_PATH_BICYCLE, 20) == 0
        edit(s)
        h = ctypes.c_void_p()
        assert lib.mpcx_create(ctypes.byref(s), ctypes.byref(h)) == -1 and not h.value
        return lib.mpcx_last_error().decode()

    def setpar(i, v):
        def edit(s):
            s.par[i] = v
        return edit

    assert "L" in refused(setpar(0, 0.0)) and "L" in refused(setpar(0, -3.5))
    for i, v in ((0, math.nan), (1, math.inf), (2, math.nan), (3, -math.inf)):
        assert "finite" in refused(setpar(i, v))
    assert "STAGEREF" in refused(lambda s: setattr(s, "param_layout", _lib.P_X0_XREF))
    assert "NODE" in refused(lambda s: setattr(s, "cost", _lib.COST_QUADRATURE))


def test_builder_matches_default_spec(lib):
    from mpcx import _lib, ode
    from mpcx.ocp import to_spec

    s = _lib.Spec()
    assert lib.mpcx_default_spec(ctypes.byref(s), _lib.MODEL_PATH_BICYCLE, 20) == 0
    t = to_spec(ode.path_bicycle_lane_keeping(N=20))
    for name in ("model", "cost", "param_layout", "N", "M", "nx", "nu", "T"):
        assert getattr(s, name) == getattr(t, name), name
    for name, n in (("Q", 4), ("R", 2), ("lbu", 2), ("ubu", 2), ("lbx", 4), ("ubx", 4), ("par", 8)):
        assert list(getattr(s, name))[:n] == list(getattr(t, name))[:n], name
    w = ode.path_bicycle_lane_keeping(N=20, steer="as_written")
    assert w.par == (3.5, 1.0 / 3.5, 1.0, 10.0 / 21)


def test_odeocp_validation_and_params():
    from mpcx import ode

    ocp = ode.path_bicycle_lane_keeping(N=5, rate_max=0.2, delta_max=0.3, a_max=1.0)
    assert (ocp.nx, ocp.nu, ocp.n_p) == (4, 2, 4 + 6 * 5)
    assert ocp.u_lb == (-0.2, -1.0) and ocp.x_ub[3] == 0.3 and ocp.x_lb[:3] == (-math.inf,) * 3
    with pytest.raises(ValueError):
        ode.path_bicycle_lane_keeping(steer="ackermann")
    with pytest.raises(ValueError):
        ode.path_bicycle_lane_keeping(L=0.0)
    kw = dict(model="path_bicycle", N=5, T=0.05, Q=(1.0,) * 4, R=(1.0,) * 2, u_lb=(-1.0,) * 2, u_ub=(1.0,) * 2,
              x_lb=(-1.0,) * 4, x_ub=(1.0,) * 4)
    ode.OdeOCP(par=(3.5, 1.0, 1.0, 0.1), **kw)
    for bad in ((3.5, 1.0, 1.0), (-1.0, 1.0, 1.0, 0.1), (3.5, math.nan, 1.0, 0.1)):
        with pytest.raises(ValueError):
            ode.OdeOCP(par=bad, **kw)
    with pytest.raises(ValueError):
        ode.OdeOCP(par=(3.5, 1.0, 1.0, 0.1), param="x0_xref", **kw)
    with pytest.raises(ValueError):
        ode.OdeOCP(par=(3.5, 1.0, 1.0, 0.1), **dict(kw, Q=(1.0,) * 3))
    rows = np.arange(30.0).reshape(5, 6)
    P = ode.path_bicycle_params(ocp, [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [0.1, 0.2], rows)
    assert P.shape == (2, 34)
    assert P[1, :4].tolist() == [4.0, 5.0, 6.0, 0.2] and P[0, 4:].tolist() == rows.reshape(-1).tolist()
    assert ode.path_bicycle_params(ocp, [1.0, 2.0, 3.0], 0.3, rows)[0, :4].tolist() == [1.0, 2.0, 3.0, 0.3]
    with pytest.raises(ValueError):
        ode.path_bicycle_params(ocp, [1.0, 2.0, 3.0, 0.0], 0.3, rows)


def _golden_rows():
    """The script's parameter array p (Nt = 20 rows of (y_ref, phi_ref, slot 2, slot 3), its own slot
    order) after the fill of steps 0, 1, 250 and the last ones on lane_change.csv: recorded
    results (tests/golden/test2_parameter_rows.json)."""
    import json

    with open(os.path.join(ROOT, "tests", "golden", "test2_parameter_rows.json")) as f:
        d = json.load(f)
    assert d["Nt"] == 20
    return {int(t): np.array(r) for t, r in d["steps"].items()}


def test_references_match_the_recorded_rows():
    from mpcx import ode

    x, y, v = _csv()
    n = len(x)
    ref = _golden_rows()
    # every branch: the first rows, the interior, and each rule of the path's end
    assert sorted(ref) == [0, 1, 250, n - 21, n - 20, n - 19, n - 2, n - 1]
    for t, p in ref.items():
        w = ode.path_bicycle_references(x, y, v, t, 20, as_written=True)
        assert w.shape == (20, 6)
        # as the script's functions read its rows: slot 2 is their kappa, slot 3 their vdes
        assert np.array_equal(w[:, [0, 1]], p[:, [0, 1]]), t
        assert np.array_equal(w[:, 3], p[:, 2]) and np.array_equal(w[:, 2], p[:, 3]), t
        assert np.all(w[:, 4:] == 0.0)
        m = ode.path_bicycle_references(x, y, v, t, 20)
        assert np.array_equal(m[:, [0, 1]], p[:, [0, 1]]) and np.array_equal(m[:, 2], p[:, 2]), t
        assert np.all(np.isfinite(m)) and np.all(m[:, 4:] == 0.0)


def test_references_rules_per_index():
    """The rules as closed formulas of the path index i = t + k, over every step of the csv: a row
    depends on i alone; the heading is that of the segment arriving at min(i, n - 1) (0 at i = 0);
    y and vdes hold their last rows; the second-difference slot is the placeholder below i = 2 and
    holds the value of index n - 2 from there on."""
    from mpcx import ode

    x, y, v = _csv()
    n, N = len(x), 20
    i = np.arange(n + N)
    c = np.minimum(i, n - 1)
    head = np.where(i == 0, 0.0, np.arctan2(y[c] - y[np.maximum(c - 1, 0)], x[c] - x[np.maximum(c - 1, 0)]))
    j = np.clip(i, 2, n - 2)
    dd = np.hypot(x[j - 1] - 2 * x[j] + x[j + 1], y[j - 1] - 2 * y[j] + y[j + 1]) / 0.05**2
    dd = np.where(i < 2, 1.0, dd)
    for t in range(n):
        w = ode.path_bicycle_references(x, y, v, t, N, as_written=True)
        k = t + np.arange(N)
        assert np.array_equal(w[:, 0], y[c[k]]) and np.array_equal(w[:, 1], head[k]), t
        assert np.array_equal(w[:, 3], v[c[k]]), t
        assert np.allclose(w[:, 2], dd[k], rtol=1e-13, atol=0), t
    w = ode.path_bicycle_references(x, y, v, n - 5, N, as_written=True)
    assert np.all(w[3:, 2] == w[3, 2])  # held from index n - 2 on
    # by meaning: the signed curvature; its size is |(x'', y'')| / speed^2 less the tangential part
    m = ode.path_bicycle_references(x, y, v, 240, 20)
    i = 240 + np.arange(20)
    dx, dy = (x[i + 1] - x[i - 1]) / 0.1, (y[i + 1] - y[i - 1]) / 0.1
    ddx, ddy = (x[i - 1] - 2 * x[i] + x[i + 1]) / 0.0025, (y[i - 1] - 2 * y[i] + y[i + 1]) / 0.0025
    assert np.allclose(m[:, 3], (dx * ddy - dy * ddx) / (dx**2 + dy**2) ** 1.5, rtol=1e-12, atol=0)
    assert np.all(np.abs(m[:, 3]) <= np.hypot(ddx, ddy) / (dx**2 + dy**2) + 1e-12)
    assert ode.path_bicycle_references(x, y, v, 0, 3)[:2, 3].tolist() == [0.0, 0.0]


def _points(pr, rng, n):
    z = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(0.5, 10, (n, 1)), rng.uniform(-0.3, 0.3, (n, 1)),
                        rng.uniform(-0.1, 0.1, (n, 1)), rng.uniform(-2, 2, (n, 1))], axis=1)
    row = np.zeros((n, 6))
    row[:, 3] = rng.uniform(-0.2, 0.2, n)
    row[:, 0] = z[:, 0] - rng.uniform(-1, 1, n)  # |y - yt| <= 1: 1 - (y - yt) kappa >= 0.8
    row[:, 1] = rng.uniform(-0.5, 0.5, n)
    row[:, 2] = rng.uniform(0.5, 10, n)
    row[:, 5] = rng.uniform(-1, 1, n)
    return z, row


@pytest.mark.parametrize("steer", ["bicycle", "as_written"])
def test_helper_derivatives_match_central_differences(steer):
    from mpcx import ode
    from path_bicycle_ref import PathProblem

    pr = PathProblem(ode.path_bicycle_lane_keeping(N=4, steer=steer))
    pr.M = 2
    z, row = _points(pr, np.random.default_rng(5), 16)
    J, g = pr.jac(z, row), pr.grad_l(z, row)
    assert J.shape == (16, 4, 6) and g.shape == (16, 6)
    h = 1e-6
    for j in range(6):
        e = np.zeros(6)
        e[j] = h
        Jfd = (pr.F(z + e, row) - pr.F(z - e, row)) / (2 * h)
        gfd = (pr.l(z + e, row) - pr.l(z - e, row)) / (2 * h)
        assert np.max(np.abs(J[:, :, j] - Jfd)) <= 1e-7 * max(1.0, np.max(np.abs(J)))
        assert np.max(np.abs(g[:, j] - gfd)) <= 1e-7 * max(1.0, np.max(np.abs(g)))
    # the carried state: s+ = s + d exactly, whatever the rest
    assert np.array_equal(pr.F(z, row)[:, 3], z[:, 3] + z[:, 4])
    assert np.array_equal(J[:, 3, :], np.tile([0, 0, 0, 1.0, 1.0, 0], (16, 1)))
    # s and d enter only through delta = s + d
    assert pr.W[3] == 0.0 and pr.W[4] == 0.0  # the builder weighs neither s nor d
    assert np.array_equal(J[:, :, 3], J[:, :, 4]) and np.allclose(g[:, 3], g[:, 4], rtol=1e-14, atol=1e-15)


def test_helper_straight_path_is_the_kinematic_bicycle():
    """kappa = 0, yt = phit = 0, d = 0: (y, phi) follow the (Y, psi) rows of oracle/ode_ref.py's
    f_kin_bicycle at the same v and delta (a = 0 keeps v; the oracle's v is an input)."""
    from mpcx import ode
    from oracle import ode_ref
    from path_bicycle_ref import PathProblem

    N, L = 12, 3.5
    pr = PathProblem(ode.path_bicycle_lane_keeping(N=N, L=L))
    kin = ode_ref.Problem(ode.kinematic_bicycle_tracking(N=N, T=0.05, L=L))
    for v, delta, y0, phi0 in ((5.0, 0.2, 0.3, -0.1), (0.7, -0.38, -1.0, 0.4)):
        X = pr.rollout(np.zeros((N, 2)), [y0, phi0, v, delta], np.zeros((N, 6)))
        K = kin.rollout(np.tile([v, delta], (N, 1)), [0.0, y0, phi0])
        assert np.max(np.abs(X[:, 0] - K[:, 1])) <= 1e-13 * max(1.0, np.max(np.abs(K[:, 1])))
        assert np.max(np.abs(X[:, 1] - K[:, 2])) <= 1e-13
        assert np.array_equal(X[:, 2], np.full(N + 1, v)) and np.array_equal(X[:, 3], np.full(N + 1, delta))


def test_helper_certifies_its_own_optimum():
    """The helper's SLSQP optimum of the single-shooting form, with the multipliers of the
    multiple-shooting form rebuilt from the adjoints, passes the helper's own certificate where no
    steering bound is active (the rate bound's multipliers are minus the reduced gradient)."""
    from mpcx import ode
    from path_bicycle_ref import NX, NZ, PathProblem

    N = 8
    ocp = ode.path_bicycle_lane_keeping(N=N)
    pr = PathProblem(ocp)
    rows = np.zeros((N, 6))
    rows[:, 2] = 10.0
    rows[:, 3] = 0.01
    P = ode.path_bicycle_params(ocp, [1.0, 0.0, 10.0], 0.0, rows)[0]
    U, X, J, r = pr.solve_slsqp(P, np.zeros((N, 2)))
    assert r.status == 0 and np.max(np.abs(X[:, 3])) < 0.38  # steering bound idle
    assert np.any(np.abs(U[:, 0]) >= 0.1225 - 1e-12)       # rate bound active
    Z = np.concatenate([X[:-1], U], axis=1)
    Jac, gl = pr.jac(Z, rows), pr.grad_l(Z, rows)
    lam = np.zeros((N + 1, NX))
    lam_x = np.zeros(NX + NZ * N)
    for k in range(N - 1, -1, -1):
        gu = gl[k, NX:] + Jac[k, :, NX:].T @ lam[k + 1]
        lam_x[NX + NZ * k: NX + NZ * k + 2] = -gu
        if k > 0:
            lam[k] = gl[k, :NX] + Jac[k, :, :NX].T @ lam[k + 1]
    c = pr.kkt(pr.join_w(X, U), lam.reshape(-1), lam_x, P)
    assert c["stat"] <= 1e-12 and c["feas"] <= 1e-14 and c["bound"] <= 1e-12
    free = np.abs(np.abs(U[:, 0]) - 0.1225) > 1e-9
    assert np.max(np.abs(lam_x.reshape(-1)[NX:].reshape(N, NZ)[free, 0])) <= 1e-6
    assert c["sign"] == 0.0
    assert abs(pr.objective(pr.join_w(X, U), P) - J) <= 1e-14
