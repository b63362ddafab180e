"""GPU tests of the path-frame kinematic bicycle MPC with steering-rate limits (model 7,
``mpcx.ode.path_bicycle_lane_keeping``; ``Trajectory Tracking/test2.py``) through the C ABI.

PARITY UNPINNED: the script writes no output file.  The reference is the NumPy helper
tests/helpers/path_bicycle_ref.py (complex-step derivatives, written from the model's equations;
tests/test_path_bicycle_cpu.py ties it to oracle/ode_ref.py's kinematic bicycle).  Tolerances as
tests/test_gpu_ode.py: plant 1e-12 relative; optima 1e-6 relative at solver tol 1e-10; KKT
stationarity <= 1e-6, feasibility <= 1e-9 (bounds to the same 1e-9), complementarity <= 1e-6.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

pytestmark = pytest.mark.gpu

NX, NU, NZ = 4, 2, 6
TOL = {"ipopt": {"max_iter": 300, "tol": 1e-10}}


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1.0))


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def _csv():
    import pandas as pd

    g = pd.read_csv(os.path.join(ROOT, "tests", "golden", "lane_change.csv"))
    return np.asarray(g.x, float), np.asarray(g.y, float), np.asarray(g.uref, float)


def cases(B, N, seed=0, steer="bicycle", **kw):
    """(ocp, P (B, n_p)) of a small seeded batch: a path of constant curvature |kappa| <= 0.05
    with a slowly drifting lateral position, driven at 3-10 m/s from up to 1 m beside it."""
    from mpcx import ode

    rng = np.random.default_rng(seed)
    ocp = ode.path_bicycle_lane_keeping(N=N, steer=steer, **kw)
    k = np.arange(N)[None, :]
    rows = np.zeros((B, N, NZ))
    rows[..., 0] = rng.uniform(-0.5, 0.5, (B, 1)) + 0.01 * k * rng.uniform(-1, 1, (B, 1))
    rows[..., 1] = rng.uniform(-0.05, 0.05, (B, 1))
    rows[..., 2] = rng.uniform(3.0, 10.0, (B, 1))
    rows[..., 3] = rng.uniform(-0.05, 0.05, (B, 1))
    rows[..., 5] = rng.uniform(-0.2, 0.2, (B, 1))
    x = np.stack([rows[:, 0, 0] + rng.uniform(-1, 1, B), rows[:, 0, 1] + rng.normal(0, 0.05, B),
                  rows[:, 0, 2] + rng.normal(0, 0.5, B)], axis=1)
    return ocp, ode.path_bicycle_params(ocp, x, rng.uniform(-0.1, 0.1, B), rows)


def certify(pr, r, P, b, tag=""):
    c = pr.kkt(r["w"][b], r["lam_g"][b], r["lam_x"][b], P[b])
    print(f"kkt {tag} b={b}: " + " ".join(f"{k}={v:.3e}" for k, v in c.items()))
    assert c["stat"] <= 1e-6 and c["feas"] <= 1e-9, (tag, b, c)
    assert c["bound"] <= 1e-9 and c["sign"] == 0.0 and c["compl"] <= 1e-6, (tag, b, c)
    return c


@pytest.mark.parametrize("steer", ["bicycle", "as_written"])
def test_plant_matches_helper(mpcx, steer):
    from mpcx import ode
    from path_bicycle_ref import PathProblem

    B = 64
    rng = np.random.default_rng(11)
    ocp = ode.path_bicycle_lane_keeping(N=3, steer=steer)
    rows = np.zeros((B, 3, NZ))
    rows[..., 0] = rng.uniform(-2, 2, (B, 1))
    rows[..., 1] = rng.uniform(-0.5, 0.5, (B, 1))
    rows[..., 2] = rng.uniform(0.5, 10, (B, 1))
    rows[..., 3] = rng.uniform(-0.2, 0.2, (B, 1))
    rows[..., 5] = rng.uniform(-1, 1, (B, 1))
    x = np.stack([rows[:, 0, 0] + rng.uniform(-1, 1, B),  # |y - yt| <= 1: 1 - (y - yt) kappa >= 0.8
                  rows[:, 0, 1] + rng.uniform(-0.5, 0.5, B), rng.uniform(0.5, 10, B)], axis=1)
    s = rng.uniform(-0.3, 0.3, B)
    P = ode.path_bicycle_params(ocp, x, s, rows)
    U = np.stack([rng.uniform(-0.1225, 0.1225, B), rng.uniform(-2, 2, B)], axis=1)
    xf, qf = mpcx.integrator(ocp).batch(P, U)
    pr = PathProblem(ocp)
    z = np.concatenate([P[:, :NX], U], axis=1)
    print("plant rel", rel(xf, pr.F(z, rows[:, 0])), rel(qf, pr.l(z, rows[:, 0])))
    assert rel(xf, pr.F(z, rows[:, 0])) <= 1e-12
    assert rel(qf, pr.l(z, rows[:, 0])) <= 1e-12
    assert np.array_equal(xf[:, 3], s + U[:, 0])  # the carried state: exactly s + d


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("N,B", [(1, 5), (20, 6), (40, 4), (70, 3)])
def test_optimum_is_certified_by_helper(mpcx, N, B, policy):
    """A single interval, the script's horizon (32-lane group), a full wave, a two-wave group."""
    from path_bicycle_ref import PathProblem

    ocp, P = cases(B, N, seed=N)
    solver = mpcx.nlpsol("pb", "mi355x", ocp, dict(TOL, group_policy=policy))
    r = solver.solve_batch(P)
    assert np.all(r["status"] == 0), (r["status"], r["iters"])
    pr = PathProblem(ocp)
    for b in range(B):
        certify(pr, r, P, b, f"N={N}")
        assert abs(r["f"][b] - pr.objective(r["w"][b], P[b])) <= 1e-8 * max(1.0, abs(r["f"][b]))
        if N <= 20:  # the helper's own solve, started at the GPU point: the same local optimum
            X, U = pr.split_w(r["w"][b])
            Uo, Xo, Jo, info = pr.solve_slsqp(P[b], U)
            print(f"slsqp N={N} b={b}: status={info.status} relU={rel(U, Uo):.3e} relX={rel(X, Xo):.3e} "
                  f"df={abs(r['f'][b] - Jo):.3e} f={Jo:.6e}")
            assert info.status == 0, info
            assert rel(U, Uo) <= 1e-6 and rel(X, Xo) <= 1e-6
            assert abs(r["f"][b] - Jo) <= 1e-6 * max(1.0, abs(Jo))


def _offset_case(ode, off, **kw):
    ocp = ode.path_bicycle_lane_keeping(N=20, **kw)
    rows = np.zeros((20, NZ))
    rows[:, 2] = 10.0
    return ocp, ode.path_bicycle_params(ocp, [off, 0.0, 10.0], 0.0, rows)


@pytest.mark.parametrize("off", [2.0, 3.0])
def test_rate_and_steering_limits_are_active(mpcx, off):
    """N = 20, delta_prev = 0, a straight path driven at 10 m/s from `off` metres beside it.  The
    helper's own solve (CPU) has the rate bound active in the first three intervals and the
    steering bound after them from 2 m on; at 1 m the steering stays inside 0.26 rad, so the
    offsets are 2 m and 3 m."""
    from mpcx import ode
    from path_bicycle_ref import PathProblem

    ocp, P = _offset_case(ode, off)
    r = mpcx.nlpsol("pb", "mi355x", ocp, TOL).solve_batch(P)
    assert r["status"][0] == 0
    pr = PathProblem(ocp)
    certify(pr, r, P, 0, f"off={off}")
    X, U = pr.split_w(r["w"][0])
    lx = r["lam_x"][0][NX:].reshape(20, NZ)  # per interval: (d, a, y, phi, v, s of the next node)
    print("rate multipliers", np.abs(lx[:, 0]).max(), "steering multipliers", np.abs(lx[:, 5]).max())
    assert np.abs(lx[:, 0]).max() > 1e-3 and np.abs(lx[:, 5]).max() > 1e-3
    assert np.sum(np.abs(U[:, 0]) >= 0.1225 - 1e-6) >= 2 and np.sum(np.abs(X[:, 3]) >= 0.384 - 1e-6) >= 1
    Uo, Xo, Jo, info = pr.solve_slsqp(P[0], U)
    print(f"slsqp off={off}: relU={rel(U, Uo):.3e} df={abs(r['f'][0] - Jo):.3e}")
    assert info.status == 0 and rel(U, Uo) <= 1e-6 and abs(r["f"][0] - Jo) <= 1e-6 * max(1.0, abs(Jo))


def test_without_rate_limit_matches_helper(mpcx):
    """rate_max = 1e20 (no bound): the helper's optimum of the problem without rate limits."""
    from mpcx import ode
    from path_bicycle_ref import PathProblem

    ocp, P = _offset_case(ode, 2.0, rate_max=1e20)
    r = mpcx.nlpsol("pb", "mi355x", ocp, TOL).solve_batch(P)
    assert r["status"][0] == 0
    pr = PathProblem(ocp)
    assert not np.isfinite(pr.z_lb[4]) and not np.isfinite(pr.z_ub[4])
    certify(pr, r, P, 0, "free rate")
    X, U = pr.split_w(r["w"][0])
    assert np.abs(U[:, 0]).max() > 0.1225 + 1e-3  # the limited problem's optimum is another one
    assert np.all(r["lam_x"][0][NX:].reshape(20, NZ)[:, 0] == 0.0)
    Uo, Xo, Jo, info = pr.solve_slsqp(P[0], U)
    # and the helper's solve from its own cold start: the same optimal value
    _, _, Jc, cold = pr.solve_slsqp(P[0], np.zeros((20, NU)))
    print(f"slsqp free rate: relU={rel(U, Uo):.3e} df={abs(r['f'][0] - Jo):.3e} cold df={abs(r['f'][0] - Jc):.3e}")
    assert cold.status == 0 and abs(r["f"][0] - Jc) <= 1e-6 * max(1.0, abs(Jc))
    assert info.status == 0 and rel(U, Uo) <= 1e-6 and abs(r["f"][0] - Jo) <= 1e-6 * max(1.0, abs(Jo))


def test_run_equals_lockstep(mpcx):
    import torch
    from mpcx.device import DeviceLoop

    ocp, P = cases(32, 20, seed=7)
    solver = mpcx.nlpsol("s", "mi355x", ocp)
    lock, run = DeviceLoop(solver, P), DeviceLoop(solver, P)
    st_l, it_l = [], []
    for _ in range(3):
        lock.step()
        torch.cuda.synchronize()
        st_l.append(lock.status.cpu().numpy().copy())
        it_l.append(lock.iters.cpu().numpy().copy())
    st_r, it_r = run.run(3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st_r.cpu().numpy(), np.array(st_l))
    np.testing.assert_array_equal(it_r.cpu().numpy(), np.array(it_l))
    assert np.all(np.array(st_l) == 0)
    for n in ("P", "w", "w0", "lam", "lamx", "f"):
        np.testing.assert_array_equal(getattr(run, n).cpu().numpy(), getattr(lock, n).cpu().numpy(), err_msg=n)


def test_batch_independence(mpcx):
    ocp, P = cases(200, 20, seed=9)
    solver = mpcx.nlpsol("s", "mi355x", ocp, TOL)
    big = solver.solve_batch(P)
    for b in (0, 137):
        one = solver.solve_batch(P[b:b + 1])
        for n in ("w", "f", "lam_g", "lam_x", "status", "iters"):
            np.testing.assert_array_equal(one[n][0], big[n][b], err_msg=f"{n} of instance {b}")


def test_closed_loop_on_lane_change(mpcx):
    """60 closed-loop steps on lane_change.csv from 8 start rows: one multi-step launch with Pseq
    against 60 lock-step launches (the same bits), whose per-step states give the applied steering."""
    import torch
    from mpcx import ode
    from mpcx.device import DeviceLoop
    from path_bicycle_ref import PathProblem

    x, y, v = _csv()
    B, K, N = 8, 60, 20
    t0 = np.linspace(0, 400, B).astype(int)
    ocp = ode.path_bicycle_lane_keeping(N=N)
    rows = np.stack([[ode.path_bicycle_references(x, y, v, int(t) + s, N) for t in t0] for s in range(K)])  # K, B, N, 6
    x0 = np.stack([rows[0, :, 0, 0], rows[0, :, 0, 1], rows[0, :, 0, 2]], axis=1)
    Pseq = np.stack([ode.path_bicycle_params(ocp, x0, 0.0, rows[s]) for s in range(K)])
    solver = mpcx.nlpsol("cl", "mi355x", ocp, TOL)
    run, lock = DeviceLoop(solver, Pseq[0]), DeviceLoop(solver, Pseq[0])
    st, _ = run.run(K, Pseq=torch.from_numpy(Pseq).cuda())
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert np.all(st <= 1), st
    pr = PathProblem(ocp)
    refs = torch.from_numpy(np.ascontiguousarray(Pseq[:, :, NX:])).cuda()
    applied = [np.zeros(B)]
    for s in range(K):
        lock.set_stage_refs(refs[s])
        Pb = lock.P.cpu().numpy().copy()
        lock.step()
        torch.cuda.synchronize()
        applied.append(lock.P[:, 3].cpu().numpy().copy())
        if s in (0, 30, 59):
            r = {"w": lock.w.cpu().numpy(), "lam_g": lock.lam.cpu().numpy(), "lam_x": lock.lamx.cpu().numpy()}
            for b in (4, 5):  # start rows 228 and 285: inside the lane change
                certify(pr, r, Pb, b, f"step {s}")
    applied = np.array(applied)
    print("max |delta|", np.abs(applied).max(), "max step", np.abs(np.diff(applied, axis=0)).max())
    assert np.abs(applied).max() <= 0.384 + 1e-9
    assert np.abs(np.diff(applied, axis=0)).max() <= 0.1225 + 1e-9
    # (the multi-step launch reads its rows from Pseq and leaves those of P as they were)
    np.testing.assert_array_equal(run.P[:, :NX].cpu().numpy(), lock.P[:, :NX].cpu().numpy(), err_msg="x0")
    for n in ("w", "w0", "lam", "lamx", "f"):
        np.testing.assert_array_equal(getattr(run, n).cpu().numpy(), getattr(lock, n).cpu().numpy(), err_msg=n)


def test_nmpc_facade_runs_the_script_loop(mpcx):
    """Ten iterations of the loop body of test2.py:122-143 through mpcx.nmpc equal the same ten
    through nlpsol + path_bicycle_params."""
    from mpcx import ode

    x, y, v = _csv()
    N = 20
    ocp = ode.path_bicycle_lane_keeping(N=N)
    x0 = np.array([0.05, 0.0, 0.4])
    solver = mpcx.nmpc(ocp, x0=x0, p=np.zeros((N, NZ)), uprev=[0.0], opts=TOL)
    uf, xf_, duf = [], [], []
    for t in range(10):
        p = ode.path_bicycle_references(x, y, v, t, N)
        for k in range(N):
            solver.par["p", k] = p[k, :]
        solver.solve()
        assert solver.stats["status"] == "Solve_Succeeded"
        solver.saveguess()
        solver.fixvar("x", 0, solver.var["x", 1])
        uf.append(np.array(solver.var["u", 0, :]).flatten())
        duf.append(np.array(solver.var["Du", 0]).flatten())
        xf_.append(np.array(solver.var["x", 1]).flatten())
        assert solver.var["x", 0].shape == (3, 1) and len(solver.var["x", :, :]) == N + 1
    raw = mpcx.nlpsol("raw", "mi355x", ocp, TOL)
    xs, dprev, guess = x0.copy(), 0.0, None
    for t in range(10):
        P = ode.path_bicycle_params(ocp, xs, dprev, ode.path_bicycle_references(x, y, v, t, N))
        r = raw.solve_batch(P, w0=guess, want_lam=False)
        w = r["w"][0]
        X = np.stack([w[0:NX]] + [w[NX + NZ * k + NU:NX + NZ * (k + 1)] for k in range(N)])
        U = np.stack([w[NX + NZ * k:NX + NZ * k + NU] for k in range(N)])
        Xs, Us = np.concatenate([X[1:], X[-1:]]), np.concatenate([U[1:], U[-1:]])
        guess = np.concatenate([Xs[0]] + [np.concatenate([Us[k], Xs[k + 1]]) for k in range(N)])[None, :]
        applied = dprev + U[0, 0]
        assert np.array_equal(uf[t], [applied, U[0, 1]]) and np.array_equal(duf[t], U[0, 0:1])
        assert np.array_equal(xf_[t], X[1, :3])
        xs, dprev = X[1, :3], applied
    assert abs(dprev) <= 0.384 + 1e-9
    up = lambda: float(np.asarray(solver.par["uprev"][0]).reshape(-1)[0])  # noqa: E731
    assert up() == dprev
    # a loop without saveguess: fixvar alone carries the applied steering into uprev, once
    for t in range(10, 13):
        for k in range(N):
            solver.par["p", k] = ode.path_bicycle_references(x, y, v, t, N)[k, :]
        before = up()
        solver.solve()
        applied = float(solver.var["u", 0][0, 0])
        assert applied == before + float(solver.var["Du", 0][0, 0]) and abs(applied - before) <= 0.1225 + 1e-9
        solver.fixvar("x", 0, solver.var["x", 1])
        assert up() == applied
        solver.fixvar("x", 0, solver.var["x", 1])  # a second fixvar does not move it again
        assert up() == applied
    solver.solve()
    solver.par["uprev"] = [0.05]  # set by hand after a solve: fixvar leaves it
    solver.fixvar("x", 0, solver.var["x", 1])
    assert up() == 0.05
