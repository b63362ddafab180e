"""GPU tests of per-instance and per-step box bounds (mpcx_set_bounds_dev, Solver.solve_batch with
(B, n_w) bounds, DeviceLoop.set_bounds).

The reference is the shared-bounds path that existed before: an instance with its own bounds must
come out as it does alone, ``solve_batch(P[b:b+1], lbw=lb[b], ubw=ub[b])``, bit for bit (an
instance's bits do not depend on its batch).  The one exception is a batch that mixes
instances with and without state bounds: it runs the state-bounded unit, so its unbounded
instances are compiled differently from their solo run and are held to 1e-6 relative (the
tolerance of two compilations of one algorithm converged to tol = 1e-8)."""
import contextlib
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("w", "f", "lam_g", "lam_x", "status", "iters")
REF_OPTS = {"max_iter": 2000, "acceptable_tol": 1e-8, "acceptable_obj_change_tol": 1e-6}


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def assert_same_bits(got, want, what, rows=None):
    for key in KEYS:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        if rows is not None:
            g = np.ascontiguousarray(g[rows])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {key} differs"


def spec_rows(ocp, B):
    """(B, n_w) lbw / ubw rows equal to the problem's own bounds (user layout)."""
    nx, nu, N = ocp.nx, ocp.nu, ocp.N
    fin = lambda v, inf: np.array([inf if not math.isfinite(x) else x for x in v])  # noqa: E731
    lb, ub = np.full(nx + (nx + nu) * N, -1e20), np.full(nx + (nx + nu) * N, 1e20)
    for k in range(N):
        o = nx + (nx + nu) * k
        lb[o:o + nu], ub[o:o + nu] = fin(ocp.u_lb, -1e20), fin(ocp.u_ub, 1e20)
        lb[o + nu:o + nu + nx], ub[o + nu:o + nu + nx] = fin(ocp.x_lb, -1e20), fin(ocp.x_ub, 1e20)
    return np.tile(lb, (B, 1)), np.tile(ub, (B, 1))


@contextlib.contextmanager
def installed(solver, lb, ub, rows, n_steps=1):
    """lb / ub ((n_steps,) rows, n_w) in the user layout installed on the solver's handle."""
    import torch

    pd = solver._pad
    if pd is not None:
        lb, ub = pd.scatter(lb, pd.w_idx, pd.n_w_pad, -1e20), pd.scatter(ub, pd.w_idx, pd.n_w_pad, 1e20)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (lb, ub)]
    solver._install_bounds((t[0], t[1], rows, n_steps), torch.cuda.current_stream(dev).cuda_stream)
    try:
        yield
    finally:
        solver._install_bounds(None)


def unicycle_P(B, seed=1, y=None):
    rng = np.random.default_rng(seed)
    P = np.zeros((B, 6))
    P[:, 0:2] = rng.uniform(-0.3, 0.3, (B, 2))
    P[:, 2] = rng.uniform(-0.5, 0.5, B)
    P[:, 3] = rng.uniform(1.0, 2.0, B)
    P[:, 4] = rng.uniform(0.5, 1.5, B) if y is None else y
    P[:, 5] = rng.uniform(-0.3, 0.3, B)
    return P


def shape_case(mpcx, name):
    """(ocp, P, ipopt options) of the small batches the bounds are tried on."""
    from mpcx import lti, ode

    if name in ("unicycle_N10", "unicycle_N30"):
        return mpcx.unicycle_point_to_point(N=int(name[-2:])), unicycle_P(5), REF_OPTS
    if name == "kin_bicycle_N10":
        B, N = 5, 10
        rng = np.random.default_rng(2)
        ocp = ode.kinematic_bicycle_tracking(N=N)
        ref = ode.bicycle_circular_reference(rng.uniform(0, 20 * math.pi, B), 0, N)
        return ocp, ocp.params(ref[:, 0, :3] + rng.normal(0, 0.1, (B, 3)), ref), {"max_iter": 500}
    if name == "padded_dint_N8":
        N, T = 8, 0.1
        A, Bm = np.array([[1.0, T], [0.0, 1.0]]), np.array([[0.5 * T * T], [T]])
        lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 0.1, 0.01])[None],
                            tab=np.zeros(N, np.int32), u_lb=(-1.0,), u_ub=(1.0,))
        x0 = np.array([[5.0, 0.0], [-3.0, 1.0], [0.5, -0.5], [2.0, 2.0], [-1.0, 0.0]])
        return lin, lin.params(x0, np.zeros((N, 3))), {"max_iter": 200}
    assert name == "cartpole_qp_N70"
    lin = lti.inverted_pendulum_qp(N=70)
    x = np.array([[0.0, 0.0, 0.1, 0.0], [1.0, 0.5, -0.1, 0.2]])
    return lin, lti.pendulum_params(lin, x, 0.0), {"max_iter": 200}


# ------------------------------------------------------------------------------------------
# 1. rows that all equal the problem's bounds == the shared path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unicycle_N10", "unicycle_N30", "kin_bicycle_N10", "padded_dint_N8",
                                  "cartpole_qp_N70"])
def test_equal_rows_equal_the_shared_path(mpcx, name):
    ocp, P, opts = shape_case(mpcx, name)
    B = P.shape[0]
    solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": opts})
    want = solver.solve_batch(P)
    assert np.all(want["status"] <= 1), want["status"]
    lb, ub = spec_rows(ocp, B)
    with installed(solver, lb[:1], ub[:1], rows=1):
        assert_same_bits(solver.solve_batch(P), want, f"{name}, one shared row")
    assert_same_bits(solver.solve_batch(P, lbw=lb, ubw=ub), want, f"{name}, {B} rows")
    assert solver._dev_bounds is None
    assert_same_bits(solver.solve_batch(P), want, f"{name}, after the per-instance call")


# ------------------------------------------------------------------------------------------
# 2. heterogeneous bounds: every instance as it comes out alone
# ------------------------------------------------------------------------------------------
def check_each_equals_solo(solver, P, lb, ub, what):
    r = solver.solve_batch(P, lbw=lb, ubw=ub)
    assert np.all(r["status"] <= 1), (what, r["status"])
    for b in range(P.shape[0]):
        solo = solver.solve_batch(P[b:b + 1], lbw=lb[b], ubw=ub[b])
        assert_same_bits(r, solo, f"{what}, instance {b}", rows=slice(b, b + 1))
    return r


def test_heterogeneous_input_bounds_unicycle(mpcx):
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("fleet", "mi355x", ocp, {"ipopt": REF_OPTS})
    B = 5
    P = unicycle_P(B)
    lb, ub = spec_rows(ocp, B)
    vmax = np.linspace(0.2, 1.0, B)
    lb[:, 3::5], ub[:, 3::5] = -vmax[:, None], vmax[:, None]
    r = check_each_equals_solo(solver, P, lb, ub, "|v| limits")
    v = r["w"][:, 3::5]
    assert np.all(np.abs(v) <= vmax[:, None] + 1e-9)
    assert np.max(np.abs(v[0])) > 0.19  # the tightest limit is active


def test_heterogeneous_state_bounds_unicycle(mpcx):
    """A different finite Y bound on every instance (all state-bounded), below the target's y."""
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("corridor", "mi355x", ocp, {"ipopt": REF_OPTS})
    B = 5
    P = unicycle_P(B, y=1.5)
    lb, ub = spec_rows(ocp, B)
    ymax = 0.5 + 0.1 * np.arange(B)
    ub[:, 6::5] = ymax[:, None]  # Y of X_1..X_N
    r = check_each_equals_solo(solver, P, lb, ub, "Y bounds")
    assert np.all(r["w"][:, 6::5] <= ymax[:, None] + 1e-9)


def test_heterogeneous_input_bounds_kin_bicycle(mpcx):
    ocp, P, opts = shape_case(mpcx, "kin_bicycle_N10")
    solver = mpcx.nlpsol("kin", "mi355x", ocp, {"ipopt": opts})
    B = P.shape[0]
    lb, ub = spec_rows(ocp, B)
    scale = np.linspace(0.6, 1.0, B)
    for i in range(2):
        lb[:, 3 + i::5] *= scale[:, None]
        ub[:, 3 + i::5] *= scale[:, None]
    check_each_equals_solo(solver, P, lb, ub, "kinematic bicycle input limits")


# ------------------------------------------------------------------------------------------
# 3. a batch mixing state-bounded and unbounded instances runs the state-bounded unit
# ------------------------------------------------------------------------------------------
def test_mixed_batch_runs_the_state_bounded_unit(mpcx):
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("mixed", "mi355x", ocp, {"ipopt": REF_OPTS})
    B = 5
    P = unicycle_P(B, y=1.5)
    lb, ub = spec_rows(ocp, B)
    bounded = np.array([1, 3])
    free = np.array([0, 2, 4])
    ub[bounded[:, None], np.arange(6, 3 + 5 * 10, 5)[None, :]] = np.array([0.6, 0.8])[:, None]
    assert "UnicycleFreeModel" in solver._h.launch_shape(B)[2]  # the problem's own bounds: no state bounded
    with installed(solver, lb, ub, rows=B):
        assert "mpcx::UnicycleModel," in solver._h.launch_shape(B)[2]
        r = solver.solve_batch(P)
    with installed(solver, lb[free], ub[free], rows=free.size):
        assert "UnicycleFreeModel" in solver._h.launch_shape(free.size)[2]
    assert np.all(r["status"] <= 1), r["status"]
    for b in bounded:
        solo = solver.solve_batch(P[b:b + 1], lbw=lb[b], ubw=ub[b])
        assert_same_bits(r, solo, f"bounded instance {b}", rows=slice(b, b + 1))
    for b in free:
        solo = solver.solve_batch(P[b:b + 1], lbw=lb[b], ubw=ub[b])
        err = np.max(np.abs(r["w"][b] - solo["w"][0])) / max(1.0, np.max(np.abs(solo["w"][0])))
        print(f"mixed batch, unbounded instance {b}: relative difference to its solo solve {err:.2e}, "
              f"iterations {int(r['iters'][b])} vs {int(solo['iters'][0])} "
              f"(difference {int(r['iters'][b]) - int(solo['iters'][0])})")
        assert r["status"][b] == solo["status"][0]
        assert err <= 1e-6


# ------------------------------------------------------------------------------------------
# 4. the restoration phase (resume launch) reads the instance's own row
# ------------------------------------------------------------------------------------------
def test_restoration_reads_the_instances_row(mpcx):
    """Instances whose cold-start line search fails and that IPOPT's restoration recovers in the
    resume launch, each with its own input limits, next to one that never parks (row 0): every one
    as it comes out alone.  Precondition (asserted, through the shared path alone): the solo result
    with the instance's bounds changes when restoration is switched off, so the resume launch ran.
    The instances are the 6-state bicycle's 262, 483 and 10 of the config-4 batch, the ones
    tests/test_gpu_resto.py and tests/test_gpu_hard.py park: measured on MI355X, no instance of the
    hard unicycle batch (N = 20, 1024 starts) or of the config-3 kinematic-bicycle batch (N = 30,
    1024 starts) changes with restoration off, with the problem's bounds or with per-instance
    input limits scaled by up to 30 %, so those batches cannot show the resume launch."""
    from mpcx import dist as mdist

    N = 50
    idx = [0, 262, 483, 10]
    ocp = mpcx.dynamic_bicycle_lane_change(N=N)
    t0, x0, (X, Y, V) = mdist.config4_bicycle_inputs(0, 1024)
    refs = np.stack([mpcx.ode.dyn_bicycle_references(X, Y, V, int(t0[i]), N).reshape(-1) for i in idx])
    P = ocp.params(x0[idx], refs)
    B = len(idx)
    opts = {"max_iter": 3000}
    on = mpcx.nlpsol("park", "mi355x", ocp, {"ipopt": opts})
    off = mpcx.nlpsol("park_off", "mi355x", ocp, {"ipopt": opts, "restoration": False})
    lb0, ub0 = spec_rows(ocp, 1)

    def scaled(scale):  # the problem's bounds with both input limits scaled
        l, u = lb0[0].copy(), ub0[0].copy()
        for i in range(ocp.nu):
            l[ocp.nx + i::ocp.nx + ocp.nu] *= scale
            u[ocp.nx + i::ocp.nx + ocp.nu] *= scale
        return l, u

    # row 0: an instance that never parks, limits scaled by 0.9.  A failed line search is a fragile
    # event, so each parking instance takes the largest of three reductions of its limits under
    # which it still ends at status 3 without restoration (its own, different from every other row's).
    rows, keep, solos = [scaled(0.9)], [0], []
    solos.append(on.solve_batch(P[0:1], lbw=rows[0][0], ubw=rows[0][1]))
    for b in range(1, B):
        for eps in (3e-2, 3e-3, 3e-4):
            l, u = scaled(1.0 - eps * b)
            s_off = off.solve_batch(P[b:b + 1], lbw=l, ubw=u)
            s_on = on.solve_batch(P[b:b + 1], lbw=l, ubw=u)
            print(f"instance {idx[b]}, limits x {1.0 - eps * b}: status {int(s_off['status'][0])} without "
                  f"restoration, {int(s_on['status'][0])} with ({int(s_on['iters'][0])} iterations)")
            if s_off["status"][0] == 3 and s_on["status"][0] <= 1:
                assert s_on["w"].tobytes() != s_off["w"].tobytes()  # the recovery decides the result
                rows.append((l, u))
                keep.append(b)
                solos.append(s_on)
                break
    assert len(keep) >= 3, "precondition: at least two instances that need the restoration"
    assert all(s["status"][0] <= 1 for s in solos)
    lb, ub = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert all(not np.array_equal(lb[j], lb[0]) for j in range(1, len(keep)))
    P, idx, B = P[keep], [idx[b] for b in keep], len(keep)
    r = on.solve_batch(P, lbw=lb, ubw=ub)
    for b in range(B):
        assert_same_bits(r, solos[b], f"instance {idx[b]}", rows=slice(b, b + 1))


# ------------------------------------------------------------------------------------------
# 5. closed loop
# ------------------------------------------------------------------------------------------
LOOP_FIELDS = ("P", "w", "w0", "lam", "lam0", "lamx", "lamx0", "f")


def loop_setup(mpcx, B=4):
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("loop", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(B, seed=3, y=1.5)
    lb, ub = spec_rows(ocp, B)
    vmax = np.linspace(0.4, 1.0, B)
    lb[:, 3::5], ub[:, 3::5] = -vmax[:, None], vmax[:, None]
    return ocp, solver, P, lb, ub


def test_closed_loop_run_equals_lockstep_with_instance_bounds(mpcx):
    import torch
    from mpcx.device import DeviceLoop

    _, solver, P, lb, ub = loop_setup(mpcx)
    K, B = 3, P.shape[0]
    dev = torch.device("cuda", 0)
    lock, run = DeviceLoop(solver, P), DeviceLoop(solver, P)
    lock.set_bounds(torch.from_numpy(lb).to(dev), torch.from_numpy(ub).to(dev))
    st_l, it_l = [], []
    for _ in range(K):
        lock.step()
        torch.cuda.synchronize()
        st_l.append(lock.status.cpu().numpy().copy())
        it_l.append(lock.iters.cpu().numpy().copy())
    st_r, it_r = run.run(K)
    torch.cuda.synchronize()
    lock.set_bounds(None, None)
    assert np.all(np.array(st_l) <= 1)
    np.testing.assert_array_equal(st_r.cpu().numpy(), np.array(st_l))
    np.testing.assert_array_equal(it_r.cpu().numpy(), np.array(it_l))
    for n in LOOP_FIELDS:
        got, want = getattr(run, n).cpu().numpy(), getattr(lock, n).cpu().numpy()
        assert got.tobytes() == want.tobytes(), n
    vmax = ub[:, 3]
    assert np.all(np.abs(lock.w.cpu().numpy()[:, 3::5]) <= vmax[:, None] + 1e-9)


def test_closed_loop_per_step_corridor(mpcx):
    """(K, B, n_w) bounds, a Y corridor that tightens every step, served in lock step: the step's
    block installed before each step(), every solve == the solo solve of that instance from the same
    start with that step's bounds.  The multi-step launch does not reload bounds at its step
    boundaries (the reload cost the 20-step unicycle launch 7 %, profiles/instance_bounds/), so
    run() with per-step bounds is refused."""
    import torch
    from mpcx.device import DeviceLoop

    _, solver, P, lb, ub = loop_setup(mpcx)
    K, B = 3, P.shape[0]
    dev = torch.device("cuda", 0)
    lb3, ub3 = np.tile(lb, (K, 1, 1)), np.tile(ub, (K, 1, 1))
    for s in range(K):
        ub3[s][:, 6::5] = (1.2 - 0.2 * s + 0.05 * np.arange(B))[:, None]
    tl, tu = torch.from_numpy(lb3).to(dev), torch.from_numpy(ub3).to(dev)
    lock, run = DeviceLoop(solver, P), DeviceLoop(solver, P)
    st_l, it_l = [], []
    for s in range(K):
        start = {n: getattr(lock, n).cpu().numpy().copy() for n in ("P", "w0", "lam0", "lamx0")}
        lock.set_bounds(tl[s], tu[s])
        lock.step()
        torch.cuda.synchronize()
        st_l.append(lock.status.cpu().numpy().copy())
        it_l.append(lock.iters.cpu().numpy().copy())
        got = {"w": lock.w.cpu().numpy(), "f": lock.f.cpu().numpy(), "lam_g": lock.lam.cpu().numpy(),
               "lam_x": lock.lamx.cpu().numpy(), "status": st_l[-1], "iters": it_l[-1]}
        lock.set_bounds(None, None)
        for b in range(B):
            warm = {} if s == 0 else {"w0": start["w0"][b:b + 1], "lam_g0": start["lam0"][b:b + 1],
                                      "lam_x0": start["lamx0"][b:b + 1]}
            solo = solver.solve_batch(start["P"][b:b + 1], lbw=lb3[s, b], ubw=ub3[s, b], **warm)
            assert_same_bits(got, solo, f"step {s}, instance {b}", rows=slice(b, b + 1))
    assert np.all(np.array(st_l) <= 1)
    # the corridor of the last step holds on the last solution
    assert np.all(lock.w.cpu().numpy()[:, 6::5] <= ub3[K - 1][:, 6::5] + 1e-9)
    # a multi-step launch does not follow per-step blocks: refused (DeviceLoop and the library), and
    # nothing ran -- the loop's tensors are untouched
    run.set_bounds(tl, tu)
    before = {n: getattr(run, n).cpu().numpy().copy() for n in LOOP_FIELDS}
    with pytest.raises(ValueError, match="per-step bounds"):
        run.run(K)
    kept, solver._dev_bounds = solver._dev_bounds, None  # past the Python check: the library's own
    with pytest.raises(mpcx._lib.MpcxError, match="per-step bounds"):
        run.run(K)
    solver._dev_bounds = kept
    torch.cuda.synchronize()
    for n in LOOP_FIELDS:
        assert getattr(run, n).cpu().numpy().tobytes() == before[n].tobytes(), n
    run.set_bounds(tl[:1], tu[:1])  # one block is no per-step array
    run.run(1)
    torch.cuda.synchronize()
    run.set_bounds(None, None)


# ------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------
def test_refused_contents_name_the_entry_and_launch_nothing(mpcx):
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("refuse", "mi355x", ocp, {"ipopt": REF_OPTS})
    B = 5
    P = unicycle_P(B)
    want = solver.solve_batch(P)
    lb, ub = spec_rows(ocp, B)

    def planted(edit):
        l, u = lb.copy(), ub.copy()
        edit(l, u)
        return l, u

    nan = planted(lambda l, u: l.__setitem__((2, 13), np.nan))
    crossed = planted(lambda l, u: (l.__setitem__((2, 8), 0.5), u.__setitem__((2, 8), 0.25)))
    fixed = planted(lambda l, u: (l.__setitem__((3, 9), 0.1), u.__setitem__((3, 9), 0.1)))
    for (l, u), msg in ((nan, r"NaN or lb > ub at step 0, row 2, index 13"),
                        (crossed, r"NaN or lb > ub at step 0, row 2, index 8"),
                        (fixed, r"fixed variable.*step 0, row 3, index 9")):
        with pytest.raises(mpcx._lib.MpcxError, match=msg):
            solver.solve_batch(P, lbw=l, ubw=u)
        assert solver._dev_bounds is None
        assert_same_bits(solver.solve_batch(P), want, "after a refused install")  # nothing was installed
    # the first offender in array order is the one named; a later step's block is named by its step
    both = planted(lambda l, u: (l.__setitem__((4, 20), np.nan), l.__setitem__((1, 30), np.nan)))
    with pytest.raises(mpcx._lib.MpcxError, match=r"row 1, index 30"):
        solver.solve_batch(P, lbw=both[0], ubw=both[1])
    l2, u2 = np.stack([lb, nan[0]]), np.stack([ub, nan[1]])
    with pytest.raises(mpcx._lib.MpcxError, match=r"step 1, row 2, index 13"):
        with installed(solver, l2, u2, rows=B, n_steps=2):
            pass
    # lb == ub inside X_0 is accepted (X_0 is pinned by g_0; its bounds are never read)
    x0fix = planted(lambda l, u: (l.__setitem__((slice(None), slice(0, 3)), 0.5),
                                  u.__setitem__((slice(None), slice(0, 3)), 0.5)))
    assert_same_bits(solver.solve_batch(P, lbw=x0fix[0], ubw=x0fix[1]), want, "lb == ub in X_0")


def test_refused_shapes_and_calls(mpcx):
    import torch
    from mpcx.device import DeviceLoop

    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("refuse2", "mi355x", ocp, {"ipopt": REF_OPTS})
    B = 5
    P = unicycle_P(B)
    want = solver.solve_batch(P)
    lb, ub = spec_rows(ocp, B)
    dev = torch.device("cuda", 0)
    # rows = 3 with B = 5
    with installed(solver, lb[:3], ub[:3], rows=3):
        with pytest.raises(mpcx._lib.MpcxError, match="bound rows"):
            solver.solve_batch(P)
        loop = DeviceLoop(solver, P)
        with pytest.raises(mpcx._lib.MpcxError, match="bound rows"):
            loop.step()
        with pytest.raises(mpcx._lib.MpcxError, match="bound rows"):
            loop.solve()
        assert np.all(solver.solve_batch(P[:3])["status"] <= 1)  # three instances fit
    # one NULL pointer
    t = torch.from_numpy(lb).to(dev)
    for a, b in ((t.data_ptr(), None), (None, t.data_ptr())):
        with pytest.raises(mpcx._lib.MpcxError, match="both"):
            solver._h.set_bounds_dev(a, b, B, 1)
    for rows, n_steps in ((0, 1), (B, 0)):
        with pytest.raises(mpcx._lib.MpcxError, match=">= 1"):
            solver._h.set_bounds_dev(t.data_ptr(), t.data_ptr(), rows, n_steps)
    # n_steps = 2 with run(3): refused by DeviceLoop and by the library
    loop = DeviceLoop(solver, P)
    l2, u2 = torch.from_numpy(np.stack([lb, lb])).to(dev), torch.from_numpy(np.stack([ub, ub])).to(dev)
    loop.set_bounds(l2, u2)
    with pytest.raises(ValueError, match="per-step bounds"):
        loop.run(3)
    kept, solver._dev_bounds = solver._dev_bounds, None  # past the Python check: the library's own
    with pytest.raises(mpcx._lib.MpcxError, match="per-step bounds"):
        loop.run(3)
    solver._dev_bounds = kept
    with pytest.raises(ValueError):
        loop.set_bounds(l2[0], None)
    with pytest.raises(ValueError):
        loop.set_bounds(l2[:, :3], u2[:, :3])
    # revert: NULL, NULL gives the problem's bounds again
    loop.set_bounds(None, None)
    assert solver._dev_bounds is None
    assert_same_bits(solver.solve_batch(P), want, "after the revert")
