"""Non-finite data never ends as success.

The termination test of the solve kernel takes maxima (qmax_abs / fmax), and a max drops a quiet NaN:
a NaN residual leaves E = 0.  These tests plant ONE NaN in one instance of a batch of 8 and check

* for every instance: status <= 1 (converged / acceptable) implies that w, f, lam_g and lam_x are all
  finite;
* a NaN in the problem data of an instance (an x0 entry, a target or stage-reference entry of P) ends
  that instance with a failure status (>= 2): no NLP with a NaN parameter has a solution, whatever the
  outputs look like;
* every other instance -- the wave-mate of the poisoned one included -- is bit-identical in w, f,
  lam_g, status and iters to the same batch solved without the NaN.

Problems (single-wave groups only; a NaN that made a branch around a workgroup barrier non-uniform
would be a hang, and the multi-wave collectives are tested in tests/test_gpu_collectives.py with
uniform branching by construction): the unicycle at G = 16, 32, the replicated 32-lane shape and
G = 64, the kinematic bicycle at N = 12, an LTI QP without bounds at N = 20 whose poisoned instance
starts at x0 = 0.  Starts: cold, and warm from the clean converged solve of the same P (the feasible,
complementary start, where only the dropped residual is left).  Sites: x0, a reference entry of P,
a state and an input entry of w0, an entry of lam_g0, an entry of lam_x0 (the kernel may sanitise the
last one through the multiplier push; success with finite outputs is then allowed).

Outcome on one MI355X: see DESIGN.md §3 "What the device tests pin".
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, BAD = 8, 3  # instance 3 shares its wave with instance 2 (G = 32) or with 0, 1, 2 (G = 16)
PROBLEMS = ("unicycle_N10_G16", "unicycle_N20_G32", "unicycle_N20_replicated", "unicycle_N40_G64", "kin_bicycle_N12",
            "lti_unbounded_N20")
COLD_SITES = ("x0", "p_ref")
WARM_SITES = ("x0", "p_ref", "w0_state", "w0_input", "lam_g0", "lam_x0")


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def problem(name):
    """(ocp, P, solver options)"""
    import mpcx
    from mpcx import dist, lti, ode

    if name.startswith("unicycle"):
        N = int(name.split("_")[1][1:])
        policy = 1 if name.endswith(("G16", "G32")) else 0
        return mpcx.unicycle_point_to_point(N=N), dist.config2_inputs(0, B), {"group_policy": policy}
    if name == "kin_bicycle_N12":
        N = 12
        rng = np.random.default_rng(2)
        ocp = ode.kinematic_bicycle_tracking(N=N)
        ref = ode.bicycle_circular_reference(rng.uniform(0, 20 * math.pi, B), 0, N)
        return ocp, ocp.params(ref[:, 0, :3] + rng.normal(0, 0.1, (B, 3)), ref), {}
    assert name == "lti_unbounded_N20"
    rng = np.random.default_rng(7)
    nx, nu, N = 4, 1, 20
    A = rng.normal(size=(nx, nx))
    A *= 0.95 / np.max(np.abs(np.linalg.eigvals(A)))
    Bm = rng.normal(size=(nx, nu))
    lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 2.0, 1.0, 0.5, 0.1])[None], tab=np.zeros(N, np.int32))
    assert not np.isfinite(lin.u_lb + lin.u_ub + lin.x_lb + lin.x_ub).any()  # no bounds at all
    x0 = rng.normal(size=(B, nx))
    x0[BAD] = 0.0  # the solution is w = 0: feasible and optimal from the first iterate
    return lin, lin.params(x0, np.zeros((N, nx + nu))), {}


@functools.lru_cache(maxsize=None)
def clean(name):
    """(solver, ocp, P, clean cold result, warm-start arrays, clean warm result); never modified"""
    import mpcx

    ocp, P, opts = problem(name)
    solver = mpcx.nlpsol(name, "mi355x", ocp, dict(opts, ipopt={"max_iter": 100}))
    cold = solver.solve_batch(P)
    assert cold["status"][BAD] == 0, cold["status"]  # the warm start below is a converged point
    for k in ("w", "f", "lam_g", "lam_x"):
        assert np.isfinite(cold[k]).all()
    start = {"w0": cold["w"].copy(), "lam_g0": cold["lam_g"].copy(), "lam_x0": cold["lam_x"].copy()}
    warm = solver.solve_batch(P, **start)
    for r in (cold, warm, start):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    P.setflags(write=False)
    return solver, ocp, P, cold, start, warm


def poison(ocp, P, start, site):
    """copies of (P, start) with one NaN in instance BAD"""
    nx, nu, N = ocp.nx, ocp.nu, ocp.N
    nz, k = nx + nu, ocp.N // 2
    P = P.copy()
    start = None if start is None else {n: v.copy() for n, v in start.items()}
    if site == "x0":
        P[BAD, 1] = np.nan
    elif site == "p_ref":  # the target (x0_xref) or the reference of stage k (x0_stageref)
        P[BAD, nx + 1 if P.shape[1] == 2 * nx else nx + nz * k + 1] = np.nan
    elif site == "w0_state":  # w = [X_0 | U_0 X_1 | ...]
        start["w0"][BAD, nx + nz * (k - 1) + nu + 1] = np.nan
    elif site == "w0_input":
        start["w0"][BAD, nx + nz * k] = np.nan
    elif site == "lam_g0":
        start["lam_g0"][BAD, nx * k + 1] = np.nan
    else:
        assert site == "lam_x0"
        start["lam_x0"][BAD, nx + nz * k] = np.nan  # an input's bound multiplier
    return P, start


CASES = [(p, "cold", s) for p in PROBLEMS for s in COLD_SITES] + [(p, "warm", s) for p in PROBLEMS for s in WARM_SITES]


@pytest.mark.parametrize("name,start_kind,site", CASES, ids=["-".join(c) for c in CASES])
def test_one_nan_never_ends_as_success(mpcx, name, start_kind, site):
    solver, ocp, P, cold, start, warm = clean(name)
    ref = cold if start_kind == "cold" else warm
    Pn, sn = poison(ocp, P, None if start_kind == "cold" else start, site)
    r = solver.solve_batch(Pn, **(sn or {}))
    finite = np.array([all(np.isfinite(r[k][b]).all() for k in ("w", "f", "lam_g", "lam_x")) for b in range(B)])
    print(f"{name} {start_kind} {site}: status {int(r['status'][BAD])} after {int(r['iters'][BAD])} iterations, outputs "
          f"{'finite' if finite[BAD] else 'not finite'} (clean: status {int(ref['status'][BAD])}, "
          f"{int(ref['iters'][BAD])} iterations)")
    ok = r["status"] <= 1
    assert finite[ok].all(), (r["status"], finite)
    if site in ("x0", "p_ref"):
        assert r["status"][BAD] >= 2, r["status"]
    others = [b for b in range(B) if b != BAD]
    for k in ("w", "f", "lam_g", "status", "iters"):
        np.testing.assert_array_equal(r[k][others], ref[k][others], err_msg=k)
