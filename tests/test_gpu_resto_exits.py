"""GPU tests of the restoration phase's exits and lanes (mpc-verde_amd/csrc/resto.h recover(), the
park / resume plumbing of kernels.h) on infeasible problems.

The family (tests/helpers/resto_family.py; tests/test_resto_cpu.py runs the CPU oracle on it): a
per-instance bound puts X_1 outside what one step can reach, so every instance goes through soft
restoration into the restoration phase and can only leave it by a failure exit -- IPOPT status 4
(local infeasibility), 3 (restoration failed), 2 (max_iter) or 5 (delta > kDwMax).  The unicycle at
N = 2, 10, 20, 40, 70, 130 (lane groups 16, 16, 32, 64, 128, 256, with group_policy 1; policy 0
widens the small groups, 32 lanes to the replicated 32 x 2 shape), the kinematic bicycle (N = 5, 30),
the cart-pole (N = 5, 70) and the 6-state bicycle (N = 5, 20): recover() for NX = 3, 4 and 6.
max_iter = 300.

What is asserted of the device, with both group policies:
1. no infeasible instance reports success: status in {2, 3, 4, 5}, iters <= max_iter, w, lam_g,
   lam_x, f finite;
2. the resume launch ran: with restoration off the same instances end at status 3 with other w;
3. the end point is the oracle's: the maximum constraint violation of the returned w, by the
   oracle's constraint function, equals that of the oracle's own end point (and lo - 0.2 for the
   unicycle at heading 0) to 10 x the largest spread of the oracle's end-point violation over the
   scalings 1 + {0, 1e-13, -1e-13, 3e-13} of P (instances whose every scaled oracle run ends at 3
   or 4; the three others are left out);
4. the status is the oracle's wherever the oracle's (status, iterations) is the same under the
   seven scalings 1 + {0, +-1e-13, +-3e-13, +-1e-12} (resto_family.py says why seven); iteration
   counts are printed;
5. a status-5 instance (unicycle, heading 0, lo = 0.25, N = 20 and 40) and one with max_iter two
   above the iteration at which the phase is entered: the oracle's status and iteration count;
6. lanes do not leak: a batch interleaving feasible and infeasible instances (B = 5 for G >= 64,
   33 below, so the last wave has an empty group) gives every instance the bits of its solo
   solve, under either policy.  The feasible instances carry the problem's bounds and a bound
   of +-1e3 around X_1's first state: finite and never active, so that their solo solve runs the
   same state-bounded kernel as the batch (a batch that mixes state-bounded and unbounded
   instances runs the state-bounded unit, tests/test_gpu_instance_bounds.py).

Measured on the CPU oracle: largest spread 2.4e-8 (cart-pole, N = 70, d = 2), hence the tolerance
2.4e-7; 4 of the 72 instances stable under the seven scalings (7 under the first four), 3 left out
of check 3.
Measured on one MI355X (the two policies give the same bits everywhere, so one row per case;
statuses of the case's six instances):

case (group, policy 1)    device statuses      oracle statuses
unicycle N = 2   (16)     4 3 4 3 4 3          3 3 4 4 4 4
unicycle N = 10  (16)     3 3 4 3 4 3          4 3 4 3 4 3
unicycle N = 20  (32)     3 3 4 3 2 3          3 3 4 3 4 3
unicycle N = 40  (64)     4 3 4 3 3 3          4 3 4 3 4 3
unicycle N = 70  (128)    3 3 4 3 4 3          4 3 4 3 4 3
unicycle N = 130 (256)    3 3 4 3 4 3          3 3 4 3 4 3
kin. bicycle N = 5  (16)  4 3 4 3 3 3          4 3 3 3 3 3
kin. bicycle N = 30 (32)  3 3 3 3 4 3          3 3 3 3 4 3
cart-pole N = 5  (16)     3 3 3 3 3 3          3 4 4 4 3 3
cart-pole N = 70 (128)    4 3 4 4 4 4          4 4 4 3 4 3
6-state bic. N = 5  (16)  3 4 3 4 4 4          4 4 3 4 4 4
6-state bic. N = 20 (32)  4 5 4 4 4 4          4 5 4 4 4 4

Every end-point violation is within 2.4e-8 of the oracle's (tolerance 2.4e-7; each test takes
under a second once the oracle's runs, 13 s on the CPU, are there).  On the 4 stable
instances (unicycle N = 2 and 130, cart-pole N = 70: status 4; 6-state bicycle N = 20: status 5)
the device has the oracle's status, and 0 of their iteration counts differ.  Status 5 at (5, 57)
and (5, 36), status 2 at (2, 8): the oracle's.  Status 2 also appears inside the family (unicycle
N = 20, theta = -2, lo = 0.5: 300 iterations, where the oracle stops at (4, 17) -- the instance
is not stable: the oracle takes 140 and 275 iterations under two of the scalings).

The first run of test_lanes_do_not_leak and of the policy comparison failed on the unicycle's 16-
and 32-lane groups (N = 2, 10, 20): the inline soft restoration step (kernels.h) ran on the whole
wave once one group of the wave wanted it and overwrote the derivative arrays of its wave mates,
so a feasible instance next to an infeasible one differed from its solo solve.  The step now runs
on the groups that take it only.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resto_family as rf  # noqa: E402

KEYS = ("w", "f", "lam_g", "lam_x", "status", "iters")
CASES = rf.all_cases()
IDS = [f"{m}-N{N}" for m, N in CASES]


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


def solver_of(mpcx, ocp, policy=0, restoration=True, max_iter=rf.MAX_ITER):
    return mpcx.nlpsol("resto", "mi355x", ocp, {"ipopt": {"max_iter": max_iter}, "group_policy": policy,
                                                "restoration": restoration})


def check_failed_exit(r, max_iter, what):
    assert np.all((r["status"] >= 2) & (r["status"] <= 5)), (what, r["status"])
    assert np.all(r["iters"] <= max_iter), (what, r["iters"])
    for k in ("w", "lam_g", "lam_x", "f"):
        assert np.all(np.isfinite(r[k])), (what, k)


@pytest.mark.parametrize("model,N", CASES, ids=IDS)
def test_infeasible_instances_end_where_the_oracle_ends(mpcx, model, N):
    c, o = rf.case(model, N), rf.oracle_case(model, N)
    tol, _ = rf.tolerance()
    ocp, P, lb, ub = c["ocp"], c["P"], c["lb"], c["ub"]
    B = len(P)
    res = []
    for policy in (0, 1):
        on = solver_of(mpcx, ocp, policy)
        shape = on._h.launch_shape(B)[:2]
        r = on.solve_batch(P, lbw=lb, ubw=ub)
        off = solver_of(mpcx, ocp, policy, restoration=False).solve_batch(P, lbw=lb, ubw=ub)
        res.append(r)
        what = f"{model} N={N} policy {policy} (launch shape {shape[0]} x {shape[1]})"
        print(f"{what}: device (status, iterations) {list(zip(r['status'].tolist(), r['iters'].tolist()))}, oracle "
              f"{list(zip(o['status'][0].tolist(), o['iters'][0].tolist()))}; without restoration "
              f"{list(zip(off['status'].tolist(), off['iters'].tolist()))}")
        check_failed_exit(r, rf.MAX_ITER, what)  # 1
        assert np.all(off["status"] == 3), (what, off["status"])  # 2
        for b in range(B):
            assert r["w"][b].tobytes() != off["w"][b].tobytes(), (what, b)
        for b in range(B):  # 3
            v = rf.violation(ocp, r["w"][b], P[b])
            print(f"  {c['label'][b]}: violation {v:.12g}, oracle {o['viol'][0, b]:.12g} (difference "
                  f"{v - o['viol'][0, b]:.1e}, tolerance {tol:.1e}){'' if o['asserted'][b] else ' -- left out'}")
            if o["asserted"][b]:
                assert abs(v - o["viol"][0, b]) <= tol, (what, b, v, o["viol"][0, b])
                if model == "unicycle" and c["theta"][b] == 0.0:
                    assert abs(v - rf.geometric_minimum(c["lo"][b], 0.0)) <= tol, (what, b, v)
        st = np.flatnonzero(o["stable"])  # 4
        n_it = int(np.sum(r["iters"][st] != o["iters"][0, st]))
        print(f"  stable instances {st.tolist()}: {n_it} iteration counts differ from the oracle")
        assert np.array_equal(r["status"][st], o["status"][0, st]), (what, st, r["status"][st], o["status"][0, st])
    assert_same_bits(res[0], res[1], f"{model} N={N}: the two group policies")  # 6


def test_launch_shapes_at_N20(mpcx):
    """The two policies run the replicated 32 x 2 and the narrow 32 x 1 kernels on the small batches
    used here."""
    ocp = rf.case("unicycle", 20)["ocp"]
    for B in (6, 33):
        assert solver_of(mpcx, ocp, 0)._h.launch_shape(B)[:2] == (32, 2)
        assert solver_of(mpcx, ocp, 1)._h.launch_shape(B)[:2] == (32, 1)


@pytest.mark.parametrize("N", [20, 40])
def test_status5_as_the_oracle(mpcx, N):
    """delta > kDwMax inside the phase: the unicycle at heading 0 with lo = 0.25; the oracle ends at
    status 5 at the same iteration under every scaling, and so does the device."""
    c, o = rf.status5_case(N)
    assert np.all(o["status"] == 5) and o["stable"][0]
    for policy in (0, 1):
        r = solver_of(mpcx, c["ocp"], policy).solve_batch(c["P"], lbw=c["lb"], ubw=c["ub"])
        print(f"unicycle N={N} lo=0.25 policy {policy}: device ({int(r['status'][0])}, {int(r['iters'][0])}), oracle "
              f"({int(o['status'][0, 0])}, {int(o['iters'][0, 0])})")
        check_failed_exit(r, rf.MAX_ITER, f"N={N} policy {policy}")
        assert r["status"][0] == 5 and r["iters"][0] == o["iters"][0, 0]


def test_max_iter_inside_the_phase_as_the_oracle(mpcx):
    c, b, k, st_off, ref = rf.max_iter_case()
    assert st_off == 3 and ref["status"][0] == 2 and ref["iters"][0] == k + 2
    P, lb, ub = c["P"][b:b + 1], c["lb"][b:b + 1], c["ub"][b:b + 1]
    for policy in (0, 1):
        off = solver_of(mpcx, c["ocp"], policy, restoration=False).solve_batch(P, lbw=lb, ubw=ub)
        assert off["status"][0] == 3 and off["iters"][0] == k  # the phase is entered at the oracle's iteration
        r = solver_of(mpcx, c["ocp"], policy, max_iter=k + 2).solve_batch(P, lbw=lb, ubw=ub)
        print(f"{c['label'][b]} max_iter {k + 2} policy {policy}: device ({int(r['status'][0])}, {int(r['iters'][0])})")
        check_failed_exit(r, k + 2, f"policy {policy}")
        assert r["status"][0] == 2 and r["iters"][0] == k + 2


@pytest.mark.parametrize("model,N", CASES, ids=IDS)
def test_lanes_do_not_leak(mpcx, model, N):
    c = rf.case(model, N)
    ocp, i1 = c["ocp"], c["i1"]
    B = 5 if c["G"] >= 64 else 33
    # unique rows: the case's infeasible instances, and their P with the problem's bounds (and a
    # finite, inactive bound on X_1's first state)
    rows = [(c["P"][b], c["lb"][b], c["ub"][b], False) for b in range(len(c["P"]))]
    for b in range(0, len(c["P"]), 2):
        lo, hi = c["lb0"].copy(), c["ub0"].copy()
        lo[i1], hi[i1] = max(lo[i1], c["P"][b][0] - 1e3), min(hi[i1], c["P"][b][0] + 1e3)
        rows.append((c["P"][b], lo, hi, True))
    n_inf, n_feas = len(c["P"]), len(rows) - len(c["P"])
    pick = [(n_inf + (j // 2) % n_feas) if j % 2 == 0 else (j // 2) % n_inf for j in range(B)]  # feasible first
    P, lb, ub = (np.stack([rows[j][q] for j in pick]) for q in range(3))
    feas = np.array([rows[j][3] for j in pick])
    s0, s1 = solver_of(mpcx, ocp, 0), solver_of(mpcx, ocp, 1)
    solo = {j: s0.solve_batch(rows[j][0][None], lbw=rows[j][1], ubw=rows[j][2]) for j in sorted(set(pick))}
    for policy, s in ((0, s0), (1, s1)):
        r = s.solve_batch(P, lbw=lb, ubw=ub)
        print(f"{model} N={N} B={B} policy {policy} launch shape {s._h.launch_shape(B)[:2]}: statuses "
              f"{r['status'].tolist()}")
        assert np.all(r["status"][feas] == 0), r["status"]
        assert np.all((r["status"][~feas] >= 2) & (r["status"][~feas] <= 5)), r["status"]
        for i, j in enumerate(pick):
            assert_same_bits(r, solo[j], f"{model} N={N} policy {policy}, instance {i} (row {j})", rows=slice(i, i + 1))
