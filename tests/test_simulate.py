"""The closed-loop arrays mpcx records are the ones the reference's visualisation animates
("the driver loop ... plus simulation_code.simulate, must run unchanged on these
outputs").

tests/golden/simulate_frames.npz holds what the reference's ``simulate(cat_states, cat_controls, t,
step_horizon, N, reference)`` drew, frame by frame, when it ran unchanged on the arrays of
``reference_loop_log`` below (recorded by tests/golden/make_simulate_frames.py: the data of the path
line, the horizon line and the pose polygons after every frame, the axes' limits, and the shapes
of the arrays it accepted; the script itself is not part of this repository).  The arrays come from
mpcx/record.py's ClosedLoopLog -- the class the GPU closed-loop test
(tests/test_gpu_parity.py::test_casadi_call_shapes_and_closed_loop) fills from mpcx.nlpsol --
here filled by the reference's driver loop (Casadi/multiple_shooting_casadi.py:224-298, its
stacked-layout warm start included) run on the C++ CPU oracle, which reproduces 1exemplo.xlsx.
The test rebuilds the log and holds it to the recording: same shapes and dtypes as the arrays the
script accepted, one frame per entry of ``t``, and every drawn path point and horizon node equal to
the log's entry.  CPU only.

Tolerance: the recording and the rebuilt log are the same oracle loop, each solve converged to
IPOPT's tol 1e-8, possibly on another CPU or compiler; 1e-6 absolute is the bound that pins this
loop to the reference's exported rows below, on states of magnitude up to 10.
"""
import math
import os

import numpy as np

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulate_frames.npz")
TOL = 1e-6


def reference_loop_log(N=10, T=0.2):
    """The driver loop of multiple_shooting_casadi.py:224-298 on the C++ oracle, recorded by
    ClosedLoopLog as the script records cat_states / cat_controls / t / times (:210-270)."""
    from mpcx.record import ClosedLoopLog
    from oracle import ipm_ref, nlp_ref

    ocp = nlp_ref.UnicycleOCP(N=N)
    state_init = np.zeros(3)
    state_target = np.array([10.0, 10.0, 0.0])
    w0 = np.zeros(3 + 5 * N)
    log = ClosedLoopLog(3, 2, N, T, state_init)
    mpc_iter, t0 = 0, 0.0
    while np.linalg.norm(state_init - state_target) > 1e-1 and mpc_iter * T < 20:
        P = np.concatenate([state_init, state_target])[None, :]
        r = ipm_ref.solve(ocp, P, w0=w0[None, :], max_iter=2000, acceptable_tol=1e-8, acceptable_obj_change_tol=1e-6)
        assert r["status"][0] <= 1
        x = r["w"][0]
        u = np.array([x[3 + 5 * k:5 + 5 * k] for k in range(N)]).T
        X0 = np.array([x[0:3]] + [x[5 + 5 * k:8 + 5 * k] for k in range(N)]).T
        log.record(x, t0, wall_time=0.0)
        t0 += T
        state_init, _ = nlp_ref.F(P[0, 0:3], u[:, 0], state_target, ocp)
        u0 = np.hstack([u[:, 1:], u[:, -1:]])
        X0 = np.hstack([X0[:, 1:], X0[:, -1:]])
        w0 = np.concatenate([X0.T.reshape(-1), u0.T.reshape(-1)])  # the script's stacked layout (:284-287)
        mpc_iter += 1
    return log, mpc_iter


def test_closed_loop_log_reproduces_recorded_simulate_frames(golden):
    N, T = 10, 0.2
    log, iters = reference_loop_log(N, T)
    rows = np.array(golden["multiple_shooting"]["rows"])
    rec = np.load(FRAMES)
    assert iters == 84 and log.cat_states.shape == (3, N + 1, 85)
    # the arrays are the reference's (cat_states[:, 0, :] = its exported state rows)
    assert np.max(np.abs(log.cat_states[:, 0, :].T - rows[:, 0:3])) < TOL
    # the call the recording made is the script's own (commented) one, :312-313:
    # simulate(cat_states, cat_controls, times, T, N, reference), on arrays shaped and typed like the log's
    assert int(rec["N"]) == N and float(rec["step_horizon"]) == T
    for a, shape in ((log.cat_states, rec["shape_cat_states"]), (log.cat_controls, rec["shape_cat_controls"]),
                     (log.times, rec["shape_t"]), (log.t, rec["shape_t"])):
        assert a.dtype == np.float64 and a.shape == tuple(shape)
    n = int(rec["frames"])
    assert n == len(log.times) == len(log.t) == 85  # one frame per record
    assert rec["horizon"].shape == (n, 2, N + 1) and rec["path_x"].shape == rec["path_y"].shape == (n, n)
    # every frame's horizon line is that record's predicted (x, y) trajectory ...
    assert np.max(np.abs(rec["horizon"] - log.cat_states[0:2].transpose(2, 0, 1))) < TOL
    # ... and its path line the first predicted node of every record so far (nothing drawn beyond)
    first = log.cat_states[0:2, 0, :]
    for c, drawn in enumerate((rec["path_x"], rec["path_y"])):
        want = np.where(np.tri(n, dtype=bool), first[c][None, :], np.nan)
        assert np.array_equal(np.isnan(drawn), np.isnan(want))
        assert np.nanmax(np.abs(drawn - want)) < TOL
    # what it drew stays inside the axes it set from `reference`; the vehicle polygon moves with the pose
    lo, hi = float(rec["xlim"][0]), float(rec["xlim"][1])
    assert tuple(rec["ylim"]) == (lo, hi) and lo <= rec["horizon"].min() and rec["horizon"].max() <= hi
    assert np.array_equal(rec["reference"], [0.0, 0.0, 0.0, 10.0, 10.0, 0.0])
    assert rec["vehicle"].shape == (n, 4, 2) and np.all(np.isfinite(rec["vehicle"]))
    assert math.isclose(float(log.t[-1, 0]), 83 * T)
