"""Closed-loop rate of the path-frame bicycle MPC (model 7): solves/s of multi-step launches and
microseconds per IPM iteration of lock-step launches.

    python tools/path_bicycle_bench.py [B] [steps] [reps]      (defaults 1024, 20, 7)

The batch keeps B seeded instances on paths of constant curvature (|kappa| <= 0.05 /m, the
rows the same at every step) at 3-10 m/s, started up to 1 m beside the path with up to 0.1 rad of
steering applied, N = 20.  Timed with device events
after two warm-up repetitions of every launch shape; every repetition restarts from the same
state.  Prints one JSON line: the median and the min-max spread over the repetitions.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-verde_amd"))
import torch  # noqa: E402

import mpcx  # noqa: E402
from mpcx import ode  # noqa: E402
from mpcx.device import DeviceLoop  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    N = 20
    rng = np.random.default_rng(0)
    ocp = ode.path_bicycle_lane_keeping(N=N)
    rows = np.zeros((B, N, 6))
    rows[..., 0] = rng.uniform(-0.5, 0.5, (B, 1))
    rows[..., 1] = rng.uniform(-0.05, 0.05, (B, 1))
    rows[..., 2] = rng.uniform(3.0, 10.0, (B, 1))
    rows[..., 3] = rng.uniform(-0.05, 0.05, (B, 1))
    x0 = np.stack([rows[:, 0, 0] + rng.uniform(-1, 1, B), rows[:, 0, 1] + rng.normal(0, 0.05, B),
                   rows[:, 0, 2] + rng.normal(0, 0.5, B)], axis=1)
    P0 = ode.path_bicycle_params(ocp, x0, rng.uniform(-0.1, 0.1, B), rows)
    solver = mpcx.nlpsol("bench", "mi355x", ocp)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    run_ms, lock_ms, lock_it = [], [], None
    for rep in range(reps + 2):
        loop = DeviceLoop(solver, P0)
        a, b = ev(), ev()
        a.record()
        st, it = loop.run(K)
        b.record()
        torch.cuda.synchronize()
        loop = DeviceLoop(solver, P0)
        its = torch.zeros((K, B), dtype=torch.int32, device="cuda")
        c, d = ev(), ev()
        c.record()
        for s in range(K):
            loop.step(iters_out=its[s])
        d.record()
        torch.cuda.synchronize()
        if rep >= 2:
            run_ms.append(a.elapsed_time(b))
            lock_ms.append(c.elapsed_time(d))
        lock_it = its.cpu().numpy()
        status = st.cpu().numpy()
    run_ms, lock_ms = np.array(run_ms), np.array(lock_ms)
    itmax = float(lock_it.max(axis=1).sum())  # a lock-step launch lasts as long as its slowest instance
    G, Rr, kname = solver._h.launch_shape(B)
    rate = B * K / (run_ms * 1e-3)
    us = lock_ms * 1e3 / itmax
    print(json.dumps({
        "model": "path_bicycle", "N": N, "B": B, "steps": K, "reps": reps, "kernel": kname, "lanes": G, "replicas": Rr,
        "solves_per_s_run": {"median": round(float(np.median(rate)), 1), "min": round(float(rate.min()), 1),
                             "max": round(float(rate.max()), 1)},
        "solves_per_s_lockstep": round(float(B * K / (np.median(lock_ms) * 1e-3)), 1),
        "us_per_ipm_iteration": {"median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2),
                                 "max": round(float(us.max()), 2)},
        "iters_mean": round(float(lock_it.mean()), 2), "iters_max": int(lock_it.max()),
        "status_gt1": int((status > 1).sum()), "source_hash": mpcx._lib.source_hash()}))


if __name__ == "__main__":
    main()
