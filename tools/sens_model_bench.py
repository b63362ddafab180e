"""Time of one model-sensitivity launch (mpcx_sens_model_dev, mpcx_sens_model_vjp_dev) next to the weight pair
(mpcx_sens_weights_dev, mpcx_sens_weights_vjp_dev) and one lock-step solve of the same batch.

    python tools/sens_model_bench.py [B] [reps]      (defaults 1024, 9)

Two shapes, the config-equivalent ODE batches of bench.py --model: the kinematic bicycle on the config-3 circle at
N = 30 and the 6-state bicycle on the scaled lane change at N = 50.  Each batch is stepped twice (a cold and a warm closed-loop step), then every
repetition times one warm lock-step step (DeviceLoop.step: solve + fused shift), one DeviceLoop.sens_weights
and sens_weights_vjp launch and one DeviceLoop.sens_model and sens_model_vjp launch of m = 3 seeded per-stage
directions / cotangents (per-stage rows and their sum), all at the loop's resident solution, each with device events,
after two warm-up repetitions.  Prints one JSON line per shape: medians, min-max spreads and ratios."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-verde_amd"))
import torch  # noqa: E402

import mpcx  # noqa: E402
from mpcx import dist  # noqa: E402
from mpcx.device import DeviceLoop  # noqa: E402


def shapes(B):
    ocp = mpcx.kinematic_bicycle_tracking(N=30)
    yield "kin_bicycle_N30", ocp, dist.config3_bicycle_inputs(0, B, N=30)[1]
    ocp = mpcx.dynamic_bicycle_lane_change(N=50)
    t0, x0, (X, Y, V) = dist.config4_bicycle_inputs(0, B)
    refs = np.stack([mpcx.ode.dyn_bicycle_references(X, Y, V, int(t), 50).reshape(-1) for t in t0])
    yield "dyn_bicycle_N50", ocp, ocp.params(x0, refs)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    m = 3
    for name, ocp, P in shapes(B):
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": {"max_iter": 3000}})
        loop = DeviceLoop(solver, P)
        loop.step()
        loop.step()
        its = torch.zeros(B, dtype=torch.int32, device=loop.device)
        rng = np.random.default_rng(5)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(loop.device)  # noqa: E731
        gw = dev(rng.normal(size=(B, m, loop.w.shape[1])))
        dwt = dev(rng.normal(size=(B, m, ocp.N, solver._h.weight_dims())))
        n_th = solver._h.model_dims()
        dth = dev(rng.normal(size=(B, m, ocp.N, n_th)) * np.array(ocp.par, float)[:n_th])
        calls = {
            "lockstep_step": lambda: loop.step(iters_out=its),
            "sens_weights": lambda o=loop.sens_weights(dwt): loop.sens_weights(dwt, dw_out=o[0], flag_out=o[1]),
            "sens_weights_vjp": lambda o=loop.sens_weights_vjp(gw): loop.sens_weights_vjp(gw, gWk_out=o[0], gW_out=o[1], flag_out=o[2]),
            "sens_model": lambda o=loop.sens_model(dth): loop.sens_model(dth, dw_out=o[0], flag_out=o[1]),
            "sens_model_vjp": lambda o=loop.sens_model_vjp(gw): loop.sens_model_vjp(gw, gThk_out=o[0], gTh_out=o[1], flag_out=o[2]),
        }
        ms, it_max = {k: [] for k in calls}, []
        for rep in range(reps + 2):
            evs = {}
            for k, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(loop.stream):
                    a.record()
                    fn()
                    b.record()
                evs[k] = (a, b)
            torch.cuda.synchronize()
            if rep >= 2:
                for k, (a, b) in evs.items():
                    ms[k].append(a.elapsed_time(b))
                it_max.append(int(its.max()))
        q = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),  # noqa: E731
                       "max": round(float(np.max(v)), 4)}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        flags = int(loop.sens_model(dth)[1].sum()), int(loop.sens_model_vjp(gw)[2].sum())
        print(json.dumps({"shape": name, "N": ocp.N, "B": B, "m": m, "reps": reps, "n_th": n_th,
                          **{k + "_ms": q(v) for k, v in ms.items()},
                          "ratio_sens_model_over_sens_weights": round(med["sens_model"] / med["sens_weights"], 2),
                          "ratio_sens_model_vjp_over_sens_weights_vjp": round(med["sens_model_vjp"] / med["sens_weights_vjp"], 2),
                          "ratio_sens_model_vjp_over_lockstep_step": round(med["sens_model_vjp"] / med["lockstep_step"], 3),
                          "ipm_iterations_of_the_steps_max": it_max,
                          "irregular_sens_model": flags[0], "irregular_sens_model_vjp": flags[1],
                          "status_gt1": int((loop.status > 1).sum()), "source_hash": mpcx._lib.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
