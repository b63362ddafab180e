"""Time of one sensitivity launch (mpcx_sens_x0_dev, mpcx_sens_p_dev, mpcx_sens_vjp_dev, mpcx_sens_bounds_dev,
mpcx_sens_bounds_vjp_dev, mpcx_sens_weights_dev, mpcx_sens_weights_vjp_dev) next to one lock-step solve of the
same batch.

    python tools/sens_bench.py [B] [reps]      (defaults 1024, 9)

Two shapes: config 2 (unicycle point-to-point, N = 20) and the cart-pole QP at N = 50.  Each batch
is stepped twice (a cold and a warm closed-loop step), then every repetition times one warm
lock-step step (DeviceLoop.step: solve + fused shift), one DeviceLoop.sens_x0 launch, one
DeviceLoop.sens_p launch of m = 3 seeded directions over the whole parameter row and one
DeviceLoop.sens_vjp launch of m = 3 and of m = 1 seeded cotangents over the whole of w, and one
DeviceLoop.sens_bounds launch of m = 3 seeded directions of both bounds and one
DeviceLoop.sens_bounds_vjp launch of the m = 3 cotangents, one DeviceLoop.sens_weights launch of m = 3
seeded per-stage directions of the weight rows and one DeviceLoop.sens_weights_vjp launch of the m = 3
cotangents (per-stage rows and their sum), all at the loop's
resident solution, each with device events, after two warm-up repetitions.  Prints one JSON line per
shape: medians, min-max spreads, and the ratios sens / solve, sens_p / sens_x0 and sens_vjp / sens_p."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-verde_amd"))
import torch  # noqa: E402

import mpcx  # noqa: E402
from mpcx import dist, lti  # noqa: E402
from mpcx.device import DeviceLoop  # noqa: E402

REF_OPTS = {"max_iter": 2000, "acceptable_tol": 1e-8, "acceptable_obj_change_tol": 1e-6}


def shapes(B):
    yield "config2_unicycle_N20", mpcx.unicycle_point_to_point(N=20), dist.config2_inputs(0, B), REF_OPTS
    lin = lti.inverted_pendulum_qp(N=50)
    yield "cartpole_qp_N50", lin, lti.pendulum_params(lin, dist.config5_inputs(0, B), 0.0), {"max_iter": 300}


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for name, ocp, P, opts in shapes(B):
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": opts})
        loop = DeviceLoop(solver, P)
        loop.step()
        loop.step()
        dw, K0, flag = loop.sens_x0()
        m = 3
        dP = torch.from_numpy(np.random.default_rng(0).normal(size=(B, m, loop.P.shape[1]))).to(loop.device)
        dwp, flagp = loop.sens_p(dP)
        gw = torch.from_numpy(np.random.default_rng(1).normal(size=(B, m, loop.w.shape[1]))).to(loop.device)
        gw1 = gw[:, :1].contiguous()
        gP, flagv = loop.sens_vjp(gw)
        gP1, _ = loop.sens_vjp(gw1)
        dlb, dub = (torch.from_numpy(np.random.default_rng(s).normal(size=(B, m, loop.w.shape[1]))).to(loop.device)
                    for s in (2, 3))
        dwb, flagb = loop.sens_bounds(dlb, dub)
        glb, gub, flagbv = loop.sens_bounds_vjp(gw)
        n_wt = solver._h.weight_dims()
        dwt = torch.from_numpy(np.random.default_rng(4).normal(size=(B, m, ocp.N, n_wt))).to(loop.device)
        dww, flagw = loop.sens_weights(dwt)
        gwk, gws, flagwv = loop.sens_weights_vjp(gw)
        its = torch.zeros(B, dtype=torch.int32, device="cuda")
        solve_ms, sens_ms, sensp_ms, vjp_ms, vjp1_ms, it_max = [], [], [], [], [], []
        bnd_ms, bvjp_ms, wt_ms, wvjp_ms = [], [], [], []
        for rep in range(reps + 2):
            a, b, c, d, e, f = ev(), ev(), ev(), ev(), ev(), ev()
            a.record()
            loop.step(iters_out=its)
            b.record()
            c.record()
            loop.sens_x0(dw_out=dw, K0_out=K0, flag_out=flag)
            d.record()
            e.record()
            loop.sens_p(dP, dw_out=dwp, flag_out=flagp)
            f.record()
            g, h, i, j = ev(), ev(), ev(), ev()
            g.record()
            loop.sens_vjp(gw, gP_out=gP, flag_out=flagv)
            h.record()
            i.record()
            loop.sens_vjp(gw1, gP_out=gP1, flag_out=flagv)
            j.record()
            k, l, o, p = ev(), ev(), ev(), ev()
            k.record()
            loop.sens_bounds(dlb, dub, dw_out=dwb, flag_out=flagb)
            l.record()
            o.record()
            loop.sens_bounds_vjp(gw, glbw_out=glb, gubw_out=gub, flag_out=flagbv)
            p.record()
            t, u, v, x = ev(), ev(), ev(), ev()
            t.record()
            loop.sens_weights(dwt, dw_out=dww, flag_out=flagw)
            u.record()
            v.record()
            loop.sens_weights_vjp(gw, gWk_out=gwk, gW_out=gws, flag_out=flagwv)
            x.record()
            torch.cuda.synchronize()
            if rep >= 2:
                solve_ms.append(a.elapsed_time(b))
                sens_ms.append(c.elapsed_time(d))
                sensp_ms.append(e.elapsed_time(f))
                vjp_ms.append(g.elapsed_time(h))
                vjp1_ms.append(i.elapsed_time(j))
                bnd_ms.append(k.elapsed_time(l))
                bvjp_ms.append(o.elapsed_time(p))
                wt_ms.append(t.elapsed_time(u))
                wvjp_ms.append(v.elapsed_time(x))
                it_max.append(int(its.max()))
        solve_ms, sens_ms, sensp_ms = np.array(solve_ms), np.array(sens_ms), np.array(sensp_ms)
        vjp_ms, vjp1_ms = np.array(vjp_ms), np.array(vjp1_ms)
        bnd_ms, bvjp_ms = np.array(bnd_ms), np.array(bvjp_ms)
        wt_ms, wvjp_ms = np.array(wt_ms), np.array(wvjp_ms)
        q = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4),  # noqa: E731
                       "max": round(float(v.max()), 4)}
        print(json.dumps({"shape": name, "N": ocp.N, "B": B, "reps": reps, "lockstep_step_ms": q(solve_ms),
                          "sens_x0_ms": q(sens_ms), "ratio_sens_over_step": round(float(np.median(sens_ms) / np.median(solve_ms)), 3),
                          "sens_p_m": m, "sens_p_ms": q(sensp_ms),
                          "ratio_sens_p_over_sens_x0": round(float(np.median(sensp_ms) / np.median(sens_ms)), 3),
                          "sens_vjp_m": m, "sens_vjp_ms": q(vjp_ms), "sens_vjp_m1_ms": q(vjp1_ms),
                          "ratio_sens_vjp_over_sens_p": round(float(np.median(vjp_ms) / np.median(sensp_ms)), 3),
                          "irregular_sens_vjp": int(flagv.sum()),
                          "sens_bounds_m": m, "sens_bounds_ms": q(bnd_ms), "sens_bounds_vjp_ms": q(bvjp_ms),
                          "ratio_sens_bounds_over_sens_p": round(float(np.median(bnd_ms) / np.median(sensp_ms)), 3),
                          "ratio_sens_bounds_vjp_over_sens_vjp": round(float(np.median(bvjp_ms) / np.median(vjp_ms)), 3),
                          "irregular_sens_bounds": int(flagb.sum()), "irregular_sens_bounds_vjp": int(flagbv.sum()),
                          "sens_weights_m": m, "sens_weights_ms": q(wt_ms), "sens_weights_vjp_ms": q(wvjp_ms),
                          "ratio_sens_weights_over_sens_bounds": round(float(np.median(wt_ms) / np.median(bnd_ms)), 3),
                          "ratio_sens_weights_vjp_over_sens_bounds_vjp": round(float(np.median(wvjp_ms) / np.median(bvjp_ms)), 3),
                          "irregular_sens_weights": int(flagw.sum()), "irregular_sens_weights_vjp": int(flagwv.sum()),
                          "ipm_iterations_of_the_steps_max": it_max, "irregular": int(flag.sum()),
                          "irregular_sens_p": int(flagp.sum()),
                          "status_gt1": int((loop.status > 1).sum()), "source_hash": mpcx._lib.source_hash()}), flush=True)


if __name__ == "__main__":
    main()
