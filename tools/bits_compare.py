#!/usr/bin/env python3
"""Results of one library build for a bit-for-bit comparison with another (A/B of a change that must
not change any result), saved to an .npz.

    MPCX_LIB=... MPCX_ALLOW_STALE_LIB=1 python tools/bits_compare.py {c2,c5,dyn,sens} OUT.npz
    python tools/bits_compare.py --diff A.npz B.npz

c2, c5, dyn: a cold solve_batch of a bench workload's batch and a 3-step device closed loop.

sens: every output array and flag of the nine sensitivity calls through ``Solver``, through ``DeviceLoop``
and through raw ctypes calls of their eighteen C entry points, and the ``mpcx_last_error`` text of a fixed
list of refused calls (A/B of the plumbing between the caller and the kernels; copied into another
tree, the script compares that tree's Python layers too).  B = 5 (a partial last block at every lane
group) of the unicycle at N = 15 (16 lanes), the kinematic bicycle at N = 20 (32 lanes), the 6-state
bicycle at N = 40 (64 lanes), the path-frame bicycle at N = 20 (no sens_p / sens_vjp) and a double
integrator padded into LinearModel<4,1> at N = 10; m = 1, nx and, through ``Solver``, nx + 2 columns; rows
shared by the stages and per stage; each ``*_vjp`` with the per-stage output, the sum, and both; no
bounds, bounds shared by the batch and per instance; the loop's resident point and a saved one.
"""
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-verde_amd"))
import numpy as np  # noqa: E402

if sys.argv[1] == "--diff":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    def same(k):  # (bits: NaN rows of flagged instances included)
        return (k in a.files and k in b.files and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
                and a[k].tobytes() == b[k].tobytes())

    keys = list(a.files) + [k for k in b.files if k not in a.files]
    bad = [k for k in keys if not same(k)]
    for k in keys if len(keys) <= 40 else bad:
        print(k, "DIFFERENT" if k in bad else "identical")
    print(f"{len(keys) - len(bad)} of {len(keys)} arrays identical")
    sys.exit(1 if bad else 0)

import torch  # noqa: E402

import mpcx  # noqa: E402
from mpcx import _lib, ode  # noqa: E402
from mpcx import dist as mdist  # noqa: E402
from mpcx.device import DeviceLoop  # noqa: E402

work, out = sys.argv[1], sys.argv[2]


# ---- the sens workload ---------------------------------------------------------------------------
def sens_problems():
    """(name, ocp, P (5, n_p), ipopt options) of the five shapes."""
    B, rng = 5, np.random.default_rng(7)
    ref_opts = {"max_iter": 2000, "acceptable_tol": 1e-8, "acceptable_obj_change_tol": 1e-6}
    P = np.zeros((B, 6))
    P[:, 0:2], P[:, 2] = rng.uniform(-0.3, 0.3, (B, 2)), rng.uniform(-0.5, 0.5, B)
    P[:, 3], P[:, 4], P[:, 5] = rng.uniform(1.0, 2.0, B), rng.uniform(0.5, 1.5, B), rng.uniform(-0.3, 0.3, B)
    yield "unicycle_N15", mpcx.unicycle_point_to_point(N=15), P, ref_opts
    ocp = ode.kinematic_bicycle_tracking(N=20)
    ref = ode.bicycle_circular_reference(rng.uniform(0, 20 * math.pi, B), 0, 20)
    yield "kin_bicycle_N20", ocp, ocp.params(ref[:, 0, :3] + rng.normal(0, 0.1, (B, 3)), ref), {"max_iter": 500}
    ocp = ode.dynamic_bicycle_lane_change(N=40)
    ref = np.zeros((B, 40, 8))
    ref[..., 0], ref[..., 3] = 6.0 * ocp.T * np.arange(40), 6.0
    x0 = ref[:, 0, :6] + rng.normal(0, 1, (B, 6)) * np.array([0.2, 0.2, 0.05, 0.3, 0.1, 0.05])
    yield "dyn_bicycle_N40", ocp, ocp.params(x0, ref), {"max_iter": 1000}
    ocp = ode.path_bicycle_lane_keeping(N=20)
    rows = np.zeros((B, 20, 6))
    rows[..., 0], rows[..., 2] = rng.uniform(-0.5, 0.5, (B, 1)), rng.uniform(5.0, 10.0, (B, 1))
    x = np.stack([rows[:, 0, 0] + rng.uniform(-0.3, 0.3, B), rng.normal(0, 0.02, B),
                  rows[:, 0, 2] + rng.normal(0, 0.3, B)], axis=1)
    yield "path_bicycle_N20", ocp, ode.path_bicycle_params(ocp, x, 0.0, rows), {"max_iter": 1000, "tol": 1e-8}
    T, N = 0.1, 10
    lin = mpcx.LinearOCP(N=N, A=np.array([[1.0, T], [0.0, 1.0]])[None], B=np.array([[0.5 * T * T], [T]])[None],
                         W=np.diag([1.0, 0.1, 0.01])[None], tab=np.zeros(N, np.int32), u_lb=(-1.0,), u_ub=(1.0,))
    x0 = np.array([[5.0, 0.0], [2.0, 2.0], [-1.0, 0.0], [-6.0, 0.5], [-0.2, 0.1]])
    yield "padded_dint_N10", lin, lin.params(x0, np.zeros((N, 3))), {"max_iter": 300}


def box_around(w):
    """Finite bounds every instance's w lies strictly inside: (shared lb, ub), (per-instance lb, ub)."""
    step = 0.25 * np.arange(w.shape[0])[:, None]
    return (w.min(axis=0) - 1.0, w.max(axis=0) + 1.0), (w - 1.0 - step, w + 2.0 + step)


def sens_solver(res, tag, solver, P, r, rng):
    """The nine Solver methods: m = 1, nx, nx + 2 (the chunk loop); bounds none / shared / per instance."""
    ocp = solver.ocp
    nx, nu, N, nw, B = ocp.nx, ocp.nu, ocp.N, solver.n_w, P.shape[0]
    shared, each = box_around(r["w"])

    def keep(name, call):
        try:
            for k, v in call().items():
                res[f"{tag}/solver/{name}/{k}"] = v
        except (ValueError, _lib.MpcxError) as e:  # (a refusal is a result too: its text)
            res[f"{tag}/solver/{name}/refused"] = np.array(f"{type(e).__name__}: {e}")

    for bname, (lb, ub) in (("none", (None, None)), ("shared", shared), ("each", each)):
        keep(f"x0_{bname}", lambda: solver.sens_x0(P, r, lbw=lb, ubw=ub))
        for m in (1, nx, nx + 2):
            t = f"m{m}_{bname}"
            gw, dlb, dub = (rng.normal(size=(B, m, nw)) for _ in range(3))
            keep(f"p_{t}", lambda: solver.sens_p(P, r, rng.normal(size=(B, m, solver.n_p)), lbw=lb, ubw=ub))
            keep(f"vjp_{t}", lambda: solver.sens_vjp(P, r, gw, lbw=lb, ubw=ub))
            keep(f"bounds_{t}", lambda: solver.sens_bounds(P, r, dlb, dub, lbw=lb, ubw=ub))
            keep(f"bounds_lower_only_{t}", lambda: solver.sens_bounds(P, r, dlb[:, 0], None, lbw=lb, ubw=ub))
            keep(f"bounds_vjp_{t}", lambda: solver.sens_bounds_vjp(P, r, gw, lbw=lb, ubw=ub))
            keep(f"weights_vjp_{t}", lambda: solver.sens_weights_vjp(P, r, gw, lbw=lb, ubw=ub))
            keep(f"model_vjp_{t}", lambda: solver.sens_model_vjp(P, r, gw, lbw=lb, ubw=ub))
            for S in ((), (N,)):  # rows shared by the stages, one row per stage
                t = f"m{m}_{bname}_{'stage' if S else 'all'}"
                if ocp.model == "linear":
                    nz = nx + nu
                    wt = {"dW": rng.normal(size=(B, m) + S + (nz * (nz + 1) // 2,))}
                    md = {"dA": rng.normal(size=(B, m) + S + (nx, nx)), "dc": rng.normal(size=(B, m) + S + (nx,))}
                else:
                    wt = {"dQ": rng.normal(size=(B, m) + S + (nx,)), "dR": rng.normal(size=(B, m) + S + (nu,))}
                    md = {"dpar": rng.normal(size=(B, m) + S + (solver._h.model_dims(),))}
                keep(f"weights_{t}", lambda: solver.sens_weights(P, r, lbw=lb, ubw=ub, **wt))
                keep(f"model_{t}", lambda: solver.sens_model(P, r, lbw=lb, ubw=ub, **md))


def sens_loop(res, tag, solver, loop, rng):
    """The nine DeviceLoop methods: m = 1 and nx; the resident point and a saved one; the bounds in force
    and per-instance bounds installed; outputs allocated and given."""
    B, nx, N = loop.B, loop._knx, solver.ocp.N
    nw, n_p, n_wt, n_th = loop.w.shape[1], loop.P.shape[1], solver._h.weight_dims(), solver._h.model_dims()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(loop.device)  # noqa: E731
    saved = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    w_user = loop.w.cpu().numpy() if solver._pad is None else loop.w.cpu().numpy()[:, solver._pad.w_idx]
    each = [dev(v) for v in box_around(w_user)[1]]

    def keep(name, call):
        try:
            for i, t in enumerate(call()):
                if t is not None:
                    res[f"{tag}/loop/{name}/{i}"] = t.cpu().numpy()
        except (ValueError, _lib.MpcxError) as e:
            res[f"{tag}/loop/{name}/refused"] = np.array(f"{type(e).__name__}: {e}")

    for bname in ("in_force", "each"):
        if bname == "each":
            loop.set_bounds(*each)
        keep(f"x0_{bname}", loop.sens_x0)
        for m in (1, nx):
            gw, dlb, dub = (dev(rng.normal(size=(B, m, nw))) for _ in range(3))
            dP = dev(rng.normal(size=(B, m, n_p)))
            keep(f"p_m{m}_{bname}", lambda: loop.sens_p(dP))
            for pname, point in (("resident", None), ("saved", saved)):
                t = f"m{m}_{bname}_{pname}"
                keep(f"vjp_{t}", lambda: loop.sens_vjp(gw, point=point))
                keep(f"bounds_{t}", lambda: loop.sens_bounds(dlb, dub, point=point))
                keep(f"bounds_upper_only_{t}", lambda: loop.sens_bounds(None, dub, point=point))
                keep(f"bounds_vjp_{t}", lambda: loop.sens_bounds_vjp(gw, point=point))
                for stage in (True, False):
                    s = "stage" if stage else "all"
                    dW = dev(rng.normal(size=(B, m, N, n_wt) if stage else (B, m, n_wt)))
                    keep(f"weights_{t}_{s}", lambda: loop.sens_weights(dW, point=point))
                    keep(f"weights_vjp_{t}_{s}", lambda: loop.sens_weights_vjp(gw, point=point, per_stage=stage))
                    if n_th:
                        dTh = dev(rng.normal(size=(B, m, N, n_th) if stage else (B, m, n_th)))
                        keep(f"model_{t}_{s}", lambda: loop.sens_model(dTh, point=point))
                    keep(f"model_vjp_{t}_{s}", lambda: loop.sens_model_vjp(gw, point=point, per_stage=stage))
        # outputs given: written in place
        full = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=loop.device)  # noqa: E731
        fl = torch.full((B,), 7, dtype=torch.int32, device=loop.device)
        keep(f"x0_given_{bname}", lambda: loop.sens_x0(dw_out=full(B, nw, nx), flag_out=fl))
        gw = dev(rng.normal(size=(B, nx, nw)))
        keep(f"weights_vjp_given_{bname}",
             lambda: loop.sens_weights_vjp(gw, gWk_out=full(B, nx, N, n_wt), per_stage=False))
    loop.set_bounds(None, None)
    torch.cuda.synchronize()


def raw_calls(D):
    """The nine calls by the arguments between the point and the flag: name -> (shapes of the inputs, has a
    per_stage argument, has m, shapes of the outputs, either output may be left out), as functions of m
    and the rows' stage axis S = () or (N,)."""
    B, nw, n_p, N, nx, nu, n_wt, n_th = (D[k] for k in ("B", "nw", "np", "N", "nx", "nu", "n_wt", "n_th"))
    return {
        "x0": (lambda m, S: [], False, False, lambda m: [(B, nw, nx), (B, nu, nx)], True),
        "p": (lambda m, S: [(B, m, n_p)], False, True, lambda m: [(B, nw, m)], False),
        "vjp": (lambda m, S: [(B, m, nw)], False, True, lambda m: [(B, m, n_p)], False),
        "bounds": (lambda m, S: [(B, m, nw)] * 2, False, True, lambda m: [(B, nw, m)], False),
        "bounds_vjp": (lambda m, S: [(B, m, nw)], False, True, lambda m: [(B, m, nw)] * 2, False),
        "weights": (lambda m, S: [(B, m) + S + (n_wt,)], True, True, lambda m: [(B, nw, m)], False),
        "weights_vjp": (lambda m, S: [(B, m, nw)], False, True, lambda m: [(B, m, N, n_wt), (B, m, n_wt)], True),
        "model": (lambda m, S: [(B, m) + S + (n_th,)], True, True, lambda m: [(B, nw, m)], False),
        "model_vjp": (lambda m, S: [(B, m, nw)], False, True, lambda m: [(B, m, N, n_th), (B, m, n_th)], True),
    }


def sens_raw(res, tag, solver, loop, rng, refusals):
    """Raw ctypes calls of the host-pointer entry points at the loop's point (the kernel's layout): m = 1
    and nx, no bounds and shared ones, rows shared and per stage, every subset of optional outputs, with
    and without the flag.  With ``refusals``, the text of the calls both kinds of entry point refuse."""
    lib, h = _lib.load(), solver._h.ptr
    point = [t.cpu().numpy() for t in (loop.P, loop.w, loop.lam, loop.lamx)]
    D = {"B": loop.B, "nw": point[1].shape[1], "np": point[0].shape[1], "N": solver.ocp.N, "nx": loop._knx,
         "nu": solver.ocp.nu, "n_wt": solver._h.weight_dims(), "n_th": solver._h.model_dims()}
    B, nx, N = D["B"], D["nx"], D["N"]
    lb, ub = box_around(point[1])[0]

    def host(name, m, S, ins, outs, flag, lbw=None, ubw=None, B=B, point=point):
        _, has_ps, has_m, _, _ = raw_calls(D)[name]
        mid = ([int(bool(S))] if has_ps else []) + ([m] if has_m else [])
        return getattr(lib, "mpcx_sens_" + name)(h, B, *map(_lib.dptr, point), _lib.dptr(lbw), _lib.dptr(ubw),
                                                 *map(_lib.dptr, ins), *mid, *map(_lib.dptr, outs), _lib.iptr(flag))

    def device(name, m, S, ins, outs, flag, B=B, point=(loop.P, loop.w, loop.lam, loop.lamx)):
        _, has_ps, has_m, _, _ = raw_calls(D)[name]
        mid = ([int(bool(S))] if has_ps else []) + ([m] if has_m else [])
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return getattr(lib, "mpcx_sens_" + name + "_dev")(h, B, *map(ptr, point), *map(ptr, ins), *mid, *map(ptr, outs),
                                                          ptr(flag), ctypes.c_void_p(loop.stream.cuda_stream))

    model = solver.ocp.model
    for name, (in_shapes, has_ps, has_m, out_shapes, either) in raw_calls(D).items():
        runs = not (model == "path_bicycle" and name in ("p", "vjp")) and not (model == "unicycle" and "model" in name)
        for m in (1, nx) if has_m and runs else (nx,):
            for S in ((), (N,)) if has_ps and runs else ((),):
                ins = [rng.normal(size=s) for s in in_shapes(m, S)]
                subsets = [(True, True), (True, False), (False, True)] if either else [(True,) * len(out_shapes(m))]
                for bname, (lbw, ubw) in (("none", (None, None)), ("shared", (lb, ub))):
                    for want in subsets if runs else subsets[:1]:
                        outs = [np.full(s, 7.0) if w else None for s, w in zip(out_shapes(m), want)]
                        flag = np.full(B, 7, np.int32) if want[0] else None  # (the flag is optional everywhere)
                        rc = host(name, m, S, ins, outs, flag, lbw, ubw)
                        t = f"{tag}/raw/{name}_m{m}_{'stage' if S else 'all'}_{bname}_{''.join('01'[w] for w in want)}"
                        res[t + "/rc"] = np.array(rc)
                        if rc != 0:
                            res[t + "/refused"] = np.array(lib.mpcx_last_error().decode())
                        for i, o in enumerate(outs + [flag]):
                            if o is not None:
                                res[f"{t}/{i}"] = o
        if not refusals:
            continue
        # refused calls: the arrays are valid ones throughout, so a call that is not refused is a valid call
        S, m = (N,) if has_ps else (), min(2, nx)
        ins = [rng.normal(size=s) for s in in_shapes(nx, S)]  # (room for any m <= nx)
        outs, flag = [np.full(s, 7.0) for s in out_shapes(nx)], np.zeros(B, np.int32)
        d_point = (loop.P, loop.w, loop.lam, loop.lamx)
        d_ins = [torch.from_numpy(v).to(loop.device) for v in ins]
        d_outs = [torch.from_numpy(v).to(loop.device) for v in outs]
        d_flag = torch.zeros(B, dtype=torch.int32, device=loop.device)
        for kind, call, pt, ii, oo, ff in (("host", host, point, ins, outs, flag),
                                           ("dev", device, d_point, d_ins, d_outs, d_flag)):
            def refused(label, rc):
                res[f"{tag}/refusal/{name}_{kind}/{label}"] = np.array(f"{rc}: {lib.mpcx_last_error().decode()}")

            refused("B0", call(name, m, S, ii, oo, ff, B=0))
            if has_m:
                refused("m0", call(name, 0, S, ii, oo, ff))
                refused("m_nx_plus_1", call(name, nx + 1, S, ii, oo, ff))
            without = lambda ts, i: [None if j == i else t for j, t in enumerate(ts)]  # noqa: E731
            for i in range(4):  # one null pointer per position: the point, ...
                refused(f"null_point_{i}", call(name, m, S, ii, oo, ff, point=without(pt, i)))
            for i in range(len(ii)):  # ... the inputs, ...
                refused(f"null_in_{i}", call(name, m, S, without(ii, i), oo, ff))
            if either:  # ... and the outputs (of a pair either may be left out: both)
                refused("null_outs", call(name, m, S, ii, [None] * len(oo), ff))
            else:
                for i in range(len(oo)):
                    refused(f"null_out_{i}", call(name, m, S, ii, without(oo, i), ff))
        torch.cuda.synchronize()


def sens_workload():
    res = {}
    for i, (tag, ocp, P, opts) in enumerate(sens_problems()):
        rng = np.random.default_rng(100 + i)
        solver = mpcx.nlpsol(tag, "mi355x", ocp, {"ipopt": opts})
        r = solver.solve_batch(P)
        for k in ("w", "lam_g", "lam_x", "status", "iters"):
            res[f"{tag}/solve/{k}"] = r[k]
        sens_solver(res, tag, solver, P, r, rng)
        loop = DeviceLoop(solver, P)
        loop.solve()
        sens_loop(res, tag, solver, loop, rng)
        sens_raw(res, tag, solver, loop, rng, refusals=True)
        print(f"{tag}: statuses {np.bincount(r['status'])}, {len(res)} arrays so far", flush=True)
    # N = 64: refused by every entry point before anything is read (a handle is all it takes)
    solver = mpcx.nlpsol("unicycle_N64", "mi355x", mpcx.unicycle_point_to_point(N=64), {})
    lib, h = _lib.load(), solver._h.ptr
    d, i32 = np.zeros(1 << 16), np.zeros(8, np.int32)  # (large enough for B = 1, were a call not refused)
    dz = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p, q, v = _lib.dptr(d), _lib.iptr(i32), ctypes.c_void_p(dz.data_ptr())
    mids = {"x0": (), "p": (1,), "vjp": (1,), "bounds": (1,), "bounds_vjp": (1,), "weights": (0, 1),
            "weights_vjp": (1,), "model": (0, 1), "model_vjp": (1,)}
    n_in = {"x0": 0, "bounds": 2}  # (the others: one input)
    n_out = {"x0": 2, "bounds_vjp": 2, "weights_vjp": 2, "model_vjp": 2}  # (the others: one output)
    for name, mid in mids.items():
        i, o = n_in.get(name, 1), n_out.get(name, 1)
        rc = getattr(lib, "mpcx_sens_" + name)(h, 1, p, p, p, p, None, None, *[p] * i, *mid, *[p] * o, q)
        res[f"unicycle_N64/refusal/{name}_host"] = np.array(f"{rc}: {lib.mpcx_last_error().decode()}")
        rc = getattr(lib, "mpcx_sens_" + name + "_dev")(h, 1, v, v, v, v, *[v] * i, *mid, *[v] * o, v, None)
        res[f"unicycle_N64/refusal/{name}_dev"] = np.array(f"{rc}: {lib.mpcx_last_error().decode()}")
    return res


if work == "sens":
    res = sens_workload()
    np.savez(out, **res)
    print(f"sens: {len(res)} arrays")
    sys.exit(0)
if work == "dyn":  # config 4 variant: 6-state dynamic bicycle, N = 50, B = 1024
    N, B = 50, 1024
    ocp = mpcx.dynamic_bicycle_lane_change(N=N)
    t0, x0, (X, Y, V) = mdist.config4_bicycle_inputs(0, B)
    refs = np.stack([mpcx.ode.dyn_bicycle_references(X, Y, V, int(t), N).reshape(-1) for t in t0])
    P = ocp.params(x0, refs)
elif work == "c2":  # config 2
    ocp = mpcx.unicycle_point_to_point(N=20)
    P = mdist.config2_inputs(0, 1024)
elif work == "c5":  # config 5: cart-pole QP, N = 100, B = 2048 (two-wave groups, the suffix scan)
    from mpcx import lti

    ocp = lti.inverted_pendulum_qp(N=100)
    P = lti.pendulum_params(ocp, mdist.config5_inputs(0, 2048), 0.0)
else:
    raise SystemExit(f"unknown workload {work}")
solver = mpcx.nlpsol("s", "mi355x", ocp, {"ipopt": {"max_iter": 3000}})
r = solver.solve_batch(P)
loop = DeviceLoop(solver, P)
st, it = loop.run(3)
torch.cuda.synchronize()
np.savez(out, w=r["w"], iters=r["iters"], status=r["status"], lam_g=r["lam_g"], st=st.cpu().numpy(),
         it=it.cpu().numpy(), loop_w=loop.w.cpu().numpy())
print(f"{work}: iters mean {r['iters'].mean():.2f}, statuses {np.bincount(r['status'])}")
