"""The family of infeasible problems of tests/test_resto_cpu.py and tests/test_gpu_resto_exits.py:
a per-instance bound that puts X_1 outside what one step can reach, so every instance goes through
soft restoration into the restoration phase and leaves it by one of its failure exits (IPOPT
statuses 2: max_iter, 3: restoration failed, 4: local infeasibility, 5: delta > kDwMax).

* unicycle (``mpcx.unicycle_point_to_point``): N in UNI_N (lane groups 16, 16, 32, 64, 128, 256),
  P = [0.3, -0.2, theta, 1.5, 1.0, 0.5], the problem's own bounds except X_1's x in
  [0.3 + lo, 0.3 + lo + 1]; one step reaches 0.2 at most (v_max T), so for theta = 0 the least
  constraint violation is exactly lo - 0.2.
* kinematic bicycle, cart-pole, 6-state bicycle: three instances each from the first rows of
  mpcx.dist's config-3, config-5 and config-4 inputs, X_1[0] bound to [x1* + d, x1* + 2 d], x1* the
  feasible solve's value.

The CPU oracle (oracle/ipm_ref.cpp) takes one shared bounds row, so it is called per instance; its
results are computed once per process, shared, and never modified.
"""
import functools
import math

import numpy as np

MAX_ITER = 300
# relative scalings of P over which the spread of the oracle's end-point violation is taken ...
SCALINGS = (0.0, 1e-13, -1e-13, 3e-13)
# ... and the further ones under which an instance's oracle exit must not change either to count as
# stable: the set made symmetric, and one decade out.  Added after the first device run: the unicycle
# at N = 40, theta = -2, lo = 0.5 keeps (4, 15) under SCALINGS but takes 17 iterations under -1e-12
# (and 16 or 17 under 1e-15, -1e-14 and 1e-11) -- its exit test passes by a hair (the oracle's trace:
# error 3.6e-9 at iteration 15 against tol 1e-8, 4.8e-6 the iteration before, in its second visit of
# the restoration phase) -- and the device ended it at (3, 18).  Rounding alone, so the filter was
# narrowed, not the assertion: 7 stable instances of 72 became 4 (6 with the two status-5 ones).
MORE_SCALINGS = (-3e-13, 1e-12, -1e-12)
ALL_SCALINGS = SCALINGS + MORE_SCALINGS
UNI_N = (2, 10, 20, 40, 70, 130)
UNI_THETA = (0.0, 0.7, -2.0)
UNI_LO = (0.5, 1.0)
UNI_LO_HARD = 0.25  # runs into max_iter or status 5 on a third of the instances: not in the asserted set
ODE_CASES = {"kin_bicycle": ((5, 30), (1.0, 5.0)), "cartpole": ((5, 70), (0.5, 2.0)), "dyn_bicycle": ((5, 20), (0.5, 2.0))}


def group_of(N):
    """Lanes of an instance's group: the next power of two above N, 16 at least."""
    return max(16, 1 << N.bit_length())


def _ocp(model, N):
    import mpcx

    return {"unicycle": mpcx.unicycle_point_to_point, "kin_bicycle": mpcx.kinematic_bicycle_tracking,
            "cartpole": mpcx.cartpole_swingup, "dyn_bicycle": mpcx.dynamic_bicycle_lane_change}[model](N=N)


def own_bounds(ocp):
    """The problem's own lbw / ubw (n_w), infinities as -+1e20."""
    from oracle import ipm_ref

    lb, ub = ipm_ref.ms_bounds_any(ocp)
    return np.where(np.isfinite(lb), lb, -1e20), np.where(np.isfinite(ub), ub, 1e20)


def _ode_P(model, ocp, N, B=3):
    import mpcx
    from mpcx import dist as mdist

    if model == "kin_bicycle":
        return mdist.config3_bicycle_inputs(0, B, N=N)[1]
    if model == "cartpole":
        return mdist.config5_swingup_inputs(0, B)
    t0, x0, (X, Y, V) = mdist.config4_bicycle_inputs(0, B)
    refs = np.stack([mpcx.ode.dyn_bicycle_references(X, Y, V, int(t), N).reshape(-1) for t in t0])
    return ocp.params(x0, refs)


@functools.lru_cache(maxsize=None)
def case(model, N):
    """One (model, horizon): dict(ocp, P (B, n_p), lb, ub (B, n_w), lb0, ub0 (n_w: the problem's
    own), label (B strings), lo (B: the unicycle's lo, NaN elsewhere), theta (B)).  The unicycle's
    rows are theta-major over UNI_LO; the ODE models' are instance-major over d."""
    from oracle import ipm_ref

    ocp = _ocp(model, N)
    lb0, ub0 = own_bounds(ocp)
    i1 = ipm_ref.pb_dims(ocp)[1]  # X_1[0]: after X_0 and U_0
    P, lb, ub, label, los, ths = [], [], [], [], [], []
    if model == "unicycle":
        for th in UNI_THETA:
            for lo in UNI_LO:
                P.append([0.3, -0.2, th, 1.5, 1.0, 0.5])
                lo_, hi_ = lb0.copy(), ub0.copy()
                lo_[i1], hi_[i1] = 0.3 + lo, 0.3 + lo + 1.0
                lb.append(lo_), ub.append(hi_), los.append(lo), ths.append(th)
                label.append(f"unicycle N={N} theta={th} lo={lo}")
    else:
        P0 = _ode_P(model, ocp, N)
        feas = ipm_ref.solve(ocp, P0, max_iter=3000)
        assert np.all(feas["status"] == 0), (model, N, feas["status"])
        for b in range(len(P0)):
            for d in ODE_CASES[model][1]:
                x1 = feas["w"][b, i1]
                lo_, hi_ = lb0.copy(), ub0.copy()
                lo_[i1], hi_[i1] = x1 + d, x1 + 2.0 * d
                P.append(P0[b]), lb.append(lo_), ub.append(hi_), los.append(math.nan), ths.append(math.nan)
                label.append(f"{model} N={N} instance {b} d={d}")
    out = dict(ocp=ocp, model=model, N=N, G=group_of(N), P=np.array(P, float), lb=np.array(lb), ub=np.array(ub),
               lb0=lb0, ub0=ub0, label=label, lo=np.array(los), theta=np.array(ths), i1=i1)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def all_cases():
    return [("unicycle", N) for N in UNI_N] + [(m, N) for m, (Ns, _) in ODE_CASES.items() for N in Ns]


def oracle_rows(ocp, P, lb, ub, **opts):
    """ipm_ref.solve per instance (one bounds row each; P (B, n_p) or a list of such blocks, solved
    side by side on a few threads -- the library call releases the interpreter lock), stacked."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import ipm_ref

    ipm_ref.lib()
    opts.setdefault("max_iter", MAX_ITER)
    blocks = [P] if isinstance(P, np.ndarray) else list(P)
    jobs = [(Pb, b) for Pb in blocks for b in range(len(Pb))]
    with ThreadPoolExecutor(max_workers=8) as pool:
        rows = list(pool.map(lambda j: ipm_ref.solve(ocp, j[0][j[1]:j[1] + 1], lbw=lb[j[1]], ubw=ub[j[1]], nthreads=1,
                                                     **opts), jobs))
    out = [{k: np.concatenate([r[k] for r in rows[i * len(lb):(i + 1) * len(lb)]]) for k in rows[0]}
           for i in range(len(blocks))]
    return out[0] if isinstance(P, np.ndarray) else out


def violation(ocp, w, P):
    """Maximum constraint violation max |g(w)| of one point, by the oracle's constraint function
    (nlp_ref.ms_functions, which nlp_ref.kkt_residual_ms reports, for the unicycle;
    ode_ref.Problem.kkt_residual otherwise)."""
    from oracle import nlp_ref, ode_ref

    if getattr(ocp, "model", "unicycle") == "unicycle":
        return float(np.max(np.abs(nlp_ref.ms_functions(np.asarray(w, float), np.asarray(P, float), ocp)[1])))
    pr = ode_ref.Problem(ocp)
    return pr.kkt_residual(w, np.zeros(pr.nx * (pr.N + 1)), np.zeros(len(w)), P)[1]


@functools.lru_cache(maxsize=None)
def oracle_case(model, N):
    """The oracle on case(model, N) under every scaling of P (ALL_SCALINGS, row 0 unscaled):
    dict(status, iters (S, B), viol (S, B: the end point's violation), w (B, n_w: scaling 0), stable
    (B: same (status, iterations) under all scalings), asserted (B: every scaled run ends at 3 or
    4), spread (B: max - min of viol over SCALINGS))."""
    c = case(model, N)
    return _scaled_runs(c["ocp"], c["P"], c["lb"], c["ub"])


def _scaled_runs(ocp, P, lb, ub, **opts):
    Ps = [P * (1.0 + s) for s in ALL_SCALINGS]
    rs = oracle_rows(ocp, Ps, lb, ub, **opts)
    st, it = [r["status"] for r in rs], [r["iters"] for r in rs]
    vi = [[violation(ocp, r["w"][b], Pb[b]) for b in range(len(Pb))] for r, Pb in zip(rs, Ps)]
    w0 = rs[0]["w"]
    st, it, vi = np.array(st), np.array(it), np.array(vi)
    out = dict(status=st, iters=it, viol=vi, w=w0, stable=np.all((st == st[0]) & (it == it[0]), axis=0),
               asserted=np.all((st == 3) | (st == 4), axis=0),
               spread=vi[:len(SCALINGS)].max(axis=0) - vi[:len(SCALINGS)].min(axis=0),
               spread_all=vi.max(axis=0) - vi.min(axis=0))
    for v in out.values():
        v.setflags(write=False)
    return out


def geometric_minimum(lo, theta):
    """The unicycle's least constraint violation for heading 0: X_1's x is at least 0.3 + lo, one
    step from x = 0.3 reaches 0.3 + v_max T = 0.5 at most, exactly so for theta = 0 (omega = 0
    keeps the heading; RK4 integrates a constant exactly)."""
    assert theta == 0.0
    return lo - 0.2


@functools.lru_cache(maxsize=None)
def status5_case(N):
    """The unicycle at theta = 0 with lo = UNI_LO_HARD: the inertia correction of the restoration
    phase gives up (delta > kDwMax, status 5).  dict(ocp, P (1, 6), lb, ub (1, n_w)) and the oracle
    under every scaling as oracle_case returns it."""
    c = case("unicycle", N)
    lb, ub = c["lb0"].copy(), c["ub0"].copy()
    lb[c["i1"]], ub[c["i1"]] = 0.3 + UNI_LO_HARD, 0.3 + UNI_LO_HARD + 1.0
    P = np.array([[0.3, -0.2, 0.0, 1.5, 1.0, 0.5]])
    return dict(ocp=c["ocp"], P=P, lb=lb[None], ub=ub[None], lb0=c["lb0"], ub0=c["ub0"]), _scaled_runs(c["ocp"], P, lb[None], ub[None])


MAX_ITER_CASE = ("unicycle", 40, 4)  # model, N, row of case(): theta = -2.0, lo = 0.5


@functools.lru_cache(maxsize=None)
def max_iter_case():
    """One instance with max_iter two above the iteration at which the restoration phase is
    entered.  Without restoration the oracle's line search fails at iteration k (status 3); with it,
    the soft step of that iteration is rejected on this instance (the oracle's trace: "soft
    restoration step accepted=0", "enter restoration" at it = k), so the phase starts at k and
    max_iter = k + 2 is reached inside it, after two of its steps.  Returns (case, row, k,
    the oracle's result with max_iter = k + 2)."""
    from oracle import ipm_ref

    model, N, b = MAX_ITER_CASE
    c = case(model, N)
    args = dict(lbw=c["lb"][b], ubw=c["ub"][b])
    off = ipm_ref.solve(c["ocp"], c["P"][b:b + 1], max_iter=MAX_ITER, restoration=0, **args)
    k = int(off["iters"][0])
    return c, b, k, int(off["status"][0]), ipm_ref.solve(c["ocp"], c["P"][b:b + 1], max_iter=k + 2, **args)


def tolerance():
    """(tol, worst spread): 10 x the largest spread of the oracle's end-point violation over the
    scalings of P, over the instances of the whole family whose every scaled run ends at 3 or 4."""
    worst = max(float(o["spread"][o["asserted"]].max()) for o in (oracle_case(*mc) for mc in all_cases()))
    return 10.0 * worst, worst
