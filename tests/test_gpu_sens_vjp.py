"""GPU tests of the adjoint sensitivities of the MPC solution (mpcx_sens_vjp / mpcx_sens_vjp_dev,
Solver.sens_vjp, Solver.gain_p, DeviceLoop.sens_vjp, mpcx.autograd; csrc/sens.h sens_vjp_kernel).

References: tests/helpers/sens_vjp_ref.py -- the adjoint restated in long double from the GPU's own
point -- and the project's forward mode, Solver.sens_p, through the dot-product identity
<g, sens_p(dP)> = <sens_vjp(g), dP>.  Cases and shapes are those of tests/test_gpu_sens.py and
tests/test_gpu_sens_p.py (their constructors and cached solves are imported): the smallest that reach
every lane group (16, 32, 64) and every solve unit."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402
import sens_vjp_ref as sv  # noqa: E402
from test_gpu_sens import LINEAR_CASES, REF_OPTS, linear_case, linear_problem, unicycle_P  # noqa: E402
from test_gpu_sens_p import NONLINEAR_CASES, linear_p_case, nonlinear_p_problem  # noqa: E402

LD = np.longdouble


@pytest.fixture(scope="module")
def mpcx():
    import mpcx as m

    m._lib.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def identity_gap(g, dw, gP, dP):
    """(|<g, dw> - <gP, dP>|, bound 2 of the issue) per (instance, cotangent, direction):
    g (B, mg, n_w), dw (B, n_w, md), gP (B, mg, n_p), dP (B, md, n_p).  The bound is
    64 e_ref_p sum |g_i| max(1, |dw_i|) + 64 e_ref_vjp sum |dP_j| max(1, |gP_j|): both results lie within
    their entrywise bound of exact quantities that satisfy the identity exactly."""
    lhs = np.einsum("bci,bij->bcj", g, dw)
    rhs = np.einsum("bcp,bjp->bcj", gP, dP)
    bound = (64.0 * sp.e_ref_p() * np.einsum("bci,bij->bcj", np.abs(g), np.maximum(1.0, np.abs(dw)))
             + 64.0 * sv.e_ref_vjp() * np.einsum("bcp,bjp->bcj", np.maximum(1.0, np.abs(gP)), np.abs(dP)))
    return np.abs(lhs - rhs), bound


# ------------------------------------------------------------------------------------------
# linear cases: the solves and sens_p results of test_gpu_sens_p.py's linear_p_case, shared, never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_vjp_case(name):
    """(lin, P, solve result, solver, dP, sens_p result, g (B, nx, n_w) seeded normal over the whole of w,
    sens_vjp result)"""
    lin, P, r, solver, dP, s = linear_p_case(name)
    g = np.random.default_rng(300 + LINEAR_CASES.index(name)).normal(size=(P.shape[0], lin.nx, lin.n_w_ms))
    v = solver.sens_vjp(P, r, g)
    for a in (g, *v.values()):
        a.setflags(write=False)
    return lin, P, r, solver, dP, s, g, v


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_against_the_restatement(mpcx, name):
    """1. The kernel against the adjoint restated in long double at the same point and tables (helpers (a)
    and (c)), m = nx seeded normal cotangents over the whole of w: 64 x e_ref_vjp relative to
    max(1, |entry|), the convention of tests/test_gpu_scan.py::scan_tolerance (e_ref_vjp = the float64
    restatement's own worst error against long double, 3.7e-15, so 2.3e-13).
    Measured on one MI355X: padded_dint_N8 1.8e-16, lin4x2_N12 1.4e-16, cartpole_qp_N50
    1.8e-16 (the case the refinement round is for), ltv_N40 1.1e-16."""
    lin, P, r, _, _, _, g, v = linear_vjp_case(name)
    tol = 64.0 * sv.e_ref_vjp()
    B = P.shape[0]
    assert np.all(v["flag"] == 0), v["flag"]
    assert v["gP"].shape == (B, lin.nx, P.shape[1])
    lb, ub = sr.ocp_bounds(lin)
    worst = 0.0
    for b in range(B):
        A, Bm, H = sr.linear_operands(lin, b)
        Sig = sr.sigma_of(r["w"][b], r["lam_x"][b], lb, ub, lin.nx, lin.nu, LD)
        lam0, zt, _, ok = sv.adjoint_sens(A, Bm, H, Sig, np.asarray(g[b].T, LD), LD)
        assert ok
        worst = max(worst, sr.rel_err(v["gP"][b], sv.linear_vjp(lin, lam0, zt, b)))
    print(f"{name}: worst error against the long-double restatement {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


@pytest.mark.parametrize("name", LINEAR_CASES)
def test_linear_dot_product_identity(mpcx, name):
    """2. <g, dw> = <gP, dP> with dw the project's own sens_p at the same point along seeded dP, within
    bound 2 (identity_gap).  A transposition, sign or missing-term error gives an O(1) violation.
    Measured on one MI355X, worst gap / bound: padded_dint_N8 2.7e-4, lin4x2_N12 4.0e-4, cartpole_qp_N50
    2.1e-3 (gap 1.6e-12), ltv_N40 7.4e-4."""
    _, _, _, _, dP, s, g, v = linear_vjp_case(name)
    gap, bound = identity_gap(g, s["dw"], v["gP"], dP)
    print(f"{name}: worst identity gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)


@pytest.mark.parametrize("name", NONLINEAR_CASES)
def test_nonlinear_dot_product_identity(mpcx, name):
    """2. The same identity on the nonlinear models -- the bounded unicycle, the stage-reference tracking
    unicycle, the N = 30 scan unit, the kinematic bicycle, the cart-pole, the 6-state bicycle -- with two
    seeded normal directions over the whole parameter row and two seeded normal cotangents over the whole
    of w, bound 2.  Measured on one MI355X, worst gap / bound: unicycle_N10 4.1e-4, unicycle_N30 9.4e-4,
    unicycle_bounded_N10 7.6e-4, unicycle_tracking_N10 2.9e-4, kin_bicycle_N10 2.5e-4, cartpole_N20 1.3e-3
    (entries of dw and gP up to 317 and 401, gap 6.8e-13), dyn_bicycle_N10 4.1e-4: none exceeds the bound."""
    ocp, P, opts = nonlinear_p_problem(name)
    solver = mpcx.nlpsol(name + "_vjp", "mi355x", ocp, {"ipopt": opts})
    nom = solver.solve_batch(P)
    assert np.all(nom["status"] <= 1), nom["status"]
    B = P.shape[0]
    rng = np.random.default_rng(400 + NONLINEAR_CASES.index(name))
    dP, g = rng.normal(size=(B, 2, P.shape[1])), rng.normal(size=(B, 2, nom["w"].shape[1]))
    s, v = solver.sens_p(P, nom, dP), solver.sens_vjp(P, nom, g)
    assert np.all(s["flag"] == 0) and np.all(v["flag"] == 0)
    assert v["gP"].shape == (B, 2, P.shape[1])
    gap, bound = identity_gap(g, s["dw"], v["gP"], dP)
    print(f"{name}: |dw| {np.abs(s['dw']).max():.3g}, |gP| {np.abs(v['gP']).max():.3g}, worst identity gap "
          f"{gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound)
    assert np.max(np.abs(v["gP"][:, :, ocp.nx:])) > 1e-3  # the references do get a gradient


# ------------------------------------------------------------------------------------------
# 3. exact properties
# ------------------------------------------------------------------------------------------
def exact_properties(solver, P, r, g, nx, alone=None):
    """zero cotangent -> zeros; X_0 rows only -> gP[:nx] = gX_0, zeros elsewhere; column c of an m-column
    launch (and of a call split over several launches) = that cotangent alone; an instance alone = inside
    the batch (the instances `alone`, default all).  g (B, m > nx, n_w)."""
    B, m, n_w = g.shape
    v = solver.sens_vjp(P, r, g)
    assert np.all(v["flag"] == 0) and v["gP"].shape == (B, m, P.shape[1])
    zero = solver.sens_vjp(P, r, np.zeros((B, 2, n_w)))
    assert np.all(zero["flag"] == 0) and np.all(zero["gP"] == 0.0)
    gx = np.zeros((B, 2, n_w))
    gx[:, :, :nx] = g[:, :2, :nx]
    vx = solver.sens_vjp(P, r, gx)
    assert bits(vx["gP"][:, :, :nx]) == bits(gx[:, :, :nx]) and np.all(vx["gP"][:, :, nx:] == 0.0)
    first = solver.sens_vjp(P, r, g[:, :nx])
    assert bits(first["gP"]) == bits(v["gP"][:, :nx])
    for c in range(m):
        one = solver.sens_vjp(P, r, g[:, c])  # (B, n_w): a single cotangent
        assert one["gP"].shape == (B, 1, P.shape[1]) and bits(one["gP"][:, 0]) == bits(v["gP"][:, c]), c
    for b in range(B) if alone is None else alone:
        solo = solver.sens_vjp(P[b:b + 1], {k: r[k][b:b + 1] for k in ("w", "lam_g", "lam_x")}, g[b:b + 1, :nx])
        assert bits(solo["gP"][0]) == bits(first["gP"][b]) and solo["flag"][0] == 0, b
    return v


def test_exact_properties_unicycle(mpcx):
    """The quadrature-cost unicycle on the x0_xref layout (the reference gradient by differences of derivs,
    summed over the lane group) and the tracking unicycle (node cost, stage references); the
    single-shooting form takes cotangents over the control rows."""
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("exact_vjp", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(5, 1)
    r = solver.solve_batch(P)
    g = np.random.default_rng(13).normal(size=(5, 5, 53))  # five cotangents: launches of 3 and 2 columns
    v = exact_properties(solver, P, r, g, 3)
    assert np.max(np.abs(v["gP"][:, :, 3:])) > 1e-3
    ss = mpcx.nlpsol("ss_vjp", "mi355x", mpcx.unicycle_point_to_point(N=10, formulation="single_shooting"),
                     {"ipopt": REF_OPTS})
    rows = np.concatenate([3 + 5 * k + np.arange(2) for k in range(10)])
    gu = np.zeros_like(g[:, :3])
    gu[:, :, rows] = g[:, :3, rows]
    assert bits(ss.sens_vjp(P, r, g[:, :3, rows])["gP"]) == bits(solver.sens_vjp(P, r, gu)["gP"])
    assert bits(ss.gain_p(P, r)["dU0_dP"]) == bits(solver.gain_p(P, r)["dU0_dP"])
    with pytest.raises(ValueError):
        solver.sens_vjp(P, r, np.zeros((4, 3, 53)))
    with pytest.raises(ValueError):
        solver.sens_vjp(P, r, np.zeros((5, 3, 52)))
    ocp, Pt, opts = nonlinear_p_problem("unicycle_tracking_N10")
    tr = mpcx.nlpsol("exact_vjp_tr", "mi355x", ocp, {"ipopt": opts})
    exact_properties(tr, Pt, tr.solve_batch(Pt), np.random.default_rng(14).normal(size=(Pt.shape[0], 4, 53)), 3)


@pytest.mark.parametrize("name", ["padded_dint_N8", "ltv_N40"])
def test_exact_properties_linear(mpcx, name):
    lin, P, r, solver, _, _, g, v = linear_vjp_case(name)
    rng = np.random.default_rng(15)
    more = np.concatenate([g, rng.normal(size=(P.shape[0], 1, lin.n_w_ms))], axis=1)  # nx + 1: two launches
    # (a schedule per instance, ltv_N40: a batch of one reads the first row, so instance 0 is the one alone)
    got = exact_properties(solver, P, r, more, lin.nx, alone=None if lin.tab.ndim == 1 else [0])
    assert bits(got["gP"][:, :lin.nx]) == bits(v["gP"])


# ------------------------------------------------------------------------------------------
# 4. gain_p
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINEAR_CASES)
def test_gain_p_x0_block_is_K0(mpcx, name):
    """The x0 block of dU_0/dP against sens_x0's K0 at the same point: 64 x (e_ref + e_ref_vjp) relative to
    max(1, |entry|) -- each lies within its own bound of the same exact gain.  Measured on one MI355X:
    the same bits in all four cases (tolerance 2.7e-13): for a unit cotangent on U_0 the backward sweep's
    p~_0 is K_0's row itself."""
    lin, P, r, sx, solver = linear_case(name)
    gp = solver.gain_p(P, r)
    tol = 64.0 * (sr.e_ref() + sv.e_ref_vjp())
    assert np.all(gp["flag"] == 0) and gp["dU0_dP"].shape == (P.shape[0], lin.nu, P.shape[1])
    worst = sr.rel_err(gp["dU0_dP"][:, :, :lin.nx], sx["K0"])
    print(f"{name}: worst difference of gain_p's x0 block to K0 {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


def test_gain_p_xref_block_is_Kr(mpcx):
    """On an x0_xref problem (the point-to-point unicycle, N = 10: the linear cases carry stage references
    and have no x_ref) the x_ref block against sens_xref's Kr: 64 x (e_ref_p + e_ref_vjp) relative to
    max(1, |entry|); the x0 block against K0 as above.  Measured on one MI355X: x_ref block 2.1e-16 (|Kr| up to 2.6),
    x0 block the same bits."""
    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("gain_p", "mi355x", ocp, {"ipopt": REF_OPTS})
    P = unicycle_P(5, 1)
    r = solver.solve_batch(P)
    gp, kr, k0 = solver.gain_p(P, r), solver.sens_xref(P, r), solver.sens_x0(P, r)
    assert np.all(gp["flag"] == 0) and gp["dU0_dP"].shape == (5, 2, 6)
    e_r = sr.rel_err(gp["dU0_dP"][:, :, 3:], kr["Kr"])
    e_0 = sr.rel_err(gp["dU0_dP"][:, :, :3], k0["K0"])
    print(f"unicycle_N10: x_ref block to Kr {e_r:.3e}, x0 block to K0 {e_0:.3e}, |Kr| {np.abs(kr['Kr']).max():.3g}")
    assert e_r <= 64.0 * (sp.e_ref_p() + sv.e_ref_vjp())
    assert e_0 <= 64.0 * (sr.e_ref() + sv.e_ref_vjp())
    assert np.max(np.abs(kr["Kr"])) > 1e-3


# ------------------------------------------------------------------------------------------
# 5. host and device entry points agree
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unicycle_N10", "padded_dint_N8"])
def test_device_loop_equals_host_call(mpcx, name):
    """DeviceLoop.sens_vjp after solve() against Solver.sens_vjp on the loop's tensors copied back, bit for
    bit; the point= override on a saved copy gives the same bits after the loop has solved something else."""
    import torch
    from mpcx.device import DeviceLoop

    if name == "unicycle_N10":
        ocp, P = mpcx.unicycle_point_to_point(N=10), unicycle_P(5, 1)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": REF_OPTS})
        n_w = 53
    else:
        ocp, P = linear_problem(name)
        solver = mpcx.nlpsol(name, "mi355x", ocp, {"ipopt": {"max_iter": 300}})
        n_w = ocp.n_w_ms
    pd = solver._pad
    B, m = P.shape[0], ocp.nx
    g = np.random.default_rng(16).normal(size=(B, m, n_w))
    gk = g if pd is None else pd.scatter(g.reshape(B * m, -1), pd.w_idx, pd.n_w_pad).reshape(B, m, -1)
    loop = DeviceLoop(solver, P, device="cuda:0")
    d_g = torch.from_numpy(np.ascontiguousarray(gk)).to("cuda:0")
    loop.solve()
    gP, flag = loop.sens_vjp(d_g)
    saved = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in (("P", loop.P), ("w", loop.w), ("lam_g", loop.lam), ("lam_x", loop.lamx))}
    gP_np = gP.cpu().numpy()
    if pd is not None:  # the loop's tensors hold the kernel's padded layout
        host = {"P": host["P"][:, pd.p_idx], "w": host["w"][:, pd.w_idx], "lam_g": host["lam_g"][:, pd.g_idx],
                "lam_x": host["lam_x"][:, pd.w_idx]}
        gP_np = gP_np[:, :, pd.p_idx]
    v = solver.sens_vjp(host["P"], host, g)
    assert np.all(v["flag"] == 0) and bits(flag.cpu().numpy()) == bits(v["flag"])
    assert bits(gP_np) == bits(v["gP"])
    loop.step()  # the resident point moves on
    loop.solve()
    out = torch.full((B, m, loop.P.shape[1]), 7.0, dtype=torch.float64, device="cuda:0")
    again = loop.sens_vjp(d_g, gP_out=out, point=saved)[0]
    moved = loop.sens_vjp(d_g)[0]
    torch.cuda.synchronize()
    assert again is out and bits(out.cpu().numpy()) == bits(gP.cpu().numpy())
    assert bits(moved.cpu().numpy()) != bits(gP.cpu().numpy())
    with pytest.raises(ValueError):
        loop.sens_vjp(d_g, gP_out=out[:, :1])
    with pytest.raises(ValueError):
        loop.sens_vjp(torch.zeros((B, loop._knx + 1, loop.w.shape[1]), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        loop.sens_vjp(d_g, point=(saved[0], saved[1][:, :-1].contiguous(), saved[2], saved[3]))


# ------------------------------------------------------------------------------------------
# 6. autograd
# ------------------------------------------------------------------------------------------
def test_autograd_backward(mpcx):
    """solve_differentiable on unicycle_N10: the backward equals DeviceLoop.sens_vjp on the saved point bit
    for bit; for L = 1/2 |U_0 - u_t|^2, P.grad is within bound 2 of J^T (U_0 - u_t) with J = dU_0/dP from
    sens_p's identity directions (per entry j of the row: g = U_0 - u_t on the U_0 rows, dP = e_j, dw = J's
    column); irregular="zero" zeros exactly the flagged rows, the default lets the NaN through.
    Measured on one MI355X: |P.grad| up to 11.8, worst difference 4.4e-16, 4.1e-4 of the bound."""
    import torch
    from mpcx.autograd import solve_differentiable
    from mpcx.device import DeviceLoop

    ocp = mpcx.unicycle_point_to_point(N=10)
    solver = mpcx.nlpsol("autograd", "mi355x", ocp, {"ipopt": REF_OPTS})
    P0 = unicycle_P(5, 1)
    B, nx, nu, n_p = 5, 3, 2, 6
    loop = DeviceLoop(solver, P0, device="cuda:0")
    P = torch.tensor(P0, dtype=torch.float64, device="cuda:0", requires_grad=True)
    u_t = torch.tensor(np.random.default_rng(17).uniform(-0.5, 0.5, (B, nu)), dtype=torch.float64, device="cuda:0")
    w = solve_differentiable(loop, P)
    assert w.shape == (B, 53) and w.requires_grad
    point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    loss = 0.5 * ((w[:, nx:nx + nu] - u_t) ** 2).sum()
    loss.backward()
    gw = torch.zeros((B, 1, 53), dtype=torch.float64, device="cuda:0")
    gw[:, 0, nx:nx + nu] = (w[:, nx:nx + nu] - u_t).detach()
    loop.step()  # the loop moves on: the backward used its saved point
    direct, flag = loop.sens_vjp(gw, point=point)
    torch.cuda.synchronize()
    grad = P.grad.cpu().numpy()
    assert int(flag.sum()) == 0 and bits(grad) == bits(direct[:, 0].cpu().numpy())
    res = {"w": point[1].cpu().numpy(), "lam_g": point[2].cpu().numpy(), "lam_x": point[3].cpu().numpy()}
    eye = np.broadcast_to(np.eye(n_p), (B, n_p, n_p)).copy()
    J = solver.sens_p(P0, res, eye)
    assert np.all(J["flag"] == 0)
    g = gw.cpu().numpy()
    gap, bound = identity_gap(g, J["dw"], grad[:, None, :], eye)
    ref = np.einsum("bi,bij->bj", g[:, 0], J["dw"])
    print(f"autograd: |grad| {np.abs(grad).max():.3g}, worst |P.grad - J^T (U_0 - u_t)| {gap.max():.3e}, "
          f"worst gap / bound {np.max(gap / bound):.3e}")
    assert np.all(gap <= bound) and np.max(np.abs(ref)) > 1e-3
    # an irregular instance: U_3 of instance 2 placed on its bound in the saved point
    for mode in ("nan", "zero"):
        Pm = torch.tensor(P0, dtype=torch.float64, device="cuda:0", requires_grad=True)
        wm = solve_differentiable(loop, Pm, irregular=mode)
        fn = wm.grad_fn
        fn.saved_tensors[1].data[2, nx + (nx + nu) * 3] = 1.0  # |v| <= 1 (.data: the saved copy itself, untracked)
        (0.5 * ((wm[:, nx:nx + nu] - u_t) ** 2).sum()).backward()
        gm = Pm.grad.cpu().numpy()
        assert np.all(np.isfinite(gm[[0, 1, 3, 4]])) and np.abs(gm[[0, 1, 3, 4]]).max() > 1e-6
        assert np.all(gm[2] == 0.0) if mode == "zero" else np.all(np.isnan(gm[2]))
    with pytest.raises(ValueError):
        solve_differentiable(loop, P, irregular="skip")
    with pytest.raises(ValueError):
        solve_differentiable(loop, P[:4])


# ------------------------------------------------------------------------------------------
# 7. irregular instances: ordinary statuses, nothing faults; refusals
# ------------------------------------------------------------------------------------------
def assert_only_irregular(v, bad, regular=None):
    for b in range(v["flag"].shape[0]):
        if b == bad:
            assert v["flag"][b] == 1 and np.all(np.isnan(v["gP"][b]))
        else:
            assert v["flag"][b] == 0 and np.all(np.isfinite(v["gP"][b]))
            if regular is not None:  # the neighbours keep their bits
                assert bits(v["gP"][b]) == bits(regular["gP"][b]), b


def test_variable_on_its_bound_is_flagged(mpcx):
    lin, P, r, solver, _, _, g, v = linear_vjp_case("padded_dint_N8")
    w = r["w"].copy()
    w[2, lin.nx + (lin.nx + lin.nu) * 3] = 1.0  # U_3 of instance 2 placed on its upper bound
    assert_only_irregular(solver.sens_vjp(P, {"w": w, "lam_g": r["lam_g"], "lam_x": r["lam_x"]}, g), 2, v)


def test_indefinite_stage_is_flagged(mpcx):
    """A negative input weight on the last stage of instance 1 of 3 (test_gpu_sens_p.py's case)."""
    from mpcx import lti

    rng = np.random.default_rng(11)
    nx, nu, N, B = 4, 1, 20, 3
    A = np.eye(nx) + 0.05 * rng.normal(size=(nx, nx))
    Bm = rng.normal(size=(nx, nu)) + 1.0
    W = np.zeros((2, nx + nu, nx + nu))
    W[:, :nx, :nx] = 5.0 * np.eye(nx)
    W[0, nx, nx] = 0.5
    W[1, nx, nx] = -0.05
    tab = np.zeros((B, N), np.int32)
    tab[1, -1] = 1
    lin = lti.LinearOCP(N=N, A=np.stack([A, A]), B=np.stack([Bm, Bm]), W=W, tab=tab, u_lb=(-1.0,), u_ub=(1.0,))
    solver = mpcx.nlpsol("indef_vjp", "mi355x", lin, {"ipopt": {"max_iter": 300}})
    P = lin.params(rng.normal(size=(B, nx)), np.zeros((N, nx + nu)))
    point = {"w": np.zeros((B, lin.n_w_ms)), "lam_g": np.zeros((B, lin.n_g_ms)), "lam_x": np.zeros((B, lin.n_w_ms))}
    assert_only_irregular(solver.sens_vjp(P, point, rng.normal(size=(B, 2, lin.n_w_ms))), 1)


def test_refusals(mpcx):
    """MPCX_EINVAL with a message and nothing launched, on both entry points: m = 0 and m = nx + 1, a
    null gw or gP, N = 64, the path-frame bicycle (and B < 1, a null point)."""
    import torch
    from mpcx import _lib, ode

    lib = _lib.load()
    EINVAL = -1

    def host_call(solver, B=2, m=1, n_null=()):
        h = solver._h
        n, mm = max(B, 1), max(m, 1)
        arr = [np.zeros((n, h.n_p)), np.zeros((n, h.n_w)), np.zeros((n, h.n_g)), np.zeros((n, h.n_w)),
               np.zeros((n, mm, h.n_w)), np.full((n, mm, h.n_p), 7.0)]
        a = [None if i in n_null else _lib.dptr(v) for i, v in enumerate(arr)]
        rc = lib.mpcx_sens_vjp(h.ptr, B, a[0], a[1], a[2], a[3], None, None, a[4], m, a[5], None)
        assert rc != 0 and np.all(arr[5] == 7.0)
        return rc, lib.mpcx_last_error().decode()

    solver = mpcx.nlpsol("ok_vjp", "mi355x", mpcx.unicycle_point_to_point(N=10), {"ipopt": REF_OPTS})
    long = mpcx.nlpsol("n64_vjp", "mi355x", mpcx.unicycle_point_to_point(N=64), {"ipopt": REF_OPTS})
    path = mpcx.nlpsol("path_vjp", "mi355x", ode.path_bicycle_lane_keeping(N=20), {"ipopt": {"max_iter": 100}})
    buf = torch.zeros(2 * long._h.n_w * 4, dtype=torch.float64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())

    def dev_call(h, B=2, m=1, lam_g=p, gw=p, gP=p):
        rc = lib.mpcx_sens_vjp_dev(h.ptr, B, p, p, lam_g, p, gw, m, gP, None, None)
        return rc, lib.mpcx_last_error().decode()

    for call, hs in ((host_call, (solver, long, path)), (dev_call, (solver._h, long._h, path._h))):
        ok, n64, pth = hs
        for m in (0, 4):
            rc, msg = call(ok, m=m)
            assert rc == EINVAL and "between 1 and nx" in msg, (m, msg)
        for B in (0, -3):
            rc, msg = call(ok, B=B)
            assert rc == EINVAL and "B must be >= 1" in msg
        rc, msg = call(n64)
        assert rc == EINVAL and "N >= 64" in msg
        rc, msg = call(pth)
        assert rc == EINVAL and "path-frame bicycle" in msg
    for i in range(6):  # P, w, lam_g, lam_x, gw, gP
        rc, msg = host_call(solver, n_null=(i,))
        assert rc == EINVAL and "required" in msg
    for kw in ({"lam_g": None}, {"gw": None}, {"gP": None}):
        rc, msg = dev_call(solver._h, **kw)
        assert rc == EINVAL and "required" in msg
    rc = lib.mpcx_sens_vjp_dev(None, 2, p, p, p, p, p, 1, p, None, None)
    assert rc == EINVAL and "null handle" in lib.mpcx_last_error().decode()
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched
