"""CPU tests of the references of the sensitivities to the model (tests/helpers/sens_model_ref.py), which
tests/test_gpu_sens_model.py holds the kernels csrc/sens.h sens_mdl_kernel / sens_mdl_vjp_kernel to, and of the C
ABI's new entry points.  Nothing here runs the kernels: the ODE points are the CPU oracle's solutions of the cases of
tests/test_gpu_sens.py (tests/test_sens_nonlinear_cpu.py's cpu_case, shared), the linear ones seeded LQ problems.

1. the two-round recursion with both right-hand sides (the first with d != 0) against the dense KKT solve;
2. the linear closed form against central differences of a fixed-mu barrier LQ solve under perturbed A, B, c -- and
   the teeth of that check: without d_k, or without the mixed term r_k, it fails;
3. the hyper-dual tangent matrices G, D of the ODE models against central differences, in long double, of the
   models' own first derivatives under perturbed constants;
4. the reverse references against the forward ones (the dot-product identity: sign and costate convention);
5. the ODE references have teeth: dropping d_k or the mixed term moves them far beyond the GPU test's bound;
6. the yardsticks E64(case, call), printed and asserted <= 1e-12;
7. the header declares the entry points, the library exports them, the binding lists them.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import sens_bounds_ref as sb  # noqa: E402
import sens_model_ref as sm  # noqa: E402
import sens_nonlinear_ref as sn  # noqa: E402
import sens_p_ref as sp  # noqa: E402
import sens_ref as sr  # noqa: E402
import sens_vjp_ref as sv  # noqa: E402
import stage_derivs_ref as sd  # noqa: E402
import test_sens_nonlinear_cpu as tn  # noqa: E402  (cpu_case / points_of: the oracle's solutions, cached there)

LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")
HDR = os.path.join(ROOT, "include", "mpcx.h")
SYMBOLS = ("mpcx_model_dims", "mpcx_set_par", "mpcx_sens_model", "mpcx_sens_model_dev", "mpcx_sens_model_vjp",
           "mpcx_sens_model_vjp_dev")
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
LQ_CASES = [(s, shape, sg) for s, shape in enumerate(sr.LQ_SHAPES) for sg in sr.LQ_SIGMAS]
ODE_CASES = ("kin_bicycle_N10", "cartpole_N20", "path_bicycle_N20", "dyn_bicycle_N10")


def lq_problem(seed, shape, sigma, states=True):
    """Random LQ stages with Sigma on a seeded 40 % of the inputs and on two states (states=False: on the inputs
    alone, the mask of the helpers' yardsticks e_ref_p, e_ref_w: the reverse mode's outputs are formed from the
    costates lam~ = P X~ + p~, and under a Sigma of 1e9 on a state, P of 1e9 times an X~ of 1e-9, they are
    ill-conditioned whatever computes them), seeded stage points and multipliers, and nx seeded per-stage
    directions of the tables (A, B, c)"""
    nx, nu, N = shape
    A, B, H = sr.random_lq(nx, nu, N, seed)
    if states:
        lo, up = sb.random_bound_mask(nx, nu, N, seed)
        Sig = sb.stage_sigma(np.where(lo | up, sigma, 0.0), nx, nu)
    else:
        Sig = np.where(sr.random_input_mask(nx, nu, N, seed), sigma, 0.0)
    rng = np.random.default_rng(seed + 11000)
    Z, lam = rng.normal(size=(N, nx + nu)), rng.normal(size=(N, nx))
    dth = rng.normal(size=(nx, N, nx * nx + nx * nu + nx))
    return A, B, H, Sig, Z, lam, dth


# ------------------------------------------------------------------------------------------
# 1. the recursion with d != 0 against the dense KKT solve
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, shape, sigma", LQ_CASES)
def test_recursion_against_the_dense_kkt_solve(seed, shape, sigma):
    """The two rounds with the linear model's right-hand sides (r_k and d_k both non-zero) against the dense solve
    of the same system, float64: 16 x cond x eps x max(1, |dw|_max), tests/test_sens_p_cpu.py's rule.  dX_0 = 0
    exactly; one round alone equals sens_p_ref.affine_sens bit for bit."""
    nx, nu, N = shape
    A, B, H, Sig, Z, lam, dth = lq_problem(seed, shape, sigma)
    r, d = sm.linear_rhs(nx, nu, Z, lam, dth, np.float64)
    assert np.abs(d).max() > 1e-3 and np.abs(r).max() > 1e-3
    dw, ok = sm.forward(A, B, H, Sig, r, d, np.float64)
    assert ok and not dw[:nx].any()
    plain, _ = sp.affine_sens(A, B, H, Sig, r, d, np.zeros((nx, nx)))
    assert np.array_equal(sm.forward(A, B, H, Sig, r, d, np.float64, rounds=1)[0], plain)
    ref, cond = sp.dense_kkt_sens(A, B, H, Sig, r, d, np.zeros((nx, nx)))
    tol = 16.0 * cond * EPS * max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(dw - ref)))
    print(f"{shape} Sigma {sigma:g}: |two rounds - dense| {err:.3e}, cond {cond:.3e}, bound {tol:.3e}")
    assert err <= tol and np.max(np.abs(dw)) > 1e-3


# ------------------------------------------------------------------------------------------
# 2. the linear closed form against central differences of a barrier solve
# ------------------------------------------------------------------------------------------
def barrier_lq_model(A, B, cd, H, c, x0, lb, ub, mu, w_start, tol=1e-12, max_iter=200):
    """sens_bounds_ref.barrier_lq with an offset cd (N, nx) in the dynamics X_{k+1} = A_k X_k + B_k U_k + cd_k, and the
    multipliers of the defects returned too, in the kernel's convention (g_{k+1} = F_k - X_{k+1}, a plus sign):
    (w, lam_x, lam (N, nx), residual norm)"""
    A, B, H = (np.asarray(v, np.float64) for v in (A, B, H))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    Hw, J, _, rhs = sp._kkt(A, B, H, np.zeros((N, nx + nu, 1)), np.asarray(cd, float)[:, :, None], np.asarray(x0, float)[:, None])
    rhs = rhs[:, 0]
    nw, ng = Hw.shape[0], J.shape[0]
    hl, hu = lb > -sr.INF_BOUND, ub < sr.INF_BOUND
    hl[:nx] = hu[:nx] = False
    w, lam = np.array(w_start, float), np.zeros(ng)

    def resid(w, lam):
        zL = np.where(hl, mu / np.where(hl, w - lb, 1.0), 0.0)
        zU = np.where(hu, mu / np.where(hu, ub - w, 1.0), 0.0)
        return np.concatenate([Hw @ w + c - zL + zU + J.T @ lam, J @ w - rhs]), zL, zU

    for _ in range(max_iter):
        F, zL, zU = resid(w, lam)
        nrm = float(np.max(np.abs(F)))
        if nrm <= tol:
            break
        Sg = np.where(hl, zL / np.where(hl, w - lb, 1.0), 0.0) + np.where(hu, zU / np.where(hu, ub - w, 1.0), 0.0)
        step = np.linalg.solve(np.block([[Hw + np.diag(Sg), J.T], [J, np.zeros((ng, ng))]]), -F)
        dw, dl = step[:nw], step[nw:]
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = np.where(hl & (dw < 0), -(w - lb) / dw, np.inf)
            tu = np.where(hu & (dw > 0), (ub - w) / dw, np.inf)
        a = min(1.0, 0.99 * float(min(tl.min(), tu.min())))
        while a > 1e-12 and float(np.max(np.abs(resid(w + a * dw, lam + a * dl)[0]))) > (1 - 1e-4 * a) * nrm:
            a *= 0.5
        w, lam = w + a * dw, lam + a * dl
    F, zL, zU = resid(w, lam)
    # J's row block k + 1 is X_{k+1} - A_k X_k - B_k U_k: the kernel's defect with the other sign
    return w, zU - zL, -lam[nx:].reshape(N, nx), float(np.max(np.abs(F)))


@pytest.mark.parametrize("seed, shape", list(enumerate(sr.LQ_SHAPES))[:3])
def test_linear_against_central_differences_of_a_barrier_solve(seed, shape):
    """A fixed-mu (1e-3) barrier LQ problem with one-sided bounds (tests/test_sens_weights_cpu.py's), its tables
    perturbed along seeded (dA_k, dB_k, dc_k): column 0 one direction per stage, column 1 the same at every stage.
    Central differences at h = 1e-4 and h / 2; asserted |dw - FD(h/2)| <= spread + 1e-7 -- and, the teeth, that the
    same check FAILS by a factor 100 and more without d_k, and without the mixed term r_k: both terms, their signs
    and the multiplier's sign and index are pinned by the problem itself."""
    nx, nu, N = shape
    nz, nw = nx + nu, nx + (nx + nu) * N
    A, B, H = sr.random_lq(nx, nu, N, seed)
    lo, up = sb.random_bound_mask(nx, nu, N, seed)
    rng = np.random.default_rng(seed + 12000)
    c, x0, cd = rng.normal(size=nw), rng.normal(size=nx), rng.normal(size=(N, nx))
    mu = 1e-3
    free = (np.full(nw, -1e20), np.full(nw, 1e20))
    w_unc, _, _, res = barrier_lq_model(A, B, cd, H, c, x0, *free, mu, np.zeros(nw))
    assert res <= 1e-11
    off = rng.choice([-0.05, 0.3], size=nw)
    lb, ub = np.where(lo, w_unc - off, -1e20), np.where(up, w_unc + off, 1e20)
    start = np.where(lo, np.maximum(w_unc, lb + 0.1), np.where(up, np.minimum(w_unc, ub - 0.1), w_unc))
    w, lam_x, lam, res = barrier_lq_model(A, B, cd, H, c, x0, lb, ub, mu, start)
    assert res <= 1e-11 and np.sum(np.abs(lam_x) > 1e-2) >= 2
    Sig = sr.sigma_of(w, lam_x, lb, ub, nx, nu)
    dth = 0.3 * rng.normal(size=(2, N, nx * nx + nx * nu + nx))
    dth[1] = dth[1, 0]  # the stage-uniform column
    Z = np.stack([np.concatenate([w[sr.ix_w(nx, nu, k)], w[sr.iu_w(nx, nu, k)]]) for k in range(N)])
    r, d = sm.linear_rhs(nx, nu, Z, lam, dth, np.float64)
    dw, ok = sm.forward(A, B, H, Sig, r, d, np.float64)
    assert ok
    dA = dth[..., :nx * nx].reshape(2, N, nx, nx)
    dB = dth[..., nx * nx:nx * nx + nx * nu].reshape(2, N, nx, nu)
    dc = dth[..., nx * nx + nx * nu:]
    fd = {}
    for h in (1e-4, 5e-5):
        cols = []
        for j in range(2):
            side = []
            for sgn in (1.0, -1.0):
                wl, _, _, res = barrier_lq_model(A + sgn * h * dA[j], B + sgn * h * dB[j], cd + sgn * h * dc[j], H, c, x0,
                                                 lb, ub, mu, w)
                assert res <= 1e-11
                side.append(wl)
            cols.append((side[0] - side[1]) / (2 * h))
        fd[h] = np.stack(cols, axis=1)
    spread = float(np.max(np.abs(fd[1e-4] - fd[5e-5])))
    err = float(np.max(np.abs(dw - fd[5e-5])))
    no_d = float(np.max(np.abs(sm.forward(A, B, H, Sig, r, 0.0 * d, np.float64)[0] - fd[5e-5])))
    no_r = float(np.max(np.abs(sm.forward(A, B, H, Sig, 0.0 * r, d, np.float64)[0] - fd[5e-5])))
    flip = float(np.max(np.abs(sm.forward(A, B, H, Sig, -r, d, np.float64)[0] - fd[5e-5])))
    print(f"{shape}: |dw| {np.abs(dw).max():.3g}, FD spread {spread:.3e}, |dw - FD| {err:.3e}; without d_k {no_d:.3e}, "
          f"without the mixed term {no_r:.3e}, with the multiplier's sign flipped {flip:.3e}")
    assert err <= spread + 1e-7
    assert min(no_d, no_r, flip) > 100.0 * (spread + 1e-7)
    assert np.min(np.max(np.abs(dw), axis=0)) > 1e-3  # both columns move the solution


# ------------------------------------------------------------------------------------------
# 3. the ODE models' tangent matrices against central differences in long double
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ode_points(name):
    """[(ocp, P_b, sol_b, pt, pt64)] of a case at the oracle's solution"""
    ocp, P, r, lb, ub, _ = tn.cpu_case(name)
    return [(ocp, P[b], tn.sol_of(r, b), pt, pt64) for b, (pt, pt64) in enumerate(tn.points_of(name))]


@pytest.mark.parametrize("name", ODE_CASES)
def test_tangent_matrices_against_central_differences(name):
    """G = d(grad_z (q + lam^T F))/dpar and D = dF/dpar of the hyper-dual passes with the constants seeded, against
    central differences (h = 1e-6 |par_j|, long double: truncation h^2, cancellation 1e-19 / h) of
    stage_derivs_ref.stage_derivs' own g + [A B]^T lam and xf at perturbed constants: relative 1e-8 of the largest
    entry of each block.  Every constant of the row moves something; the path-frame bicycle's L and w_z move G alone
    (they are in its cost hook), and its G carries the hook's term (asserted: G[:, 3:5] of w_z is not zero)."""
    ocp, P_b, sol, pt, _ = ode_points(name)[0]
    model, nx, nu = sn.model_of(ocp), ocp.nx, ocp.nu
    lam = sn.multipliers(ocp, sol["lam_g"], LD)
    zr = pt.zr.copy()
    if model == "path_bicycle":  # (the case's path is straight: a curvature, so that L -- which acts through L kappa -- shows)
        zr[:, 3] = 0.02
    G, D = sm.ode_tangent(ocp, pt.Z, zr, lam, LD)

    def first(par):
        d = sd.stage_derivs(model, pt.Z, lam, zr, 1.0, ocp.T, ocp.M, ocp.Q, ocp.R, par, LD, cost=ocp.cost)
        gl = d["g"] + np.concatenate([np.einsum("kri,kr->ki", d["A"], lam), np.einsum("kri,kr->ki", d["B"], lam)], axis=1)
        return gl, d["xf"]

    par = np.array(ocp.par, LD)
    for j in range(sm.N_TH[model]):
        h = LD(1e-6) * abs(par[j])
        up, dn = par.copy(), par.copy()
        up[j] += h
        dn[j] -= h
        (gu, xu), (gd, xd) = first(list(up)), first(list(dn))
        Gf, Df = (gu - gd) / (2 * h), (xu - xd) / (2 * h)
        eg = float(np.max(np.abs(G[:, :, j] - Gf)) / max(float(np.max(np.abs(Gf))), 1e-300))
        ed = float(np.max(np.abs(D[:, :, j] - Df)) / max(float(np.max(np.abs(Df))), 1e-300)) if np.any(Df) else 0.0
        print(f"{name} {sm.PAR_NAMES[model][j]}: |G| {float(np.max(np.abs(G[:, :, j]))):.3g} off by {eg:.2e}, "
              f"|D| {float(np.max(np.abs(D[:, :, j]))):.3g} off by {ed:.2e}")
        assert eg <= 1e-8 and ed <= 1e-8
        assert np.any(G[:, :, j]) or np.any(D[:, :, j])
        if model == "path_bicycle" and j in (0, 3):
            assert not np.any(D[:, :, j]) and np.any(G[:, 3:5, j])


# ------------------------------------------------------------------------------------------
# 4. reverse against forward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, shape, sigma", LQ_CASES)
def test_linear_dot_product_identity(seed, shape, sigma):
    """<g, dw> = <gthk, dth> for the linear closed forms, nx seeded per-stage directions of (A, B, c) against nx seeded
    cotangents, in float64 (residuals in long double) and long double: relative to the sum of the absolute terms
    of both sides, 2^20 roundings (tests/test_sens_vjp_cpu.py's bound).  With the costate of the stage's own node in
    place of the next one's, or the sign of the d-term flipped, the identity is off by more than 1e-3."""
    nx, nu, N = shape
    A, B, H, Sig, Z, lam, dth = lq_problem(seed, shape, sigma, states=False)
    g = sv.random_cotangent(nx, nu, N, seed).T  # (m, n_w)
    for dt, bound in ((np.float64, 2.0 ** 20 * EPS), (LD, 2.0 ** 20 * float(np.finfo(LD).eps))):
        Zd, ld, dd = (np.asarray(v, dt) for v in (Z, lam, dth))
        r, d = sm.linear_rhs(nx, nu, Zd, ld, dd, dt)
        dw, _ = sm.forward(A, B, H, Sig, r, d, dt)
        zt, lt, _ = sm.adjoint(A, B, H, Sig, g, dt)
        gk = sm.linear_cotangent(nx, nu, Zd, ld, zt, lt)
        gd = np.asarray(g, dt)
        lhs, rhs = gd @ dw, np.einsum("ckn,dkn->cd", gk, dd)
        mag = np.abs(gd) @ np.abs(dw) + np.einsum("ckn,dkn->cd", np.abs(gk), np.abs(dd))
        viol = float(np.max(np.abs(lhs - rhs) / mag))
        print(f"{shape} Sigma {sigma:g}: identity violation {viol:.3e} in {np.dtype(dt).name}")
        assert viol <= bound
        wrong = sm.linear_cotangent(nx, nu, Zd, ld, zt, -lt)
        assert np.max(np.abs(lhs - np.einsum("ckn,dkn->cd", wrong, dd))) > 1e-3


@pytest.mark.parametrize("name", ODE_CASES)
def test_ode_reverse_reference_against_the_forward_one(name):
    """<g, dw> = <gthk, dth> in long double at the oracle's points: nx seeded per-stage relative directions against nx
    seeded cotangents.  Bound: 64 x 2^-11 x max(E64 of the two calls, e_ref_p) x (sum |g| max(1, |dw|) + sum
    max(1, |gthk|) |dth|), tests/test_sens_nonlinear_cpu.py's.  gth is the stage sum."""
    worst = 0.0
    Y = yardsticks(name)
    unit = 64.0 * 2.0 ** -11 * max(Y["model"], Y["model_vjp"], sp.e_ref_p())
    for b, (ocp, P_b, sol, pt, _) in enumerate(ode_points(name)):
        dth, gw = directions(ocp, b)
        dw, _ = sm.reference_model(pt, sol, dth)
        gk, gs, _ = sm.reference_model_vjp(pt, sol, gw)
        g = np.asarray(gw, LD)
        big = lambda v: np.maximum(1.0, np.abs(v))  # noqa: E731
        lhs, rhs = g @ dw, np.einsum("ckn,dkn->cd", gk, np.asarray(dth, LD))
        sc = np.abs(g) @ big(dw) + np.einsum("ckn,dkn->cd", big(gk), np.abs(np.asarray(dth, LD)))
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / (unit * sc))))
        assert np.array_equal(gs, gk.sum(axis=1))
    print(f"{name}: worst identity gap / bound {worst:.3e} (unit {unit:.2e})")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------
# 5, 6. teeth and yardsticks at the oracle's points
# ------------------------------------------------------------------------------------------
def directions(ocp, b):
    """(dth (nx, N, n_th) seeded, relative to each constant's size; gw (nx, n_w) seeded normal) of instance b"""
    nw = ocp.nx + (ocp.nx + ocp.nu) * ocp.N
    return sm.relative_directions(ocp, ocp.nx, 400 + b), np.random.default_rng(500 + b).normal(size=(ocp.nx, nw))


@functools.lru_cache(maxsize=None)
def yardsticks(name):
    out = {"model": 0.0, "model_vjp": 0.0}
    for b, (ocp, P_b, sol, pt, pt64) in enumerate(ode_points(name)):
        dth, gw = directions(ocp, b)
        for call, arg in (("model", dth), ("model_vjp", gw)):
            e, _, ok = sm.e64(call, pt, pt64, sol, arg)
            assert ok
            out[call] = max(out[call], e)
    return out


@pytest.mark.parametrize("name", ODE_CASES)
def test_yardsticks(name):
    """E64(case, call): the float64 pipeline (float64 hyper-dual tangent and operands, the float64 rounds with
    residuals in long double) against the long-double one, relative to max(1, |entry|), worst instance, for
    directions relative to each constant's size.  A reference that is itself ill-conditioned is no reference:
    E64 <= 1e-12."""
    Y = yardsticks(name)
    print(f"{name}: E64 model {Y['model']:.2e}  model_vjp {Y['model_vjp']:.2e}")
    assert 0.0 < Y["model"] <= 1e-12 and 0.0 < Y["model_vjp"] <= 1e-12


@pytest.mark.parametrize("seed, shape, sigma", LQ_CASES)
def test_linear_yardsticks(seed, shape, sigma):
    """The same for the linear closed forms on the seeded LQ problems: E64 <= 1e-12."""
    nx, nu, N = shape
    A, B, H, Sig, Z, lam, dth = lq_problem(seed, shape, sigma, states=False)
    g = sv.random_cotangent(nx, nu, N, seed).T
    out = []
    for dt in (np.float64, LD):
        r, d = sm.linear_rhs(nx, nu, Z, lam, dth, dt)
        zt, lt, _ = sm.adjoint(A, B, H, Sig, g, dt)
        out.append((sm.forward(A, B, H, Sig, r, d, dt)[0], sm.linear_cotangent(nx, nu, np.asarray(Z, dt), np.asarray(lam, dt), zt, lt)))
    ef, er = sr.rel_err(out[0][0], out[1][0]), sr.rel_err(out[0][1], out[1][1])
    print(f"{shape} Sigma {sigma:g}: E64 forward {ef:.2e}, reverse {er:.2e}")
    assert ef <= 1e-12 and er <= 1e-12


@pytest.mark.parametrize("name", ODE_CASES)
def test_the_reference_has_teeth(name):
    """Dropping the defect term d_k, or the mixed term r_k, moves dw by more than 1000 x the GPU test's bound of the
    case, 64 E64(case, model); the worst instance counts.  (The path-frame bicycle: L and w_z act through r_k
    alone, c1 and c2 through both.)"""
    need = 1000.0 * 64.0 * yardsticks(name)["model"]
    moved = {"drop_defect": 0.0, "drop_mixed": 0.0}
    for b, (ocp, P_b, sol, pt, _) in enumerate(ode_points(name)):
        dth, _ = directions(ocp, b)
        ref, _ = sm.reference_model(pt, sol, dth)
        for key in moved:
            moved[key] = max(moved[key], sr.rel_err(sm.reference_model(pt, sol, dth, **{key: True})[0], ref))
    print(f"{name}: without d_k dw moves by {moved['drop_defect']:.3e}, without the mixed term by {moved['drop_mixed']:.3e}; "
          f"1000 x the GPU bound = {need:.3e}")
    assert moved["drop_defect"] > need and moved["drop_mixed"] > need


# ------------------------------------------------------------------------------------------
# 7. the C ABI: the entry points are declared and exported
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mpc-verde_amd")], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_the_entry_points():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*int\s+(mpcx_\w+)\s*\(", src, re.M))
    for s in SYMBOLS:
        assert s in declared, s
    # the header states the right-hand sides, the reverse formula, the identity and the unicycle's refusal
    for text in ("d_k = (dF_k/dth) dTh_k", "d_k = dA_k x_k + dB_k u_k + dc_k", "r_k = (dA_k^T lam_{k+1}; dB_k^T lam_{k+1})",
                 "gThk_k = (dr_k/dth_k)^T z~_k + (dd_k/dth_k)^T lam~_{k+1}", "B x m x (per_stage ? N : 1) x n_th",
                 "MPCX_MODEL_UNICYCLE: 0"):
        assert text in src, text


def test_library_exports_the_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(rf"\bT {s}$", out, re.M), s


def test_python_binding_lists_the_entry_points():
    import mpcx
    from mpcx.autograd import MPCParFunction
    from mpcx.device import DeviceLoop

    for s in SYMBOLS:
        assert s in mpcx._lib.EXPORTS
    assert callable(mpcx.Solver.sens_model) and callable(mpcx.Solver.sens_model_vjp) and callable(mpcx.Solver.set_par)
    assert callable(DeviceLoop.sens_model) and callable(DeviceLoop.sens_model_vjp)
    assert callable(MPCParFunction.apply)
