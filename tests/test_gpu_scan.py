"""Device tests of the backward sweeps that had none (mpc-verde_amd/csrc/backward.h), through the
harnesses tests/hip/scan_check.hip and tests/hip/suffix_check.hip, which call the very functions the
solve kernel runs:

* backward_scan (pscan.h relem_stage, relem_combine_lds: the log-depth Riccati scan of five models) and
  the chains it falls back to (backward_chain in 16-, 32- and 64-lane groups, backward_chain_waves),
  against the sequential recursion in numpy long double.  The scan ends with a self-check that sends
  the instance to the sequential recursion, so a wrong combine rule only costs speed and every
  end-to-end test still passes: here the fallback flag itself is asserted.
* dec_suffix_setup, dec_suffix_split and suffix_scan (the reused decoupled suffix of LinearModel<5, 1>
  as a chain and as the radix-4 scan), at suffixes that start at, just before and just after a wave
  boundary, a one-stage suffix, G = 256, a table change inside a launch, and with the scan's
  conditions off.

Tolerances.  Value functions and gains are compared node by node, each quantity normalised by
max(1, max |reference|) at that node, to 64 times the worst error of the float64 restatement of the
scan (test_pscan_cpu's algebra, batched here) against the same long-double reference over all the scan
cases below: the restatement's worst is 5.7e-14 (LinearModel<4, 1>, G = 32, N = 16), so 3.6e-12 -- the
factor pays for the device's fma order, the non-pivoting Gauss-Jordan inverse and rcp64.  The reused
suffix's p_k is held to the a-priori bound of test_suffix_scan_cpu (C_BOUND = 1).

Measured on one MI355X.  The scan's worst error is 1.0e-13 (LinearModel<4, 1>, G = 32, N = 16: 2.4
times the restatement's on that case, 1.8 times its worst, 36 times under the tolerance); its worst
ratio to the restatement on the same case is 40 (LinearModel<4, 2>, G = 64, N = 40, delta = 1e-4: 7.0e-14
against 1.7e-15).  The sequential paths stay within 5.3e-15 (2.2 times the restatement's).  The radix-4
suffix scan reaches 0.26 of the bound at most (G = 256, N = 200, kb = 193; the restatement 0.15), and
below kb the reused paths are within 3.2e-13 of the long-double recursion (G = 256, N = 255, kb = 128,
spectral radius up to 1.02: 5.6 times the scan restatement's worst).  No case disagreed with the
reference.  The NaN case of test_scan_fallback_is_group_uniform did expose a defect: the self-check
took its deviation with fmax, which returns the other operand for a NaN, so an instance with a NaN in
a stage gradient was reported as scanned; backward_scan now also requires the differences' sum to be
finite.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import test_suffix_scan_cpu as sfx
from test_suffix_scan_cpu import LD, inv_small, riccati

pytestmark = pytest.mark.gpu

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip")
SCAN_LIB, SUFFIX_LIB = os.path.join(HIP, "libscan_check.so"), os.path.join(HIP, "libsuffix_check.so")


def full_mask(r, c):
    return [(i, j) for i in range(r) for j in range(c)]


# the models' Jacobian structure (models.h, ode.h): entries of A, B that may be non-zero, entries of A
# that are exactly 1.  KinBicycle: INDEP = {X, Y} (ode.h), so columns 0 and 1 of A are unit vectors
# (OdeModel::amask) and B is dense.
KIN_INDEP = 0b011
MODELS = {
    "unicycle": dict(id=0, nx=3, nu=2, amask=[(0, 0), (0, 2), (1, 1), (1, 2), (2, 2)], aone=[(0, 0), (1, 1), (2, 2)],
                     bmask=[(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)], linear=False),
    "lin41": dict(id=1, nx=4, nu=1, amask=full_mask(4, 4), aone=[], bmask=full_mask(4, 1), linear=True),
    "lin42": dict(id=2, nx=4, nu=2, amask=full_mask(4, 4), aone=[], bmask=full_mask(4, 2), linear=True),
    "kinbicycle": dict(id=3, nx=3, nu=2, amask=[(c, j) for c in range(3) for j in range(3)
                                                 if not (KIN_INDEP >> j) & 1 or c == j],
                       aone=[], bmask=full_mask(3, 2), linear=False),
}
SCAN_CASES = ([("unicycle", G, N) for G, N in [(32, 25), (32, 31), (64, 32), (64, 63), (128, 64), (128, 127)]] +
              [("lin41", G, N) for G, N in [(16, 1), (16, 15), (32, 16), (64, 50), (64, 63), (128, 64), (128, 100),
                                            (256, 128), (256, 255)]] +
              [("lin42", 64, 40), ("kinbicycle", 64, 40)])
DELTAS = [0.0, 1e-4]
INDEFINITE_CASES = [("unicycle", 32, 31), ("lin41", 64, 63)]
FALLBACK_CASES = [("lin41", 16, 15), ("unicycle", 32, 25)]


def batch_of(G):
    return 33 if G < 64 else 5  # sub-wave groups: the last wave has an empty group


def scan_problem(model, G, N, shift=0.0, fallback=False):
    """Random stages with the model's structure (the device code assumes it): entries of A and B
    outside the masks zero, unit entries exactly 1; the linear models draw A (spectral radius 0.95), B,
    c and W = M M^T / nz + 0.1 I from three tables by a random schedule, the others get a stage Hessian
    M M^T / nz + 0.1 I per stage; Sigma in [0, 1], gradients O(1), defects O(1e-2).  `shift`: that
    multiple of I subtracted from Hxx.  `fallback`: every third instance gets one stage with an
    indefinite R = Hd_uu under a large state weight that keeps Huu' = R + B^T P B positive definite,
    and instance 1 a NaN in that stage's gradient."""
    m = MODELS[model]
    nx, nu = m["nx"], m["nu"]
    nz, B = nx + nu, batch_of(G)
    rng = np.random.default_rng(1000 * G + 10 * N + m["id"] + (5 if shift else 0) + (7 if fallback else 0))
    am, bm = np.zeros((nx, nx)), np.zeros((nx, nu))
    for i, j in m["amask"]:
        am[i, j] = 1.0
    for i, j in m["bmask"]:
        bm[i, j] = 1.0
    if m["linear"]:
        tab = rng.integers(0, 3, size=(B, G))
        At = rng.normal(size=(3, nx, nx))
        At *= (0.95 / np.abs(np.linalg.eigvals(At)).max(axis=-1))[:, None, None]
        Mt = rng.normal(size=(3, nz, nz))
        Wt = Mt @ np.swapaxes(Mt, -1, -2) / nz + 0.1 * np.eye(nz)
        A, Bm, c, H = At[tab], rng.normal(size=(3, nx, nu))[tab], 0.1 * rng.normal(size=(3, nx))[tab], 2.0 * Wt[tab]
    else:
        A = np.eye(nx) + 0.2 * rng.normal(size=(B, G, nx, nx)) * (1.0 - np.eye(nx))
        if not m["aone"]:
            A += 0.1 * rng.normal(size=(B, G, nx, nx)) * np.eye(nx)
        Bm = 0.2 * rng.normal(size=(B, G, nx, nu))
        c = 1e-2 * rng.normal(size=(B, G, nx))
        M = rng.normal(size=(B, G, nz, nz))
        H = M @ np.swapaxes(M, -1, -2) / nz + 0.1 * np.eye(nz)
    A, Bm = A * am, Bm * bm
    for i, j in m["aone"]:
        A[..., i, j] = 1.0
    H = H.copy()
    H[..., :nx, :nx] -= shift * np.eye(nx)
    sig, g = rng.uniform(0.0, 1.0, size=(B, G, nz)), rng.normal(size=(B, G, nz))
    bad = np.zeros(B, bool)
    if fallback:
        bad[::3] = True
        j0 = N // 2
        H[bad, :, :nx, :nx] += 5.0 * np.eye(nx)
        H[bad, j0, nx:, nx:] = -0.05 * np.eye(nu)
        H[bad, j0, :nx, nx:] = 0.0
        H[bad, j0, nx:, :nx] = 0.0
        sig[bad, j0, nx:] = 0.0
        Bfix = np.array([[0.3, 0.1], [-0.1, 0.3], [0.0, 0.4], [0.2, -0.2]])[:nx, :nu] if nu == 2 else np.full((nx, 1), 0.5)
        Bm[bad, j0] = Bfix * bm
        g[1, j0, 0] = np.nan
    return dict(model=model, G=G, N=N, B=B, nx=nx, nu=nu, H=H, sig=sig, g=g, A=A, Bm=Bm, c=c, bad=bad)


def operands(pr, delta, dtype):
    nx, nz, N = pr["nx"], pr["nx"] + pr["nu"], pr["N"]
    Hd = pr["H"].astype(dtype) + (pr["sig"].astype(dtype) + dtype(delta))[..., None] * np.eye(nz, dtype=dtype)
    PN = (pr["sig"][:, N, :nx, None].astype(dtype) + dtype(delta)) * np.eye(nx, dtype=dtype)
    return (Hd, pr["A"].astype(dtype), pr["Bm"].astype(dtype), pr["c"].astype(dtype), pr["g"].astype(dtype), N, PN,
            pr["g"][:, N, :nx].astype(dtype))


def scan_restated(Hd, A, Bm, c, g, N, PN, pN, G):
    """backward_scan in float64, batched over instances and lanes: pscan.h's elements (relem_stage),
    combination rule (relem_combine_lds) and scan order as test_pscan_cpu restates them, then one
    Riccati step per node from the scan's value function of node k + 1.  Returns P, p, K, kf as
    riccati() does, and the self-check quantity dev / mag per instance."""
    nx = A.shape[-1]
    Bn = A.shape[0]
    T = lambda X: np.swapaxes(X, -1, -2)  # noqa: E731
    mv = lambda M, v: (M @ v[..., None])[..., 0]  # noqa: E731
    Q, S, R, q, r = Hd[:, :N, :nx, :nx], Hd[:, :N, :nx, nx:], Hd[:, :N, nx:, nx:], g[:, :N, :nx], g[:, :N, nx:]
    F, L, cc = A[:, :N], Bm[:, :N], c[:, :N]
    Ri = inv_small(R)
    eA, eb, eC = np.zeros((Bn, G, nx, nx)), np.zeros((Bn, G, nx)), np.zeros((Bn, G, nx, nx))
    eJ, ep = np.zeros((Bn, G, nx, nx)), np.zeros((Bn, G, nx))
    eA[:, :N], eb[:, :N], eC[:, :N] = F - L @ Ri @ T(S), cc - mv(L @ Ri, r), L @ Ri @ T(L)
    eJ[:, :N], ep[:, :N] = Q - S @ Ri @ T(S), q - mv(S @ Ri, r)
    eJ[:, N], ep[:, N] = PN, pN
    eA[:, N + 1:] = np.eye(nx)  # the identity past node N
    d = 1
    while d < G and d <= N:
        A1, b1, C1, J1, p1 = eA[:, :G - d], eb[:, :G - d], eC[:, :G - d], eJ[:, :G - d], ep[:, :G - d]
        A2, b2, C2, J2, p2 = eA[:, d:], eb[:, d:], eC[:, d:], eJ[:, d:], ep[:, d:]
        Mi = np.linalg.inv(np.eye(nx) + C1 @ J2)
        T1, T2 = A2 @ Mi, Mi @ A1
        new = (T1 @ A1, mv(T1, b1 - mv(C1, p2)) + b2, T1 @ C1 @ T(A2) + C2, T(T2) @ J2 @ A1 + J1,
               mv(T(T2), p2 + mv(J2, b1)) + p1)
        for dst, src in zip((eA, eb, eC, eJ, ep), new):
            dst[:, :G - d] = src
        d *= 2
    P, p = eJ[:, :N + 1].copy(), ep[:, :N + 1].copy()
    Pn, pn = P[:, 1:], p[:, 1:]
    Hxx, Hux, Huu = Q + T(F) @ Pn @ F, T(S) + T(L) @ Pn @ F, R + T(L) @ Pn @ L
    s = pn + mv(Pn, cc)
    gx, gu = q + mv(T(F), s), r + mv(T(L), s)
    Hi = inv_small(Huu)
    K, kf = -Hi @ Hux, -mv(Hi, gu)
    Ps, ps = Hxx + T(Hux) @ K, gx + mv(T(Hux), kf)
    dev = np.maximum(np.abs(Ps - P[:, :N]).max(axis=(1, 2, 3)), np.abs(ps - p[:, :N]).max(axis=(1, 2)))
    mag = np.maximum(1.0, np.maximum(np.abs(Ps).max(axis=(1, 2, 3)), np.abs(ps).max(axis=(1, 2))))
    P[:, :N], p[:, :N] = Ps, ps
    return P, p, K, kf, dev / mag


def node_errors(got, ref):
    """Worst error of (P, p, K, kf) against the reference, each normalised by max(1, max |reference|)
    of that quantity at that node; per instance."""
    out = 0.0
    for a, b in zip(got, ref):
        ax = tuple(range(2, b.ndim))
        with np.errstate(invalid="ignore"):
            e = np.abs(a.astype(LD) - b).max(axis=ax) / np.maximum(1.0, np.abs(b).max(axis=ax))
        out = np.maximum(out, np.where(np.isnan(e), np.inf, e).max(axis=1).astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def scan_case(model, G, N, delta, shift=0.0, fallback=False):
    """The case's operands, its long-double reference, and the float64 restatement's error against it
    (computed once per session, shared, never modified)."""
    pr = scan_problem(model, G, N, shift, fallback)
    ref = riccati(*operands(pr, delta, LD))
    if fallback:
        return pr, ref, None
    rs = scan_restated(*operands(pr, delta, np.float64), G)
    assert np.all(ref[4] > 0) and np.all(rs[4] <= 1e-8)  # well conditioned: the restatement does not fall back
    return pr, ref, float(node_errors(rs[:4], ref[:4]).max())


@functools.lru_cache(maxsize=None)
def scan_tolerance():
    """(64 times the restatement's worst error over all the scan cases, that worst error)."""
    worst = max([scan_case(m, G, N, d)[2] for m, G, N in SCAN_CASES for d in DELTAS] +
                [scan_case(m, G, N, 0.0, 0.5)[2] for m, G, N in INDEFINITE_CASES])
    return 64.0 * worst, worst


def sym_unpack(x, n):
    out = np.zeros(x.shape[:-1] + (n, n))
    for q, (i, j) in enumerate([(i, j) for i in range(n) for j in range(i, n)]):
        out[..., i, j] = out[..., j, i] = x[..., q]
    return out


def sym_pack(M):
    n = M.shape[-1]
    return np.stack([M[..., i, j] for i in range(n) for j in range(i, n)], axis=-1)


def load(path):
    if not os.path.exists(path):
        pytest.fail(f"{path} not built (make -C tests/hip)")
    return ctypes.CDLL(path)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_scan_check(pr, delta):
    """One launch of the harness: (scan record, fallback-path record, flag), records as dicts of
    P, p, K, kf [B, N(+1), ...], okl and fac_ok [B, N+1], fac (the factors' fields)."""
    import torch

    lib = load(SCAN_LIB)
    lib.scan_check.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] + [ctypes.c_void_p] * 4
    m, G, N, B, nx, nu = MODELS[pr["model"]], pr["G"], pr["N"], pr["B"], pr["nx"], pr["nu"]
    n_in, n_out = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.scan_check_sizes(m["id"], ctypes.byref(n_in), ctypes.byref(n_out)) == 0
    x = np.concatenate([sym_pack(pr["H"]), pr["sig"], pr["g"], pr["A"].reshape(B, G, -1), pr["Bm"].reshape(B, G, -1),
                        pr["c"]], axis=-1)
    assert x.shape == (B, G, n_in.value)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    o_scan = torch.full((B, G, n_out.value), np.nan, dtype=torch.float64, device="cuda")
    o_seq = torch.full_like(o_scan, np.nan)
    flag = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    assert lib.scan_check(m["id"], G, N, B, delta, ptr(d_in), ptr(o_scan), ptr(o_seq), ptr(flag)) == 0
    recs = []
    for o in (o_scan, o_seq):
        o = o.cpu().numpy()
        assert np.isnan(o[:, N + 1:]).all()  # nothing written beyond node N
        o = o[:, :N + 1]
        npk = nx * (nx + 1) // 2
        f0 = npk + nx
        k0 = f0 + 5 + 2 * nx
        recs.append(dict(P=sym_unpack(o[..., :npk], nx), p=o[..., npk:f0], fac=o[:, :N, f0:k0],
                         K=o[:, :N, k0:k0 + nu * nx].reshape(B, N, nu, nx), kf=o[:, :N, k0 + nu * nx:k0 + nu * nx + nu],
                         okl=o[..., -2], fac_ok=o[..., -1]))
    return recs[0], recs[1], flag.cpu().numpy()


def quad(rec):
    return rec["P"], rec["p"], rec["K"], rec["kf"]


def check_against_reference(pr, ref, delta, rows=slice(None), rs_err=None):
    """The assertions on well-conditioned instances (`rows`): no fallback, okl on every node lane, both
    records within the tolerance of the long-double reference, fac_ok on every stage lane of the
    fallback path's.  `rs_err`: the restatement's error on this case, for the printed ratio.  Returns
    the records and the worst errors (scan, fallback path)."""
    tol, worst = scan_tolerance()
    rs_err = worst if rs_err is None else rs_err
    scan, seq, flag = run_scan_check(pr, delta)
    np.testing.assert_array_equal(flag[rows], 0)
    np.testing.assert_array_equal(scan["okl"][rows], 1.0)
    e_scan, e_seq = node_errors(quad(scan), ref[:4])[rows].max(), node_errors(quad(seq), ref[:4])[rows].max()
    print(f"{pr['model']} G={pr['G']} N={pr['N']} delta={delta}: scan {e_scan:.2e}, sequential {e_seq:.2e}, "
          f"tolerance {tol:.2e}; restatement {rs_err:.2e}, GPU / restatement {e_scan / rs_err:.2f}, {e_seq / rs_err:.2f}")
    assert e_scan <= tol
    assert e_seq <= tol
    np.testing.assert_array_equal(seq["fac_ok"][rows, :pr["N"]], 1.0)
    np.testing.assert_array_equal(seq["okl"][rows], 1.0)
    return (scan, seq, flag), (e_scan, e_seq)


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("model,G,N", SCAN_CASES)
def test_scan_is_the_long_double_recursion(model, G, N, delta):
    """The scan never falls back on well-conditioned stages (the restatement's self-check quantity is
    six orders under its limit) and its P_k, p_k, K, kf -- and the sequential path's on the same
    operands -- agree with the long-double recursion.  N + 1 = G leaves no identity lane, N = G / 2
    puts the terminal node on the first lane of the upper half or of the next wave, N = 1 is a
    two-level scan, G = 128 and 256 read partners across waves through LDS.  Measured on one MI355X:
    worst GPU error over restatement error on the same case 40 for the scan (7.0e-14 against 1.7e-15,
    LinearModel<4, 2>, delta = 1e-4), 2.2 for the sequential path; worst GPU error 1.0e-13, 1.8 times
    the restatement's worst over all cases (the tolerance allows 64)."""
    pr, ref, rs_err = scan_case(model, G, N, delta)
    check_against_reference(pr, ref, delta, rs_err=rs_err)


@pytest.mark.parametrize("model,G,N", INDEFINITE_CASES)
def test_scan_with_mildly_indefinite_state_hessians(model, G, N):
    """0.5 I subtracted from Hxx, as the exact Lagrangian Hessian of the nonlinear models produces:
    still no fallback, the same tolerance."""
    pr, ref, rs_err = scan_case(model, G, N, 0.0, 0.5)
    check_against_reference(pr, ref, 0.0, rs_err=rs_err)


@pytest.mark.parametrize("model,G,N", FALLBACK_CASES)
def test_scan_fallback_is_group_uniform(model, G, N):
    """Several instances per wave: an instance whose stage R is indefinite (every third) or whose
    gradient holds a NaN (instance 1) reports the fallback, exactly those; the neighbours sharing
    their waves keep their scan results, and the flagged instances' sequential path meets the
    reference (its reduced Huu' is positive definite)."""
    tol, _ = scan_tolerance()
    pr, ref, _ = scan_case(model, G, N, 0.0, 0.0, True)
    bad, nan = pr["bad"], np.arange(pr["B"]) == 1
    assert np.all(ref[4][~nan] > 0)  # the generator's promise: Huu' positive definite at every stage
    want = (bad | nan).astype(np.int32)
    (scan, seq, flag), _ = check_against_reference(pr, ref, 0.0, ~(bad | nan))
    np.testing.assert_array_equal(flag, want)
    e = node_errors(quad(seq), ref[:4])[bad].max()
    print(f"flagged instances, sequential path: {e:.2e}")
    assert e <= tol
    np.testing.assert_array_equal(seq["fac_ok"][bad, :N], 1.0)
    np.testing.assert_array_equal(seq["okl"][bad], 1.0)


# ---- the reused decoupled suffix


def run_suffix_check(pr, shared=True, tab1=None):
    """One launch: passes [3] of dicts P [B, N+1, 5, 5], p, g0, okl, and whether the scan ran.  `tab1`:
    the passes run on pr's schedule first and then, in the same launch, on tab1 (suffix_check_twice)."""
    import torch

    lib = load(SUFFIX_LIB)
    lib.suffix_check.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 5
    lib.suffix_check_twice.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 6
    G, N, kb, B = pr["G"], pr["N"], pr["kb"], pr["B"]
    x = np.concatenate([sym_pack(pr["H"]), pr["sig"], pr["g"], pr["Bm"].reshape(B, G, -1), pr["c"]], axis=-1)
    assert x.shape == (B, G, 43) and pr["tab"].min() >= 0 and pr["tab"].max() < sfx.N_TAB
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_A = torch.from_numpy(np.ascontiguousarray(pr["A"])).cuda()
    d_tab = torch.from_numpy(np.ascontiguousarray(pr["tab"])).cuda()
    out = torch.full((B, 3, G, 22), np.nan, dtype=torch.float64, device="cuda")
    ran = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    if tab1 is None:
        rc = lib.suffix_check(G, N, kb, B, sfx.N_TAB, int(shared), ptr(d_in), ptr(d_A), ptr(d_tab), ptr(out), ptr(ran))
    else:
        assert tab1.shape == pr["tab"].shape and tab1.dtype == np.int32 and tab1.min() >= 0 and tab1.max() < sfx.N_TAB
        d_tab1 = torch.from_numpy(np.ascontiguousarray(tab1)).cuda()
        rc = lib.suffix_check_twice(G, N, kb, B, sfx.N_TAB, ptr(d_in), ptr(d_A), ptr(d_tab), ptr(d_tab1), ptr(out), ptr(ran))
    assert rc == 0
    o = out.cpu().numpy()
    assert np.isnan(o[:, :, N + 1:]).all() and not np.isnan(o[:, :, :N + 1]).any()
    o = o[:, :, :N + 1]
    return o, ran.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def assert_pass_equal(a, b):
    """p_k, g0 and okl bit for bit; P_k bit for bit up to the sign of an exact zero."""
    np.testing.assert_array_equal(bits(a[..., 15:]), bits(b[..., 15:]))
    np.testing.assert_array_equal(a[..., :15], b[..., :15])  # (no NaN here: -0.0 == 0.0, nothing looser)


@pytest.mark.parametrize("G,N,kb", sfx.CASES)
def test_reused_suffix_chain_and_scan(G, N, kb):
    """Pass 2 (the reused suffix as a chain) is pass 1 (the fresh factorisation) bit for bit; pass 3's
    scan runs on every instance, its p_k on the suffix meets the a-priori bound of test_suffix_scan_cpu
    against the long-double chain on the stored P_k, and below kb passes 2 and 3 meet the long-double
    full recursion to the scan tests' tolerance.  Measured on one MI355X: C_BOUND = 1 and the scan at
    most 0.26 of it (G = 256, N = 200, kb = 193; the float64 restatement 0.15); below kb at most 3.2e-13
    (G = 256, N = 255, kb = 128), 5.6 times the scan restatement's worst."""
    tol, worst = scan_tolerance()
    pr = sfx.suffix_problem(G, N, kb)
    o, ran = run_suffix_check(pr)
    np.testing.assert_array_equal(ran, 1)
    assert_pass_equal(o[:, 1], o[:, 0])
    np.testing.assert_array_equal(o[:, :, :, 21], 1.0)  # okl: every Huu' here is positive definite
    P1 = sym_unpack(o[:, 0, :, :15], 5)
    ratio = max(sfx.suffix_bound_ratio(pr, P1[b], o[b, 2, :, 15:20], b) for b in range(pr["B"]))
    np.testing.assert_array_equal(bits(o[:, 2, kb:, :15]), bits(o[:, 1, kb:, :15]))  # the stored P_k, both ways
    np.testing.assert_array_equal(bits(o[:, 2, kb:, 20:]), bits(o[:, 1, kb:, 20:]))  # g0, okl on the suffix
    ref = riccati(*sfx.stage_operands(pr, LD), N, *sfx.terminal(pr, LD))
    errs = [0.0, 0.0]
    for ps in (1, 2) if kb > 0 else ():
        got = (sym_unpack(o[:, ps, :kb, :15], 5), o[:, ps, :kb, 15:20])
        errs[ps - 1] = float(node_errors(got, (ref[0][:, :kb], ref[1][:, :kb])).max())
    print(f"G={G} N={N} kb={kb}: scan error {ratio:.3f} of the bound's unit (C_BOUND {sfx.C_BOUND}); nodes < kb "
          f"against long double: chain {errs[0]:.2e}, scan {errs[1]:.2e}, tolerance {tol:.2e} "
          f"(GPU / restatement {max(errs) / worst:.2f})")
    assert ratio <= sfx.C_BOUND
    assert max(errs) <= tol


@pytest.mark.parametrize("G,N,kb", sfx.CASES)
def test_suffix_table_change_inside_a_launch(G, N, kb):
    """The matrix powers cached in LDS belong to one table: a second factorisation in the same launch
    whose suffix uses another table gives, bit for bit, what a fresh launch on that table gives."""
    pr0, pr1 = sfx.suffix_problem(G, N, kb, suffix_tab=1), sfx.suffix_problem(G, N, kb, suffix_tab=2)
    assert (pr0["tab"][:, kb:N] != pr1["tab"][:, kb:N]).all() and (pr0["tab"][:, :kb] == pr1["tab"][:, :kb]).all()
    fresh, ran_f = run_suffix_check(pr1)
    twice, ran_t = run_suffix_check(pr0, tab1=pr1["tab"])
    np.testing.assert_array_equal(ran_f, 1)
    np.testing.assert_array_equal(ran_t, 1)
    np.testing.assert_array_equal(bits(twice), bits(fresh))


@pytest.mark.parametrize("G,N,kb", sfx.CASES)
def test_suffix_scan_conditions_off(G, N, kb):
    """Without shared tables, or with two tables inside the suffix, the scan does not run and pass 3
    is pass 2 bit for bit (and pass 2 still pass 1)."""
    variants = [(sfx.suffix_problem(G, N, kb), False)]
    if N - kb >= 2:
        variants.append((sfx.suffix_problem(G, N, kb, split=True), True))
        assert len(np.unique(variants[1][0]["tab"][0, kb:N])) == 2
    for pr, shared in variants:
        o, ran = run_suffix_check(pr, shared=shared)
        np.testing.assert_array_equal(ran, 0)
        np.testing.assert_array_equal(bits(o[:, 2]), bits(o[:, 1]))
        assert_pass_equal(o[:, 1], o[:, 0])
