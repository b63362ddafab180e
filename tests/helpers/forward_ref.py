"""References for the solve kernel's forward sweep and step lengths (mpc-verde_amd/csrc/forward.h:
forward_sweep, bound_step, step_lengths), shared by tests/test_forward_cpu.py and
tests/test_gpu_forward.py:

* sweep_reference: the sequential recursion in numpy long double,
      dx_0 = c0,  dx_1 = c_0 + B_0 kf_0 (whatever A_0 and K_0 hold),
      dx_{k+1} = (A_k + B_k K_k) dx_k + c_k + B_k kf_k,
      du_k = kf_k + K_k dx_k (k < N; 0 at k = N),  dlam_k = P_k dx_k + p_k - lam_k,  zeros beyond N;
* sweep_restated: the device's composition order restated in numpy, batched over instances and lanes --
  the closed-loop maps, the in-row Kogge-Stone levels, the two row broadcasts with scan_takes and the
  chaining of the waves -- in the dtype of its operands: float64, or Python integers (dtype object) for
  the exact cases, with every intermediate handed to a callback;
* steps_reference: the bound-dual steps and the step lengths in long double, and slack_shortfall, a
  brute-force check of a step length against the fraction-to-boundary rule;
* the problem generators of the cases (exact integer operands, rounded operands of a given spectral
  radius, interior iterates for the step lengths) and the record layout of tests/hip/forward_check.hip.
"""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52  # kernels.h kEps
U = 2.0 ** -53    # unit round-off of float64


def full_mask(r, c):
    return [(i, j) for i in range(r) for j in range(c)]


def ode_amask(nx, indep):
    """OdeModel::amask (ode.h): column j of A is the unit vector e_j when f does not read x_j."""
    return [(c, j) for c in range(nx) for j in range(nx) if not (indep >> j) & 1 or c == j]


# the models forward_check.hip instantiates and the groups it has them at; entries of A and B the device reads
MODELS = {
    "unicycle": dict(id=0, nx=3, nu=2, amask=[(0, 0), (0, 2), (1, 1), (1, 2), (2, 2)],
                     bmask=[(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)], groups=(16, 32, 64, 128)),
    "lin41": dict(id=1, nx=4, nu=1, amask=full_mask(4, 4), bmask=full_mask(4, 1), groups=(16, 32, 64, 128, 256)),
    "lin42": dict(id=2, nx=4, nu=2, amask=full_mask(4, 4), bmask=full_mask(4, 2), groups=(64,)),
    "pathbicycle": dict(id=3, nx=4, nu=2, amask=ode_amask(4, 0), bmask=full_mask(4, 2), groups=(64,)),
    "dynbicycle": dict(id=4, nx=6, nu=2, amask=ode_amask(6, 0b11), bmask=full_mask(6, 2), groups=(64,)),
}
HORIZONS = {16: (1, 8, 15), 32: (16, 17, 31), 64: (32, 33, 63), 128: (64, 65, 127),
            256: (128, 129, 191, 192, 193, 255)}
CASES = [(m, G, N) for m, d in MODELS.items() for G in d["groups"] for N in HORIZONS[G]]
HOT_CASE = ("lin41", 64, 63)  # the one case at spectral radius 1.1


def batch_of(G):
    return 33 if G < 64 else 5  # sub-wave groups: several instances per wave, an empty group in the last wave


def masks(model, dtype=np.float64):
    m = MODELS[model]
    am, bm = np.zeros((m["nx"], m["nx"]), dtype), np.zeros((m["nx"], m["nu"]), dtype)
    for i, j in m["amask"]:
        am[i, j] = 1
    for i, j in m["bmask"]:
        bm[i, j] = 1
    return am, bm


def mask_bits(model):
    """(AMASK, BMASK) as the device holds them: bit r * NX + m, r * NU + l."""
    m = MODELS[model]
    return (sum(1 << (i * m["nx"] + j) for i, j in m["amask"]), sum(1 << (i * m["nu"] + j) for i, j in m["bmask"]))


def mv(M, v):
    return (M @ v[..., None])[..., 0]


def sym_pack(M):
    n = M.shape[-1]
    return np.stack([M[..., i, j] for i in range(n) for j in range(i, n)], axis=-1)


# ---------------------------------------------------------------------------------- the forward sweep
SWEEP_KEYS = ("A", "Bm", "K", "P", "lam")
RHS_KEYS = ("cc", "kf", "pv", "c0v")


def sweep_reference(pr, call=0):
    """The sequential recursion in long double: (dz [B, G, nz], dlam [B, G, nx]) of right-hand side `call`."""
    N, G, nx, nu = pr["N"], pr["G"], pr["nx"], pr["nu"]
    am, bm = masks(pr["model"], LD)
    A, Bm, K, P, lam = (pr[k].astype(LD) for k in SWEEP_KEYS)
    cc, kf, pv, c0v = (pr[k][call].astype(LD) for k in RHS_KEYS)
    A, Bm = A * am, Bm * bm
    Bn = A.shape[0]
    dz, dlam = np.zeros((Bn, G, nx + nu), LD), np.zeros((Bn, G, nx), LD)
    dx = c0v[:, 0]
    for k in range(N + 1):
        if k == 1:
            dx = cc[:, 0] + mv(Bm[:, 0], kf[:, 0])
        elif k > 1:
            j = k - 1
            dx = mv(A[:, j] + Bm[:, j] @ K[:, j], dx) + cc[:, j] + mv(Bm[:, j], kf[:, j])
        dz[:, k, :nx] = dx
        if k < N:
            dz[:, k, nx:] = kf[:, k] + mv(K[:, k], dx)
        dlam[:, k] = mv(P[:, k], dx) + pv[:, k] - lam[:, k]
    return dz, dlam


def sweep_restated(pr, call=0, dtype=np.float64, seen=None):
    """forward_sweep's composition order, batched over instances and lanes, in `dtype` (float64, or object
    for Python integers).  Lane k starts with the map T_{k-1} (lane 0: the constant c0, lane 1: the
    constant part of T_0) and composes with its partner's partial map at each level: lane k - d inside
    the 16-lane row for d = 1, 2, 4, 8 (lanes with (kw & 15) >= d), the last lane of the previous row
    for d = 16 (rows 1 and 3 of the wave), lane 31 of the wave for d = 32 (rows 2 and 3); kw = the
    position in the wave's scanned span, GW = min(G, 64) lanes.  Wave w > 0 of a wider group then applies
    its maps to dx of the last lane of wave w - 1, in order.  `seen(array)`: called with every intermediate."""
    N, G, nx, nu = pr["N"], pr["G"], pr["nx"], pr["nu"]
    see = seen if seen is not None else (lambda a: None)
    conv = (lambda a: np.vectorize(lambda v: int(v), otypes=[object])(a)) if dtype is object else (lambda a: a.astype(dtype))
    am, bm = (conv(m) for m in masks(pr["model"]))
    A, Bm, K, P, lam = (conv(pr[k]) for k in SWEEP_KEYS)
    cc, kf, pv, c0v = (conv(pr[k][call]) for k in RHS_KEYS)
    A, Bm = A * am, Bm * bm
    Bn = A.shape[0]
    Acl, ccl = A + Bm @ K, cc + mv(Bm, kf)
    see(Acl), see(ccl)
    zero = conv(np.zeros(1))[0]
    Am = np.full((Bn, G, nx, nx), zero, dtype=Acl.dtype)
    cm = np.full((Bn, G, nx), zero, dtype=Acl.dtype)
    Am[:, 2:], cm[:, 1:], cm[:, 0] = Acl[:, 1:G - 1], ccl[:, :G - 1], c0v[:, 0]
    GW = min(G, 64)
    k = np.arange(G)
    kw = k & (GW - 1)
    for d in (1, 2, 4, 8, 16, 32):
        if d >= GW:
            break
        if d <= 8:
            src, takes = k - d, (kw & 15) >= d
        elif d == 16:
            src, takes = (k & ~15) - 1, (kw & 16) != 0
        else:
            src, takes = (k & ~63) + 31, (kw & 32) != 0
        src = np.where(takes, src, 0)
        assert np.all(src >= 0) and np.all((src // GW == k // GW) | ~takes)  # the partner is a lane of the same span
        Ao, co = Am[:, src], cm[:, src]
        An, cn = Am @ Ao, mv(Am, co) + cm
        see(An[:, takes]), see(cn[:, takes])
        Am, cm = np.where(takes[None, :, None, None], An, Am), np.where(takes[None, :, None], cn, cm)
    for w in range(1, G // 64):
        lanes = slice(64 * w, 64 * w + 64)
        cm[:, lanes] = mv(Am[:, lanes], cm[:, 64 * w - 1][:, None, :]) + cm[:, lanes]
        see(cm[:, lanes])
    dz = np.full((Bn, G, nx + nu), zero, dtype=Acl.dtype)
    dz[..., :nx] = cm
    dz[:, :N, nx:] = (kf + mv(K, cm))[:, :N]
    dlam = mv(P, cm) + pv - lam
    see(dz), see(dlam)
    dz[:, N + 1:], dlam[:, N + 1:] = zero, zero
    return dz, dlam


def node_error(got, ref):
    """Worst error against the long-double reference, node by node, normalised by max(1, max |reference|)
    at the node: [B, G]."""
    with np.errstate(invalid="ignore"):
        e = np.abs(got.astype(LD) - ref).max(axis=-1) / np.maximum(1.0, np.abs(ref).max(axis=-1))
    return np.where(np.isnan(e), np.inf, e).astype(np.float64)


def sweep_error(got, ref):
    """max over dz and dlam of node_error, over all nodes and instances."""
    return float(max(node_error(g, r).max() for g, r in zip(got, ref)))


def signed_permutations(rng, shape, n):
    """Random signed permutation matrices [..., n, n] (integers as float64)."""
    perm = rng.permuted(np.broadcast_to(np.arange(n), shape + (n,)), axis=-1)
    sign = rng.choice([-1.0, 1.0], size=shape + (n,))
    out = np.zeros(shape + (n, n))
    np.put_along_axis(out, perm[..., None], sign[..., None], axis=-1)
    return out


def integer_jacobians(rng, model, shape):
    """Integer A inside the model's mask whose products stay small: a signed permutation of the states
    whose column is dense (the whole matrix for the dense models; one state of the unicycle: a unit
    entry), a unit diagonal on the others and integer shear entries from the dense columns into
    their rows.  Outside the mask: non-zero integers, which the device must not read."""
    m = MODELS[model]
    nx = m["nx"]
    am, _ = masks(model)
    dense = [j for j in range(nx) if am[:, j].all()]
    rest = [j for j in range(nx) if j not in dense]
    A = np.zeros(shape + (nx, nx))
    if len(dense) > 1:
        A[np.ix_(*[range(s) for s in shape], dense, dense)] = signed_permutations(rng, shape, len(dense))
    else:
        A[..., dense[0], dense[0]] = 1.0
    for j in rest:
        A[..., j, j] = 1.0
        A[..., j, dense] = rng.integers(-2, 3, size=shape + (len(dense),))
    assert np.all((A * (1.0 - am)) == 0.0)
    return A + rng.integers(1, 4, size=shape + (nx, nx)) * (1.0 - am)  # garbage where the device must not look


@functools.lru_cache(maxsize=None)
def exact_problem(model, G, N):
    """Small-integer operands: every product and sum of the sweep is exact whatever the association.  A
    from integer_jacobians; even instances have K = 0 beyond node 0, odd ones B = 0 beyond node 0, so
    A + B K = A (on the lanes beyond N too: their products are formed and must stay exact to be
    comparable); K_0, B_0, A_0 and, on the lanes beyond N, A and every right-hand side are non-zero;
    every lane of every instance holds different data; two sets of right-hand sides."""
    m = MODELS[model]
    nx, nu, B = m["nx"], m["nu"], batch_of(G)
    rng = np.random.default_rng(77000 + 1000 * m["id"] + 10 * G + N)
    ints = lambda *s: rng.integers(-3, 4, size=s).astype(np.float64)  # noqa: E731
    nonzero = lambda *s: (rng.integers(1, 4, size=s) * rng.choice([-1, 1], size=s)).astype(np.float64)  # noqa: E731
    _, bm = masks(model)
    A = integer_jacobians(rng, model, (B, G))
    A[:, 0] = nonzero(B, nx, nx)  # A_0: never used
    Bm, K = nonzero(B, G, nx, nu), nonzero(B, G, nu, nx)
    K[0::2, 1:] = 0.0
    Bm[1::2, 1:] = 0.0
    M = ints(B, G, nx, nx)
    P = M + np.swapaxes(M, -1, -2)
    pr = dict(model=model, G=G, N=N, B=B, nx=nx, nu=nu, A=A, Bm=Bm, K=K, P=P, lam=ints(B, G, nx),
              cc=nonzero(2, B, G, nx), kf=nonzero(2, B, G, nu), pv=ints(2, B, G, nx), c0v=nonzero(2, B, G, nx))
    return freeze(pr)


@functools.lru_cache(maxsize=None)
def rounded_problem(model, G, N, radius=None):
    """Random operands; A + B K of every node scaled to a spectral radius drawn from [0.9, 1.02]
    (`radius`: that one for every node).  A near the identity inside the mask, B and K O(0.2), P
    symmetric O(1), right-hand sides O(1) (defects O(0.1)); the lanes beyond N hold operands of the
    same kind."""
    m = MODELS[model]
    nx, nu, B = m["nx"], m["nu"], batch_of(G)
    rng = np.random.default_rng(55000 + 1000 * m["id"] + 10 * G + N + (3 if radius else 0))
    am, bm = masks(model)
    A = (np.eye(nx) + 0.2 * rng.normal(size=(B, G, nx, nx)) * (1.0 - np.eye(nx))
         + 0.1 * rng.normal(size=(B, G, nx, nx)) * np.eye(nx)) * am
    Bm, K = 0.2 * rng.normal(size=(B, G, nx, nu)) * bm, 0.3 * rng.normal(size=(B, G, nu, nx))
    rho = np.abs(np.linalg.eigvals(A + Bm @ K)).max(axis=-1)
    t = rng.uniform(0.9, 1.02, size=(B, G)) if radius is None else np.full((B, G), radius)
    A, Bm = A * (t / rho)[..., None, None], Bm * (t / rho)[..., None, None]
    assert np.allclose(np.abs(np.linalg.eigvals(A + Bm @ K)).max(axis=-1), t, rtol=1e-9)
    M = rng.normal(size=(B, G, nx, nx))
    P = 0.5 * (M + np.swapaxes(M, -1, -2))
    pr = dict(model=model, G=G, N=N, B=B, nx=nx, nu=nu, A=A, Bm=Bm, K=K, P=P, lam=rng.normal(size=(B, G, nx)),
              cc=0.1 * rng.normal(size=(2, B, G, nx)), kf=rng.normal(size=(2, B, G, nu)),
              pv=rng.normal(size=(2, B, G, nx)), c0v=rng.normal(size=(2, B, G, nx)))
    return freeze(pr)


def freeze(pr):
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def rounded_case(model, G, N, radius=None):
    """(problem, long-double reference of both calls, the float64 restatement's worst error against it);
    computed once per session, shared, never modified."""
    pr = rounded_problem(model, G, N, radius)
    refs = [sweep_reference(pr, c) for c in (0, 1)]
    err = max(sweep_error(sweep_restated(pr, c), refs[c]) for c in (0, 1))
    return pr, refs, err


@functools.lru_cache(maxsize=None)
def sweep_tolerance():
    """(64 times the restatement's worst error over all the rounded cases, that worst error, its case)."""
    errs = {c: rounded_case(*c)[2] for c in CASES}
    errs[HOT_CASE + (1.1,)] = rounded_case(*HOT_CASE, 1.1)[2]
    worst = max(errs, key=errs.get)
    return 64.0 * errs[worst], errs[worst], worst


# ------------------------------------------------------------------------------------ the step lengths
def steps_reference(st, dz=None, dzL=None, dzU=None):
    """Bound-dual steps and step lengths in long double from the operands st (z, lb, ub, hL, hU, zL, zU,
    gp, dz [B, G, nz]; mu, tau, N): dict of dzL, dzU [B, G, nz], amax, az, gd [B] and tiny [B] (bool).
    dzL / dzU given: az from those instead (the device takes az from its own rounded dzL, dzU).

      dzL = mu / (z - lb) - zL - zL dz / (z - lb),  dzU = mu / (ub - z) - zU + zU dz / (ub - z),
      amax = min(1, min_{dz_i < 0, lower} -tau (z_i - lb_i) / dz_i, min_{dz_i > 0, upper} tau (ub_i - z_i) / dz_i),
      az = min(1, min_{dzL_i < 0} -tau zL_i / dzL_i, min_{dzU_i < 0} -tau zU_i / dzU_i),
      gd = sum gp_i dz_i and tiny = max |dz_i| / (1 + |z_i|) < 10 eps over the owned entries (x of the
      lanes k <= N, u of the lanes k < N)."""
    N, nx = st["N"], st["nx"]
    z, lb, ub, zL, zU, gp = (st[k].astype(LD) for k in ("z", "lb", "ub", "zL", "zU", "gp"))
    dz = (st["dz"] if dz is None else dz).astype(LD)
    hL, hU = st["hL"].astype(bool), st["hU"].astype(bool)
    mu, tau = LD(st["mu"]), LD(st["tau"])
    one, inf = LD(1), LD(np.inf)
    with np.errstate(all="ignore"):
        sL, sU = np.where(hL, z - lb, one), np.where(hU, ub - z, one)
        rL = np.where(hL, mu / sL - zL - zL * dz / sL, 0)
        rU = np.where(hU, mu / sU - zU + zU * dz / sU, 0)
        amax = np.minimum(np.where(hL & (dz < 0), -tau * sL / dz, inf).min(axis=(1, 2)),
                          np.where(hU & (dz > 0), tau * sU / dz, inf).min(axis=(1, 2)))
        dL, dU = (rL if dzL is None else dzL.astype(LD)), (rU if dzU is None else dzU.astype(LD))
        az = np.minimum(np.where(hL & (dL < 0), -tau * zL / dL, inf).min(axis=(1, 2)),
                        np.where(hU & (dU < 0), -tau * zU / dU, inf).min(axis=(1, 2)))
        own = owned(st)
        terms = np.where(own, gp * dz, 0)
        ratio = np.where(own, np.abs(dz) / (1 + np.abs(z)), 0)
    return dict(dzL=rL, dzU=rU, amax=np.minimum(one, amax), az=np.minimum(one, az), gd=terms.sum(axis=(1, 2)),
                gd_abs=np.abs(terms).sum(axis=(1, 2)), tiny=ratio.max(axis=(1, 2)) < 10 * LD(EPS),
                mag_L=np.where(hL, np.abs(mu / sL) + np.abs(zL) + np.abs(zL * dz / sL), 0),
                mag_U=np.where(hU, np.abs(mu / sU) + np.abs(zU) + np.abs(zU * dz / sU), 0))


def owned(st):
    """[B, G, nz]: the entries the lanes own (x_k for k <= N, u_k for k < N)."""
    B, G, nz = st["z"].shape
    k = np.arange(G)[None, :, None]
    return np.broadcast_to(np.where(np.arange(nz)[None, None, :] < st["nx"], k <= st["N"], k < st["N"]), (B, G, nz))


def slack_shortfall(st, alpha, dz=None):
    """The fraction-to-boundary rule by brute force, in long double: over the bounded components with a
    finite step, the worst of ((1 - tau) s_i - s_i(alpha)) / (tau s_i) with s_i the slack and s_i(alpha)
    the slack of z + alpha dz, per instance [B]: <= 0 iff alpha keeps every slack at (1 - tau) of its value."""
    z, lb, ub = (st[k].astype(LD) for k in ("z", "lb", "ub"))
    dz = (st["dz"] if dz is None else dz).astype(LD)
    hL, hU = st["hL"].astype(bool), st["hU"].astype(bool)
    tau, a = LD(st["tau"]), np.asarray(alpha, LD)[:, None, None]
    with np.errstate(all="ignore"):
        fin = np.isfinite(dz)
        zn = z + a * np.where(fin, dz, 0)
        sL, sU = np.where(hL, z - lb, 1), np.where(hU, ub - z, 1)
        wL = np.where(hL & fin, ((1 - tau) * sL - (zn - lb)) / (tau * sL), -np.inf)
        wU = np.where(hU & fin, ((1 - tau) * sU - (ub - zn)) / (tau * sU), -np.inf)
    return np.maximum(wL.max(axis=(1, 2)), wU.max(axis=(1, 2)))


def binding_lanes(G, N):
    """Where the step-length cases place the component that binds amax, by instance (cyclic): lane 0,
    lane N (a state-only node), the last lane of a 16-lane row, a lane of wave 1 or later (of the upper
    half of the nodes when the group has one wave), and none (the true amax is exactly 1)."""
    row_end = min(15, N) if N < 31 else (31 if N < 47 else 47)
    later = (64 + N) // 2 if N >= 64 else (N + 1) // 2 + N // 4
    return [0, N, row_end, min(later, N), None]


@functools.lru_cache(maxsize=None)
def steps_problem(model, G, N):
    """Random interior iterates: per entry no bound, a lower, an upper or both (only on owned entries, as
    the kernel sets the flags; the others hold infinite bounds), slacks in [0.05, 2], bound multipliers
    in [0.01, 2], a step scaled so that every component's limit is at least 2, then the component of
    binding_lanes given a step whose limit is amax = 0.1 ... 0.9 (odd instances against a lower bound,
    even ones against an upper bound)."""
    m = MODELS[model]
    nx, nu, B = m["nx"], m["nu"], batch_of(G)
    nz = nx + nu
    rng = np.random.default_rng(33000 + 1000 * m["id"] + 10 * G + N)
    mu, tau = 0.05, 0.95
    st = dict(model=model, G=G, N=N, B=B, nx=nx, nu=nu, mu=mu, tau=tau)
    own = owned(dict(z=np.zeros((B, G, nz)), nx=nx, N=N))
    kind = rng.integers(0, 4, size=(B, G, nz))  # 0 none, 1 lower, 2 upper, 3 both
    hL, hU = own & ((kind & 1) != 0), own & ((kind & 2) != 0)
    z = rng.normal(size=(B, G, nz))
    lb = np.where(hL, z - rng.uniform(0.05, 2.0, size=z.shape), -np.inf)
    ub = np.where(hU, z + rng.uniform(0.05, 2.0, size=z.shape), np.inf)
    dz = rng.normal(size=z.shape)
    with np.errstate(all="ignore"):
        lim = np.minimum(np.where(hL & (dz < 0), tau * (z - lb) / -dz, np.inf),
                         np.where(hU & (dz > 0), tau * (ub - z) / dz, np.inf))
    dz = dz * np.minimum(1.0, lim / rng.uniform(2.0, 4.0, size=z.shape))  # every limit >= 2
    where = binding_lanes(G, N)
    for i in range(B):
        lane = where[i % len(where)]
        if lane is None:
            continue
        j = nx + i % nu if lane == 0 else i % nx  # lane 0: a control (x_0 is pinned by g_0); else a state
        frac = rng.uniform(0.1, 0.9)
        if i % 2:
            hL[i, lane, j], lb[i, lane, j] = True, z[i, lane, j] - 0.7
            dz[i, lane, j] = -tau * (z[i, lane, j] - lb[i, lane, j]) / frac
        else:
            hU[i, lane, j], ub[i, lane, j] = True, z[i, lane, j] + 0.4
            dz[i, lane, j] = tau * (ub[i, lane, j] - z[i, lane, j]) / frac
    st.update(z=z, lb=lb, ub=ub, hL=hL.astype(np.float64), hU=hU.astype(np.float64), dz=dz,
              zL=np.where(hL, rng.uniform(0.01, 2.0, size=z.shape), 0.0),
              zU=np.where(hU, rng.uniform(0.01, 2.0, size=z.shape), 0.0), gp=rng.normal(size=z.shape))
    return freeze(st)


# ------------------------------------------------------------------ the harness's records (forward_check.hip)
def pack_records(pr=None, st=None, shape=None):
    """Node records [B, G, n_in] of tests/hip/forward_check.hip from a sweep problem and / or step-length
    operands (zeros for the part that is not given; st["dz"] becomes the override of the first sweep's dz)."""
    src = pr if pr is not None else st
    B, G, nx, nu = src["B"], src["G"], src["nx"], src["nu"]
    nz = nx + nu
    parts = []
    if pr is not None:
        parts += [pr["A"].reshape(B, G, -1), pr["Bm"].reshape(B, G, -1), pr["K"].reshape(B, G, -1), sym_pack(pr["P"]),
                  pr["lam"]]
        for c in (0, 1):
            parts += [pr[k][c] for k in RHS_KEYS]
    else:
        parts.append(np.zeros((B, G, nx * nx + 2 * nx * nu + nx * (nx + 1) // 2 + nx + 2 * (3 * nx + nu))))
    if st is not None:
        parts += [st[k] for k in ("z", "lb", "ub", "hL", "hU", "zL", "zU", "gp", "dz")] + [np.ones((B, G, 1))]
    else:
        parts.append(np.zeros((B, G, 9 * nz + 1)))
    return np.ascontiguousarray(np.concatenate(parts, axis=-1))
