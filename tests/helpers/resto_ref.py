"""References for the small dense algebra of the restoration phase (mpc-verde_amd/csrc/resto.h:
chol_small, chol_solve_small, resto_chol, resto_transform).

* ``exact``: the DEFINITIONS  S = D^-1 + P,  Pt = D^-1 - D^-1 S^-1 D^-1,  pt = D^-1 S^-1 p, and
  x = fl(S)^-1 p (chol_small / chol_solve_small on their own: the float64 S is their input) in
  exact rational arithmetic (fractions.Fraction on the float64 inputs, Gaussian elimination,
  n <= 6), each entry rounded once to float64.  Long double is not enough here: on the
  class "D^-1 huge" the form of Pt cancels 6 to 10 digits.
* ``restated``: the device algorithm in float64 -- the same loops, plain numpy, batched over the
  cases (no fma, IEEE division where the device takes 1 / l once).
* ``draw`` / ``edge_cases``: the case classes of tests/test_resto_cpu.py and
  tests/test_gpu_resto_algebra.py, at fixed seeds.
* ``a_priori``: the forward-error bound of a Cholesky solve that test_resto_cpu holds the
  restatement to.
"""
import functools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
NXS = (3, 4, 6)  # the state dimensions of the models that declare kResto
# class -> (log10 range of D, log10 range of the eigenvalues of P)
CLASSES = {"p_huge": ((-6, 2), (4, 12)), "balanced": ((-2, 2), (-2, 2)), "dinv_huge": ((-9, -5), (-2, 2))}
N_DRAWS = 300


def symix(i, j, n):
    if i > j:
        i, j = j, i
    return i * n - i * (i - 1) // 2 + (j - i)


def pack(P):
    """(..., n, n) symmetric -> (..., n (n + 1) / 2), the device's packed order (riccati.h symix)."""
    n = P.shape[-1]
    return np.stack([P[..., i, j] for i in range(n) for j in range(i, n)], axis=-1)


def unpack(Pp, n):
    out = np.zeros(Pp.shape[:-1] + (n, n), Pp.dtype)
    for i in range(n):
        for j in range(n):
            out[..., i, j] = Pp[..., symix(i, j, n)]
    return out


# --------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------
def draw(cls, nx, count=N_DRAWS):
    """D (count, nx) log-uniform, P = Q diag(ev) Q^T (count, nx, nx; exactly symmetric) with
    log-uniform ev and Q from the QR factorisation of a Gaussian matrix, p (count, nx) standard
    normal."""
    (d0, d1), (e0, e1) = CLASSES[cls]
    rng = np.random.default_rng(7000 + 100 * list(CLASSES).index(cls) + nx)
    D = 10.0 ** rng.uniform(d0, d1, (count, nx))
    ev = 10.0 ** rng.uniform(e0, e1, (count, nx))
    Q = np.linalg.qr(rng.normal(size=(count, nx, nx)))[0]
    P = Q @ (ev[..., None] * np.swapaxes(Q, -1, -2))
    P = unpack(pack(P), nx)  # the upper triangle, mirrored
    return D, P, rng.normal(size=(count, nx))


def edge_cases(nx):
    """Regular edges (S positive definite; compared with the exact reference as a class "edges"):
    P = 0 off the diagonal (the terminal node's value function: Sigma_x + delta) and P exactly
    singular (v v^T with an integer v, rank 1), D in 1e-2..1e2."""
    rng = np.random.default_rng(7900 + nx)
    m = 12
    D = 10.0 ** rng.uniform(-2, 2, (2 * m, nx))
    P = np.zeros((2 * m, nx, nx))
    P[:m] = (10.0 ** rng.uniform(-6, 6, (m, nx)))[..., None] * np.eye(nx)
    v = rng.integers(-3, 4, (m, nx)).astype(float)
    v[:, 0] = 1.0
    P[m:] = v[:, :, None] * v[:, None, :]
    return D, P, rng.normal(size=(2 * m, nx))


def broken_cases(nx):
    """Cases where ok must be false.  Built from small integers and powers of two so that every
    operation of the device's Cholesky is exact, fma or not: S = L0 L0^T with L0 lower triangular,
    integer, unit-or-larger diagonal except L0[n-1, n-1] = 0, so the nx-th pivot is exactly 0;
    the same with 2^-40 taken from S[n-1, n-1], so it is exactly -2^-40; and a NaN in P (at the
    first, a middle and the last packed entry).  D = 1/2 or 1/4 (D^-1 exact), P = S - D^-1.
    Returns D, P, p and kind (0: pivot 0, 1: pivot negative, 2: NaN)."""
    rng = np.random.default_rng(7950 + nx)
    m = 8
    Ds, Ps, kinds = [], [], []
    for kind in (0, 1, 2):
        for c in range(m):
            L0 = np.tril(rng.integers(-1, 3, (nx, nx))).astype(float)
            L0[np.arange(nx), np.arange(nx)] = rng.integers(1, 3, nx)
            if kind < 2:
                L0[nx - 1, nx - 1] = 0.0
            S = L0 @ L0.T
            if kind == 1:
                S[nx - 1, nx - 1] -= 2.0 ** -40
            D = rng.choice([0.5, 0.25], nx)
            P = S - np.diag(1.0 / D)
            if kind == 2:
                i, j = [(0, 0), (0, nx - 1), (nx - 1, nx - 1), (1, 2)][c % 4]
                P[i, j] = P[j, i] = np.nan
            Ds.append(D)
            Ps.append(P)
            kinds.append(kind)
    return np.array(Ds), np.array(Ps), rng.integers(-2, 3, (3 * m, nx)).astype(float), np.array(kinds)


# --------------------------------------------------------------------------------------------
# the definitions, exactly
# --------------------------------------------------------------------------------------------
def _solve_exact(S, R):
    """S^-1 R for lists of lists of Fractions (Gaussian elimination, first non-zero pivot)."""
    n, m = len(S), len(R[0])
    M = [list(S[i]) + list(R[i]) for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [[M[i][n + j] for j in range(m)] for i in range(n)]


def exact_one(D, P, p):
    """One case: float64 D (n), P (n, n), p (n) -> dict of float64 arrays S, Di, Pt, pt, X = S^-1
    D^-1 and x = Sf^-1 p (Sf: S as resto_chol forms it in float64), each entry the exact rational
    value rounded once."""
    n = len(D)
    Di = [1 / Fraction(float(d)) for d in D]
    Pf = [[Fraction(float(P[i][j])) for j in range(n)] for i in range(n)]
    S = [[Pf[i][j] + (Di[i] if i == j else 0) for j in range(n)] for i in range(n)]
    R = [[(Di[i] if i == j else Fraction(0)) for j in range(n)] + [Fraction(float(p[i]))] for i in range(n)]
    X = _solve_exact(S, R)  # S^-1 [D^-1 | p]
    Pt = [[(Di[i] if i == j else 0) - Di[i] * X[i][j] for j in range(n)] for i in range(n)]
    # chol_small / chol_solve_small on their own take the float64 S: its solve, exactly
    Sf = np.array(P, float) + np.diag(1.0 / np.asarray(D, float))
    xs = _solve_exact([[Fraction(float(v)) for v in r] for r in Sf], [[Fraction(float(v))] for v in p])
    f = lambda rows: np.array([[float(v) for v in r] for r in rows])  # noqa: E731
    return dict(S=f(S), Di=np.array([float(v) for v in Di]), Pt=f(Pt),
                pt=np.array([float(Di[i] * X[i][n]) for i in range(n)]), x=np.array([float(r[0]) for r in xs]),
                X=f([r[:n] for r in X]), Sf=Sf)


def exact(D, P, p):
    """Batched exact_one: dict of stacked arrays."""
    rows = [exact_one(D[c], P[c], p[c]) for c in range(len(D))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# --------------------------------------------------------------------------------------------
# the device algorithm in float64
# --------------------------------------------------------------------------------------------
def chol_small(S):
    """resto.h chol_small, batched: L (cases, n, n) and ok (cases).  A non-positive or NaN pivot
    clears ok and the factorisation goes on with sqrt(max(d, 1e-300))."""
    n = S.shape[-1]
    L = np.zeros_like(S)
    ok = np.ones(S.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = S[:, j, j].copy()
            for q in range(j):
                d = d - L[:, j, q] * L[:, j, q]
            ok &= d > 0.0
            l = np.sqrt(np.fmax(d, 1e-300))
            rl = 1.0 / l
            L[:, j, j] = l
            for i in range(j + 1, n):
                t = S[:, i, j].copy()
                for q in range(j):
                    t = t - L[:, i, q] * L[:, j, q]
                L[:, i, j] = t * rl
    return L, ok


def chol_solve_small(L, b):
    n = L.shape[-1]
    b = b.copy()
    with np.errstate(all="ignore"):
        for i in range(n):
            t = b[:, i].copy()
            for q in range(i):
                t = t - L[:, i, q] * b[:, q]
            b[:, i] = t / L[:, i, i]
        for i in range(n - 1, -1, -1):
            t = b[:, i].copy()
            for q in range(i + 1, n):
                t = t - L[:, q, i] * b[:, q]
            b[:, i] = t / L[:, i, i]
    return b


def resto_chol(D, P):
    """resto.h resto_chol: Di, S, L, ok (P full symmetric; the device reads its upper triangle)."""
    n = D.shape[-1]
    with np.errstate(all="ignore"):
        Di = 1.0 / D
    S = P + Di[:, :, None] * np.eye(n)
    L, ok = chol_small(S)
    return Di, S, L, ok


def resto_transform(D, P, p):
    """resto.h resto_transform: Pt (cases, n, n), pt (cases, n), ok."""
    n = D.shape[-1]
    Di, _, L, ok = resto_chol(D, P)
    X = np.zeros((D.shape[0], n, n + 1))
    for c in range(n + 1):
        b = np.zeros_like(D)
        if c < n:
            b[:, c] = Di[:, c]
        else:
            b = p.copy()
        X[:, :, c] = chol_solve_small(L, b)
    Pt = np.zeros_like(P)
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(i, n):
                Pt[:, i, j] = (Di[:, i] if i == j else 0.0) - 0.5 * (Di[:, i] * X[:, i, j] + Di[:, j] * X[:, j, i])
                Pt[:, j, i] = Pt[:, i, j]
        pt = Di * X[:, :, n]
    return Pt, pt, ok


def naive_transform(P, S):
    """P - P S^-1 P in float64 (the form resto_transform's comment warns against)."""
    return P - P @ np.linalg.solve(S, P)


# --------------------------------------------------------------------------------------------
# errors
# --------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """Per case: max |got - ref| over the case's entries / max(1e-300, max |ref|); a non-finite
    entry counts as inf.  The difference is taken in long double."""
    ax = tuple(range(1, ref.ndim))
    with np.errstate(all="ignore"):
        e = np.abs(got.astype(np.longdouble) - ref.astype(np.longdouble)).max(axis=ax)
        e = e / np.maximum(1e-300, np.abs(ref).max(axis=ax))
    return np.where(np.isfinite(e), e, np.inf).astype(np.float64)


def llt_err(L, S):
    """L L^T (in long double) against S, as rel_err."""
    Lq = L.astype(np.longdouble)
    return rel_err(Lq @ np.swapaxes(Lq, -1, -2), S)


def errors(got, ex):
    """The compared quantities of one class: got = dict(L, x, Di, Pt, pt) from the device or the
    restatement, ex = exact(...).  Returns name -> per-case error."""
    return {"L L^T": llt_err(got["L"], ex["S"]), "chol L L^T": llt_err(got["L0"], ex["Sf"]),
            "x": rel_err(got["x"], ex["x"]), "Di": rel_err(got["Di"], ex["Di"]), "Pt": rel_err(got["Pt"], ex["Pt"]),
            "pt": rel_err(got["pt"], ex["pt"])}


def restated(D, P, p):
    Di, S, L, ok = resto_chol(D, P)
    Pt, pt, ok2 = resto_transform(D, P, p)
    return dict(L=L, L0=L, x=chol_solve_small(L, p), Di=Di, Pt=Pt, pt=pt, ok=ok & ok2, S=S)


def a_priori(ex):
    """Per case, bounds on the restatement's rel_err of x, Pt and pt from the error analysis of a
    Cholesky solve (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.4 and
    10.6 with van der Sluis' scaling): with H = Delta^-1 S Delta^-1, Delta = diag(sqrt(s_ii)), the
    computed solution of S x = b has ||Delta (x^ - x)||_2 <= e ||Delta x||_2, e = 2 n (3 n + 1) u
    kappa_2(H) (the factor 2 pays for 1 - n gamma kappa and for the rounded S = D^-1 + P).  Entry i
    is then off by at most e ||Delta x||_2 / Delta_i; the operations after the solve add their own
    roundings.  L L^T - S: |S - L L^T| <= gamma_(n+1) |L| |L^T| <= gamma_(n+1) max |S| (Thm 10.3)
    and two roundings in S, held here to n (n + 1) u."""
    S, Di, X, x = ex["S"], ex["Di"], ex["X"], ex["x"]
    n = S.shape[-1]
    dl = np.sqrt(np.einsum("cii->ci", S))
    H = S / (dl[:, :, None] * dl[:, None, :])
    e = 2.0 * n * (3 * n + 1) * EPS * np.linalg.cond(H)
    colnorm = lambda V: np.sqrt(np.sum((dl[:, :, None] * V) ** 2, axis=1))  # noqa: E731  (cases, columns)
    eX = e[:, None, None] * colnorm(X)[:, None, :] / dl[:, :, None]  # |X^ - X| entrywise
    ex_ = e[:, None] * colnorm(x[:, :, None])[:, 0, None] / dl
    ePt = 0.5 * (Di[:, :, None] * eX + Di[:, None, :] * np.swapaxes(eX, 1, 2))
    # the roundings after the solve: two products, their mean, the difference from D^-1
    ePt = ePt + 4.0 * EPS * (Di[:, :, None] * np.eye(n) + np.abs(Di[:, :, None] * X))
    nrm = lambda E, R: E.reshape(len(E), -1).max(axis=1) / np.maximum(1e-300, np.abs(R).reshape(len(R), -1).max(axis=1))  # noqa: E731
    return {"x": nrm(ex_, x), "Pt": nrm(ePt, ex["Pt"]), "pt": nrm(Di * ex_, ex["pt"]) + 2.0 * EPS,
            "L L^T": np.full(len(S), n * (n + 1) * EPS), "chol L L^T": np.full(len(S), n * (n + 1) * EPS)}


@functools.lru_cache(maxsize=None)
def class_case(cls, nx):
    """(D, P, p), exact reference, restatement and its per-quantity worst error of one class and
    dimension (cls in CLASSES or "edges"); computed once per process, shared, never modified."""
    D, P, p = edge_cases(nx) if cls == "edges" else draw(cls, nx)
    ex = exact(D, P, p)
    rs = restated(D, P, p)
    worst = {k: float(v.max()) for k, v in errors(rs, ex).items()}
    for a in (D, P, p, *ex.values(), *[v for v in rs.values()]):
        a.setflags(write=False)
    return (D, P, p), ex, rs, worst
