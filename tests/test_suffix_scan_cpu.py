"""CPU check of the reused decoupled suffix as a log-depth scan (mpc-verde_amd/csrc/backward.h
suffix_scan): on the reused suffix of LinearModel<5, 1> the recursion only carries the vector part,

    p_k = v_k + A^T p_{k+1},   v_k = gp_x + A^T (P_{k+1} c_k)  (kb <= k < N),   v_N = p_N,

and when every stage of the suffix uses one table the kernel sums it by a radix-4 Hillis-Steele suffix
scan, v_k += (A^T)^d v_{k+d} + (A^T)^{2d} v_{k+2d} + (A^T)^{3d} v_{k+3d} for d = 1, 4, 16, 64, with the
powers (A^T)^(j 4^l) formed by repeated products.  This restates the scan in numpy float64 (the level
order, the products that form the powers, one buffer per level read for all three partners, lanes
without a partner keeping their value) and holds it to the chain in long double by an a-priori
rounding bound; tests/test_gpu_scan.py imports the generators, the restatement and the bound, so the
device code is checked on the same inputs by the same rule.

The bound: the error of component i of p_k is at most C_BOUND * NX * (N - k + 1) * 2^-53 * S_k[i] with
S_k = sum_j |(A^T)^j| |v_{k+j}| (componentwise, long double).  C_BOUND is the smallest power of two at
which this restatement passes with 4x room over all the cases below: the restatement's worst ratio
error / (NX (N - k + 1) 2^-53 S_k) is 0.146 (G = 256, N = 200, kb = 193), so C_BOUND = 1 (0.5 leaves less
than 4x).  On one MI355X the device's worst ratio is 0.26 (the same case; tests/test_gpu_scan.py).
"""
import numpy as np
import pytest

LD = np.longdouble
NX, NU, NZ = 5, 1, 6
N_TAB = 3
U53 = 2.0 ** -53
C_BOUND = 1.0
# (G, N, kb): a suffix that starts just before, at and just after a wave boundary, a one-stage suffix,
# a suffix that is the whole horizon, G = 256
CASES = [(128, 100, 5), (128, 100, 63), (128, 100, 64), (128, 100, 65), (128, 100, 99), (128, 64, 60), (128, 127, 0),
         (256, 255, 120), (256, 255, 128), (256, 200, 191), (256, 200, 192), (256, 200, 193)]


def suffix_problem(G, N, kb, B=4, suffix_tab=1, split=False):
    """Random operands of B instances of LinearModel<5, 1> with a decoupled suffix from stage kb: per
    instance three tables of A scaled to spectral radius 0.9, 1.0, 1.02 (instance b: the (b mod 3)-th),
    a schedule that is random below kb and `suffix_tab` from kb on (`split`: the upper half of the
    suffix on the next table), stage Hessians M M^T / nz + 0.1 I, Sigma in [0, 1], gradients O(1),
    defects O(1e-2); on the suffix B = 0 and the stage Hessian has no x-u block."""
    rng = np.random.default_rng(100000 * G + 100 * N + kb)
    A = rng.normal(size=(B, N_TAB, NX, NX))
    rho = np.array([0.9, 1.0, 1.02])[np.arange(B) % 3]
    A *= (rho[:, None] / np.abs(np.linalg.eigvals(A)).max(axis=-1))[..., None, None]
    tab = rng.integers(0, N_TAB, size=(B, G)).astype(np.int32)
    tab[:, kb:] = suffix_tab
    if split:
        tab[:, kb + (N - kb + 1) // 2:] = (suffix_tab + 1) % N_TAB
    tab[:, N:] = 0
    M = rng.normal(size=(B, G, NZ, NZ))
    H = M @ np.swapaxes(M, -1, -2) / NZ + 0.1 * np.eye(NZ)
    H[:, kb:, :NX, NX:] = 0.0
    H[:, kb:, NX:, :NX] = 0.0
    Bm = rng.normal(size=(B, G, NX, NU))
    Bm[:, kb:] = 0.0
    return dict(G=G, N=N, kb=kb, B=B, A=A, tab=tab, H=H, sig=rng.uniform(0.0, 1.0, size=(B, G, NZ)),
                g=rng.normal(size=(B, G, NZ)), Bm=Bm, c=1e-2 * rng.normal(size=(B, G, NX)))


def stage_operands(pr, dtype=np.float64):
    """(Hd, A, B, c, g) per node with Hd = H + diag(Sigma) and A expanded through the schedule."""
    Hd = pr["H"].astype(dtype) + pr["sig"].astype(dtype)[..., None] * np.eye(NZ, dtype=dtype)
    A = np.take_along_axis(pr["A"], pr["tab"][:, :, None, None].astype(np.int64), axis=1).astype(dtype)
    return Hd, A, pr["Bm"].astype(dtype), pr["c"].astype(dtype), pr["g"].astype(dtype)


def inv_small(M):
    """Explicit inverse of a batch of 1 x 1 or 2 x 2 matrices (no pivoting, no LAPACK: any dtype)."""
    if M.shape[-1] == 1:
        return 1 / M
    a, b, c, d = M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1]
    det = a * d - b * c
    return np.stack([np.stack([d, -b], -1), np.stack([-c, a], -1)], -2) / det[..., None, None]


def riccati(Hd, A, Bm, c, g, N, PN, pN):
    """The sequential recursion (riccati.h riccati_step, node N-1 .. 0), batched over the leading
    dimension, in the dtype of its operands: P [B, N+1, nx, nx], p [B, N+1, nx], K = -Huu'^-1 Hux'
    [B, N, nu, nx], kf = -Huu'^-1 gu' [B, N, nu], and the smallest pivot of Huu' per stage."""
    nx = A.shape[-1]
    T = lambda X: np.swapaxes(X, -1, -2)  # noqa: E731
    P, p = [None] * N + [PN], [None] * N + [pN]
    K, kf, piv = [None] * N, [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Ak, Bk, Pn = A[:, k], Bm[:, k], P[k + 1]
        Hxx = Hd[:, k, :nx, :nx] + T(Ak) @ Pn @ Ak
        Hux = Hd[:, k, nx:, :nx] + T(Bk) @ Pn @ Ak
        Huu = Hd[:, k, nx:, nx:] + T(Bk) @ Pn @ Bk
        s = p[k + 1] + (Pn @ c[:, k, :, None])[..., 0]
        gx = g[:, k, :nx] + (T(Ak) @ s[..., None])[..., 0]
        gu = g[:, k, nx:] + (T(Bk) @ s[..., None])[..., 0]
        Ri = inv_small(Huu)
        K[k] = -Ri @ Hux
        kf[k] = -(Ri @ gu[..., None])[..., 0]
        P[k] = Hxx + T(Hux) @ K[k]
        p[k] = gx + (T(Hux) @ kf[k][..., None])[..., 0]
        d0 = Huu[..., 0, 0]
        piv[k] = d0 if Huu.shape[-1] == 1 else np.minimum(d0, Huu[..., 1, 1] - Huu[..., 0, 1] ** 2 / d0)
    return np.stack(P, 1), np.stack(p, 1), np.stack(K, 1), np.stack(kf, 1), np.stack(piv, 1)


def terminal(pr, dtype=np.float64):
    """Node N's value function: P_N = diag(Sigma_x), p_N = the barrier gradient (delta = 0)."""
    N = pr["N"]
    return (pr["sig"][:, N, :NX, None] * np.eye(NX)).astype(dtype), pr["g"][:, N, :NX].astype(dtype)


def radix4_scan(AT, v, G, N, wrong_q2=False):
    """backward.h suffix_scan in float64: AT = A^T of the suffix's table, v [G, NX] the lanes' vectors
    (zeros outside the suffix and node N).  Returns the scanned vectors.  `wrong_q2`: a defect for the
    sensitivity test below, the q = 2 partner taken with the power of q = 1."""
    kLev = 4 if G <= 256 else 5
    M = [None] * (3 * kLev)
    M[0] = AT.copy()
    for l in range(kLev):  # mpow[(3 l + j - 1)] = (A^T)^(j 4^l)
        if l > 0:
            M[3 * l] = M[3 * l - 2] @ M[3 * l - 2]
        M[3 * l + 1] = M[3 * l] @ M[3 * l]
        M[3 * l + 2] = M[3 * l + 1] @ M[3 * l]
    v = v.copy()
    l, d = 0, 1
    while l < kLev and d <= N:
        cur = v.copy()  # every partner of the level is read from the previous level's buffer
        for q in (1, 2, 3):
            if q * d < G:  # lanes t + q d >= G have no partner: they keep v
                v[:G - q * d] += cur[q * d:] @ M[3 * l + (0 if wrong_q2 and q == 2 else q - 1)].T
        l, d = l + 1, d * 4
    return v


def suffix_vectors(pr, P, b, dtype):
    """v_k of instance b from the stored P (an array of float64 values, taken as data): [G, NX] in
    `dtype`, zeros below kb and above N, and A^T of the suffix's table."""
    G, N, kb = pr["G"], pr["N"], pr["kb"]
    AT = pr["A"][b, pr["tab"][b, kb]].T.astype(dtype)
    v = np.zeros((G, NX), dtype)
    v[N] = pr["g"][b, N, :NX].astype(dtype)
    for k in range(kb, N):
        v[k] = pr["g"][b, k, :NX].astype(dtype) + AT @ (P[k + 1].astype(dtype) @ pr["c"][b, k].astype(dtype))
    return AT, v


def suffix_bound_ratio(pr, P, p_got, b):
    """Worst error of p_got[k] (kb <= k <= N, instance b) against the long-double chain on the vectors
    formed from the stored P, in units of NX (N - k + 1) 2^-53 S_k (componentwise)."""
    N, kb = pr["N"], pr["kb"]
    AT, v = suffix_vectors(pr, P, b, LD)
    p = v.copy()
    for k in range(N - 1, kb - 1, -1):
        p[k] = v[k] + AT @ p[k + 1]
    L = N - kb
    pw = [np.eye(NX, dtype=LD)]
    for _ in range(L):
        pw.append(AT @ pw[-1])
    apw, av = np.abs(np.stack(pw)), np.abs(v)
    worst = 0.0
    for k in range(kb, N + 1):
        S = np.einsum("jim,jm->i", apw[:N - k + 1], av[k:N + 1])
        err = np.abs(p_got[k].astype(LD) - p[k])
        assert np.all(S > 0)
        worst = max(worst, float((err / (NX * (N - k + 1) * U53 * S)).max()))
    return worst


def restated_ratio(G, N, kb):
    """The float64 restatement on the case's operands: its worst ratio to the bound's unit, and its
    worst difference from the float64 chain relative to the largest |p_k|."""
    pr = suffix_problem(G, N, kb)
    Hd, A, Bm, c, g = stage_operands(pr)
    P, p, _, _, piv = riccati(Hd, A, Bm, c, g, N, *terminal(pr))
    assert np.all(piv > 0)
    worst, diff = 0.0, 0.0
    for b in range(pr["B"]):
        AT, v = suffix_vectors(pr, P[b], b, np.float64)
        got = radix4_scan(AT, v, G, N)
        worst = max(worst, suffix_bound_ratio(pr, P[b], got, b))
        diff = max(diff, np.abs(got[kb:N + 1] - p[b, kb:]).max() / max(1.0, np.abs(p[b, kb:]).max()))
        assert np.all(got[N + 1:] == 0.0)  # nothing beyond node N enters
    return worst, diff


@pytest.mark.parametrize("G,N,kb", CASES)
def test_radix4_suffix_scan_is_the_chain(G, N, kb):
    worst, diff = restated_ratio(G, N, kb)
    print(f"G={G} N={N} kb={kb}: restatement error {worst:.3f} of NX (N - k + 1) 2^-53 S_k, "
          f"{diff:.1e} from the float64 chain")
    assert diff <= 1e-12
    assert 4.0 * worst <= C_BOUND


def test_scan_of_a_wrong_power_misses_the_bound():
    """The bound is tight enough to see one wrong power: with (A^T)^(4^l) in place of (A^T)^(2 4^l)
    (the q = 2 partner of every level) the restatement misses it by orders of magnitude."""
    G, N, kb = 128, 100, 63
    pr = suffix_problem(G, N, kb)
    Hd, A, Bm, c, g = stage_operands(pr)
    P = riccati(Hd, A, Bm, c, g, N, *terminal(pr))[0]
    AT, v = suffix_vectors(pr, P[0], 0, np.float64)
    v = radix4_scan(AT, v, G, N, wrong_q2=True)
    assert suffix_bound_ratio(pr, P[0], v, 0) > 1e6 * C_BOUND
