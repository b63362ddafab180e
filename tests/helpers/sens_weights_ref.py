"""NumPy references of the sensitivities of the MPC solution to the cost weights (the kernels csrc/sens.h
sens_wt_kernel and sens_wt_vjp_kernel).

The system is that of helpers/sens_p_ref.py,
    (H_k + Sigma_k) dz_k + [A_k B_k]^T lam_{k+1} - [lam_k; 0] + r_k = 0,   Sigma_x dX_N - lam_N = 0,
    A_k dX_k + B_k dU_k - dX_{k+1} = 0,   dX_0 = 0,
and only the stage cost q_k depends on the weights, linearly, so a direction of the weights gives
    r_k = d(grad_z q_k)/d(weights) . dwt_k:    diagonal weights   r_{k,i} = 2 dwt_{k,i} e_{k,i},
                                               packed table W     r_k = 2 dW_k e_k   (dW_k symmetric),
with e_k the residual z_k - zr_k of the cost.  The reverse mode: with z~ the adjoint solve of
helpers/sens_vjp_ref.py for a cotangent g, <g, dw> = sum_k z~_k^T r_k, so per stage
    diagonal  gwt_{k,i} = 2 z~_{k,i} e_{k,i};   packed  gW_k[a,a] = 2 z~_a e_a,  gW_k[a,b] = 2 (z~_a e_b + z~_b e_a).

(a) ``diag_rhs`` / ``packed_rhs``: the right-hand sides; ``diag_vjp`` / ``packed_vjp``: their transposes.
(b) ``weights_sens``: the recursion (sens_p_ref.affine_sens with d = 0, dx0 = 0), float64 or np.longdouble.
(c) ``refined_weights_sens`` / ``refined_adjoint_z``: one step of the kernel's refinement
    (sens_bounds_ref.refined_solve); ``reference`` / ``reference_z``: both rounds in long double.

Layouts as in sens_ref.py: e (N, nz); directions dwt (m, N, nz) or packed dWp (m, N, nz (nz + 1) / 2), the upper
triangle row by row (lti.pack_sym); r (N, nz, m); zt (N, nz, m); gradient rows (m, N, .); dw (n_w, m).
"""
import numpy as np
import sens_bounds_ref as sb
import sens_p_ref as sp
import sens_ref as sr
import sens_vjp_ref as sv


def unpack_sym(p, nz):
    """(..., nz (nz + 1) / 2) packed upper triangles -> (..., nz, nz) symmetric matrices"""
    p = np.asarray(p)
    iu = np.triu_indices(nz)
    W = np.zeros(p.shape[:-1] + (nz, nz), p.dtype)
    W[..., iu[0], iu[1]] = p
    W[..., iu[1], iu[0]] = p
    return W


def diag_rhs(dwt, e):
    """r (N, nz, m) of diagonal directions dwt (m, N, nz) at the residuals e (N, nz)"""
    return np.ascontiguousarray(np.transpose(2 * dwt * e[None], (1, 2, 0)))


def packed_rhs(dWp, e):
    """r (N, nz, m) of packed directions dWp (m, N, nh) at the residuals e (N, nz): r_k = 2 dW_k e_k"""
    dW = unpack_sym(dWp, e.shape[1])
    return np.ascontiguousarray(np.transpose(2 * np.einsum("ckij,kj->cki", dW, e), (1, 2, 0)))


def diag_vjp(zt, e):
    """gwt (m, N, nz) of the adjoint solution zt (N, nz, m): 2 z~ e"""
    return np.ascontiguousarray(np.transpose(2 * zt * e[:, :, None], (2, 0, 1)))


def packed_vjp(zt, e):
    """gW (m, N, nh): the packed entry [a, b], a < b, stands for W_ab and W_ba: 2 (z~_a e_b + z~_b e_a)"""
    nz = e.shape[1]
    iu = np.triu_indices(nz)
    za, zb = zt[:, iu[0], :], zt[:, iu[1], :]  # (N, nh, m)
    ea, eb = e[:, iu[0], None], e[:, iu[1], None]
    g = np.where((iu[0] == iu[1])[None, :, None], 2 * za * ea, 2 * (za * eb + zb * ea))
    return np.ascontiguousarray(np.transpose(g, (2, 0, 1)))


def _zeros(A, m, dtype):
    N, nx = A.shape[0], A.shape[1]
    return np.zeros((N, nx, m), dtype), np.zeros((nx, m), dtype)


def weights_sens(A, B, H, Sig, r, dtype=np.float64):
    """(dw (n_w, m), regular): recursion (b) in ``dtype``."""
    d, dx0 = _zeros(A, r.shape[2], dtype)
    return sp.affine_sens(A, B, H, Sig, np.asarray(r, dtype), d, dx0, dtype)


def _split(r, A):
    N, nx = A.shape[0], A.shape[1]
    return [r[k][:nx] for k in range(N)] + [np.zeros_like(r[0][:nx])], [r[k][nx:] for k in range(N)]


def refined_weights_sens(A, B, H, Sig, r, resid_dtype=np.longdouble, dtype=np.float64):
    """(dw before, dw after) the kernel's refinement round on the weight right-hand sides."""
    A, B, H, Sig, r = (np.asarray(v, dtype) for v in (A, B, H, Sig, r))
    nx, nu = A.shape[1], B.shape[2]
    rq, rr = _split(r, A)
    b, a, _ = sb.refined_solve(A, B, H, Sig, rq, rr, dtype, resid_dtype)
    return sp._pack(*b, nx, nu, dtype), sp._pack(*a, nx, nu, dtype)


def reference(A, B, H, Sig, r):
    """dw of the kernel's two rounds restated in long double (residuals in long double too)."""
    return refined_weights_sens(A, B, H, Sig, r, np.longdouble, np.longdouble)[1]


def adjoint_z(A, B, H, Sig, g, dtype=np.float64):
    """(zt (N, nz, m), regular): the adjoint solve of sens_vjp_ref in ``dtype``."""
    _, zt, _, regular = sv.adjoint_sens(A, B, H, Sig, g, dtype)
    return zt, regular


def refined_adjoint_z(A, B, H, Sig, g, resid_dtype=np.longdouble, dtype=np.float64):
    """zt (N, nz, m) after the kernel's refinement round on the adjoint solve."""
    A, B, H, Sig, g = (np.asarray(v, dtype) for v in (A, B, H, Sig, g))
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    rq, rr, _ = sv._rhs_of(g, nx, nu, N)
    _, (X, U), _ = sb.refined_solve(A, B, H, Sig, rq, rr, dtype, resid_dtype)
    return np.stack([np.concatenate([X[k], U[k]]) for k in range(N)])


def reference_z(A, B, H, Sig, g):
    """zt of the kernel's two rounds restated in long double."""
    return refined_adjoint_z(A, B, H, Sig, g, np.longdouble, np.longdouble)


# ---------------------------------------------------------------------------------------------------
# seeded problems
# ---------------------------------------------------------------------------------------------------
def random_residuals(nx, nu, N, seed):
    """Seeded normal residuals e (N, nz)."""
    return np.random.default_rng(seed + 7000).normal(size=(N, nx + nu))


def random_packed(nx, nu, N, seed, m=None):
    """Seeded normal packed directions (m, N, nh), one per stage, m default nx."""
    nz = nx + nu
    return np.random.default_rng(seed + 8000).normal(size=(nx if m is None else m, N, nz * (nz + 1) // 2))


_E_REF_W = []


def _e_ref_pair():
    if not _E_REF_W:
        fwd = rev = 0.0
        for s, (nx, nu, N) in enumerate(sr.LQ_SHAPES):
            A, B, H = sr.random_lq(nx, nu, N, s)
            e = random_residuals(nx, nu, N, s)
            dWp = random_packed(nx, nu, N, s)
            g = sv.random_cotangent(nx, nu, N, s)
            for sg in sr.LQ_SIGMAS:
                Sig = np.where(sr.random_input_mask(nx, nu, N, s), sg, 0.0)
                d64, ok = weights_sens(A, B, H, Sig, packed_rhs(dWp, e), np.float64)
                dld, _ = weights_sens(A, B, H, Sig, packed_rhs(np.asarray(dWp, np.longdouble), np.asarray(e, np.longdouble)),
                                      np.longdouble)
                assert ok
                fwd = max(fwd, sr.rel_err(d64, dld))
                z64, ok = adjoint_z(A, B, H, Sig, g, np.float64)
                zld, _ = adjoint_z(A, B, H, Sig, g, np.longdouble)
                assert ok
                rev = max(rev, sr.rel_err(packed_vjp(z64, e), packed_vjp(zld, np.asarray(e, np.longdouble))))
        _E_REF_W.extend([fwd, rev])
    return _E_REF_W


def e_ref_w():
    """The yardstick of the forward mode, computed as sens_bounds_ref.e_ref_b is: the worst relative error
    (sens_ref.rel_err) of the float64 recursion (b) against the long-double one over LQ_SHAPES x LQ_SIGMAS
    (Sigma on a random 40 % of the inputs) with the weight right-hand sides of nx seeded normal packed
    per-stage directions at seeded normal residuals; computed once."""
    return _e_ref_pair()[0]


def e_ref_wvjp():
    """The yardstick of the reverse mode: the same for the packed gradient rows of nx seeded normal cotangents."""
    return _e_ref_pair()[1]
