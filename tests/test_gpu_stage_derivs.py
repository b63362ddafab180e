"""GPU: the ODE models' stage derivatives (mpc-verde_amd/csrc/ode.h OdeModel<Dyn>::derivs: F, q,
A = dF/dx, B = dF/du, g = fs grad q and the packed Hessian of fs q + lam^T F) through the device
harness tests/hip/derivs_check.hip, against the long-double hyper-dual reference
tests/helpers/stage_derivs_ref.py (itself checked against the oracles and against mpmath in
tests/test_stage_derivs_cpu.py), entry by entry, on every path of ode.h: the cached passes
(TrigRecord / TrigReplay), the direct passes (TrigDirect: M past the cache, or no cache), the
6-state bicycle's adjoint path, both parameter layouts and a stage index k > 0.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stage_derivs_ref as sd  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SENTINEL = 1e30  # fills x0 and the stage rows before k: a wrong row index cannot pass
VP = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hip", "libderivs_check.so"))
    lib.derivs_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, VP, VP, VP, VP, VP,
                                 VP, ctypes.c_int, VP, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.derivs_check.restype = ctypes.c_int
    return lib


def _arr8(v):
    return (ctypes.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))


def _call(model_id, n, T, M, Q, R, par, Z, lam, P, fs, p_layout, k, use_cache, which, n_out, fill=0.0):
    """One launch of the harness; returns (return code, out (n, n_out))."""
    import torch

    dev = lambda a: torch.from_numpy(np.array(a, np.float64)).cuda()  # noqa: E731
    d_z, d_l, d_p = dev(Z), dev(lam), dev(P)
    out = torch.full((len(Z) * n_out,), fill, dtype=torch.float64, device="cuda")
    rc = _lib().derivs_check(model_id, n, T, M, 0, _arr8(Q), _arr8(R), _arr8(par), VP(d_z.data_ptr()), VP(d_l.data_ptr()),
                             VP(d_p.data_ptr()), P.shape[1], VP(out.data_ptr()), fs, p_layout, k, use_cache, which)
    return rc, out.cpu().numpy().reshape(len(Z), n_out)


def _params(model, p_layout, k):
    """P (n, pstride): x0 (never read by the stage evaluation), then the target (layout 0) or the stage rows 0..k."""
    nx, nu = sd.NXU[model]
    nz = nx + nu
    zr = sd.stage_rows(model, p_layout)
    n = len(zr)
    if p_layout == 0:
        P = np.full((n, 2 * nx), SENTINEL)
        P[:, nx:] = zr[:, :nx]
    else:
        P = np.full((n, nx + nz * (k + 1)), SENTINEL)
        P[:, nx + nz * k:] = zr
    return P


@functools.lru_cache(maxsize=None)
def _device(model, M, steer, fs, p_layout, k, use_cache, which):
    """The harness's blocks for one configuration (shared by the cases that compare runs)."""
    T, _, Q, R, par = sd.constants(model, steer)
    Z, lam, _ = sd.points(model)
    rc, out = _call(sd.MODEL_ID[model], len(Z), T, M, Q, R, par, Z, lam, _params(model, p_layout, k), fs, p_layout, k,
                    use_cache, which, sd.n_out(model))
    assert rc == 0, rc
    return sd.split_flat(model, out)


@pytest.mark.parametrize("case,fs,p_layout,k", [g[:4] for g in sd.grid()], ids=[g[4] for g in sd.grid()])
def test_stage_derivs_match_reference(case, fs, p_layout, k):
    """Every block of the device's stage derivatives at 256 seeded points of the model's domain
    (helpers/stage_derivs_ref.py points) agrees with the long-double reference within
    max(16 E64, 4 * 2^-52), relative to each point's largest entry of the block.  E64 is the case's
    yardstick: the reference's own algorithm in float64 against its long-double run
    (tests/test_stage_derivs_cpu.py prints the table).  16: the device differs from that float64
    run by fma contraction, summation order, the closed-form adjoint against forward passes and the
    device library's sincos / tan, each a small multiple of the same rounding, while a wrong or
    missing term shows at 1e-3 or more of the entry.

    E64 and the device's measured error, per path:
    (one MI355X; E64 / device, the worst over fs, layouts and k; the device's worst share of its
    bound is 0.16, the cart-pole's H)
    kin-M1-cached             xf 3.5e-16/2.5e-16 q 2.7e-16/2.7e-16 A 8.0e-17/8.0e-17 B 3.5e-16/3.6e-16 g 1.6e-16/1.6e-16 H 5.8e-16/5.8e-16
    kin-M3-direct             xf 3.5e-16/3.5e-16 q 2.7e-16/2.7e-16 A 7.1e-17/7.1e-17 B 3.5e-16/3.5e-16 g 1.6e-16/1.6e-16 H 5.1e-16/5.1e-16
    cart-M1-cached            xf 2.5e-16/1.8e-16 q 3.3e-16/2.8e-16 A 5.3e-16/5.3e-16 B 4.3e-16/4.3e-16 g 1.6e-16/1.6e-16 H 2.3e-15/5.1e-15
    cart-M2-direct            xf 1.9e-16/3.1e-16 q 3.3e-16/2.8e-16 A 6.2e-16/5.7e-16 B 4.9e-16/6.1e-16 g 1.6e-16/1.6e-16 H 2.6e-15/2.1e-15
    dyn-M4-adjoint            xf 3.5e-16/3.5e-16 q 4.1e-16/3.5e-16 A 6.0e-16/7.1e-16 B 3.3e-16/2.8e-16 g 1.6e-16/1.9e-16 H 1.4e-15/1.9e-15
    dyn-M4-passes-cached      xf 3.5e-16/3.5e-16 q 4.1e-16/3.5e-16 A 6.0e-16/8.2e-16 B 3.3e-16/2.5e-16 g 1.6e-16/1.9e-16 H 1.4e-15/2.0e-15
    dyn-M5-direct             xf 2.9e-16/2.9e-16 q 4.1e-16/3.5e-16 A 3.8e-16/3.8e-16 B 3.1e-16/2.8e-16 g 1.6e-16/1.9e-16 H 1.5e-15/3.0e-15
    dyn-M1-adjoint            xf 8.2e-15/3.7e-15 q 4.1e-16/3.5e-16 A 1.5e-14/6.7e-15 B 1.6e-14/7.1e-15 g 1.6e-16/1.9e-16 H 2.3e-14/1.1e-14
    path-M1-cached            xf 1.0e-16/1.0e-16 q 4.7e-16/4.7e-16 A 3.5e-16/3.5e-16 B 1.5e-16/1.5e-16 g 3.5e-16/3.4e-16 H 1.8e-15/1.2e-15
    path-M1-cached-as_written xf 1.0e-16/1.0e-16 q 4.7e-16/4.7e-16 A 2.9e-16/2.9e-16 B 1.6e-16/1.3e-16 g 3.5e-16/3.4e-16 H 8.2e-16/8.2e-16
    path-M2-direct            xf 2.0e-16/2.0e-16 q 4.7e-16/4.7e-16 A 3.3e-16/2.8e-16 B 1.7e-16/1.4e-16 g 3.5e-16/3.4e-16 H 1.3e-15/7.4e-16
    the four no-cache cases: the figures of kin-M1-cached, cart-M1-cached, dyn-M4-passes-cached and
    path-M1-cached (the same arithmetic on recomputed values).
    (dyn-M1: one RK4 substep of 0.05 s is outside the stability region at small vx, which E64 shows.)

    Exact: the columns of A of the states f does not read are unit vectors; H is exactly 0 where the
    reference is exactly 0; xf, q equal Model::value's (what the line search evaluates) bit for
    bit, with the cache on and off; g is bit-identical with the cache on and off.  (Before
    PathBicycle::cost_extra took explicit fmas, q of every path-frame case differed from value()'s
    in the last bit at 4 of the 256 points.)"""
    cid, model, M, use_cache, which, steer = case
    nx, nu = sd.NXU[model]
    ref = sd.reference(model, M, steer, fs, p_layout)
    E = sd.yardstick(model, M, steer, fs, p_layout)
    got = _device(model, M, steer, fs, p_layout, k, use_cache, which)
    assert all(np.isfinite(got[b]).all() for b in sd.BLOCKS)
    err = sd.block_errors(got, ref)
    tol = {b: max(16 * E[b], 4 * EPS) for b in sd.BLOCKS}
    print(f"\n{cid} fs={fs} layout={p_layout} k={k}: "
          + " ".join(f"{b} {err[b]:.1e} (E64 {E[b]:.1e}, {err[b] / tol[b]:.2f} of bound)" for b in sd.BLOCKS))
    for b in sd.BLOCKS:
        assert err[b] <= tol[b], (b, err[b], tol[b])
    # exact structure
    A = got["A"].reshape(-1, nx, nx)
    for j in sd.INDEP[model]:
        assert np.all(ref["A"][:, :, j] == np.eye(nx)[:, j])  # the reference finds the same, from the equations
        np.testing.assert_array_equal(A[:, :, j], np.broadcast_to(np.eye(nx)[:, j], (len(A), nx)))
    zero = ref["H"] == 0.0
    if sd.INDEP[model]:
        assert zero.all(axis=0).any()  # the pairs with a state f does not read, at least
    np.testing.assert_array_equal(got["H"][zero], 0.0)
    # the value the line search evaluates, and the cost gradient, whatever the cache
    for cache in (0, 1):
        val = _device(model, M, steer, fs, p_layout, k, cache, 2)
        np.testing.assert_array_equal(got["xf"], val["xf"], err_msg=f"xf against value(), cache {cache}")
        np.testing.assert_array_equal(got["q"], val["q"], err_msg=f"q against value(), cache {cache}")
    other = _device(model, M, steer, fs, p_layout, k, 1 - use_cache, which)
    np.testing.assert_array_equal(got["g"], other["g"], err_msg="g with the cache on against off")


@pytest.mark.parametrize("n,M,model_id,code", [(100, 1, 3, -3), (0, 1, 3, -3), (64, 0, 4, -3), (64, 1, 2, -4), (64, 1, 9, -4)])
def test_harness_rejects_bad_arguments(n, M, model_id, code):
    """n not a positive multiple of 64, M < 1 and an unknown model return the negative code and
    launch nothing: the output keeps its fill."""
    model = "kin_bicycle"
    T, _, Q, R, par = sd.constants(model)
    Z, lam, _ = sd.points(model)
    rc, out = _call(model_id, n, T, M, Q, R, par, Z, lam, _params(model, 0, 0), 1.0, 0, 0, 1, 0, 64, fill=-7.0)
    assert rc == code
    np.testing.assert_array_equal(out, -7.0)
