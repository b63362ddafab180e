"""CPU: the host side of per-instance box bounds (mpcx_set_bounds_dev) -- the new entry point's
declaration and binding, the shape rules of ``Solver.solve_batch(lbw=, ubw=)`` (decided before any
library call) and the padded layout of 2-D bounds for linear models embedded by ``lti.StatePad``."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpcx.h")
LIB = os.path.join(ROOT, "mpc-verde_amd", "mpcx", "libmpcx.so")


def test_header_library_and_binding_name_the_setter():
    """include/mpcx.h declares mpcx_set_bounds_dev with six arguments, libmpcx.so exports it and
    the ctypes prototype has as many arguments as the declaration."""
    import mpcx

    src = open(HDR).read()
    m = re.search(r"^int\s+mpcx_set_bounds_dev\s*\(([^)]*)\)\s*;", src, re.M | re.S)
    assert m, "mpcx_set_bounds_dev not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6 and args[0].startswith("mpcx_handle*") and args[-1].startswith("void*"), args
    assert "mpcx_set_bounds_dev" in mpcx._lib.EXPORTS
    lib = mpcx._lib.load()
    assert len(lib.mpcx_set_bounds_dev.argtypes) == len(args)
    assert hasattr(mpcx._lib.Handle, "set_bounds_dev")


def _stub_solver(n_w, n_p, monkeypatch):
    """A Solver without a handle: solve_batch must raise on the arguments alone."""
    import mpcx
    from mpcx.nlpsol import Solver

    def no_library(*a, **k):
        raise AssertionError("the library was reached before the shape check")

    monkeypatch.setattr(mpcx._lib, "load", no_library)
    s = object.__new__(Solver)
    s.ocp = types.SimpleNamespace(formulation="multiple_shooting")
    s._h = types.SimpleNamespace(n_w=n_w, n_g=0, n_p=n_p)
    s._pad = None
    s._dev_bounds = None
    return s


@pytest.mark.parametrize("shape", [(4, 53), (5, 52), (5, 54), (2, 5, 53), (53, 5)])
def test_solve_batch_refuses_wrong_bound_shapes_before_the_library(monkeypatch, shape):
    s = _stub_solver(53, 6, monkeypatch)
    P = np.zeros((5, 6))
    good = np.zeros((5, 53))
    with pytest.raises(ValueError, match="lbw"):
        s.solve_batch(P, lbw=np.zeros(shape), ubw=good + 1)
    with pytest.raises(ValueError, match="ubw"):
        s.solve_batch(P, lbw=good, ubw=np.ones(shape))


def test_solve_batch_bound_argument_forms(monkeypatch):
    from mpcx.nlpsol import _batch_bounds

    B, nw = 3, 8
    # the shared forms stay what they were: None, scalar, n_w entries (row or column)
    lb, ub, per = _batch_bounds(None, 2.0, B, nw)
    assert lb is None and not per and ub.shape == (nw,) and np.all(ub == 2.0)
    lb, ub, per = _batch_bounds(np.arange(nw)[:, None], np.arange(nw)[None, :] + 1.0, B, nw)
    assert not per and lb.shape == ub.shape == (nw,)
    with pytest.raises(ValueError, match="expected 8 entries"):
        _batch_bounds(np.zeros(7), None, B, nw)
    # one row per instance; a scalar or vector counterpart is repeated
    L = -np.arange(1.0, B * nw + 1).reshape(B, nw)
    lb, ub, per = _batch_bounds(L, 5.0, B, nw)
    assert per and lb.shape == ub.shape == (B, nw) and np.array_equal(lb, L) and np.all(ub == 5.0)
    assert lb.flags["C_CONTIGUOUS"] and ub.flags["C_CONTIGUOUS"] and lb.dtype == ub.dtype == np.float64
    with pytest.raises(ValueError, match="both lbw and ubw"):
        _batch_bounds(L, None, B, nw)
    # infinities become +-1e20, NaN is left for the library to refuse
    U = np.full((B, nw), np.inf)
    U[1, 2] = np.nan
    U[2, 3] = 3e19
    L2 = L.copy()
    L2[0, 0] = -np.inf
    lb, ub, per = _batch_bounds(L2, U, B, nw)
    assert lb[0, 0] == -1e20 and ub[0, 0] == 1e20 and ub[2, 3] == 1e20 and np.isnan(ub[1, 2])


def test_state_pad_scatters_2d_bounds():
    """A (2, 1) double integrator embedded in the 4-state kernel: user rows land on the model's
    entries of the padded layout, the pad states get -+1e20 -- the values the 1-D path gives."""
    from mpcx import lti

    N, B = 4, 3
    A = np.array([[1.0, 0.1], [0.0, 1.0]])
    Bm = np.array([[0.005], [0.1]])
    lin = lti.LinearOCP(N=N, A=A[None], B=Bm[None], W=np.diag([1.0, 0.1, 0.01])[None], tab=np.zeros(N, np.int32),
                        u_lb=(-1.0,), u_ub=(1.0,))
    pd = lti.state_pad(lin)
    assert pd is not None and (pd.n_w, pd.n_w_pad) == (2 + 3 * N, 4 + 5 * N)
    rng = np.random.default_rng(0)
    lb = -rng.uniform(1, 2, (B, pd.n_w))
    ub = rng.uniform(1, 2, (B, pd.n_w))
    lbp, ubp = pd.scatter(lb, pd.w_idx, pd.n_w_pad, -1e20), pd.scatter(ub, pd.w_idx, pd.n_w_pad, 1e20)
    assert lbp.shape == ubp.shape == (B, pd.n_w_pad)
    assert np.array_equal(lbp[:, pd.w_idx], lb) and np.array_equal(ubp[:, pd.w_idx], ub)
    pad = np.setdiff1d(np.arange(pd.n_w_pad), pd.w_idx)
    assert pad.size == 2 * (N + 1)
    assert np.all(lbp[:, pad] == -1e20) and np.all(ubp[:, pad] == 1e20)
    for b in range(B):  # row by row the 1-D path's result
        assert np.array_equal(lbp[b], pd.scatter(lb[b][None, :], pd.w_idx, pd.n_w_pad, -1e20)[0])
        assert np.array_equal(ubp[b], pd.scatter(ub[b][None, :], pd.w_idx, pd.n_w_pad, 1e20)[0])
