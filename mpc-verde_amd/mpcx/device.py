"""Device-resident batched receding-horizon loop (torch tensors as device memory).

PyTorch provides device allocations, streams and events only; all arithmetic is
in libmpcx's HIP kernels, reached through the ``*_dev`` C entry points.  One
closed-loop step for B instances = one fused solve launch + one shift/plant
launch (``Casadi/multiple_shooting_casadi.py:226-287``, batched), with no host
synchronisation in between.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .nlpsol import Solver


def _ptr(t):
    return None if t is None else ctypes_void(t.data_ptr())


def ctypes_void(p):
    import ctypes

    return ctypes.c_void_p(p)


def _check(t, name, dtype, shape, device):
    """Every tensor handed to the kernels as a raw device pointer: right dtype, exact shape,
    contiguous, on the loop's device.  A wrong one would be an out-of-bounds access or a host
    pointer dereferenced by the GPU, so it is rejected here."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if t.device != device:
        raise ValueError(f"{name}: must live on {device}, got {t.device}")
    return t


class DeviceLoop:
    """B independent MPC instances stepped on one GPU.

    P (B, n_p) float64 parameters live on the device; w holds the last solution
    and w0 the shifted warm start.  With warm_duals (default) the constraint and
    bound multipliers are shifted as well and the next solve starts as IPOPT's
    warm_start_init_point (spec.warm_*); the first solve is always cold.
    ``step()`` enqueues one fused solve + plant/shift launch on ``stream`` and
    returns immediately (``solve()`` / ``shift()`` do the two halves separately).
    A linear model embedded in a larger kernel instantiation (``lti.StatePad``) takes P0 in
    its own layout; the device tensors hold the kernel's padded layout
    (``solver._pad.w_idx`` / ``p_idx`` / ``g_idx`` select the model's entries).
    """

    def __init__(self, solver: Solver, P0, device="cuda", stream=None, cold_first=True, warm_duals=True):
        self.solver = solver
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceLoop needs a HIP device (torch 'cuda' device)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        P0 = np.ascontiguousarray(np.asarray(P0, np.float64))
        if P0.ndim != 2 or P0.shape[1] != solver.n_p:
            raise ValueError(f"P0: expected (B, {solver.n_p}), got {P0.shape}")
        pd = getattr(solver, "_pad", None)
        if pd is not None:
            P0 = pd.scatter(P0, pd.p_idx, pd.n_p_pad)
        self._knx = pd.nxp if pd is not None else solver.ocp.nx  # states of the kernel layout
        self.B = P0.shape[0]
        nw, ng = solver._h.n_w, solver._h.n_g
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)  # noqa: E731
        self.P = torch.from_numpy(P0).to(self.device)
        self.w, self.w0 = z(self.B, nw), z(self.B, nw)
        self.lam, self.lam0 = z(self.B, ng), z(self.B, ng)
        self.lamx, self.lamx0 = z(self.B, nw), z(self.B, nw)
        self.f = z(self.B)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.iters = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.warm_duals = warm_duals
        self._cold = cold_first

    def solve(self, status_out=None, iters_out=None):
        """Enqueue one batched solve.  status_out / iters_out: optional int32 device
        tensors (B,) that receive this step's statuses / iteration counts directly
        from the kernel (no extra launch)."""
        lib = _lib.load()
        s = ctypes_void(self.stream.cuda_stream)
        w0 = None if self._cold else _ptr(self.w0)
        warm = self.warm_duals and not self._cold
        st = self.status if status_out is None else _check(status_out, "status_out", torch.int32, (self.B,), self.device)
        it = self.iters if iters_out is None else _check(iters_out, "iters_out", torch.int32, (self.B,), self.device)
        _lib.check(lib.mpcx_solve_batch_dev(self.solver._h.ptr, self.B, _ptr(self.P), w0,
                                            _ptr(self.lam0) if warm else None, _ptr(self.lamx0) if warm else None,
                                            _ptr(self.w), _ptr(self.f), _ptr(self.lam), _ptr(self.lamx), _ptr(st),
                                            _ptr(it), s))
        self._cold = False

    def shift(self):
        lib = _lib.load()
        s = ctypes_void(self.stream.cuda_stream)
        d = self.warm_duals
        _lib.check(lib.mpcx_shift_dev(self.solver._h.ptr, self.B, _ptr(self.P), _ptr(self.w), _ptr(self.w0),
                                      _ptr(self.lam) if d else None, _ptr(self.lam0) if d else None,
                                      _ptr(self.lamx) if d else None, _ptr(self.lamx0) if d else None, s))

    def _point(self, point):
        n_p, nw, ng = self.P.shape[1], self.solver._h.n_w, self.lam.shape[1]
        if point is None:
            return self.P, self.w, self.lam, self.lamx
        if len(point) != 4:
            raise ValueError("point: expected (P, w, lam, lamx)")
        for t, name, n in zip(point, ("point P", "point w", "point lam", "point lamx"), (n_p, nw, ng, nw)):
            _check(t, name, torch.float64, (self.B, n), self.device)
        return point

    def _cotangents(self, gw):
        """The cotangents of a ``*_vjp`` call, (B, m, n_w) with 1 <= m <= nx: validated; returns m."""
        nw, nx = self.solver._h.n_w, self._knx
        if not isinstance(gw, torch.Tensor) or gw.dim() != 3 or not 1 <= gw.shape[1] <= nx:
            raise ValueError(f"gw: expected a ({self.B}, m, {nw}) tensor with 1 <= m <= {nx}")
        _check(gw, "gw", torch.float64, (self.B, gw.shape[1], nw), self.device)
        return gw.shape[1]

    def _stage_rows(self, d, name, n):
        """The directions of weight or model rows (n entries each), (B, m, n) for rows used at every
        stage or (B, m, N, n) for one row per stage, 1 <= m <= nx: validated; returns (m, per_stage)."""
        nx, N = self._knx, self.solver.ocp.N
        if not isinstance(d, torch.Tensor) or d.dim() not in (3, 4) or not 1 <= d.shape[1] <= nx:
            raise ValueError(f"{name}: expected a ({self.B}, m, {n}) or ({self.B}, m, {N}, {n}) tensor with "
                             f"1 <= m <= {nx}")
        m, per_stage = d.shape[1], int(d.dim() == 4)
        _check(d, name, torch.float64, (self.B, m, N, n) if per_stage else (self.B, m, n), self.device)
        return m, per_stage

    def _sens(self, entry, point, args, flag_out, *outs):
        """What the sensitivity methods share once their inputs are validated: resolve ``point``, take
        the outputs ``outs`` = (name, tensor given or None, shape[, allocate]) and the flag -- one not
        given is allocated on the loop's stream (or stays None with allocate False: not computed), one
        given is validated -- and enqueue the C entry point ``entry`` (point, *args, outputs, flag,
        stream) on the loop's stream.  Returns (*outputs, flag)."""
        point = self._point(point)
        outs = [o if len(o) == 4 else o + (True,) for o in outs] + [("flag_out", flag_out, (self.B,), True)]
        dtypes = [torch.float64] * (len(outs) - 1) + [torch.int32]
        with torch.cuda.stream(self.stream):
            ts = [torch.empty(shape, dtype=dt, device=self.device) if t is None and alloc else t
                  for (_, t, shape, alloc), dt in zip(outs, dtypes)]
        for (name, _, shape, _), t, dt in zip(outs, ts, dtypes):
            if t is not None:
                _check(t, name, dt, shape, self.device)
        _lib.check(getattr(_lib.load(), entry)(self.solver._h.ptr, self.B, *map(_ptr, point), *args, *map(_ptr, ts),
                                               ctypes_void(self.stream.cuda_stream)))
        return tuple(ts)

    def sens_x0(self, dw_out=None, K0_out=None, flag_out=None):
        """Enqueue one sensitivity launch (mpcx_sens_x0_dev) at the loop's resident P, w, lam, lamx:
        dw_dx0 (B, n_w, nx), K0 (B, nu, nx) -- the feedback gain, u ~ u0* + K0 (x - x0) -- and
        flag (B,) int32 (1 = irregular instance, NaN outputs), in the kernel's layout (a padded
        linear model: its pad states included).  Tensors given are written in place, the others are
        allocated; returns (dw_dx0, K0, flag) without waiting for the stream.  After ``solve()``
        P still holds the x0 the solution belongs to; ``step()`` has already advanced it."""
        nw, nx, nu = self.solver._h.n_w, self._knx, self.solver.ocp.nu
        return self._sens("mpcx_sens_x0_dev", None, (), flag_out,
                          ("dw_out", dw_out, (self.B, nw, nx)), ("K0_out", K0_out, (self.B, nu, nx)))

    def sens_p(self, dP, dw_out=None, flag_out=None):
        """Enqueue one parameter-sensitivity launch (mpcx_sens_p_dev) at the loop's resident P, w, lam,
        lamx: dP (B, m, n_p) float64 device tensor of m <= nx directions, each shaped like a row of the
        resident P (the kernel's layout: a padded linear model's pad entries included), gives
        dw (B, n_w, m), the first-order change of w along each direction, and flag (B,) int32
        (1 = irregular instance, NaN outputs).  Tensors given are written in place, the others are
        allocated; returns (dw, flag) without waiting for the stream."""
        nw, nx = self.solver._h.n_w, self._knx
        if not isinstance(dP, torch.Tensor) or dP.dim() != 3 or not 1 <= dP.shape[1] <= nx:
            raise ValueError(f"dP: expected a ({self.B}, m, {self.P.shape[1]}) tensor with 1 <= m <= {nx}")
        m = dP.shape[1]
        _check(dP, "dP", torch.float64, (self.B, m, self.P.shape[1]), self.device)
        return self._sens("mpcx_sens_p_dev", None, (_ptr(dP), m), flag_out, ("dw_out", dw_out, (self.B, nw, m)))

    def sens_vjp(self, gw, gP_out=None, flag_out=None, point=None):
        """Enqueue one adjoint-sensitivity launch (mpcx_sens_vjp_dev) at the loop's resident P, w, lam,
        lamx: gw (B, m, n_w) float64 device tensor of m <= nx cotangents, each shaped like a row of the
        resident w (the kernel's layout: a padded linear model's pad entries included), gives
        gP (B, m, n_p) = (dw/dP)^T gw, the gradient rows shaped like the resident P, and flag (B,) int32
        (1 = irregular instance, NaN outputs).  point = (P, w, lam, lamx): device tensors of the
        resident ones' shapes to take the point from instead (the next solve overwrites the resident
        ones; a saved point does not move).  Tensors given are written in place, the others are
        allocated; returns (gP, flag) without waiting for the stream."""
        m = self._cotangents(gw)
        return self._sens("mpcx_sens_vjp_dev", point, (_ptr(gw), m), flag_out,
                          ("gP_out", gP_out, (self.B, m, self.P.shape[1])))

    def sens_bounds(self, dlbw, dubw, dw_out=None, flag_out=None, point=None):
        """Enqueue one bound-sensitivity launch (mpcx_sens_bounds_dev) at the loop's resident P, w, lam,
        lamx and the bounds in force (``set_bounds``, else the problem's): dlbw / dubw (B, m, n_w)
        float64 device tensors of m <= nx directions of the lower / upper bounds, each shaped like a
        row of the resident w (the kernel's layout), either None (zeros), give dw (B, n_w, m) and
        flag (B,) int32 (1 = irregular instance, NaN outputs).  point: as :meth:`sens_vjp`.  Tensors
        given are written in place, the others are allocated; returns (dw, flag) without waiting for
        the stream."""
        nw, nx = self.solver._h.n_w, self._knx
        given = dlbw if dlbw is not None else dubw
        if not isinstance(given, torch.Tensor) or given.dim() != 3 or not 1 <= given.shape[1] <= nx:
            raise ValueError(f"dlbw / dubw: expected ({self.B}, m, {nw}) tensors with 1 <= m <= {nx} (one may be None)")
        m = given.shape[1]
        with torch.cuda.stream(self.stream):
            dlbw, dubw = (torch.zeros_like(given) if t is None else t for t in (dlbw, dubw))
        _check(dlbw, "dlbw", torch.float64, (self.B, m, nw), self.device)
        _check(dubw, "dubw", torch.float64, (self.B, m, nw), self.device)
        return self._sens("mpcx_sens_bounds_dev", point, (_ptr(dlbw), _ptr(dubw), m), flag_out,
                          ("dw_out", dw_out, (self.B, nw, m)))

    def sens_bounds_vjp(self, gw, glbw_out=None, gubw_out=None, flag_out=None, point=None):
        """Enqueue one launch of the reverse mode of :meth:`sens_bounds` (mpcx_sens_bounds_vjp_dev): gw
        (B, m, n_w) float64 device tensor of m <= nx cotangents shaped like rows of the resident w gives
        glbw, gubw (B, m, n_w), the gradient rows with respect to the bounds in force (every entry
        written: 0 where there is no finite bound), and flag (B,) int32.  point = (P, w, lam, lamx): as
        :meth:`sens_vjp`; the bounds are always the ones in force at the call.  Returns (glbw, gubw,
        flag) without waiting for the stream."""
        m, nw = self._cotangents(gw), self.solver._h.n_w
        return self._sens("mpcx_sens_bounds_vjp_dev", point, (_ptr(gw), m), flag_out,
                          ("glbw_out", glbw_out, (self.B, m, nw)), ("gubw_out", gubw_out, (self.B, m, nw)))

    def sens_weights(self, dW, dw_out=None, flag_out=None, point=None):
        """Enqueue one weight-sensitivity launch (mpcx_sens_weights_dev) at the loop's resident P, w, lam,
        lamx, the solver's weights and the bounds in force: dW a float64 device tensor of m <= nx
        directions of the weight rows in the kernel's layout (n_wt = ``solver._h.weight_dims()`` entries:
        (Q, R), or a padded linear model's packed table, pad entries included), (B, m, n_wt) for rows
        used at every stage or (B, m, N, n_wt) for one row per stage, gives dw (B, n_w, m) and flag (B,)
        int32 (1 = irregular instance, NaN outputs).  point: as :meth:`sens_vjp`.  Tensors given are
        written in place, the others are allocated; returns (dw, flag) without waiting for the stream."""
        m, per_stage = self._stage_rows(dW, "dW", self.solver._h.weight_dims())
        return self._sens("mpcx_sens_weights_dev", point, (_ptr(dW), per_stage, m), flag_out,
                          ("dw_out", dw_out, (self.B, self.solver._h.n_w, m)))

    def sens_weights_vjp(self, gw, gWk_out=None, gW_out=None, flag_out=None, point=None, per_stage=True):
        """Enqueue one launch of the reverse mode of :meth:`sens_weights` (mpcx_sens_weights_vjp_dev): gw
        (B, m, n_w) float64 device tensor of m <= nx cotangents shaped like rows of the resident w gives
        gWk (B, m, N, n_wt), the gradient rows with respect to every stage's own weight row (None with
        per_stage=False and no gWk_out: not computed), gW (B, m, n_wt), their sum over the stages, and
        flag (B,) int32, in the kernel's layout.  point = (P, w, lam, lamx): as :meth:`sens_vjp`; the
        weights and bounds are the ones in force at the call.  Returns (gWk, gW, flag) without waiting
        for the stream."""
        N, n_wt = self.solver.ocp.N, self.solver._h.weight_dims()
        m = self._cotangents(gw)
        return self._sens("mpcx_sens_weights_vjp_dev", point, (_ptr(gw), m), flag_out,
                          ("gWk_out", gWk_out, (self.B, m, N, n_wt), per_stage), ("gW_out", gW_out, (self.B, m, n_wt)))

    def sens_model(self, dTh, dw_out=None, flag_out=None, point=None):
        """Enqueue one model-sensitivity launch (mpcx_sens_model_dev) at the loop's resident P, w, lam, lamx,
        the solver's constants or tables and the bounds in force: dTh a float64 device tensor of m <= nx
        directions of the model rows in the kernel's layout (n_th = ``solver._h.model_dims()`` entries: the
        constants of ``par`` the model reads, or a linear model's (A, B, c) of the padded layout), (B, m, n_th)
        for rows used at every stage or (B, m, N, n_th) for one row per stage, gives dw (B, n_w, m) and flag
        (B,) int32 (1 = irregular instance, NaN outputs).  point: as :meth:`sens_vjp`.  Tensors given are
        written in place, the others are allocated; returns (dw, flag) without waiting for the stream."""
        m, per_stage = self._stage_rows(dTh, "dTh", self.solver._h.model_dims())
        return self._sens("mpcx_sens_model_dev", point, (_ptr(dTh), per_stage, m), flag_out,
                          ("dw_out", dw_out, (self.B, self.solver._h.n_w, m)))

    def sens_model_vjp(self, gw, gThk_out=None, gTh_out=None, flag_out=None, point=None, per_stage=True):
        """Enqueue one launch of the reverse mode of :meth:`sens_model` (mpcx_sens_model_vjp_dev): gw
        (B, m, n_w) float64 device tensor of m <= nx cotangents shaped like rows of the resident w gives
        gThk (B, m, N, n_th), the gradient rows with respect to every stage's own model row (None with
        per_stage=False and no gThk_out: not computed), gTh (B, m, n_th), their sum over the stages, and
        flag (B,) int32, in the kernel's layout.  point = (P, w, lam, lamx): as :meth:`sens_vjp`; the
        constants and bounds are the ones in force at the call.  Returns (gThk, gTh, flag) without waiting
        for the stream."""
        N, n_th = self.solver.ocp.N, self.solver._h.model_dims()
        m = self._cotangents(gw)
        return self._sens("mpcx_sens_model_vjp_dev", point, (_ptr(gw), m), flag_out,
                          ("gThk_out", gThk_out, (self.B, m, N, n_th), per_stage),
                          ("gTh_out", gTh_out, (self.B, m, n_th)))

    def set_stage_refs(self, refs):
        """Per-step stage references (tracking, param layout x0_stageref): refs is a
        (B, N*(nx+nu)) float64 device tensor copied into P[:, nx:] on the loop's stream
        (Trajectory_tracking.py:105-106 sets solver.par["p", k] each step)."""
        nx = self._knx
        _check(refs, "refs", torch.float64, (self.B, self.P.shape[1] - nx), self.device)
        with torch.cuda.stream(self.stream):
            self.P[:, nx:].copy_(refs, non_blocking=True)

    def run(self, K, status_out=None, iters_out=None, Pseq=None, tabseq=None):
        """K closed-loop steps in ONE launch (mpcx_run_dev): each instance runs its own
        receding-horizon loop without waiting for the others between steps; the results
        equal K calls of step() bit for bit.  status_out / iters_out: int32 (K, B) device
        tensors (or None -> allocated).  Pseq (K, B, n_p) float64 and tabseq (K, B, N) int32
        device tensors give per-step stage references / linear schedules (row 0 = the
        current ones).  Returns (status, iters)."""
        lib = _lib.load()
        s = ctypes_void(self.stream.cuda_stream)
        K = int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        bnd = self.solver._dev_bounds
        if bnd is not None and bnd[3] > 1:
            raise ValueError(f"run: per-step bounds ({bnd[3]} steps) are installed and a multi-step launch loads an "
                             "instance's bounds once, at its start; call step() with set_bounds() before each step")
        z = lambda: torch.zeros((K, self.B), dtype=torch.int32, device=self.device)  # noqa: E731
        st = z() if status_out is None else _check(status_out, "status_out", torch.int32, (K, self.B), self.device)
        it = z() if iters_out is None else _check(iters_out, "iters_out", torch.int32, (K, self.B), self.device)
        if Pseq is not None:
            _check(Pseq, "Pseq", torch.float64, (K, self.B, self.P.shape[1]), self.device)
        if tabseq is not None:
            _check(tabseq, "tabseq", torch.int32, (K, self.B, self.solver.ocp.N), self.device)
        flags = _lib.STEP_COLD if self._cold else 0
        if not self.warm_duals:
            flags |= _lib.STEP_PRIMAL_ONLY
        d = self.warm_duals
        _lib.check(lib.mpcx_run_dev(self.solver._h.ptr, self.B, K, _ptr(self.P), _ptr(self.w0),
                                    _ptr(self.lam0) if d else None, _ptr(self.lamx0) if d else None, flags, _ptr(Pseq),
                                    _ptr(tabseq), _ptr(self.w), _ptr(self.f), _ptr(self.lam), _ptr(self.lamx), _ptr(st),
                                    _ptr(it), s))
        self._cold = False
        return st, it

    def set_schedule(self, tab):
        """Per-step stage schedule of a linear model: tab is a (B, N) int32 device tensor
        of table indices read by the next solves/shifts (mpcx_set_linear_tab_dev; LTV
        re-linearisation per step, Trajectory_tracking_dynamic_model.py:117-141).  The
        tensor must stay alive while it is in use; None reverts to the uploaded schedule."""
        lib = _lib.load()
        if tab is None:
            _lib.check(lib.mpcx_set_linear_tab_dev(self.solver._h.ptr, None, 0))
            self._tab = None
            return
        _check(tab, "tab", torch.int32, (self.B, self.solver.ocp.N), self.device)
        self._tab = tab
        _lib.check(lib.mpcx_set_linear_tab_dev(self.solver._h.ptr, ctypes_void(tab.data_ptr()), self.B))

    def set_bounds(self, lbw, ubw):
        """Per-instance box bounds of the next solves (mpcx_set_bounds_dev): lbw / ubw are float64
        device tensors (B, n_w), one row per instance in the solver's w layout, +-1e20 = no bound
        (the X_0 entries are not read); None, None reverts to the problem's bounds.  (K, B, n_w)
        tensors hold K steps' bounds (a corridor that moves with time): solve() and step() read
        block 0 and run() refuses them -- such a loop is stepped in lock step, set_bounds(lb[s],
        ub[s]) before step s.  The tensors are validated on the loop's stream (the call waits for it; a NaN,
        lb > ub or lb == ub raises and leaves the bounds as they were) and are kept alive here;
        they must not be written to while installed -- call set_bounds again after changing them."""
        if lbw is None and ubw is None:
            self.solver._install_bounds(None)
            return
        if lbw is None or ubw is None:
            raise ValueError("set_bounds: lbw and ubw must both be given (or both None)")
        pd = getattr(self.solver, "_pad", None)
        n_w = pd.n_w if pd is not None else self.solver._h.n_w
        K = lbw.shape[0] if isinstance(lbw, torch.Tensor) and lbw.dim() == 3 else None
        shape = (self.B, n_w) if K is None else (K, self.B, n_w)
        _check(lbw, "lbw", torch.float64, shape, self.device)
        _check(ubw, "ubw", torch.float64, shape, self.device)
        if pd is not None:  # user layout -> the kernel's padded layout, pad states unbounded
            idx = torch.from_numpy(pd.w_idx).to(self.device)
            with torch.cuda.stream(self.stream):
                full = [torch.full(shape[:-1] + (pd.n_w_pad,), inf, dtype=torch.float64, device=self.device)
                        for inf in (-1e20, 1e20)]
                full[0][..., idx] = lbw
                full[1][..., idx] = ubw
            lbw, ubw = full
        self.solver._install_bounds((lbw, ubw, self.B, 1 if K is None else K), self.stream.cuda_stream)

    def step(self, status_out=None, iters_out=None):
        """One closed-loop step = ONE kernel launch (mpcx_step_dev): the batched solve and,
        fused into its epilogue, the plant + shifted warm start (same result as
        solve() followed by shift())."""
        lib = _lib.load()
        s = ctypes_void(self.stream.cuda_stream)
        flags = _lib.STEP_COLD if self._cold else (0 if self.warm_duals else _lib.STEP_PRIMAL_ONLY)
        d = self.warm_duals
        st = self.status if status_out is None else _check(status_out, "status_out", torch.int32, (self.B,), self.device)
        it = self.iters if iters_out is None else _check(iters_out, "iters_out", torch.int32, (self.B,), self.device)
        _lib.check(lib.mpcx_step_dev(self.solver._h.ptr, self.B, _ptr(self.P), _ptr(self.w0),
                                     _ptr(self.lam0) if d else None, _ptr(self.lamx0) if d else None, flags,
                                     _ptr(self.w), _ptr(self.f), _ptr(self.lam), _ptr(self.lamx), _ptr(st), _ptr(it),
                                     s))
        self._cold = False
