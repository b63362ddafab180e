"""CasADi-``nlpsol``-shaped façade over libmpcx (the drop-in for the hot path).

Reference boundary (``Casadi/multiple_shooting_casadi.py``):

    solver = ca.nlpsol('solver', 'ipopt', prob, opts)                       # :197
    sol = solver(x0=w0, lbx=lbw, ubx=ubw, lbg=lbg, ubg=ubg, p=P)           # :235-242
    u = sol['x'][3:5] ...                                                   # :243-256
    state_init = F(args['p'], u[:, 0])[0]                                   # :273

Here:

    solver = mpcx.nlpsol('solver', 'mi355x', ocp, opts)
    sol = solver(x0=w0, lbx=lbw, ubx=ubw, lbg=lbg, ubg=ubg, p=P)
    F = mpcx.integrator(ocp)

``sol`` holds numpy column vectors with CasADi's shapes and sign conventions:
'x' (n_w,1), 'f' (1,1), 'g' (n_g,1), 'lam_g' (n_g,1), 'lam_x' (n_w,1),
'lam_p' (n_p,1; zeros).  ``solver.stats()`` mirrors CasADi's stats dict
('return_status', 'success', 'iter_count', 't_wall_total').  Batched use:
``solver.solve_batch(P, w0)``.  Every call runs the HIP kernel on the GPU.
"""
from __future__ import annotations

import dataclasses
import math
import time

import numpy as np

from . import _lib
from .lti import LinearOCP, state_pad
from .ocp import IPOPT_OPTIONS, OCP, to_spec
from .ode import OdeOCP


def _vec(v, n, name, fill=None):
    """CasADi-style input coercion: list / ndarray / DM-like / scalar (broadcast)."""
    if v is None:
        if fill is None:
            return None
        return np.full(n, float(fill))
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1 and n != 1:
        a = np.full(n, float(a[0]))
    if a.size != n:
        raise ValueError(f"{name}: expected {n} entries, got {a.size}")
    return np.ascontiguousarray(a)


def _batch_bounds(lbw, ubw, B, nw):
    """The lbw / ubw arguments of ``solve_batch``: (lbw, ubw, per_instance).  Scalars and n_w vectors
    (rows and columns included) are one bound vector for the batch, as ever (None = the spec's);
    a matrix is one row per instance and must be (B, n_w) -- then both are returned as (B, n_w)
    arrays, a scalar or vector counterpart repeated for every instance.  Entries at or beyond
    +-1e19 become +-1e20 (no bound); NaN is kept for the library to refuse."""
    arrs = [None if v is None else np.asarray(v, dtype=np.float64) for v in (lbw, ubw)]
    matrix = [a is not None and a.ndim >= 2 and (a.ndim > 2 or min(a.shape) > 1) for a in arrs]
    if not any(matrix):
        return _vec(lbw, nw, "lbw"), _vec(ubw, nw, "ubw"), False
    out = []
    for a, m, name, inf in zip(arrs, matrix, ("lbw", "ubw"), (-1e20, 1e20)):
        if a is None:
            raise ValueError(f"{name}: per-instance bounds need both lbw and ubw")
        if m and a.shape != (B, nw):
            raise ValueError(f"{name}: expected ({B}, {nw}) per-instance bounds or {nw} entries, got {a.shape}")
        if not m:
            a = np.broadcast_to(_vec(a, nw, name), (B, nw))
        keep = np.isnan(a) | (a > -1e19 if inf < 0 else a < 1e19)
        out.append(np.ascontiguousarray(np.where(keep, a, inf)))
    return out[0], out[1], True


class Solver:
    """Callable returned by :func:`nlpsol`."""

    _pad = None  # lti.StatePad of a linear model embedded in a larger kernel instantiation
    _dev_bounds = None  # installed device bounds: (lbw, ubw, rows, n_steps), the tensors kept alive

    def __init__(self, name: str, ocp: OCP, opts: dict | None = None, device: int = 0):
        opts = dict(opts or {})
        ip = dict(opts.get("ipopt", {}))
        self.name = name
        self.ocp = ocp
        self.max_iter = int(ip.pop("max_iter", 3000))
        self.tol = float(ip.pop("tol", 1e-8))
        # output options have no effect here (no iteration log is printed)
        for k in ("print_level", "sb"):
            ip.pop(k, None)
        # termination options (acceptable_tol / acceptable_obj_change_tol at :192-193), IPOPT's
        # semantics; the rest keep IPOPT's defaults
        term = {k: ip.pop(k) for k in IPOPT_OPTIONS if k in ip}
        if ip:
            raise ValueError(f"unsupported ipopt options: {sorted(ip)}")
        # not CasADi options: lanes per instance (0 = fill idle SIMDs, 1 = narrowest group; same
        # results); restoration (False: a failed line search ends the solve, IPOPT has no such switch)
        self.group_policy = int(opts.get("group_policy", 0))
        self.restoration = bool(opts.get("restoration", True))
        # a linear model without its own kernel instantiation runs embedded in one (lti.StatePad)
        self._pad = state_pad(ocp)
        kocp = self._pad.ocp if self._pad else ocp
        self._h = _lib.Handle(to_spec(kocp, self.max_iter, self.tol, device, group_policy=self.group_policy, ipopt=term,
                                      restoration=self.restoration))
        if ocp.model == "linear":
            self._h.set_linear_model(kocp)
        self._stats = {}

    def _install_bounds(self, state, stream=None):
        """mpcx_set_bounds_dev with device tensors (lbw, ubw, rows, n_steps), or None = the spec bounds."""
        if state is None:
            self._h.set_bounds_dev(None, None)
        else:
            lb, ub, rows, n_steps = state
            self._h.set_bounds_dev(lb.data_ptr(), ub.data_ptr(), rows, n_steps, stream)
        self._dev_bounds = state

    def set_linear_model(self, lin=None):
        """Re-upload stage tables (LTV: new tables or per-instance schedule for the next step)."""
        if lin is not None:
            if lin.model != "linear" or (lin.nx, lin.nu, lin.N) != (self.ocp.nx, self.ocp.nu, self.ocp.N):
                raise ValueError("set_linear_model: incompatible problem")
            self.ocp = lin
        if self._pad is not None:
            self._pad = state_pad(self.ocp)
        self._h.set_linear_model(self._pad.ocp if self._pad else self.ocp)

    # ---------------------------------------------------------------- layout
    @property
    def n_w(self):
        return self.ocp.N * self.ocp.nu if self.ocp.formulation == "single_shooting" else self._ms_nw

    @property
    def n_g(self):
        return self.ocp.N * self._ss_ng if self.ocp.formulation == "single_shooting" else self._ms_ng

    @property
    def _ms_nw(self):
        """Multiple-shooting layout sizes of the user's problem (the kernel's unless padded)."""
        return self._pad.n_w if self._pad else self._h.n_w

    @property
    def _ms_ng(self):
        return self._pad.n_g if self._pad else self._h.n_g

    @property
    def _ss_ng(self):
        """Single shooting: g entries per node k = 1..N -- (x_k, y_k) for the unicycle
        (``single_shooting_v2.py:115-158``), the whole state for the ODE models."""
        return 2 if self.ocp.model == "unicycle" else self.ocp.nx

    @property
    def n_p(self):
        return self._pad.n_p if self._pad else self._h.n_p

    def stats(self):
        return dict(self._stats)

    # ---------------------------------------------------------------- batched core
    def solve_batch(self, P, w0=None, lbw=None, ubw=None, want_lam=True, want_g=False, lam_g0=None, lam_x0=None):
        """Solve B independent NLPs (multiple-shooting layout).

        P (B, n_p); w0 (B, n_w) or None (cold start X_k = x0, U = 0);
        lbw / ubw: None (the problem's bounds), a scalar or n_w entries shared by the batch, or
        (B, n_w) arrays with one row per instance (uploaded and installed as device bounds for
        this call, mpcx_set_bounds_dev, then whatever was installed before is put back);
        lam_g0 (B, n_g) / lam_x0 (B, n_w): warm-start multipliers (IPOPT
        warm_start_init_point), or None.
        Returns dict of arrays: w (B,n_w), f (B,), lam_g (B,n_g), lam_x (B,n_w), status (B,), iters (B,),
        g (B,n_g).
        """
        P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, np.float64)))
        B = P.shape[0]
        if P.shape[1] != self.n_p:
            raise ValueError(f"P: expected {self.n_p} columns, got {P.shape[1]}")
        nw, ng = self._ms_nw, self._ms_ng
        w0a = None
        if w0 is not None:
            w0a = np.ascontiguousarray(np.asarray(w0, np.float64).reshape(B, nw))
        lbw, ubw, per_instance = _batch_bounds(lbw, ubw, B, nw)  # the library reads n_w entries of each row
        l0 = None if lam_g0 is None else np.ascontiguousarray(np.asarray(lam_g0, np.float64).reshape(B, ng))
        lx0 = None if lam_x0 is None else np.ascontiguousarray(np.asarray(lam_x0, np.float64).reshape(B, nw))
        pd = self._pad
        if pd is not None:  # user layout -> the kernel's padded layout (pad states unbounded, 0)
            P = pd.scatter(P, pd.p_idx, pd.n_p_pad)
            w0a = pd.scatter(w0a, pd.w_idx, pd.n_w_pad)
            if per_instance:
                lbw, ubw = pd.scatter(lbw, pd.w_idx, pd.n_w_pad, -1e20), pd.scatter(ubw, pd.w_idx, pd.n_w_pad, 1e20)
            else:
                lbw = None if lbw is None else pd.scatter(lbw[None, :], pd.w_idx, pd.n_w_pad, -1e20)[0]
                ubw = None if ubw is None else pd.scatter(ubw[None, :], pd.w_idx, pd.n_w_pad, 1e20)[0]
            l0 = pd.scatter(l0, pd.g_idx, pd.n_g_pad)
            lx0 = pd.scatter(lx0, pd.w_idx, pd.n_w_pad)
            nw, ng = pd.n_w_pad, pd.n_g_pad
        w = np.empty((B, nw))
        f = np.empty(B)
        lam = np.empty((B, ng)) if want_lam else None
        lamx = np.empty((B, nw)) if want_lam else None
        g = np.empty((B, ng)) if want_g else None
        st = np.empty(B, np.int32)
        it = np.empty(B, np.int32)
        lib = _lib.load()
        before = self._dev_bounds
        if per_instance:  # device memory comes from PyTorch, as in mpcx.device
            import torch

            dev = torch.device("cuda", self._h.spec.device)
            self._install_bounds((torch.from_numpy(lbw).to(dev), torch.from_numpy(ubw).to(dev), B, 1),
                                 torch.cuda.current_stream(dev).cuda_stream)
            lbw = ubw = None
        t0 = time.perf_counter()
        try:
            _lib.check(lib.mpcx_solve_batch(self._h.ptr, B, _lib.dptr(P), _lib.dptr(w0a), _lib.dptr(l0),
                                            _lib.dptr(lx0), _lib.dptr(lbw), _lib.dptr(ubw), _lib.dptr(w), _lib.dptr(f),
                                            _lib.dptr(g), _lib.dptr(lam), _lib.dptr(lamx), _lib.iptr(st),
                                            _lib.iptr(it)))
        finally:
            if per_instance:  # (the solve has finished: mpcx_solve_batch waits for its results)
                self._install_bounds(before)
        t = time.perf_counter() - t0
        if pd is not None:
            w, lamx = pd.gather(w, pd.w_idx), pd.gather(lamx, pd.w_idx)
            lam, g = pd.gather(lam, pd.g_idx), pd.gather(g, pd.g_idx)
        return {"w": w, "f": f, "lam_g": lam, "lam_x": lamx, "g": g, "status": st, "iters": it, "t_wall": t}

    def sens_x0(self, P, res, lbw=None, ubw=None):
        """Sensitivities of the solutions ``res`` (a ``solve_batch`` result: 'w', 'lam_g', 'lam_x') to the
        initial state x0 = P[:, :nx] (mpcx_sens_x0): one launch of the sensitivity kernel, no solve.

        lbw / ubw: the bounds the solve used -- None (the problem's, or installed device bounds), a
        scalar or n_w entries shared by the batch.
        Returns {'dw_dx0': (B, n_w, nx), 'K0': (B, nu, nx), 'flag': (B,)}: row i of dw_dx0[b] is
        d w_i / d x0 (the X_0 rows are the identity), K0 = dU_0/dx0 is the feedback gain
        u ~ u0* + K0 (x - x0); flag 1 marks an irregular instance (a variable on its bound, an
        indefinite reduced Hessian), whose outputs are NaN.  These are the sensitivities of the barrier
        problem at the multipliers given: the active-set ones to O(mu) at a strictly complementary
        solution.  The single-shooting form gets the rows of its own w, the controls: (B, N nu, nx)."""
        B, point, (lbw, ubw, _) = self._sens_point(P, res, lbw, ubw, instance_bounds=False)
        nx, nu = self.ocp.nx, self.ocp.nu
        nw, knx, _ = self._kdims
        dw = np.empty((B, nw, knx))
        K0 = np.empty((B, nu, knx))
        flag = np.empty(B, np.int32)
        _lib.check(_lib.load().mpcx_sens_x0(self._h.ptr, B, *map(_lib.dptr, point), _lib.dptr(lbw), _lib.dptr(ubw),
                                            _lib.dptr(dw), _lib.dptr(K0), _lib.iptr(flag)))
        pd = self._pad
        if pd is not None:  # the model's own states and inputs only
            dw, K0 = dw[:, pd.w_idx, :nx], K0[:, :, :nx]
        if self.ocp.formulation == "single_shooting":
            dw = dw[:, self._ss_rows()]
        return {"dw_dx0": np.ascontiguousarray(dw), "K0": np.ascontiguousarray(K0), "flag": flag}

    def sens_p(self, P, res, dP, lbw=None, ubw=None):
        """Directional sensitivities of the solutions ``res`` to the whole parameter row -- x0 and the
        target or the stage references -- (mpcx_sens_p): dw = (d w*/d P) dP, no solve.

        dP: (B, m, n_p) directions, each shaped like a row of P, or (B, n_p) for a single one; any m
        (launches of at most nx columns each; a column's bits do not depend on the others).
        lbw / ubw: as for :meth:`sens_x0`.
        Returns {'dw': (B, n_w, m), 'du0': (B, nu, m), 'flag': (B,)}: column j of dw[b] is the
        first-order change of w along dP[b, j] -- w(P + dP) ~ w + dw -- du0 its rows of U_0, and
        flag 1 marks an irregular instance (NaN outputs), as :meth:`sens_x0`.  The X_0 rows are
        dP[:, :, :nx].  The single-shooting form gets the control rows.  Not for the path-frame
        bicycle (its stage rows enter the dynamics)."""
        B, point, bounds = self._sens_point(P, res, lbw, ubw, instance_bounds=False)
        dP = self._sens_cols(dP, B, "dP", of="p")
        (dw,), flag = self._sens_launches("mpcx_sens_p", B, point, bounds, [dP], (), [(2, (B, self._kdims[0]))])
        if self._pad is not None:  # the model's own states and inputs only
            dw = dw[:, self._pad.w_idx]
        nx, nu = self.ocp.nx, self.ocp.nu
        du0 = dw[:, nx:nx + nu]
        if self.ocp.formulation == "single_shooting":
            dw = dw[:, self._ss_rows()]
        return {"dw": np.ascontiguousarray(dw), "du0": np.ascontiguousarray(du0), "flag": flag}

    def sens_xref(self, P, res, lbw=None, ubw=None):
        """Sensitivities of the solutions ``res`` to the target x_ref of the x0_xref parameter layout
        (:meth:`sens_p` with the identity directions on x_ref).  Returns {'dw_dxref': (B, n_w, nx),
        'Kr': (B, nu, nx) = dU_0/dx_ref, 'flag'}: with :meth:`sens_x0`'s gain,
        u ~ u0* + K0 (x - x0) + Kr (x_ref' - x_ref)."""
        if self.ocp.param != "x0_xref":
            raise ValueError("sens_xref: the parameter layout has no target x_ref (stage references: use sens_p)")
        nx = self.ocp.nx
        B = np.atleast_2d(np.asarray(P)).shape[0]
        dP = np.zeros((B, nx, self.n_p))
        dP[:, np.arange(nx), nx + np.arange(nx)] = 1.0
        s = self.sens_p(P, res, dP, lbw, ubw)
        return {"dw_dxref": s["dw"], "Kr": s["du0"], "flag": s["flag"]}

    def sens_vjp(self, P, res, gw, lbw=None, ubw=None):
        """Adjoint sensitivities of the solutions ``res`` (mpcx_sens_vjp): gP = (d w*/d P)^T gw, the
        gradient with respect to every entry of the parameter row of a scalar loss whose gradient on the
        solution w is gw -- reverse mode of :meth:`sens_p`, no solve: <gw, sens_p(dP)> = <gP, dP>.

        gw: (B, m, n_w) cotangents, each shaped like a row of w, or (B, n_w) for a single one; any m
        (launches of at most nx columns each; a cotangent's bits do not depend on the others).  The
        single-shooting form takes them over its own w, the control rows.
        lbw / ubw: as for :meth:`sens_x0`.
        Returns {'gP': (B, m, n_p), 'flag': (B,)}; flag 1 marks an irregular instance (NaN outputs), as
        :meth:`sens_x0`.  Not for the path-frame bicycle (its stage rows enter the dynamics)."""
        B, point, bounds = self._sens_point(P, res, lbw, ubw, instance_bounds=False)
        gw = self._sens_cols(gw, B, "gw")
        (gP,), flag = self._sens_launches("mpcx_sens_vjp", B, point, bounds, [gw], (), [(1, (B, self._kdims[2]))])
        if self._pad is not None:  # the model's own parameters only
            gP = gP[:, :, self._pad.p_idx]
        return {"gP": np.ascontiguousarray(gP), "flag": flag}

    def gain_p(self, P, res, lbw=None, ubw=None):
        """The first move's gain on every parameter, dU_0/dP, from one launch (:meth:`sens_vjp` with the
        nu unit cotangents on the rows of U_0).  Returns {'dU0_dP': (B, nu, n_p), 'flag': (B,)}: its
        x0 block is :meth:`sens_x0`'s K0, and on the x0_xref layout its x_ref block is :meth:`sens_xref`'s
        Kr, each to rounding: u ~ u0* + dU0_dP (P' - P)."""
        nx, nu = self.ocp.nx, self.ocp.nu
        B = np.atleast_2d(np.asarray(P)).shape[0]
        single = self.ocp.formulation == "single_shooting"
        gw = np.zeros((B, nu, self.ocp.N * nu if single else self._ms_nw))
        gw[:, np.arange(nu), (0 if single else nx) + np.arange(nu)] = 1.0
        s = self.sens_vjp(P, res, gw, lbw, ubw)
        return {"dU0_dP": s["gP"], "flag": s["flag"]}

    def _sens_point(self, P, res, lbw, ubw, instance_bounds=True):
        """What the sensitivity calls share: the point (P and ``res``: 'w', 'lam_g', 'lam_x') and the
        bounds in the kernel's layout.  instance_bounds False: bounds shared by the batch only ((B, n_w)
        arrays are refused).  Returns (B, (P, w, lam, lamx), (lbw, ubw, per_instance))."""
        P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, np.float64)))
        B = P.shape[0]
        if P.shape[1] != self.n_p:
            raise ValueError(f"P: expected {self.n_p} columns, got {P.shape[1]}")
        nw, ng = self._ms_nw, self._ms_ng
        w, lam, lamx = (np.ascontiguousarray(np.asarray(res[key], np.float64).reshape(B, n))
                        for key, n in (("w", nw), ("lam_g", ng), ("lam_x", nw)))
        if instance_bounds:
            lbw, ubw, per_instance = _batch_bounds(lbw, ubw, B, nw)
        else:
            lbw, ubw, per_instance = _vec(lbw, nw, "lbw"), _vec(ubw, nw, "ubw"), False
        pd = self._pad
        if pd is not None:  # user layout -> the kernel's padded layout (pad states unbounded, 0)
            P = pd.scatter(P, pd.p_idx, pd.n_p_pad)
            w, lamx = pd.scatter(w, pd.w_idx, pd.n_w_pad), pd.scatter(lamx, pd.w_idx, pd.n_w_pad)
            lam = pd.scatter(lam, pd.g_idx, pd.n_g_pad)
            if per_instance:
                lbw, ubw = pd.scatter(lbw, pd.w_idx, pd.n_w_pad, -1e20), pd.scatter(ubw, pd.w_idx, pd.n_w_pad, 1e20)
            else:
                lbw = None if lbw is None else pd.scatter(lbw[None, :], pd.w_idx, pd.n_w_pad, -1e20)[0]
                ubw = None if ubw is None else pd.scatter(ubw[None, :], pd.w_idx, pd.n_w_pad, 1e20)[0]
        return B, (P, w, lam, lamx), (lbw, ubw, per_instance)

    @property
    def _kdims(self):
        """(n_w, nx, n_p) of the kernel's layout (the problem's own unless padded)."""
        pd = self._pad
        return (self._ms_nw, self.ocp.nx, self.n_p) if pd is None else (pd.n_w_pad, pd.nxp, pd.n_p_pad)

    def _ss_rows(self):
        """The rows of the multiple-shooting w that are the single-shooting form's w: the controls."""
        nx, nu = self.ocp.nx, self.ocp.nu
        return np.concatenate([nx + (nx + nu) * k + np.arange(nu) for k in range(self.ocp.N)])

    def _sens_cols(self, v, B, name, of="w"):
        """A block of m directions or cotangents, each shaped like a row of w (of the single-shooting
        form: its control rows) or, with of="p", of P: (B, m, n), or (B, n) for a single one, as
        (B, m, n) in the kernel's layout."""
        single = of == "w" and self.ocp.formulation == "single_shooting"
        n = self.n_p if of == "p" else self.ocp.N * self.ocp.nu if single else self._ms_nw
        v = np.asarray(v, np.float64)
        if v.ndim == 2:
            v = v[:, None, :]
        if v.ndim != 3 or v.shape[0] != B or v.shape[2] != n or v.shape[1] < 1:
            raise ValueError(f"{name}: expected ({B}, m, {n}) or ({B}, {n}), got {v.shape}")
        m = v.shape[1]
        if single:  # the control rows of a zero row of w
            full = np.zeros((B, m, self._ms_nw))
            full[:, :, self._ss_rows()] = v
            v = full
        pd = self._pad
        if pd is not None:
            idx, n_pad = (pd.p_idx, pd.n_p_pad) if of == "p" else (pd.w_idx, pd.n_w_pad)
            v = pd.scatter(v.reshape(B * m, -1), idx, n_pad).reshape(B, m, -1)
        return v

    def _sens_launches(self, entry, B, point, bounds, cols, mid, outs):
        """The launches of one sensitivity call over m columns, at most nx (of the kernel's layout) of
        them each: ``entry`` is the host-pointer C entry point (point, bounds, column blocks, *mid, m,
        outputs, flag), cols the (B, m, .) column blocks and outs a (column axis, shape without it) for
        every output.  Returns ([the outputs assembled over all m columns], the launches' flags ORed)."""
        m, knx = cols[0].shape[1], self._kdims[1]
        entry = getattr(_lib.load(), entry)
        full = [np.empty(rest[:ax] + (m,) + rest[ax:]) for ax, rest in outs]
        flag = np.zeros(B, np.int32)

        def call(lb, ub):
            for c0 in range(0, m, knx):
                mc = min(knx, m - c0)
                parts, fl = [np.empty(rest[:ax] + (mc,) + rest[ax:]) for ax, rest in outs], np.empty(B, np.int32)
                blocks = [np.ascontiguousarray(v[:, c0:c0 + mc]) for v in cols]
                _lib.check(entry(self._h.ptr, B, *map(_lib.dptr, point), _lib.dptr(lb), _lib.dptr(ub),
                                 *map(_lib.dptr, blocks), *mid, mc, *map(_lib.dptr, parts), _lib.iptr(fl)))
                for (ax, _), f, part in zip(outs, full, parts):
                    f[(slice(None),) * ax + (slice(c0, c0 + mc),)] = part
                np.bitwise_or(flag, fl, out=flag)

        self._with_bounds(B, *bounds, call)
        return full, flag

    def _sens_stage_rows(self, entry, B, point, bounds, d):
        """:meth:`sens_weights` / :meth:`sens_model` once their directions d (B, m, N or 1, .) are rows of
        the kernel's layout."""
        (dw,), flag = self._sens_launches(entry, B, point, bounds, [d], (int(d.shape[2] > 1),),
                                          [(2, (B, self._kdims[0]))])
        if self._pad is not None:  # the model's own states and inputs only
            dw = dw[:, self._pad.w_idx]
        return {"dw": np.ascontiguousarray(dw), "flag": flag}

    def _sens_stage_vjp(self, entry, P, res, gw, lbw, ubw, n_row):
        """:meth:`sens_weights_vjp` / :meth:`sens_model_vjp` in the kernel's layout (rows of n_row entries):
        (B, m, the per-stage rows (B, m, N, n_row), their sums over the stages (B, m, n_row), flag)."""
        B, point, bounds = self._sens_point(P, res, lbw, ubw)
        gw = self._sens_cols(gw, B, "gw")
        (gk, gs), flag = self._sens_launches(entry, B, point, bounds, [gw], (),
                                             [(1, (B, self.ocp.N, n_row)), (1, (B, n_row))])
        return B, gw.shape[1], gk, gs, flag

    def _sum_by_table(self, B, gk):
        """Per-stage rows gk (B, m, N, ...) of a linear model summed per table through every instance's
        schedule: (B, m, n_tab, ...)."""
        m, N = gk.shape[1], self.ocp.N
        tab = np.asarray(self.ocp.tab)
        tab = tab[None, :] if tab.ndim == 1 else tab
        tab = np.broadcast_to(tab, (B, N)) if tab.shape[0] == 1 else tab[:B]
        acc = np.zeros((B, m, self.ocp.n_tab) + gk.shape[3:])
        bi = np.broadcast_to(np.arange(B)[:, None], (B, N))
        np.add.at(acc, (bi[:, None, :], np.arange(m)[None, :, None], tab[:, None, :]), gk)
        return acc

    def _with_bounds(self, B, lbw, ubw, per_instance, call):
        """Run call(lbw, ubw) with (B, n_w) bounds installed as device bounds for its duration, as
        ``solve_batch`` does (then whatever was installed before is put back); otherwise as given."""
        if not per_instance:
            return call(lbw, ubw)
        import torch  # device memory comes from PyTorch, as in mpcx.device

        dev = torch.device("cuda", self._h.spec.device)
        before = self._dev_bounds
        self._install_bounds((torch.from_numpy(lbw).to(dev), torch.from_numpy(ubw).to(dev), B, 1),
                             torch.cuda.current_stream(dev).cuda_stream)
        try:
            return call(None, None)
        finally:  # (the host-pointer calls wait for their results)
            self._install_bounds(before)

    def sens_bounds(self, P, res, dlbw, dubw, lbw=None, ubw=None):
        """Directional sensitivities of the solutions ``res`` to the box bounds (mpcx_sens_bounds):
        dw = (d w*/d lbw) dlbw + (d w*/d ubw) dubw, no solve, every model.

        dlbw / dubw: (B, m, n_w) directions of the lower / upper bounds, each shaped like a row of w, or
        (B, n_w) for a single one; either may be None (zeros).  Any m (launches of at most nx columns
        each; a column's bits do not depend on the others).  Entries on X_0 and where the bound is not
        finite are ignored.
        lbw / ubw: the bounds the solve used -- None (the problem's, or installed device bounds), a
        scalar or n_w entries shared by the batch, or (B, n_w) arrays with one row per instance
        (installed as device bounds for this call, as ``solve_batch`` does).
        Returns {'dw': (B, n_w, m), 'flag': (B,)}: w(lbw + dlbw, ubw + dubw) ~ w + dw; a strictly active
        variable moves with its bound, an inactive bound has an O(mu) effect.  flag 1 marks an
        irregular instance (NaN outputs), as :meth:`sens_x0`.  These are barrier-problem sensitivities
        with the one-sided multiplier split of include/mpcx.h (mpcx_sens_bounds)."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_bounds: multiple-shooting layout only (bounds are given on its w)")
        B, point, bounds = self._sens_point(P, res, lbw, ubw)
        if dlbw is None and dubw is None:
            raise ValueError("sens_bounds: at least one of dlbw / dubw must be given")
        d = [None if v is None else self._sens_cols(v, B, name) for v, name in ((dlbw, "dlbw"), (dubw, "dubw"))]
        if d[0] is not None and d[1] is not None and d[0].shape != d[1].shape:
            sl, su = (v.shape[:2] + (self._ms_nw,) for v in d)  # (as given: the problem's own layout)
            raise ValueError(f"dlbw {sl} and dubw {su}: the same number of directions expected")
        d = [np.zeros_like(d[1 - i]) if v is None else v for i, v in enumerate(d)]
        (dw,), flag = self._sens_launches("mpcx_sens_bounds", B, point, bounds, d, (), [(2, (B, self._kdims[0]))])
        if self._pad is not None:  # the model's own states and inputs only
            dw = dw[:, self._pad.w_idx]
        return {"dw": np.ascontiguousarray(dw), "flag": flag}

    def sens_bounds_vjp(self, P, res, gw, lbw=None, ubw=None):
        """Reverse mode of :meth:`sens_bounds` (mpcx_sens_bounds_vjp): the gradients with respect to every
        entry of lbw and ubw of a scalar loss whose gradient on the solution w is gw, from one launch:
        <gw, sens_bounds(dlbw, dubw)> = <glbw, dlbw> + <gubw, dubw>.

        gw: (B, m, n_w) cotangents or (B, n_w) for a single one; any m (launches of at most nx each).
        lbw / ubw: as for :meth:`sens_bounds`.
        Returns {'glbw': (B, m, n_w), 'gubw': (B, m, n_w), 'flag': (B,)}; the entries on X_0 and where
        there is no finite bound are 0; flag 1 marks an irregular instance (NaN outputs)."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_bounds_vjp: multiple-shooting layout only (bounds are given on its w)")
        B, point, bounds = self._sens_point(P, res, lbw, ubw)
        gw = self._sens_cols(gw, B, "gw")
        nw = self._kdims[0]
        (gl, gu), flag = self._sens_launches("mpcx_sens_bounds_vjp", B, point, bounds, [gw], (),
                                             [(1, (B, nw)), (1, (B, nw))])
        if self._pad is not None:  # the model's own states and inputs only
            gl, gu = gl[:, :, self._pad.w_idx], gu[:, :, self._pad.w_idx]
        return {"glbw": np.ascontiguousarray(gl), "gubw": np.ascontiguousarray(gu), "flag": flag}

    def set_weights(self, Q, R):
        """Replace the diagonal cost weights Q (nx) and R (nu) of the problem (mpcx_set_weights; not for
        linear models, whose weights are their tables): every later solve and sensitivity call uses them,
        bit for bit as a solver created with these weights would."""
        if self.ocp.model == "linear":
            raise ValueError("set_weights: a linear model's weights are its tables (set_linear_model)")
        self._h.set_weights(Q, R)
        self.ocp = dataclasses.replace(self.ocp, Q=tuple(float(v) for v in np.ravel(Q)),
                                       R=tuple(float(v) for v in np.ravel(R)))

    def _wt_sel(self):
        """Where the entries of the problem's own packed W lie in the kernel's packed weight row."""
        nz = self.ocp.nx + self.ocp.nu
        pd = self._pad
        nzk = nz if pd is None else pd.nxp + self.ocp.nu
        ix = np.arange(nz) if pd is None else np.r_[np.arange(self.ocp.nx), pd.nxp + np.arange(self.ocp.nu)]
        iu = np.triu_indices(nz)
        a, b = ix[iu[0]], ix[iu[1]]
        return a * nzk - a * (a - 1) // 2 + (b - a), nzk * (nzk + 1) // 2

    def _weight_rows(self, B, dQ, dR, dW):
        """The directions of :meth:`sens_weights` as (B, m, N or 1, n_wt) in the kernel's layout."""
        lin = self.ocp.model == "linear"
        if lin != (dW is not None) or (lin and (dQ is not None or dR is not None)):
            raise ValueError("sens_weights: dW for a linear model, dQ / dR for the others")
        N = self.ocp.N

        def rows(v, n, name):
            v = np.asarray(v, np.float64)
            if v.ndim == 2:
                v = v[:, None, None, :]
            elif v.ndim == 3:
                v = v[:, :, None, :]
            if v.ndim != 4 or v.shape[0] != B or v.shape[1] < 1 or v.shape[2] not in (1, N) or v.shape[3] != n:
                raise ValueError(f"{name}: expected ({B}, {n}), ({B}, m, {n}) or ({B}, m, {N}, {n}), got {v.shape}")
            return v

        if lin:
            sel, n_k = self._wt_sel()
            v = rows(dW, sel.size, "dW")
            d = np.zeros(v.shape[:3] + (n_k,))
            d[..., sel] = v
            return d
        if dQ is None and dR is None:
            raise ValueError("sens_weights: at least one of dQ / dR must be given")
        q = None if dQ is None else rows(dQ, self.ocp.nx, "dQ")
        r = None if dR is None else rows(dR, self.ocp.nu, "dR")
        q = np.zeros(r.shape[:3] + (self.ocp.nx,)) if q is None else q
        r = np.zeros(q.shape[:3] + (self.ocp.nu,)) if r is None else r
        if q.shape[:2] != r.shape[:2]:
            raise ValueError(f"dQ {q.shape} and dR {r.shape}: the same number of directions expected")
        if q.shape[2] != r.shape[2]:  # one of them per stage: the other repeated
            q, r = (np.broadcast_to(v, v.shape[:2] + (N,) + v.shape[3:]) for v in (q, r))
        return np.concatenate([q, r], axis=3)

    def sens_weights(self, P, res, dQ=None, dR=None, dW=None, lbw=None, ubw=None):
        """Directional sensitivities of the solutions ``res`` to the cost weights (mpcx_sens_weights):
        dw = (d w*/d weights) d(weights), no solve, every model.

        dQ / dR (the unicycle and the ODE models): directions of the diagonal weights, (B, nx) / (B, nu)
        for a single one, (B, m, nx) / (B, m, nu) for m of them used at every stage, or per stage
        (B, m, N, nx) / (B, m, N, nu); either may be None (zeros).
        dW (linear models): the same shapes with the packed upper triangle (``lti.pack_sym``) of a
        symmetric direction of the stage table in the problem's own (x, u) in place of the rows.
        Any m (launches of at most nx columns each; a column's bits do not depend on the others).
        lbw / ubw: as for :meth:`sens_bounds`.
        Returns {'dw': (B, n_w, m), 'flag': (B,)}: w(weights + d) ~ w + dw (the X_0 rows are exact
        zeros); flag 1 marks an irregular instance (NaN outputs), as :meth:`sens_x0`.  Barrier-problem
        sensitivities (include/mpcx.h, mpcx_sens_weights)."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_weights: multiple-shooting layout only")
        B, point, bounds = self._sens_point(P, res, lbw, ubw)
        return self._sens_stage_rows("mpcx_sens_weights", B, point, bounds, self._weight_rows(B, dQ, dR, dW))

    def sens_weights_vjp(self, P, res, gw, lbw=None, ubw=None):
        """Reverse mode of :meth:`sens_weights` (mpcx_sens_weights_vjp): the gradients with respect to the
        cost weights of a scalar loss whose gradient on the solution w is gw, from one launch:
        <gw, sens_weights(per-stage d)> = <gQk, dQ> + <gRk, dR>  (linear models: <gWk, dW>).

        gw: (B, m, n_w) cotangents or (B, n_w) for a single one; any m (launches of at most nx each).
        lbw / ubw: as for :meth:`sens_bounds`.
        Returns 'flag' (B,) and, for the unicycle and the ODE models, 'gQk' (B, m, N, nx), 'gRk'
        (B, m, N, nu) per stage and their sums over the stages 'gQ' (B, m, nx), 'gR' (B, m, nu): the
        gradient with respect to the problem's Q, R.  For linear models 'gWk' (B, m, N, nz (nz + 1) / 2),
        packed as dW of :meth:`sens_weights`, and 'gW' (B, m, n_tab, .): the stages' rows summed per
        table through the instance's schedule.  NaN outputs where flag is 1."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_weights_vjp: multiple-shooting layout only")
        B, m, gk, gs, flag = self._sens_stage_vjp("mpcx_sens_weights_vjp", P, res, gw, lbw, ubw, self._h.weight_dims())
        if self.ocp.model != "linear":
            nx = self.ocp.nx
            return {"gQ": np.ascontiguousarray(gs[..., :nx]), "gR": np.ascontiguousarray(gs[..., nx:]),
                    "gQk": np.ascontiguousarray(gk[..., :nx]), "gRk": np.ascontiguousarray(gk[..., nx:]), "flag": flag}
        sel, _ = self._wt_sel()
        gk = np.ascontiguousarray(gk[..., sel])
        return {"gWk": gk, "gW": self._sum_by_table(B, gk), "flag": flag}

    def set_par(self, par):
        """Replace the constants ``par`` of an ODE model (mpcx_set_par; not for linear models, whose constants
        are their tables, nor the unicycle, which has none): every later solve and sensitivity call uses them,
        bit for bit as a solver created with these constants would."""
        if self.ocp.model == "linear":
            raise ValueError("set_par: a linear model's constants are its tables (set_linear_model)")
        if self.ocp.model == "unicycle":
            raise ValueError("set_par: the unicycle has no model constants")
        par = tuple(float(v) for v in np.ravel(par))
        self._h.set_par(par)
        self.ocp = dataclasses.replace(self.ocp, par=par)

    def _model_dims(self):
        """(nx of the kernel's layout, nu, entries of the kernel's model row)."""
        knx = self.ocp.nx if self._pad is None else self._pad.nxp
        return knx, self.ocp.nu, self._h.model_dims()

    def _model_rows(self, B, dpar, dA, dB, dc):
        """The directions of :meth:`sens_model` as (B, m, N or 1, n_th) in the kernel's layout."""
        if self.ocp.model == "unicycle":
            raise ValueError("sens_model: the unicycle has no model constants")
        lin = self.ocp.model == "linear"
        if lin != (dpar is None) or (not lin and any(v is not None for v in (dA, dB, dc))):
            raise ValueError("sens_model: dA / dB / dc for a linear model, dpar for the ODE models")
        N, nx, nu = self.ocp.N, self.ocp.nx, self.ocp.nu
        knx, _, n_th = self._model_dims()

        def rows(v, tail, name):
            v = np.asarray(v, np.float64)
            lead = v.ndim - len(tail)
            if lead == 1:
                v = v[:, None, None]
            elif lead == 2:
                v = v[:, :, None]
            if v.ndim != 3 + len(tail) or v.shape[0] != B or v.shape[1] < 1 or v.shape[2] not in (1, N) \
                    or v.shape[3:] != tail:
                raise ValueError(f"{name}: expected ({B},) + {tail}, ({B}, m) + {tail} or ({B}, m, {N}) + {tail}, "
                                 f"got {v.shape}")
            return v

        if not lin:
            return np.ascontiguousarray(rows(dpar, (n_th,), "dpar"))
        if dA is None and dB is None and dc is None:
            raise ValueError("sens_model: at least one of dA / dB / dc must be given")
        parts = [None if v is None else rows(v, t, n) for v, t, n in
                 ((dA, (nx, nx), "dA"), (dB, (nx, nu), "dB"), (dc, (nx,), "dc"))]
        given = [p for p in parts if p is not None]
        m = given[0].shape[1]
        if any(p.shape[1] != m for p in given):
            raise ValueError("dA / dB / dc: the same number of directions expected")
        S = max(p.shape[2] for p in given)  # one of them per stage: the others repeated
        d = np.zeros((B, m, S, n_th))
        A = d[..., :knx * knx].reshape(B, m, S, knx, knx)
        Bm = d[..., knx * knx:knx * knx + knx * nu].reshape(B, m, S, knx, nu)
        c = d[..., knx * knx + knx * nu:]
        if parts[0] is not None:
            A[..., :nx, :nx] = parts[0]
        if parts[1] is not None:
            Bm[..., :nx, :] = parts[1]
        if parts[2] is not None:
            c[..., :nx] = parts[2]
        return d

    def sens_model(self, P, res, dpar=None, dA=None, dB=None, dc=None, lbw=None, ubw=None):
        """Directional sensitivities of the solutions ``res`` to the model (mpcx_sens_model):
        dw = (d w*/d model) d(model), no solve; every model but the unicycle, which has no constants.

        dpar (the ODE models): directions of the constants the model reads (``par``: n_th entries), (B, n_th)
        for a single one, (B, m, n_th) for m of them used at every stage, or per stage (B, m, N, n_th).
        dA / dB / dc (linear models): directions of the stage tables in the problem's own (x, u), with
        (nx, nx) / (nx, nu) / (nx,) in place of the row; any of them may be None (zeros); shared by the
        stages or one per stage.  Any m (launches of at most nx columns each; a column's bits do not depend
        on the others).  lbw / ubw: as for :meth:`sens_bounds`.
        Returns {'dw': (B, n_w, m), 'flag': (B,)}: w(model + d) ~ w + dw (the X_0 rows are exact zeros);
        flag 1 marks an irregular instance (NaN outputs), as :meth:`sens_x0`.  Barrier-problem
        sensitivities (include/mpcx.h, mpcx_sens_model)."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_model: multiple-shooting layout only")
        if self.ocp.model == "unicycle":
            raise ValueError("sens_model: the unicycle has no model constants")
        B, point, bounds = self._sens_point(P, res, lbw, ubw)
        return self._sens_stage_rows("mpcx_sens_model", B, point, bounds, self._model_rows(B, dpar, dA, dB, dc))

    def sens_model_vjp(self, P, res, gw, lbw=None, ubw=None):
        """Reverse mode of :meth:`sens_model` (mpcx_sens_model_vjp): the gradients with respect to the model
        of a scalar loss whose gradient on the solution w is gw, from one launch:
        <gw, sens_model(per-stage d)> = <gpark, dpar>  (linear models: <gAk, dA> + <gBk, dB> + <gck, dc>).

        gw: (B, m, n_w) cotangents or (B, n_w) for a single one; any m (launches of at most nx each).
        lbw / ubw: as for :meth:`sens_bounds`.
        Returns 'flag' (B,) and, for the ODE models, 'gpark' (B, m, N, n_th) per stage and their sum over
        the stages 'gpar' (B, m, n_th): the gradient with respect to the problem's ``par``.  For linear
        models 'gAk' (B, m, N, nx, nx), 'gBk' (B, m, N, nx, nu), 'gck' (B, m, N, nx) and 'gA', 'gB', 'gc'
        (B, m, n_tab, ...): the stages' rows summed per table through the instance's schedule.  NaN
        outputs where flag is 1."""
        if self.ocp.formulation == "single_shooting":
            raise ValueError("sens_model_vjp: multiple-shooting layout only")
        if self.ocp.model == "unicycle":
            raise ValueError("sens_model_vjp: the unicycle has no model constants")
        knx, nu, n_th = self._model_dims()
        B, m, gk, gs, flag = self._sens_stage_vjp("mpcx_sens_model_vjp", P, res, gw, lbw, ubw, n_th)
        if self.ocp.model != "linear":
            return {"gpar": gs, "gpark": gk, "flag": flag}
        nx, N = self.ocp.nx, self.ocp.N
        gAk = np.ascontiguousarray(gk[..., :knx * knx].reshape(B, m, N, knx, knx)[..., :nx, :nx])
        gBk = np.ascontiguousarray(gk[..., knx * knx:knx * knx + knx * nu].reshape(B, m, N, knx, nu)[..., :nx, :])
        gck = np.ascontiguousarray(gk[..., knx * knx + knx * nu:][..., :nx])
        out = {"gAk": gAk, "gBk": gBk, "gck": gck, "flag": flag}
        for name, v in (("gA", gAk), ("gB", gBk), ("gc", gck)):  # summed over the schedule, as gW is
            out[name] = self._sum_by_table(B, v)
        return out

    def rk4_sens(self, w, P):
        """Per-interval defects, costs and Jacobians at w (B, n_w) -- the sweep kernel."""
        if self.ocp.model != "unicycle":
            raise ValueError("rk4_sens: the sweep kernel evaluates the unicycle model only")
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(w, np.float64)))
        P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, np.float64)))
        B, N = w.shape[0], self.ocp.N
        if w.shape[1] != self._h.n_w or P.shape != (B, self._h.n_p):
            raise ValueError(f"rk4_sens: w (B, {self._h.n_w}) and P (B, {self._h.n_p}) expected")
        c = np.empty((B, N, 3))
        q = np.empty((B, N))
        A = np.empty((B, N, 3, 3))
        Bm = np.empty((B, N, 3, 2))
        gq = np.empty((B, N, 5))
        _lib.check(_lib.load().mpcx_rk4_sens(self._h.ptr, B, _lib.dptr(w), _lib.dptr(P), _lib.dptr(c), _lib.dptr(q),
                                             _lib.dptr(A), _lib.dptr(Bm), _lib.dptr(gq)))
        return {"c": c, "q": q, "A": A, "B": Bm, "gq": gq}

    def lam_x_from_kkt(self, w, P, lam_g):
        """Bound multipliers reconstructed from stationarity, grad f + J^T lam_g + lam_x = 0
        (evaluated with the sweep kernel; used to cross-check the solver's own lam_x).  Interval 0
        integrates from x0 = P[:3] (multiple_shooting_casadi.py:125,157), so X_0 enters only g_0."""
        we = np.array(np.atleast_2d(w), np.float64)
        P2 = np.atleast_2d(np.asarray(P, np.float64))
        we[:, 0:3] = P2[:, 0:3]  # the sweep evaluates interval 0 at (x0, U_0)
        s = self.rk4_sens(we, P2)
        B, N = s["q"].shape
        r = np.zeros((B, self._h.n_w))
        lam_g = np.asarray(lam_g).reshape(B, -1)
        ix = lambda k: np.arange(3) if k == 0 else 3 + 5 * (k - 1) + 2 + np.arange(3)  # noqa: E731
        r[:, 0:3] -= lam_g[:, 0:3]
        for k in range(N):
            l1 = lam_g[:, 3 * (k + 1):3 * (k + 2)]
            if k > 0:
                r[:, ix(k)] += s["gq"][:, k, 0:3] + np.einsum("bij,bi->bj", s["A"][:, k], l1)
            r[:, 3 + 5 * k:5 + 5 * k] += s["gq"][:, k, 3:5] + np.einsum("bij,bi->bj", s["B"][:, k], l1)
            r[:, ix(k + 1)] -= l1
        return -r

    # ---------------------------------------------------------------- CasADi-shaped call
    def __call__(self, x0=None, lbx=None, ubx=None, lbg=None, ubg=None, p=None, lam_x0=None, lam_g0=None):
        if p is None:
            raise ValueError("p is required")
        ocp = self.ocp
        P = _vec(p, self.n_p, "p")[None, :]
        ss = ocp.formulation == "single_shooting"
        lbx = _vec(lbx, self.n_w, "lbx", -math.inf)
        ubx = _vec(ubx, self.n_w, "ubx", math.inf)
        lbg = _vec(lbg, self.n_g, "lbg", 0.0 if not ss else -math.inf)
        ubg = _vec(ubg, self.n_g, "ubg", 0.0 if not ss else math.inf)
        if ss and ocp.model == "linear":
            raise ValueError("single shooting is mapped for the unicycle and ODE models (stage-invariant dynamics)")
        if ss:
            if np.any(np.isfinite(lbg)) or np.any(np.isfinite(ubg)):
                raise ValueError("single shooting: only inactive (+-inf) bounds on g are supported")
        elif np.any(lbg != 0) or np.any(ubg != 0):
            raise ValueError("multiple shooting: g are the shooting equalities, lbg = ubg = 0 required")
        N, nx, nu = ocp.N, ocp.nx, ocp.nu
        nz = nx + nu
        l0 = lx0 = None
        if ss:  # decision = U; bounds on U map onto the U slots of the multiple-shooting w
            lbw = np.full(self._h.n_w, -1e20)
            ubw = np.full(self._h.n_w, 1e20)
            for k in range(N):
                lbw[nx + nz * k:nx + nz * k + nu] = lbx[nu * k:nu * (k + 1)]
                ubw[nx + nz * k:nx + nz * k + nu] = ubx[nu * k:nu * (k + 1)]
            w0 = None
            if x0 is not None:
                U = _vec(x0, nu * N, "x0").reshape(N, nu)
                X = self._rollout(P[0], U)
                w0 = np.concatenate([X[0]] + [np.concatenate([U[k], X[k + 1]]) for k in range(N)])[None, :]
        else:
            lbw, ubw = lbx, ubx
            w0 = None if x0 is None else _vec(x0, self.n_w, "x0")[None, :]
            l0 = None if lam_g0 is None else _vec(lam_g0, self.n_g, "lam_g0")[None, :]
            lx0 = None if lam_x0 is None else _vec(lam_x0, self.n_w, "lam_x0")[None, :]
        lbw = np.where(np.isfinite(lbw), lbw, -1e20)
        ubw = np.where(np.isfinite(ubw), ubw, 1e20)
        r = self.solve_batch(P, w0, np.ascontiguousarray(lbw), np.ascontiguousarray(ubw), want_lam=True,
                             want_g=True, lam_g0=l0, lam_x0=lx0)
        st = int(r["status"][0])
        self._stats = {"return_status": _lib.STATUS.get(st, str(st)), "success": st <= 1,
                       "iter_count": int(r["iters"][0]), "t_wall_total": r["t_wall"], "status_code": st}
        w = r["w"][0]
        lam_x = r["lam_x"][0]
        if ss:
            U = np.stack([w[nx + nz * k:nx + nz * k + nu] for k in range(N)]).reshape(-1)
            Xs = np.stack([w[nx + nz * k + nu:nx + nz * (k + 1)] for k in range(N)])
            g = Xs[:, 0:self._ss_ng].reshape(-1)
            lx = np.concatenate([lam_x[nx + nz * k:nx + nz * k + nu] for k in range(N)])
            return {"x": U[:, None], "f": np.array([[r["f"][0]]]), "g": g[:, None],
                    "lam_g": np.zeros((self.n_g, 1)), "lam_x": lx[:, None], "lam_p": np.zeros((self.n_p, 1))}
        return {"x": w[:, None], "f": np.array([[r["f"][0]]]), "g": r["g"][0][:, None],
                "lam_g": r["lam_g"][0][:, None], "lam_x": lam_x[:, None], "lam_p": np.zeros((self.n_p, 1))}

    def _rollout(self, P, U):
        """X_{k+1} = F(X_k, U_k) on the plant kernel, stage k's references in the stage-0 slot."""
        N, nx, nz = self.ocp.N, self.ocp.nx, self.ocp.nx + self.ocp.nu
        X = [np.asarray(P[0:nx], float)]
        F = Integrator(self.ocp, handle=self._h)
        for k in range(N):
            p = np.array(P, float).copy()
            p[0:nx] = X[-1]
            if self.ocp.param == "x0_stageref":
                p[nx:nx + nz] = P[nx + nz * k:nx + nz * (k + 1)]
            X.append(F(p, U[k])[0].reshape(-1))
        return np.array(X)


class Integrator:
    """``F = ca.Function('F', [P, U], [X, Q], ['x0','p'], ['xf','qf'])`` (:114).

    For a LinearOCP this is stage 0's map x+ = A_j x + B_j u + c_j, q = l_0 (the
    reference's discrete ``f``, e.g. ``inverted_pendulum...py:24-28``).

    ``F(p, u)`` -> [xf (3,1), qf (1,1)];  ``F(x0=p, p=u)`` -> {'xf', 'qf'};
    ``F.batch(P, U)`` -> (xf (B,3), qf (B,)).  Evaluated by the plant kernel.
    """

    def __init__(self, ocp: OCP, device: int = 0, handle=None):
        self.ocp = ocp
        self._pad = state_pad(ocp)
        kocp = self._pad.ocp if self._pad else ocp
        self._h = handle if handle is not None else _lib.Handle(to_spec(kocp, device=device))
        if handle is None and ocp.model == "linear":
            self._h.set_linear_model(kocp)

    @property
    def n_p(self):
        return self._pad.n_p if self._pad else self._h.n_p

    def batch(self, P, U):
        P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, np.float64)))
        U = np.ascontiguousarray(np.atleast_2d(np.asarray(U, np.float64)))
        B = P.shape[0]
        nx, nu = self.ocp.nx, self.ocp.nu
        if P.shape[1] != self.n_p:
            raise ValueError(f"P must be (B, {self.n_p})")
        if U.shape != (B, nu):
            raise ValueError(f"U must be (B, {nu})")
        pd = self._pad
        if pd is not None:
            P = pd.scatter(P, pd.p_idx, pd.n_p_pad)
        xf = np.empty((B, pd.nxp if pd else nx))
        qf = np.empty(B)
        _lib.check(_lib.load().mpcx_plant_step(self._h.ptr, B, _lib.dptr(P), _lib.dptr(U), _lib.dptr(xf),
                                               _lib.dptr(qf)))
        return np.ascontiguousarray(xf[:, :nx]), qf

    def __call__(self, *args, **kw):
        if kw:
            p = kw.get("x0")
            u = kw.get("p")
            xf, qf = self.batch(_vec(p, self.n_p, "x0")[None, :], _vec(u, self.ocp.nu, "p")[None, :])
            return {"xf": xf[0][:, None], "qf": qf[:, None]}
        p, u = args
        xf, qf = self.batch(_vec(p, self.n_p, "p")[None, :], _vec(u, self.ocp.nu, "u")[None, :])
        return [xf[0][:, None], qf[:, None]]


def nlpsol(name: str, plugin: str, prob: OCP, opts: dict | None = None, device: int = 0) -> Solver:
    """Create a solver (``ca.nlpsol`` signature).  plugin must be 'mi355x'."""
    if plugin not in ("mi355x",):
        raise ValueError(f"unknown plugin {plugin!r} (available: 'mi355x')")
    if not isinstance(prob, (OCP, LinearOCP, OdeOCP)):
        raise TypeError("prob must be an mpcx.OCP, LinearOCP or OdeOCP (symbolic CasADi problems are not supported)")
    return Solver(name, prob, opts, device)


def integrator(ocp: OCP, device: int = 0) -> Integrator:
    return Integrator(ocp, device)
