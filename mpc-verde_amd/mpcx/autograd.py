"""The batched MPC solve as a differentiable PyTorch function (reverse mode).

``solve_differentiable(loop, P)`` solves the loop's B problems at the parameter rows P and returns
the solutions w (B, n_w) as a tensor that carries a backward: for a scalar loss L(w), ``P.grad`` is
(dw*/dP)^T dL/dw, from ONE adjoint-sensitivity launch (``DeviceLoop.sens_vjp``, mpcx_sens_vjp_dev) on
the loop's stream -- no solve, no host synchronisation, every entry of the row at once::

    loop = DeviceLoop(solver, P0)
    P = torch.tensor(P0, device="cuda", requires_grad=True)
    w = solve_differentiable(loop, P)
    loss = 0.5 * ((w[:, nx:nx + nu] - u_target) ** 2).sum()      # imitation loss on the first move
    loss.backward()                                              # P.grad: (B, n_p)

PyTorch provides the tensors, streams and the autograd graph only; the arithmetic is libmpcx's HIP
kernels.  Layouts are the kernel's, as for the other ``DeviceLoop`` methods (a padded linear model:
its pad entries included).  These are the sensitivities of the barrier problem at the returned
multipliers (include/mpcx.h, mpcx_sens_x0).
"""
from __future__ import annotations

import contextlib

import torch

from .device import DeviceLoop

__all__ = ["MPCFunction", "MPCBoundsFunction", "MPCWeightsFunction", "MPCParFunction", "solve_differentiable"]


@contextlib.contextmanager
def _on_loop_stream(loop):
    """The body runs with the loop's stream current, ordered after the work queued so far on the caller's
    stream, which in turn is ordered after the body's work (device-side ordering only: nothing waits on
    the host)."""
    cur = torch.cuda.current_stream(loop.device)
    loop.stream.wait_stream(cur)
    with torch.cuda.stream(loop.stream):
        yield
    cur.wait_stream(loop.stream)


def _forward(ctx, P, loop, zero_irregular, *also_saved):
    """The four classes' forward, on the loop's stream: copies P into the loop, enqueues ``loop.solve()``,
    saves copies of the point (P, w, lam, lamx), then ``also_saved``, and returns a copy of w."""
    loop.P.copy_(P.detach(), non_blocking=True)
    loop.solve()
    point = tuple(t.clone() for t in (loop.P, loop.w, loop.lam, loop.lamx))
    ctx.loop, ctx.zero_irregular = loop, zero_irregular
    ctx.save_for_backward(*point, *also_saved)
    return point[1].clone()


def _backward(ctx, gw, point, own=None):
    """The four classes' backward, on the loop's stream, with dL/dw as the one cotangent: own(g) makes
    the class's own launch and returns (*rows, flag), rows being (B, .) gradients; ``loop.sens_vjp`` is
    launched for P's rows when there is no own launch or P requires a gradient.  The rows of an
    instance flagged irregular are zeroed if the forward asked for it.  Returns (gP or None, rows)."""
    g = gw.detach().to(torch.float64).contiguous().unsqueeze(1)  # one cotangent: m = 1
    rows, flag, gP = [], None, None
    if own is not None:
        *rows, flag = own(g)
    if own is None or ctx.needs_input_grad[0]:
        gP, flag_p = ctx.loop.sens_vjp(g, point=point)  # (the same factors: the same flag)
        gP, flag = gP[:, 0], flag_p if flag is None else flag
    if ctx.zero_irregular:
        bad = flag[:, None] != 0
        rows = [torch.where(bad, torch.zeros_like(t), t) for t in rows]
        if gP is not None:
            gP = torch.where(bad, torch.zeros_like(gP), gP)
    return gP, rows


class MPCFunction(torch.autograd.Function):
    """forward(P, loop, zero_irregular): copies P into the loop, enqueues ``loop.solve()`` and returns a
    copy of w; the point (P, w, lam, lamx) is saved as copies, so later solves of the same loop do not
    move it.  backward: one ``loop.sens_vjp`` launch at the saved point with dL/dw as the cotangent."""

    @staticmethod
    def forward(ctx, P, loop, zero_irregular):
        with _on_loop_stream(loop):
            return _forward(ctx, P, loop, zero_irregular)

    @staticmethod
    def backward(ctx, gw):
        with _on_loop_stream(ctx.loop):
            gP, _ = _backward(ctx, gw, ctx.saved_tensors)
        return gP, None, None


class MPCBoundsFunction(torch.autograd.Function):
    """forward(P, lbw, ubw, loop, zero_irregular): installs copies of the per-instance bounds
    (``loop.set_bounds``), then as :class:`MPCFunction`.  backward: one ``loop.sens_bounds_vjp`` launch at
    the saved point for ``lbw.grad`` / ``ubw.grad`` and, only when P requires a gradient, one
    ``loop.sens_vjp`` launch for ``P.grad`` (so a model without ``sens_vjp``, the path-frame bicycle,
    works with bounds gradients alone).  The backward differentiates at the forward's bounds: the
    copies stay installed after the forward, and when the loop's installed bounds are no longer those
    copies they are installed again for the launches and what was there is put back.

    Host synchronisation: ``set_bounds`` validates the tensors on the loop's stream and waits for the
    verdict, so the forward waits once for the stream, and the backward twice more only when it has to
    re-install (once for the copies, once to put the others back).  The launches themselves never wait."""

    @staticmethod
    def forward(ctx, P, lbw, ubw, loop, zero_irregular):
        with _on_loop_stream(loop):
            lb, ub = lbw.detach().clone(), ubw.detach().clone()
            loop.set_bounds(lb, ub)
            ctx.state = loop.solver._dev_bounds
            return _forward(ctx, P, loop, zero_irregular, lb, ub)

    @staticmethod
    def backward(ctx, gw):
        loop = ctx.loop
        *point, lb, ub = ctx.saved_tensors
        before = loop.solver._dev_bounds
        moved = before is not ctx.state
        if moved:  # the forward's bounds, for the launches below
            loop.set_bounds(lb, ub)

        def own(g):
            gl, gu, flag = loop.sens_bounds_vjp(g, point=point)
            gl, gu = gl[:, 0], gu[:, 0]
            pd = getattr(loop.solver, "_pad", None)
            if pd is not None:  # the bounds were given in the model's own layout
                idx = torch.from_numpy(pd.w_idx).to(loop.device)
                gl, gu = gl[:, idx], gu[:, idx]
            return gl, gu, flag

        with _on_loop_stream(loop):
            try:
                gP, (gl, gu) = _backward(ctx, gw, point, own)
            finally:
                if moved:  # (stream-ordered after the launches; the validation waits for the stream)
                    loop.solver._install_bounds(before, loop.stream.cuda_stream if before is not None else None)
        return gP, gl if ctx.needs_input_grad[1] else None, gu if ctx.needs_input_grad[2] else None, None, None


class MPCWeightsFunction(torch.autograd.Function):
    """forward(P, Q, R, loop, zero_irregular): sets the solver's diagonal cost weights from the values of
    the tensors Q (nx,) and R (nu,), shared by the batch (``Solver.set_weights``; they stay set), then as
    :class:`MPCFunction`.  backward: one ``loop.sens_weights_vjp`` launch at the saved point; ``Q.grad`` /
    ``R.grad`` are its stage sums added over the batch (an instance flagged irregular puts NaN into the
    sum unless irregular="zero" drops its row).  Only when P requires a gradient, one ``loop.sens_vjp``
    launch for ``P.grad`` (so a model without ``sens_vjp``, the path-frame bicycle, works with weight
    gradients alone).  The backward differentiates at the forward's weights: when the solver's weights
    are no longer those, they are set for the launches and the others are put back.

    Host synchronisation: the forward reads the values of Q and R on the host (one device-to-host copy,
    which waits for the work that produces them), because the weights are launch arguments, not device
    memory.  Nothing else waits; the backward's launches never do."""

    @staticmethod
    def forward(ctx, P, Q, R, loop, zero_irregular):
        q, r = (tuple(float(v) for v in t.detach().cpu().tolist()) for t in (Q, R))  # (the one host read)
        loop.solver.set_weights(q, r)
        ctx.weights = (q, r)
        with _on_loop_stream(loop):
            return _forward(ctx, P, loop, zero_irregular)

    @staticmethod
    def backward(ctx, gw):
        loop, solver = ctx.loop, ctx.loop.solver
        point = ctx.saved_tensors
        before = (tuple(solver.ocp.Q), tuple(solver.ocp.R))
        moved = before != ctx.weights
        if moved:  # the forward's weights, for the launches below (launch arguments: taken at the call)
            solver.set_weights(*ctx.weights)
        nx = solver.ocp.nx

        def own(g):
            _, gs, flag = loop.sens_weights_vjp(g, point=point, per_stage=False)
            return gs[:, 0], flag

        with _on_loop_stream(loop):
            try:
                gP, (gs,) = _backward(ctx, gw, point, own)
                gs = gs.sum(dim=0)
                gQ, gR = gs[:nx].contiguous(), gs[nx:].contiguous()
            finally:
                if moved:
                    solver.set_weights(*before)
        return gP, gQ if ctx.needs_input_grad[1] else None, gR if ctx.needs_input_grad[2] else None, None, None


class MPCParFunction(torch.autograd.Function):
    """forward(P, par, loop, zero_irregular): sets the constants of the solver's ODE model from the values of
    the tensor par (n_th,), shared by the batch (``Solver.set_par``; they stay set), then as
    :class:`MPCFunction`.  backward: one ``loop.sens_model_vjp`` launch at the saved point; ``par.grad`` is its
    stage sum added over the batch (an instance flagged irregular puts NaN into the sum unless
    irregular="zero" drops its row).  Only when P requires a gradient, one ``loop.sens_vjp`` launch for
    ``P.grad`` (so the path-frame bicycle, which has no ``sens_vjp``, works with ``par.grad`` alone).  The
    backward differentiates at the forward's constants: when the solver's are no longer those, they are
    set for the launches and the others are put back.

    Host synchronisation: the forward reads the values of par on the host (one device-to-host copy), because
    the constants are launch arguments, not device memory.  Nothing else waits."""

    @staticmethod
    def forward(ctx, P, par, loop, zero_irregular):
        pv = tuple(float(v) for v in par.detach().cpu().tolist())  # (the one host read)
        loop.solver.set_par(pv)
        ctx.par = pv
        with _on_loop_stream(loop):
            return _forward(ctx, P, loop, zero_irregular)

    @staticmethod
    def backward(ctx, gw):
        loop, solver = ctx.loop, ctx.loop.solver
        point = ctx.saved_tensors
        before = tuple(float(v) for v in solver.ocp.par)
        moved = before != ctx.par
        if moved:  # the forward's constants, for the launches below (launch arguments: taken at the call)
            solver.set_par(ctx.par)

        def own(g):
            _, gs, flag = loop.sens_model_vjp(g, point=point, per_stage=False)
            return gs[:, 0], flag

        with _on_loop_stream(loop):
            try:
                gP, (gs,) = _backward(ctx, gw, point, own)
                gpar = gs.sum(dim=0).contiguous()
            finally:
                if moved:
                    solver.set_par(before)
        return gP, gpar if ctx.needs_input_grad[1] else None, None, None


def solve_differentiable(loop: DeviceLoop, P, irregular="nan", lbw=None, ubw=None, Q=None, R=None, par=None):
    """Solve the loop's problems at P (B, n_p float64 device tensor, the loop's resident layout) and
    return w (B, n_w) with the backward described above.  The loop is used as it stands: its warm
    start is the one its next ``solve()`` would take, and its resident P, w, lam, lamx, status and
    iters are this solve's afterwards.

    irregular: what an instance flagged irregular (a variable on its bound, an indefinite reduced
    Hessian) contributes to the gradients -- "nan" (default: its row is NaN, the others are unaffected)
    or "zero" (its row is replaced by zeros).

    lbw / ubw: None (the loop's bounds as they stand, :class:`MPCFunction`), or both (B, n_w) float64
    device tensors in ``DeviceLoop.set_bounds``' layout: copies of them are installed as the loop's
    per-instance bounds (and stay installed), and the backward fills ``lbw.grad`` / ``ubw.grad`` from one
    ``sens_bounds_vjp`` launch; ``P.grad`` is computed only when P requires it
    (:class:`MPCBoundsFunction`, which also says where the host waits).

    Q / R: None, or both float64 device tensors of shape (nx,) and (nu,): the diagonal cost weights, shared
    by the batch.  The solver's weights are set from their values (one host read of the two tensors; they
    stay set), and the backward fills ``Q.grad`` / ``R.grad`` with the stage-and-batch sum from one
    ``sens_weights_vjp`` launch; ``P.grad`` is computed only when P requires it
    (:class:`MPCWeightsFunction`).  Not together with lbw / ubw, and not for linear models, whose weights
    are their tables (``Solver.sens_weights_vjp`` gives their gradients).

    par: None, or a float64 device tensor of shape (n_th,): the constants of the loop's ODE model, shared by the
    batch.  The solver's constants are set from its values (one host read; they stay set), and the backward
    fills ``par.grad`` with the stage-and-batch sum from one ``sens_model_vjp`` launch; ``P.grad`` is computed
    only when P requires it (:class:`MPCParFunction`).  Not together with lbw / ubw or Q / R, not for the
    unicycle, which has no constants, and not for linear models, whose constants are their tables
    (``Solver.sens_model_vjp`` gives their gradients)."""
    if irregular not in ("nan", "zero"):
        raise ValueError('irregular: "nan" or "zero"')
    if not isinstance(P, torch.Tensor) or P.dtype != torch.float64 or tuple(P.shape) != tuple(loop.P.shape) \
            or P.device != loop.device:
        raise ValueError(f"P: expected a float64 tensor of shape {tuple(loop.P.shape)} on {loop.device}")
    if par is not None:
        if lbw is not None or ubw is not None or Q is not None or R is not None:
            raise ValueError("par cannot be combined with lbw / ubw or Q / R")
        if loop.solver.ocp.model == "linear":
            raise ValueError("par: a linear model's constants are its tables (Solver.sens_model_vjp)")
        if loop.solver.ocp.model == "unicycle":
            raise ValueError("par: the unicycle has no model constants")
        n_th = loop.solver._h.model_dims()
        if not isinstance(par, torch.Tensor) or par.dtype != torch.float64 or tuple(par.shape) != (n_th,) \
                or par.device != loop.device:
            raise ValueError(f"par: expected a float64 tensor of shape ({n_th},) on {loop.device}")
        return MPCParFunction.apply(P, par, loop, irregular == "zero")
    if Q is not None or R is not None:
        if lbw is not None or ubw is not None:
            raise ValueError("Q / R and lbw / ubw cannot be combined")
        if loop.solver.ocp.model == "linear":
            raise ValueError("Q / R: a linear model's weights are its tables (Solver.sens_weights_vjp)")
        if Q is None or R is None:
            raise ValueError("Q and R must both be given (or both None)")
        for t, name, n in ((Q, "Q", loop.solver.ocp.nx), (R, "R", loop.solver.ocp.nu)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (n,) \
                    or t.device != loop.device:
                raise ValueError(f"{name}: expected a float64 tensor of shape ({n},) on {loop.device}")
        return MPCWeightsFunction.apply(P, Q, R, loop, irregular == "zero")
    if lbw is None and ubw is None:
        return MPCFunction.apply(P, loop, irregular == "zero")
    if lbw is None or ubw is None:
        raise ValueError("lbw and ubw must both be given (or both None)")
    return MPCBoundsFunction.apply(P, lbw, ubw, loop, irregular == "zero")
