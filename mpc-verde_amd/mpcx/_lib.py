"""ctypes binding of ``libmpcx.so`` (the C ABI declared in ``include/mpcx.h``).

The HIP library is the only compute path: if it is missing or cannot be loaded
this module raises immediately -- there is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCX_LIB", os.path.join(_HERE, "libmpcx.so"))

Model = collections.namedtuple("Model", "id nx nu ode")
# The stage models by name: the value of mpcx_model (include/mpcx.h; 6 is unassigned), the dimensions the
# model fixes (the linear model takes them from its tables) and whether it is a nonlinear ODE model.
# ocp.MODEL_IDS and ode.MODELS are views of this table.
MODEL_TABLE = {"unicycle": Model(1, 3, 2, False), "linear": Model(2, None, None, False),
               "kin_bicycle": Model(3, 3, 2, True), "dyn_bicycle": Model(4, 6, 2, True),
               "cartpole": Model(5, 4, 1, True), "path_bicycle": Model(7, 4, 2, True)}
MODEL_UNICYCLE = MODEL_TABLE["unicycle"].id
MODEL_LINEAR = MODEL_TABLE["linear"].id
MODEL_KIN_BICYCLE = MODEL_TABLE["kin_bicycle"].id
MODEL_DYN_BICYCLE = MODEL_TABLE["dyn_bicycle"].id
MODEL_CARTPOLE = MODEL_TABLE["cartpole"].id
MODEL_PATH_BICYCLE = MODEL_TABLE["path_bicycle"].id
COST_QUADRATURE = 0
COST_NODE = 1
P_X0_XREF = 0
P_X0_STAGEREF = 1

STATUS = {0: "Solve_Succeeded", 1: "Solved_To_Acceptable_Level", 2: "Maximum_Iterations_Exceeded",
          3: "Restoration_Failed", 4: "Infeasible_Problem_Detected", 5: "Error_In_Step_Computation"}

# C-ABI entry points (include/mpcx.h) -- checked by tests/test_capi_symbols.py
EXPORTS = ("mpcx_default_spec", "mpcx_create", "mpcx_destroy", "mpcx_last_error", "mpcx_dims", "mpcx_solve_batch",
           "mpcx_solve_batch_dev", "mpcx_plant_step", "mpcx_shift_dev", "mpcx_rk4_sens", "mpcx_rk4_sens_dev",
           "mpcx_set_linear_model", "mpcx_set_linear_tab_dev", "mpcx_step_dev", "mpcx_run_dev",
           "mpcx_source_hash", "mpcx_launch_shape", "mpcx_set_bounds_dev", "mpcx_sens_x0", "mpcx_sens_x0_dev",
           "mpcx_sens_p", "mpcx_sens_p_dev", "mpcx_sens_vjp", "mpcx_sens_vjp_dev", "mpcx_sens_bounds",
           "mpcx_sens_bounds_dev", "mpcx_sens_bounds_vjp", "mpcx_sens_bounds_vjp_dev", "mpcx_weight_dims",
           "mpcx_set_weights", "mpcx_sens_weights", "mpcx_sens_weights_dev", "mpcx_sens_weights_vjp",
           "mpcx_sens_weights_vjp_dev", "mpcx_model_dims", "mpcx_set_par", "mpcx_sens_model", "mpcx_sens_model_dev",
           "mpcx_sens_model_vjp", "mpcx_sens_model_vjp_dev")
STEP_COLD = 1
STEP_PRIMAL_ONLY = 2


class Spec(ctypes.Structure):
    """Mirror of ``mpcx_spec`` (include/mpcx.h)."""

    _fields_ = [("model", ctypes.c_int32), ("cost", ctypes.c_int32), ("param_layout", ctypes.c_int32),
                ("N", ctypes.c_int32), ("M", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("device", ctypes.c_int32), ("group_policy", ctypes.c_int32), ("T", ctypes.c_double),
                ("tol", ctypes.c_double), ("Q", ctypes.c_double * 8), ("R", ctypes.c_double * 8),
                ("lbu", ctypes.c_double * 8), ("ubu", ctypes.c_double * 8), ("lbx", ctypes.c_double * 8),
                ("ubx", ctypes.c_double * 8), ("warm_mu_init", ctypes.c_double),
                ("warm_bound_push", ctypes.c_double), ("warm_mult_push", ctypes.c_double),
                ("nx", ctypes.c_int32), ("nu", ctypes.c_int32), ("par", ctypes.c_double * 8),
                ("dual_inf_tol", ctypes.c_double), ("constr_viol_tol", ctypes.c_double),
                ("compl_inf_tol", ctypes.c_double), ("acceptable_tol", ctypes.c_double),
                ("acceptable_dual_inf_tol", ctypes.c_double), ("acceptable_constr_viol_tol", ctypes.c_double),
                ("acceptable_compl_inf_tol", ctypes.c_double), ("acceptable_obj_change_tol", ctypes.c_double),
                ("acceptable_iter", ctypes.c_int32), ("no_restoration", ctypes.c_int32)]


_lib = None


class MpcxError(RuntimeError):
    pass


def _bind_single_hip_runtime():
    """Make libmpcx resolve libamdhip64.so.7 to the copy PyTorch uses, if PyTorch is installed.

    PyTorch-ROCm ships its own libamdhip64 (NEEDED as "libamdhip64.so", found via
    its RPATH) while libmpcx is linked against /opt/rocm's (NEEDED
    "libamdhip64.so.7"); both carry the soname libamdhip64.so.7.  Loaded in the
    wrong order a process ends up with two HIP runtimes, and the second one cannot
    open the GPU ("No HIP GPUs are available").  Loading PyTorch's copy first
    (without importing torch) makes every later lookup resolve to that one file.
    """
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(p):
        ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)


def source_hash():
    """Hash of the library's sources in the tree, computed as mpc-verde_amd/Makefile does
    (the sorted csrc/*.hip, csrc/capi.cpp, the sorted csrc/*.h, include/mpcx.h, then the Makefile
    for its compiler flags; sha256, 16 hex digits), or None
    when the sources are not next to the package (an installed copy)."""
    import glob
    import hashlib

    pkg = os.path.dirname(_HERE)
    files = sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")))
    files.append(os.path.join(pkg, "csrc", "capi.cpp"))
    files += sorted(glob.glob(os.path.join(pkg, "csrc", "*.h")))
    files.append(os.path.join(os.path.dirname(pkg), "include", "mpcx.h"))
    files.append(os.path.join(pkg, "Makefile"))
    if not all(os.path.exists(f) for f in files):
        return None
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """Load libmpcx.so (raises if it has not been built, or was built from other sources
    than the tree's -- a stale binary must not run as the product)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcxError(f"{LIB_PATH} not found: build it with `make -C mpc-verde_amd` (hipcc, gfx950)")
    _bind_single_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int32)
    vp = ctypes.c_void_p
    H = ctypes.c_void_p
    lib.mpcx_default_spec.argtypes = [ctypes.POINTER(Spec), ctypes.c_int32, ctypes.c_int32]
    lib.mpcx_create.argtypes = [ctypes.POINTER(Spec), ctypes.POINTER(H)]
    lib.mpcx_destroy.argtypes = [H]
    lib.mpcx_destroy.restype = None
    lib.mpcx_last_error.restype = ctypes.c_char_p
    lib.mpcx_dims.argtypes = [H, ip, ip, ip]
    lib.mpcx_launch_shape.argtypes = [H, ctypes.c_int32, ip, ip, ctypes.c_char_p, ctypes.c_int32]
    lib.mpcx_solve_batch.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
    lib.mpcx_solve_batch_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcx_plant_step.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp]
    lib.mpcx_shift_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcx_rk4_sens.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp]
    lib.mpcx_rk4_sens_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp]
    lib.mpcx_set_linear_model.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, ip, ctypes.c_int32]
    lib.mpcx_set_linear_tab_dev.argtypes = [H, ctypes.c_void_p, ctypes.c_int32]
    lib.mpcx_set_bounds_dev.argtypes = [H, vp, vp, ctypes.c_int32, ctypes.c_int32, vp]
    lib.mpcx_step_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcx_run_dev.argtypes = [H, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp,
                                 vp, vp, vp, vp]
    lib.mpcx_sens_x0.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, dp, ip]
    lib.mpcx_sens_x0_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcx_sens_p.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, ip]
    lib.mpcx_sens_p_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]
    lib.mpcx_sens_vjp.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, ip]
    lib.mpcx_sens_vjp_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]
    lib.mpcx_sens_bounds.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, ip]
    lib.mpcx_sens_bounds_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]
    lib.mpcx_sens_bounds_vjp.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, dp, ip]
    lib.mpcx_sens_bounds_vjp_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    lib.mpcx_weight_dims.argtypes = [H, ip]
    lib.mpcx_set_weights.argtypes = [H, dp, dp]
    lib.mpcx_sens_weights.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, ctypes.c_int32, dp, ip]
    lib.mpcx_sens_weights_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp]
    lib.mpcx_sens_weights_vjp.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, dp, ip]
    lib.mpcx_sens_weights_vjp_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    lib.mpcx_model_dims.argtypes = [H, ip]
    lib.mpcx_set_par.argtypes = [H, dp]
    lib.mpcx_sens_model.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, ctypes.c_int32, dp, ip]
    lib.mpcx_sens_model_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp]
    lib.mpcx_sens_model_vjp.argtypes = [H, ctypes.c_int32, dp, dp, dp, dp, dp, dp, dp, ctypes.c_int32, dp, dp, ip]
    lib.mpcx_sens_model_vjp_dev.argtypes = [H, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp, vp]
    for name in EXPORTS:
        getattr(lib, name)  # AttributeError if an export is missing
    lib.mpcx_source_hash.restype = ctypes.c_char_p
    built, tree = lib.mpcx_source_hash().decode(), source_hash()
    if tree is not None and built != tree and os.environ.get("MPCX_ALLOW_STALE_LIB") != "1":
        raise MpcxError(f"{LIB_PATH} was built from other sources (hash {built}) than the tree's ({tree}): "
                        "rebuild it with `make -C mpc-verde_amd`")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().mpcx_last_error().decode(errors="replace")
        raise MpcxError(f"mpcx error {rc}: {msg}")


def dptr(a):
    """double* of a C-contiguous float64 ndarray (or None)."""
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("expected a C-contiguous float64 ndarray")
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def iptr(a):
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("expected a C-contiguous int32 ndarray")
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class Handle:
    """Owning wrapper of an ``mpcx_handle*``."""

    def __init__(self, spec: Spec):
        lib = load()
        self._spec = spec
        self._h = ctypes.c_void_p()
        check(lib.mpcx_create(ctypes.byref(spec), ctypes.byref(self._h)))
        nw, ng, npar = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib.mpcx_dims(self._h, ctypes.byref(nw), ctypes.byref(ng), ctypes.byref(npar)))
        self.n_w, self.n_g, self.n_p = nw.value, ng.value, npar.value

    @property
    def ptr(self):
        return self._h

    def set_linear_model(self, lin):
        """Upload the stage tables of a LinearOCP (mpcx_set_linear_model)."""
        n_tab, A, B, c, Wp, tab, rows = lin.tables()
        A, B, c, Wp = (np.ascontiguousarray(v, np.float64) for v in (A, B, c, Wp))
        tab = np.ascontiguousarray(tab, np.int32)
        check(load().mpcx_set_linear_model(self._h, int(n_tab), dptr(A), dptr(B), dptr(c), dptr(Wp), iptr(tab),
                                           int(rows)))
        self._lin_refs = (A, B, c, Wp, tab)

    def launch_shape(self, B):
        """(lanes per group, replicas per wave, kernel name) of a B-instance solve launch
        (mpcx_launch_shape: the instantiation rocprofv3 will name)."""
        G, R = ctypes.c_int32(), ctypes.c_int32()
        buf = ctypes.create_string_buffer(256)
        check(load().mpcx_launch_shape(self._h, int(B), ctypes.byref(G), ctypes.byref(R), buf, len(buf)))
        return G.value, R.value, buf.value.decode()

    def set_bounds_dev(self, d_lbw, d_ubw, rows=1, n_steps=1, stream=None):
        """Install caller-owned device bounds (mpcx_set_bounds_dev): d_lbw / d_ubw are device addresses
        (int) of n_steps x rows x n_w float64 arrays that stay alive and unchanged while installed; both
        None reverts to the spec bounds.  The call validates them on ``stream`` and waits for it."""
        vp = ctypes.c_void_p
        check(load().mpcx_set_bounds_dev(self._h, None if d_lbw is None else vp(d_lbw),
                                         None if d_ubw is None else vp(d_ubw), int(rows), int(n_steps),
                                         None if stream is None else vp(stream)))

    def weight_dims(self):
        """Entries of a stage's weight row (mpcx_weight_dims)."""
        n = ctypes.c_int32()
        check(load().mpcx_weight_dims(self._h, ctypes.byref(n)))
        return n.value

    def set_weights(self, Q, R):
        """Replace the diagonal cost weights (mpcx_set_weights); the spec mirror follows."""
        Q, R = (np.ascontiguousarray(v, np.float64).ravel() for v in (Q, R))
        if Q.size != self._spec.nx or R.size != self._spec.nu:
            raise ValueError(f"set_weights: expected Q ({self._spec.nx},) and R ({self._spec.nu},)")
        check(load().mpcx_set_weights(self._h, dptr(Q), dptr(R)))
        for i, v in enumerate(Q):
            self._spec.Q[i] = v
        for i, v in enumerate(R):
            self._spec.R[i] = v

    def model_dims(self):
        """Entries of a stage's model row (mpcx_model_dims)."""
        n = ctypes.c_int32()
        check(load().mpcx_model_dims(self._h, ctypes.byref(n)))
        return n.value

    def set_par(self, par):
        """Replace the constants of an ODE model (mpcx_set_par); the spec mirror follows."""
        par = np.ascontiguousarray(par, np.float64).ravel()
        n = self.model_dims()
        if par.size != n:
            raise ValueError(f"set_par: expected {n} constants")
        buf = np.zeros(8)  # (the C side reads n_th entries; refusals come from there)
        buf[:n] = par
        check(load().mpcx_set_par(self._h, dptr(buf)))
        for i, v in enumerate(par):
            self._spec.par[i] = v

    @property
    def spec(self):
        return self._spec

    def close(self):
        if self._h:
            load().mpcx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
