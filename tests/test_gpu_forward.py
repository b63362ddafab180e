"""Device tests of the two phases of the solve kernel's iteration that had none of their own
(mpc-verde_amd/csrc/forward.h), through the harness tests/hip/forward_check.hip, which calls the very
functions the solve kernel runs: forward_sweep (the closed-loop maps, their DPP prefix scan, the LDS
hand-offs between the waves of a wide group, du and dlam), bound_step (the bound-dual steps and a lane's
fraction-to-boundary limits) and step_lengths (amax, az, gd and the tiny-step flag over the group).  The
references are in tests/helpers/forward_ref.py; tests/test_forward_cpu.py checks them against each
other without a GPU.  A wrong scan partner, a value from the neighbouring instance of the wave or a
wrong dlam on one lane still gives a descent direction that the line search absorbs, so no end-to-end
test sees it: here every lane is compared.

Cases: the horizons 1, 8, 15 (G = 16), 16, 17, 31 (32), 32, 33, 63 (64), 64, 65, 127 (128) and 128, 129,
191, 192, 193, 255 (256) of every instantiation of the harness -- UnicycleModel (masked A, B) at G = 16 ...
128, LinearModel<4, 1> at 16 ... 256, LinearModel<4, 2>, OdeModel<PathBicycle> (NX = 4) and
OdeModel<DynBicycle> (NX = 6, masked A: the widest map, 42 values per lane) at G = 64; B = 33 instances for
G < 64 (several different instances per wave, an empty group in the last wave), 5 otherwise.  Every launch
makes the main step's call and the second-order correction's (other right-hand sides, the same gains),
with the step lengths' exchange between them, so a multi-wave group enters the second sweep on the other
LDS slot.

Tolerances.
* Exact cases: integer operands whose every intermediate is an integer below 2^53 (test_forward_cpu
  redoes them in Python integers), asserted bit for bit on every lane, the zeros beyond N included.
* Rounded cases: node by node, normalised by max(1, max |reference|) at the node, to 64 times the worst
  error of the float64 restatement of the composition order against long double over all cases: the
  restatement's worst is 1.9e-15 (LinearModel<4, 1>, G = 64, N = 63 at spectral radius 1.1), so 1.24e-13.
* Step lengths, with u = 2^-53.  rcp64(x) is within one ulp of the correctly rounded 1 / x
  (test_gpu_collectives asserts it), so rcp64(x) = (1 + e) / x with |e| <= 2u (1 + u).
  A limit -tau s rcp64(dz) takes s = fl(z - lb) (u), two product roundings (2u) and the reciprocal (2u):
  5u to first order; amax, a minimum of such limits and 1, is asserted to 6u of the long-double value
  (the sixth u covers the second-order terms and the long double's own rounding).  The invariant -- every
  slack of z + amax dz at least (1 - tau) of the old slack -- is asserted from the device's own amax in long
  double with the same allowance: the shortfall is at most 6u tau s_i.
  dzL = fma(mu, rs, -zL) - zL rs dz with rs = rcp64(s), s = fl(z - lb): rs carries 3u; mu rs - zL rounds once
  (u), zL rs dz twice (2u), the difference once (u), so |error| <= 6u (|mu / s| + |zL| + |zL dz / s|) to
  first order; asserted with 7u.  dzU alike.
  az is a minimum over limits -tau zL rcp64(dzL) of the device's own, rounded dzL: two products and the
  reciprocal, 4u; asserted to 5u of the long-double minimum over the device's dzL and dzU (themselves
  asserted as above).
  gd: |error| <= n eps sum |gp_i dz_i| with n the number of owned entries and eps = 2^-52.
  The tiny-step flag, and amax where the true value is exactly 1, are asserted exactly.

Measured on one MI355X.  Every exact case is bit for bit the recursion, both calls.  The sweep's worst
error on the rounded cases is 1.66e-15 (LinearModel<4, 1>, G = 64, N = 63 at radius 1.1: 0.86 times the
restatement's on that case, 75 times under the tolerance); its worst ratio to the restatement on the same
case is 2.4 (UnicycleModel, G = 32, N = 17: 1.35e-15 against 5.7e-16).  Step lengths, worst over all
cases and edges, in u: dzL 1.95 and dzU 2.02 (of 7), amax 1.63 (of 6), the slack invariant short by 1.63
(of 6), az 2.12 (of 5); gd reaches 0.05 of its bound.  No case disagreed with the reference, and no
defect was found in forward.h.  One was found in how this file used the harness: the library has to be
loaded after torch, or its launches report that no device is present (load() imports torch first).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import forward_ref as fr  # noqa: E402
from forward_ref import LD, U  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = os.path.join(HERE, "hip", "libforward_check.so")
STEP_CASES = ([("lin41", G, N) for G in (16, 32, 64, 128, 256) for N in fr.HORIZONS[G]] +
              [("unicycle", G, fr.HORIZONS[G][-1]) for G in (16, 32, 64, 128)] +
              [("lin42", 64, 33), ("dynbicycle", 64, 63)])
EDGE_CASES = [("unicycle", 16, 8), ("lin41", 32, 17), ("lin41", 64, 33), ("lin41", 128, 65), ("lin41", 256, 193)]
ids = lambda v: str(v)  # noqa: E731


def load():
    import torch  # noqa: F401  (first: the harness library must find the HIP runtime torch has loaded, not load another)

    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (make -C tests/hip)")
    lib = ctypes.CDLL(LIB)
    lib.forward_check.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_void_p] * 3
    return lib


def sizes(lib, model_id):
    dims, masks = (ctypes.c_int * 5)(), (ctypes.c_ulonglong * 2)()
    assert lib.forward_check_sizes(model_id, dims, masks) == 0
    return list(dims), list(masks)


def run_forward_check(pr=None, st=None):
    """One launch of the harness on a sweep problem and / or step-length operands: dict of dz, dlam (the
    two calls: [2, B, G, ...]), dzL, dzU [2, B, G, nz] and the per-instance amax, az, gd, tiny, amax2, az2."""
    import torch

    lib = load()
    src = pr if pr is not None else st
    m, G, N, B, nx, nu = fr.MODELS[src["model"]], src["G"], src["N"], src["B"], src["nx"], src["nu"]
    nz = nx + nu
    (dnx, dnu, n_in, n_out, n_inst), bits = sizes(lib, m["id"])
    assert (dnx, dnu) == (nx, nu) and tuple(bits) == fr.mask_bits(src["model"])  # the reference's masks are the device's
    x = fr.pack_records(pr, st)
    assert x.shape == (B, G, n_in)
    d_in = torch.from_numpy(x).cuda()
    out = torch.full((B, G, n_out), np.nan, dtype=torch.float64, device="cuda")
    oinst = torch.full((B, n_inst), np.nan, dtype=torch.float64, device="cuda")
    mu, tau = (st["mu"], st["tau"]) if st is not None else (0.1, 0.99)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.forward_check(m["id"], G, N, B, mu, tau, p(d_in), p(out), p(oinst)) == 0
    o, q = out.cpu().numpy(), oinst.cpu().numpy()
    cut = np.cumsum([0, nz, nx, nz, nx, nz, nz, nz, nz])
    f = [o[..., a:b] for a, b in zip(cut[:-1], cut[1:])]
    assert cut[-1] == n_out
    return dict(dz=np.stack([f[0], f[2]]), dlam=np.stack([f[1], f[3]]), dzL=np.stack([f[4], f[6]]),
                dzU=np.stack([f[5], f[7]]), amax=q[:, 0], az=q[:, 1], gd=q[:, 2], tiny=q[:, 3], amax2=q[:, 4], az2=q[:, 5])


def test_entry_refuses_shapes_without_an_instantiation():
    lib = load()
    dims, masks = (ctypes.c_int * 5)(), (ctypes.c_ulonglong * 2)()
    assert lib.forward_check_sizes(5, dims, masks) == 2
    assert lib.forward_check(0, 256, 200, 1, 0.1, 0.99, None, None, None) == 2  # no unicycle at G = 256
    assert lib.forward_check(2, 32, 20, 1, 0.1, 0.99, None, None, None) == 2
    assert lib.forward_check(1, 48, 20, 1, 0.1, 0.99, None, None, None) == 2
    assert lib.forward_check(1, 64, 64, 1, 0.1, 0.99, None, None, None) == 1  # N >= G
    assert lib.forward_check(1, 64, 0, 1, 0.1, 0.99, None, None, None) == 1
    assert lib.forward_check(1, 64, 10, 0, 0.1, 0.99, None, None, None) == 1


@pytest.mark.parametrize("model,G,N", fr.CASES, ids=ids)
def test_exact_sweep_bit_for_bit(model, G, N):
    """(a) and (c): integer operands, both calls of the launch; dz and dlam equal the sequential
    recursion on every lane of every instance -- with A_0, K_0, the entries of A outside the model's mask
    and the lanes beyond N holding non-zero values that must not matter, and exact zeros beyond N."""
    pr = fr.exact_problem(model, G, N)
    got = run_forward_check(pr)
    for call in (0, 1):
        dz, dlam = fr.sweep_reference(pr, call)
        for name, g, r in (("dz", got["dz"][call], dz), ("dlam", got["dlam"][call], dlam)):
            bad = np.argwhere(g != r.astype(np.float64))
            assert len(bad) == 0, f"{name} of call {call}: {len(bad)} entries differ, first (instance, lane, entry) {bad[:5].tolist()}"
        assert np.all(got["dz"][call][:, N + 1:] == 0) and np.all(got["dlam"][call][:, N + 1:] == 0)
    assert np.all(got["dzL"] == 0) and np.all(got["dzU"] == 0)
    assert np.all(got["amax"] == 1) and np.all(got["az"] == 1) and np.all(got["amax2"] == 1) and np.all(got["az2"] == 1)


ROUNDED = [c + (None,) for c in fr.CASES] + [fr.HOT_CASE + (1.1,)]


@pytest.mark.parametrize("model,G,N,radius", ROUNDED, ids=ids)
def test_rounded_sweep_against_long_double(model, G, N, radius):
    """(b) and (c): random operands with A + B K of spectral radius in [0.9, 1.02] (one case at 1.1),
    both calls, node by node against the long-double recursion."""
    tol, worst, _ = fr.sweep_tolerance()
    pr, refs, rs_err = fr.rounded_case(model, G, N, radius)
    got = run_forward_check(pr)
    errs = [fr.sweep_error((got["dz"][c], got["dlam"][c]), refs[c]) for c in (0, 1)]
    print(f"forward_sweep {model} G={G} N={N} radius={radius}: device {errs[0]:.3e} / {errs[1]:.3e} (second call), "
          f"restatement {rs_err:.3e}, ratio {max(errs) / rs_err:.2f}; tolerance {tol:.3e} = 64 x {worst:.3e}")
    assert max(errs) <= tol
    for c in (0, 1):
        assert np.all(got["dz"][c][:, N + 1:] == 0) and np.all(got["dlam"][c][:, N + 1:] == 0)
        assert np.all(got["dz"][c][:, N, pr["nx"]:] == 0)


def check_steps(st, got, label):
    """The assertions of (d) on one launch's results; returns the worst figures in units of u."""
    ref = fr.steps_reference(st)
    B, N = st["B"], st["N"]
    worst = {}
    with np.errstate(all="ignore"):
        for name, mag in (("dzL", ref["mag_L"]), ("dzU", ref["mag_U"])):
            err = np.abs(got[name][0].astype(LD) - ref[name])
            assert np.all(np.isfinite(got[name][0]))
            assert np.all(err <= 7 * U * mag), f"{label} {name}: {float((err / np.maximum(mag, 1e-300)).max() / U):.2f} u"
            worst[name] = float(np.where(mag > 0, err / np.where(mag > 0, mag, 1), 0).max() / U)
            assert np.all(got[name][0][mag == 0] == 0)  # no bound, no step
        rel = np.abs(got["amax"].astype(LD) - ref["amax"]) / ref["amax"]
        worst["amax"] = float(rel.max() / U)
        assert np.all(rel <= 6 * U), f"{label} amax: {worst['amax']:.2f} u"
        assert np.all(got["amax"][ref["amax"] == 1] == 1.0)  # the true amax is exactly 1
        short = fr.slack_shortfall(st, got["amax"])
        worst["invariant"] = float(short.max() / U)
        assert np.all(short <= 6 * U), f"{label} fraction to the boundary from the device's amax: short by {worst['invariant']:.2f} u"
        az_ref = fr.steps_reference(st, dzL=got["dzL"][0], dzU=got["dzU"][0])["az"]
        rel = np.abs(got["az"].astype(LD) - az_ref) / az_ref
        worst["az"] = float(rel.max() / U)
        assert np.all(rel <= 5 * U), f"{label} az: {worst['az']:.2f} u"
        n = int(fr.owned(st)[0].sum())
        gerr = np.abs(got["gd"].astype(LD) - ref["gd"])
        assert np.all(gerr <= n * fr.EPS * ref["gd_abs"]), f"{label} gd"
        worst["gd"] = float((gerr / np.maximum(n * fr.EPS * ref["gd_abs"], 1e-300)).max())
        assert np.array_equal(got["tiny"] > 0.5, ref["tiny"]) and np.all((got["tiny"] == 0) | (got["tiny"] == 1))
    # the correction's calls: its sweep had zero operands, so its step is zero
    zero = fr.steps_reference(st, dz=np.zeros_like(st["z"]))
    assert np.all(got["amax2"] == 1.0)
    az2 = fr.steps_reference(st, dz=np.zeros_like(st["z"]), dzL=got["dzL"][1], dzU=got["dzU"][1])["az"]
    assert np.all(np.abs(got["az2"].astype(LD) - az2) <= 5 * U * az2)
    assert np.all(np.abs(got["dzL"][1].astype(LD) - zero["dzL"]) <= 7 * U * zero["mag_L"])
    assert np.all(np.abs(got["dzU"][1].astype(LD) - zero["dzU"]) <= 7 * U * zero["mag_U"])
    return worst


@pytest.mark.parametrize("model,G,N", STEP_CASES, ids=ids)
def test_step_lengths_against_long_double(model, G, N):
    """(d): random interior iterates with no, one-sided and two-sided bounds; the component that binds
    amax on lane 0, on lane N, on the last lane of a 16-lane row, in wave 1 or later, and nowhere (the
    true amax exactly 1), by instance."""
    st = fr.steps_problem(model, G, N)
    got = run_forward_check(st=st)
    worst = check_steps(st, got, f"{model} G={G} N={N}")
    print(f"step lengths {model} G={G} N={N}: in u (gd: of its bound) " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    ref = fr.steps_reference(st)
    where = fr.binding_lanes(G, N)
    assert all((ref["amax"][i] < 1) == (where[i % 5] is not None) for i in range(st["B"]))


@pytest.mark.parametrize("model,G,N", EDGE_CASES, ids=ids)
def test_step_length_edges(model, G, N):
    """(d), edges: dz = +0, -0, subnormals (rcp64 gives NaN below 2^-1024: the limit must drop out of the
    minimum, as the infinite true limit does) and +-1e300 on bounded components; infinite bounds with
    hL = hU = false; NaN in dz on entries no lane owns (u of node N, the lanes beyond N), which must
    reach no output; an instance whose true amax is exactly 1."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.steps_problem(model, G, N).items()}
    nx = st["nx"]

    def bound(i, lane, j):
        st["hL"][i, lane, j] = st["hU"][i, lane, j] = 1.0
        st["lb"][i, lane, j], st["ub"][i, lane, j] = st["z"][i, lane, j] - 0.5, st["z"][i, lane, j] + 0.25
        st["zL"][i, lane, j], st["zU"][i, lane, j] = 0.3, 0.7

    l1, l2, l3, l4 = (1, 2, 3, 4) if N >= 5 else (0, 0, 0, 0)
    for lane, j, v in ((l1, 0, 0.0), (l2, 1, -0.0), (l3, 2, -1e-310), (l4, 0, 4.9e-324), (N, 1, -2.5e-308), (N, 0, 1e-320)):
        bound(0, lane, j)
        st["dz"][0, lane, j] = v
    bound(1, N // 2, 1)
    st["dz"][1, N // 2, 1] = 1e300
    bound(2, N, 2)
    st["dz"][2, N, 2] = -1e300
    st["dz"][3, N, nx:] = np.nan
    st["dz"][3, N + 1:] = np.nan
    st["gp"][3, N + 1:] = np.nan
    assert not st["hL"][3, N + 1:].any() and not st["hU"][3, N, nx:].any() and np.isinf(st["lb"][3, N + 1:]).all()
    got = run_forward_check(st=st)
    for k, v in got.items():
        assert not np.isnan(v).any(), f"NaN in {k}"
    worst = check_steps(st, got, f"edges {model} G={G} N={N}")
    print(f"step length edges {model} G={G} N={N}: in u " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    ref = fr.steps_reference(st)
    assert ref["amax"][4] == 1 and got["amax"][4] == 1.0
    assert got["amax"][1] < 1e-299 and got["amax"][2] < 1e-299 and got["az"][1] < 1e-299 and got["az"][2] < 1e-299


@pytest.mark.parametrize("model,G,N", [("lin41", G, fr.HORIZONS[G][-1]) for G in (16, 32, 64, 128, 256)] + [("unicycle", 16, 8)],
                         ids=ids)
def test_tiny_step_flag_is_exact(model, G, N):
    """(d): one entry of one lane a factor 2 above (odd instances) or below (even ones) IPOPT's threshold
    |dz_i| = 10 eps (1 + |z_i|), every other owned entry zero; entries no lane owns hold a large step."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.steps_problem(model, G, N).items()}
    B, nx = st["B"], st["nx"]
    st["dz"][:] = 0.0
    st["dz"][:, N, nx:] = 1.0
    st["dz"][:, N + 1:] = -1.0
    for i in range(B):
        lane, j = (7 * i) % (N + 1), i % nx
        st["dz"][i, lane, j] = (2.0 if i % 2 else 0.5) * 10 * fr.EPS * (1 + abs(st["z"][i, lane, j])) * (-1) ** (i // 2)
    got = run_forward_check(st=st)
    assert np.array_equal(got["tiny"], (np.arange(B) % 2 == 0).astype(np.float64))
    assert np.array_equal(fr.steps_reference(st)["tiny"], np.arange(B) % 2 == 0)
    assert np.all(got["amax"] == 1.0)
