"""The references of tests/test_gpu_forward.py checked against each other on the CPU
(tests/helpers/forward_ref.py): the float64 restatement of forward_sweep's composition order against
the sequential long-double recursion on every case of the GPU test; the exact cases redone in Python
integers, every intermediate of the restatement an integer below 2^53 (so the device's result does
not depend on its fma order or association either); and the long-double step lengths against a
brute-force check of the fraction-to-boundary rule.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import forward_ref as fr  # noqa: E402
from forward_ref import LD  # noqa: E402

# one case per model and group size here, the horizons that change the path (a partial last row, a
# lane past a wave boundary); the GPU test's tolerance runs the restatement on all of them
STEP_CASES = [("lin41", G, fr.HORIZONS[G][1]) for G in (16, 32, 64, 128, 256)] + [("unicycle", 32, 31), ("lin42", 64, 63)]


def test_case_table_is_the_issue_s():
    assert fr.HORIZONS == {16: (1, 8, 15), 32: (16, 17, 31), 64: (32, 33, 63), 128: (64, 65, 127),
                           256: (128, 129, 191, 192, 193, 255)}
    assert [fr.batch_of(G) for G in (16, 32, 64, 128, 256)] == [33, 33, 5, 5, 5]
    assert len(fr.CASES) == 4 * 3 + (4 * 3 + 6) + 3 * 3


def test_restatement_agrees_with_the_sequential_reference():
    """Rounded operands, both right-hand sides, every case: the composition order restated in float64
    is the recursion up to rounding (1e-9 is far above any rounding error here and far below a wrong
    partner's effect, which is O(1); the GPU test's tolerance is 64 times the worst figure printed)."""
    tol, worst, case = fr.sweep_tolerance()
    print(f"restatement against long double: worst {worst:.3e} at {case}; device tolerance {tol:.3e}")
    assert 0.0 < worst < 1e-9


@pytest.mark.parametrize("model,G,N", fr.CASES, ids=lambda v: str(v))
def test_exact_cases_are_exact(model, G, N):
    """The integer cases in Python integers (no rounding possible) and in float64: the same values at
    every intermediate of the restatement, all below 2^53 -- and both equal the sequential recursion."""
    pr = fr.exact_problem(model, G, N)
    for call in (0, 1):
        ints, flts = [], []
        zi = fr.sweep_restated(pr, call, dtype=object, seen=ints.append)
        zf = fr.sweep_restated(pr, call, dtype=np.float64, seen=flts.append)
        assert len(ints) == len(flts) > 4
        for a, b in zip(list(ints) + list(zi), list(flts) + list(zf)):
            big = max((abs(v) for v in a.ravel()), default=0)
            assert big < 2 ** 53
            assert all(isinstance(v, int) for v in a.ravel())
            assert np.array_equal(a.astype(np.float64), b)
        ref = fr.sweep_reference(pr, call)
        for got, want in zip(zf, ref):
            assert np.array_equal(got.astype(LD), want)
        assert np.all(ref[0][:, N + 1:] == 0) and np.all(ref[1][:, N + 1:] == 0) and np.all(ref[0][:, N, pr["nx"]:] == 0)
        assert np.abs(ref[0][:, :N + 1, :pr["nx"]]).min(axis=-1).max() > 0  # not a trivial problem


def test_exact_cases_do_not_depend_on_what_must_not_be_read():
    """A_0, K_0's effect on dx, the lanes beyond N and the entries of A outside the mask: other values
    there give the same reference, so a device result that equals it did not read them."""
    for model, G, N in [("unicycle", 32, 17), ("lin41", 128, 65), ("dynbicycle", 64, 33)]:
        pr = dict(fr.exact_problem(model, G, N))
        am, _ = fr.masks(model)
        ref = fr.sweep_reference(pr)
        A = pr["A"] * am + 7.0 * (1.0 - am)
        A[:, 0], A[:, N + 1:] = 5.0, 9.0
        pr2 = dict(pr, A=A, lam=pr["lam"].copy(), cc=pr["cc"].copy())
        pr2["lam"][:, N + 1:], pr2["cc"][:, :, N + 1:] = 11.0, 13.0
        for got, want in zip(fr.sweep_reference(pr2), ref):
            assert np.array_equal(got, want)
        nx = pr["nx"]
        c0, c_0, kf0 = pr["c0v"][0][:, 0], pr["cc"][0][:, 0], pr["kf"][0][:, 0]
        assert np.array_equal(ref[0][:, 0, nx:], kf0 + fr.mv(pr["K"][:, 0], c0))  # du_0 = kf_0 + K_0 c0
        assert np.array_equal(ref[0][:, 1, :nx], c_0 + fr.mv(pr["Bm"][:, 0] * fr.masks(model)[1], kf0))
        assert np.any(pr["K"][:, 0] != 0) and np.any(pr["A"][:, 0] != 0)


@pytest.mark.parametrize("model,G,N", STEP_CASES, ids=lambda v: str(v))
def test_step_lengths_against_brute_force(model, G, N):
    """amax of the long-double reference is the largest step in (0, 1] that keeps every slack at
    (1 - tau) of its value: feasible at amax, and where amax < 1 infeasible a little beyond it; the
    binding components are where binding_lanes puts them."""
    st = fr.steps_problem(model, G, N)
    ref = fr.steps_reference(st)
    amax = ref["amax"]
    where = fr.binding_lanes(G, N)
    assert where[0] == 0 and where[1] == N and (where[2] % 16 == 15 or N < 15)
    assert (where[3] >= 64) == (N >= 64) and where[3] <= N
    assert np.all(amax > 0) and np.all(amax <= 1)
    assert np.all(fr.slack_shortfall(st, amax) <= 1e-17)
    short = amax < 1
    assert np.all(fr.slack_shortfall(st, amax * (1 + LD(1e-12)))[short] > 0)
    for i in range(st["B"]):
        lane = where[i % len(where)]
        assert short[i] == (lane is not None)
        if lane is not None:  # removing that lane's step frees the instance
            dz = st["dz"].copy()
            dz[i, lane] = 0.0
            assert fr.steps_reference(st, dz=dz)["amax"][i] == 1
    # the same for the bound multipliers: zL + az dzL >= (1 - tau) zL
    az = ref["az"][:, None, None]
    for z_, d_, h_ in ((st["zL"], ref["dzL"], st["hL"]), (st["zU"], ref["dzU"], st["hU"])):
        keep = np.where(h_ > 0, z_ + az * d_ - (1 - LD(st["tau"])) * z_, 1)
        assert np.all(keep >= -1e-17)
    assert np.any(ref["az"] < 1)


def test_tiny_step_reference():
    st = dict(fr.steps_problem("lin41", 64, 33))
    z = st["z"]
    for factor, want in ((0.5, True), (2.0, False)):
        dz = np.zeros_like(z)
        dz[:, 7, 1] = factor * 10 * fr.EPS * (1 + np.abs(z[:, 7, 1]))
        dz[:, 33, 4] = 1.0  # u of node N: not owned
        dz[:, 40, 0] = 1.0  # beyond N
        assert np.all(fr.steps_reference(st, dz=dz)["tiny"] == want)
