"""The lane-group collectives (mpc-verde_amd/csrc/collectives.h) on the device, through the harness
tests/hip/collectives_check.hip, against the plain NumPy reference tests/helpers/collectives_ref.py
(itself checked against exact arithmetic in tests/test_collectives_ref_cpu.py).

Every lane of the launch writes what it received: group sizes 16 ... 256, several groups per wave,
one wave whose surplus lanes repeat the last group, multi-wave groups with the LDS exchange.

1. gsum / gmax / gmin and greduce_n<0, 1, 2, 3>: lane-uniform bits, independence of the other groups,
   the prescribed summation order bit for bit, the error bound of that order, NaN / inf / +-0.
2. gall / gany: a single false lane at every position, the replicated form gall<32, 64>.
3. from_next / from_prev / group_next / from_lane, the scan partners as an inclusive prefix scan.
4. The two-slot LDS exchange with waves that drift apart between exchanges.
5. qmax / qmin / qmax_abs element-wise.  6. rcp64 against the correctly rounded reciprocal.

Measured on one MI355X (printed by the tests, `pytest -s`): see DESIGN.md §3 "What the device tests
pin" and the comment above rcp64.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import collectives_ref as cr  # noqa: E402

LIB = os.path.join(ROOT, "tests", "hip", "libcollectives_check.so")
GS = cr.GROUP_SIZES
REDUCE, VOTE, MOVE, DRIFT, SCAN, ELEM = range(6)


class Harness:
    def __init__(self):
        import torch

        if not os.path.exists(LIB):
            pytest.fail(f"{LIB} not built (make -C tests/hip)")
        self.torch = torch
        lib = self.lib = ctypes.CDLL(LIB)
        P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
        lib.collectives_check.argtypes = [I, I, I, I, P, P, P, P, I, D, D]
        lib.collectives_check_lanes.argtypes = [I, I]
        lib.collectives_check_lanes.restype = L
        lib.collectives_check_scan.argtypes = [I, P, P, P]
        lib.collectives_check_elem.argtypes = [L, P, P, P]
        lib.collectives_check_rcp.argtypes = [L, P, P]

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(None if t is None else t.data_ptr())

    def group(self, what, G, a, b=None, out_dtype=np.float64, in_dtype=np.float64, b_dtype=np.float64):
        """inputs [cases, groups * G] -> outputs [cases, n_out, T]"""
        a = np.atleast_2d(a)
        cases, groups = a.shape[0], a.shape[1] // G
        T = self.lib.collectives_check_lanes(G, groups)
        assert T == cr.n_lanes(G, groups)
        n_out = self.lib.collectives_check_outputs(what)
        da = self.dev(a, in_dtype)
        db = None if b is None else self.dev(np.atleast_2d(b), b_dtype)
        # (poisoned, so that a lane the kernel did not write shows)
        out = self.torch.full((cases, n_out, T), -77, dtype=getattr(self.torch, np.dtype(out_dtype).name), device="cuda")
        rc = self.lib.collectives_check(what, G, groups, cases, self.ptr(da), self.ptr(db), self.ptr(out), None, 0, 0.0, 0.0)
        assert rc == 0
        return out.cpu().numpy()

    def drift(self, G, v0, rounds, work):
        groups = len(v0) // G
        T = self.lib.collectives_check_lanes(G, groups)
        da = self.dev(v0, np.float64)
        out = self.torch.full((6, T), -77.0, dtype=self.torch.float64, device="cuda")
        sink = self.torch.zeros(T, dtype=self.torch.float64, device="cuda")
        trace = self.torch.full((rounds, T), -77.0, dtype=self.torch.float64, device="cuda")
        rc = self.lib.collectives_check(DRIFT, G, groups, rounds, self.ptr(da), self.ptr(trace), self.ptr(out),
                                        self.ptr(sink), work, 0.5, 1.0)
        assert rc == 0
        return out.cpu().numpy(), trace.cpu().numpy(), sink.cpu().numpy()

    def scan(self, a, b):
        da, db = self.dev(a, np.float64), self.dev(b, np.float64)
        out = self.torch.empty((3,) + a.shape, dtype=self.torch.float64, device="cuda")
        assert self.lib.collectives_check_scan(a.shape[0], self.ptr(da), self.ptr(db), self.ptr(out)) == 0
        return out.cpu().numpy()

    def elem(self, a, b):
        da, db = self.dev(a, np.float64), self.dev(b, np.float64)
        out = self.torch.empty((3, len(a)), dtype=self.torch.float64, device="cuda")
        assert self.lib.collectives_check_elem(len(a), self.ptr(da), self.ptr(db), self.ptr(out)) == 0
        return out.cpu().numpy()

    def rcp(self, x):
        dx = self.dev(x, np.float64)
        out = self.torch.empty(len(x), dtype=self.torch.float64, device="cuda")
        assert self.lib.collectives_check_rcp(len(x), self.ptr(dx), self.ptr(out)) == 0
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def hx():
    return Harness()


def reduce_run(hx, G, v, flag=None):
    """[cases, groups * G] -> dict of per-lane outputs [cases, T]"""
    v = np.atleast_2d(v)
    flag = np.ones_like(v) if flag is None else np.atleast_2d(flag)
    o = hx.group(REDUCE, G, v, flag)
    names = ("gsum", "gmax", "gmin", "n_sum", "n_max", "n_min", "n_all")
    return {n: o[:, i, :] for i, n in enumerate(names)}


def assert_lane_uniform(x, G):
    """all lanes of a group hold the same bits"""
    b = cr.bits(x).reshape(x.shape[:-1] + (-1, G))
    np.testing.assert_array_equal(b, np.repeat(b[..., :1], G, axis=-1))


def same_bits(a, b):
    np.testing.assert_array_equal(cr.bits(a), cr.bits(b))


# ---------------------------------------------------------------------------------------------
# 1. reductions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_reductions_order_accuracy_and_lane_uniform_bits(hx, G):
    """Wide-magnitude data, different in every group.  All lanes of a group hold the same bits;
    greduce_n's values are the single reductions' bits; max and min are NumPy's; the sum has the bits
    of the order the header prescribes (balanced tree over the lanes of a wave in lane order, the
    waves' partial sums left to right) and lies within gamma_d sum|v| of the exact sum (math.fsum),
    d = log2 min(G, 64) + G / 64 - 1."""
    rng = np.random.default_rng(100 + G)
    groups = cr.n_groups(G)
    v = cr.wide_values(rng, (4, groups * G))
    r = reduce_run(hx, G, v)
    vT = cr.expand(v, G, groups)
    for n in r:
        assert_lane_uniform(r[n], G)
    same_bits(r["n_sum"], r["gsum"])
    same_bits(r["n_max"], r["gmax"])
    same_bits(r["n_min"], r["gmin"])
    np.testing.assert_array_equal(r["gmax"], np.repeat(vT.reshape(4, -1, G).max(axis=-1), G, axis=-1))
    np.testing.assert_array_equal(r["gmin"], np.repeat(vT.reshape(4, -1, G).min(axis=-1), G, axis=-1))
    same_bits(r["gsum"], cr.tree_sum(vT, G))
    exact, absum = cr.exact_sums(vT, G)
    dev = r["gsum"].reshape(-1, G)[:, 0]
    ratio = np.abs(dev - exact) / (cr.gamma(G) * absum)
    print(f"G={G}: |gsum - exact| / (gamma_{cr.sum_depth(G)} sum|v|) max {ratio.max():.3f}")
    assert np.all(np.abs(dev - exact) <= cr.gamma(G) * absum)


@pytest.mark.parametrize("G", GS)
def test_reductions_do_not_see_the_other_groups(hx, G):
    """A group's results do not change by a bit when only the other groups' inputs are replaced
    (neighbouring groups share a wave for G < 64, and the surplus lanes repeat the last group)."""
    rng = np.random.default_rng(200 + G)
    groups = cr.n_groups(G)
    v = cr.wide_values(rng, (groups, G))
    f = (rng.random((groups, G)) < 0.9).astype(np.float64)
    base = reduce_run(hx, G, v.reshape(1, -1), f.reshape(1, -1))
    # case g: every group but g replaced (values, flags and all)
    v2 = np.repeat(cr.wide_values(rng, (1, groups, G)) * 1e3, groups, axis=0)
    f2 = np.repeat(1.0 - f[None], groups, axis=0)
    for g in range(groups):
        v2[g, g], f2[g, g] = v[g], f[g]
    other = reduce_run(hx, G, v2.reshape(groups, -1), f2.reshape(groups, -1))
    for n in base:
        for g in range(groups):
            same_bits(other[n][g, g * G:(g + 1) * G], base[n][0, g * G:(g + 1) * G])
    # flags: the reference (every group has its own answer in `base` or in a replaced case)
    fT = cr.expand(np.concatenate([f.reshape(1, -1), f2.reshape(groups, -1)]), G, groups)
    got = np.concatenate([base["n_all"], other["n_all"]])
    np.testing.assert_array_equal(got, cr.flags_all(fT, G))


@pytest.mark.parametrize("G", GS)
def test_reductions_integers_zeros_and_infinities(hx, G):
    """Small integer-valued doubles: sums exact (==).  Mixes of +0 and -0: value equality and
    lane-uniform bits; which zero wins is printed, not prescribed.  +-inf: NumPy's results (the sum
    of +inf and -inf is NaN)."""
    rng = np.random.default_rng(300 + G)
    groups = cr.n_groups(G)
    vi = cr.small_integers(rng, (3, groups * G))
    r = reduce_run(hx, G, vi)
    t = cr.expand(vi, G, groups).reshape(3, -1, G)
    for n, ref in (("gsum", t.sum(-1)), ("gmax", t.max(-1)), ("gmin", t.min(-1))):
        np.testing.assert_array_equal(r[n], np.repeat(ref, G, axis=-1))
        same_bits(r["n_" + n[1:]], r[n])
    # zeros: case 0 all +0, case 1 all -0, cases 2.. mixes
    vz = cr.zero_mix(rng, (6, groups * G))
    vz[0], vz[1] = 0.0, -0.0
    r = reduce_run(hx, G, vz)
    zT = cr.expand(vz, G, groups)
    neg_in = np.signbit(zT).reshape(6, -1, G)
    mixed = np.repeat(neg_in.any(-1) & ~neg_in.all(-1), G, axis=-1)
    assert mixed[2:].any()
    for n in ("gsum", "gmax", "gmin", "n_sum", "n_max", "n_min"):
        assert np.all(r[n] == 0.0)
        assert_lane_uniform(r[n], G)
        # uniform inputs keep their sign; for mixed groups record which zero comes out
        assert not np.signbit(r[n][0]).any() and np.signbit(r[n][1]).all()
        s = np.signbit(r[n])[mixed]
        print(f"G={G} {n} of mixed +0/-0: -0 in {int(s.sum())} of {s.size} lanes")
    same_bits(r["n_sum"], r["gsum"])
    same_bits(r["n_max"], r["gmax"])
    same_bits(r["n_min"], r["gmin"])
    # infinities
    vf = cr.inf_cases(rng, G, groups)
    r = reduce_run(hx, G, vf)
    t = cr.expand(vf, G, groups).reshape(3, -1, G)
    with np.errstate(invalid="ignore"):
        same_bits(r["gsum"][:2], cr.tree_sum(cr.expand(vf, G, groups), G)[:2])  # (not the NaN's payload)
        assert np.all(r["gsum"][0] == np.inf) and np.all(r["gsum"][1] == -np.inf) and np.isnan(r["gsum"][2]).all()
    np.testing.assert_array_equal(r["gmax"], np.repeat(t.max(-1), G, axis=-1))
    np.testing.assert_array_equal(r["gmin"], np.repeat(t.min(-1), G, axis=-1))
    for n in r:
        assert_lane_uniform(r[n], G)


@pytest.mark.parametrize("G", GS)
def test_reductions_nan_semantics(hx, G):
    """A quiet NaN in one lane, in several lanes, in all lanes of every second group: gmax / gmin
    ignore NaN lanes (np.fmax.reduce / np.fmin.reduce) and give NaN only for an all-NaN group, gsum
    gives NaN, and the neighbouring groups keep the bits of the clean run."""
    rng = np.random.default_rng(400 + G)
    groups = cr.n_groups(G)
    v, base, bad = cr.nan_cases(rng, G, groups)
    clean = reduce_run(hx, G, base.reshape(1, -1))
    r = reduce_run(hx, G, v)
    t = cr.expand(v, G, groups).reshape(3, -1, G)
    lane_group = np.minimum(np.arange(t.shape[1] * G) // G, groups - 1)
    is_bad = np.isin(lane_group, bad)
    for n in ("gsum", "n_sum"):
        assert np.isnan(r[n][:, is_bad]).all()
    with np.errstate(invalid="ignore"):
        fmax, fmin = np.fmax.reduce(t, axis=-1), np.fmin.reduce(t, axis=-1)
    assert np.isnan(fmax[2]).any() and not np.isnan(fmax[:2]).any()
    for n, ref in (("gmax", fmax), ("n_max", fmax), ("gmin", fmin), ("n_min", fmin)):
        np.testing.assert_array_equal(r[n], np.repeat(ref, G, axis=-1))  # (NaN == NaN here)
    for n in r:
        assert_lane_uniform(r[n], G)
        for c in range(3):
            same_bits(r[n][c, ~is_bad], clean[n][0, ~is_bad])


# ---------------------------------------------------------------------------------------------
# 2. gall / gany
# ---------------------------------------------------------------------------------------------
def vote_check(hx, G, cond):
    groups = cond.shape[1] // G
    o = hx.group(VOTE, G, cond, out_dtype=np.int32, in_dtype=np.int32)
    cT = cr.expand(cond, G, groups)
    L2 = 64 if G == 32 else G
    np.testing.assert_array_equal(o[:, 0], cr.vote_all(cT, G))
    np.testing.assert_array_equal(o[:, 1], ~cr.vote_all(~cT.astype(bool), G))
    np.testing.assert_array_equal(o[:, 2], cr.vote_all(cT, G, L2))
    np.testing.assert_array_equal(o[:, 3], ~cr.vote_all(~cT.astype(bool), G, L2))
    # gany(c) == !gall(!c): the same launch on the negated conditions
    n = hx.group(VOTE, G, 1 - cond, out_dtype=np.int32, in_dtype=np.int32)
    np.testing.assert_array_equal(o[:, 1], 1 - n[:, 0])
    np.testing.assert_array_equal(o[:, 3], 1 - n[:, 2])
    return o


@pytest.mark.parametrize("G", GS)
def test_votes_single_false_lane_at_every_position(hx, G):
    """"False only at lane k" for every k of the group (a different k in each group of a wave), all
    true, all false, random patterns; for G > 64 a single false lane in each wave in turn.
    gall<32, 64>, the replicated form, is the AND over the whole wave, the same in both halves."""
    rng = np.random.default_rng(500 + G)
    groups = cr.n_groups(G)
    cond = [cr.false_only_at(G, groups), np.ones((1, groups * G), np.int32), np.zeros((1, groups * G), np.int32),
            (rng.random((8, groups * G)) < 0.97).astype(np.int32), (rng.random((4, groups * G)) < 0.5).astype(np.int32)]
    one_true = 1 - cr.false_only_at(G, groups)[::max(1, G // 8)]  # gany's single true lane
    cond.append(one_true)
    if G > 64:
        cond.append(cr.false_in_one_wave(G, groups))
    cond = np.concatenate(cond)
    o = vote_check(hx, G, cond)
    # flag op 3 of greduce_n on the same patterns (its own code: a min chain, or a ballot for a full wave)
    flags = reduce_run(hx, G, np.ones(cond.shape), cond.astype(np.float64))["n_all"]
    np.testing.assert_array_equal(flags, cr.flags_all(cr.expand(cond, G, groups), G))
    np.testing.assert_array_equal(flags, o[:, 0])
    # the first G cases: every group has exactly one false lane, so gall is false on every lane
    assert not o[:G, 0].any() and o[:G, 1].all()
    assert o[G, 0].all() and not o[G + 1, 1].any()


# ---------------------------------------------------------------------------------------------
# 3. moves
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_neighbour_and_lane_moves(hx, G):
    """from_next / from_prev: lane k receives lane k +- 1 of the wave, and wave lane 63 / 0 reads 0.0
    (the bound_ctrl claim; no input is 0).  group_next<G, 1> and <G, 3>: the same, and in multi-wave
    groups lane 63 of wave w < W - 1 receives lane 0 of wave w + 1, the group's last lane 0.0.
    from_lane: a random permutation of the wave's lanes and a broadcast of one lane."""
    rng = np.random.default_rng(600 + G)
    groups = cr.n_groups(G)
    T = cr.n_lanes(G, groups)
    v = rng.uniform(1.0, 2.0, (2, groups * G)) * rng.choice([-1.0, 1.0], (2, groups * G))
    vT = cr.expand(v, G, groups)
    # source lanes are per lane of the launch; the harness reads them through the same group map, so
    # build them per group: a permutation of the wave for G >= 64, of the wave's lanes otherwise
    src = np.empty((2, groups * G), np.int32)
    for g in range(groups):
        src[0, g * G:(g + 1) * G] = np.concatenate([rng.permutation(64) for _ in range(max(1, G // 64))])[:G]
        src[1, g * G:(g + 1) * G] = (11 * g + 5) % 64
    o = hx.group(MOVE, G, v, src, b_dtype=np.int32)
    same_bits(o[:, 0], cr.wave_next(vT))
    same_bits(o[:, 1], cr.wave_prev(vT))
    assert np.all(o[:, 0].reshape(2, -1, 64)[..., 63] == 0.0) and np.all(o[:, 1].reshape(2, -1, 64)[..., 0] == 0.0)
    nxt = cr.group_next(vT, G)
    same_bits(o[:, 2], nxt)
    same_bits(o[:, 3], nxt)
    same_bits(o[:, 4], -nxt + 0.0 * (nxt == 0))  # (-x; the out-of-range lanes read +0.0)
    same_bits(o[:, 5], 2.0 * nxt)
    same_bits(o[:, 6], cr.wave_gather(vT, cr.expand(src, G, groups)))
    assert T % 64 == 0


def test_scan_partners_give_an_inclusive_prefix_scan(hx):
    """scan_partner<D> / scan_takes<D>, D = 1 ... 32, combined as kernels.h and sens.h combine them:
    the prefix sum of integer-valued doubles over the wave equals the exact cumulative sum, and the
    prefix composition of affine maps (exact products and sums; maps do not commute) pins which
    operand is the earlier one."""
    rng = np.random.default_rng(700)
    a, b = cr.scan_inputs(rng, waves=5)
    o = hx.scan(a, b)
    S, A, C = cr.scan_ref(a, b)
    np.testing.assert_array_equal(o[0], S.astype(np.float64))
    np.testing.assert_array_equal(o[0], np.cumsum(a, axis=1))
    np.testing.assert_array_equal(o[1], A.astype(np.float64))
    np.testing.assert_array_equal(o[2], C.astype(np.float64))


# ---------------------------------------------------------------------------------------------
# 4. exchange slots under drift
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [128, 256])
def test_exchange_slots_under_drift(hx, G):
    """200 rounds of gsum, greduce_n, group_next<1>, group_next<3>, gall; before each exchange every
    wave runs a different number of dependent FMAs (fixed by wave index, round and position), and
    each lane's next value is an integer function of all it received.  The final values equal the
    NumPy emulation exactly -- a slot overwritten while a slower wave still reads it would show as a
    wrong value -- and every exchange flips the slot (recorded after each exchange of round 0)."""
    rng = np.random.default_rng(800 + G)
    groups, rounds = 3, 200
    v0 = rng.integers(0, 61, groups * G)
    out, trace, sink = hx.drift(G, v0.astype(np.float64), rounds, work=40)
    ref = cr.drift_ref(v0, G, rounds)
    bad = np.flatnonzero((trace.astype(np.int64) != ref).any(axis=1))
    if len(bad):  # name the first round that differs and its lanes (lane = 64 wave + position)
        r0 = int(bad[0])
        lanes = np.flatnonzero(trace[r0].astype(np.int64) != ref[r0])
        pytest.fail(f"round {r0}: {len(lanes)} lanes differ, first {lanes[:16].tolist()}: device "
                    f"{trace[r0, lanes[:16]].tolist()}, reference {ref[r0, lanes[:16]].tolist()}")
    np.testing.assert_array_equal(out[0].astype(np.int64), ref[-1])
    np.testing.assert_array_equal(out[1:], np.repeat(np.array([1.0, 0.0, 1.0, 0.0, 1.0])[:, None], out.shape[1], axis=1))
    assert np.isfinite(sink).all()


# ---------------------------------------------------------------------------------------------
# 5. element-wise max / min
# ---------------------------------------------------------------------------------------------
def test_elementwise_max_min_are_fmax_fmin(hx):
    """qmax, qmin, qmax_abs equal np.fmax(a, b), np.fmin(a, b), np.fmax(a, |b|) on random values,
    +-0, +-inf and a quiet NaN in either operand or in both (NaN only when both are)."""
    rng = np.random.default_rng(900)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, -5e-324, 1.7976931348623157e308])
    a = np.concatenate([cr.wide_values(rng, 4096), np.repeat(sp, len(sp)), sp, cr.wide_values(rng, len(sp))])
    b = np.concatenate([cr.wide_values(rng, 4096), np.tile(sp, len(sp)), cr.wide_values(rng, len(sp)), sp])
    o = hx.elem(a, b)
    with np.errstate(invalid="ignore"):
        ref = (np.fmax(a, b), np.fmin(a, b), np.fmax(a, np.abs(b)))
    for i, name in enumerate(("qmax", "qmin", "qmax_abs")):
        np.testing.assert_array_equal(o[i], ref[i], err_msg=name)  # values (NaN == NaN, +0 == -0)
        np.testing.assert_array_equal(np.isnan(o[i]), np.isnan(a) & np.isnan(b), err_msg=name)
    # which zero wins for (+0, -0) and (-0, +0): recorded
    for x, y in ((0.0, -0.0), (-0.0, 0.0)):
        j = np.flatnonzero((cr.bits(a) == cr.bits(np.array([x]))[0]) & (cr.bits(b) == cr.bits(np.array([y]))[0]))[0]
        print(f"qmax({x}, {y}) = {o[0, j]}, qmin = {o[1, j]}, qmax_abs = {o[2, j]}")


# ---------------------------------------------------------------------------------------------
# 6. rcp64
# ---------------------------------------------------------------------------------------------
def test_rcp64_within_one_ulp_of_the_correctly_rounded_reciprocal(hx):
    """About 10^5 arguments of both signs, log-uniform over 2^-1021 <= |x| <= 2^1021, and the edge
    arguments (powers of two, their neighbours, 3, 1/3, the largest mantissa): the error against the
    exact 1/x (fractions.Fraction) is at most 1 ulp of the correctly rounded reciprocal -- after the
    two Newton steps the last fma rounds once (1/2 ulp) on a residual error far below 1/2 ulp.
    Measured on one MI355X: see the comment above rcp64."""
    x = cr.rcp_main_arguments(np.random.default_rng(1000))
    assert np.all((np.abs(x) >= 2.0 ** -1021) & (np.abs(x) <= 2.0 ** 1021))
    r = hx.rcp(x)
    err, exact = cr.rcp_ulp_errors(x, r)
    share = float(np.mean(r == exact))
    print(f"rcp64: {len(x)} arguments, max error {err.max():.4f} ulp, correctly rounded {100 * share:.3f} %")
    assert err.max() <= 1.0


def test_rcp64_outside_its_domain(hx):
    """What rcp64 returns outside 2^-1021 <= |x| <= 2^1021, as the comment above it states: NaN -- not
    +-inf or +-0 -- for +-0 and +-inf (fma(-x, r, 1) is 0 * inf), for NaN, and for every x whose
    reciprocal overflows (|x| < 2^-1024: v_rcp_f64 gives inf and the Newton steps turn it into NaN);
    for subnormal x with a finite reciprocal and for |x| > 2^1021 (subnormal reciprocals) still a
    number within one ulp of 1/x.  Every return is printed."""
    nan_x = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -1030, -2.0 ** -1030, 2.0 ** -1024,
             np.nextafter(2.0 ** -1024, 0.0), -2.0 ** -1024]
    num_x = [1.25 * 2.0 ** -1024, 1.5 * 2.0 ** -1024, 2.0 ** -1023, np.nextafter(2.0 ** -1022, 0.0),
             2.0 ** -1022, 2.0 ** 1022, 1.5 * 2.0 ** 1022, 2.0 ** 1023, 1.7976931348623157e308]
    num_x = num_x + [-v for v in num_x]
    x = np.array(nan_x + num_x)
    r = hx.rcp(x)
    for xi, ri in zip(x, r):
        print(f"rcp64({float(xi).hex()}) = {float(ri).hex()}")
    assert np.isnan(r[:len(nan_x)]).all()
    exact = cr.rcp_exact(np.array(num_x))  # (finite: the largest is just below 2^1024)
    got = r[len(nan_x):]
    print(f"rcp64 on {len(num_x)} arguments beyond the main range: {int(np.sum(got == exact))} correctly rounded")
    assert np.all(np.isfinite(exact)) and np.all(np.abs(got - exact) <= np.spacing(np.abs(exact)))
