"""tests/helpers/collectives_ref.py -- the reference and the input generators of
tests/test_gpu_collectives.py -- against exact arithmetic and naive restatements, on the CPU."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import collectives_ref as cr  # noqa: E402

GS = cr.GROUP_SIZES


def pairwise(v):
    """balanced pairwise sum in lane order, written as the recursion"""
    if len(v) == 1:
        return v[0]
    h = len(v) // 2
    return pairwise(v[:h]) + pairwise(v[h:])


@pytest.mark.parametrize("G", GS)
def test_layout_and_expand(G):
    groups = cr.n_groups(G)
    T = cr.n_lanes(G, groups)
    assert T % max(G, 64) == 0 and T >= groups * G
    assert (T > groups * G) == (G < 64)  # 16 and 32: one wave with surplus lanes
    if G < 64:
        assert groups * G // 64 >= 2 and 64 // G >= 2  # whole waves with several groups each
    v = np.arange(groups * G, dtype=np.float64)
    e = cr.expand(v, G, groups)
    np.testing.assert_array_equal(e[:groups * G], v)
    np.testing.assert_array_equal(e[groups * G:].reshape(-1, G), np.tile(v[-G:], ((T - groups * G) // G, 1)))


@pytest.mark.parametrize("G", GS)
def test_tree_sum_is_the_pairwise_tree_and_meets_its_bound(G):
    """The permutation form of the in-wave levels is the balanced pairwise tree in lane order, waves
    added left to right; its error on normal * 10^U(-8, 8) inputs stays below gamma_d sum|v|."""
    rng = np.random.default_rng(G)
    groups = cr.n_groups(G)
    v = cr.wide_values(rng, (20, groups * G))
    assert np.log10(np.abs(v).max() / np.abs(v).min()) > 12 and (v > 0).any() and (v < 0).any()
    vT = cr.expand(v, G, groups)
    s = cr.tree_sum(vT, G)
    for row_in, row_out in zip(vT.reshape(-1, G), s.reshape(-1, G)):
        waves = [pairwise(list(row_in[i:i + 64])) for i in range(0, G, 64)] if G > 64 else [pairwise(list(row_in))]
        ref = waves[0]
        for w in waves[1:]:
            ref = ref + w
        assert np.all(cr.bits(row_out) == cr.bits(np.array([ref]))[0])
    exact, absum = cr.exact_sums(vT, G)
    ratio = np.abs(s.reshape(-1, G)[:, 0] - exact) / (cr.gamma(G) * absum)
    assert ratio.max() <= 1.0
    d = cr.sum_depth(G)
    assert d == {16: 4, 32: 5, 64: 6, 128: 7, 256: 9}[G]
    assert cr.gamma(G) == d * 2.0 ** -53 / (1 - d * 2.0 ** -53)


def test_max_min_and_flag_references():
    rng = np.random.default_rng(1)
    for G in GS:
        groups = cr.n_groups(G)
        vT = cr.expand(cr.wide_values(rng, (3, groups * G)), G, groups)
        np.testing.assert_array_equal(cr.group_reduce(vT, G, np.fmax), np.repeat(vT.reshape(3, -1, G).max(-1), G, -1))
        np.testing.assert_array_equal(cr.group_reduce(vT, G, np.fmin), np.repeat(vT.reshape(3, -1, G).min(-1), G, -1))
        f = (rng.random((40, groups * G)) < 0.995).astype(np.float64)
        fT = cr.expand(f, G, groups)
        ref = np.array([[float(all(row[g * G:(g + 1) * G] == 1.0)) for g in range(len(row) // G) for _ in range(G)]
                        for row in fT])
        np.testing.assert_array_equal(cr.flags_all(fT, G), ref)
        assert ref.any() and not ref.all()
        c = fT.astype(np.int32)
        np.testing.assert_array_equal(cr.vote_all(c, G), ref.astype(bool))
        if G == 32:
            w = np.array([[all(row[i // 64 * 64:i // 64 * 64 + 64]) for i in range(len(row))] for row in c])
            np.testing.assert_array_equal(cr.vote_all(c, G, 64), w)


@pytest.mark.parametrize("G", GS)
def test_input_generators_meet_their_conditions(G):
    rng = np.random.default_rng(10 + G)
    groups = cr.n_groups(G)
    per_wave = max(1, 64 // G)
    # integers: every partial sum exact
    vi = cr.small_integers(rng, (3, groups * G))
    assert np.all(vi == np.round(vi)) and np.abs(vi).max() * 256 < 2.0 ** 53
    # zeros of both signs in every case
    z = cr.zero_mix(rng, (4, groups * G))
    assert np.all(z == 0) and np.signbit(z).any(axis=1).all() and (~np.signbit(z)).any(axis=1).all()
    # infinities
    vf = cr.inf_cases(rng, G, groups).reshape(3, groups, G)
    assert np.all((vf[0] == np.inf).sum(-1) == 1) and not (vf[0] == -np.inf).any()
    assert np.all((vf[1] == -np.inf).sum(-1) == 1) and not (vf[1] == np.inf).any()
    assert np.all((vf[2] == np.inf).sum(-1) == 1) and np.all((vf[2] == -np.inf).sum(-1) == 1)
    assert not np.isnan(vf).any()
    # NaNs: one lane, several lanes, all lanes of the poisoned groups; clean groups untouched; a
    # poisoned group shares its wave with a clean one wherever several groups share a wave
    v, base, bad = cr.nan_cases(rng, G, groups)
    v, base = v.reshape(3, groups, G), base.reshape(groups, G)
    n = np.isnan(v).sum(-1)
    clean = np.setdiff1d(np.arange(groups), bad)
    assert np.all(n[0, bad] == 1) and np.all(n[1, bad] == 5) and np.all(n[2, bad] == G) and not n[:, clean].any()
    np.testing.assert_array_equal(v[:, clean], np.repeat(base[None, clean], 3, axis=0))
    assert len(clean) >= 1 and not np.isnan(base).any()
    if per_wave > 1:
        assert all(any(c // per_wave == b // per_wave for c in clean) for b in bad if b < groups - 1)
    # single false lane: every (group, position) once; different positions inside a wave
    c = cr.false_only_at(G, groups).reshape(G, groups, G)
    assert np.all((c == 0).sum(-1) == 1)
    pos = np.argmin(c, axis=-1)  # [case, group]
    for g in range(groups):
        assert sorted(pos[:, g]) == list(range(G))
    for w in range(0, groups - per_wave + 1, per_wave):
        if per_wave > 1:
            assert all(len(set(p[w:w + per_wave])) == per_wave for p in pos)
    if G > 64:
        W = G // 64
        cw = cr.false_in_one_wave(G, groups).reshape(W * groups, groups, W, 64)
        assert np.all((cw == 0).sum(axis=(1, 2, 3)) == 1)
        hit = {(int(g), int(w)) for case in cw for g, w, _ in np.argwhere(case == 0)}
        assert hit == {(g, w) for g in range(groups) for w in range(W)}


def test_move_references():
    rng = np.random.default_rng(3)
    for G in GS:
        groups = cr.n_groups(G)
        T = cr.n_lanes(G, groups)
        v = rng.uniform(1, 2, (2, T))
        nx, pv, gn = cr.wave_next(v), cr.wave_prev(v), cr.group_next(v, G)
        for i in range(T):
            assert np.all(nx[:, i] == (v[:, i + 1] if i % 64 != 63 else 0.0))
            assert np.all(pv[:, i] == (v[:, i - 1] if i % 64 != 0 else 0.0))
            assert np.all(gn[:, i] == (v[:, i + 1] if i % max(G, 64) != max(G, 64) - 1 else 0.0))
        src = rng.integers(0, 64, (2, T))
        ga = cr.wave_gather(v, src)
        for i in range(T):
            assert np.all(ga[:, i] == v[np.arange(2), i // 64 * 64 + src[:, i]])


def test_scan_inputs_are_exact_and_the_reference_is_the_composition():
    rng = np.random.default_rng(4)
    a, b = cr.scan_inputs(rng, waves=5)
    assert np.all(np.isin(np.abs(a), (1.0, 2.0))) and np.all((np.abs(a) == 2.0).sum(1) == 16) and (a < 0).any()
    assert np.all(b == np.round(b)) and np.abs(b).max() <= 8
    # every composition over a lane range has integer coefficients below 2^16 * 8 * 64 < 2^53
    assert 2 ** 16 * 8 * 64 < 2 ** 53
    S, A, C = cr.scan_ref(a, b)
    assert max(abs(int(x)) for x in C.reshape(-1)) < 2 ** 53 and max(abs(int(x)) for x in A.reshape(-1)) < 2 ** 53
    for w in range(a.shape[0]):
        for x0 in (0, 1, -3):
            x = Fraction(x0)
            for k in range(64):
                x = Fraction(a[w, k]) * x + Fraction(b[w, k])  # T_k after T_{k-1} ... T_0
                assert x == A[w, k] * x0 + C[w, k]
    np.testing.assert_array_equal(S.astype(np.float64), np.cumsum(a, axis=1))
    # the maps do not commute: composing in the opposite order gives another constant term
    rev = [0] * a.shape[0]
    for w in range(a.shape[0]):
        c = 0
        for k in reversed(range(64)):
            c = int(a[w, k]) * c + int(b[w, k])
        rev[w] = c
    assert all(rev[w] != C[w, 63] for w in range(a.shape[0]))


@pytest.mark.parametrize("G", [128, 256])
def test_drift_reference(G):
    """the vectorised emulation against a lane-by-lane restatement; values stay in [0, 61); both
    outcomes of the flag reduction and of the vote occur in the 200 rounds"""
    rng = np.random.default_rng(5 + G)
    groups = 3
    v0 = rng.integers(0, 61, groups * G)
    x = [list(map(int, v0[g * G:(g + 1) * G])) for g in range(groups)]
    seen_f, seen_a = set(), set()
    for r in range(200):
        for g in range(groups):
            xs = x[g]
            s, mx, mn = sum(xs), max(xs), min(xs)
            f = int(all(v != (r * 7) % 61 for v in xs))
            a = all(v != (r * 11 + 3) % 61 for v in xs)
            seen_f.add(f)
            seen_a.add(a)
            new = []
            for k in range(G):
                n = xs[k + 1] if k + 1 < G else None
                n1, n30, n31, n32 = (n, n + 1, 2 * n, n + s) if n is not None else (0, 0, 0, 0)
                acc = (3 * xs[k] + s + 5 * s + 7 * mx + 11 * mn + 13 * f + 17 * n1 + 19 * n30 + 23 * n31 + 29 * n32
                       + (31 if a else 0) + k + r)
                new.append(acc % 61)
            x[g] = new
        if r in (0, 6, 199):
            np.testing.assert_array_equal(cr.drift_ref(v0, G, r + 1)[-1], np.array(x).reshape(-1))
    assert seen_f == {0, 1} and seen_a == {False, True}
    assert 0 <= min(map(min, x)) and max(map(max, x)) < 61


def test_rcp_reference_and_arguments():
    """The Fraction route gives the correctly rounded reciprocal: it equals IEEE division (correctly
    rounded by definition) on a sample and on every edge argument; the exact error measure gives at
    most 1/2 ulp for it and between 1/2 and 3/2 for its neighbours."""
    x = cr.rcp_main_arguments(np.random.default_rng(6), n=5000)
    assert np.all((np.abs(x) >= 2.0 ** -1021) & (np.abs(x) <= 2.0 ** 1021)) and (x > 0).any() and (x < 0).any()
    e = np.frexp(np.abs(x[:5000]))[1]
    assert e.min() < -900 and e.max() > 900  # log-uniform over the range
    for p in (1.0, 2.0 ** -1021, 2.0 ** 1021, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 3.0, 1.0 / 3.0,
              np.nextafter(2.0, 0.0)):
        assert p in x and -p in x
    ref = cr.rcp_exact(x)
    np.testing.assert_array_equal(ref, 1.0 / x)
    assert np.all(np.isfinite(ref)) and np.all(np.abs(ref) >= 2.0 ** -1022)  # results are normal numbers
    err, ref2 = cr.rcp_ulp_errors(x, ref)
    np.testing.assert_array_equal(ref2, ref)
    assert err.max() <= 0.5
    up, _ = cr.rcp_ulp_errors(x, np.nextafter(ref, np.inf))
    dn, _ = cr.rcp_ulp_errors(x, np.nextafter(ref, -np.inf))
    interior = np.frexp(np.abs(ref))[0] != 0.5  # (below a power of two the spacing halves)
    assert np.all(up[interior] >= 0.5) and np.all(up[interior] <= 1.5)
    assert np.all(dn[interior] >= 0.5) and np.all(dn[interior] <= 1.5)
    assert np.all(np.minimum(up, dn)[interior] <= 1.0)
    # an exact case by hand: 1/3 rounds to 0x3FD5555555555555, error 1/3 ulp
    e3, r3 = cr.rcp_ulp_errors(np.array([3.0]), np.array([1.0 / 3.0]))
    assert r3[0].hex() == "0x1.5555555555555p-2" and abs(e3[0] - 1.0 / 3.0) < 1e-12
    assert math.isinf(cr.rcp_ulp_errors(np.array([3.0]), np.array([np.nan]))[0][0])
