"""Plain NumPy reference of the lane-group collectives (mpc-verde_amd/csrc/collectives.h) for
tests/test_gpu_collectives.py, and the input generators of those tests.  tests/test_collectives_ref_cpu.py
checks this file against exact arithmetic and the generators against the conditions they promise.

Lane layout of the harness (tests/hip/collectives_check.hip): a case is `groups` groups of G lanes;
the kernel runs whole blocks of max(G, 64) lanes, and the surplus lanes of the last block repeat the
last group.  `expand` gives the per-lane view [..., T] of an input [..., groups * G]; every wave-level
reference below works on that view, because DPP moves and ballots do not know about groups.
"""
import math
from fractions import Fraction

import numpy as np

GROUP_SIZES = (16, 32, 64, 128, 256)
U = 2.0 ** -53
QNAN = np.float64("nan")


def n_groups(G):
    """several groups per wave and one wave whose surplus lanes repeat the last group (G <= 64)"""
    return 2 * (64 // G) + 1 if G <= 64 else 3


def n_lanes(G, groups):
    bs = max(G, 64)
    return (groups * G + bs - 1) // bs * bs


def expand(v, G, groups):
    """[..., groups * G] -> [..., T]: the value every lane of the launch reads"""
    v = np.asarray(v)
    assert v.shape[-1] == groups * G
    T = n_lanes(G, groups)
    lane = np.arange(T)
    g = np.minimum(lane // G, groups - 1)
    return v[..., g * G + lane % G]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------
def _wave_levels(G):
    """lane permutations of the in-wave levels a group of min(G, 64) lanes goes through, from the DPP
    controls: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, then the other
    16-lane row of the 32-lane half (permlane16 swap), the other half (permlane32 swap)"""
    i = np.arange(64)
    lv = [i ^ 1, i ^ 2, (i & ~7) | (7 - (i & 7)), (i & ~15) | (15 - (i & 15))]
    if G >= 32:
        lv.append(i ^ 16)
    if G >= 64:
        lv.append(i ^ 32)
    return lv


def wave_reduce(v, G, op):
    """[..., 64] -> [..., 64]: what every lane of a wave holds after the in-wave levels; op(a, b) is
    commutative, so lane and partner compute the same bits"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in _wave_levels(G):
            v = op(v, v[..., p])
    return v


def group_reduce(vT, G, op):
    """per-lane result [..., T] of greduce<G, op> on the lane view [..., T]: the in-wave tree, then for
    multi-wave groups the waves' partial results combined left to right"""
    vT = np.asarray(vT, dtype=np.float64)
    T = vT.shape[-1]
    w = wave_reduce(vT.reshape(vT.shape[:-1] + (T // 64, 64)), G, op)
    if G <= 64:
        return w.reshape(vT.shape)
    W = G // 64
    part = w[..., 0].reshape(vT.shape[:-1] + (T // G, W))  # lane 0 of every wave
    with np.errstate(invalid="ignore", over="ignore"):
        r = part[..., 0]
        for j in range(1, W):
            r = op(r, part[..., j])
    return np.repeat(r, G, axis=-1)


def tree_sum(vT, G):
    return group_reduce(vT, G, np.add)


def sum_depth(G):
    """roundings on the path of one input through the prescribed order"""
    return int(math.log2(min(G, 64))) + (G // 64 - 1 if G > 64 else 0)


def gamma(G):
    d = sum_depth(G)
    return d * U / (1 - d * U)


def exact_sums(v, G):
    """[..., n * G] -> (fsum of every group, fsum of |.| of every group)"""
    g = np.asarray(v, dtype=np.float64).reshape(-1, G)
    s = np.array([math.fsum(r) for r in g])
    a = np.array([math.fsum(np.abs(r)) for r in g])
    return s, a


def flags_all(fT, G):
    """op 3 of greduce_n: 1.0 on every lane of a group iff every lane holds 1.0 (the ballot form of a
    full wave counts the wave's lanes; multi-wave groups take the minimum of the waves' answers)"""
    fT = np.asarray(fT)
    ok = (fT > 0.5).reshape(fT.shape[:-1] + (-1, min(G, 64)))
    r = np.repeat(ok.all(axis=-1), min(G, 64), axis=-1)
    if G > 64:
        r = np.repeat(r.reshape(fT.shape[:-1] + (-1, G)).all(axis=-1), G, axis=-1)
    return r.astype(np.float64)


def vote_all(cT, G, L=None):
    """gall<G, L>: AND over the L = G lanes of the group, or over the whole wave for L = 64"""
    L = G if L is None else L
    c = np.asarray(cT).astype(bool)
    return np.repeat(c.reshape(c.shape[:-1] + (-1, L)).all(axis=-1), L, axis=-1)


# ------------------------------------------------------------------------------------------------
# moves
# ------------------------------------------------------------------------------------------------
def wave_next(vT):
    """from_next: lane k of a wave receives lane k + 1; lane 63 reads 0.0 (bound_ctrl)"""
    w = np.asarray(vT, dtype=np.float64).reshape(vT.shape[:-1] + (-1, 64))
    out = np.zeros_like(w)
    out[..., :-1] = w[..., 1:]
    return out.reshape(vT.shape)


def wave_prev(vT):
    w = np.asarray(vT, dtype=np.float64).reshape(vT.shape[:-1] + (-1, 64))
    out = np.zeros_like(w)
    out[..., 1:] = w[..., :-1]
    return out.reshape(vT.shape)


def group_next(vT, G):
    """group_next: from_next, and for multi-wave groups lane 63 of wave w < W - 1 receives lane 0 of
    wave w + 1 of the same group; the last lane of the group's last wave reads 0.0"""
    if G <= 64:
        return wave_next(vT)
    g = np.asarray(vT, dtype=np.float64).reshape(vT.shape[:-1] + (-1, G))
    out = np.zeros_like(g)
    out[..., :-1] = g[..., 1:]
    return out.reshape(vT.shape)


def wave_gather(vT, src):
    """from_lane: lane l receives lane src[l] & 63 of its wave"""
    w = np.asarray(vT).reshape(vT.shape[:-1] + (-1, 64))
    s = (np.asarray(src) & 63).reshape(w.shape)
    return np.take_along_axis(w, s, axis=-1).reshape(vT.shape)


def scan_inputs(rng, waves, twos=16):
    """integer-valued affine maps x -> a x + b per lane whose every composition over a lane range of
    the wave is exact in float64: a in {1, -1, 2, -2} with at most `twos` factors of +-2 per wave,
    |b| <= 8, so every coefficient is an integer below 2^twos * 8 * 64 << 2^53"""
    a = rng.choice([1.0, -1.0], size=(waves, 64))
    for w in range(waves):
        a[w, rng.choice(64, size=twos, replace=False)] *= 2.0
    b = rng.integers(-8, 9, size=(waves, 64)).astype(np.float64)
    return a, b


def scan_ref(a, b):
    """inclusive prefix over each wave in exact integers: lane k holds T_k o ... o T_0 with
    T_j(x) = a_j x + b_j (the later map applied after the earlier ones); returns (cumsum a, A, C)"""
    a, b = np.asarray(a), np.asarray(b)
    A = np.empty(a.shape, dtype=object)
    C = np.empty(a.shape, dtype=object)
    S = np.empty(a.shape, dtype=object)
    for w in range(a.shape[0]):
        pa, pc, ps = 1, 0, 0
        for k in range(64):
            ak, bk = int(a[w, k]), int(b[w, k])
            pa, pc, ps = ak * pa, ak * pc + bk, ps + ak
            A[w, k], C[w, k], S[w, k] = pa, pc, ps
    return S, A, C


# ------------------------------------------------------------------------------------------------
# exchange slots under drift (collectives_check.hip drift_kernel, the same sequence)
# ------------------------------------------------------------------------------------------------
def drift_ref(v0, G, rounds):
    """v0 [groups * G] integers in [0, 61) -> values after every round [rounds, groups * G] (int64)"""
    x = np.asarray(v0, dtype=np.int64).reshape(-1, G).copy()
    k = np.arange(G, dtype=np.int64)[None, :]
    hist = []

    def nxt(v):
        o = np.zeros_like(v)
        o[:, :-1] = v[:, 1:]
        return o

    for r in range(rounds):
        s = x.sum(axis=1, keepdims=True)
        t0, t1, t2 = s, x.max(axis=1, keepdims=True), x.min(axis=1, keepdims=True)
        t3 = (x != (r * 7) % 61).all(axis=1, keepdims=True).astype(np.int64)
        n1 = nxt(x)
        n30, n31, n32 = nxt(x + 1), nxt(2 * x), nxt(x + s)
        a = (x != (r * 11 + 3) % 61).all(axis=1, keepdims=True)
        acc = (3 * x + s + 5 * t0 + 7 * t1 + 11 * t2 + 13 * t3 + 17 * n1 + 19 * n30 + 23 * n31 + 29 * n32
               + np.where(a, 31, 0) + k + r)
        x = acc % 61
        hist.append(x.reshape(-1).copy())
    return np.array(hist)


# ------------------------------------------------------------------------------------------------
# input generators
# ------------------------------------------------------------------------------------------------
def wide_values(rng, shape):
    """normal * 10^U(-8, 8): sixteen decades of magnitude, both signs"""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-8, 8, size=shape)


def small_integers(rng, shape):
    """integer-valued doubles in [-1000, 1000]: every partial sum of up to 256 of them is exact"""
    return rng.integers(-1000, 1001, size=shape).astype(np.float64)


def zero_mix(rng, shape):
    """+0 and -0 at random"""
    return np.where(rng.random(shape) < 0.5, 0.0, -0.0)


def inf_cases(rng, G, groups):
    """[3, groups * G]: +inf in one lane of every group, -inf in one lane, and both (sum NaN)"""
    v = wide_values(rng, (3, groups, G))
    for g in range(groups):
        p, q = rng.choice(G, size=2, replace=False)
        v[0, g, p] = np.inf
        v[1, g, q] = -np.inf
        v[2, g, p], v[2, g, q] = np.inf, -np.inf
    return v.reshape(3, groups * G)


def nan_cases(rng, G, groups):
    """[3, groups * G] and the poisoned groups: a quiet NaN in one lane, in several lanes and in all
    lanes of every second group (groups 0, 2, ...: each shares its wave with a clean neighbour when
    G < 64); the other groups hold the same data in all three cases"""
    base = wide_values(rng, (groups, G))
    v = np.repeat(base[None], 3, axis=0)
    bad = np.arange(0, groups, 2)
    for g in bad:
        v[0, g, rng.integers(G)] = QNAN
        v[1, g, rng.choice(G, size=5, replace=False)] = QNAN
        v[2, g, :] = QNAN
    return v.reshape(3, groups * G), base.reshape(groups * G), bad


def false_only_at(G, groups):
    """[G, groups * G] conditions: case c is true everywhere except lane (c + 5 g) % G of group g -- over
    the G cases every lane position of every group is the false one once, and the groups that share
    a wave have different positions in the same case"""
    c = np.ones((G, groups, G), dtype=np.int32)
    for case in range(G):
        for g in range(groups):
            c[case, g, (case + 5 * g) % G] = 0
    return c.reshape(G, groups * G)


def false_in_one_wave(G, groups):
    """G > 64: [W * groups, groups * G]: one false lane, in wave w of group g only"""
    W = G // 64
    c = np.ones((W * groups, groups, G), dtype=np.int32)
    for g in range(groups):
        for w in range(W):
            c[g * W + w, g, 64 * w + (7 * w + 3 * g + 1) % 64] = 0
    return c.reshape(W * groups, groups * G)


# ------------------------------------------------------------------------------------------------
# rcp64
# ------------------------------------------------------------------------------------------------
def rcp_main_arguments(rng, n=100_000):
    """n arguments of both signs, log-uniform over 2^-1021 <= |x| <= 2^1021, then the edge arguments:
    powers of two, their neighbours one ulp up and down, 3, 1/3 and the largest mantissa, scaled
    over the range"""
    e = rng.integers(-1021, 1021, size=n)
    x = np.ldexp(rng.uniform(1.0, 2.0, size=n), e) * rng.choice([-1.0, 1.0], size=n)
    edge = [3.0, 1.0 / 3.0]
    for k in (-1021, -1020, -1000, -512, -53, -1, 0, 1, 52, 53, 511, 1000, 1020):
        p = math.ldexp(1.0, k)
        edge += [p, np.nextafter(p, np.inf), np.nextafter(2.0 * p, 0.0), 1.5 * p, p * (4.0 / 3.0)]
        if k > -1021:
            edge.append(np.nextafter(p, 0.0))
    edge = np.array(edge + [2.0 ** 1021])
    return np.concatenate([x, edge, -edge])


def rcp_exact(x):
    """the correctly rounded 1 / x from exact rational arithmetic"""
    return np.array([float(1 / Fraction(float(v))) for v in np.asarray(x).reshape(-1)]).reshape(np.shape(x))


def ulp_of(y):
    """unit in the last place of the binade of y (finite, nonzero, normal)"""
    return np.ldexp(1.0, np.frexp(np.abs(y))[1] - 53)


def rcp_ulp_errors(x, r):
    """|r - 1/x| in ulps of the correctly rounded 1/x, exactly (rational arithmetic)"""
    cr = rcp_exact(x)
    ulp = ulp_of(cr)
    out = np.empty(len(x))
    for i, (xi, ri, ui) in enumerate(zip(x, r, ulp)):
        if not math.isfinite(ri):
            out[i] = math.inf
        else:
            out[i] = float(abs(Fraction(float(ri)) - 1 / Fraction(float(xi))) / Fraction(float(ui)))
    return out, cr
