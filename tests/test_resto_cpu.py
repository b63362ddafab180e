"""CPU: the reference side of the restoration-phase tests (tests/test_gpu_resto_algebra.py,
tests/test_gpu_resto_exits.py).

1. The small dense algebra (tests/helpers/resto_ref.py).  The float64 restatement of resto.h's
   chol_small / chol_solve_small / resto_chol / resto_transform is held, case by case, to the forward
   error bound of a Cholesky solve (resto_ref.a_priori) against the definitions evaluated in exact
   rational arithmetic, on the three regimes and the regular edges.  Measured (300 draws per class
   and NX; error normalised by max |reference| of the case; worst over NX = 3, 4, 6):

   class        Pt (resto_transform's form)   pt        naive P - P S^-1 P
   P huge       1.3e-10 .. 6.4e-10            1.1e-9    1e-6 .. 8e-5  (7e3 .. 2e5 times worse)
   balanced     8e-14 .. 5e-13                3e-14
   D^-1 huge    3.7e-7 .. 2.1e-6              6e-16     <= 1e-16

   so the form "stays accurate when barrier terms make P huge" as resto.h claims, and loses 6 to
   10 digits to cancellation when D^-1 is huge against P (printed by
   test_dinv_huge_loss_is_characterised); its pt is accurate everywhere.

2. The family of infeasible problems (tests/helpers/resto_family.py) on the CPU oracle
   (oracle/ipm_ref.cpp), 72 instances, each under seven scalings of P: every run ends at status 2,
   3, 4 or 5; the end point's constraint violation does not move (largest spread over the scalings
   1 + {0, +-1e-13, 3e-13}: 2.4e-8, cart-pole N = 70, d = 2; below 7e-10 on the unicycle; hence the
   tolerance 2.4e-7 of the device test), while the exit does: 7 of the 72 keep the same (status,
   iterations) under those four scalings and 4 under all seven (6 with the two status-5 instances
   at lo = 0.25: status 4 on the unicycle at N = 2 and 130 and the cart-pole at N = 70, status 5 on
   the 6-state bicycle at N = 20 and the unicycle at N = 20 and 40).  Three instances run into
   status 2 or 5 under some scaling and are left out of the end-point check.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resto_family as rf  # noqa: E402
import resto_ref as rr  # noqa: E402

ALL_CLASSES = list(rr.CLASSES) + ["edges"]


# ------------------------------------------------------------------------------------------
# 1. the algebra
# ------------------------------------------------------------------------------------------
def test_exact_solve_is_exact():
    """The rational Gaussian elimination solves S X = [D^-1 | p] with a zero residual, in
    rational arithmetic, on an ill-conditioned draw of every class."""
    for cls in rr.CLASSES:
        D, P, p = rr.draw(cls, 6, count=2)
        for c in range(2):
            n = 6
            Di = [1 / Fraction(float(d)) for d in D[c]]
            S = [[Fraction(float(P[c, i, j])) + (Di[i] if i == j else 0) for j in range(n)] for i in range(n)]
            R = [[(Di[i] if i == j else Fraction(0)) for j in range(n)] + [Fraction(float(p[c, i]))] for i in range(n)]
            X = rr._solve_exact(S, R)
            for i in range(n):
                for j in range(n + 1):
                    assert sum(S[i][q] * X[q][j] for q in range(n)) == R[i][j]


def test_packing_is_the_devices():
    n = 4
    P = np.arange(16.0).reshape(4, 4)
    P = P + P.T
    pk = rr.pack(P[None])[0]
    assert pk.shape == (10,)
    assert all(pk[rr.symix(i, j, n)] == P[i, j] for i in range(n) for j in range(n))
    assert np.array_equal(rr.unpack(pk[None], n)[0], P)
    # riccati.h symix: row-major upper triangle
    assert [rr.symix(0, 0, 3), rr.symix(0, 2, 3), rr.symix(1, 1, 3), rr.symix(2, 1, 3), rr.symix(2, 2, 3)] == [0, 2, 3, 4, 5]


@pytest.mark.parametrize("nx", rr.NXS)
@pytest.mark.parametrize("cls", ALL_CLASSES)
def test_restatement_against_the_exact_reference(cls, nx):
    (D, P, p), ex, rs, worst = rr.class_case(cls, nx)
    assert np.all(rs["ok"])
    err, bound = rr.errors(rs, ex), rr.a_priori(ex)
    print(f"{cls} NX={nx}: restatement's worst error " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
          "; worst ratio to the a-priori bound " + ", ".join(f"{k} {float((err[k] / bound[k]).max()):.2f}" for k in bound))
    assert worst["Di"] == 0.0  # one IEEE division either way
    for k in bound:
        assert np.all(err[k] <= bound[k]), (k, int(np.argmax(err[k] / bound[k])))


@pytest.mark.parametrize("nx", rr.NXS)
def test_p_huge_class_exercises_the_claim(nx):
    """On the class "P huge" the naive P - P S^-1 P in float64 is at least 1e3 times worse than
    resto_transform's form (worst case of the class against worst case)."""
    (D, P, p), ex, rs, worst = rr.class_case("p_huge", nx)
    naive = rr.rel_err(rr.naive_transform(P, rs["S"]), ex["Pt"])
    print(f"P huge NX={nx}: naive form's worst error {naive.max():.1e}, resto_transform's form {worst['Pt']:.1e} "
          f"(ratio {naive.max() / worst['Pt']:.1e})")
    assert naive.max() >= 1e3 * worst["Pt"]


def test_dinv_huge_loss_is_characterised():
    """What resto.h's comment did not say: with D^-1 huge against P the form D^-1 - D^-1 S^-1 D^-1
    cancels.  Printed per NX: the loss, against the balanced class and against the naive form
    (which is exact to rounding there)."""
    for nx in rr.NXS:
        (D, P, p), ex, rs, worst = rr.class_case("dinv_huge", nx)
        bal = rr.class_case("balanced", nx)[3]
        naive = rr.rel_err(rr.naive_transform(P, rs["S"]), ex["Pt"])
        e = rr.errors(rs, ex)["Pt"]
        print(f"D^-1 huge NX={nx}: Pt error {e.min():.1e} .. {worst['Pt']:.1e} (balanced class: worst {bal['Pt']:.1e}; "
              f"naive form here: worst {naive.max():.1e}); pt {worst['pt']:.1e}")
        assert worst["pt"] <= 64 * rr.EPS  # pt does not cancel


@pytest.mark.parametrize("nx", rr.NXS)
def test_restatement_on_broken_cases(nx):
    """Pivot exactly 0, exactly -2^-40, NaN in P: ok false; with a finite S every output finite
    (chol_small goes on with sqrt(max(d, 1e-300)))."""
    D, P, p, kind = rr.broken_cases(nx)
    Di, S, L, ok = rr.resto_chol(D, P)
    Pt, pt, ok2 = rr.resto_transform(D, P, p)
    x = rr.chol_solve_small(L, p)
    assert not ok.any() and not ok2.any()
    fin = kind < 2
    # the construction is exact: the last pivot is what it was built to be
    piv = S[:, nx - 1, nx - 1] - np.sum(L[:, nx - 1, :nx - 1] ** 2, axis=1)
    assert np.all(piv[kind == 0] == 0.0) and np.all(piv[kind == 1] == -2.0 ** -40)
    assert np.all(L[fin, nx - 1, nx - 1] == 1e-150)
    for a in (L, x, Pt, pt):
        assert np.all(np.isfinite(a[fin]))


# ------------------------------------------------------------------------------------------
# 2. the family of infeasible problems on the oracle
# ------------------------------------------------------------------------------------------
def test_family_lane_groups():
    assert [rf.group_of(N) for N in rf.UNI_N] == [16, 16, 32, 64, 128, 256]


def test_family_on_the_oracle():
    """Every run ends at 2, 3, 4 or 5 within max_iter; the instances left out of the end-point
    check (an oracle run at 2 or 5 under some scaling) are at most a quarter of the family; the
    end point is the geometric minimum for heading 0; the stability filter leaves at least 6
    instances (the two status-5 ones at lo = 0.25 among them), a status-4 one at N >= 64 among
    them."""
    tol, worst = rf.tolerance()
    print(f"largest spread of the oracle's end-point violation over the scalings {rf.SCALINGS}: {worst:.1e}; "
          f"tolerance {tol:.1e}")
    assert 0 < tol <= 1e-5  # a violation is O(1): a tolerance above this would compare nothing
    total = left_out = 0
    stable = []
    for model, N in rf.all_cases():
        c, o = rf.case(model, N), rf.oracle_case(model, N)
        assert o["status"].shape == (len(rf.ALL_SCALINGS), len(c["P"]))
        assert np.all((o["status"] >= 2) & (o["status"] <= 5)), (model, N, o["status"])
        assert np.all(o["iters"] <= rf.MAX_ITER)
        total += len(c["P"])
        left_out += int(np.sum(~o["asserted"]))
        for b in range(len(c["P"])):
            runs = list(zip(o["status"][:, b].tolist(), o["iters"][:, b].tolist()))
            print(f"{c['label'][b]} (G = {c['G']}): {runs} violation {o['viol'][0, b]:.12g} spread {o['spread'][b]:.1e}"
                  f"{' stable' if o['stable'][b] else ''}{'' if o['asserted'][b] else ' (left out)'}")
            if o["stable"][b]:
                stable.append((model, N, int(o["status"][0, b])))
            if model == "unicycle" and c["theta"][b] == 0.0 and o["asserted"][b]:
                assert abs(o["viol"][0, b] - rf.geometric_minimum(c["lo"][b], 0.0)) <= tol
    for N in (20, 40):
        if rf.status5_case(N)[1]["stable"][0]:
            stable.append(("unicycle", N, int(rf.status5_case(N)[1]["status"][0, 0])))
    print(f"{len(stable)} instances keep (status, iterations) under every scaling {rf.ALL_SCALINGS}: {stable}; "
          f"{left_out} of {total} left out of the end-point check")
    assert 4 * left_out <= total
    assert len(stable) >= 6
    assert any(st == 4 and N >= 64 for _, N, st in stable)


def test_status5_and_max_iter_instances_on_the_oracle():
    """The exits the device test compares exactly: the unicycle at theta = 0, lo = 0.25 ends at
    status 5 with the same iteration count under every scaling (N = 20 and 40); an instance with
    max_iter two above the iteration at which restoration is entered ends at status 2 there."""
    for N in (20, 40):
        _, o = rf.status5_case(N)
        print(f"unicycle N={N} theta=0 lo={rf.UNI_LO_HARD}: {list(zip(o['status'][:, 0].tolist(), o['iters'][:, 0].tolist()))}")
        assert np.all(o["status"] == 5) and o["stable"][0]
    c, b, k, st_off, r = rf.max_iter_case()
    print(f"{c['label'][b]}: line search fails at iteration {k} without restoration; max_iter = {k + 2}: status "
          f"{int(r['status'][0])} at {int(r['iters'][0])}")
    assert st_off == 3 and r["status"][0] == 2 and r["iters"][0] == k + 2
