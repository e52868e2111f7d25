"""The certificate rule of the fused ICP pass, restated in numpy and checked against a k-d tree (CPU).

Pass p finds a slot's nearest neighbour at distance d1 inside the search radius rho = KAPPA d1 and bounds every other
target point from below by L = min(rho, second nearest distance); the certificate is c = L rounded down to float32.
The point then moves by m: c' = c - m, rounded down, and the slot is certified when the distance to the old neighbour,
rounded up, is strictly below c'.  The claim: a certified slot's old neighbour is the unique nearest neighbour of the
moved point.  (The kernel's L is looser -- its second nearest distance is itself a lower bound -- so what holds here
holds there; that the kernel's bounds are lower bounds is what tests/test_icp_certificate_gpu.py's byte comparisons see.)"""
import numpy as np
import pytest
from scipy import spatial as scipy_spatial

KAPPA = (1.25, 1.5, 2.0)
DOWN, UP = 1.0 - 2e-7, 1.0 + 1e-12  # rounding down to float32; covering float64's own roundings


def certificate(d1, d2, kappa):
    rho = (kappa * (d1.astype(np.float32) * np.float32(1.00001))).astype(np.float64)
    L = np.minimum(rho, d2)
    return (L * DOWN).astype(np.float32)


def certified(c, m, dprev):
    c_new = ((c.astype(np.float64) - m * UP) * DOWN).astype(np.float32)
    ok = np.isfinite(c_new) & np.isfinite(dprev) & (c_new > 0) & (dprev * UP < c_new.astype(np.float64))
    return ok, np.where(ok, c_new, np.float32(0))


@pytest.mark.parametrize("kappa", KAPPA)
def test_certified_slots_keep_their_unique_nearest_neighbour(kappa):
    rng = np.random.default_rng(int(kappa * 100))
    tgt = rng.normal(0.0, 1.0, (20000, 3))
    tgt[1000:1200] = tgt[:200]  # exact duplicates: two-way ties at every distance
    tree = scipy_spatial.cKDTree(tgt)
    n = 100000
    p = tgt[rng.integers(0, len(tgt), n)] + rng.normal(0.0, 0.01, (n, 3))
    d, j = tree.query(p, k=2)
    c = certificate(d[:, 0], d[:, 1], kappa)
    # motions from far below to far above the margins the certificates leave (the scene's second neighbour is 0.05 away)
    step = 10.0 ** rng.uniform(-7.0, -1.0, n)
    v = rng.normal(size=(n, 3))
    q = p + v / np.linalg.norm(v, axis=1, keepdims=True) * step[:, None]
    m = np.sqrt(((q - p) ** 2).sum(1))
    dprev = np.sqrt(((q - tgt[j[:, 0]]) ** 2).sum(1))
    ok, c_new = certified(c, m, dprev)
    d_after, j_after = tree.query(q, k=2)
    assert 0.1 * n < ok.sum() < 0.99 * n, ok.sum()  # both outcomes are on trial
    assert np.array_equal(j_after[ok, 0], j[ok, 0])
    assert (d_after[ok, 0] < d_after[ok, 1]).all()
    assert np.array_equal(d_after[ok, 0], dprev[ok])
    tied = d[:, 0] == d[:, 1]
    assert tied.sum() > 100 and not ok[tied].any()
    # the bound carried over is a bound again: a second move is judged by c_new
    assert (c_new[ok].astype(np.float64) <= d_after[ok, 1]).all()


def test_nothing_certifies_without_a_neighbour_or_a_bound():
    z = np.zeros(4, np.float32)
    nan = np.full(4, np.nan)
    assert not certified(z, np.zeros(4), np.full(4, 1e-3))[0].any()
    assert not certified(np.ones(4, np.float32), np.zeros(4), nan)[0].any()
    assert not certified(np.ones(4, np.float32), nan, np.full(4, 1e-3))[0].any()
    assert not certified(np.full(4, np.inf, np.float32), np.zeros(4), np.full(4, 1e-3))[0].any()
