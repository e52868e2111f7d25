"""The systems tests/test_icp_lane_solve_*.py solve, and a numpy restatement of csrc/icp/solve_lanes.h's schedule:
the pivoted 6x6 LDLT of a pass's close with a row per lane -- the exchanges first, then the elimination -- operation order
included."""
import numpy as np

DBL_MIN = 2.2250738585072014e-308


def systems():
    """(A (2004, 6, 6), b (2004, 6), n_finite): 400 Gauss-Newton matrices each of m = 3, 5, 6, 12, 200 rows with columns
    scaled over six decades (ranks 3, 5 and 6; every pivot choice), then 3 I (ties), the zero matrix, and -- the last
    two -- a system with a NaN entry and one with an infinite entry."""
    rng = np.random.default_rng(20261021)
    As, bs = [], []
    for m in (3, 5, 6, 12, 200):
        for _ in range(400):
            J = rng.normal(size=(m, 6)) * 10.0 ** rng.uniform(-3, 3, 6)
            JtJ = J.T @ J
            As.append((JtJ + JtJ.T) / 2)
            bs.append(rng.normal(size=6))
    n_random = len(As)
    As.append(3.0 * np.eye(6)); bs.append(np.arange(1.0, 7.0))
    As.append(np.zeros((6, 6))); bs.append(np.ones(6))
    bad = As[7].copy(); bad[2, 4] = bad[4, 2] = np.nan
    As.append(bad); bs.append(bs[7].copy())
    bad = As[11].copy(); bad[3, 3] = np.inf
    As.append(bad); bs.append(bs[11].copy())
    return np.array(As), np.array(bs), n_random + 2


def solve6_lanes_ref(Ain, b):
    """x, ok, tr, zero_pivot of the row-per-lane schedule.  The exchanges are played through on the six input diagonals
    first (step k of the elimination writes column k below the diagonal and A[k][k] only, behind its pivot choice, so
    every pivot choice reads input diagonals); position i then holds the row and the columns that end up there, and
    the elimination runs without an exchange.  R[i] is position i's row; what the kernel broadcasts is read from the
    owning row here; every sum runs over j ascending."""
    f = np.float64
    A0 = np.asarray(Ain, np.float64).reshape(6, 6)
    b0 = np.asarray(b, np.float64)
    tr, zero_pivot = [0] * 6, False
    with np.errstate(all="ignore"):
        dv, idx = [abs(A0[i, i]) for i in range(6)], list(range(6))
        for k in range(6):
            p, big = k, dv[k]
            for i in range(k + 1, 6):
                if dv[i] > big:                         # strict: the first of the largest
                    big, p = dv[i], i
            tr[k] = p
            dv[k], dv[p] = dv[p], dv[k]                 # positions k and p change places
            idx[k], idx[p] = idx[p], idx[k]
        R = [[f(A0[idx[i], idx[j]]) for j in range(6)] for i in range(6)]
        y = [f(b0[idx[i]]) for i in range(6)]
        dd = [f(0.0)] * 6
        for k in range(6):
            if k > 0:
                tmp = [dd[j] * R[k][j] for j in range(k)]     # the diagonal, and position k's row broadcast
                for i in range(k, 6):                   # every position at once (those above k write entries nobody reads)
                    u = f(0.0)
                    for j in range(k):
                        u = u + R[i][j] * tmp[j]
                    R[i][k] = R[i][k] - u
            akk = R[k][k]                               # broadcast from position k
            dd[k] = akk
            if abs(akk) > 0.0:
                for i in range(k + 1, 6):
                    R[i][k] = R[i][k] / akk
            else:
                zero_pivot = True
        for j in range(5):                              # forward, by columns
            for i in range(j + 1, 6):
                y[i] = y[i] - R[i][j] * y[j]
        for i in range(6):
            y[i] = y[i] / dd[i] if abs(dd[i]) > DBL_MIN else f(0.0)
        for i in range(5, -1, -1):                      # backward: one chain
            for j in range(i + 1, 6):
                y[i] = y[i] - R[j][i] * y[j]
        x = np.empty(6, np.float64)
        for i in range(6):                              # the exchanges undone
            x[idx[i]] = y[i]
    return x, bool(np.isfinite(x).all()), tr, zero_pivot


def coverage(A, b, n):
    """The (k, p) pivot choices and the count of exactly zero pivots the first n systems take."""
    pairs, zeros = set(), 0
    for s in range(n):
        _, _, tr, zp = solve6_lanes_ref(A[s], b[s])
        pairs.update((k, p) for k, p in enumerate(tr))
        zeros += bool(zp)
    return pairs, zeros


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)
