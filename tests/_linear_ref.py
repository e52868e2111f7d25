"""Shared by the linear-layer tests: inputs, the float64 references with DESIGN.md s4.14's error bounds, and numpy emulations
of the kernels' arithmetic (float16 operands, float32 accumulation over K in the kernel's order of 32-wide steps, float32
epilogue, one rounding) with switches for the designed faults.

With a position table the A operand is xa = half(float32(x) + pos[r % S]) in the emulation AND in the reference: the
reference is taken after that rounding, so the bounds carry no term for it."""
import numpy as np

PLAIN, RELU, ADD_LN = 0, 1, 2
U32, U16 = 2.0 ** -24, 2.0 ** -11      # unit roundoffs of float32 and float16
LN_N = 512
EPS = 1e-5


def inputs(M, K, N, seed=0, S=None, x_ld=None):
    """Gaussian operands of a call: x M x K float16 (with x_ld > K the [:, :K] view of an M x x_ld array), w N x K float16
    ~ N(0, 1.5^2 / K), bias, gamma, beta float32, res M x N float16, and with S a table `pos` of max(M, S) + 1 rows x
    max(K, N) float32 in [-1, 1] whose rows all differ."""
    rng = np.random.default_rng(seed)
    wide = rng.standard_normal((M, x_ld or K)).astype(np.float16)
    d = {"x": wide[:, :K], "w": (rng.standard_normal((N, K)) * 1.5 / np.sqrt(K)).astype(np.float16),
         "bias": (0.3 * rng.standard_normal(N)).astype(np.float32), "res": rng.standard_normal((M, N)).astype(np.float16),
         "gamma": (1 + 0.3 * rng.standard_normal(N)).astype(np.float32), "beta": (0.2 * rng.standard_normal(N)).astype(np.float32)}
    if S is not None:
        r, c = np.arange(max(M, S) + 1)[:, None], np.arange(max(K, N))[None]
        d["pos"] = np.sin(0.37 * r + 0.011 * c * (r + 1)).astype(np.float32)
    return d


def integer_inputs(M, K, N, seed=0):
    """Operands whose product float32 holds exactly in any order of the sums and float16 holds exactly as a result: x with
    integers -2 .. 2, w with -1, 0, 1, no bias.  Every partial sum is an integer of at most 2 K < 2^24."""
    rng = np.random.default_rng(seed)
    return {"x": rng.integers(-2, 3, (M, K)).astype(np.float16), "w": rng.integers(-1, 2, (N, K)).astype(np.float16), "bias": None}


def sparse_inputs(M, K, N, seed=0, S=None, every=32):
    """inputs() with one entry of x kept in every `every` columns (at a place drawn per row and group) and zeros elsewhere,
    and w ~ N(0, 0.15^2 / (K / every)): every K tile still adds to the product, its standard deviation is 0.15 next to the
    residual's 1, and sum_k |x| |w|, the term the bound's (K + 3) 2^-24 multiplies, is that of a product K / every long.
    For a large K, where the bound on dense operands is far above what a kernel with a designed fault does."""
    d = inputs(M, K, N, seed, S)
    rng = np.random.default_rng(seed + 1)
    groups = K // every
    at = rng.integers(0, every, (M, groups)) + every * np.arange(groups)[None]
    keep = np.zeros((M, K), bool)
    keep[np.arange(M)[:, None], at] = True
    d["x"] = np.where(keep, d["x"], np.float16(0))
    d["w"] = (d["w"].astype(np.float32) * (0.1 * np.sqrt(every))).astype(np.float16)
    return d


def operand(x, pos=None, S=None, no_wrap=False):
    """The A operand as float16: x, or half(float32(x) + pos[r % S]) (no_wrap: pos[r], the designed fault)."""
    x = np.asarray(x, np.float16)
    if pos is None:
        return x
    r = np.arange(len(x))
    rows = pos[r if no_wrap else r % S, :x.shape[1]]
    return (x.astype(np.float32) + rows).astype(np.float16)


def _res(res, pos, S, no_wrap=False):
    r = np.arange(len(res))
    return res if pos is None else res + pos[r if no_wrap else r % S, :res.shape[1]]


def reference(x, w, bias, epilogue, res=None, pos=None, S=None, gamma=None, beta=None, eps=EPS, pos_a=True):
    """(y_ref, bound), float64.  PLAIN / RELU, per element:
        |y - y_ref| <= (K + 3) 2^-24 (sum_k |xa| |w| + |b|) + 2^-11 |y_ref| + 2^-24.
    ADD_LN, with v = res' + xa.w + b, g the float32 error of v (the product's term above plus 2^-23 (|res| + |pos| + |v|)),
    G = max_n g, s = sqrt(var + eps), z = (v - mean) / s and D = 2 G + N 2^-24 mean|v| + 2^-24 max|v - mean| the error
    of a centred element:
        |y - y_ref| <= |gamma| ((1 + |z|) D / s / (1 - D / s) + |z| (N / 2 + 8) 2^-24) + 2^-23 (|gamma z| + |beta|)
                       + 2^-11 |y_ref| + 2^-24."""
    K = x.shape[1]
    ln = epilogue == ADD_LN
    xa = operand(x, pos if (not ln or pos_a) else None, S).astype(np.float64)
    w64 = np.asarray(w, np.float16).astype(np.float64)
    b = np.zeros(len(w64)) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    lin = xa @ w64.T + b
    gemm = (K + 3) * U32 * (np.abs(xa) @ np.abs(w64).T + np.abs(b))
    if not ln:
        y = np.maximum(lin, 0) if epilogue == RELU else lin
        return y, gemm + U16 * np.abs(y) + U32
    N = lin.shape[1]
    r16 = np.asarray(res, np.float16).astype(np.float64)
    rp = _res(r16, None if pos is None else pos.astype(np.float64), S)
    v = rp + lin
    g = gemm + 2 * U32 * (np.abs(r16) + np.abs(rp - r16) + np.abs(v))
    mean = v.mean(1, keepdims=True)
    d = v - mean
    s = np.sqrt((d * d).mean(1, keepdims=True) + eps)
    z = d / s
    ga = np.asarray(gamma, np.float32).astype(np.float64)
    be = np.zeros(N) if beta is None else np.asarray(beta, np.float32).astype(np.float64)
    y = z * ga + be
    D = 2 * g.max(1, keepdims=True) + N * U32 * np.abs(v).mean(1, keepdims=True) + U32 * np.abs(d).max(1, keepdims=True)
    rho = D / s
    assert float(rho.max()) < 0.5, "the inputs leave the first-order bound's range"
    dz = (1 + np.abs(z)) * rho / (1 - rho) + np.abs(z) * (N / 2 + 8) * U32
    return y, np.abs(ga) * dz + 2 * U32 * (np.abs(ga * z) + np.abs(be)) + U16 * np.abs(y) + U32


def emulate(x, w, bias, epilogue, res=None, pos=None, S=None, gamma=None, beta=None, eps=EPS, pos_a=True, drop_last_k_block=False,
            no_bias=False, res_shift=False, pos_no_wrap=False, stat_cols=None, last_tile_first_weights=False):
    """The kernel's arithmetic in numpy -> float16.  Faults: drop_last_k_block leaves the last 64 of K out; no_bias; res_shift
    takes residual row r + 1 for row r; pos_no_wrap takes pos[r] for pos[r % S]; stat_cols = n takes mean and variance over
    the first n columns only; last_tile_first_weights computes the last tile of 128 columns with the first tile's rows of w
    (a column tile's offset left out of the W rows; PLAIN / RELU, N > 128)."""
    K = x.shape[1]
    ln = epilogue == ADD_LN
    xa = operand(x, pos if (not ln or pos_a) else None, S, pos_no_wrap).astype(np.float32)
    w32 = np.asarray(w, np.float16).astype(np.float32)
    if last_tile_first_weights:
        n0 = (len(w32) - 1) // 128 * 128
        w32 = np.concatenate([w32[:n0], w32[:len(w32) - n0]])
    acc = np.zeros((len(xa), len(w32)), np.float32)
    for k in range(0, K - 64 if drop_last_k_block else K, 32):          # one MFMA step: 32 products added to the accumulator
        acc = acc + (xa[:, k:k + 32] @ w32[:, k:k + 32].T).astype(np.float32)
    if bias is not None and not no_bias:
        acc = acc + np.asarray(bias, np.float32)
    if not ln:
        return (np.maximum(acc, 0) if epilogue == RELU else acc).astype(np.float16)
    r = np.asarray(res, np.float16).astype(np.float32)
    if res_shift:
        r = np.roll(r, -1, axis=0)
    v = _res(r, pos, S, pos_no_wrap).astype(np.float32) + acc
    n = stat_cols or v.shape[1]
    mean = (v[:, :n].sum(1, keepdims=True, dtype=np.float32) / np.float32(n)).astype(np.float32)
    d = v - mean
    var = ((d[:, :n] * d[:, :n]).sum(1, keepdims=True, dtype=np.float32) / np.float32(n)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = d * rstd * np.asarray(gamma, np.float32)
    if beta is not None:
        y = y + np.asarray(beta, np.float32)
    return y.astype(np.float16)


def loud_row(d, row, gain=100.0):
    """Row `row` of x and res times `gain`: its sums stand far above the other rows'."""
    d = dict(d)
    d["x"], d["res"] = d["x"].copy(), d["res"].copy()
    d["x"][row] = (d["x"][row].astype(np.float32) * gain / 16).astype(np.float16)       # |x| stays far below 65504
    d["res"][row] = (d["res"][row].astype(np.float32) * gain).astype(np.float16)
    return d


def flat_row(d, row, level=1.0):
    """Row `row` of res + bias is the constant `level` up to float16 rounding and x's row is scaled so that the product's
    variance is about eps: the row's variance + eps stays within a few eps."""
    d = dict(d)
    d["x"], d["res"] = d["x"].copy(), d["res"].copy()
    d["res"][row] = (level - d["bias"]).astype(np.float16)
    d["x"][row] = (d["x"][row].astype(np.float32) * 2e-3).astype(np.float16)
    return d


# ---------------------------------------------------------------- token_pool

def pool_inputs(B, S, n_out=None, seed=0, loud_next=False):
    """x (B * S + 1) x 512 float16 (one row more than the groups take) and, with n_out, w n_out x 512 and bias float32.
    loud_next: the first row of every group but the first is 8 in every channel, with the sign of w[0] where w is given, so a
    leak into the next group moves every mean and the first output by far more than the bound."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B * S + 1, LN_N)).astype(np.float32)
    d = {"w": None, "bias": None}
    if n_out:
        d["w"] = (rng.standard_normal((n_out, LN_N)) * 1.5 / np.sqrt(LN_N)).astype(np.float32)
        d["bias"] = (0.3 * rng.standard_normal(n_out)).astype(np.float32)
    if loud_next:
        x[S::S] = 8.0 * (np.sign(d["w"][0]) if n_out else 1.0)
    d["x"] = x.astype(np.float16)
    return d


def pool_reference(x, B, S, w=None, bias=None):
    """(out_ref, bound), float64.  A column's float32 mean is off by at most a = (ceil(S / 4) + 3) 2^-24 mean|x| (a thread adds
    every fourth row, three more operations join the partial sums and divide); without w
        |out - m| <= a + 2^-11 |m| + 2^-24,
    with w  |out - out_ref| <= sum_c |w_c| a_c + (E + 3) 2^-24 (sum_c |m_c| |w_c| + |b|) + 2^-11 |out_ref| + 2^-24."""
    g = np.asarray(x, np.float16).astype(np.float64)[:B * S].reshape(B, S, -1)
    m = g.mean(1)
    a = ((S + 3) // 4 + 3) * U32 * np.abs(g).mean(1)
    if w is None:
        return m, a + U16 * np.abs(m) + U32
    w64 = np.asarray(w, np.float64)
    b = np.zeros(len(w64)) if bias is None else np.asarray(bias, np.float64)
    out = m @ w64.T + b
    return out, a @ np.abs(w64).T + (g.shape[2] + 3) * U32 * (np.abs(m) @ np.abs(w64).T + np.abs(b)) + U16 * np.abs(out) + U32


def pool_emulate(x, B, S, w=None, bias=None, leak=False):
    """The kernel's arithmetic -> float16; leak: every group's mean runs over S + 1 rows (into the next group)."""
    x32 = np.asarray(x, np.float16).astype(np.float32)
    n = S + 1 if leak else S
    out = []
    for b in range(B):
        g = x32[b * S:b * S + n]
        part = []
        for ph in range(4):
            s = np.zeros(g.shape[1], np.float32)
            for row in g[ph::4]:
                s = s + row
            part.append(s)
        out.append(((part[0] + part[1]) + (part[2] + part[3])) / np.float32(n))
    m = np.stack(out).astype(np.float32)
    if w is None:
        return m.astype(np.float16)
    prod = m[:, None, :] * np.asarray(w, np.float32)[None]
    dots = (prod[..., 0::2] + prod[..., 1::2]).sum(-1, dtype=np.float32)
    if bias is not None:
        dots = dots + np.asarray(bias, np.float32)
    return dots.astype(np.float16)


def used_share(y, y_ref, bound):
    return float((np.abs(np.asarray(y, np.float64) - y_ref) / bound).max())
