"""Shared by the attention tests: inputs, the float64 reference with DESIGN.md s4.13's error bound, and a numpy emulation of
the kernel's arithmetic (float32 scores and accumulation, float16 P, float16 result) with switches for the designed faults.

All arrays are B x S x E with head h in channels h * D .. (h + 1) * D, D = 128."""
import numpy as np

D = 128
SCALE = 1.0 / np.sqrt(D)
BK = 64  # keys per tile of the kernel: where the running maximum is updated


def gaussian_qkv(B, S, H, seed=0, q_gain=3.0):
    """float16 q, k, v ~ N(0, 1), q times q_gain: the scores SCALE * q.k then have a standard deviation of about q_gain,
    so the softmax is peaked and a wrong or missing key moves the result."""
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((B, S, H * D)).astype(np.float32) for _ in range(3))
    return (q * q_gain).astype(np.float16), k.astype(np.float16), v.astype(np.float16)


def _heads(x, H):
    B, S, _ = x.shape
    return x.reshape(B, S, H, D).transpose(0, 2, 1, 3)          # B x H x S x D


def _merge(x):
    B, H, S, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, S, H * D)


def reference(q, k, v, H, scale=SCALE):
    """(o_ref, bound), both B x S x E float64: the float64 attention of the float16-rounded inputs and
    |o - o_ref| <= (2^-11 + 4 E_i + (S + 4) 2^-24) A + S 2^-25 max_j |v_jd| + 2^-11 |o_ref| + 2^-24 with
    A = sum_j p_ij |v_jd| and E_i = (D + 4) 2^-24 max_j(scale sum_d |q_id| |k_jd|) + 2^-21."""
    q, k, v = (_heads(np.asarray(x, np.float16).astype(np.float64), H) for x in (q, k, v))
    S = q.shape[2]
    x = scale * (q @ k.transpose(0, 1, 3, 2))
    p = np.exp(x - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = p @ v
    A = p @ np.abs(v)
    E = (D + 4) * 2.0 ** -24 * (abs(scale) * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2))).max(-1, keepdims=True) + 2.0 ** -21
    bound = ((2.0 ** -11 + 4 * E + (S + 4) * 2.0 ** -24) * A + S * 2.0 ** -25 * np.abs(v).max(2, keepdims=True)
             + 2.0 ** -11 * np.abs(o) + 2.0 ** -24)
    return _merge(o), _merge(bound)


def emulate(q, k, v, H, scale=SCALE, drop_last_key=False, leak_keys=0, skip_rescale_at=None):
    """The kernel's arithmetic in numpy -> B x S x E float16.  Faults: drop_last_key leaves key S - 1 out (a tail mask off
    by one); leak_keys = n lets batch b also see the first n keys of batch b + 1 (a tile that runs past the batch's last row);
    skip_rescale_at = t leaves the accumulator and the sum unscaled when the maximum moves at tile t (a broken rescale)."""
    qh, kh, vh = (_heads(np.asarray(x, np.float16).astype(np.float32), H) for x in (q, k, v))
    B, _, S, _ = qh.shape
    c = np.float32(np.float32(scale) * np.float32(1.4426950408889634))
    out = np.empty((B, H, S, D), np.float16)
    for b in range(B):
        kk, vv = kh[b], vh[b]
        if drop_last_key:
            kk, vv = kk[:, :S - 1], vv[:, :S - 1]
        if leak_keys and b + 1 < B:
            kk = np.concatenate([kk, kh[b + 1][:, :leak_keys]], 1)
            vv = np.concatenate([vv, vh[b + 1][:, :leak_keys]], 1)
        n = kk.shape[1]
        m = np.full((H, S, 1), -np.inf, np.float32)
        l = np.zeros((H, S, 1), np.float32)
        acc = np.zeros((H, S, D), np.float32)
        for t, j0 in enumerate(range(0, n, BK)):
            x = (qh[b] @ kk[:, j0:j0 + BK].transpose(0, 2, 1)).astype(np.float32) * c
            mn = np.maximum(m, x.max(-1, keepdims=True))
            with np.errstate(invalid="ignore"):
                alpha = np.exp2(m - mn).astype(np.float32)
            if skip_rescale_at == t:
                alpha = np.ones_like(alpha)
            p = np.exp2(x - mn).astype(np.float32)
            l = l * alpha + p.sum(-1, keepdims=True, dtype=np.float32)
            acc = acc * alpha + p.astype(np.float16).astype(np.float32) @ vv[:, j0:j0 + BK]
            m = mn
        out[b] = (acc / l).astype(np.float16)
    return _merge(out)


def dominate_last_key(q, k, H):
    """Every row's score against key S - 1 stands about 25 above the rest: channel 0 of every head is 8 in q and 40 in the
    last key (SCALE * 320 = 28)."""
    q, k = q.copy(), k.copy()
    q[:, :, 0::D] = 8.0
    k[:, -1, :] = 0.0
    k[:, -1, 0::D] = 40.0
    return q, k


def spike(q, k, H, row, key, gain=0.5):
    """Key `key` of every (batch, head) becomes gain * q[row]: row `row`'s score against it is SCALE * gain * |q|^2, about 50
    for gaussian q with gain 3, so the row's running maximum jumps by far more than 20 at that key's tile."""
    k = k.copy()
    k[:, key, :] = (q[:, row, :].astype(np.float32) * gain).astype(np.float16)
    return k


def used_share(o, o_ref, bound):
    return float((np.abs(np.asarray(o, np.float64) - o_ref) / bound).max())
