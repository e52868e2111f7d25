"""tests/golden/g10_reference.npz for the two test files that read it: the loaded fixture, the comparisons they share
(equal in every bit; the float32 three-term dot product bound; float64 steps), and the few
arrays that are rebuilt from stored ones (poses around the stored translations, the 3 x 3 windows from their four varying
entries, the 6d rows of the stored rotation deltas)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_reference.npz")
U23 = 2.0 ** -23
_cache = {}


def fixture():
    """Every array of the fixture, loaded once (no pickles: numbers and names only)."""
    if not _cache:
        with np.load(PATH, allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
        for v in _cache.values():
            v.setflags(write=False)
    return _cache


def _differ(a, b):
    """Where two arrays of one shape and dtype differ in bits (a NaN equals any NaN)."""
    if a.dtype.kind != "f":
        return a != b
    ua, ub = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
    return ~((ua == ub) | (np.isnan(a) & np.isnan(b)))


def same_bits(a, b):
    """Same shape, same dtype, equal bit for bit, except that any NaN equals any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and not _differ(a, b).any()


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    bad = np.argwhere(_differ(got, want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at {i}: {got[i]!r} for {want[i]!r}")


def ulps64(a, b):
    """Distance in float64 steps between finite values of one sign."""
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


STATS = ("n_pos", "n_valid", "n_med", "umin", "umax", "vmin", "vmax")
GT_CASES = ["37x53_c_bool_odd", "37x53_q_uint8_even", "37x53_c_float32_even", "37x53_q_float32_odd", "64x96_q_bool_odd",
            "64x96_q_uint8_even", "64x96_q_float32_even", "64x96_q_float32_odd", "1x1_bool", "1x1_uint8", "1x1_negative",
            "zero_mask", "no_valid"]
DIAM_CASES = ["1", "2", "255", "256", "257", "513", "equal", "far"]


def stats_record(fx, name):
    """The seven counts / box fields of a guess_translation case; n_med is left out where the reference returned before
    it looked at the depths (an empty `mask > 0`: stored as -1)."""
    rec = {k: int(fx[f"gt/{name}/{k}"]) for k in STATS}
    if rec["n_med"] < 0:
        del rec["n_med"]
    return rec


def crop_poses(trans, seed=7):
    """B x 4 x 4 float32 poses with the stored translations; the rotation block, which the window does not read, is filled
    with seeded noise so that a reader of the wrong entries shows."""
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4, dtype=np.float32), (len(trans), 1, 1))
    P[:, :3, :3] = rng.uniform(-1, 1, (len(trans), 3, 3))
    P[:, :3, 3] = trans
    return P


def crop_tf(fx, di, oi):
    """The reference's B x 3 x 3 windows of diameter di and out_size oi: the four stored entries among +0 and 1."""
    sx = fx[f"crop/d{di}_o{oi}/sx"]
    tf = np.zeros((len(sx), 3, 3), np.float32)
    tf[:, 2, 2] = 1
    tf[:, 0, 0], tf[:, 0, 2] = sx, fx[f"crop/d{di}_o{oi}/tx"]
    tf[:, 1, 1], tf[:, 1, 2] = fx[f"crop/d{di}_o{oi}/sy"], fx[f"crop/d{di}_o{oi}/ty"]
    return tf


CROP_CASES = [(0, 0), (1, 0), (1, 1), (2, 0)]        # (diameter, out_size) pairs the fixture holds


def half_edges(fx):
    """The window edges (left, right, top, bottom) of `crop/half`'s poses before rounding, all of them exact in float32."""
    t = fx["crop/half/trans"].astype(np.float64)
    cu, cv = 600.0 * t[:, 0] / t[:, 2] + 319.5, 600.0 * t[:, 1] / t[:, 2] + 239.5
    rad = 600.0 * (float(fx["crop/half/diameter"]) * float(fx["crop/half/crop_ratio"]) / 2) / t[:, 2]
    return np.stack([cu - rad, cu + rad, cv - rad, cv + rad], 1)


def rot6d_of(Rd):
    """Raw '6d' network outputs whose Gram-Schmidt result is Rd's transpose up to float32 rounding: its first two rows."""
    R = np.asarray(Rd, np.float32).transpose(0, 2, 1)
    return np.ascontiguousarray(R[:, :2, :].reshape(len(R), 6))


def compose_bound(Rd, A):
    """3 * 2^-23 * sum_k |Rd_ik| |A_kj| per entry of Rd @ A[:3, :3]: a float32 three-term dot product, in any order and with
    or without FMA, is within 3 * 2^-24 of that sum of the exact value, so two of them are within twice that of each other."""
    Rd, A = np.abs(np.asarray(Rd, np.float64)), np.abs(np.asarray(A, np.float64)[:, :3, :3])
    return 3 * U23 * (Rd @ A)


def big_triangle():
    """One triangle across every pixel ray of the fixture's cameras at z = 100: every selected pixel hits it."""
    return (np.array([[-1e4, -1e4, 100.0], [3e4, -1e4, 100.0], [-1e4, 3e4, 100.0]], np.float32),
            np.array([[0, 1, 2]], np.uint32))
