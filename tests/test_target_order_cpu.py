"""The rule of the target pack's compact row order, as tools/target_tiles_model.py restates it (plain numpy, no GPU):
where segments end, that the rule is deterministic, and what it does with ties."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("target_tiles_model", os.path.join(ROOT, "tools", "target_tiles_model.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


def _rows(name):
    from pedp_hip import synth

    rng = np.random.default_rng(5)
    if name in ("tiny", "parity"):
        p = synth.Frame(name).model_points
        p = p[tool.hilbert_order(p)]
        return (p - p.mean(0)).astype(np.float32)
    if name.startswith("n"):
        return rng.normal(0.0, 1.0, (int(name[1:]), 3)).astype(np.float32)
    if name == "identical":
        return np.tile(np.float32([0.25, -0.5, 1.0]), (1500, 1))
    if name == "collinear":
        t = np.zeros((1500, 3), np.float32)
        t[:, 1] = rng.normal(0.0, 1.0, 1500)
        return t
    assert name == "duplicated"
    return np.repeat(rng.normal(0.0, 1.0, (700, 3)).astype(np.float32), 3, axis=0)   # (equal rows side by side, as the Hilbert order leaves them)


def _recursive(xyz, pos):
    """The rule once more, written as a recursion over lists of positions."""
    m = len(pos)
    if m <= 16:
        return list(pos)
    p = xyz[pos]
    ext = [np.float32(p[:, a].max()) - np.float32(p[:, a].min()) for a in range(3)]
    axis = max(range(3), key=lambda a: (ext[a], -a))
    ranked = sorted(range(m), key=lambda k: (p[k, axis], k))
    u = 1024 if m > 1024 else 64 if m > 64 else 16
    h = u * ((m + 2 * u - 1) // (2 * u))
    return _recursive(xyz, [pos[k] for k in ranked[:h]]) + _recursive(xyz, [pos[k] for k in ranked[h:]])


SHAPES = ["tiny", "parity", "n1", "n15", "n16", "n17", "n63", "n65", "n1023", "n1024", "n1025", "n2049", "identical", "collinear",
          "duplicated"]


@pytest.mark.parametrize("name", SHAPES)
def test_rule(name):
    xyz = _rows(name)
    n = len(xyz)
    log = []
    order = tool.compact_order(xyz, log)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(order, tool.compact_order(xyz.copy()))                 # deterministic
    assert np.array_equal(order, _recursive(xyz, list(range(n))))
    # every split ends its left part on a multiple of 1024 / 64 / 16, so every word, unit and tile is a subtree
    assert (len(log) > 0) == (n > 16)
    cuts = {0, n}
    for s, m, axis, h in log:
        u = 1024 if m > 1024 else 64 if m > 64 else 16
        assert s % u == 0 and h % u == 0 and 0 < h < m and h >= m - h
        cuts.add(s + h)
    for u in (16, 64, 1024):
        assert all(k in cuts for k in range(0, n, u)), u
    got = sorted(cuts)
    assert all(b - a <= 16 for a, b in zip(got, got[1:]))
    # a split separates: nothing on the left lies beyond anything on the right on the split's axis
    state = np.arange(n)
    for s, m, axis, h in log:
        seg = state[s:s + m]
        state[s:s + m] = seg[np.argsort(xyz[seg, axis], kind="stable")]
        assert xyz[state[s:s + h], axis].max() <= xyz[state[s + h:s + m], axis].min()
    assert np.array_equal(state, order)


def test_ties_keep_the_order_so_far():
    xyz = _rows("identical")
    assert np.array_equal(tool.compact_order(xyz), np.arange(len(xyz)))          # zero extent on every axis: nothing moves
    xyz = _rows("duplicated")
    order = tool.compact_order(xyz)
    where = np.empty(len(xyz), np.int64)
    where[order] = np.arange(len(xyz))
    w = where.reshape(-1, 3)                                                      # the three copies of a row
    assert (np.diff(w, axis=1) > 0).all()
    assert (w[:, 2] // 16 != w[:, 0] // 16).any()                                # ... some of them in different tiles
    z = np.zeros((40, 3), np.float32)
    z[::2, 0] = -0.0                                                              # -0 counts as +0
    assert np.array_equal(tool.compact_order(z), np.arange(40))


def test_left_rows():
    assert [tool.left_rows(m) for m in (17, 32, 33, 64, 65, 128, 1000, 1024, 1025, 2048, 2049, 100000)] == \
        [16, 16, 32, 32, 64, 64, 512, 512, 1024, 1024, 2048, 50176]
