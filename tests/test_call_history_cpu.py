"""The call-history harness (tests/_history_ops.py) on fake pure-Python operations: it must flag exactly the operation
that depends on what ran before it, say where, and compare bytes -- not values."""
import numpy as np
import pytest

import _history_ops as H


class FakeEnv:
    """What a fake operation may carry from call to call."""

    def __init__(self):
        self.calls = 0


def _ops():
    def pure(k):
        return H.Op(f"pure{k}@small", lambda env: {"x": np.arange(4, dtype=np.float64) * k, "n": np.asarray(k, np.int32)},
                    lambda out: None, "a")

    def counter(env):
        env.calls += 1
        return {"x": np.asarray(env.calls, np.int64)}

    return [pure(k) for k in range(1, 12)] + [H.Op("counter@small", counter, lambda out: None, "a")]


def _fresh(ops):
    return {op.name: H.call(op, FakeEnv()) for op in ops}


def test_only_the_history_dependent_operation_is_flagged_with_its_position_and_predecessors():
    ops = _ops()
    fresh = _fresh(ops)
    assert fresh["counter@small"]["x"] == 1
    pure = [op for op in ops if op.base != "counter"]
    assert H.replay(H.histories(pure, 5), FakeEnv(), fresh, seed=5) == 2 * len(pure)        # pure operations: any history passes
    for seed in (0, 1, 2):
        history = H.histories(ops, seed)
        first, second = [i for i, op in enumerate(history) if op.base == "counter"]
        assert first < len(ops) <= second
        with pytest.raises(H.HistoryError) as err:
            H.replay(history, FakeEnv(), fresh, seed=seed)
        e = err.value
        # the first call of the counter gives the fresh 1; the second one, in the second pass, gives 2
        assert (e.op, e.position, e.seed) == ("counter@small", second, seed)
        assert e.before == [op.name for op in history[second - 8:second]] and len(e.before) == 8
        text = str(e)
        assert f"position {second}" in text and f"seed {seed}" in text and "counter@small" in text
        assert "BEFORE = [" + ", ".join(repr(n) for n in e.before) + "]" in text             # pasteable
        assert "x:" in e.detail and "2" in e.detail and "1" in e.detail


def test_a_short_history_reports_the_calls_it_has():
    ops = _ops()
    fresh = _fresh(ops)
    counter = ops[-1]
    with pytest.raises(H.HistoryError) as err:
        H.replay([ops[0], counter, ops[1], counter], FakeEnv(), fresh, seed=None)
    assert err.value.position == 3 and err.value.before == ["pure1@small", "counter@small", "pure2@small"]


def test_two_envs_in_turn_each_keep_their_own_history():
    ops = _ops()
    fresh = _fresh(ops)
    counter = ops[-1]
    assert H.replay([counter, counter], [FakeEnv(), FakeEnv()], fresh) == 2                 # one call each: both fresh
    with pytest.raises(H.HistoryError) as err:
        H.replay([counter, counter, ops[0], counter], [FakeEnv(), FakeEnv()], fresh)
    assert err.value.position == 3                                                          # the second call on the second env


def test_an_exception_in_a_call_is_reported_like_a_difference():
    def boom(env):
        raise RuntimeError("no such kernel")

    ops = _ops()
    with pytest.raises(H.HistoryError, match="raised RuntimeError: no such kernel") as err:
        H.replay([ops[0], H.Op("boom@small", boom)], FakeEnv(), _fresh(ops))
    assert err.value.position == 1 and err.value.before == ["pure1@small"]


def test_check_only_entries_go_through_their_check():
    def check(out):
        assert out["x"] >= 1, "x below 1"

    counter = H.Op("counter@small", _ops()[-1].run, check)
    fresh = {"counter@small": {"x": np.asarray(1, np.int64)}}
    assert H.replay([counter, counter], FakeEnv(), fresh, check_only={"counter@small"}) == 2
    bad = H.Op("counter@small", lambda env: {"x": np.asarray(0, np.int64)}, check)
    with pytest.raises(H.HistoryError, match="its check failed: x below 1"):
        H.replay([bad], FakeEnv(), fresh, check_only={"counter@small"})


def test_same_bytes_tells_zeros_nans_dtypes_and_shapes_apart():
    z = {"v": np.array([1.0, 0.0])}
    assert H.same_bytes(z, {"v": np.array([1.0, 0.0])}) is None
    assert np.array_equal(z["v"], np.array([1.0, -0.0]))                                    # equal as values ...
    diff = H.same_bytes(z, {"v": np.array([1.0, -0.0])})                                    # ... not as bytes
    assert diff is not None and diff.startswith("v:") and "index 1" in diff
    quiet = np.array([0x7FF8000000000000, 0x7FF8000000000001], np.uint64).view(np.float64)
    assert np.isnan(quiet).all()
    assert H.same_bytes({"v": quiet[:1]}, {"v": quiet[:1].copy()}) is None                  # the same NaN
    assert H.same_bytes({"v": quiet[:1]}, {"v": quiet[1:]}).startswith("v:")                # another payload
    assert "dtype" in H.same_bytes({"v": np.zeros(2, np.float32)}, {"v": np.zeros(1, np.float64)})
    assert "dtype" in H.same_bytes({"v": np.zeros(2, np.int32)}, {"v": np.zeros(2, np.uint32)})
    assert "shape" in H.same_bytes({"v": np.zeros((2, 3))}, {"v": np.zeros((3, 2))})
    assert "shape" in H.same_bytes({"v": np.zeros(0)}, {"v": np.zeros((0, 3))})
    assert H.same_bytes({"v": np.zeros((0, 3))}, {"v": np.zeros((0, 3))}) is None
    # the first differing key is named, and a key on one side only
    a = {"p": np.ones(3), "q": np.arange(3), "r": np.zeros(2)}
    b = {"p": np.ones(3), "q": np.array([0, 1, 3]), "r": np.ones(2)}
    assert H.same_bytes(a, b).startswith("q:")
    assert "keys" in H.same_bytes(a, {"p": np.ones(3)})
    assert H.same_bytes({"v": np.arange(6).reshape(2, 3)[:, ::2]}, {"v": np.array([[0, 2], [3, 5]])}) is None   # strided views


def test_the_same_seed_gives_the_same_history():
    ops = _ops()
    a, b = H.histories(ops, 7), H.histories(ops, 7)
    assert [o.name for o in a] == [o.name for o in b] and len(a) == 2 * len(ops)
    assert sorted(o.name for o in a[:len(ops)]) == sorted(o.name for o in ops) == sorted(o.name for o in a[len(ops):])
    assert [o.name for o in a] != [o.name for o in H.histories(ops, 8)]
    assert [o.name for o in a[:len(ops)]] != [o.name for o in a[len(ops):]]                # two shuffles, not one twice
    assert len(H.histories(ops, 7, passes=3)) == 3 * len(ops)


def test_ops_name_their_operation_and_groups_and_pair_by_size():
    small, large = H.Op("voxel@5", None, None, "pinned"), H.Op("voxel@2", None, None, ("pinned", "cloud_ws"))
    lone = H.Op("lone@1", None)
    assert small.base == large.base == "voxel" and small.group == {"pinned"} and large.group == {"pinned", "cloud_ws"}
    assert lone.group == frozenset()
    assert H.pairs_by_size([small, lone, large]) == {"voxel": (small, large)}


def test_a_deferred_result_is_fetched_behind_the_next_call_and_reported_at_its_own_position():
    """A fake device-memory call leaves its result in a buffer of the env and hands back a Later; a fake host call that
    scribbles over that buffer at once is caught only because nothing fetched the result in between."""
    def device(env):
        env.buffer = np.arange(3.0)
        return H.Later(lambda: {"x": env.buffer.copy()})

    def scribble(env):
        env.buffer = np.zeros(3)
        return {"y": np.ones(1)}

    dev, bad, good = H.Op("device@small", device), H.Op("scribble@small", scribble), _ops()[0]
    fresh = {op.name: H.outputs(H.call(op, FakeEnv())) for op in (dev, bad, good)}
    assert fresh["device@small"]["x"].tolist() == [0.0, 1.0, 2.0]
    assert H.replay([good, dev, good, dev], FakeEnv(), fresh) == 4                          # the last one is fetched at the end
    with pytest.raises(H.HistoryError) as err:
        H.replay([good, dev, bad, good], FakeEnv(), fresh, seed=3)
    assert (err.value.op, err.value.position, err.value.before) == ("device@small", 1, ["pure1@small"])
    with pytest.raises(H.HistoryError) as err:                                              # two deferred calls in a row
        H.replay([dev, dev, bad], FakeEnv(), fresh)
    assert err.value.position == 1

    def broken(env):
        def fetch():
            raise RuntimeError("copy failed")
        return H.Later(fetch)

    with pytest.raises(H.HistoryError, match="fetching its outputs raised RuntimeError: copy failed") as err:
        H.replay([good, H.Op("broken@small", broken), good], FakeEnv(), fresh)
    assert err.value.position == 1
