"""Call histories: every public operation as a function of its arguments alone.

The harness (Op, same_bytes, histories, replay, HistoryError) is plain Python and imports without a GPU; the tests of
tests/test_call_history_cpu.py run it on fake operations.  The catalogue (catalogue(), built on first use) has one entry
per public operation at two sizes, each with the reference its module's own test file compares against; an Env gives an
entry a library context and the torch side stream that context runs on, so that the explicit-ctx calls and the
stream-dispatched wrappers of one history share one context.  tests/test_call_history_gpu.py runs the histories."""
import contextlib
import functools
import random

import numpy as np


# ================================================================ the harness

class Op:
    """One call of the catalogue.  run(env) -> dict[str, np.ndarray]: copies of the call's outputs (no diagnostics: no
    sweep times, no *_last_* counters, no variants).  check(out): asserts the outputs against the module's reference.
    group: the shared state the call touches (names of test (d)'s neighbourhoods).  `name` is "<operation>@<size>"."""

    def __init__(self, name, run, check=None, group=()):
        self.name, self.run, self.check = name, run, check
        self.group = frozenset((group,) if isinstance(group, str) else group)
        self.base = name.split("@")[0]

    def __repr__(self):
        return f"Op({self.name!r})"


def _bytes_of(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)


def same_bytes(a, b):
    """None if the two dicts hold the same keys and, key by key, arrays of one dtype, one shape and the same bytes
    (-0.0 is not 0.0, a NaN equals only the NaN of its payload); else a line that names the first differing key."""
    if sorted(a) != sorted(b):
        return f"keys {sorted(a)} against {sorted(b)}"
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype:
            return f"{k}: dtype {x.dtype} against {y.dtype}"
        if x.shape != y.shape:
            return f"{k}: shape {x.shape} against {y.shape}"
        bx, by = _bytes_of(x), _bytes_of(y)
        if not np.array_equal(bx, by):
            bad = np.flatnonzero(bx != by)
            i = int(bad[0]) // max(x.dtype.itemsize, 1)
            return (f"{k}: {len(np.unique(bad // max(x.dtype.itemsize, 1)))} of {x.size} values differ, first at flat index {i}: "
                    f"{x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r}")
    return None


def histories(ops, seed, passes=2):
    """`passes` shuffles of `ops`, one behind the other, drawn from `seed` alone (the same seed: the same list)."""
    rng = random.Random(seed)
    out = []
    for _ in range(passes):
        order = list(ops)
        rng.shuffle(order)
        out += order
    return out


class HistoryError(AssertionError):
    """A call of a history differed from the fresh result (or raised).  op, position, seed, before (the names of up to
    eight calls in front of it, oldest first) and detail are attributes; the message holds them as a pasteable list."""

    def __init__(self, op, position, seed, before, detail):
        self.op, self.position, self.seed, self.before, self.detail = op, position, seed, list(before), detail
        super().__init__(report(op, position, seed, before, detail))


def report(op, position, seed, before, detail):
    names = ", ".join(repr(n) for n in before)
    return (f"{op} at position {position} of the history (seed {seed}) differs from a fresh context: {detail}\n"
            f"the calls before it, oldest first -- replay([by_name[n] for n in BEFORE + [{op!r}]], ...):\n"
            f"BEFORE = [{names}]")


class Later:
    """What a device-memory call returns instead of its outputs: the call is enqueued, fetch() downloads them.  replay
    fetches only after the NEXT call of the history has been made, so that call starts with this one still in flight --
    nothing waits between the two but what the calls wait for themselves."""

    def __init__(self, fetch):
        self.fetch, self.env = fetch, None


def outputs(result):
    """The outputs of call()'s result: a Later is fetched, on its env's stream."""
    if not isinstance(result, Later):
        return result
    on = getattr(result.env, "on_stream", None)
    with (on() if on else contextlib.nullcontext()):
        return result.fetch()


DEVICE_FAULT_WORDS = ("illegal memory access", "hipErrorIllegalAddress", "unspecified launch failure", "hipErrorLaunchFailure")


def call(op, env):
    """op.run(env) on the env's stream (an env without a stream, as the fake ones of the CPU test: called as it is)."""
    on = getattr(env, "on_stream", None)
    try:
        with (on() if on else contextlib.nullcontext()):
            result = op.run(env)
        if isinstance(result, Later):
            result.env = env
        return result
    except Exception as e:
        if any(w in str(e) for w in DEVICE_FAULT_WORDS):       # the device itself faulted: nothing more is started on it
            import pytest

            pytest.exit(f"{op.name}: the GPU reported a fault ({e}); the session ends here", returncode=3)
        raise


def replay(history, envs, yardstick, seed=None, check_only=()):
    """Runs history[i] on envs[i % len(envs)] and compares each result with yardstick[name], byte for byte, before the
    next call -- a device-memory call's (a Later) behind the next call, so nothing is waited for in between.  check_only: names compared through their `check` instead.  Raises HistoryError
    for the first call that differs; returns the number of calls made."""
    envs = list(envs) if isinstance(envs, (list, tuple)) else [envs]

    def compare(pos, result):
        op = history[pos]
        before = [o.name for o in history[max(0, pos - 8):pos]]
        try:
            got = outputs(result)
        except Exception as e:
            raise HistoryError(op.name, pos, seed, before, f"fetching its outputs raised {type(e).__name__}: {e}") from e
        if op.name in check_only:
            try:
                op.check(got)
            except AssertionError as e:
                raise HistoryError(op.name, pos, seed, before, f"its check failed: {e}") from e
            return
        diff = same_bytes(got, yardstick[op.name])
        if diff is not None:
            raise HistoryError(op.name, pos, seed, before, diff)

    in_flight = None                      # (position, Later) of a device-memory call whose outputs are not fetched yet
    for pos, op in enumerate(history):
        try:
            result = call(op, envs[pos % len(envs)])
        except Exception as e:
            before = [o.name for o in history[max(0, pos - 8):pos]]
            raise HistoryError(op.name, pos, seed, before, f"the call raised {type(e).__name__}: {e}") from e
        if in_flight is not None:
            compare(*in_flight)
        in_flight = (pos, result) if isinstance(result, Later) else None
        if in_flight is None:
            compare(pos, result)
    if in_flight is not None:
        compare(*in_flight)
    return len(history)


# ================================================================ a context and its stream

_live_envs = {}


class Env:
    """A fresh library context on a fresh torch side stream, registered as THE context of that stream
    (_bridge.stream_context(device, stream.cuda_stream) is env.ctx), so the wrappers that take no ctx run on it under
    `with env.on_stream()`.  torch hands side streams out of a pool of 32 and reuses their handles: an entry of
    _bridge._stream_ctx left for the handle by an earlier owner is closed and dropped.  `kept` holds what an operation
    keeps between its calls on this env (meshes, ray sets, defect maps, buffers); close() closes them and the context."""

    def __init__(self, device=0):
        import torch
        from pedp_hip import _bridge, _lib

        self.torch, self.device = torch, device
        self.dev = torch.device(f"cuda:{device}")
        held = []
        for _ in range(40):                       # a handle a live Env of ours owns: draw the pool's next one
            self.stream = torch.cuda.Stream(device)
            self.key = (device, self.stream.cuda_stream)
            if self.key not in _live_envs:
                break
            held.append(self.stream)
        else:
            raise RuntimeError("no free torch side stream")
        stale = _bridge._stream_ctx.pop(self.key, None)
        if stale is not None:
            stale.close()
        self.ctx = _lib.Context(device, stream=self.stream.cuda_stream)
        _bridge._stream_ctx[self.key] = self.ctx
        _live_envs[self.key] = self
        self.kept = {}

    def on_stream(self):
        return self.torch.cuda.stream(self.stream)

    def keep(self, key, make):
        if key not in self.kept:
            self.kept[key] = make()
        return self.kept[key]

    def cuda(self, a, dtype=None):
        """A host array on the device (call under on_stream(): the copy is ordered there)."""
        return self.torch.as_tensor(np.array(a, order="C"), device=self.dev, dtype=dtype)      # (a copy: the inputs are read-only)

    def close(self):
        from pedp_hip import _bridge

        if self.ctx is None:
            return
        self.stream.synchronize()
        for v in self.kept.values():
            for h in (v if isinstance(v, (list, tuple)) else (v,)):
                if hasattr(h, "close"):
                    h.close()
        self.kept.clear()
        if _bridge._stream_ctx.get(self.key) is self.ctx:
            del _bridge._stream_ctx[self.key]
        _live_envs.pop(self.key, None)
        self.ctx.close()
        self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ================================================================ the catalogue's inputs (made once, never written to)

def _oracle():
    import pedp_oracle

    pedp_oracle.build()
    return pedp_oracle


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def frame(config):
    from pedp_hip import synth

    return synth.Frame(config)


@functools.lru_cache(maxsize=None)
def frame_hits(config):
    f = frame(config)
    return _oracle().raycast(f.verts_posed, f.tris, f.rays6, bvh=True)


@functools.lru_cache(maxsize=None)
def frame_scene(config):
    """The scene cloud of test_icp_gpu._frame_scene."""
    return _ro(frame(config).scene(frame_hits(config)["t_hit"]))


@functools.lru_cache(maxsize=None)
def scattered_rays(n):
    """n rays with origins of their own towards the tiny frame's mesh (test_ray_gpu's general-origin rays)."""
    f = frame("tiny")
    rng = np.random.default_rng(5 + n)
    o = rng.normal(0, 150, size=(n, 3))
    tgt = f.verts_posed[rng.integers(0, len(f.verts_posed), n)] + rng.normal(0, 5, size=(n, 3))
    d = (tgt - o) * rng.uniform(0.01, 3.0, size=(n, 1))
    return _ro(np.hstack([o, d]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def heatmap(config, seed, fill=0.3, nan=True):
    import test_project_gpu

    f = frame(config)
    hm = test_project_gpu._heatmap(f.height, f.width, seed, fill)
    return _ro(hm if nan else np.nan_to_num(hm, nan=0.0))


def _c2d():
    M = np.eye(4)
    M[:3, :3] = _oracle().rot_xyz([0.02, -0.01, 0.03])
    M[:3, 3] = (31.0, -2.5, 1.75)
    return M


def _copy(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def _host(t):
    return t.detach().cpu().numpy().copy()


def _later(**tensors):
    """The named device tensors of an enqueued call, downloaded when the harness fetches them (None: left out)."""
    return Later(lambda: {k: _host(v) for k, v in tensors.items() if v is not None})


def _mesh(env, config):
    f = frame(config)
    from pedp_hip import _lib

    return env.keep(("mesh", config), lambda: _lib.Mesh(env.ctx, f.verts_posed, f.tris))


# ---------------------------------------------------------------- rays

def _same_rays(res, ref, uv=True):
    assert np.array_equal(res["primitive_ids"], ref["primitive_ids"]), "primitive_ids"
    assert np.array_equal(res["t_hit"].view(np.uint32), ref["t_hit"].view(np.uint32)), "t_hit"
    if uv:
        assert np.array_equal(res["primitive_uvs"].view(np.uint32), ref["primitive_uvs"].view(np.uint32)), "primitive_uvs"


def _ray_ops():
    from pedp_hip import _lib

    ops = []
    for config in ("tiny", "parity"):
        ops.append(Op(f"rays_frame@{config}", lambda env, c=config: _copy(_mesh(env, c).cast_rays(frame(c).rays6)),
                      lambda out, c=config: _same_rays(out, frame_hits(c)), ("ray_in", "mesh")))

        def rayset(env, c=config):
            rs = env.keep(("rayset", c), lambda: _lib.RaySet(env.ctx, frame(c).rays6))
            return _copy(_mesh(env, c).cast_rayset(rs))
        ops.append(Op(f"rays_rayset@{config}", rayset, lambda out, c=config: _same_rays(out, frame_hits(c)), ("mesh",)))

        def device(env, c=config):
            torch, r = env.torch, frame(c).rays6
            d = env.cuda(r)
            t = torch.empty(len(r), dtype=torch.float32, device=env.dev)
            ids = torch.empty(len(r), dtype=torch.int32, device=env.dev)
            uv = torch.empty((len(r), 2), dtype=torch.float32, device=env.dev)
            _mesh(env, c).cast_rays_device(d.data_ptr(), len(r), t.data_ptr(), ids.data_ptr(), uv.data_ptr())
            return Later(lambda: {"t_hit": _host(t), "primitive_ids": _host(ids).view(np.uint32), "primitive_uvs": _host(uv)})
        ops.append(Op(f"rays_device@{config}", device, lambda out, c=config: _same_rays(out, frame_hits(c)), ("mesh",)))

        def posed(env, c=config):
            g = frame(c)
            pm = env.keep(("posable", c), lambda: _lib.Mesh(env.ctx, g.model_points, g.tris, posable=True))
            pm.set_pose(g.T_gt)
            out = _copy(pm.cast_rays(g.rays6))
            out["posed_vertices"] = np.array(pm.posed_vertices(g.T_start), copy=True)
            return out

        def posed_check(out, c=config):
            g, o = frame(c), _oracle()
            _same_rays(out, o.raycast(o.pose_vertices(g.T_gt, g.model_points), g.tris, g.rays6, bvh=True))
            assert np.array_equal(out["posed_vertices"], o.pose_vertices(g.T_start, g.model_points, dtype=np.float64))
        ops.append(Op(f"rays_posed@{config}", posed, posed_check, ("mesh",)))

        def moved_pose(c=config):
            T = frame(c).T_gt.copy()
            T[:3, 3] += (3.0, -2.0, 5.0)
            T[:3, :3] = T[:3, :3] @ _oracle().rot_xyz([0.05, -0.03, 0.04])
            return T

        def posed_moved(env, c=config, moved_pose=moved_pose):       # the SAME posable handle under another pose, no uv
            g = frame(c)
            pm = env.keep(("posable", c), lambda: _lib.Mesh(env.ctx, g.model_points, g.tris, posable=True))
            pm.set_pose(moved_pose())
            return _copy(pm.cast_rays(g.rays6, want_uv=False))

        def posed_moved_check(out, c=config, moved_pose=moved_pose):
            g, o = frame(c), _oracle()
            ref = o.raycast(o.pose_vertices(moved_pose(), g.model_points), g.tris, g.rays6, bvh=True)
            assert (ref["primitive_ids"] != frame_hits(c)["primitive_ids"]).any()
            _same_rays(out, ref, uv=False)
        ops.append(Op(f"rays_posed_moved@{config}", posed_moved, posed_moved_check, ("mesh",)))

        def shuffled(c=config):
            return np.random.default_rng(1).permutation(len(frame(c).rays6))

        def shuffled_check(out, c=config, shuffled=shuffled):
            ref = frame_hits(c)
            _same_rays(out, {k: ref[k][shuffled()] for k in ("primitive_ids", "t_hit", "primitive_uvs")})
        # as many rays as the frame in another order: the direction order kept from the frame's cast does not fit them
        ops.append(Op(f"rays_shuffled@{config}", lambda env, c=config, shuffled=shuffled: _copy(_mesh(env, c).cast_rays(frame(c).rays6[shuffled()])),
                      shuffled_check, ("ray_in", "mesh")))
    for n in (257, 1000):
        ops.append(Op(f"rays_scattered@{n}", lambda env, n=n: _copy(_mesh(env, "tiny").cast_rays(scattered_rays(n))),
                      lambda out, n=n: _same_rays(out, _oracle().raycast(frame("tiny").verts_posed, frame("tiny").tris, scattered_rays(n))),
                      ("ray_in",)))
    return ops


# ---------------------------------------------------------------- projection

def _projection(out):
    d = {k: np.array(v, copy=True) for k, v in out.items() if k != "n_rays"}
    d["n_rays"] = np.asarray(out["n_rays"], np.int64)
    return d


def _check_projection(out, ref):
    import test_project_gpu

    assert len(ref["points"]) > 5
    test_project_gpu._check(dict(out, n_rays=int(out["n_rays"])), ref)


def _project_ops():
    from pedp_hip.ray_projection import _jet_lut

    ops = []
    for config, thr in (("tiny", 0.5), ("parity", 0.75)):
        ops.append(Op(f"project@{config}",
                      lambda env, c=config, t=thr: _projection(_mesh(env, c).project_heatmap(heatmap(c, 3), frame(c).K, t)),
                      lambda out, c=config, t=thr: _check_projection(out, _oracle().project_heatmap(
                          frame(c).verts_posed, frame(c).tris, heatmap(c, 3), frame(c).K, t)),
                      ("ray_in", "mesh")))

        # every pixel selected: more hits than the room the mesh handle kept from its last projection (Mesh._hit_cap)
        ops.append(Op(f"project_dense@{config}",
                      lambda env, c=config: _projection(_mesh(env, c).project_heatmap(np.ones((frame(c).height, frame(c).width)), frame(c).K, 0.5)),
                      lambda out, c=config: _check_projection(out, _oracle().project_heatmap(
                          frame(c).verts_posed, frame(c).tris, np.ones((frame(c).height, frame(c).width)), frame(c).K, 0.5)),
                      ("ray_in", "mesh")))

        def jet(env, c=config):
            return _projection(_mesh(env, c).project_heatmap(heatmap(c, 8, 0.5), frame(c).K, 0.6, jet_lut=_jet_lut(), post=_c2d()))

        def jet_check(out, c=config):
            from pedp_hip import compat

            o, f, hm = _oracle(), frame(c), heatmap(c, 8, 0.5)
            ref = o.project_heatmap(f.verts_posed, f.tris, hm, f.K, 0.6)
            assert len(ref["points"]) > 5
            for k in ("pixels", "primitive_ids", "intensities"):
                assert np.array_equal(out[k], ref[k]), k
            assert np.abs(out["points"] - o.transform(_c2d(), ref["points"])).max() < 1e-9, "points"
            assert np.array_equal(out["colors"], np.asarray(compat.create_intersection_pcd(ref["points"], ref["intensities"]).colors))
        ops.append(Op(f"project_jet_post@{config}", jet, jet_check, ("pinned",)))

        def cuda32(env, c=config):
            hm32 = heatmap(c, 8, 0.5, nan=False).astype(np.float32)
            return _projection(_mesh(env, c).project_heatmap(env.cuda(hm32), frame(c).K, 0.6, jet_lut=_jet_lut(), post=_c2d()))

        def cuda32_check(out, c=config):
            from pedp_hip import compat

            o, f = _oracle(), frame(c)
            hm32 = heatmap(c, 8, 0.5, nan=False).astype(np.float32)
            ref = o.project_heatmap(f.verts_posed, f.tris, hm32.astype(np.float64), f.K, 0.6)
            assert len(ref["points"]) > 5
            for k in ("pixels", "primitive_ids", "intensities"):
                assert np.array_equal(out[k], ref[k]), k
            assert np.abs(out["points"] - o.transform(_c2d(), ref["points"])).max() < 1e-9, "points"
            assert np.array_equal(out["colors"], np.asarray(compat.create_intersection_pcd(ref["points"], ref["intensities"]).colors))
        ops.append(Op(f"project_cuda_f32@{config}", cuda32, cuda32_check))
    return ops


# ---------------------------------------------------------------- closest points

@functools.lru_cache(maxsize=None)
def closest_queries(config, n):
    import test_closest_gpu

    f = frame(config)
    return _ro(test_closest_gpu.queries(f.verts_posed, f.tris, n, n))


def face_ids(config, n):
    """n triangle ids in a scattered order; every 97th names no face (F, F + 1, ... and the miss value)."""
    F = len(frame(config).tris)
    ids = (np.arange(n, dtype=np.uint64) * 7919 % F).astype(np.uint32)
    ids[::97] = np.where(np.arange(len(ids[::97])) % 2 == 0, F + np.arange(len(ids[::97])), 0xFFFFFFFF).astype(np.uint32)
    return ids


def _closest_ops():
    import _closest_ref as cref

    ops = []
    # 1,000 points take the wave-per-point kernel, 16,385 the lane-per-point one (the switch lies behind 16,384)
    for config, n in (("parity", 1000), ("tiny", 16385)):
        def closest(env, c=config, n=n):
            return _copy(_mesh(env, c).closest_points(closest_queries(c, n)))

        def closest_check(out, c=config, n=n):
            f = frame(c)
            diff = cref.same_bits(out, cref.closest_ref(f.verts_posed, f.tris, closest_queries(c, n)))
            assert diff is None, diff
        ops.append(Op(f"closest@{n}", closest, closest_check, ("mesh",)))

        def normals(env, c=config, n=n):
            return {"normals": _mesh(env, c).face_normals(face_ids(c, n)).copy()}

        def normals_check(out, c=config, n=n):
            f = frame(c)
            ids = face_ids(c, n)
            a, ab, ac, _ = cref.records(f.verts_posed, f.tris)
            ok = ids < len(f.tris)
            assert np.isnan(out["normals"][~ok]).all() and (~ok).any()
            nrm = np.cross(ab[ids[ok]], ac[ids[ok]])
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            # one float64 rounding per operation of a cross product and a normalisation: a few ulp of a unit vector
            assert np.abs(out["normals"][ok] - nrm).max() < 1e-14
        ops.append(Op(f"face_normals@{n}", normals, normals_check))
    return ops


# ---------------------------------------------------------------- depth

DEPTH_SIZES = ((17, 65), (145, 131))


@functools.lru_cache(maxsize=None)
def depth_image(h, w, nan=True):
    from pedp_hip import synth

    return _ro(synth.depth_image(h, w, seed=2 + w, nan=nan))


def _depth_K(h, w):
    return np.array([[0.9 * w, 0, w / 2 - 0.5], [0, 0.9 * w, h / 2 - 0.5], [0, 0, 1]])


def _depth_ops():
    import test_depth_gpu
    from pedp_hip import depth_filters as df

    ops = []
    for h, w in DEPTH_SIZES:
        tag = f"{h}x{w}"
        ops.append(Op(f"erode@{tag}", lambda env, h=h, w=w: {"depth": df.erode_depth(depth_image(h, w), 2, ctx=env.ctx).copy()},
                      lambda out, h=h, w=w: test_depth_gpu._same(out["depth"], _oracle().erode_depth(depth_image(h, w), 2))))
        ops.append(Op(f"erode_device@{tag}", lambda env, h=h, w=w: _later(depth=df.erode_depth(env.cuda(depth_image(h, w)), 2, ctx=env.ctx)),
                      lambda out, h=h, w=w: test_depth_gpu._same(out["depth"], _oracle().erode_depth(depth_image(h, w), 2))))
        ops.append(Op(f"bilateral@{tag}", lambda env, h=h, w=w: {"depth": df.bilateral_filter_depth(depth_image(h, w), 2, ctx=env.ctx).copy()},
                      lambda out, h=h, w=w: test_depth_gpu._close(out["depth"], _oracle().bilateral_filter_depth(depth_image(h, w), 2))))
        ops.append(Op(f"depth2xyzmap@{tag}", lambda env, h=h, w=w: {"xyz": df.depth2xyzmap(depth_image(h, w), _depth_K(h, w), ctx=env.ctx).copy()},
                      lambda out, h=h, w=w: test_depth_gpu._same(out["xyz"], _oracle().depth2xyzmap(depth_image(h, w), _depth_K(h, w)))))

        def batch_in(h, w):
            from pedp_hip import synth

            d = np.stack([depth_image(h, w), synth.depth_image(h, w, seed=3), synth.depth_image(h, w, seed=4, nan=False)])
            K = _depth_K(h, w)
            return d, np.stack([K, K * 1.01, K * 0.97]).astype(np.float32)
        ops.append(Op(f"depth2xyzmap_batch@{tag}",
                      lambda env, h=h, w=w, b=batch_in: {"xyz": df.depth2xyzmap_batch(*b(h, w), 0.8, ctx=env.ctx).copy()},
                      lambda out, h=h, w=w, b=batch_in: test_depth_gpu._same(out["xyz"], _oracle().depth2xyzmap_batch(*b(h, w), 0.8))))

        def scene_check(out, h=h, w=w):
            o, d = _oracle(), depth_image(h, w, nan=False)
            K = _depth_K(h, w).astype(np.float32)
            b = o.bilateral_filter_depth(o.erode_depth(d))
            test_depth_gpu._close(out["depth"], b)
            # the back-projection and the selection of the library's own filtered image, bit for bit
            x = o.depth2xyzmap_batch(out["depth"][None], K[None], np.inf)[0]
            test_depth_gpu._same(out["xyz"], x)
            assert np.array_equal(out["points"], x[x[..., 2] >= 0.001].astype(np.float64) * 1000.0) and len(out["points"]) > 100

        def scene_host(env, h=h, w=w):
            d, x, p = df.depth_to_scene(depth_image(h, w, nan=False), _depth_K(h, w).astype(np.float32), ctx=env.ctx)
            return {"depth": _host(d), "xyz": _host(x), "points": _host(p)}
        ops.append(Op(f"depth_to_scene@{tag}", scene_host, scene_check, ("ray_in", "pinned")))

        def scene_cuda(env, h=h, w=w):
            buffers = env.keep("depth_to_scene buffers", dict)          # kept across the env's calls: the alternating point buffers
            d, x, p = df.depth_to_scene(env.cuda(depth_image(h, w, nan=False)), _depth_K(h, w).astype(np.float32), buffers=buffers,
                                        ctx=env.ctx)
            return {"depth": _host(d), "xyz": _host(x), "points": _host(p)}
        ops.append(Op(f"depth_to_scene_cuda@{tag}", scene_cuda, scene_check))
    return ops


# ---------------------------------------------------------------- cloud operations

@functools.lru_cache(maxsize=None)
def cloud_scene(seed=0, voxel=None, head=None, **kw):
    import test_cloudops_gpu

    pts = test_cloudops_gpu._scene(seed=seed, **kw)
    if voxel:
        pts = _oracle().voxel_down_sample(pts, voxel)[0]
    return _ro(np.ascontiguousarray(pts[:head]))


@functools.lru_cache(maxsize=None)
def surface(n, seed):
    import test_features_gpu

    return _ro(*test_features_gpu._surface(n, seed=seed))


@functools.lru_cache(maxsize=None)
def features(n, seed):
    return _ro(_oracle().fpfh(*surface(n, seed), 9.0, 100))


def _cloud_ops():
    from pedp_hip import cloud_ops as co

    o = _oracle
    ops = []
    nrm = lambda: np.random.default_rng(1).normal(size=cloud_scene().shape)       # noqa: E731
    for voxel in (5.0, 2.0):
        def vox(env, v=voxel):
            p, n = co.voxel_down_sample(cloud_scene(), v, nrm(), ctx=env.ctx)
            return {"points": p, "normals": n}

        def vox_check(out, v=voxel):
            ref, refn = o().voxel_down_sample(cloud_scene(), v, nrm())
            assert np.array_equal(out["points"], ref) and np.array_equal(out["normals"], refn) and 10 < len(ref) < len(cloud_scene())
        ops.append(Op(f"voxel@{voxel}", vox, vox_check, ("cloud_ws", "pinned")))
    for tag, kw in (("small", dict(seed=3, voxel=6.0)), ("large", dict(seed=3, voxel=3.0))):
        ops.append(Op(f"dbscan@{tag}", lambda env, kw=tuple(kw.items()): {"labels": co.cluster_dbscan(cloud_scene(**dict(kw)), 10.0, 10, ctx=env.ctx)},
                      lambda out, kw=tuple(kw.items()): _eq(out["labels"], o().cluster_dbscan(cloud_scene(**dict(kw)), 10.0, 10), positive=True),
                      ("cloud_ws", "pinned")))
    big = dict(n_plane=14000, n_obj=5000, seed=8, voxel=2.5)
    for n, kw in ((3000, dict(seed=7, voxel=4.0, head=3000)), (4097, dict(head=4097, **big))):     # a wave over ALL points up to 4,096; the grid's shells above
        ops.append(Op(f"knn@{n}", lambda env, kw=tuple(kw.items()): {"avg": co.knn_mean_distance(cloud_scene(**dict(kw)), 20, ctx=env.ctx)},
                      lambda out, kw=tuple(kw.items()): _eq(out["avg"], o().knn_mean_distance(cloud_scene(**dict(kw)), 20)), ("cloud_ws",)))
    for (radius, max_nn), head in (((2.0, 5), 1500), ((6.0, 30), 6000)):
        kw = tuple(dict(seed=13, voxel=1.5, head=head).items())

        def normals_check(out, kw=kw, r=radius, m=max_nn):
            ref = o().estimate_normals(cloud_scene(**dict(kw)), r, m)
            assert out["normals"].shape == ref.shape and np.abs(out["normals"] - ref).max() < 1e-9
        ops.append(Op(f"normals@{radius:g}_{max_nn}",
                      lambda env, kw=kw, r=radius, m=max_nn: {"normals": co.estimate_normals(cloud_scene(**dict(kw)), r, m, ctx=env.ctx)},
                      normals_check, ("cloud_ws",)))
    for n, radius in ((400, 3.0), (1500, 8.0)):
        def fpfh_check(out, n=n, r=radius):
            ref = o().fpfh(*surface(n, n + 100), r, 100)
            off = np.abs(out["fpfh"] - ref) > 1e-9 * (1.0 + np.abs(ref))
            assert out["fpfh"].shape == ref.shape == (n, 33) and off.any(axis=1).mean() <= 0.002, f"{off.any(axis=1).sum()} of {n} points differ"
        ops.append(Op(f"fpfh@{n}", lambda env, n=n, r=radius: {"fpfh": co.compute_fpfh(*surface(n, n + 100), r, 100, ctx=env.ctx)},
                      fpfh_check, ("cloud_ws",)))
    for ns, nt in ((65, 300), (900, 2500)):
        ops.append(Op(f"feature_match@{ns}x{nt}",
                      lambda env, ns=ns, nt=nt: {"idx": co.match_features(features(900, 3)[:ns], features(2500, 4)[:nt], ctx=env.ctx)},
                      lambda out, ns=ns, nt=nt: _eq(out["idx"], o().feature_match(features(900, 3)[:ns], features(2500, 4)[:nt])), ("cloud_ws",)))
    for tag, kw in (("small", dict(seed=9, voxel=6.0)), ("large", dict(seed=9, voxel=3.0))):
        def plane(env, kw=tuple(kw.items())):
            p, inl = co.segment_plane(cloud_scene(**dict(kw)), 1.0, 3, 100, seed=7, ctx=env.ctx)
            return {"plane": p, "inliers": inl}

        def plane_check(out, kw=tuple(kw.items())):
            rp, ri = o().segment_plane(cloud_scene(**dict(kw)), 1.0, 100, seed=7)
            assert np.array_equal(out["inliers"], ri) and len(ri) > 200 and np.abs(out["plane"] - rp).max() < 1e-12
        ops.append(Op(f"segment_plane@{tag}", plane, plane_check, ("cloud_ws", "pinned")))
    for first in (True, False):
        def fused(env, first=first):
            p, n, counts, status = co.preprocess_source_fused(frame_scene("parity"), 4 if first else 5, 2.0, 200, first_frame=first, seed=0,
                                                              ctx=env.ctx)
            out = {"points": p, "counts": np.asarray(counts, np.int64), "status": np.asarray(status, np.int32)}
            if n is not None:
                out["normals"] = n
            return out

        def fused_check(out, first=first):
            """The chain of test_preprocess_source_flow_matches_oracle_chain (box = False) from the oracle's operations."""
            scene = frame_scene("parity")
            down, _ = o().voxel_down_sample(scene, 4 if first else 5)
            _, inl = o().segment_plane(down, 2.0, 200, seed=0)
            rest = np.delete(down, inl, axis=0)
            labels = o().cluster_dbscan(rest, 10, 10)
            ids, counts = np.unique(labels[labels >= 0], return_counts=True)
            big = rest[labels == ids[np.argmax(counts)]]
            ref = big[o().remove_statistical_outlier(big, 75, 0.01)]
            assert int(out["status"]) == 0 and np.array_equal(out["points"], ref) and 200 < len(ref) < len(down)
            if first:
                assert np.abs(out["normals"] - o().estimate_normals(ref, 2.0, 5)).max() < 1e-9
        ops.append(Op(f"preprocess_fused@{'first' if first else 'tracking'}", fused, fused_check, ("cloud_ws", "pinned")))
    return ops


def _eq(got, ref, positive=False):
    assert got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got, ref)
    if positive:
        assert ref.max() >= 0


# ---------------------------------------------------------------- registration

@functools.lru_cache(maxsize=None)
def reg_case(name):
    """(source, target, target normals, radius, init) of the two registration sizes: the blob of the nearest-neighbour
    matrix (300 x 2,100) and the parity frame (23,040 x 2,000)."""
    if name == "blob":
        import _nn_cases
        import test_nn_matrix_gpu

        src, tgt, nrm = _nn_cases.blob(300, 2100, 11)
        return _ro(src, tgt, nrm) + (0.1, test_nn_matrix_gpu._init(tgt))      # the matrix's typical radius and start
    f = frame("parity")
    return (frame_scene("parity"), _ro(f.model_points), _ro(f.normals), 10.0, f.icp_init())


POSE_TOL = 1e-5          # test_icp_gpu's


def _clouds(env, name):
    """Handles of an entry's own, made by the call (and dropped by it: the pool's buffers go round)."""
    from pedp_hip import _lib

    src, tgt, nrm, r, init = reg_case(name)
    return _lib.Cloud(env.ctx, src), _lib.Cloud(env.ctx, tgt, nrm), r, init


def _icp_out(res):
    out = {"T": res["T"], "fitness": np.asarray(res["fitness"]), "inlier_rmse": np.asarray(res["inlier_rmse"]),
           "iters": np.asarray(res["iters"], np.int32)}
    for k in ("corr", "trace"):
        if k in res:
            out[k] = np.array(res[k], copy=True)
    return out


def _icp_check(out, name, estimator):
    src, tgt, nrm, r, init = reg_case(name)
    ref = _oracle().icp(src, tgt, nrm, r, init, estimator=estimator, max_iter=12, rel_fitness=-1, rel_rmse=-1)
    if name == "blob":                       # the comparison of test_nn_matrix_gpu
        import _nn_cases
        import test_nn_matrix_gpu

        res = dict(out, iters=int(out["iters"]), fitness=float(out["fitness"]), inlier_rmse=float(out["inlier_rmse"]))
        test_nn_matrix_gpu._same(res, ref, 12, _nn_cases.extent(tgt))
        assert ref["fitness"] > 0
        return
    assert int(out["iters"]) == ref["iters"] == 12
    assert np.array_equal(out["corr"], ref["corr"]) and float(out["fitness"]) == ref["fitness"] > 0
    assert abs(float(out["inlier_rmse"]) - ref["inlier_rmse"]) < 1e-9
    assert np.abs(out["T"] - ref["T"]).max() < POSE_TOL
    assert np.abs(out["trace"][:, :2] - ref["trace"][:, :2]).max() < 1e-9
    assert np.abs(out["trace"][:, 2:] - ref["trace"][:, 2:]).max() < POSE_TOL


def _start_poses(name, n):
    from pedp_hip import synth

    if name == "parity":
        return np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(n)])
    import test_nn_matrix_gpu

    tgt = reg_case(name)[1]
    return np.stack([test_nn_matrix_gpu._init(tgt, deg=1.0 + 0.25 * k, shift=0.01 * k) for k in range(n)])


def _registration_ops():
    from pedp_hip import _lib

    ops = []
    for name in ("blob", "parity"):
        def nn(env, name=name):
            s, t, _, init = _clouds(env, name)
            idx, d2 = _lib.nn(env.ctx, s, t, init)
            return {"idx": idx, "d2": d2}

        def nn_check(out, name=name):
            src, tgt, _, _, init = reg_case(name)
            ridx, rd2 = _oracle().nn(_oracle().transform(init, src), tgt, kdtree=name != "blob")
            assert np.array_equal(out["idx"], ridx) and np.array_equal(out["d2"].view(np.uint64), rd2.view(np.uint64))
        ops.append(Op(f"nn@{name}", nn, nn_check, ("cloud_ws",)))

        for est, label in ((_lib.POINT_TO_PLANE, "icp"), (_lib.POINT_TO_POINT, "icp_point")):
            def icp(env, name=name, est=est):
                s, t, r, init = _clouds(env, name)
                return _icp_out(_lib.icp(env.ctx, s, t, r, init, estimator=est, max_iteration=12, relative_fitness=-1, relative_rmse=-1,
                                         want_corr=True, want_trace=True))
            ops.append(Op(f"{label}@{name}", icp, lambda out, name=name, est=est: _icp_check(out, name, est),
                          ("cloud_ws",) if label == "icp" else ()))

        def begin_end(env, name=name):
            s, t, r, init = _clouds(env, name)
            _lib.icp_begin(env.ctx, s, t, r, init, max_iteration=12, relative_fitness=-1, relative_rmse=-1, want_trace=True)
            return _icp_out(_lib.icp_end(env.ctx, want_corr=True))
        ops.append(Op(f"icp_begin_end@{name}", begin_end, lambda out, name=name: _icp_check(out, name, _lib.POINT_TO_PLANE)))

        def batched(env, name=name):
            s, t, r, _ = _clouds(env, name)
            T, fit, rmse = _lib.icp_batched(env.ctx, s, t, r, _start_poses(name, 4), max_iteration=3)
            return {"T": T, "fitness": fit, "inlier_rmse": rmse}

        def batched_check(out, name=name, n=4, limit=3):
            src, tgt, nrm, r, _ = reg_case(name)
            inits = _start_poses(name, n)
            for b in range(n):
                ref = _oracle().icp(src, tgt, nrm, r, inits[b], max_iter=limit, rel_fitness=-1, rel_rmse=-1)
                assert np.abs(out["T"][b] - ref["T"]).max() < POSE_TOL and out["fitness"][b] == ref["fitness"], b
        ops.append(Op(f"icp_batched@{name}", batched, batched_check, ("cloud_ws",)))

        def batched_ex(env, name=name):
            s, t, r, _ = _clouds(env, name)
            radii = r * np.cumprod(np.random.default_rng(2).uniform(0.8, 1.2, 9))
            T, fit, rmse, its = _lib.icp_batched_ex(env.ctx, s, t, radii, _start_poses(name, 9), max_iteration=30)
            return {"T": T, "fitness": fit, "inlier_rmse": rmse, "iters": its}

        def batched_ex_check(out, name=name):
            src, tgt, nrm, r, _ = reg_case(name)
            radii = r * np.cumprod(np.random.default_rng(2).uniform(0.8, 1.2, 9))
            inits = _start_poses(name, 9)
            for b in (0, 7):
                ref = _oracle().icp(src, tgt, nrm, radii[b], inits[b])
                assert out["fitness"][b] == ref["fitness"] and out["iters"][b] == ref["iters"], b
                assert np.abs(out["T"][b] - ref["T"]).max() < POSE_TOL, b
        ops.append(Op(f"icp_batched_ex@{name}", batched_ex, batched_ex_check))

        def ransac(env, name=name):
            src, tgt, _, _, _ = reg_case(name)
            s, t = _lib.Cloud(env.ctx, src), _lib.Cloud(env.ctx, tgt)        # (no normals on either side: no angle test)
            ok, T = _lib.ransac_hypotheses(env.ctx, s, t, _ransac_corr(name), 99, 1000, 256, 0.9, _ransac_dist(name), 0.6)
            return {"accepted": ok, "T": T}

        def ransac_check(out, name=name):
            src, tgt, nrm, _, _ = reg_case(name)
            corr = _ransac_corr(name)
            for k in list(range(0, 256, 17)) + list(np.flatnonzero(out["accepted"])[:20]):
                ok_ref, T_ref = _oracle().ransac_hypothesis(99, 1000 + k, src, None, tgt, None, corr, 0.9, _ransac_dist(name), 0.6)
                assert bool(out["accepted"][k]) == ok_ref, k
                assert np.allclose(out["T"][k], T_ref, rtol=0, atol=1e-9 * (1 + np.abs(T_ref).max())), k
        ops.append(Op(f"ransac_hypotheses@{name}", ransac, ransac_check))
    return ops


@functools.lru_cache(maxsize=None)
def _ransac_corr(name):
    """The nearest target row of every source row at the case's start pose: correspondences most draws accept."""
    src, tgt, _, _, init = reg_case(name)
    return _ro(_oracle().nn(_oracle().transform(init, src), tgt, kdtree=True)[0].astype(np.int32))


def _ransac_dist(name):
    return 0.2 if name == "blob" else 10.0


# ---------------------------------------------------------------- pose arithmetic, pose errors, frame statistics

def _pose_ops():
    import _pose_ref
    import test_pose_gpu as tp
    from pedp_hip import pose

    cfg = tp.BRANCHES[1]
    ops = []
    for B in (1, 252):
        def inputs(B=B):
            rng = np.random.default_rng(B + 100)
            return tp._poses(B, rng), tp._outputs(B, 3, rng), tp._outputs(B, 3, rng)

        def update(env, inputs=inputs):
            P, t, r = inputs()
            got, td, rd = pose.pose_update(env.cuda(t), env.cuda(r), env.cuda(P), want_deltas=True, **cfg)
            return _later(poses=got, trans_delta=td, rot_mat_delta=rd)

        def update_check(out, inputs=inputs):
            P, t, r = inputs()
            for k, w in zip(("poses", "trans_delta", "rot_mat_delta"), _pose_ref.pose_update(t, r, P, **cfg)):
                tp._assert_bits(out[k], w, k)
        ops.append(Op(f"pose_update@{B}", update, update_check))
    for n in (257, 10000):
        pts = lambda n=n: np.random.default_rng(n).normal(0, [40.0, 25.0, 10.0], (n, 3))       # noqa: E731
        ops.append(Op(f"max_pair_distance@{n}", lambda env, pts=pts: {"d": np.asarray(pose.max_pair_distance(env.cuda(pts())))},
                      lambda out, pts=pts: _bits_equal(out["d"], np.asarray(_pose_ref.max_pair_distance(pts())))))
    return ops


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64)), f"{a!r} != {b!r}"


def _metrics_ops():
    import _metrics_ref
    import test_metrics_gpu as tm
    from pedp_hip import metrics

    ops = []
    for n in (129, 513):
        def inputs(n=n):
            rng = np.random.default_rng(31 + n)
            preds, gts = tm.random_poses(rng, 4)
            return preds, gts, rng.uniform(-0.06, 0.06, (n, 3))

        def errors(env, inputs=inputs):
            preds, gts, pts = inputs()
            p, g, m = env.cuda(preds), env.cuda(gts), env.cuda(pts)
            return _later(add=metrics.add_err_batch(p, g, m), adds=metrics.adds_err_batch(p, g, m))

        def errors_check(out, inputs=inputs):
            preds, gts, pts = inputs()
            for kind in ("add", "adds"):
                assert tm.same(out[kind], _metrics_ref.pose_errors(kind, preds, gts, pts)), kind
        ops.append(Op(f"pose_errors@{n}", errors, errors_check))
    return ops


def _stats_ops():
    import _estimator_ref
    import test_estimator_gpu as te
    from pedp_hip.estimator import mask_depth_stats

    ops = []
    for h, w in ((61, 83), (145, 131)):
        def inputs(h=h, w=w):
            rng = np.random.default_rng(1000 * h + 10 * w)
            return te._depth(h, w, rng, True), te._mask(h, w, rng, "float32")

        def stats(env, inputs=inputs):
            d, m = inputs()
            rec = mask_depth_stats(env.cuda(d), env.cuda(m))
            return {"counts": np.array([rec[k] for k in te.FIELDS], np.int64), "median": np.asarray(rec["median"])}

        def stats_check(out, inputs=inputs):
            want = _estimator_ref.stats(*inputs())
            assert out["counts"].tolist() == [want[k] for k in te.FIELDS] and want["n_med"] > 10
            assert out["median"].dtype == np.float32 and _estimator_ref.same_bits(out["median"], want["median"])
        ops.append(Op(f"mask_depth_stats@{h}x{w}", stats, stats_check))
    return ops


# ---------------------------------------------------------------- defect map

def _defect_ops():
    import _defect_map_ref as dref
    import test_defect_map_gpu as td
    from pedp_hip import DefectMap

    def dmap(env):
        m = td.model("torus16000")
        dm = env.keep("defect map", lambda: DefectMap((m.verts, m.tris), env.ctx))
        dm.clear()
        return m, dm

    ops = []
    for n in (65, 4097):
        def add(env, n=n):
            m, dm = dmap(env)
            dm.add(*td.rows(m.F, n, n))
            out = _copy(dm.faces())
            out["stats"] = np.array([dm.stats()[k] for k in ("observations", "rows_added", "rows_ignored")], np.int64)
            return out

        def add_check(out, n=n):
            m = td.model("torus16000")
            st = dref.State(m.F).add(*td.rows(m.F, n, n))
            td.same_faces(out, st.faces())
            assert out["stats"].tolist() == [st.stats()[k] for k in ("observations", "rows_added", "rows_ignored")]
        ops.append(Op(f"defect_add_faces@{n}", add, add_check))
    for density in (0.01, 0.3):
        def regions(env, density=density):
            m, dm = dmap(env)
            for o in td.two_observations(m.F, density, int(density * 100) + 1):
                dm.add(*o)
            got = dm.regions(0.25, 1, 1)
            return {k: np.array(v, copy=True) for k, v in got.items()}

        def regions_check(out, density=density):
            m = td.model("torus16000")
            o1, o2 = td.two_observations(m.F, density, int(density * 100) + 1)
            st = dref.State(m.F).add(*o1).add(*o2)
            got = dict(out, n_regions=int(out["n_regions"]))
            td.same_regions(got, dref.regions(m, st, 0.25, 1, 1))
            assert got["n_regions"] >= 1
        ops.append(Op(f"defect_regions@{density}", regions, regions_check))
    return ops


# ---------------------------------------------------------------- host Cloud creation (the pinned block's +12288)

def _cloud_create_ops():
    """pedp_cloud_create stages the cloud's box through the page-locked block; what it made is read back through pedp_nn of
    the cloud against itself (every row its own neighbour at distance 0) and against a shifted copy."""
    from pedp_hip import _lib

    ops = []
    for n in (257, 2049):
        pts = lambda n=n: np.random.default_rng(n).normal(0, [30.0, 20.0, 5.0], (n, 3)) + [5.0, -3.0, 400.0]     # noqa: E731

        def create(env, pts=pts):
            p = pts()
            a, b = _lib.Cloud(env.ctx, p), _lib.Cloud(env.ctx, p[::-1] + 0.25)
            idx, d2 = _lib.nn(env.ctx, a, b)
            return {"idx": idx, "d2": d2}

        def create_check(out, pts=pts):
            p = pts()
            ridx, rd2 = _oracle().nn(p, np.ascontiguousarray(p[::-1] + 0.25), kdtree=True)
            assert np.array_equal(out["idx"], ridx) and np.array_equal(out["d2"].view(np.uint64), rd2.view(np.uint64))
        ops.append(Op(f"cloud_create@{n}", create, create_check, ("pinned",)))
    return ops


# ---------------------------------------------------------------- renderer, crops, network kernels (stream-dispatched)

def _render_ops():
    import _render_ref as rref
    import test_render_gpu as tr
    from pedp_hip.compat import nvdiffrast_render, projection_matrix_from_intrinsics

    H, W = 48, 64
    ops = []
    for case in (tr.CASES[0], tr.CASES[-1]):
        config, N, textured, crop, output_size, use_light, get_normal = case

        def inputs(config=config, N=N, crop=crop):
            return tr._torus(config) + (tr._poses(N, seed=N), tr._K(W, H), tr._crop_boxes(N, H, W) if crop else None)

        def render(env, case=case, inputs=inputs):
            config, N, textured, crop, output_size, use_light, get_normal = case
            v, t, n, poses, K, bbox = inputs()
            mt = env.keep(("render mesh", config, textured), lambda: tr._mesh_tensors(v, t, n, textured))
            extra = {}
            col, dep, nrm = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=env.cuda(poses), mesh_tensors=mt,
                                              bbox2d=None if bbox is None else env.cuda(bbox), output_size=output_size,
                                              use_light=use_light, get_normal=get_normal, light_dir=np.array([0, 0, 1]), extra=extra)
            return _later(color=col, depth=dep, xyz=extra["xyz_map"], normal=nrm)

        def render_check(out, case=case, inputs=inputs):
            config, N, textured, crop, output_size, use_light, get_normal = case
            v, t, n, poses, K, bbox = inputs()
            mt = tr._mesh_tensors(v, t, n, textured)
            oh, ow = (H, W) if output_size is None else output_size
            proj = projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32)
            kw = {"tex": mt["tex"][0].cpu().numpy(), "uv": mt["uv"].cpu().numpy()} if textured else {"vcolor": mt["vertex_color"].cpu().numpy()}
            want = rref.render(v, t, n, poses, proj, H, W, oh, ow, bbox=bbox, get_normal=get_normal, use_light=use_light,
                               light_color=None, light_dir=np.array([0, 0, 1]), **kw)
            assert (want[1] != 0).sum() > 20 * N
            for w, what in zip(want, ("color", "depth", "normal", "xyz")):
                if w is None:
                    assert what not in out
                else:
                    tr._assert_bits(out[what], w, what)
        ops.append(Op(f"render@{config}_{N}", render, render_check))
    return ops


@functools.lru_cache(maxsize=None)
def clip_case(config, N, H, W):
    """Clip-space vertices of N poses of a torus (the inputs of test_interpolate_bit_equal_to_restatement) and its faces."""
    import _render_ref as rref
    import test_render_gpu as tr
    from pedp_hip.compat import projection_matrix_from_intrinsics

    v, t, _ = tr._torus(config)
    M, win = rref.pose_records(projection_matrix_from_intrinsics(tr._K(W, H), H, W, 0.001, 100).astype(np.float32), tr._poses(N, seed=40),
                               None, H, W)
    return _ro(np.stack([rref.clip_vertices(v, M[i], win[i]) for i in range(N)]), t)


@functools.lru_cache(maxsize=None)
def raster_ref(config, N, H, W):
    import _render_ref as rref

    clip, t = clip_case(config, N, H, W)
    return _ro(rref.rasterize(clip, t, H, W))


def _raster_ops():
    import _render_ref as rref
    import test_render_gpu as tr
    from pedp_hip.compat import dr

    ops = []
    for config, N, H, W in (("tiny", 3, 24, 32), ("parity", 3, 32, 48)):
        def raster(env, a=(config, N, H, W)):
            clip, t = clip_case(*a)
            rast, _ = dr.rasterize(None, env.cuda(clip), env.cuda(t), (a[2], a[3]))
            return _later(rast=rast)

        def raster_check(out, a=(config, N, H, W)):
            clip, t = clip_case(*a)
            assert (out["rast"][..., 3] > 0).sum() > 200
            tr._assert_bits(out["rast"], raster_ref(*a), "rast")
        ops.append(Op(f"rasterize@{config}", raster, raster_check))

        def attrs(a=(config, N, H, W)):
            clip, t = clip_case(*a)
            return np.random.default_rng(3).normal(size=(clip.shape[1], 3)).astype(np.float32), raster_ref(*a)

        def interp(env, a=(config, N, H, W), attrs=attrs):
            attr, rast = attrs()
            return _later(out=dr.interpolate(env.cuda(attr), env.cuda(rast), env.cuda(clip_case(*a)[1]))[0])
        ops.append(Op(f"interpolate@{config}", interp,
                      lambda out, a=(config, N, H, W), attrs=attrs: tr._assert_bits(out["out"], rref.interpolate(*attrs(), clip_case(*a)[1]), "interpolate")))
    for th, tw in ((1, 1), (13, 21)):
        def tex_in(th=th, tw=tw):
            return tr._texture_case(3, th, tw, 3, False, np.random.default_rng(th + tw))

        def texture(env, tex_in=tex_in):
            tex, uv, _ = tex_in()
            return _later(out=dr.texture(env.cuda(tex), env.cuda(uv), filter_mode="linear"))

        def texture_check(out, tex_in=tex_in):
            tex, uv, zero = tex_in()
            want = rref.texture(tex, uv)
            assert not want[:, zero].any() and want[:, ~zero].all()
            tr._assert_bits(out["out"], want, "texture")
        ops.append(Op(f"texture@{th}x{tw}", texture, texture_check))
    return ops


def _crop_ops():
    import _crop_ref as cref
    import test_crop_gpu as tc
    from pedp_hip.compat import warp_perspective
    from pedp_hip.crop import _crop_window

    ops = []
    Hs, Ws, h, w = 37, 53, 29, 41
    for B in (4, 16):
        def warp_in(B=B):
            frame = np.random.default_rng(B + 3).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
            return frame, tc._homographies(B, Hs, Ws, h, w, seed=B)

        def warp(env, B=B, warp_in=warp_in):
            frame, M = warp_in()
            src = env.cuda(frame).permute(2, 0, 1)[None].expand(B, -1, -1, -1)
            return _later(out=warp_perspective(src, env.cuda(M), (h, w), mode="bilinear", align_corners=False))
        ops.append(Op(f"warp_perspective@{B}", warp,
                      lambda out, warp_in=warp_in: tc._assert_bits(out["out"], cref.warp(warp_in()[0].transpose(2, 0, 1)[None], warp_in()[1], (h, w),
                                                                                         "bilinear", False), "warp")))
    for B in (4, 600):
        def window(env, B=B):
            tf, bb = _crop_window(env.cuda(tc._poses(B, seed=4)), tc.K_, 0.1 * 1.4 / 2, tc.CROP, tc.CROP, (tc.CROP - 1, tc.CROP - 1), True)
            return _later(tf=tf, bbox=bb)

        def window_check(out, B=B):
            tf_r, bb_r = cref.crop_window(tc._poses(B, seed=4), tc.K_, np.float32(0.1 * 1.4 / 2), tc.CROP, tc.CROP, (tc.CROP - 1, tc.CROP - 1))
            tc._assert_bits(out["tf"], tf_r, "tf_to_crops")
            tc._assert_bits(out["bbox"], bb_r, "bbox2d")
        ops.append(Op(f"crop_window@{B}", window, window_check))
    fields = ("rgbAs", "rgbBs", "xyz_mapAs", "xyz_mapBs", "normalAs", "normalBs", "depthAs", "depthBs", "tf_to_crops")
    for variant, label in ((0, "crop_refiner"), (1, "crop_scorer")):
        for B in (4, 16):
            def batch(env, variant=variant, B=B):
                scene = env.keep("crop scene", tc._scene)                  # rendered once per context, on its stream
                got = tc._fused(variant, tc._hypotheses(B, scene[-1], seed=B), scene, True, variant == 0)
                return _later(**{k: getattr(got, k, None) for k in fields})

            def batch_check(out, variant=variant, B=B):
                scene = tc._scene()
                want = tc._unfused(variant, tc._hypotheses(B, scene[-1], seed=B), scene, True, variant == 0)
                for k, v in want.items():
                    tc._assert_bits(out[k], v, k)
                assert np.abs(out["xyz_mapBs"]).sum() > 0 and out["rgbBs"].sum() > 0
            ops.append(Op(f"{label}@{B}", batch, batch_check))
    return ops


def _network_ops():
    import _linear_ref as lr
    import test_attention_gpu as ta
    import test_conv_gpu as tcv
    import test_conv_strided_gpu as tcs
    from pedp_hip import linear as L
    from pedp_hip.attention import mha_core
    from pedp_hip.conv import conv3x3, conv_strided

    ops = []
    for shape in ((1, 1, 1, 128), (3, 5, 7, 128)):
        tag = "x".join(map(str, shape))

        def conv(env, shape=shape):
            c = tcv._case(*shape, shape[3], True)
            return _later(y=conv3x3(c["x"], c["packed"], residual=c["res"], relu=True))
        ops.append(Op(f"conv3x3@{tag}", conv, lambda out, shape=shape, tag=tag: tcv._check(
            _as_half(out["y"]), tcv._case(*shape, shape[3], True), True, True, f"conv3x3 {tag}")))
    for shape in ((1, 1, 1, 64, 128), (3, 5, 7, 64, 128)):
        tag = "x".join(map(str, shape))
        ops.append(Op(f"conv_strided@{tag}", lambda env, shape=shape: _later(y=conv_strided(tcs._down_case(*shape)["x"], tcs._down_case(*shape)["packed"], relu=True)),
                      lambda out, shape=shape, tag=tag: tcs._check(_as_half(out["y"]), tcs._down_case(*shape), True, f"3x3/2 {tag}")))
    for B, S, Hh in ((2, 3, 4), (2, 65, 4)):
        def mha(env, B=B, S=S, Hh=Hh):
            q, k, v = ta._case(B, S, Hh)[:3]
            return _later(o=mha_core(env.cuda(np.concatenate([q, k, v], axis=2)), Hh))

        def mha_check(out, B=B, S=S, Hh=Hh):
            _, _, _, o_ref, bound = ta._case(B, S, Hh)
            ta._check(out["o"], o_ref, bound, f"mha {B} x {S} x {Hh}")
        ops.append(Op(f"mha@{B}x{S}x{Hh}", mha, mha_check))
    for M, K, N in ((1, 64, 64), (130, 64, 192)):
        def linear(env, M=M, K=K, N=N):
            d = lr.inputs(M, K, N, seed=M + K + N)
            packed = L.PackedLinear(env.cuda(d["w"]), env.cuda(d["bias"]))
            return _later(y=L.linear(env.cuda(d["x"]), packed, relu=True))

        def linear_check(out, M=M, K=K, N=N):
            d = lr.inputs(M, K, N, seed=M + K + N)
            y_ref, bound = lr.reference(x=d["x"], w=d["w"], bias=d["bias"], epilogue=lr.RELU, pos_a=True)
            assert lr.used_share(out["y"], y_ref, bound) < 1
        ops.append(Op(f"linear@{M}x{K}x{N}", linear, linear_check))
    for B, S in ((1, 1), (3, 16)):
        def pool(env, B=B, S=S):
            d = lr.pool_inputs(B, S, 6, seed=B + S, loud_next=True)
            packed = L.PackedLinear(env.cuda(d["w"]), env.cuda(d["bias"]))
            return _later(y=L.token_pool(env.cuda(d["x"])[:B * S], B, packed))

        def pool_check(out, B=B, S=S):
            d = lr.pool_inputs(B, S, 6, seed=B + S, loud_next=True)
            ref, bound = lr.pool_reference(d["x"], B, S, d["w"], d["bias"])
            assert lr.used_share(out["y"], ref, bound) < 1
        ops.append(Op(f"token_pool@{B}x{S}", pool, pool_check))
    return ops


def _as_half(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a))


# ================================================================ the catalogue

BUILDERS = (_ray_ops, _project_ops, _closest_ops, _depth_ops, _cloud_ops, _registration_ops, _cloud_create_ops, _pose_ops,
            _metrics_ops, _stats_ops, _defect_ops, _render_ops, _raster_ops, _crop_ops,
            _network_ops)

GROUPS = {
    "ray_in": "the ray caster's host staging: rays in host mode, the projection in host mode, depth_to_scene",
    "pinned": "the page-locked block's +8192 and +12288: projection, depth_to_scene, segment_plane, voxel, dbscan, preprocess_source_fused, "
              "host Cloud creation",
    "cloud_ws": "sort_ws / ops / ops_small / chain / cloud_pool: cloud operations, preprocess_source_fused, nn, icp, icp_batched",
    "mesh": "one mesh handle: rays, projection, closest points, set_pose",
}


@functools.lru_cache(maxsize=None)
def catalogue():
    ops = [op for build in BUILDERS for op in build()]
    names = [op.name for op in ops]
    assert len(set(names)) == len(names), "catalogue names must be unique"
    for op in ops:
        assert op.group <= set(GROUPS), op
    return tuple(ops)


def pairs_by_size(ops):
    """base operation -> its (smaller, larger) entries, in catalogue order."""
    by = {}
    for op in ops:
        by.setdefault(op.base, []).append(op)
    return {b: tuple(v) for b, v in by.items() if len(v) == 2}
