"""Every public call is a function of its arguments: whatever ran on its context before, it gives the bytes a fresh
context gives.  The catalogue of tests/_history_ops.py (one entry per operation at two sizes, each with the reference of
its module's own tests) is run on fresh contexts (a), then under seeded shuffles (b), size changes (c), neighbours on the
state the modules share (d), pooled buffers with stale tails (e), device mode followed by host mode without a wait (f),
two contexts in turn (g) and with a registration pending on the context (h).

Entries compared through their `check` instead of byte for byte would be listed in CHECK_ONLY with the line of
include/pedp.h that permits it; there are none."""
import numpy as np
import pytest

import _history_ops as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# name of a catalogue entry -> the contract line that says its bits are not promised (then (a) .. (g) use its check)
CHECK_ONLY = {}

SEEDS = (11, 12, 13)
OPS = None


def ops():
    global OPS
    if OPS is None:
        OPS = H.catalogue()
    return OPS


def by_name():
    return {op.name: op for op in ops()}


NAMES = None


def _names():
    """The catalogue's names for parametrize (building the catalogue needs no GPU)."""
    global NAMES
    if NAMES is None:
        NAMES = [op.name for op in ops()]
    return NAMES


_fresh = {}


def fresh(op):
    """The yardstick: op on a fresh context, kept for the module.  The first use runs it on TWO fresh contexts, which must
    agree byte for byte, and through its check."""
    if op.name not in _fresh:
        results = []
        for _ in range(2):
            with H.Env() as env:
                results.append(H.outputs(H.call(op, env)))
        if op.name not in CHECK_ONLY:
            diff = H.same_bytes(results[0], results[1])
            assert diff is None, f"{op.name}: two fresh contexts differ: {diff}"
        for r in results:
            op.check(r)
        for v in results[0].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _fresh[op.name] = results[0]
    return _fresh[op.name]


def yardstick(some):
    return {op.name: fresh(op) for op in some}


# ---------------------------------------------------------------- a. fresh is right and repeatable

@pytest.mark.parametrize("name", _names())
def test_a_fresh_context_is_right_and_repeatable(name):
    out = fresh(by_name()[name])
    assert out and all(isinstance(v, np.ndarray) for v in out.values())


# ---------------------------------------------------------------- b. seeded histories

@pytest.mark.parametrize("seed", SEEDS)
def test_b_seeded_histories_on_one_context(seed):
    want = yardstick(ops())
    with H.Env() as env:
        assert H.replay(H.histories(ops(), seed), env, want, seed=seed, check_only=CHECK_ONLY) == 2 * len(ops())


# ---------------------------------------------------------------- c. grow and shrink

@pytest.mark.parametrize("base", sorted(H.pairs_by_size(ops())))
def test_c_large_small_large_small(base):
    small, large = H.pairs_by_size(ops())[base]
    with H.Env() as env:
        H.replay([large, small, large, small], env, yardstick([small, large]), seed=f"grow and shrink: {base}", check_only=CHECK_ONLY)


# ---------------------------------------------------------------- d. neighbours on shared state

def _group_cases():
    return [(g, a.name) for g in H.GROUPS for a in ops() if g in a.group]


@pytest.mark.parametrize("group,first", _group_cases())
def test_d_neighbours_on_shared_state(group, first):
    """Every ordered pair (A, B) of the group with A = `first`, as A, B, A: one context per A, the pairs one behind the
    other (A, B1, A, B2, A, ...), each A compared as soon as it returns."""
    members = [op for op in ops() if group in op.group]
    a = by_name()[first]
    chain = [a]
    for b in members:
        if b is not a:
            chain += [b, a]
    with H.Env() as env:
        H.replay(chain, env, yardstick(members), seed=f"{group}: A = {a.name}, every B of the group, as A, B, A", check_only=CHECK_ONLY)


# ---------------------------------------------------------------- e. stale tails in pooled buffers

def _nn_icp(env, src, tgt, nrm, r, init):
    from pedp_hip import _lib

    s, t = _lib.Cloud(env.ctx, src), _lib.Cloud(env.ctx, tgt, nrm)
    idx, d2 = _lib.nn(env.ctx, s, t, init)
    res = H._icp_out(_lib.icp(env.ctx, s, t, r, init, max_iteration=12, relative_fitness=-1, relative_rmse=-1, want_corr=True,
                              want_trace=True))
    s.close()
    t.close()
    return dict(res, idx=idx, d2=d2)


def test_e_a_smaller_cloud_in_a_dead_clouds_buffers():
    """A target of 2,100 rows with normals is registered against and destroyed; one of 2,049 rows of other data takes its
    buffers from the pool, tail included.  The same with sources of 300 and then 257 rows."""
    import _nn_cases
    import test_nn_matrix_gpu

    src, tgt, nrm, r, init = H.reg_case("blob")
    src2, tgt2, nrm2 = _nn_cases.blob(257, 2049, 23)
    init2 = test_nn_matrix_gpu._init(tgt2)
    with H.Env() as env:
        want_tgt = _nn_icp(env, src, tgt2, nrm2, r, init2)
    with H.Env() as env:
        want_src = _nn_icp(env, src2, tgt, nrm, r, init)
    ref = H._oracle().icp(src, tgt2, nrm2, r, init2, max_iter=12, rel_fitness=-1, rel_rmse=-1)
    assert np.array_equal(want_tgt["corr"], ref["corr"]) and ref["fitness"] > 0          # fresh is right
    with H.Env() as env:
        first = _nn_icp(env, src, tgt, nrm, r, init)                                    # 300 x 2,100, then destroyed
        want = fresh(by_name()["icp@blob"])
        assert H.same_bytes({k: first[k] for k in want}, want) is None
        diff = H.same_bytes(_nn_icp(env, src, tgt2, nrm2, r, init2), want_tgt)           # 2,049 rows in the 2,100-row buffers
        assert diff is None, f"target of 2,049 rows after one of 2,100: {diff}"
        diff = H.same_bytes(_nn_icp(env, src2, tgt, nrm, r, init), want_src)             # 257 rows in the 300-row buffers
        assert diff is None, f"source of 257 rows after one of 300: {diff}"


# ---------------------------------------------------------------- f. device mode, then host mode at once

def test_f_device_mode_then_host_mode_without_a_wait():
    from pedp_hip import depth_filters

    names = ("erode_device@145x131", "rays_device@parity", "project_jet_post@parity", "cloud_create@2049")
    want = yardstick([by_name()[n] for n in names])
    f, d = H.frame("parity"), H.depth_image(145, 131)
    with H.Env() as env, env.on_stream():
        mesh = H._mesh(env, "parity")
        depth, rays = env.cuda(d), env.cuda(f.rays6)
        t = torch.empty(len(f.rays6), dtype=torch.float32, device=env.dev)
        ids = torch.empty(len(f.rays6), dtype=torch.int32, device=env.dev)
        uv = torch.empty((len(f.rays6), 2), dtype=torch.float32, device=env.dev)
        env.stream.synchronize()                        # the inputs are there; from here on nothing waits
        eroded = depth_filters.erode_depth(depth, 2, ctx=env.ctx)                                    # enqueued
        mesh.cast_rays_device(rays.data_ptr(), len(f.rays6), t.data_ptr(), ids.data_ptr(), uv.data_ptr())   # enqueued
        proj = H.outputs(H.call(by_name()["project_jet_post@parity"], env))                          # host mode, at once
        cloud = H.outputs(H.call(by_name()["cloud_create@2049"], env))
        got = {"erode_device@145x131": {"depth": H._host(eroded)},
               "rays_device@parity": {"t_hit": H._host(t), "primitive_ids": H._host(ids).view(np.uint32), "primitive_uvs": H._host(uv)},
               "project_jet_post@parity": proj, "cloud_create@2049": cloud}
    for n in names:
        diff = H.same_bytes(got[n], want[n])
        assert diff is None, f"{n}: {diff}"


# ---------------------------------------------------------------- g. two contexts in turn

def test_g_one_history_dealt_to_two_contexts():
    want = yardstick(ops())
    with H.Env() as one, H.Env() as two:
        assert one.key != two.key
        H.replay(H.histories(ops(), 21), [one, two], want, seed="21, dealt in turn to two contexts", check_only=CHECK_ONLY)


# ---------------------------------------------------------------- h. a pending registration

# The entries refused while a registration is pending on their context (PedpError, "pending"), as include/pedp.h
# states it: the registration family, and the host-memory forms of closest points, face normals and the defect map.
# cloud_create reads its clouds back through pedp_nn, which is what refuses it.  Every other entry runs and gives the
# fresh bytes.  A change of this set is a change of policy.
REFUSED_WHILE_PENDING = {
    "nn@blob", "nn@parity", "icp@blob", "icp@parity", "icp_point@blob", "icp_point@parity", "icp_begin_end@blob",
    "icp_begin_end@parity", "icp_batched@blob", "icp_batched@parity", "icp_batched_ex@blob", "icp_batched_ex@parity",
    "ransac_hypotheses@blob", "ransac_hypotheses@parity", "cloud_create@257", "cloud_create@2049",
    "closest@1000", "closest@16385", "face_normals@1000", "face_normals@16385",
    "defect_add_faces@65", "defect_add_faces@4097", "defect_regions@0.01", "defect_regions@0.3",
}


def test_h_the_refused_set_names_catalogue_entries():
    assert REFUSED_WHILE_PENDING <= set(_names())


@pytest.mark.parametrize("name", _names())
def test_h_with_a_registration_pending(name):
    from pedp_hip import _lib

    op = by_name()[name]
    want_op, want_icp = fresh(op), fresh(by_name()["icp@parity"])
    src, tgt, nrm, r, init = H.reg_case("parity")
    with H.Env() as env:
        s, t = _lib.Cloud(env.ctx, src), _lib.Cloud(env.ctx, tgt, nrm)
        _lib.icp_begin(env.ctx, s, t, r, init, max_iteration=12, relative_fitness=-1, relative_rmse=-1, want_trace=True)
        refused, got = None, None
        try:
            try:
                got = H.call(op, env)               # (a device-memory call: enqueued behind the registration, fetched after its end)
            except _lib.PedpError as e:
                refused = str(e)
        finally:
            res = H._icp_out(_lib.icp_end(env.ctx, want_corr=True))
        diff = H.same_bytes(res, want_icp)
        assert diff is None, f"the pending registration's result after {name}: {diff}"
        if refused is not None:
            assert "pending" in refused, refused
        else:
            diff = H.same_bytes(H.outputs(got), want_op)
            assert diff is None, f"{name} with a registration pending: {diff}"
        assert (refused is not None) == (name in REFUSED_WHILE_PENDING), refused or "the call ran"
        if refused is not None:                # refused leaves nothing behind: afterwards the call is the fresh one
            diff = H.same_bytes(H.outputs(H.call(op, env)), want_op)
            assert diff is None, f"{name} after its refusal and the registration's end: {diff}"
        s.close()
        t.close()
