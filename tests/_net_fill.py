"""The by-name fill of the network fixtures (tests/golden/g9_networks.npz), shared by its generator and the tests: no
weights are committed, every tensor is a function of its place in the fixture's key list.

For the i-th key, r = np.random.RandomState(i) and g = r.standard_normal(shape):

    num_batches_tracked                 0
    pos_embed.pe                        untouched
    running_var                         1 + 0.25 * r.random_sample(shape)   (drawn after g)
    tensors with ndim >= 2              g * sqrt(2 / numel of one output row)
    1-D keys ending in .weight          1 + 0.1 * g       (the norm layers)
    every other 1-D tensor              0.1 * g
"""
import numpy as np
import torch

CASES = {  # name -> (network, batch, (C, H, W), L, input seed)
    "refiner_3x32x32": ("refiner", 3, (6, 32, 32), None, 101),
    "refiner_2x48x32": ("refiner", 2, (6, 48, 32), None, 102),
    "scorer_4x32x32": ("scorer", 4, (6, 32, 32), 4, 103),
    "scorer_6x32x48": ("scorer", 6, (6, 32, 48), 3, 104),
}
ROT_REPS = ("axis_angle", "6d")


def fill_value(i, key, shape):
    """float64 array for the i-th key, or None where the tensor stays as built."""
    r = np.random.RandomState(i)
    g = r.standard_normal(tuple(shape))
    if key.endswith("num_batches_tracked"):
        return np.zeros(tuple(shape))
    if key == "pos_embed.pe":
        return None
    if key.endswith("running_var"):
        return 1 + 0.25 * r.random_sample(tuple(shape))
    if len(shape) >= 2:
        return g * np.sqrt(2.0 / max(int(np.prod(shape[1:])), 1))
    if key.endswith(".weight"):
        return 1 + 0.1 * g
    return 0.1 * g


def fill(module, keys=None):
    """Fill the module in place by the rule; `keys` is the fixture's list (default: the module's own order)."""
    sd = module.state_dict()
    keys = list(sd.keys()) if keys is None else [str(k) for k in keys]
    with torch.no_grad():
        for i, k in enumerate(keys):
            if k not in sd:
                continue
            v = fill_value(i, k, tuple(sd[k].shape))
            if v is not None:
                sd[k].copy_(torch.from_numpy(np.asarray(v)).to(sd[k].dtype))
    return module


def inputs(case, dtype=torch.float64):
    """(A, B) of a case: standard normals from RandomState(seed), A drawn first."""
    _, n, chw, _, seed = CASES[case]
    r = np.random.RandomState(seed)
    a = r.standard_normal((n, *chw))
    b = r.standard_normal((n, *chw))
    return torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype)
