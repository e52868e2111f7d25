"""Writes tests/golden/g9_networks.npz from the reference's own network definitions.

    python tests/golden/make_network_golden.py /path/to/FoundationPose

Runs only where the reference tree exists; no test calls it.  The class and function definitions are taken out of
learning/models/{network_modules,refine_network,score_network}.py with `ast`, so the files' imports (cv2, Utils) never
execute; the networks are built on the CPU in float64 with use_BN=True and c_in=6 (the refiner for both rot_reps) and
filled by tests/_net_fill.py.  The fixture holds names and numbers only: the ordered state_dict keys with shapes and
dtypes, and per case the float64 outputs, the first sample's pair-encoder output (`feat`), the reference's own
float32-minus-float64 difference (`e_ref32`) and the change when A and B are swapped (`d_swap`), and the input seed
(tests/_net_fill.py's CASES)."""
import ast
import math
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _net_fill  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def definitions(ref_root):
    ns = {"torch": torch, "nn": nn, "F": F, "math": math, "np": np, "partial": partial}
    for name in ("network_modules", "refine_network", "score_network"):
        path = os.path.join(ref_root, "learning", "models", name + ".py")
        tree = ast.parse(open(path).read(), path)
        tree.body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))]
        exec(compile(tree, path, "exec"), ns)
    return ns


def run(net, kind, A, B, L):
    with torch.no_grad():
        out = net(A, B) if kind == "refiner" else net(A, B, L=L)
    return {k: v.double().numpy() for k, v in out.items()}


def main(ref_root):
    ns = definitions(ref_root)
    out = {}
    for kind, variants in (("refiner", _net_fill.ROT_REPS), ("scorer", (None,))):
        for rot in variants:
            cfg = Cfg(use_BN=True, rot_rep=rot or "axis_angle")
            net = (ns["RefineNet"] if kind == "refiner" else ns["ScoreNetMultiPair"])(cfg=cfg, c_in=6).double().eval()
            sd = net.state_dict()
            tag = kind if rot is None else f"{kind}_{rot}"
            out[f"{tag}/keys"] = np.array(list(sd.keys()))
            out[f"{tag}/shapes"] = np.array([",".join(str(int(s)) for s in v.shape) for v in sd.values()])
            out[f"{tag}/dtypes"] = np.array([str(v.dtype).replace("float64", "float32") for v in net.float().state_dict().values()])
            net.double()
            _net_fill.fill(net)
            enc = net.encodeAB if kind == "refiner" else net.encoderAB
            feats = []
            hook = enc.register_forward_hook(lambda m, i, o: feats.append(o[0].detach().double().numpy().copy()))
            for case, (k, n, chw, L, seed) in _net_fill.CASES.items():
                if k != kind:
                    continue
                A, B = _net_fill.inputs(case)
                feats.clear()
                y64 = run(net, kind, A, B, L)
                feat = feats[0]
                ysw = run(net, kind, B, A, L)
                net.float()
                y32 = run(net, kind, A.float(), B.float(), L)
                net.double()
                _net_fill.fill(net)   # the float32 round trip rounded the weights: fill again
                for name, v in y64.items():
                    out[f"{case}/{tag}/{name}"] = v
                    out[f"{case}/{tag}/{name}/e_ref32"] = np.abs(y32[name] - v).max()
                    out[f"{case}/{tag}/{name}/d_swap"] = np.abs(ysw[name] - v).max()
                out[f"{case}/feat"] = feat    # the encoders do not depend on rot_rep: one copy per case
                out[f"{case}/seed"] = np.int64(seed)
            hook.remove()
    path = os.path.join(HERE, "g9_networks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        if k.endswith("e_ref32") or k.endswith("d_swap"):
            print(k, float(v))


if __name__ == "__main__":
    main(sys.argv[1])
