"""Host time per call of the lightest wrapper on the shared-stream path of _bridge.launch: linear.token_pool on one group of
one row, on a non-default torch stream, 10,000 calls back to back with one synchronise after them.
    python tools/bridge_overhead.py [TREE]      TREE: a checkout to measure instead of this one (e.g. the parent commit's)
-> one JSON line; `us_per_call` is the median of 9 such loops (profiles/bridge_overhead.json)."""
import json, os, statistics, sys, time
tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, tree)
import torch
from pedp_hip import linear

assert os.path.dirname(os.path.dirname(os.path.abspath(linear.__file__))) == tree, linear.__file__
CALLS, REPS = 10000, 9
x = torch.zeros((1, 512), dtype=torch.float16, device="cuda")
stream = torch.cuda.Stream()
reps = []
with torch.cuda.stream(stream):
    for _ in range(2000):
        linear.token_pool(x, 1)
    stream.synchronize()
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            linear.token_pool(x, 1)
        t1 = time.perf_counter()
        stream.synchronize()
        reps.append((t1 - t0) / CALLS * 1e6)
print(json.dumps({"tree": tree, "calls": CALLS, "us_per_call": statistics.median(reps), "reps_us": reps}))
