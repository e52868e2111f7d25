"""Per-launch durations of a single registration's kernels from a rocprofv3 --kernel-trace CSV of bench.py:
    python tools/icp_launch_stats.py <kernel_trace.csv> <side> [registrations]
A registration begins with icp_state_start_kernel; launch k is its k-th pass launch (generic pass kernel or the steady
launch).  Prints `side,launch,kernel,launches,median_us,min_us,max_us` over the last `registrations` (default 20) ones, and
the sum of a registration's launches in the row `all`."""
import csv, re, sys
import numpy as np

rows = list(csv.DictReader(open(sys.argv[1])))
side = sys.argv[2]
last = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ks = []
for r in rows:
    name = re.sub(r"^void |\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0].split("<")[0]
    if name in ("icp_state_start_kernel", "icp_pass_kernel", "icp_steady_kernel"):
        ks.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
ks.sort()
regs = []
for _, name, us in ks:
    if name == "icp_state_start_kernel":
        regs.append([])
    elif regs:
        regs[-1].append((name, us))
shape = [n for n, _ in regs[-1]]
regs = [r for r in regs if [n for n, _ in r] == shape][-last:]  # (registrations of the same launch sequence as the last one)
print("side,launch,kernel,launches,median_us,min_us,max_us")
for k, name in enumerate(shape):
    v = np.array([r[k][1] for r in regs])
    print(f"{side},{k},{name},{len(v)},{np.median(v):.2f},{v.min():.2f},{v.max():.2f}")
v = np.array([sum(us for _, us in r) for r in regs])
print(f"{side},all,sum,{len(v)},{np.median(v):.2f},{v.min():.2f},{v.max():.2f}")
