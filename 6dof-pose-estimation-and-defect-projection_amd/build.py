"""Build libpedp_hip.so (gfx950) in-tree with hipcc.

    python "6dof-pose-estimation-and-defect-projection_amd/build.py" [--force]

The library has no torch / Python dependency: plain HIP + a C ABI (include/pedp.h).
Flags that matter for parity with the oracle:
  -ffp-contract=off   an FMA only where the source says __fmaf_rn / fma
  no -ffast-math      IEEE division, no reassociation
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libpedp_hip.so")
# source -> extra flags.  pedp_icp.hip: MFMA results stay in VGPRs (no v_accvgpr_read
# copies) and min/med3 on them need no sNaN-quieting v_max (its inputs are never NaN:
# finite coordinates, +inf only as the running-min seed).  pedp_ray.hip keeps strict
# IEEE semantics everywhere (its one extra flag only picks the register file of MFMA results).
SOURCES = {
    "pedp_ctx.hip": [],
    "pedp_ray.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],   # (MFMA results in VGPRs: no v_accvgpr_read copies in the matrix sweep)
    "pedp_icp.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "pedp_project.hip": [],
    "pedp_depth.hip": [],
    "pedp_cloudops.hip": [],
    "pedp_comm.hip": [],
    "pedp_render.hip": [],
    "pedp_crop.hip": [],
    "pedp_pose.hip": [],
    "pedp_estimator.hip": [],
    "pedp_metrics.hip": [],
    "pedp_closest.hip": [],
    "pedp_defectmap.hip": [],
    "pedp_coverage.hip": [],
    "pedp_viewplan.hip": [],
    "pedp_deviationmap.hip": [],
    "pedp_solid.hip": [],
    "pedp_refine.hip": [],
    "pedp_sample.hip": [],
    "pedp_surface_fit.hip": [],
    "pedp_conv.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
    "pedp_attn.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
    "pedp_linear.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
    "pedp_cluster.cpp": [],
}
HEADERS = ["pedp_internal.h", os.path.join("..", "..", "include", "pedp.h")]
ARCH = "gfx950"
COMMON = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
          "-fno-math-errno", "-Wall", "-Wno-unused-function"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"


def up_to_date(out):
    if not os.path.exists(out):
        return False
    t = os.path.getmtime(out)
    deps = [os.path.join(CSRC, s) for s in list(SOURCES) + HEADERS] + [os.path.abspath(__file__)]
    # every header under csrc/ (pedp_icp.hip's kernels live in csrc/icp/*.h)
    deps += [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs if f.endswith(".h")]
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force=False, verbose=True, extra_flags=(), out=OUT):
    """Compile every source to an object (in parallel) and link the shared library."""
    if not force and up_to_date(out):
        return out
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for src, flags in SOURCES.items():
        obj = os.path.join(objdir, os.path.basename(out) + "." + src + ".o")
        cmd = [hipcc(), *COMMON, *flags, *extra_flags, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[pedp build]", " ".join(cmd), flush=True)
        procs.append((cmd, obj, subprocess.Popen(cmd)))
    objs = []
    for cmd, obj, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
        objs.append(obj)
    link = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-ldl", "-o", out]
    if verbose:
        print("[pedp build]", " ".join(link), flush=True)
    subprocess.run(link, check=True)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
