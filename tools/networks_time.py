"""Times of the refine and score networks on cuda:0 -> profiles/networks_time.json (or the path given).

    layers      per block-convolution shape of a 252-pair forward at 160 x 160 (128 channels at 40 x 40 for 504 images, 256
                at 40 x 40 for 252, 512 at 20 x 20 for 252): conv.conv3x3 against F.conv2d on the same channels-last float16
                tensors (convolution and bias alone), and the whole fused step (norm folded, identity add, ReLU) against
                torch's conv + BatchNorm + add + ReLU; the two taking turns in one loop after a warm-up, HIP events on a
                side stream.  networks._AUTO is read off the first pair.
    heads       the heads' attention at (B, S) = (252, 400) and (1, 252), 4 heads of 128, on gaussian float16 data:
                attention.mha_core on the packed in-projection output against F.scaled_dot_product_attention on its
                B x H x S x D views, and attention.self_attention against nn.MultiheadAttention as the scorer calls it
                (need_weights=True) and with need_weights=False, under float16 autocast; then one refiner and one scorer
                forward at 252 pairs per `heads` value (backend 'torch').  The variants take turns in one loop; median
                and minimum are reported besides the mean.
    forward     one refiner forward and one scorer forward at 252 pairs of 160 x 160 under float16 autocast, backend
                'torch' against 'hip' (and 'auto'), taking turns in one loop after a warm-up
    first       the first forward's wall time in a fresh process, per backend (torch's convolution library chooses its
                kernels then; the packed weights are built then)
    strided     the three stride-2 layers of a 252-pair forward (the 7x7 stem on 2 x 252 float32 crops of 6 x 160 x 160, 3x3
                64 -> 128 on 504 x 80 x 80, 3x3 256 -> 512 on 252 x 40 x 40): conv.conv_stem / conv.conv_strided against
                F.conv2d on channels-last float16 tensors (convolution and bias alone; for the stem also torch's whole
                entry: cat, autocast's cast and the convolution from the float32 crops), then one refiner and one scorer
                forward at 252 pairs with strided 'torch' against 'hip' (backend 'hip'), taking turns in one loop
    strided_first   the first forward's wall time in a fresh process per `strided` value (backend 'hip'): with 'hip' no
                convolution of the encoders goes to torch's convolution library, whose search for kernels the first
                forward otherwise pays
    linears     the heads' linear layers at M = 100,800 (252 x 400 tokens) and M = 252, K = 512, on gaussian float16 data:
                linear.linear per epilogue (N = 1536 plain and with the position table, N = 512 plain and with ReLU) and
                linear.linear_add_norm against the torch ops they replace as autocast runs them (F.linear on float16; the
                table's add, the residual add and F.layer_norm in float32, cast back to float16), linear.token_pool against
                Linear + mean; then one refiner and one scorer forward at 252 pairs with linears 'torch' against 'hip'
                (backend 'hip', strided 'hip', heads 'hip'), taking turns in one loop
    estimator   register (252 hypotheses, 5 iterations) and track_one (2 iterations) at 576 x 640 around the real
                architectures, as tools/estimator_time.py times them around its stand-ins

Every step is a child process under its own time limit; the first one that fails ends the run.  `--only a,b` runs the
named steps alone and keeps the other steps' results of an existing file.  Weights are the modules'
random initial values (use_BN on): times do not depend on them.  Kernel times per forward come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/networks_time.py --step traced
    python tools/networks_time.py --summarize TRACE profiles/networks_kernel_stats.csv"""
import collections
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS, CROP = 252, 160
SHAPES = [(2 * PAIRS, 40, 40, 128), (PAIRS, 40, 40, 256), (PAIRS, 20, 20, 512)]
PEAK_F16_TFLOPS = 2500.0   # dense float16 MFMA peak of the MI355X
STEPS = [("layers", 300), ("heads", 300), ("linears", 420), ("forward", 420), ("first torch", 300), ("first hip", 300), ("strided", 420),
         ("strided_first torch", 300), ("strided_first hip", 300), ("estimator", 420)]
CFG = {"use_BN": True, "c_in": 6, "rot_rep": "axis_angle", "input_resize": (CROP, CROP), "trans_normalizer": [0.02, 0.02, 0.05],
       "rot_normalizer": 0.35}


def _stats(ms):
    import numpy as np

    return {"mean_ms": float(np.mean(ms)), "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
            "max_ms": float(np.max(ms)), "reps": len(ms)}


def _event_ms(fns, reps, warm=3):
    """Milliseconds of each function by HIP events on a side stream, the functions taking turns within one loop."""
    import torch

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    with torch.cuda.stream(s):
        for _ in range(warm):
            for f in fns:
                f()
        for _ in range(reps):
            for k, f in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                t[k].append(a.elapsed_time(b))
    s.synchronize()
    return [_stats(x) for x in t]


def layers():
    import torch
    import torch.nn.functional as F
    from pedp_hip.conv import conv3x3, pack_conv3x3

    out = {}
    for n, h, w, c in SHAPES:
        conv = torch.nn.Conv2d(c, c, 3, 1, 1).cuda()
        bn = torch.nn.BatchNorm2d(c).cuda().eval()
        with torch.no_grad():
            bn.running_var.uniform_(1.0, 1.25)
            bn.running_mean.normal_(0, 0.1)
        plain, folded = pack_conv3x3(conv), pack_conv3x3(conv, bn)
        x = torch.randn((n, h, w, c), device="cuda").half()
        res = torch.randn((n, h, w, c), device="cuda").half()
        y = torch.empty_like(x)
        xv, rv = x.permute(0, 3, 1, 2), res.permute(0, 3, 1, 2)          # the same memory as NCHW channels-last views
        w16 = conv.weight.detach().half().contiguous(memory_format=torch.channels_last)
        b16 = conv.bias.detach().half()
        bnh = torch.nn.BatchNorm2d(c).cuda().eval().half()

        def torch_step():
            return torch.relu_(bnh(F.conv2d(xv, w16, b16, 1, 1)).add_(rv))

        with torch.inference_mode():
            k_conv, t_conv, k_step, t_step = _event_ms(
                [lambda: conv3x3(x, plain, relu=False, out=y), lambda: F.conv2d(xv, w16, b16, 1, 1),
                 lambda: conv3x3(x, folded, residual=res, relu=True, out=y), torch_step], 20)
        flop = 2.0 * n * h * w * c * 9 * c
        tf = flop / (k_conv["mean_ms"] * 1e-3) / 1e12
        out[f"{c}ch_{h}x{w}_x{n}"] = {
            "gflop": flop / 1e9, "kernel_conv": k_conv, "torch_conv": t_conv, "kernel_fused_step": k_step,
            "torch_conv_bn_add_relu": t_step, "kernel_tflops": tf, "kernel_fraction_of_f16_peak": tf / PEAK_F16_TFLOPS,
            "torch_tflops": flop / (t_conv["mean_ms"] * 1e-3) / 1e12,
            "kernel_not_slower": bool(k_conv["mean_ms"] <= t_conv["mean_ms"])}
    return out


def heads():
    import torch
    import torch.nn.functional as F
    from pedp_hip.attention import mha_core, self_attention

    H, D = 4, 128
    E = H * D
    out = {"core": {}, "module": {}}
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, S in ((PAIRS, 400), (1, PAIRS)):
        qkv = torch.randn((B, S, 3 * E), device="cuda", generator=g).half()
        q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, S, H, D).transpose(1, 2) for i in range(3))
        o = torch.empty((B, S, E), dtype=torch.float16, device="cuda")
        mha = torch.nn.MultiheadAttention(E, H, bias=True, batch_first=True).cuda().eval()
        x = torch.randn((B, S, E), device="cuda", generator=g)
        with torch.inference_mode(), torch.autocast("cuda"):
            k_core, t_core = _event_ms([lambda: mha_core(qkv, H, out=o), lambda: F.scaled_dot_product_attention(q, k, v)], 30)
            k_mod, t_weights, t_plain = _event_ms([lambda: self_attention(mha, x), lambda: mha(x, x, x)[0],
                                                   lambda: mha(x, x, x, need_weights=False)[0]], 30)
        flop = 4.0 * B * H * S * S * D
        tf = flop / (k_core["median_ms"] * 1e-3) / 1e12
        out["core"][f"{B}x{S}"] = {"gflop": flop / 1e9, "mha_core": k_core, "torch_sdpa": t_core, "kernel_tflops": tf,
                                   "kernel_fraction_of_f16_peak": tf / PEAK_F16_TFLOPS,
                                   "kernel_over_sdpa": k_core["median_ms"] / t_core["median_ms"]}
        out["module"][f"{B}x{S}"] = {"self_attention": k_mod, "torch_need_weights": t_weights, "torch_no_weights": t_plain,
                                     "kernel_over_need_weights": k_mod["median_ms"] / t_weights["median_ms"]}
    A, Bi = _inputs()
    rn, sn = _nets("torch")
    refine, score = _forward_fns(rn, sn, A, Bi)

    def with_heads(net, value, fn):
        def run():
            net.set_heads(value)
            return fn()
        return run

    out["forward"] = {}
    for name, net, fn in (("refiner", rn, refine), ("scorer", sn, score)):
        t, h = _event_ms([with_heads(net, v, fn) for v in ("torch", "hip")], 10, warm=2)
        out["forward"][name] = {"torch": t, "hip": h, "hip_over_torch": h["median_ms"] / t["median_ms"]}
    return out


def _nets(backend, strided="torch", heads="torch"):
    from pedp_hip import networks

    return (networks.RefineNet(CFG, backend=backend, strided=strided, heads=heads).cuda().eval(),
            networks.ScoreNetMultiPair(CFG, backend=backend, strided=strided, heads=heads).cuda().eval())


def linears():
    import torch
    import torch.nn.functional as F
    from pedp_hip import linear as L
    from pedp_hip.networks import _PositionTable

    E, S = 512, 400
    out = {"kernel": {}, "forward": {}}
    g = torch.Generator(device="cuda").manual_seed(0)
    pe = _PositionTable(E, S).cuda().pe[0]
    for M in (PAIRS * S, PAIRS):
        x = torch.randn((M, E), device="cuda", generator=g).half()
        res = torch.randn((M, E), device="cuda", generator=g).half()
        res32 = res.float()
        lin3, lin1, norm = torch.nn.Linear(E, 3 * E).cuda(), torch.nn.Linear(E, E).cuda(), torch.nn.LayerNorm(E).cuda()
        p3, p1 = L.pack_linear(lin3), L.pack_linear(lin1)
        w3, b3, w1, b1 = (t.detach().half() for t in (lin3.weight, lin3.bias, lin1.weight, lin1.bias))
        y3 = torch.empty((M, 3 * E), dtype=torch.float16, device="cuda")
        y1 = torch.empty((M, E), dtype=torch.float16, device="cuda")
        pairs = {
            "plain_n1536": (lambda: L.linear(x, p3, out=y3), lambda: F.linear(x, w3, b3), 3 * E),
            "plain_n512": (lambda: L.linear(x, p1, out=y1), lambda: F.linear(x, w1, b1), E),
            "relu_n512": (lambda: L.linear(x, p1, relu=True, out=y1), lambda: torch.relu(F.linear(x, w1, b1)), E),
            "add_ln_n512": (lambda: L.linear_add_norm(x, p1, res, norm, out=y1),
                            lambda: F.layer_norm(res32 + F.linear(x, w1, b1), (E,), norm.weight, norm.bias, norm.eps).half(), E)}
        if M % S == 0:
            x3 = x.view(-1, S, E)
            pairs["plain_pos_n1536"] = (lambda: L.linear(x, p3, pos=pe, period=S, out=y3),
                                        lambda: F.linear((x3 + pe).half(), w3, b3), 3 * E)
            small = torch.nn.Linear(E, 3).cuda()
            ps, ws, bs = L.pack_f32(small), small.weight.detach().half(), small.bias.detach().half()
            pairs["token_pool_n3"] = (lambda: L.token_pool(x, M // S, ps), lambda: F.linear(x3, ws, bs).mean(dim=1), 0)
        out["kernel"][f"M{M}"] = {}
        for name, (kernel, stock, n) in pairs.items():
            with torch.inference_mode():
                k, t = _event_ms([kernel, stock], 20)
            row = {"kernel": k, "torch": t, "kernel_over_torch": k["median_ms"] / t["median_ms"]}
            if n:
                flop = 2.0 * M * n * E
                row.update(gflop=flop / 1e9, kernel_tflops=flop / (k["median_ms"] * 1e-3) / 1e12,
                           torch_tflops=flop / (t["median_ms"] * 1e-3) / 1e12)
                row["kernel_fraction_of_f16_peak"] = row["kernel_tflops"] / PEAK_F16_TFLOPS
            out["kernel"][f"M{M}"][name] = row
        del x, res, res32, y3, y1
    A, B = _inputs()
    rn, sn = _nets("hip", "hip", "hip")
    refine, score = _forward_fns(rn, sn, A, B)

    def with_linears(net, value, fn):
        def run():
            net.set_linears(value)
            return fn()
        return run

    for name, net, fn in (("refiner", rn, refine), ("scorer", sn, score)):
        t, h = _event_ms([with_linears(net, v, fn) for v in ("torch", "hip")], 10, warm=2)
        out["forward"][name] = {"torch": t, "hip": h, "hip_over_torch": h["median_ms"] / t["median_ms"]}
    return out


def strided():
    import torch
    import torch.nn.functional as F
    from pedp_hip.conv import conv_stem, conv_strided, pack_conv

    out = {"layers": {}, "forward": {}}
    A, B = _inputs()
    for name, (n, h, w, cin, cout, k) in (("stem_7x7_6to64_160x160_x504", (2 * PAIRS, CROP, CROP, 6, 64, 7)),
                                          ("3x3_64to128_80x80_x504", (2 * PAIRS, 80, 80, 64, 128, 3)),
                                          ("3x3_256to512_40x40_x252", (PAIRS, 40, 40, 256, 512, 3))):
        conv = torch.nn.Conv2d(cin, cout, k, 2, (k - 1) // 2).cuda()
        packed = pack_conv(conv)
        w16 = conv.weight.detach().half().contiguous(memory_format=torch.channels_last)
        b16 = conv.bias.detach().half()
        y = torch.empty((n, h // 2, w // 2, cout), dtype=torch.float16, device="cuda")
        if k == 7:
            x16 = torch.cat([A, B], 0).half().contiguous(memory_format=torch.channels_last)

            def entry():
                with torch.autocast("cuda"):
                    return conv(torch.cat([A, B], 0))

            fns = [lambda: conv_stem(A, B, packed, relu=False, out=y), lambda: F.conv2d(x16, w16, b16, 2, 3), entry]
        else:
            x = torch.randn((n, h, w, cin), device="cuda").half()
            xv = x.permute(0, 3, 1, 2)                                   # the same memory as an NCHW channels-last view
            fns = [lambda: conv_strided(x, packed, relu=False, out=y), lambda: F.conv2d(xv, w16, b16, 2, 1)]
        with torch.inference_mode():
            t = _event_ms(fns, 20)
        flop = 2.0 * n * (h // 2) * (w // 2) * cout * k * k * cin
        tf = flop / (t[0]["median_ms"] * 1e-3) / 1e12
        out["layers"][name] = {"gflop": flop / 1e9, "kernel": t[0], "torch_conv": t[1], "kernel_tflops": tf,
                               "kernel_fraction_of_f16_peak": tf / PEAK_F16_TFLOPS,
                               "kernel_over_torch": t[0]["median_ms"] / t[1]["median_ms"]}
        if k == 7:
            out["layers"][name]["torch_cat_cast_conv"] = t[2]
            del x16
    rn, sn = _nets("hip")
    refine, score = _forward_fns(rn, sn, A, B)

    def with_strided(net, value, fn):
        def run():
            net.set_strided(value)
            return fn()
        return run

    for name, net, fn in (("refiner", rn, refine), ("scorer", sn, score)):
        t, h = _event_ms([with_strided(net, v, fn) for v in ("torch", "hip")], 10, warm=2)
        out["forward"][name] = {"torch": t, "hip": h, "hip_over_torch": h["median_ms"] / t["median_ms"]}
    return out


def _forward_fns(rn, sn, A, B):
    import torch

    def refine():
        with torch.inference_mode(), torch.autocast("cuda"):
            return rn(A, B)["trans"]

    def score():
        with torch.inference_mode(), torch.autocast("cuda"):
            return sn(A, B, L=len(A))["score_logit"]

    return refine, score


def _inputs():
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    return (torch.randn((PAIRS, 6, CROP, CROP), device="cuda", generator=g),
            torch.randn((PAIRS, 6, CROP, CROP), device="cuda", generator=g))


def forward():
    A, B = _inputs()
    rn, sn = _nets("torch")
    refine, score = _forward_fns(rn, sn, A, B)

    def with_backend(net, backend, fn):
        def run():
            net.set_backend(backend)
            return fn()
        return run

    out = {}
    for name, net, fn in (("refiner", rn, refine), ("scorer", sn, score)):
        t, h, a = _event_ms([with_backend(net, b, fn) for b in ("torch", "hip", "auto")], 10, warm=2)
        out[name] = {"torch": t, "hip": h, "auto": a, "hip_over_torch": h["mean_ms"] / t["mean_ms"]}
    return out


def first(backend, strided="torch"):
    import torch

    A, B = _inputs()
    rn, sn = _nets(backend, strided)
    out = {}
    for name, fn in zip(("refiner", "scorer"), _forward_fns(rn, sn, A, B)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out[name] = {"first_forward_ms": (t1 - t0) * 1e3, "second_forward_ms": (time.perf_counter() - t1) * 1e3}
    return out


def _estimator(backend, H=576, W=640):
    import numpy as np
    import torch
    from pedp_hip import synth
    from pedp_hip.compat import TriangleMesh, make_mesh_tensors, nvdiffrast_render
    from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor

    v, t, n = synth.bumpy_torus(60, 40)
    v = v * 0.0008
    mesh = TriangleMesh(v, t)
    mesh.vertex_normals = np.asarray(n, np.float64)
    K = np.array([[W * 0.9, 0, W / 2 - 0.5], [0, W * 0.9, H / 2 - 0.5], [0, 0, 1]])
    rn, sn = _nets(backend)
    est = FoundationPose(v, mesh.vertex_normals, mesh=mesh, refiner=PoseRefinePredictor(rn, CFG), scorer=ScorePredictor(sn, CFG))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.rot_x(0.4)[:3, :3] @ synth.rot_z(0.3)[:3, :3]
    T[:3, 3] = [0.01, -0.01, 0.5]
    color, depth, _ = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(T[None], device="cuda"),
                                        mesh_tensors=make_mesh_tensors(mesh))
    rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
    d = depth[0].cpu().numpy()
    mask = d > 0
    rng = np.random.default_rng(0)
    d = (d + rng.normal(0, 0.002, d.shape).astype(np.float32) * mask + 1.2 * ~mask).astype(np.float32)
    return est, K, rgb, d, mask


def _wall_ms(f, reps, warm):
    import torch

    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return _stats(t)


def estimator():
    out = {}
    for backend in ("torch", "auto"):
        est, K, rgb, depth, mask = _estimator(backend)
        out[backend] = {
            "register_5_iterations": _wall_ms(lambda: est.register(K=K, rgb=rgb, depth=depth, ob_mask=mask, iteration=5), 3, 1),
            "track_one_2_iterations": _wall_ms(lambda: est.track_one(rgb=rgb, depth=depth, K=K, iteration=2), 10, 2)}
    return out


def traced():
    import torch

    A, B = _inputs()
    rn, sn = _nets("hip")
    refine, score = _forward_fns(rn, sn, A, B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            refine(), score()
        s.synchronize()
        torch.empty(1, dtype=torch.int16, device="cuda").fill_(1)      # marker: the trace is cut here
        s.synchronize()
        refine()
        s.synchronize()
        torch.empty(1, dtype=torch.int16, device="cuda").fill_(2)
        s.synchronize()
        score()
        s.synchronize()
        torch.empty(1, dtype=torch.int16, device="cuda").fill_(3)
        s.synchronize()


def summarize(trace_dir, out_csv):
    """Per phase of the traced run (one fused refiner forward, one fused scorer forward): every kernel's launches and time."""
    paths = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    kernels = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))
    is_marker = lambda r: "short" in r["Kernel_Name"] and "Fill" in r["Kernel_Name"]  # noqa: E731
    cuts = [int(r["Start_Timestamp"]) for r in kernels if is_marker(r)]
    phases = ["warm-up", "refiner forward (hip)", "scorer forward (hip)", "end"]
    if len(cuts) != 3:
        raise SystemExit(f"expected 3 marker launches, found {len(cuts)}")
    groups = collections.defaultdict(list)
    for r in kernels:
        if is_marker(r):
            continue
        name = re.sub(r"^void |\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0]
        groups[(phases[sum(int(r["Start_Timestamp"]) >= c for c in cuts)], name[:90])].append(
            int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["phase", "name", "calls", "total_ns", "mean_ns"])
        for p in phases[1:-1]:
            rows = [(k[1], d) for k, d in groups.items() if k[0] == p]
            for name, d in sorted(rows, key=lambda kv: -sum(kv[1])):
                w.writerow([p, name, len(d), sum(d), int(sum(d) / len(d))])
            w.writerow([p, "total", sum(len(d) for _, d in rows), sum(sum(d) for _, d in rows), ""])
    print(open(out_csv).read())


def main(out_path, only=None):
    """`only`: step names to run; an existing result file's other steps are kept."""
    res = {"pairs": PAIRS, "crop": CROP, "peak_f16_tflops": PEAK_F16_TFLOPS}
    if only and os.path.exists(out_path):
        res.update(json.load(open(out_path)))
    for step, limit in STEPS:
        if only and step not in only:
            continue
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", *step.split()], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step!r} ran past {limit} s: stopping", flush=True)
            res[step] = {"error": f"time limit of {limit} s"}
            break
        if p.returncode != 0:
            print(f"step {step!r} failed with exit status {p.returncode}: stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            res[step] = {"error": f"exit status {p.returncode}"}
            break
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"step {step!r}: {time.perf_counter() - t0:.1f} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if all("error" not in v for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    elif len(sys.argv) > 2 and sys.argv[1] == "--step":
        if sys.argv[2] == "traced":
            traced()
        else:
            import torch

            res = {"layers": layers, "heads": heads, "linears": linears, "forward": forward, "estimator": estimator, "strided": strided,
                   "strided_first": lambda: first("hip", sys.argv[3])}.get(sys.argv[2], lambda: first(sys.argv[3]))()
            if sys.argv[2] in ("layers", "heads", "linears", "strided"):
                res["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(res))
    else:
        args = sys.argv[1:]
        only = None
        if "--only" in args:                                   # --only heads,layers
            i = args.index("--only")
            only, args = args[i + 1].split(","), args[:i] + args[i + 2:]
        sys.exit(main(args[0] if args else os.path.join(ROOT, "profiles", "networks_time.json"), only))
