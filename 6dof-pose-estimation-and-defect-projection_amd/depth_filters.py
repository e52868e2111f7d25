"""Host mirror of the reference's depth pre-filters (Utils.py): same names, arguments and return
types; the pixels are processed by libpedp_hip.so instead of warp-lang's CUDA JIT.

    erode_depth             Utils.py:386-396  (kernel :356-383; callers estimater.py:171, :255)
    bilateral_filter_depth  Utils.py:347-357  (kernel :304-345; callers estimater.py:172, :256)
    depth2xyzmap            Utils.py:401-420  (callers run.py:89, estimater.py:175, :212)
    depth2xyzmap_batch      Utils.py:423-442  (caller estimater.py:259)

numpy in -> numpy out; a torch tensor on the GPU in -> a torch tensor on the same device out,
processed in place on the device through its data_ptr() (no host round trip).  `device` is
accepted for signature compatibility; the context's GPU is used.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import device_of, empty, is_torch, launch, ptr, wait_for_torch


def _run(fn_name, depth, out_shape_tail, call, ctx=None):
    """Dispatch one image-shaped call on host (numpy) or device (torch) memory."""
    if is_torch(depth) and not depth.is_cuda:
        import torch

        return torch.from_numpy(_run(fn_name, depth.numpy(), out_shape_tail, call, ctx))
    dev = device_of(depth)
    if dev is not None:
        import torch

        d = depth.contiguous().to(torch.float32)
    else:
        d = np.ascontiguousarray(depth, dtype=np.float32)
    out = empty(dev, tuple(d.shape) + out_shape_tail)
    launch(dev, fn_name, lambda lib, h, mem: call(lib, h, ptr(d), mem, ptr(out), d.shape), ctx)
    return out


def _hw(shape):
    if len(shape) != 2:
        raise _lib.PedpError(f"expected an H x W depth image, got shape {tuple(shape)}")
    return int(shape[0]), int(shape[1])


def erode_depth(depth, radius=2, depth_diff_thres=0.001, ratio_thres=0.8, zfar=100, device="cuda", ctx=None):
    def call(lib, h, src, mem, dst, shape):
        H, W = _hw(shape)
        return lib.pedp_erode_depth(h, src, H, W, int(radius), float(depth_diff_thres), float(ratio_thres), float(zfar),
                                    mem, dst)
    return _run("pedp_erode_depth", depth, (), call, ctx)


def bilateral_filter_depth(depth, radius=2, zfar=100, sigmaD=2, sigmaR=100000, device="cuda", ctx=None):
    def call(lib, h, src, mem, dst, shape):
        H, W = _hw(shape)
        return lib.pedp_bilateral_filter_depth(h, src, H, W, int(radius), float(zfar), float(sigmaD), float(sigmaR),
                                               mem, dst)
    return _run("pedp_bilateral_filter_depth", depth, (), call, ctx)


def depth2xyzmap(depth, K, uvs=None, ctx=None):
    if uvs is not None:
        # Utils.py:406-409: only the listed pixels (u, v rounded) are back-projected, the rest of the
        # map stays zero.  A listed pixel's value is the full map's, so the full map comes from the
        # device and the listed pixels are picked out of it.
        full = depth2xyzmap(depth, K, None, ctx)
        on_device = is_torch(full)
        arr = full.detach().cpu().numpy() if on_device else np.asarray(full)
        uv = np.asarray(uvs.detach().cpu().numpy() if is_torch(uvs) else uvs).round().astype(int)
        out = np.zeros_like(arr)
        out[uv[:, 1], uv[:, 0]] = arr[uv[:, 1], uv[:, 0]]
        if on_device:
            import torch

            return torch.from_numpy(out).to(full.device)
        return out
    Kd = np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if is_torch(K) else K), dtype=np.float64).reshape(3, 3)

    def call(lib, h, src, mem, dst, shape):
        H, W = _hw(shape)
        return lib.pedp_depth2xyzmap(h, src, H, W, _lib._ptr(Kd), mem, dst)
    return _run("pedp_depth2xyzmap", depth, (3,), call, ctx)


def depth2xyzmap_batch(depths, Ks, zfar, ctx=None):
    Kf = np.ascontiguousarray(np.asarray(Ks.detach().cpu().numpy() if is_torch(Ks) else Ks), dtype=np.float32)

    def call(lib, h, src, mem, dst, shape):
        if len(shape) != 3:
            raise _lib.PedpError(f"expected B x H x W depths, got shape {tuple(shape)}")
        B, H, W = (int(v) for v in shape)
        if Kf.size != 9 * B:
            raise _lib.PedpError("Ks must hold one 3 x 3 matrix per image")
        return lib.pedp_depth2xyzmap_batch(h, src, B, H, W, _lib._ptr(Kf), float(zfar), mem, dst)
    return _run("pedp_depth2xyzmap_batch", depths, (3,), call, ctx)


def depth_to_scene(depth, K, erode_radius=2, bilateral_radius=2, depth_diff_thres=0.001, ratio_thres=0.8, erode_zfar=100,
                   bilateral_zfar=100, sigmaD=2, sigmaR=100000, xyz_zfar=np.inf, z_min=0.001, scale=1000.0, buffers=None, ctx=None):
    """A frame's depth entry in ONE library call (pedp_depth_to_scene): erode_depth -> bilateral_filter_depth ->
    depth2xyzmap_batch -> the points with z >= z_min as float64, scaled (estimater.py:255-259 and the scene cloud of run.py's
    loop; what `xyz[xyz[..., 2] >= z_min].double() * scale` gives after the three calls, bit for bit).  depth: H x W float32
    metres, a numpy array (uploaded by the library through its pinned staging) or a CUDA tensor.  Returns torch CUDA tensors
    (filtered depth H x W, xyz map H x W x 3, points n x 3 float64); `buffers` (a dict, optional) keeps them across frames."""
    import torch

    ctx = ctx or _lib.default_context()
    dev = torch.device(f"cuda:{ctx.device}")
    if is_torch(depth):
        d_in = depth.to(dev, torch.float32).contiguous()
        wait_for_torch(d_in)
        H, W = _hw(d_in.shape)
        src, mem, keep = C.c_void_p(d_in.data_ptr()), _lib.DEVICE, d_in
    else:
        d_in = np.ascontiguousarray(depth, dtype=np.float32)
        H, W = _hw(d_in.shape)
        src, mem, keep = _lib._ptr(d_in), _lib.HOST, d_in
    buffers = {} if buffers is None else buffers
    if buffers.get("shape") != (H, W):
        buffers["shape"] = (H, W)
        buffers["depth"] = torch.empty((H, W), dtype=torch.float32, device=dev)
        buffers["xyz"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        buffers["points"] = [torch.empty((H * W, 3), dtype=torch.float64, device=dev) for _ in range(2)]
        buffers["turn"] = 0
        wait_for_torch(buffers["depth"])
    buffers["turn"] ^= 1                                          # two point buffers in turn: a frame's cloud outlives the next call
    pts = buffers["points"][buffers["turn"]]
    Kf = np.asarray(K.detach().cpu().numpy() if is_torch(K) else K, dtype=np.float32).reshape(9)
    prm = _lib.DepthEntryParams(int(erode_radius), float(depth_diff_thres), float(ratio_thres), float(erode_zfar), int(bilateral_radius),
                                float(bilateral_zfar), float(sigmaD), float(sigmaR), (C.c_float * 9)(*Kf.tolist()), float(xyz_zfar),
                                float(z_min), float(scale))
    n = C.c_int64()
    _lib.check(_lib.load().pedp_depth_to_scene(ctx._h, src, H, W, mem, C.byref(prm), C.c_void_p(buffers["depth"].data_ptr()),
                                               C.c_void_p(buffers["xyz"].data_ptr()), C.c_void_p(pts.data_ptr()), C.byref(n)),
               "pedp_depth_to_scene")
    del keep
    return buffers["depth"], buffers["xyz"], pts[: n.value]
