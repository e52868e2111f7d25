"""The torch / numpy bridge of the wrappers over libpedp_hip.so: which side a call runs on, its arrays there, and the
launch ordered with torch's current stream.  torch is imported inside the functions only, so a numpy-only caller never
loads it."""
import ctypes as C

import numpy as np

from . import _lib


def is_torch(x):
    return type(x).__module__.startswith("torch")


def device_of(*xs):
    """The device of the first CUDA tensor among xs; None: the call uses host memory."""
    return next((x.device for x in xs if is_torch(x) and x.is_cuda), None)


def ptr(a):
    if a is None:
        return None
    try:
        return C.c_void_p(a.data_ptr())     # a tensor
    except AttributeError:
        return _lib._ptr(a)                 # a numpy array


# ---------------------------------------------------------------- dispatch

_stream_ctx = {}


def stream_context(device, stream_handle):
    """A context per (device, torch stream).  torch's default stream has handle 0, which the C
    ABI reads as "own stream": such a context is not ordered with torch and launch synchronises
    around the call instead."""
    key = (device, stream_handle)
    if key not in _stream_ctx:
        _stream_ctx[key] = _lib.Context(device, stream=stream_handle or None)
    return _stream_ctx[key]


def on_torch_stream(ctx, dev):
    """ctx runs on torch's current stream of `dev`: its launches are ordered with torch's work there and nothing waits."""
    import torch

    handle = torch.cuda.current_stream(dev).cuda_stream
    return ctx.stream_handle not in (None, 0) and ctx.stream_handle == handle


def launch(dev, fn_name, call, ctx=None):
    """call(lib, ctx_handle, mem) on the device's context ordered with torch's current stream, or on host memory.  `ctx`:
    the caller's context instead of the stream's (host memory: instead of the default one)."""
    lib = _lib.load()
    if dev is None:
        _lib.check(call(lib, (ctx or _lib.default_context())._h, _lib.HOST), fn_name)
        return
    import torch

    cur = torch.cuda.current_stream(dev)
    if ctx is None:
        ctx = stream_context(dev.index or 0, cur.cuda_stream)
    shared = on_torch_stream(ctx, dev)
    if not shared:
        cur.synchronize()  # the context runs on another stream: the inputs must be complete
    _lib.check(call(lib, ctx._h, _lib.DEVICE), fn_name)
    if not shared:
        ctx.synchronize()  # ... and the outputs before torch touches them


def wait_for_torch(t):
    """Wait for torch's current stream on t's device: the library reads t on its own stream."""
    import torch

    torch.cuda.current_stream(t.device).synchronize()


# ---------------------------------------------------------------- arrays on the call's side

def to_device(x, dev, dtype=np.float32, u8_ok=False):
    """x as a `dtype` (or, with u8_ok, uint8) tensor on `dev` without a host wait: device tensors stay where they are;
    host arrays go through page-locked memory and a copy ordered on the current stream (a pageable copy would make
    torch synchronise the stream)."""
    import torch

    want = getattr(torch, np.dtype(dtype).name)

    def cast(t):
        return t if t.dtype == want or (u8_ok and t.dtype == torch.uint8) else t.to(want)

    if is_torch(x) and x.is_cuda:
        return cast(x if x.device == dev else x.to(dev))
    t = x.detach() if is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))
    return cast(t).contiguous().pin_memory().to(dev, non_blocking=True)


def as_array(x, dev, dtype=np.float32, u8_ok=False):
    """x as a contiguous `dtype` array on the call's side (torch on `dev`, numpy on the host); float32 widens exactly."""
    if dev is not None:
        return to_device(x, dev, dtype, u8_ok).contiguous()
    if is_torch(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=x.dtype if u8_ok and getattr(x, "dtype", None) == np.uint8 else dtype)


def empty(dev, shape, dtype=np.float32):
    if dev is not None:
        import torch

        return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    return np.empty(shape, dtype)


def as_kind(a, like):
    """Host results come back as the kind of the caller's input (CPU tensor or numpy)."""
    if is_torch(a) or not is_torch(like):
        return a
    import torch

    return torch.from_numpy(a)


def check_out(name, out, shape, dtype, dev, what):
    """The library writes prod(shape) `dtype` values through out's pointer, on the inputs' side: anything else is
    refused.  `what` says in the caller's words what `out` must be."""
    where = f"on {dev}" if dev is not None else "in host memory"
    if is_torch(out):
        import torch

        ok = (out.dtype == getattr(torch, np.dtype(dtype).name) and out.is_contiguous() and tuple(out.shape) == shape
              and (out.device == dev if dev is not None else not out.is_cuda))
        kind = f"{out.dtype} tensor of shape {tuple(out.shape)} on {out.device}{'' if out.is_contiguous() else ', strided'}"
    else:
        a = out if isinstance(out, np.ndarray) else None
        ok = (dev is None and a is not None and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable
              and a.shape == shape)
        kind = (f"{type(out).__name__}" if a is None else
                f"{a.dtype} array of shape {a.shape}{'' if a.flags.c_contiguous else ', strided'}")
    if not ok:
        raise _lib.PedpError(f"{name}: out must be a {what} {where}, got a {kind}")
