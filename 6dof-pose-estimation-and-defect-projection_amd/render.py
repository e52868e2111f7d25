"""Batched mesh renderer: a drop-in for the reference's nvdiffrast use (Utils.py:104-220, :752-804).

    nvdiffrast_render           Utils.py:133-220 (callers predict_pose_refine.py:49, predict_score.py:79)
    make_mesh_tensors           Utils.py:104-130
    projection_matrix_from_intrinsics, glcam_in_cvcam   Utils.py:752-804, :68-71
    dr.RasterizeCudaContext / dr.rasterize / dr.interpolate / dr.texture   (`import nvdiffrast.torch as dr`,
                                Utils.py:18; run.py:34, estimater.py:100, :166)

The pixels come from libpedp_hip.so (csrc/pedp_render.hip).  nvdiffrast_render is one fused call: the colour, depth,
normal and xyz maps are written in their final (flipped) row order, with no intermediate N x H x W x 4 buffer.  The dr
shim is forward only and instanced only: ranges, gradients, mipmaps and other filter or boundary modes raise
NotImplementedError.

A torch CUDA tensor in gives torch tensors on the same device out, enqueued on the caller's current stream (no host
copy); numpy arrays and CPU tensors work too and come back as the same kind.

The rasterization contract (clip space, pixel centres, coverage, visibility, rast_out, lighting) is DESIGN.md
s"Renderer".  Parity with real nvdiffrast has not been checked (it has no ROCm build): edge, tie and snapping
behaviour may differ from its rasterizer by a pixel along silhouettes.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import device_of, empty, is_torch, launch, ptr

glcam_in_cvcam = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]).astype(float)

_pose_chunk = 0


def set_pose_chunk(n):
    """Poses per workspace chunk of the following render calls (0: as many as 128 MB of per-pixel keys hold).
    Results do not depend on it; tests use it to force several chunks."""
    global _pose_chunk
    if not 0 <= int(n) <= 65535:
        raise _lib.PedpError(f"pose chunk {n} out of range")
    _pose_chunk = int(n)


def projection_matrix_from_intrinsics(K, height, width, znear, zfar, window_coords="y_down"):
    """OpenGL projection of a pinhole camera (float64, 4 x 4), image origin at (0, 0)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    w, h = float(width), float(height)
    span = float(zfar - znear)
    a = -(zfar + znear) / span
    b = -2 * (zfar * znear) / span
    if window_coords == "y_down":
        row1 = [0, 2 * K[1, 1] / h, (2 * K[1, 2] - h) / h, 0]
    elif window_coords == "y_up":
        row1 = [0, -2 * K[1, 1] / h, (-2 * K[1, 2] + h) / h, 0]
    else:
        raise NotImplementedError(window_coords)
    return np.array([[2 * K[0, 0] / w, -2 * K[0, 1] / w, (-2 * K[0, 2] + w) / w, 0], row1, [0, 0, a, b], [0, 0, -1, 0]])


# ---------------------------------------------------------------- mesh tensors

def _np(x, dtype):
    if x is None:
        return None
    if is_torch(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def make_mesh_tensors(mesh, device="cuda", max_tex_size=None):
    """mesh -> dict of torch tensors on `device`: pos, faces, vnormals and either vertex_color (V x 3 in [0, 1]) or
    tex (1 x h x w x 3), uv (V x 2, v flipped) and uv_idx.  `mesh`: trimesh-like (vertices, faces, vertex_normals,
    visual.vertex_colors or visual.uv + visual.material.image) or the package's TriangleMesh."""
    import torch

    faces = getattr(mesh, "faces", None)
    if faces is None:
        faces = getattr(mesh, "triangles")
    verts = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    vn = np.asarray(getattr(mesh, "vertex_normals", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
    if len(vn) != len(verts):
        if hasattr(mesh, "compute_vertex_normals"):
            mesh.compute_vertex_normals()
            vn = np.asarray(mesh.vertex_normals, dtype=np.float64).reshape(-1, 3)
        else:
            raise ValueError("mesh has no vertex normals")
    out = {}
    visual = getattr(mesh, "visual", None)
    uv = getattr(visual, "uv", None) if visual is not None else None
    material = getattr(visual, "material", None) if visual is not None else None
    image = getattr(material, "image", None) if material is not None else None
    if uv is not None and image is not None:
        if hasattr(image, "convert"):
            image = image.convert("RGB")
        img = np.asarray(image)
        if img.ndim == 2:
            img = np.repeat(img[..., None], 3, axis=2)
        img = img[..., :3]
        if max_tex_size is not None and max(img.shape[0], img.shape[1]) > max_tex_size:
            raise NotImplementedError("max_tex_size would resize the texture (the reference uses cv2.resize, not available)")
        out["tex"] = torch.as_tensor(np.ascontiguousarray(img), device=device, dtype=torch.float)[None] / 255.0
        out["uv_idx"] = torch.as_tensor(faces.astype(np.int32), device=device, dtype=torch.int)
        uvt = torch.as_tensor(np.asarray(uv, dtype=np.float64), device=device, dtype=torch.float)
        uvt[:, 1] = 1 - uvt[:, 1]
        out["uv"] = uvt
    else:
        vc = getattr(visual, "vertex_colors", None) if visual is not None else getattr(mesh, "vertex_colors", None)
        if vc is None or len(vc) != len(verts):
            vc = np.tile(np.array([128, 128, 128]).reshape(1, 3), (len(verts), 1))
        out["vertex_color"] = torch.as_tensor(np.asarray(vc)[..., :3], device=device, dtype=torch.float) / 255.0
    out.update({
        "pos": torch.tensor(verts, device=device, dtype=torch.float),
        "faces": torch.tensor(faces.astype(np.int32), device=device, dtype=torch.int),
        "vnormals": torch.tensor(vn, device=device, dtype=torch.float),
    })
    return out


# ---------------------------------------------------------------- dispatch

class _Call:
    """The arrays of one library call on host (numpy) or device (torch CUDA) memory: inputs are made contiguous float32 /
    int32 on the call's side (host arrays by a pageable copy that torch waits for), results come back as the inputs' kind."""

    def __init__(self, *probe):
        self.dev = device_of(*probe)
        self.torch_cpu = is_torch(probe[0]) and not probe[0].is_cuda  # host results come back as the first input's kind
        self.keep = []

    def arr(self, x, dtype="f4"):
        if x is None:
            return None
        if self.dev is not None:
            import torch

            t = torch.as_tensor(x, device=self.dev, dtype=torch.float32 if dtype == "f4" else torch.int32).contiguous()
            self.keep.append(t)
            return t
        a = _np(x, np.float32 if dtype == "f4" else np.int32)
        self.keep.append(a)
        return a

    def result(self, a):
        if a is None or self.dev is not None or not self.torch_cpu:
            return a
        import torch

        return torch.from_numpy(a)


def _run(call, fn_name, fn):
    """launch with the pose chunk set on the same context in front of the call."""
    def configured(lib, h, mem):
        _lib.check(lib.pedp_render_configure(h, _pose_chunk), "pedp_render_configure")
        return fn(lib, h, mem)

    launch(call.dev, fn_name, configured)


def _shape_error(msg):
    return _lib.PedpError(msg)


def _resolution(res):
    r = [int(v) for v in np.asarray(res).reshape(-1)]
    if len(r) != 2 or r[0] <= 0 or r[1] <= 0:
        raise _shape_error(f"resolution must be (height, width) > 0, got {res}")
    return r[0], r[1]


# ---------------------------------------------------------------- nvdiffrast_render

def nvdiffrast_render(K=None, H=None, W=None, ob_in_cams=None, glctx=None, context="cuda", get_normal=False, mesh_tensors=None,
                      mesh=None, projection_mat=None, bbox2d=None, output_size=None, use_light=False, light_color=None,
                      light_dir=np.array([0, 0, 1]), light_pos=np.array([0, 0, 0]), w_ambient=0.8, w_diffuse=0.5, extra={}):
    """Plain rendering of N poses of one mesh (no gradient).  K: 3 x 3; ob_in_cams: N x 4 x 4 (OpenCV camera);
    projection_mat: 4 x 4 (default from K, znear 0.001, zfar 100); bbox2d: N x 4 (umin, vmin, umax, vmax) crop windows;
    output_size: (height, width), default (H, W).  Returns (color N x h x w x 3, depth N x h x w, normal map N x h x w x 3
    or None) and sets extra['xyz_map'] (N x h x w x 3), rows in image order."""
    if context not in ("cuda", "gl"):
        raise NotImplementedError(context)
    if mesh_tensors is None:
        dev = ob_in_cams.device if is_torch(ob_in_cams) else "cpu"
        mesh_tensors = make_mesh_tensors(mesh, device=dev)
    call = _Call(ob_in_cams, mesh_tensors["pos"])
    poses = call.arr(ob_in_cams)
    if poses.ndim != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _shape_error(f"ob_in_cams must be N x 4 x 4, got {tuple(poses.shape)}")
    N = int(poses.shape[0])
    if projection_mat is None:
        projection_mat = projection_matrix_from_intrinsics(_np(K, np.float64), height=H, width=W, znear=0.001, zfar=100)
    proj = _np(projection_mat, np.float64).astype(np.float32).reshape(-1)
    if proj.size != 16:
        raise _shape_error("projection_mat must be 4 x 4")
    if output_size is None:
        output_size = np.asarray([H, W])
    oh, ow = _resolution(output_size)
    verts = call.arr(mesh_tensors["pos"])
    faces = call.arr(mesh_tensors["faces"], "i4")
    vnormals = call.arr(mesh_tensors["vnormals"])
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise _shape_error("mesh_tensors: pos must be V x 3 and faces F x 3")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if tuple(vnormals.shape) != (V, 3):
        raise _shape_error("mesh_tensors: vnormals must be V x 3")
    has_tex = "tex" in mesh_tensors
    vcolor = uv = tex = None
    th = tw = 0
    if has_tex:
        tex = call.arr(mesh_tensors["tex"])
        uv = call.arr(mesh_tensors["uv"])
        if tex.ndim == 4:
            if tex.shape[0] != 1:
                raise NotImplementedError("one texture per mesh")
            tex = tex[0]
        if tex.ndim != 3 or tex.shape[2] != 3 or tuple(uv.shape) != (V, 2):
            raise _shape_error("mesh_tensors: tex must be [1 x] h x w x 3 and uv V x 2")
        uv_idx = mesh_tensors.get("uv_idx")
        if uv_idx is not None and not np.array_equal(_np(uv_idx, np.int32), _np(faces, np.int32)):
            raise NotImplementedError("uv_idx other than faces")
        th, tw = int(tex.shape[0]), int(tex.shape[1])
    else:
        vcolor = call.arr(mesh_tensors["vertex_color"])
        if tuple(vcolor.shape) != (V, 3):
            raise _shape_error("mesh_tensors: vertex_color must be V x 3")
    bb = None
    if bbox2d is not None:
        bb = call.arr(bbox2d)
        if tuple(bb.shape) != (N, 4):
            raise _shape_error(f"bbox2d must be N x 4, got {tuple(bb.shape)}")
    if use_light:
        get_normal = True
    prm = _lib.RenderParams()
    prm.H, prm.W = (int(H), int(W)) if H is not None else (oh, ow)
    prm.out_h, prm.out_w = oh, ow
    prm.proj[:] = proj.tolist()
    prm.use_light = int(bool(use_light))
    prm.light_mode = 0 if light_dir is not None else 1
    if light_dir is not None:
        prm.light_dir[:] = _np(light_dir, np.float32).reshape(3).tolist()
    else:
        prm.light_pos[:] = _np(light_pos, np.float32).reshape(3).tolist()
    prm.has_light_color = int(light_color is not None)
    if light_color is not None:
        prm.light_color[:] = np.broadcast_to(_np(light_color, np.float32).reshape(-1), (3,)).tolist()
    prm.w_ambient, prm.w_diffuse = float(w_ambient), float(w_diffuse)
    color = empty(call.dev, (N, oh, ow, 3))
    depth = empty(call.dev, (N, oh, ow))
    normal = empty(call.dev, (N, oh, ow, 3)) if get_normal else None
    xyz = empty(call.dev, (N, oh, ow, 3))
    p = ptr
    _run(call, "pedp_render", lambda lib, h, mem: lib.pedp_render(
        h, p(verts), V, p(faces), F, p(vnormals), p(vcolor), p(uv), p(tex), th, tw, p(poses), p(bb), N, C.byref(prm), mem,
        p(color), p(depth), p(normal), p(xyz)))
    extra["xyz_map"] = call.result(xyz)
    return call.result(color), call.result(depth), call.result(normal)


# ---------------------------------------------------------------- dr shim

class RasterizeCudaContext:
    """Token standing in for nvdiffrast's rasterizer context (the work runs on the library's context of the device)."""

    def __init__(self, device=None):
        self.device = device


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """Instanced mode: pos N x V x 4 clip space, tri F x 3 -> (rast_out N x H x W x 4, None); rast_out = (u, v, z/w,
    triangle id + 1), zero on the background, GL row order (row 0 at NDC y = -1)."""
    if ranges is not None or (is_torch(pos) and pos.requires_grad):
        raise NotImplementedError("dr.rasterize: range mode and gradients are not supported")
    if len(getattr(pos, "shape", ())) != 3:
        raise NotImplementedError("dr.rasterize: instanced mode only (pos N x V x 4)")
    call = _Call(pos, tri)
    P, T = call.arr(pos), call.arr(tri, "i4")
    if P.shape[2] != 4 or T.ndim != 2 or T.shape[1] != 3:
        raise _shape_error(f"dr.rasterize: pos must be N x V x 4 and tri F x 3, got {tuple(P.shape)}, {tuple(T.shape)}")
    H, W = _resolution(resolution)
    N, V, F = int(P.shape[0]), int(P.shape[1]), int(T.shape[0])
    out = empty(call.dev, (N, H, W, 4))
    _run(call, "pedp_rasterize", lambda lib, h, mem: lib.pedp_rasterize(h, ptr(P), N, V, ptr(T), F, H, W, mem, ptr(out)))
    return call.result(out), None


def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """attr V x A or N x V x A, rast N x H x W x 4, tri F x 3 -> (out N x H x W x A, None); zero on the background."""
    if diff_attrs is not None or (is_torch(attr) and attr.requires_grad):
        raise NotImplementedError("dr.interpolate: gradients are not supported")
    call = _Call(attr, rast, tri)
    A_, R, T = call.arr(attr), call.arr(rast), call.arr(tri, "i4")
    if R.ndim != 4 or R.shape[3] != 4 or T.ndim != 2 or T.shape[1] != 3 or A_.ndim not in (2, 3):
        raise _shape_error("dr.interpolate: attr must be V x A or N x V x A, rast N x H x W x 4, tri F x 3")
    N, H, W = (int(v) for v in R.shape[:3])
    batched = A_.ndim == 3
    if batched and A_.shape[0] != N:
        raise _shape_error(f"dr.interpolate: {A_.shape[0]} attribute sets for {N} images")
    V, A = int(A_.shape[-2]), int(A_.shape[-1])
    out = empty(call.dev, (N, H, W, A))
    _run(call, "pedp_interpolate", lambda lib, h, mem: lib.pedp_interpolate(
        h, ptr(A_), int(batched), V, A, ptr(R), N, H, W, ptr(T), int(T.shape[0]), mem, ptr(out)))
    return call.result(out), None


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    """tex 1 x h x w x C or N x h x w x C, uv N x H x W x 2 -> N x H x W x C; bilinear (texel centres at +0.5), wrap."""
    if uv_da is not None or mip_level_bias is not None or mip is not None or (max_mip_level not in (None, 0)):
        raise NotImplementedError("dr.texture: mipmaps are not supported")
    if filter_mode not in ("linear", "auto") or boundary_mode != "wrap":
        raise NotImplementedError(f"dr.texture: filter_mode {filter_mode!r} / boundary_mode {boundary_mode!r}")
    if (is_torch(tex) and tex.requires_grad) or (is_torch(uv) and uv.requires_grad):
        raise NotImplementedError("dr.texture: gradients are not supported")
    call = _Call(tex, uv)
    Tx, U = call.arr(tex), call.arr(uv)
    if Tx.ndim != 4 or U.ndim != 4 or U.shape[3] != 2:
        raise _shape_error("dr.texture: tex must be n x h x w x C and uv N x H x W x 2")
    N, H, W = (int(v) for v in U.shape[:3])
    tn, th, tw, Cc = (int(v) for v in Tx.shape)
    out = empty(call.dev, (N, H, W, Cc))
    _run(call, "pedp_texture", lambda lib, h, mem: lib.pedp_texture(h, ptr(Tx), tn, th, tw, Cc, ptr(U), N, H, W, mem,
                                                             ptr(out)))
    return call.result(out)


class _Dr:
    """`import nvdiffrast.torch as dr` stand-in: bind `dr = pedp_hip.compat.dr`."""
    RasterizeCudaContext = RasterizeCudaContext
    rasterize = staticmethod(rasterize)
    interpolate = staticmethod(interpolate)
    texture = staticmethod(texture)


dr = _Dr()
