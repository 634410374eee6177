"""The mesh pipeline of the FIT_INVERSE task without pytorch3d: OBJ loading, camera, rasteriser, G-buffer.

Everything ``build_renderer`` (src/utils/pytorch3d_envmap_shader.py:177-217) takes from pytorch3d, restated from pytorch3d's
documented behaviour for the one way the reference uses it -- one mesh, ``FoVPerspectiveCameras()`` with its defaults,
``RasterizationSettings(image_size=S, blur_radius=0.0, faces_per_pixel=1, perspective_correct=False)`` -- with the
per-vertex normals and the rasteriser + interpolation on the device (``reni_mesh_vertex_normals`` /
``reni_rasterize_mesh``, include/reni_hip.h).  The shading is the existing HIP shader (``envmap_shader``), unchanged.

Conventions (pytorch3d's): world -> view is ``p @ R + T`` with row vectors; NDC +X points left and +Y up, so image row 0
is the top and column 0 the left edge at +x; the depth kept in ``zbuf`` is view-space z; barycentrics are NDC-space.
In the reference only the environment map carries a gradient.  Here the vertex positions may too (``verts.requires_grad``):
the G-buffer's normals and positions then carry a gradient to them through ``ops.gbuffer_backward`` with the face assignment
held fixed (no silhouette or occlusion gradient).  So may the camera: an ``R``, a ``T`` or a fov tensor that requires grad gets
the gradient of the G-buffer and of the soft silhouette (``ops.gbuffer_backward_camera``,
``ops.soft_silhouette_backward_camera``); ``look_at_rotation``, ``camera_from_position`` and ``so3_exp_map`` are the
parameterisations that keep ``R`` a rotation while a pose is fitted.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib, ops, textures
from .envmap_shader import (EnvironmentMap, MicrofacetMaterials, SpatialMaterials, _Materials, _shared_grid,
                            blinn_phong_shading_gbuffer, blinn_phong_shading_materials, compose_materials,
                            microfacet_shading_materials, shade_terms_normals)
from .textures import TexturedMaterials, TexturedMicrofacetMaterials

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords", "dists"])


def load_obj(path, device="cpu"):
    """``v`` and ``f`` lines of a Wavefront OBJ file -> (verts float32 [V,3], faces int64 [F,3]).

    Face entries may be ``a``, ``a/b``, ``a//c`` or ``a/b/c``; indices are 1-based, a negative index counts back from the
    last vertex read so far; a polygon is triangulated as the fan (0, i, i+1) (pytorch3d.io.load_obj).  ``vn`` / ``vt``
    lines, groups and materials are ignored: the normals are recomputed from the faces, as ``Meshes`` does."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"OBJ file not found: {path}")
    verts, faces = [], []
    with open(path, "r") as fh:
        for ln, line in enumerate(fh, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/", 1)[0])
                    if i == 0:
                        raise ValueError(f"{path}:{ln}: OBJ indices start at 1")
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs at least three vertices")
                faces.extend([idx[0], idx[i], idx[i + 1]] for i in range(1, len(idx) - 1))
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    f = torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)
    return v.to(device), f.to(device)


def load_obj_uv(path, device="cpu"):
    """``v``, ``vt`` and ``f`` lines of a Wavefront OBJ file -> (verts float32 [V,3], faces int64 [F,3], verts_uvs float32
    [Tn,2], faces_uvs int64 [F,3]), with ``load_obj``'s rules: 1-based indices, a negative one counts back from the last
    ``v`` (``vt``) read so far, a polygon becomes the fan (0, i, i+1).  A corner written ``a`` or ``a//c`` has no texture
    coordinate: its faces_uvs entry is -1 (a face with such a corner is not textured).  The third value of a ``vt`` line, if
    any, is ignored.  The UVs have their own indexing: Tn differs from V wherever a seam duplicates a vertex."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"OBJ file not found: {path}")
    verts, uvs, faces, faces_uv = [], [], [], []
    with open(path, "r") as fh:
        for ln, line in enumerate(fh, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "vt":
                if len(tok) < 3:
                    raise ValueError(f"{path}:{ln}: a texture coordinate needs two values")
                uvs.append([float(t) for t in tok[1:3]])
            elif tok[0] == "f":
                idx, tidx = [], []
                for t in tok[1:]:
                    part = t.split("/")
                    i = int(part[0])
                    if i == 0:
                        raise ValueError(f"{path}:{ln}: OBJ indices start at 1")
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                    if len(part) > 1 and part[1] != "":
                        j = int(part[1])
                        if j == 0:
                            raise ValueError(f"{path}:{ln}: OBJ indices start at 1")
                        tidx.append(j - 1 if j > 0 else len(uvs) + j)
                    else:
                        tidx.append(-1)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs at least three vertices")
                faces.extend([idx[0], idx[i], idx[i + 1]] for i in range(1, len(idx) - 1))
                faces_uv.extend([tidx[0], tidx[i], tidx[i + 1]] for i in range(1, len(tidx) - 1))
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    f = torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)
    vt = torch.tensor(uvs, dtype=torch.float32).reshape(-1, 2)
    ft = torch.tensor(faces_uv, dtype=torch.int64).reshape(-1, 3)
    return v.to(device), f.to(device), vt.to(device), ft.to(device)


def rotate_axis_angle_y(verts: torch.Tensor, degrees: float) -> torch.Tensor:
    """``RotateAxisAngle(degrees, "Y").transform_points(verts)``: a right-handed rotation about +Y (90 deg takes +X to -Z)."""
    a = torch.tensor(float(degrees), dtype=torch.float32) / 180.0 * math.pi
    c, s = torch.cos(a), torch.sin(a)
    one, zero = torch.ones(()), torch.zeros(())
    R = torch.stack([torch.stack([c, zero, s]), torch.stack([zero, one, zero]), torch.stack([-s, zero, c])])
    return verts @ R.t().to(verts.device, verts.dtype)  # row vectors: p @ R^T = (R p^T)^T


def _look_at_axes(d: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """R [N,3,3] (world -> view, row vectors) of a camera that looks along ``d`` [N,3] with ``up`` [N,3] (pytorch3d's
    look_at_rotation: z = d normalised, x = up x z, y = z x x; x = y x z when looking straight up or down)."""
    z = torch.nn.functional.normalize(d, eps=1e-5)
    x = torch.nn.functional.normalize(torch.cross(up, z, dim=1), eps=1e-5)
    y = torch.nn.functional.normalize(torch.cross(z, x, dim=1), eps=1e-5)
    if bool(torch.isclose(x, torch.zeros_like(x), atol=5e-3).all()):  # looking straight up or down
        x = torch.nn.functional.normalize(torch.cross(y, z, dim=1), eps=1e-5)
    return torch.cat([x[:, None], y[:, None], z[:, None]], dim=1).transpose(1, 2)


def _row3(v, like: torch.Tensor = None) -> torch.Tensor:
    """three numbers or a tensor of three as [1,3]: a tensor keeps its graph, dtype and device, anything else takes ``like``'s"""
    if isinstance(v, torch.Tensor):
        return v.reshape(1, 3)
    ref = like if like is not None else torch.zeros((), dtype=torch.float32)
    return torch.tensor([float(x) for x in v], dtype=ref.dtype, device=ref.device).reshape(1, 3)


def look_at_rotation(camera_position, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)) -> torch.Tensor:
    """R [1,3,3] of a camera at ``camera_position`` ([3] or [1,3]) looking at ``at`` with ``up`` up (pytorch3d's function of
    that name).  Plain torch on the position's device and dtype, differentiable: an orthonormal R whatever the position, which
    is what makes the position a parameter a pose fit can step."""
    C = _row3(camera_position)
    return _look_at_axes(_row3(at, C) - C, _row3(up, C))


def camera_from_position(camera_position, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(R [1,3,3], T [1,3]) of the camera at ``camera_position`` looking at ``at``: ``look_at_rotation`` and T = -C R, the
    translation that puts the camera's centre at the view-space origin.  Differentiable in the position."""
    C = _row3(camera_position)
    R = look_at_rotation(C, at, up)
    return R, -torch.bmm(C[:, None, :], R)[:, 0, :]


def so3_exp_map(log_rot: torch.Tensor) -> torch.Tensor:
    """R [N,3,3] = exp(hat(w)) for axis-angle vectors w ([3] or [N,3]) by Rodrigues' formula, I + A K + B K^2 with
    A = sin(th) / th, B = (1 - cos(th)) / th^2, K = hat(w) (pytorch3d's convention).  Below th^2 = 1e-4 A and B come from
    their series (1 - th^2/6 + th^4/120, 1/2 - th^2/24 + th^4/720: exact to rounding there), so the value and the gradient are
    finite at w = 0.  Plain torch, differentiable, on the input's device and dtype."""
    w = log_rot.reshape(-1, 3)
    t2 = (w * w).sum(dim=1)
    small = t2 < 1e-4
    th = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    A = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - torch.cos(th)) / (th * th))
    zero = torch.zeros_like(t2)
    K = torch.stack([zero, -w[:, 2], w[:, 1], w[:, 2], zero, -w[:, 0], -w[:, 1], w[:, 0], zero], dim=1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=w.dtype, device=w.device)[None]
    return eye + A[:, None, None] * K + B[:, None, None] * torch.bmm(K, K)


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, degrees: bool = True, device=None):
    """Camera on a sphere round the origin looking at it with +Y up -> (R [1,3,3], T [1,3]); (2, 0, 0) gives
    R = diag(-1, 1, -1), T = (0, 0, 2).  ``dist``, ``elev`` and ``azim`` may be tensors (one value each): the result then keeps
    their graph and, unless ``device`` says otherwise, their device.  With numbers: float32 on ``device`` (default the CPU)."""
    given = [v for v in (dist, elev, azim) if isinstance(v, torch.Tensor)]
    at = given[0].device if given else "cpu"
    d, e, a = (v.to(torch.float32).reshape(1).to(at) if isinstance(v, torch.Tensor) else torch.tensor([float(v)], dtype=torch.float32, device=at)
               for v in (dist, elev, azim))
    if degrees:
        e, a = e * (math.pi / 180.0), a * (math.pi / 180.0)
    C = torch.stack([d * torch.cos(e) * torch.sin(a), d * torch.sin(e), d * torch.cos(e) * torch.cos(a)], dim=1)  # [1,3]
    R = _look_at_axes(-C, torch.tensor([[0.0, 1.0, 0.0]], device=at))  # at (origin) - C
    T = -torch.bmm(R.transpose(1, 2), C[:, :, None])[:, :, 0]
    device = at if device is None else device
    return R.to(device), T.to(device)


class FoVPerspectiveCameras:
    """pytorch3d's FoVPerspectiveCameras as ``build_renderer`` creates it: fov 60 deg, znear 1, zfar 100, aspect 1, and
    R = I, T = 0 unless given (R, T passed to a renderer call override them for that call).  ``fov`` may be a 0-d tensor: it
    is kept as given (so one that requires grad gets the rasteriser's gradient, ``tan_half_fov_tensor`` being the torch chain
    tan(fov / 2)), and ``tan_half_fov()`` reads its current value, so an optimiser's in-place step re-rasterises."""

    def __init__(self, znear=1.0, zfar=100.0, aspect_ratio=1.0, fov=60.0, degrees=True, R=None, T=None, device="cpu"):
        if float(aspect_ratio) != 1.0:
            raise ValueError("only aspect_ratio 1 (square images) is supported")
        self.znear, self.zfar, self.aspect_ratio = float(znear), float(zfar), 1.0
        self._fov_scale = math.pi / 180.0 if degrees else 1.0
        if isinstance(fov, torch.Tensor):
            if fov.dim() != 0:
                raise ValueError(f"a fov tensor must be 0-d (one camera), got {tuple(fov.shape)}")
            self.fov = fov
        else:
            self.fov, self._fov_scale = float(fov) * self._fov_scale, 1.0  # radians
        self.R = torch.eye(3)[None] if R is None else torch.as_tensor(R, dtype=torch.float32).reshape(1, 3, 3)
        self.T = torch.zeros(1, 3) if T is None else torch.as_tensor(T, dtype=torch.float32).reshape(1, 3)
        self.device = device
        self.R, self.T = self.R.to(device), self.T.to(device)

    def tan_half_fov(self) -> float:
        fov = float(self.fov.detach()) if isinstance(self.fov, torch.Tensor) else self.fov
        return math.tan(fov * self._fov_scale / 2.0)

    def tan_half_fov_tensor(self):
        """tan(fov / 2) as a function of the fov tensor, or None when the fov is a number or needs no gradient"""
        if not isinstance(self.fov, torch.Tensor) or not self.fov.requires_grad:
            return None
        return torch.tan(self.fov * (self._fov_scale / 2.0))

    def get_camera_center(self, R=None, T=None) -> torch.Tensor:
        """World position of the camera [1,3]: the C with C @ R + T = 0."""
        R = self.R if R is None else torch.as_tensor(R).reshape(1, 3, 3)
        T = self.T if T is None else torch.as_tensor(T).reshape(1, 3)
        return -torch.bmm(T[:, None, :].float(), R.float().transpose(1, 2))[:, 0, :]

    def to(self, device):
        self.R, self.T, self.device = self.R.to(device), self.T.to(device), device
        return self


class _VertexNormalsFn(torch.autograd.Function):
    """The cached vertex normals as a function of the vertices: the forward hands out the buffer ``ops.vertex_normals``
    filled, the backward is ``ops.vertex_normals_backward``."""

    @staticmethod
    def forward(ctx, verts, faces, normals, vf):
        ctx.save_for_backward(verts, faces)
        ctx.vf = vf
        return normals.detach()

    @staticmethod
    def backward(ctx, g):
        verts, faces = ctx.saved_tensors
        return ops.vertex_normals_backward(verts.detach(), faces, g.contiguous(), vf=ctx.vf), None, None, None


def _camera_grads(ctx, R, T, tanf, gR, gT, g_tan):
    """the kernel's camera gradient in the shapes, dtypes and devices of the inputs that asked for one"""
    need = ctx.needs_input_grad
    return (gR.reshape(R.shape).to(R.device, R.dtype) if need[1] else None,
            gT.reshape(T.shape).to(T.device, T.dtype) if need[2] else None,
            g_tan.reshape(tanf.shape).to(tanf.device, tanf.dtype) if need[3] else None)


class _GBufferFn(torch.autograd.Function):
    """The cached G-buffer as a function of the vertices and of the camera (R, T, tan(fov / 2); the latter a tensor or
    None): the forward hands out the buffers ``ops.rasterize_mesh`` filled (same kernel, same bits), the backward is
    ``ops.gbuffer_backward`` over the record's pix_to_face -- the vertex-normal chain included, so the normals the rasteriser
    interpolated enter as a constant -- or, when something of the camera needs a gradient, ``ops.gbuffer_backward_camera``
    (without the vertex kernels when the vertices need none).  A node per call: two renders of one cached G-buffer are
    back-propagated separately."""

    @staticmethod
    def forward(ctx, verts, R, T, tanf, rec):
        ctx.save_for_backward(verts, R, T, tanf)
        ctx.rec = rec
        ctx.set_materialize_grads(False)
        return rec["nrm"].detach(), rec["pos"].detach()

    @staticmethod
    def backward(ctx, gN, gX):
        verts, R, T, tanf = ctx.saved_tensors
        rec = ctx.rec
        need_verts, need_cam = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:4])
        if gN is None and gX is None:
            return torch.zeros_like(verts) if need_verts else None, None, None, None, None
        if rec.get("table") is None:  # the pixels sorted by face: once per G-buffer, on the device
            rec["table"] = ops.face_pixel_table(rec["p2f"], rec["faces"].shape[0])
        args = (verts.detach(), rec["faces"], rec["normals"], rec["R"], rec["T"], rec["S"], rec["p2f"],
                None if gN is None else gN.contiguous(), None if gX is None else gX.contiguous())
        if not need_cam:
            return ops.gbuffer_backward(*args, tan_half_fov=rec["tan_half_fov"], table=rec["table"], vf=rec["vf"]), None, None, None, None
        g, gR, gT, g_tan = ops.gbuffer_backward_camera(*args, tan_half_fov=rec["tan_half_fov"], table=rec["table"], vf=rec["vf"],
                                                       need_verts=need_verts)
        return (g,) + _camera_grads(ctx, R, T, tanf, gR, gT, g_tan) + (None,)


class _SilhouetteFn(torch.autograd.Function):
    """The cached soft silhouette as a function of the vertices and of the camera: the forward hands out the buffer
    ``ops.soft_silhouette`` filled, the backward is ``ops.soft_silhouette_backward`` over the record's trans, or
    ``ops.soft_silhouette_backward_camera`` when something of the camera needs a gradient.  A node per call, as ``_GBufferFn``."""

    @staticmethod
    def forward(ctx, verts, R, T, tanf, rec):
        ctx.save_for_backward(verts, R, T, tanf)
        ctx.rec = rec
        return rec["alpha"].detach()

    @staticmethod
    def backward(ctx, gA):
        verts, R, T, tanf = ctx.saved_tensors
        rec = ctx.rec
        args = (verts.detach(), rec["faces"], rec["R"], rec["T"], rec["S"], rec["tan_half_fov"], rec["sigma"], rec["blur_radius"],
                rec["trans"], gA.contiguous())
        if not any(ctx.needs_input_grad[1:4]):
            return ops.soft_silhouette_backward(*args, vf=rec["vf"]), None, None, None, None
        g, gR, gT, g_tan = ops.soft_silhouette_backward_camera(*args, vf=rec["vf"], need_verts=ctx.needs_input_grad[0])
        return (g,) + _camera_grads(ctx, R, T, tanf, gR, gT, g_tan) + (None,)


def silhouette_iou(alpha: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The soft IoU loss of a coverage ``alpha`` against a target ``mask`` of the same number of pixels (values in [0, 1]):
    1 - sum(a m) / sum(a + m - a m).  Plain torch; 0 where both are empty."""
    a, m = alpha.reshape(-1), mask.reshape(-1).to(alpha.dtype)
    if a.numel() != m.numel():
        raise ValueError(f"alpha has {a.numel()} pixels, the mask {m.numel()}")
    inter = (a * m).sum()
    union = (a + m - a * m).sum()
    return 1.0 - inter / union.clamp_min(1e-12)


class Meshes:
    """One triangle mesh in pytorch3d's packed form: ``Meshes(verts=[v], faces=[f])``; the vertex normals come from the
    HIP kernel (a device tensor is needed for them) and are kept until the vertices or faces are modified in place (the key
    is their ``_version``).  When the vertices require grad the normals carry a gradient to them.  ``verts_uvs=[vt], faces_uvs=[ft]`` (both or
    neither; ``load_obj_uv``) give the mesh texture coordinates: vt [Tn,2], ft [F,3] with its own indexing, an entry
    outside [0, Tn) marking a face without them."""

    def __init__(self, verts, faces, verts_uvs=None, faces_uvs=None):
        if len(verts) != 1 or len(faces) != 1:
            raise ValueError("one mesh per Meshes (several meshes per batch are not supported)")
        self._verts = verts[0].to(torch.float32).contiguous()
        self._faces = faces[0].to(torch.int64).contiguous()
        self._normals = None
        self._vf = None
        self._el = None
        self._st = None
        self._verts_uvs = self._faces_uvs = None
        if (verts_uvs is None) != (faces_uvs is None):
            raise ValueError("verts_uvs and faces_uvs come together")
        if verts_uvs is not None:
            if len(verts_uvs) != 1 or len(faces_uvs) != 1:
                raise ValueError("one mesh per Meshes (several meshes per batch are not supported)")
            vt, ft = verts_uvs[0].to(torch.float32).contiguous(), faces_uvs[0].to(torch.int64).contiguous()
            if vt.dim() != 2 or vt.shape[1] != 2 or vt.shape[0] < 1:
                raise ValueError(f"verts_uvs must be [Tn, 2] with Tn >= 1, got {tuple(vt.shape)}")
            if tuple(ft.shape) != tuple(self._faces.shape):
                raise ValueError(f"faces_uvs must be [F, 3] like faces, got {tuple(ft.shape)}")
            self._verts_uvs, self._faces_uvs = vt, ft

    def verts_packed(self) -> torch.Tensor:
        return self._verts

    def faces_packed(self) -> torch.Tensor:
        return self._faces

    def _vertex_faces(self):
        """the vertex -> (face, corner) lists of the backward kernels, kept per in-place version of the faces"""
        key = self._faces._version
        if self._vf is None or self._vf[0] != key:
            self._vf = (key, ops.vertex_face_lists(self._faces, self._verts.shape[0]))
        return self._vf[1]

    def _edge_lists(self):
        """the topology lists of the regularisers (``ops.mesh_edge_lists``), kept per in-place version of the faces"""
        key = self._faces._version
        if self._el is None or self._el[0] != key:
            self._el = (key, ops.mesh_edge_lists(self._faces, self._verts.shape[0]))
        return self._el[1]

    def _sample_table(self):
        """the area table of ``sample_points_from_meshes`` (``ops.mesh_sample_table``), kept per in-place version of the vertices
        and faces"""
        key = (self._verts._version, self._faces._version)
        if self._st is None or self._st[0] != key:
            self._st = (key, ops.mesh_sample_table(self._verts.detach(), self._faces))
        return self._st[1]

    def edges_packed(self) -> torch.Tensor:
        """[E, 2] int64: the unique undirected edges (a < b) of the faces taking part, in ascending (a, b)"""
        lists = self._edge_lists()
        return lists["edges"][:lists["E"]]

    def _normals_value(self) -> torch.Tensor:
        """the normals of the current vertices as a constant (no autograd node)"""
        key = (self._verts._version, self._faces._version)
        if self._normals is None or self._normals[0] != key:
            self._normals = (key, ops.vertex_normals(self._verts.detach(), self._faces, vf=self._vertex_faces()))
        return self._normals[1]

    def verts_normals_packed(self) -> torch.Tensor:
        n = self._normals_value()
        if self._verts.requires_grad and torch.is_grad_enabled():
            return _VertexNormalsFn.apply(self._verts, self._faces, n, self._vertex_faces())
        return n

    def verts_uvs_packed(self):
        return self._verts_uvs

    def faces_uvs_packed(self):
        return self._faces_uvs

    @property
    def device(self):
        return self._verts.device


_ICO_FACES = ((0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
              (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1))


def ico_sphere(level: int = 0, device="cpu") -> Meshes:
    """The unit icosphere as a ``Meshes``: level 0 is the icosahedron (12 vertices, 20 faces, outward winding); every level
    splits each face in four with ONE midpoint per edge, shared by the two faces on it, re-projected to the unit sphere.
    V = 10 * 4^level + 2, F = 20 * 4^level, E = 30 * 4^level.  Plain torch; a template to start a vertex fit from."""
    level = int(level)
    if level < 0:
        raise ValueError("level must be >= 0")
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = torch.tensor([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1),
                      (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], dtype=torch.float64)  # the cyclic permutations of (+-1, +-phi, 0)
    v = v / v.norm(dim=1, keepdim=True)
    f = torch.tensor(_ICO_FACES, dtype=torch.int64)
    for _ in range(level):
        V = v.shape[0]
        a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
        b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
        keys = torch.minimum(a, b) * V + torch.maximum(a, b)
        ukeys, inv = torch.unique(keys, return_inverse=True)  # one midpoint per undirected edge, in ascending (a, b)
        mid = v[ukeys // V] + v[ukeys % V]
        v = torch.cat([v, mid / mid.norm(dim=1, keepdim=True)])
        F = f.shape[0]
        m01, m12, m20 = V + inv[:F], V + inv[F:2 * F], V + inv[2 * F:]
        f = torch.cat([torch.stack([f[:, 0], m01, m20], 1), torch.stack([f[:, 1], m12, m01], 1),
                       torch.stack([f[:, 2], m20, m12], 1), torch.stack([m01, m12, m20], 1)])
    return Meshes(verts=[v.to(torch.float32).to(device)], faces=[f.to(device)])


class RasterizationSettings:
    """The settings the reference uses; anything else is outside what the HIP rasteriser implements."""

    def __init__(self, image_size=256, blur_radius=0.0, faces_per_pixel=1, perspective_correct=False, cull_backfaces=False):
        if not isinstance(image_size, int):
            raise ValueError("image_size must be an int (square images only)")
        if blur_radius != 0.0 or faces_per_pixel != 1 or perspective_correct or cull_backfaces:
            raise ValueError("supported: blur_radius 0, faces_per_pixel 1, perspective_correct False, no back-face culling")
        self.image_size = image_size
        self.blur_radius, self.faces_per_pixel, self.perspective_correct = 0.0, 1, False
        self.cull_backfaces = False


class MeshRasterizer(nn.Module):
    """``MeshRasterizer(cameras, raster_settings)(meshes_world, R=, T=) -> Fragments`` on the device.  The G-buffer of the
    last (mesh, R, T, size) is kept: the reference re-rasterises its constant mesh and camera on every render, here a
    training step then costs only the shader (same output).  The key is the identity and in-place version of the mesh's
    tensors and of R, T, so modifying any of them in place re-rasterises."""

    MAX_TAPS_RECORDS = 8  # texture_taps records kept per scene (albedo, ks and shininess textures of a few sizes)

    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras if cameras is not None else FoVPerspectiveCameras()
        self.raster_settings = raster_settings if raster_settings is not None else RasterizationSettings()
        self._cache = None
        self._accel_cache = None
        self._vis_cache = None
        self._uv_cache = None
        self._taps_cache = None
        self._tangent_cache = None
        self._sil_cache = None

    def gbuffer(self, meshes_world: Meshes, R=None, T=None, differentiable: bool = True):
        """-> (Fragments, pixel_normals [S*S,3], pixel_positions [S*S,3]) (interpolated, not normalised).

        When the mesh's vertices require grad (and grad is enabled, and ``differentiable``) the two G-buffers carry a
        gradient to them: the same cached buffers behind an autograd node built for this call (``ops.gbuffer_backward``:
        the face assignment is held fixed -- no silhouette or occlusion gradient).  The same holds for ``R``, ``T`` and a fov
        tensor of the cameras that require grad (``ops.gbuffer_backward_camera``: through the barycentric weights).  The
        Fragments never carry one.  Otherwise the cached tensors themselves are returned, as before."""
        R = self.cameras.R if R is None else torch.as_tensor(R)
        T = self.cameras.T if T is None else torch.as_tensor(T)
        S = self.raster_settings.image_size
        v, f = meshes_world.verts_packed(), meshes_world.faces_packed()
        key = tuple((id(t), t._version) for t in (v, f, R, T)) + (S, self.cameras.tan_half_fov())
        if self._cache is None or self._cache[0] != key:
            normals = meshes_world._normals_value()
            p2f, zbuf, bary, dists, nrm, pos = ops.rasterize_mesh(v.detach(), f, normals, R, T, S, self.cameras.tan_half_fov())
            out = (Fragments(p2f, zbuf, bary, dists), nrm, pos)
            rec = {"faces": f, "normals": normals, "R": R, "T": T, "S": S, "tan_half_fov": self.cameras.tan_half_fov(),
                   "p2f": p2f, "nrm": nrm, "pos": pos, "table": None, "vf": None}
            self._cache = (key, (v, f, R, T), out, rec)  # (the tensors are held so that their ids stay theirs)
        out, rec = self._cache[2], self._cache[3]
        tanf = self.cameras.tan_half_fov_tensor()
        if differentiable and torch.is_grad_enabled() and (v.requires_grad or R.requires_grad or T.requires_grad or tanf is not None):
            if v.requires_grad and rec["vf"] is None:
                rec["vf"] = meshes_world._vertex_faces()
            nrm, pos = _GBufferFn.apply(v, R, T, tanf, rec)
            return out[0], nrm, pos
        return out

    def silhouette(self, meshes_world: Meshes, R=None, T=None, sigma: float = 1e-4, blur_radius=None):
        """-> alpha [S, S], the soft coverage of the mesh (``ops.soft_silhouette``): 1 - prod over the faces near a pixel of
        (1 - sigmoid(-sd / sigma)), sd the signed squared NDC distance to the face's outline.  ``blur_radius`` (squared NDC
        units) cuts a face off where it is further away; None means log(1 / 1e-4 - 1) sigma, pytorch3d's convention.  It is an
        argument of this call: ``RasterizationSettings`` keeps blur_radius 0 for the hard rasteriser.

        Kept like the G-buffer, under the same key plus (sigma, blur_radius).  When the mesh's vertices require grad (and grad
        is enabled) the same cached buffer is returned behind an autograd node built for this call
        (``ops.soft_silhouette_backward``): this is the gradient that moves the outline.  ``R``, ``T`` and a fov tensor of the
        cameras that require grad get theirs from the same node (``ops.soft_silhouette_backward_camera``): the gradient a pose
        fit steps along.  Otherwise the cached tensor itself is returned."""
        R = self.cameras.R if R is None else torch.as_tensor(R)
        T = self.cameras.T if T is None else torch.as_tensor(T)
        S = self.raster_settings.image_size
        sigma = float(sigma)
        blur_radius = math.log(1.0 / 1e-4 - 1.0) * sigma if blur_radius is None else float(blur_radius)
        v, f = meshes_world.verts_packed(), meshes_world.faces_packed()
        tanf = self.cameras.tan_half_fov()
        key = tuple((id(t), t._version) for t in (v, f, R, T)) + (S, tanf, sigma, blur_radius)
        if self._sil_cache is None or self._sil_cache[0] != key:
            alpha, trans = ops.soft_silhouette(v.detach(), f, R, T, S, tanf, sigma, blur_radius)
            rec = {"faces": f, "R": R, "T": T, "S": S, "tan_half_fov": tanf, "sigma": sigma, "blur_radius": blur_radius,
                   "alpha": alpha.reshape(S, S), "trans": trans, "vf": None}
            self._sil_cache = (key, (v, f, R, T), rec)  # (the tensors are held so that their ids stay theirs)
        rec = self._sil_cache[2]
        tanf_t = self.cameras.tan_half_fov_tensor()
        if torch.is_grad_enabled() and (v.requires_grad or R.requires_grad or T.requires_grad or tanf_t is not None):
            if v.requires_grad and rec["vf"] is None:
                rec["vf"] = meshes_world._vertex_faces()
            return _SilhouetteFn.apply(v, R, T, tanf_t, rec)
        return rec["alpha"]

    def visibility(self, meshes_world: Meshes, R=None, T=None, dirs=None, t_min=None, no_cull: bool = False):
        """-> the int32 visibility mask [NB, S*S, ceil(J/32)] of ``dirs`` ([J,3] shared, NB = 1, or [B,J,3], NB = B) over the
        cached G-buffer: bit (p, j) is 1 where no face of the mesh but the pixel's own blocks direction j from the pixel's
        surface point (``ops.mesh_visibility``; ``unpack_visibility`` turns it into booleans).  t_min defaults to 1e-4 x
        the diagonal of the mesh's bounding box.  The lights are at infinity, so the mask is a constant of (mesh, camera,
        directions): the acceleration record is kept per mesh and the mask per (G-buffer key, the directions' memory, shape
        and in-place version, t_min), like the G-buffer itself."""
        if not isinstance(dirs, torch.Tensor):
            raise ValueError("dirs must be a tensor [J, 3] or [B, J, 3]")
        frags, _, pos = self.gbuffer(meshes_world, R, T, differentiable=False)  # the mask is a constant of the geometry
        gkey = self._cache[0]
        v, f = meshes_world.verts_packed(), meshes_world.faces_packed()
        akey = tuple((id(t), t._version) for t in (v, f))
        if self._accel_cache is None or self._accel_cache[0] != akey:
            diag = float((v.detach().max(dim=0).values - v.detach().min(dim=0).values).norm())
            self._accel_cache = (akey, (v, f), ops.mesh_visibility_prepare(v.detach(), f), diag)
        _, _, accel, diag = self._accel_cache
        t_min = 1e-4 * diag if t_min is None else float(t_min)
        # a view of the same memory (directions.expand(B, -1, -1)[0], a fresh Python object every step) is the same grid
        dkey = (dirs.data_ptr(), tuple(dirs.shape), tuple(dirs.stride()), dirs._version, str(dirs.device))
        key = (gkey, dkey, t_min, bool(no_cull))
        if self._vis_cache is not None and self._vis_cache[0] == key:
            return self._vis_cache[2]
        vis = ops.mesh_visibility(pos, frags.pix_to_face, dirs, accel, t_min, no_cull=no_cull)
        self._vis_cache = (key, dirs, vis)  # (dirs is held so that its memory stays its own)
        return vis

    def _uv_key(self, meshes_world: Meshes, R, T):
        vt, ft = meshes_world.verts_uvs_packed(), meshes_world.faces_uvs_packed()
        if vt is None:
            raise ValueError("the mesh has no texture coordinates (Meshes(verts_uvs=, faces_uvs=); load_obj_uv reads them)")
        self.gbuffer(meshes_world, R, T, differentiable=False)
        return (self._cache[0], tuple((id(t), t._version) for t in (vt, ft)))

    def pixel_uv(self, meshes_world: Meshes, R=None, T=None):
        """-> (uv [S*S,2], jac [S*S,4], pix_valid [S*S] int64) of the cached G-buffer (``ops.mesh_pixel_uv``): the pixel's
        texture coordinate, its per-face footprint derivative, and the pixel's face or -1 where nothing textured is seen.
        Kept beside the G-buffer under its key and the identity and in-place version of the mesh's UV tensors."""
        key = self._uv_key(meshes_world, R, T)
        if self._uv_cache is not None and self._uv_cache[0] == key:
            return self._uv_cache[2]
        frags = self._cache[2][0]
        _, (v, f, Rk, Tk), _, _ = self._cache
        vt, ft = meshes_world.verts_uvs_packed(), meshes_world.faces_uvs_packed()
        out = ops.mesh_pixel_uv(v, f, vt, ft, Rk, Tk, self.raster_settings.image_size, frags.pix_to_face, frags.bary_coords,
                                self.cameras.tan_half_fov())
        self._uv_cache = (key, (vt, ft), out)
        return out

    def pixel_tangents(self, meshes_world: Meshes, R=None, T=None):
        """-> (tangent [S*S,3], bitangent [S*S,3], valid [S*S] bool) of the cached G-buffer: the frame a tangent-space normal
        map is read in (``textures.tangent_frames`` on the pixel's face, its UVs and the G-buffer normal; plain torch, once
        per scene).  Kept beside ``pixel_uv`` under the same key."""
        key = self._uv_key(meshes_world, R, T)
        if self._tangent_cache is not None and self._tangent_cache[0] == key:
            return self._tangent_cache[2]
        _, _, valid = self.pixel_uv(meshes_world, R, T)
        _, (v, f, _, _), (_, nrm, _), _ = self._cache
        vt, ft = meshes_world.verts_uvs_packed(), meshes_world.faces_uvs_packed()
        out = textures.tangent_frames(v, f, vt, ft, valid, nrm)
        self._tangent_cache = (key, (vt, ft), out)
        return out

    def texture_taps(self, meshes_world: Meshes, R=None, T=None, size=None, levels=None, wrap: str = "clamp",
                     align_corners: bool = False, lod_bias: float = 0.0):
        """-> the ``textures.Taps`` of a texture of ``size`` = (H, W) seen through the cached G-buffer: the level per pixel
        from its footprint, 8 (element, weight) pairs, and the sorted table the gradient is gathered through.  One record is
        kept per (size, levels, wrap, align_corners, lod_bias) under the key of ``pixel_uv``, the MAX_TAPS_RECORDS newest; a
        new G-buffer or new UVs drop them all."""
        if size is None or len(tuple(size)) != 2:
            raise ValueError("size must be (H, W), the texture's size")
        key = self._uv_key(meshes_world, R, T)
        if self._taps_cache is None or self._taps_cache[0] != key:
            self._taps_cache = (key, {})
        sub = (int(size[0]), int(size[1]), None if levels is None else int(levels), wrap, bool(align_corners), float(lod_bias))
        found = self._taps_cache[1].get(sub)
        if found is None:
            uv, jac, valid = self.pixel_uv(meshes_world, R, T)
            found = textures.make_taps(uv, sub[:2], sub[2], jac=jac, pix_valid=valid, wrap=wrap, align_corners=bool(align_corners),
                                       lod_bias=float(lod_bias))
            if len(self._taps_cache[1]) >= self.MAX_TAPS_RECORDS:  # (a lod_bias sweep must not keep every table: oldest out)
                self._taps_cache[1].pop(next(iter(self._taps_cache[1])))
            self._taps_cache[1][sub] = found
        return found

    def forward(self, meshes_world: Meshes, R=None, T=None, **kwargs) -> Fragments:
        return self.gbuffer(meshes_world, R, T, differentiable=False)[0]


class HipMeshRenderer(nn.Module):
    """``renderer(meshes_world=mesh, R=R, T=T, envmap=...) -> (colors [B,S,S,3], pixel_normals [B,S,S,3])``: the call the
    reference makes on its pytorch3d MeshRenderer (RENI_module.py:393-396).  The rasteriser's G-buffer goes straight into
    ``blinn_phong_shading_gbuffer`` (the existing HIP shader and its autograd function).

    Reference quirk kept: the reference's shader asks ``cameras.get_camera_center()`` WITHOUT R and T
    (pytorch3d_envmap_shader.py:78; MeshRenderer hands R and T to the rasteriser only as keyword arguments), so its
    specular term uses the centre of the default camera -- the world origin -- not the rendering camera's (0, 0, 2).  The
    same is done here.  With the default KD_VALUE = 1 (no specular term) it has no effect.

    ``shadows=True``: the mesh blocks light (``MeshRasterizer.visibility`` of the envmap's directions, cached; the shader
    then counts only the texels a pixel sees).  The default, False, renders what the reference renders.

    ``materials=SpatialMaterials(...)``: an albedo, a ks and a shininess per render pixel (S*S of them) instead of the
    scalars kd, ks and ``materials.shininess``; the render is then differentiable with respect to them as well (the shader's
    terms path, ``envmap_shader.blinn_phong_shading_materials``), and kd / ks are not used.  With any other ``materials``
    the call and its bits are the scalar shader's.

    ``materials=TexturedMaterials(...)``: the material lives in the mesh's UV space (``reni_amd.textures``): the taps come
    from the rasteriser's cache, the textures are fetched per pixel and go down the same terms path; the render is
    differentiable with respect to the textures.  Several renderers -- each with its own rasteriser, camera and, through
    ``shader_cameras=FoVPerspectiveCameras(R=R, T=T)``, its true camera centre -- may share one such object.  With a
    ``normal`` texture the shader gets ``materials.shading_normals(...)`` (the normal map's) instead of the G-buffer's normals,
    and the render is differentiable with respect to that texture when it requires grad; the shadow mask and the returned
    ``pixel_normals`` stay the geometry's (``shading_normals(mesh, R, T)`` returns the bent ones).

    ``materials=MicrofacetMaterials(...)`` / ``TexturedMicrofacetMaterials(...)``: a base colour, a roughness and a metallic
    per render pixel / in the mesh's UV space, shaded by the microfacet (GGX) terms
    (``envmap_shader.microfacet_shading_materials``); everything said above about the two Blinn-Phong classes holds for
    their microfacet siblings, the normal texture included.

    Geometry: when the mesh's vertices require grad the render and the returned ``pixel_normals`` carry a gradient to them
    through the G-buffer's normals (``MeshRasterizer.gbuffer``): shape from shading under a fixed silhouette.  The scalar
    kd / ks renderer then goes through ``shade_terms_normals`` + ``compose_materials`` (equal to the fused scalar kernel to
    rounding; the fused kernel stays whenever the vertices need no gradient), ``SpatialMaterials`` through the same terms,
    ``MicrofacetMaterials`` as always.  Deliberately dropped: the positions are handed to the shader detached (the view
    vector's dependence on the geometry), the shadow mask is computed from detached tensors and stays constant, pixels do
    not change face.  ``TexturedMaterials`` / ``TexturedMicrofacetMaterials`` raise a ValueError: UVs, taps and tangent
    frames under moving geometry are out of scope.

    Camera: an ``R``, a ``T`` or a fov tensor that requires grad takes the same branches as vertices that do, through the same
    G-buffer node (``ops.gbuffer_backward_camera``).  Deliberately dropped as well: the shader's positions and its
    ``camera_center`` stay constants (the view vector's dependence on the pose), and the shadow mask stays constant.  The
    UV-space materials raise a ValueError that names the camera."""

    def __init__(self, rasterizer: MeshRasterizer, kd: float = None, ks: float = None, materials=None, shader_cameras=None,
                 shadows: bool = False):
        super().__init__()
        self.rasterizer = rasterizer
        self.shadows = bool(shadows)  # cast shadows: the mesh blocks the texels it hides from a pixel
        self.spatial = isinstance(materials, SpatialMaterials)
        self.microfacet = isinstance(materials, (MicrofacetMaterials, TexturedMicrofacetMaterials))
        self.textured = isinstance(materials, (TexturedMaterials, TexturedMicrofacetMaterials))
        if kd is None and not self.spatial and not self.textured and not self.microfacet:
            raise ValueError("kd is required unless materials is a SpatialMaterials, a TexturedMaterials or one of their "
                             "microfacet siblings")
        self.kd = 1.0 if kd is None else float(kd)
        self.ks = 1.0 - self.kd if ks is None else float(ks)
        self.materials = materials if materials is not None else _Materials(500.0)
        shader_cameras = shader_cameras if shader_cameras is not None else rasterizer.cameras
        # no R, T: the reference's quirk (see above); kept on the host, where the shader entry point reads it
        self.camera_center = shader_cameras.get_camera_center().detach().reshape(3).cpu()

    def forward(self, meshes_world: Meshes = None, R=None, T=None, envmap: EnvironmentMap = None, **kwargs):
        _, nrm, pos = self.rasterizer.gbuffer(meshes_world, R, T)
        geometry = nrm.requires_grad  # the vertices or the camera require grad: the G-buffer carries a gradient to them
        if geometry:
            if self.textured and not meshes_world.verts_packed().requires_grad:
                raise ValueError(f"{type(self.materials).__name__} cannot be rendered while the camera (R, T or the fov) requires "
                                 "grad: UVs, taps and tangent frames under a moving camera are out of scope (detach the camera, "
                                 "or use SpatialMaterials / MicrofacetMaterials)")
            if self.textured:
                raise ValueError(f"{type(self.materials).__name__} cannot be rendered while the mesh's vertices require grad: "
                                 "UVs, taps and tangent frames under moving geometry are out of scope (detach the vertices, "
                                 "or use SpatialMaterials / MicrofacetMaterials)")
            pos = pos.detach()  # the view vector's dependence on the geometry is dropped: the shader's positions are constants
        S = self.rasterizer.raster_settings.image_size
        B = envmap.environment_map.shape[0]
        vis = None
        if self.shadows:  # the mask of the envmap's directions: one for a shared grid, one per image for per-image lists
            vis = self.rasterizer.visibility(meshes_world, R, T, _shared_grid(envmap.directions))
        if self.microfacet:
            m = self.materials
            if m.roughness.device != nrm.device:
                m.to(nrm.device)
            shade_nrm = nrm
            if not self.textured:
                values = m.values()
            else:
                values = m.values(self.rasterizer, meshes_world, R, T)
                if m.normal is not None:  # as below: the normal map bends the shading normals only
                    shade_nrm = m.shading_normals(self.rasterizer, meshes_world, R, T, nrm)
            colors = microfacet_shading_materials(shade_nrm, pos, self.camera_center, envmap, *values, vis=vis,
                                                  roughness_min=m.roughness_min, f0_dielectric=m.f0_dielectric)
        elif self.spatial:
            if self.materials.ks.device != nrm.device:
                self.materials.to(nrm.device)
            colors = blinn_phong_shading_materials(nrm, pos, self.camera_center, envmap, *self.materials.values(), vis=vis,
                                                   differentiable_normals=geometry)
        elif self.textured:
            if self.materials.ks.device != nrm.device:
                self.materials.to(nrm.device)
            shade_nrm = nrm
            if self.materials.normal is not None:  # a normal map bends the shading normals; shadows keep the geometry's mask
                shade_nrm = self.materials.shading_normals(self.rasterizer, meshes_world, R, T, nrm)
            colors = blinn_phong_shading_materials(shade_nrm, pos, self.camera_center, envmap,
                                                   *self.materials.values(self.rasterizer, meshes_world, R, T), vis=vis,
                                                   differentiable_normals=shade_nrm.requires_grad)
        elif geometry:  # the scalar shader through its terms: the fused kernel has no gradient with respect to the normals
            shininess = float(torch.as_tensor(self.materials.shininess).reshape(-1)[0])
            D, Sp = shade_terms_normals(nrm, pos, self.camera_center, envmap, shininess, vis=vis)
            colors = compose_materials(D, Sp, self.kd, self.ks, shininess)
        else:
            colors = blinn_phong_shading_gbuffer(nrm, pos, self.camera_center, envmap, self.materials.shininess, self.kd,
                                                 self.ks, vis=vis)
        normals = torch.nn.functional.normalize(nrm, p=2, dim=-1, eps=1e-6).reshape(1, S, S, 3).repeat(B, 1, 1, 1)
        return colors.reshape(B, S, S, 3), normals

    def shading_normals(self, meshes_world: Meshes, R=None, T=None) -> torch.Tensor:
        """The unit normals the shader uses, [S, S, 3]: the G-buffer's, bent by the materials' normal texture where there is
        one (``forward`` keeps returning the geometric ones)."""
        _, nrm, _ = self.rasterizer.gbuffer(meshes_world, R, T)
        S = self.rasterizer.raster_settings.image_size
        if self.textured and self.materials.normal is not None:
            if self.materials.normal.device != nrm.device:
                self.materials.to(nrm.device)
            nrm = self.materials.shading_normals(self.rasterizer, meshes_world, R, T, nrm)
        return torch.nn.functional.normalize(nrm, p=2, dim=-1, eps=1e-6).reshape(S, S, 3)


def unpack_visibility(vis: torch.Tensor, J: int) -> torch.Tensor:
    """The packed mask of ``MeshRasterizer.visibility`` / ``ops.mesh_visibility`` (int32 [NB, NP, ceil(J/32)], bit j & 31 of
    word j >> 5) as booleans [NB, NP, J].  Plain torch: works on any device."""
    if not isinstance(vis, torch.Tensor) or vis.dtype != torch.int32 or vis.dim() != 3:
        raise ValueError("vis must be an int32 tensor [NB, NP, JW]")
    J = int(J)
    if J < 1 or (J + 31) // 32 != vis.shape[2]:
        raise ValueError(f"{J} directions need {(J + 31) // 32} words per pixel, the mask has {vis.shape[2]}")
    shifts = torch.arange(32, dtype=torch.int32, device=vis.device)
    bits = (vis.unsqueeze(-1) >> shifts) & 1  # (an arithmetic shift: the sign bit's copies are masked off)
    return bits.reshape(vis.shape[0], vis.shape[1], -1)[:, :, :J].to(torch.bool)


def build_hip_renderer(obj_path, obj_rotation, img_size, kd, device, shadows: bool = False, materials=None):
    """Same arguments and return value as the reference's ``build_renderer`` (:177-217) -- ``(renderer, R, T, mesh)`` with
    ``renderer(meshes_world=mesh, R=R, T=T, envmap=...)`` -- without pytorch3d: Materials(shininess=500), ks = 1 - kd, the
    camera at look_at_view_transform(2, 0, 0).  ``device`` must be a GPU device (there is no CPU path).  ``shadows=True``:
    the mesh casts shadows on itself (``HipMeshRenderer(shadows=True)``); the default renders what the reference does.
    ``materials``: a ``SpatialMaterials`` of img_size x img_size pixels, or a ``TexturedMaterials`` (the OBJ's ``vt`` are then
    read, ``load_obj_uv``), or their microfacet siblings ``MicrofacetMaterials`` / ``TexturedMicrofacetMaterials``; kd is not
    used with any of them; None: Materials(shininess=500)."""
    textured = isinstance(materials, (TexturedMaterials, TexturedMicrofacetMaterials))
    if textured:
        verts, faces, vt, ft = load_obj_uv(obj_path)
        if vt.shape[0] < 1:
            raise ValueError(f"{obj_path} has no texture coordinates (vt lines): {type(materials).__name__} needs them")
    else:
        verts, faces = load_obj(obj_path)
    verts = rotate_axis_angle_y(verts, obj_rotation)
    if torch.device(device).type != "cuda":
        raise _lib.RENILibraryError(f"build_hip_renderer renders on a GPU device, got {device!r}; there is no CPU path")
    if textured:
        mesh = Meshes(verts=[verts.to(device)], faces=[faces.to(device)], verts_uvs=[vt.to(device)], faces_uvs=[ft.to(device)])
    else:
        mesh = Meshes(verts=[verts.to(device)], faces=[faces.to(device)])
    mesh.verts_normals_packed()
    cameras = FoVPerspectiveCameras(device=device)
    raster = MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(image_size=int(img_size)))
    if materials is not None and not isinstance(materials, (SpatialMaterials, TexturedMaterials, MicrofacetMaterials,
                                                            TexturedMicrofacetMaterials)):
        raise ValueError("materials must be a SpatialMaterials, a TexturedMaterials, a MicrofacetMaterials, a "
                         "TexturedMicrofacetMaterials or None")
    renderer = HipMeshRenderer(raster, kd=kd, materials=_Materials(500.0) if materials is None else materials.to(device),
                               shadows=shadows)
    R, T = look_at_view_transform(2.0, 0.0, 0.0, degrees=True, device=device)
    return renderer, R, T, mesh
