"""Materials that live on the surface: textures in the mesh's UV space, looked up per render pixel through the G-buffer.

A ``SpatialMaterials`` value belongs to one image; a texture belongs to the object, so several renders -- other cameras,
other lights -- read, and send their gradients into, one shared set of texels.  The lookup is the HIP library's
(include/reni_hip.h, "UV-space textures"): ``MeshRasterizer.texture_taps`` turns the cached G-buffer into 8 (element,
weight) pairs per pixel once per (scene, texture size); a training step then costs the pyramid, the fetch and their
transposes.  Only the texture carries a gradient: UVs, footprints, levels, the mesh and the camera are constants.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops

# index int32 [P, 8], weight [P, 8]: the fetch's taps; order [8 P], offsets [E + 1]: the table its transpose gathers through;
# levels, height, width: the pyramid they address, elements = sum H_l W_l
Taps = namedtuple("Taps", ["index", "weight", "order", "offsets", "levels", "height", "width", "elements"])


def make_taps(uv, size, levels=None, jac=None, pix_valid=None, wrap: str = "clamp", align_corners: bool = False,
              lod_bias: float = 0.0) -> Taps:
    """The taps of a lookup at uv [P, 2] (any uv, not only a mesh's) into a texture of ``size`` = (H, W): ``ops.texture_taps``
    and ``ops.texture_table`` in one record.  ``MeshRasterizer.texture_taps`` calls this on the pixel UVs and caches it."""
    if isinstance(lod_bias, torch.Tensor):
        if lod_bias.requires_grad:
            raise ValueError("lod_bias is a constant of the lookup and must not require grad (only the texture carries a gradient)")
        lod_bias = float(lod_bias)
    H0, W0 = (int(x) for x in size)
    L, E, _ = ops.texture_levels(H0, W0, levels)
    idx, wgt = ops.texture_taps(uv, (H0, W0), L, jac=jac, pix_valid=pix_valid, wrap=wrap, align_corners=align_corners,
                                lod_bias=lod_bias)
    order, offsets = ops.texture_table(idx, E, wgt)
    return Taps(idx, wgt, order, offsets, L, H0, W0, E)


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, taps):
        H0, W0, C = texture.shape
        buf = torch.empty(taps.elements, C, dtype=torch.float32, device=texture.device)
        buf[: H0 * W0] = texture.reshape(H0 * W0, C)
        ops.texture_pyramid(buf, taps.levels, H0, W0)
        ctx.taps, ctx.shape = taps, (H0, W0, C)
        return ops.texture_fetch(buf, taps.index, taps.weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        taps, (H0, W0, C) = ctx.taps, ctx.shape
        g = ops.texture_fetch_backward(grad_out, taps.weight, (taps.order, taps.offsets), taps.elements)
        ops.texture_pyramid_backward(g, taps.levels, H0, W0)
        return g[: H0 * W0].reshape(H0, W0, C).clone(), None  # (a copy: a view would keep the whole [E, C] buffer alive)


def sample(texture: torch.Tensor, taps: Taps) -> torch.Tensor:
    """texture [H, W, C] (or [H, W]: one channel) looked up through ``taps`` -> [P, C] (or [P]): the pyramid is rebuilt from
    the texture (box rule), then fetched trilinearly.  Differentiable with respect to the texture; the gradient reaches
    level 0 through the pyramid's transpose.  Deterministic, forward and backward."""
    if not isinstance(taps, Taps):
        raise ValueError("taps must be a textures.Taps (MeshRasterizer.texture_taps or textures.make_taps)")
    if not isinstance(texture, torch.Tensor) or texture.dim() not in (2, 3):
        raise ValueError("texture must be a tensor [H, W, C] or [H, W]")
    flat = texture.dim() == 2
    t = texture.unsqueeze(-1) if flat else texture
    if tuple(t.shape[:2]) != (taps.height, taps.width):
        raise ValueError(f"the taps address a {taps.height} x {taps.width} texture, got {tuple(t.shape[:2])}")
    if not 1 <= t.shape[2] <= 8:
        raise ValueError(f"a texture has 1..8 channels, got {t.shape[2]}")
    if t.dtype != torch.float32:
        raise ValueError("texture must be float32")
    ops._require_cuda(t, taps.index)
    if t.device != taps.index.device:
        raise ValueError(f"the texture is on {t.device}, its taps on {taps.index.device}")
    out = _SampleFn.apply(t.contiguous(), taps)
    return out[:, 0] if flat else out


def tangent_frames(verts, faces, verts_uvs, faces_uvs, pix_valid, pixel_normals):
    """A tangent frame per pixel -> (tangent [P, 3], bitangent [P, 3], valid [P] bool) from the pixel's face (``pix_valid``
    of ``MeshRasterizer.pixel_uv``: the face, or -1) and its G-buffer normal.  Per face, with world vertices p0..p2 and UVs
    (u, v)0..2: e1 = p1 - p0, e2 = p2 - p0, det = du1 dv2 - du2 dv1, T_f = (e1 dv2 - e2 dv1) / det (the direction of growing
    u), B_f = (e2 du1 - e1 du2) / det (of growing v).  Per pixel, with N the normalised pixel normal: t = normalize(T_f -
    N (N.T_f)), b = h (N x t) with h = sign((N x t).B_f) (-1 on a face whose UVs are mirrored).  Invalid -- pix_valid < 0,
    det zero or not finite, |T_f - N (N.T_f)| < 1e-12, h = 0 -- gives t = b = 0.  Plain torch, gathers only (no scatter):
    deterministic, on any device, in the dtype of ``verts``."""
    seen = pix_valid >= 0
    face = pix_valid.clamp(min=0)
    p = verts[faces[face]]                                              # [P, 3, 3]
    uv = verts_uvs[faces_uvs[face].clamp(0, verts_uvs.shape[0] - 1)]    # (a face named by pix_valid has its three UVs)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    du1, dv1 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1]
    du2, dv2 = uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    ok = seen & torch.isfinite(det) & (det != 0)
    sdet = torch.where(ok, det, torch.ones_like(det))[:, None]
    Tf = (e1 * dv2[:, None] - e2 * dv1[:, None]) / sdet
    Bf = (e2 * du1[:, None] - e1 * du2[:, None]) / sdet
    N = torch.nn.functional.normalize(pixel_normals.to(verts.dtype), p=2, dim=-1, eps=1e-6)
    tp = Tf - N * (N * Tf).sum(-1, keepdim=True)
    ln = tp.norm(dim=-1)
    ok = ok & torch.isfinite(ln) & (ln >= 1e-12)
    t = tp / torch.where(ok, ln, torch.ones_like(ln))[:, None]
    c = torch.cross(N, t, dim=-1)
    h = torch.sign((c * Bf).sum(-1))
    ok = ok & torch.isfinite(h) & (h != 0)
    zero = torch.zeros_like(t)
    return torch.where(ok[:, None], t, zero), torch.where(ok[:, None], h[:, None] * c, zero), ok


def perturb_normals(pixel_normals, tangent, bitangent, valid, m, strength: float = 1.0):
    """Shading normals [P, 3] from a tangent-space normal m = 2 texel - 1 per pixel ([P, 3]; (0, 0, 1) is "flat"): on a
    valid pixel the direction strength m_x t + strength m_y b + m_z N (N the normalised pixel normal), returned with the
    length of the pixel's own normal, |n_p| (strength m_x t + strength m_y b) + m_z n_p -- not normalised, the shader does
    that -- so that a flat m returns ``pixel_normals`` bit for bit.  An invalid or background pixel keeps its normal exactly
    and sends no gradient to m.  Plain torch with autograd (any device, any float dtype)."""
    if pixel_normals.dim() != 2 or pixel_normals.shape[1] != 3:
        raise ValueError("pixel_normals must be [P, 3]")
    P = pixel_normals.shape[0]
    for name, x in (("tangent", tangent), ("bitangent", bitangent), ("m", m)):
        if tuple(x.shape) != (P, 3):
            raise ValueError(f"{name} must be [{P}, 3] like pixel_normals, got {tuple(x.shape)}")
    if tuple(valid.shape) != (P,) or valid.dtype != torch.bool:
        raise ValueError(f"valid must be a bool tensor [{P}], got {valid.dtype} {tuple(valid.shape)}")
    ln = pixel_normals.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    bent = ln * ((float(strength) * m[:, 0:1]) * tangent + (float(strength) * m[:, 1:2]) * bitangent) + m[:, 2:3] * pixel_normals
    return torch.where(valid[:, None], bent, pixel_normals)


class _UVMaterials(nn.Module):
    """What the materials in UV space share: the lookup options, the registration of scalars and textures (the names in
    ``learn`` as Parameters, the others as buffers), the fetch through the rasteriser's cached taps and the optional normal
    texture.  A subclass names its inputs in ``NAMES``; the first is the colour (a float, [3] or [H, W, 3]), the others are
    scalars (a float or [H, W])."""

    NAMES = ()

    def _register(self, given, learn, levels, wrap, align_corners, lod_bias, normal, normal_strength):
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for name in learn:
            if name not in self.NAMES + ("normal",):
                raise ValueError(f"learn names must be among {self.NAMES + ('normal',)}, got {name!r}")
        if "normal" in learn and normal is None:
            raise ValueError('learn names "normal", but no normal texture is given')
        self.normal_strength = float(normal_strength)
        if wrap not in ("clamp", "repeat"):
            raise ValueError(f'wrap must be "clamp" or "repeat", got {wrap!r}')
        self.levels = None if levels is None else int(levels)
        self.wrap, self.align_corners, self.lod_bias = wrap, bool(align_corners), float(lod_bias)
        vals = {}
        for name, x in zip(self.NAMES, given):
            x = torch.as_tensor(x, dtype=torch.float32).detach().clone()
            if name == self.NAMES[0]:
                if not (x.dim() == 0 or tuple(x.shape) == (3,) or (x.dim() == 3 and x.shape[2] == 3 and min(x.shape[:2]) >= 1)):
                    raise ValueError(f"{name} must be a float, [3] or a texture [H, W, 3], got {tuple(x.shape)}")
            elif not (x.dim() == 0 or (x.dim() == 2 and min(x.shape) >= 1)):
                raise ValueError(f"{name} must be a float or a texture [H, W], got {tuple(x.shape)}")
            vals[name] = x
        if normal is not None:
            x = torch.as_tensor(normal, dtype=torch.float32).detach().clone()
            if not (x.dim() == 3 and x.shape[2] == 3 and min(x.shape[:2]) >= 1):
                raise ValueError(f"normal must be a texture [H, W, 3], got {tuple(x.shape)}")
            vals["normal"] = x
        else:
            self.normal = None
        for name, x in vals.items():
            if self.is_texture(x):  # the same argument errors as a lookup would raise, now
                L = ops.texture_levels(x.shape[0], x.shape[1], self.levels)[0]
                if self.align_corners and (L > 1 or wrap != "clamp"):
                    raise ValueError(f'align_corners=True needs levels=1 and wrap="clamp" ({name} would have {L} levels)')
            if name in learn:
                setattr(self, name, nn.Parameter(x))
            else:
                self.register_buffer(name, x)

    @staticmethod
    def is_texture(x: torch.Tensor) -> bool:
        return x.dim() >= 2

    def _taps(self, x, rasterizer, mesh, R, T):
        return rasterizer.texture_taps(mesh, R, T, size=tuple(x.shape[:2]), levels=self.levels, wrap=self.wrap,
                                       align_corners=self.align_corners, lod_bias=self.lod_bias)

    def _fetched(self, rasterizer, mesh, R=None, T=None):
        """The inputs of ``NAMES`` per pixel (a texture: fetched through its taps) or as they are (a scalar)."""
        out = []
        for name in self.NAMES:
            x = getattr(self, name)
            out.append(sample(x, self._taps(x, rasterizer, mesh, R, T)) if self.is_texture(x) else x)
        return out

    def shading_normals(self, rasterizer, mesh, R=None, T=None, pixel_normals=None):
        """The normals the shader is to use, [P, 3] (not normalised): ``pixel_normals`` (the G-buffer's) bent by the normal
        texture in the pixel's tangent frame; ``pixel_normals`` itself when there is no normal texture;
        a flat texture gives the input normals exactly (``tangent_space_normals``, ``perturb_normals``)."""
        if pixel_normals is None:
            pixel_normals = rasterizer.gbuffer(mesh, R, T)[1]
        if self.normal is None:
            return pixel_normals
        t, b, valid = rasterizer.pixel_tangents(mesh, R, T)
        return perturb_normals(pixel_normals, t, b, valid, self.tangent_space_normals(rasterizer, mesh, R, T), self.normal_strength)

    def tangent_space_normals(self, rasterizer, mesh, R=None, T=None):
        """m = 2 texel - 1 per pixel, [P, 3]: the normal texture fetched through the pixel's taps and decoded.  What is
        fetched is the texture's difference from flat, m = 2 fetch(normal - (0.5, 0.5, 1)) + (0, 0, 1): the same value up to
        the rounding of the weights' sum, and exactly (0, 0, 1) for a flat texture and on a pixel that sees no texture."""
        if self.normal is None:
            raise ValueError("these materials have no normal texture")
        flat = self.normal.new_tensor([0.5, 0.5, 1.0])
        return 2.0 * sample(self.normal - flat, self._taps(self.normal, rasterizer, mesh, R, T)) + self.normal.new_tensor([0.0, 0.0, 1.0])


class TexturedMaterials(_UVMaterials):
    """A Blinn-Phong material in the mesh's UV space.  Each of albedo, ks and shininess is a scalar (albedo: or [3]) or a
    texture -- [H, W, 3] for the albedo, [H, W] for the other two; the sizes may differ.  The names in ``learn`` become
    Parameters (the caller owns their optimiser), the others buffers.  ``levels=None``: the full pyramid of each texture
    (one level where its size is no power of two).  ``values(rasterizer, mesh, R, T)`` -> the per-pixel (albedo [P, 3], ks
    [P], shininess [P]) -- or the scalars -- that ``blinn_phong_shading_materials`` takes; the shininess is clamped to
    [shininess_min, shininess_max] AFTER the fetch (a background pixel fetches 0 and is clamped too: it is never shaded).

    ``normal``: a tangent-space normal texture [H, W, 3] encoded in [0, 1] (flat: (0.5, 0.5, 1)), with its own size and
    pyramid; "normal" may be named in ``learn``.  ``shading_normals(rasterizer, mesh, R, T, pixel_normals)`` bends the
    G-buffer's normals by it (``perturb_normals`` with ``normal_strength``); ``values`` and ``NAMES`` do not know it, and
    with ``normal=None`` nothing of it runs.

    One object handed to several renderers, each with its own rasteriser and camera, accumulates one texture gradient."""

    NAMES = ("albedo", "ks", "shininess")

    def __init__(self, albedo=1.0, ks=0.0, shininess=500.0, learn=(), levels=None, wrap: str = "clamp", align_corners: bool = False,
                 lod_bias: float = 0.0, shininess_min: float = 1.0, shininess_max: float = 2000.0, normal=None,
                 normal_strength: float = 1.0):
        super().__init__()
        if not 0.0 < float(shininess_min) <= float(shininess_max):
            raise ValueError("0 < shininess_min <= shininess_max is required")
        self.shininess_min, self.shininess_max = float(shininess_min), float(shininess_max)
        self._register((albedo, ks, shininess), learn, levels, wrap, align_corners, lod_bias, normal, normal_strength)

    def values(self, rasterizer, mesh, R=None, T=None):
        out = self._fetched(rasterizer, mesh, R, T)
        return out[0], out[1], out[2].clamp(self.shininess_min, self.shininess_max)


class TexturedMicrofacetMaterials(_UVMaterials):
    """A base-colour / roughness / metallic material in the mesh's UV space (``envmap_shader.MicrofacetMaterials`` is its
    per-render-pixel sibling).  base_color: a float, [3] or a texture [H, W, 3]; roughness and metallic: a float or a texture
    [H, W]; the sizes may differ.  ``learn``, ``levels``, ``wrap``, ``align_corners``, ``lod_bias``, ``normal`` and
    ``normal_strength`` are ``TexturedMaterials``'.  ``values(rasterizer, mesh, R, T)`` -> the per-pixel (base_color [P, 3],
    roughness [P], metallic [P]) -- or the scalars -- that ``microfacet_shading_materials`` takes; AFTER the fetch the
    roughness is clamped to [roughness_min, 1] (a background pixel fetches 0 and is clamped too: it is never shaded) and the
    metallic to [0, 1].

    One object handed to several renderers, each with its own rasteriser and camera, accumulates one texture gradient."""

    NAMES = ("base_color", "roughness", "metallic")

    def __init__(self, base_color=0.8, roughness=0.5, metallic=0.0, learn=(), levels=None, wrap: str = "clamp",
                 align_corners: bool = False, lod_bias: float = 0.0, roughness_min: float = 0.1, f0_dielectric: float = 0.04,
                 normal=None, normal_strength: float = 1.0):
        super().__init__()
        if not 0.0 < float(roughness_min) <= 1.0:
            raise ValueError("0 < roughness_min <= 1 is required")
        self.roughness_min, self.f0_dielectric = float(roughness_min), float(f0_dielectric)
        self._register((base_color, roughness, metallic), learn, levels, wrap, align_corners, lod_bias, normal, normal_strength)

    def values(self, rasterizer, mesh, R=None, T=None):
        out = self._fetched(rasterizer, mesh, R, T)
        return out[0], out[1].clamp(self.roughness_min, 1.0), out[2].clamp(0.0, 1.0)
