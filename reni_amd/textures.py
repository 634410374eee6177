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


class TexturedMaterials(nn.Module):
    """A Blinn-Phong material in the mesh's UV space.  Each of albedo, ks and shininess is a scalar (albedo: or [3]) or a
    texture -- [H, W, 3] for the albedo, [H, W] for the other two; the sizes may differ.  The names in ``learn`` become
    Parameters (the caller owns their optimiser), the others buffers.  ``levels=None``: the full pyramid of each texture
    (one level where its size is no power of two).  ``values(rasterizer, mesh, R, T)`` -> the per-pixel (albedo [P, 3], ks
    [P], shininess [P]) -- or the scalars -- that ``blinn_phong_shading_materials`` takes; the shininess is clamped to
    [shininess_min, shininess_max] AFTER the fetch (a background pixel fetches 0 and is clamped too: it is never shaded).

    One object handed to several renderers, each with its own rasteriser and camera, accumulates one texture gradient."""

    NAMES = ("albedo", "ks", "shininess")

    def __init__(self, albedo=1.0, ks=0.0, shininess=500.0, learn=(), levels=None, wrap: str = "clamp", align_corners: bool = False,
                 lod_bias: float = 0.0, shininess_min: float = 1.0, shininess_max: float = 2000.0):
        super().__init__()
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for name in learn:
            if name not in self.NAMES:
                raise ValueError(f"learn names must be among {self.NAMES}, got {name!r}")
        if not 0.0 < float(shininess_min) <= float(shininess_max):
            raise ValueError("0 < shininess_min <= shininess_max is required")
        if wrap not in ("clamp", "repeat"):
            raise ValueError(f'wrap must be "clamp" or "repeat", got {wrap!r}')
        self.shininess_min, self.shininess_max = float(shininess_min), float(shininess_max)
        self.levels = None if levels is None else int(levels)
        self.wrap, self.align_corners, self.lod_bias = wrap, bool(align_corners), float(lod_bias)
        vals = {}
        a = torch.as_tensor(albedo, dtype=torch.float32).detach().clone()
        if not (a.dim() == 0 or tuple(a.shape) == (3,) or (a.dim() == 3 and a.shape[2] == 3 and min(a.shape[:2]) >= 1)):
            raise ValueError(f"albedo must be a float, [3] or a texture [H, W, 3], got {tuple(a.shape)}")
        vals["albedo"] = a
        for name, x in (("ks", ks), ("shininess", shininess)):
            x = torch.as_tensor(x, dtype=torch.float32).detach().clone()
            if not (x.dim() == 0 or (x.dim() == 2 and min(x.shape) >= 1)):
                raise ValueError(f"{name} must be a float or a texture [H, W], got {tuple(x.shape)}")
            vals[name] = x
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

    def values(self, rasterizer, mesh, R=None, T=None):
        out = []
        for name in self.NAMES:
            x = getattr(self, name)
            if self.is_texture(x):
                taps = rasterizer.texture_taps(mesh, R, T, size=tuple(x.shape[:2]), levels=self.levels, wrap=self.wrap,
                                               align_corners=self.align_corners, lod_bias=self.lod_bias)
                x = sample(x, taps)
            out.append(x)
        return out[0], out[1], out[2].clamp(self.shininess_min, self.shininess_max)
