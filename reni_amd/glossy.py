"""Environment maps as glossy lighting: maps convolved with zonal specular lobes (one map per lobe, a chain over roughness),
looked up at arbitrary directions, and what follows from the two -- the SH-domain counterpart, a prefiltered stand-in for the
Blinn-Phong shader, and the ``glossy_psnr`` columns of ``metrics.evaluate``.

The arithmetic runs in libreni_hip.so (``reni_lobe_convolve``, ``reni_envmap_lookup``: include/reni_hip.h); there is no CPU
fallback, a CPU tensor raises ``RENILibraryError``.  ``lobe_band_scale`` is host float64.

A lobe is a function f(t) of t = o . d, the cosine between an output direction and a texel.  With tc = clamp(t, 0, 1) and
m = clamp((1 + t) / 2, 0, 1):

    phong(n)        f = tc^n
    blinn(s)        f = m^(s / 2): the shader's (n . h)^s for view = normal, since with h = normalize(n + l),
                    (n . h)^2 = (1 + n . l) / 2
    ggx(roughness)  f = tc a^2 / (m (a^2 - 1) + 1)^2 with a = roughness^2: D(h) (n . l) of the split-sum prefilter under
                    n = v = r, without 1 / pi

phong(1) and ggx(1) are the clamped cosine of ``baselines.diffuse_convolve``.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import ops
from .baselines import _diffuse_device_tables, reni_grid_weights, sh_lmax_from_terms, sh_reconstruct, shTerms, l_from_idx


class Lobe(NamedTuple):
    kind: str     # "phong" | "blinn" | "ggx" (_lib.LOBE_KIND)
    param: float  # n, s, a = roughness^2


def phong(n: float) -> Lobe:
    if not float(n) > 0:
        raise ValueError(f"phong needs an exponent > 0, got {n}")
    return Lobe("phong", float(n))


def blinn(s: float) -> Lobe:
    if not float(s) > 0:
        raise ValueError(f"blinn needs a shininess > 0, got {s}")
    return Lobe("blinn", float(s))


def ggx(roughness: float) -> Lobe:
    if not 0 < float(roughness) <= 1:
        raise ValueError(f"ggx needs 0 < roughness <= 1, got {roughness}")
    return Lobe("ggx", float(roughness) ** 2)


def _lobes(lobes) -> Sequence[Lobe]:
    lobes = [lobes] if isinstance(lobes, Lobe) else list(lobes)
    if not 1 <= len(lobes) <= 16 or not all(isinstance(l, Lobe) for l in lobes):
        raise ValueError("lobes must be 1..16 of phong(n), blinn(s), ggx(roughness)")
    return lobes


def lobe_value(lobe: Lobe, t):
    """f(t) in float64 on the host (the definition the kernel is tested against)."""
    t = np.asarray(t, np.float64)
    tc, m = np.clip(t, 0.0, 1.0), np.clip((1.0 + t) / 2.0, 0.0, 1.0)
    if lobe.kind == "phong":
        return tc ** lobe.param
    if lobe.kind == "blinn":
        return m ** (lobe.param / 2.0)
    if lobe.kind == "ggx":
        a2 = lobe.param * lobe.param
        return tc * a2 / (m * (a2 - 1.0) + 1.0) ** 2
    raise ValueError(f"unknown lobe kind {lobe.kind!r}")


def _constant(**tensors):
    """Directions, weights and levels are constants of these operators, as mesh and camera are of the shader: one that asks for
    a gradient gets an error, not silence."""
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{name} requires grad, but glossy lighting is differentiable with respect to the maps only: "
                             f"{name} is a constant here (detach it)")


def _wants_grad(t) -> bool:
    return torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad


class _LobeConvolveFn(torch.autograd.Function):
    """``ops.lobe_convolve`` with its transpose ``ops.lobe_convolve_backward`` behind it.  den: the cached denominators of
    these operands, or None -- they are then computed in backward, and only there."""

    @staticmethod
    def forward(ctx, src, in_dirs, in_weight, out_dirs, kinds, params, normalise, scale, den):
        ctx.save_for_backward(in_dirs, in_weight, out_dirs, *(() if den is None else (den,)))
        ctx.consts = (kinds, params, bool(normalise), float(scale))
        ctx.planar = not (src.shape[1] == in_dirs.shape[0] and src.shape[2] == 3)  # (ops._convolve_args' reading of src)
        return ops.lobe_convolve(src, in_dirs, in_weight, out_dirs, kinds, params, normalise, scale)

    @staticmethod
    def backward(ctx, grad_out):
        in_dirs, in_weight, out_dirs, *den = ctx.saved_tensors
        kinds, params, normalise, scale = ctx.consts
        g = ops.lobe_convolve_backward(grad_out, in_dirs, in_weight, out_dirs, kinds, params, normalise, scale,
                                       den=den[0] if den else None, planar=ctx.planar)
        return g, None, None, None, None, None, None, None, None


class _LookupFn(torch.autograd.Function):
    """``ops.envmap_lookup`` with its transpose ``ops.envmap_lookup_backward`` behind it; the tap table is built in backward."""

    @staticmethod
    def forward(ctx, maps, dirs, level):
        ctx.save_for_backward(dirs, *((level,) if isinstance(level, torch.Tensor) else ()))
        ctx.level = None if isinstance(level, torch.Tensor) else level
        ctx.shape = tuple(maps.shape)
        return ops.envmap_lookup(maps, dirs, level)

    @staticmethod
    def backward(ctx, grad_out):
        dirs, *level = ctx.saved_tensors
        Lv, H, W = (1,) + ctx.shape[1:3] if len(ctx.shape) == 4 else ctx.shape[1:4]
        g = ops.envmap_lookup_backward(grad_out, Lv, H, W, dirs, level[0] if level else ctx.level)
        return g.view(ctx.shape), None, None


def _lobe_convolve(src, in_dirs, in_weight, out_dirs, lobes, normalise, scale, den=None):
    """den: None, or a function that returns the cached denominators (called only when src requires grad)"""
    lobes = _lobes(lobes)
    kinds, params = [l.kind for l in lobes], [l.param for l in lobes]
    _constant(in_dirs=in_dirs, in_weight=in_weight, out_dirs=out_dirs)
    if not _wants_grad(src):
        return ops.lobe_convolve(src, in_dirs, in_weight, out_dirs, kinds, params, normalise, scale)
    ops._require_cuda(src, in_dirs, in_weight, out_dirs)
    if src.dtype != torch.float32:
        src = src.float()
    return _LobeConvolveFn.apply(src, in_dirs, in_weight, out_dirs, kinds, params, normalise, scale,
                                 den() if den is not None and normalise else None)


def lobe_convolve(src, in_dirs, in_weight, out_dirs, lobes, normalise: bool = True, scale: float = 1.0) -> torch.Tensor:
    """out[n, l, o, c] = sum_i f_l(out_dirs[o] . in_dirs[i]) in_weight[i] src[n, i, c], divided by sum_i f_l in_weight[i]
    when normalise (0 where no texel lies in the lobe), else times scale.  src [N, Q, 3] or planar [N, 3, Q] (any strides);
    in_dirs [Q, 3], in_weight [Q], out_dirs [P, 3] -> [N, Lv, P, 3] float32.  Deterministic: a map's bits do not depend on
    the batch, a lobe's not on the other lobes of the call.

    Differentiable with respect to src (the transposed convolution, ``ops.lobe_convolve_backward``; the denominators of a
    normalised call are computed in backward).  Directions, weights and lobes are constants: one that requires grad raises."""
    return _lobe_convolve(src, in_dirs, in_weight, out_dirs, lobes, normalise, scale)


def _grid_width(envmaps):
    if envmaps.dim() == 4 and envmaps.shape[3] == 3 and 2 * envmaps.shape[1] == envmaps.shape[2]:
        return int(envmaps.shape[2])
    if envmaps.dim() == 3 and envmaps.shape[2] == 3:
        W = int(round(math.sqrt(2 * envmaps.shape[1])))
        if W * (W // 2) != envmaps.shape[1] or W % 2:
            raise ValueError(f"[N, H W, 3] maps need H W = W^2 / 2 for an even W, got {envmaps.shape[1]} pixels")
        return W
    raise ValueError(f"envmaps must be [N, H W, 3] or [N, W/2, W, 3], got {tuple(envmaps.shape)}")


def prefilter(envmaps: torch.Tensor, lobes, out_width=None) -> torch.Tensor:
    """The normalised convolution of maps on RENI's own grid (``utils.get_directions``, texels weighted by their exact band
    solid angles) with each lobe: envmaps [N, H W, 3] or [N, H, W, 3] on the GPU -> [N, Lv, Ho Wo, 3] or [N, Lv, Ho, Wo, 3]
    at out_width (default: the input width).  A constant map stays that constant under every lobe.  Differentiable with
    respect to envmaps; the denominators the backward needs are cached with the grids, per (width, out_width, lobes)."""
    from .utils import get_directions
    W = _grid_width(envmaps)
    Wo = W if out_width is None else int(out_width)
    if Wo < 2 or Wo % 2:
        raise ValueError(f"out_width must be even and >= 2, got {out_width}")
    ops._require_cuda(envmaps)
    src = envmaps.reshape(envmaps.shape[0], -1, 3)
    dirs, w = _diffuse_device_tables(("reni", W), lambda: (get_directions(W)[0], reni_grid_weights(W)), envmaps.device)
    (odirs,) = _diffuse_device_tables(("reni_out", Wo), lambda: (get_directions(Wo)[0],), envmaps.device)
    lobes = _lobes(lobes)

    def den():  # kept with the grids: a fit loop pays for the denominators once
        return _diffuse_device_tables(("reni_den", W, Wo) + tuple(lobes), lambda: (ops.lobe_denominators(
            dirs, w, odirs, [l.kind for l in lobes], [l.param for l in lobes]),), envmaps.device)[0]

    out = _lobe_convolve(src, dirs, w, odirs, lobes, True, 1.0, den)
    return out.view(out.shape[0], out.shape[1], Wo // 2, Wo, 3) if envmaps.dim() == 4 else out


def lookup(maps_or_chain: torch.Tensor, dirs: torch.Tensor, level=None) -> torch.Tensor:
    """Maps [N, H, W, 3] or chains [N, Lv, H, W, 3] on RENI's grid, sampled bilinearly on the sphere at dirs [P, 3] (shared)
    or [N, P, 3] (per map; no unit length needed, a zero vector gives a finite value) -> [N, P, 3].  level: None, a number, or
    a float tensor [P] / [N, P], clamped to [0, Lv - 1]; the result mixes the two nearest levels linearly.

    Differentiable with respect to the maps (``ops.envmap_lookup_backward``: a deterministic gather per texel, its table built
    in backward).  dirs and level are constants: one that requires grad raises."""
    _constant(dirs=dirs, level=level)
    if not _wants_grad(maps_or_chain):
        return ops.envmap_lookup(maps_or_chain, dirs, level)
    ops._require_cuda(maps_or_chain, dirs)
    maps = maps_or_chain if maps_or_chain.dtype == torch.float32 else maps_or_chain.float()
    if maps.dim() not in (4, 5):
        raise ValueError(f"maps must be [N, H, W, 3] or [N, Lv, H, W, 3], got {tuple(maps.shape)}")
    return _LookupFn.apply(maps, dirs, level)


# ------------------------------------------------------------------------------------------ SH domain
def _legendre_all(lmax, t):
    P = np.zeros((lmax + 1,) + t.shape)
    P[0] = 1.0
    if lmax >= 1:
        P[1] = t
    for l in range(2, lmax + 1):
        P[l] = ((2 * l - 1) * t * P[l - 1] - (l - 1) * P[l - 2]) / l
    return P


_GL = np.polynomial.legendre.leggauss(64)


def lobe_band_scale(lobe: Lobe, lmax: int) -> np.ndarray:
    """Funk-Hecke factors of the NORMALISED lobe, float64 [lmax + 1]: Lambda_l = int f(t) P_l(t) dt / int f(t) dt over
    [-1, 1], so that the prefiltered map of sum c_lm Y_lm is sum Lambda_l c_lm Y_lm.  Composite Gauss-Legendre (64 nodes a
    panel), split at t = 0 where the clamp has its kink, with panels halving towards t = 1 where a sharp lobe lives."""
    lmax = int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax must be >= 0, got {lmax}")
    edges = [-1.0, -0.5, 0.0] + [1.0 - 2.0 ** -k for k in range(1, 48)] + [1.0]
    x, w = _GL
    num, den = np.zeros(lmax + 1), 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        t = 0.5 * (b - a) * x + 0.5 * (b + a)
        fw = lobe_value(lobe, t) * w * (0.5 * (b - a))
        num += _legendre_all(lmax, t) @ fw
        den += fw.sum()
    return num / den


def sh_glossy(coeffs: torch.Tensor, lobe: Lobe, width: int) -> torch.Tensor:
    """The prefiltered map of SH coefficients [N, T, 3] (T a square) under one lobe, [N, width / 2, width, 3] on the SH
    grid of ``baselines.sh_reconstruct``: the reconstruction of the coefficients scaled by ``lobe_band_scale`` -- the glossy
    twin of ``baselines.sh_irradiance``'s general branch."""
    if coeffs.dim() != 3 or coeffs.shape[2] != 3:
        raise ValueError(f"coeffs must be [N, T, 3], got {tuple(coeffs.shape)}")
    if not isinstance(lobe, Lobe):
        raise ValueError("lobe must be one of phong(n), blinn(s), ggx(roughness)")
    lmax = sh_lmax_from_terms(coeffs.shape[1])
    if shTerms(lmax) != coeffs.shape[1]:
        raise ValueError(f"the number of SH terms must be a square, got {coeffs.shape[1]}")
    ops._require_cuda(coeffs)
    lam = lobe_band_scale(lobe, lmax)
    (band,) = _diffuse_device_tables(("lobe_band", lobe.kind, lobe.param, lmax),
                                     lambda: (np.asarray([lam[l_from_idx(t)] for t in range(shTerms(lmax))]),), coeffs.device)
    return sh_reconstruct(coeffs * band.view(1, -1, 1), int(width))


# ------------------------------------------------------------------------------------------ shading from a chain
def blinn_phong_norm(shininess: float) -> float:
    """The shader's specular normalisation (s + 2) / (4 (2 - exp(-s / 2)))."""
    s = float(shininess)
    return (s + 2.0) / (4.0 * (2.0 - math.exp(-s / 2.0)))


def shading_dirs(normals: torch.Tensor, positions: torch.Tensor, camera_center):
    """(n, r, mask): unit normals [NP, 3], the view direction mirrored at them r = 2 (n . v) n - v with
    v = normalize(camera - position), and mask [NP, 1] = 1 where the normal is not zero (0: background)."""
    cam = torch.as_tensor(camera_center, dtype=torch.float32).reshape(-1)[:3].to(normals.device)
    n = torch.nn.functional.normalize(normals.float(), p=2, dim=-1, eps=1e-6)
    v = torch.nn.functional.normalize(cam[None] - positions.float(), p=2, dim=-1, eps=1e-6)
    r = 2.0 * (n * v).sum(-1, keepdim=True) * n - v
    mask = (normals != 0).any(-1, keepdim=True).float()
    return n, r, mask


def shade_prefiltered(envmap, normals, positions, camera_center, shininess, kd, ks, out_width: int) -> torch.Tensor:
    """Blinn-Phong colours [B, NP, 3] of a G-buffer (interpolated normals / positions [NP, 3], not normalised) FROM A
    PREFILTERED CHAIN instead of the per-pixel sum over texels of ``ops.envmap_shade``.

    One unnormalised two-lobe call ``[phong(1), blinn(shininess)]`` with weight 1 (``EnvironmentMap.environment_map`` is
    already multiplied by the sine weight) makes a chain [B, 2, out_width / 2, out_width, 3] on RENI's grid; the diffuse term
    is its level 0 looked up at the pixel's normal, the specular term its level 1 looked up at the view direction mirrored at
    the normal; they are combined with the shader's kd, ks and (s + 2) / (4 (2 - exp(-s / 2))).  Background pixels (a zero
    normal) are 0.

    What it is: the diffuse term is the shader's own sum up to the bilinear lookup on the out_width grid; the specular term
    uses the n = v = r approximation (the lobe around the mirrored direction as if the surface were seen along its normal),
    so it differs from the shader at grazing angles whatever out_width is.  It is cheaper than ``ops.envmap_shade`` only when
    the chain is reused across views or meshes, or when out_width^2 / 2 is small against the number of pixels.

    Differentiable with respect to ``envmap.environment_map`` through ``lobe_convolve`` and ``lookup``: the backward costs
    one transposed two-lobe convolution and two gathers, not pixels x texels."""
    from .envmap_shader import _shared_grid
    from .utils import get_directions
    Wo = int(out_width)
    if Wo < 2 or Wo % 2:
        raise ValueError(f"out_width must be even and >= 2, got {out_width}")
    colors = envmap.environment_map
    ops._require_cuda(colors, normals, positions)
    grid = _shared_grid(envmap.directions)
    if grid.dim() != 2:
        raise ValueError("shade_prefiltered needs one texel grid shared by the batch")
    dev = colors.device
    (odirs,) = _diffuse_device_tables(("reni_out", Wo), lambda: (get_directions(Wo)[0],), dev)
    ones = torch.ones(grid.shape[0], dtype=torch.float32, device=dev)
    s = float(torch.as_tensor(shininess).reshape(-1)[0])
    chain = lobe_convolve(colors, grid, ones, odirs, [phong(1.0), blinn(s)], normalise=False)
    chain = chain.view(colors.shape[0], 2, Wo // 2, Wo, 3)
    n, r, mask = shading_dirs(normals, positions, camera_center)
    diffuse = lookup(chain, n, 0.0)
    specular = lookup(chain, r, 1.0)
    return (float(kd) * diffuse + (blinn_phong_norm(s) * float(ks)) * specular) * mask


class PrefilteredRenderer(torch.nn.Module):
    """``renderer(envmap=..., **kwargs) -> (colors [B, S, S, 3], pixel_normals [B, S, S, 3])`` -- the call shape
    ``RENI.set_renderer`` expects -- shading with ``shade_prefiltered`` instead of the per-pixel sum over texels, forward and
    backward.  The first argument is a ``mesh.MeshRasterizer`` (then the call takes ``meshes_world``, ``R``, ``T`` as
    ``mesh.HipMeshRenderer`` does, and the G-buffer is the rasteriser's cached one) or an ``envmap_shader.GBuffer``.

    ks defaults to 1 - kd.  camera_center defaults to what ``HipMeshRenderer`` uses -- the rasteriser's camera asked WITHOUT
    R and T, the reference's quirk -- or to the G-buffer's own; with kd = 1 the two renderers differ only by the lookup's
    interpolation on the out_width grid."""

    def __init__(self, rasterizer_or_gbuffer, kd: float, shininess: float = 500.0, out_width: int = 64, ks=None,
                 camera_center=None):
        super().__init__()
        from .envmap_shader import GBuffer
        self.gbuffer = rasterizer_or_gbuffer if isinstance(rasterizer_or_gbuffer, GBuffer) else None
        self.rasterizer = None if self.gbuffer is not None else rasterizer_or_gbuffer
        if self.gbuffer is None and not hasattr(self.rasterizer, "gbuffer"):
            raise ValueError("PrefilteredRenderer needs a mesh.MeshRasterizer or an envmap_shader.GBuffer")
        self.kd = float(kd)
        self.ks = 1.0 - self.kd if ks is None else float(ks)
        self.shininess = float(shininess)
        self.out_width = int(out_width)
        if self.out_width < 2 or self.out_width % 2:
            raise ValueError(f"out_width must be even and >= 2, got {out_width}")
        if camera_center is None:
            camera_center = (self.gbuffer.camera_center if self.gbuffer is not None
                             else self.rasterizer.cameras.get_camera_center())
        self.camera_center = torch.as_tensor(camera_center, dtype=torch.float32).detach().reshape(-1)[:3].cpu()

    def forward(self, meshes_world=None, R=None, T=None, envmap=None, **kwargs):
        dev = envmap.environment_map.device
        if self.gbuffer is not None:
            g = self.gbuffer
            if g.pixel_normals.device != dev and dev.type == "cuda":
                g.to(dev)
            nrm, pos, (Hr, Wr) = g.pixel_normals, g.pixel_positions, g.image_size
        else:
            _, nrm, pos = self.rasterizer.gbuffer(meshes_world, R, T)
            Hr = Wr = self.rasterizer.raster_settings.image_size
        B = envmap.environment_map.shape[0]
        colors = shade_prefiltered(envmap, nrm, pos, self.camera_center, self.shininess, self.kd, self.ks, self.out_width)
        normals = torch.nn.functional.normalize(nrm, p=2, dim=-1, eps=1e-6).reshape(1, Hr, Wr, 3).repeat(B, 1, 1, 1)
        return colors.reshape(B, Hr, Wr, 3), normals
