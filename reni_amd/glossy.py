"""Environment maps as glossy lighting: maps convolved with zonal specular lobes (one map per lobe, a chain over roughness),
looked up at arbitrary directions, and what follows from the two -- the SH-domain counterpart, a prefiltered stand-in for the
Blinn-Phong shader, and the ``glossy_psnr`` columns of ``metrics.evaluate``.

The arithmetic runs in libreni_hip.so (``reni_lobe_convolve``, ``reni_envmap_lookup``: include/reni_hip.h); there is no CPU
fallback, a CPU tensor raises ``RENILibraryError``.  ``lobe_band_scale`` is host float64.

``sample`` is ``lookup`` made differentiable in its query (``reni_envmap_lookup_dquery``), ``ggx_dfg`` the directional-albedo
table of the microfacet material (``reni_ggx_dfg``), and ``shade_split_sum`` / ``PrefilteredRenderer(materials=...)`` shade
base-colour / roughness / metallic materials from a chain with the two.

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


class _SampleFn(torch.autograd.Function):
    """``ops.envmap_lookup`` differentiable in its query as well: the maps' gradient is ``_LookupFn``'s gather, the gradients of
    dirs and of a level tensor come from ``ops.envmap_lookup_dquery`` -- launched only when one of the two is asked for, and
    each half only when asked."""

    @staticmethod
    def forward(ctx, maps, dirs, level):
        tensor_level = isinstance(level, torch.Tensor)
        ctx.save_for_backward(maps, dirs, *((level,) if tensor_level else ()))
        ctx.level = None if tensor_level else level
        return ops.envmap_lookup(maps, dirs, level)

    @staticmethod
    def backward(ctx, grad_out):
        maps, dirs, *level = ctx.saved_tensors
        level = level[0] if level else ctx.level
        need_maps, need_dirs = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_level = ctx.needs_input_grad[2] and isinstance(level, torch.Tensor)
        gm = gd = gl = None
        grad_out = grad_out.contiguous()
        if need_maps:
            Lv, H, W = (1,) + tuple(maps.shape[1:3]) if maps.dim() == 4 else tuple(maps.shape[1:4])
            gm = ops.envmap_lookup_backward(grad_out, Lv, H, W, dirs, level).view(maps.shape)
        if need_dirs or need_level:
            gd, gl = ops.envmap_lookup_dquery(maps, dirs, level, grad_out, need_dirs=need_dirs, need_level=need_level)
            if gd is not None:
                gd = gd.to(dirs.dtype)
            if gl is not None:
                gl = gl.to(level.dtype)
        return gm, gd, gl


def sample(maps_or_chain: torch.Tensor, dirs: torch.Tensor, level=None) -> torch.Tensor:
    """``lookup`` -- the same arguments, the same forward bits -- differentiable in its QUERY too: in the maps (the gather of
    ``lookup``), in dirs and in a tensor level (``ops.envmap_lookup_dquery``, one lane per direction).  The direction's
    gradient is the chain rule through the equirectangular coordinates on the lookup's own four taps (0 at a pole direction
    and for the zero vector); the level's is the slope of the piecewise-linear mix, right-sided at a knot, left-sided at the top
    level, 0 outside [0, Lv - 1].  Shared dirs [P, 3] / level [P] get the sum over the maps."""
    if not (_wants_grad(maps_or_chain) or _wants_grad(dirs) or _wants_grad(level)):
        return ops.envmap_lookup(maps_or_chain, dirs, level)
    tensor_level = isinstance(level, torch.Tensor) and level.dim() > 0
    ops._require_cuda(maps_or_chain, dirs, level if tensor_level else None)
    maps = maps_or_chain if maps_or_chain.dtype == torch.float32 else maps_or_chain.float()
    if maps.dim() not in (4, 5):
        raise ValueError(f"maps must be [N, H, W, 3] or [N, Lv, H, W, 3], got {tuple(maps.shape)}")
    if isinstance(level, torch.Tensor) and not tensor_level:
        level = float(level)  # a 0-d tensor is a number here, as in ``lookup``
    return _SampleFn.apply(maps, dirs, level)


# ------------------------------------------------------------------------------------------ directional albedo (DFG)
DFG_NODES = 128  # the table's quadrature: DFG_NODES x DFG_NODES midpoint nodes per entry


def ggx_dfg(size: int = 32, roughness_min: float = 0.1, device="cuda") -> torch.Tensor:
    """The directional-albedo table [2, size, size] of the microfacet material (``ops.ggx_dfg``, 128 x 128 nodes):
    table[m, j, i] = A_m at N.V = i / (size - 1) and roughness = roughness_min + j (1 - roughness_min) / (size - 1), with
    A0 = int k d omega and A1 = int k f d omega over the hemisphere (k, f: ``envmap_shader.shade_terms_ggx``).  Cached per
    (size, roughness_min, device) like the other device tables: treat it as a constant."""
    size, roughness_min = int(size), float(roughness_min)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ops._lib.RENILibraryError("RENI HIP ops need tensors on a GPU device (got a CPU device); there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return _diffuse_device_tables(("ggx_dfg", size, roughness_min, DFG_NODES),
                                  lambda: (ops.ggx_dfg(size, size, roughness_min, DFG_NODES, DFG_NODES, dev),), dev)[0]


def dfg_lookup(table: torch.Tensor, nv: torch.Tensor, roughness: torch.Tensor, roughness_min: float = 0.1):
    """(A0, A1), each shaped like nv: the bilinear read of a ``ggx_dfg`` table built with roughness_min at N.V = nv and
    roughness (both clamped to the table's range; roughness broadcasts against nv).  Plain torch, any device and float dtype;
    the table is a constant, so autograd gives d nv and d roughness without a scatter."""
    if table.dim() != 3 or table.shape[0] != 2 or min(table.shape[1:]) < 2:
        raise ValueError(f"table must be [2, R_r, R_v] with R_r, R_v >= 2, got {tuple(table.shape)}")
    Rr, Rv = int(table.shape[1]), int(table.shape[2])
    t = table.detach().to(nv.dtype)
    roughness = torch.as_tensor(roughness, dtype=nv.dtype, device=nv.device)
    x = nv.clamp(0.0, 1.0) * (Rv - 1)
    y = ((roughness.clamp(float(roughness_min), 1.0) - float(roughness_min)) * ((Rr - 1) / (1.0 - float(roughness_min)))).expand_as(nv)
    i0 = x.detach().floor().clamp(0, Rv - 2).long()
    j0 = y.detach().floor().clamp(0, Rr - 2).long()
    fx, fy = x - i0, y - j0
    flat = t.reshape(2, -1)
    e = j0 * Rv + i0
    t00, t01, t10, t11 = flat[:, e], flat[:, e + 1], flat[:, e + Rv], flat[:, e + Rv + 1]
    A = (1 - fy) * ((1 - fx) * t00 + fx * t01) + fy * ((1 - fx) * t10 + fx * t11)
    return A[0], A[1]


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


CHAIN_ROUGHNESS = (0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.0)  # the default knots of ``shade_split_sum``'s specular levels


def _chain_roughness(chain_roughness):
    rho = tuple(float(x) for x in chain_roughness)
    if not 1 <= len(rho) <= 15 or not all(0.0 < x <= 1.0 for x in rho) or any(b <= a for a, b in zip(rho[:-1], rho[1:])):
        raise ValueError(f"chain_roughness must be 1..15 ascending values in (0, 1], got {chain_roughness!r}")
    return rho


def roughness_level(roughness: torch.Tensor, chain_roughness) -> torch.Tensor:
    """The chain level of a roughness (already clamped to [rho_0, rho_{K-1}]): piecewise linear through rho_k -> 1 + k, the
    segment to the right of an interior knot and to the left of the last one -- the side ``sample`` takes the level's slope on.
    Plain torch, differentiable."""
    rho = _chain_roughness(chain_roughness)
    K = len(rho)
    if K == 1:
        return torch.ones_like(roughness)
    knots = torch.as_tensor(rho, dtype=roughness.dtype, device=roughness.device)
    k = torch.bucketize(roughness.detach(), knots[1:-1].contiguous(), right=True)  # segment 0 .. K - 2
    lo, hi = knots[k], knots[k + 1]
    return (1.0 + k.to(roughness.dtype)) + (roughness - lo) / (hi - lo)


def shade_split_sum(envmap, normals, positions, camera_center, base_color, roughness, metallic,
                    chain_roughness=CHAIN_ROUGHNESS, out_width: int = 64, roughness_min: float = 0.1,
                    f0_dielectric: float = 0.04, dfg_size: int = 32) -> torch.Tensor:
    """Microfacet (GGX) colours [B, NP, 3] of a G-buffer FROM A PREFILTERED CHAIN by the split-sum approximation, instead of
    the per-pixel sums over texels of ``envmap_shader.microfacet_shading_materials`` (whose arguments base_color, roughness,
    metallic, roughness_min and f0_dielectric mean the same here).

    ``envmap.environment_map`` [B, H W, 3] must live on RENI's own grid, multiplied by the sine weight as ``EnvironmentMap``
    does.  One unnormalised ``lobe_convolve`` with weight 1 builds the chain [phong(1), ggx(rho_0), ..., ggx(rho_{K-1})] on
    the out_width grid (rho = chain_roughness, ascending); the specular levels are divided by the cached lobe denominators of
    the sine weight, so they hold the lobe-weighted MEAN radiance.  With n the unit normal, v the view direction,
    r = 2 (n.v) n - v and rc = clamp(roughness, max(roughness_min, rho_0), rho_{K-1}):

        D   = sample(chain, n, 0)                          the shader's own diffuse sum, up to the bilinear lookup
        P   = sample(chain, r, level(rc))                  level piecewise linear through rho_k -> 1 + k
        S_m = P A_m(clamp(n.v, 0, 1), rc) Q / (2 pi^2)      A = ``ggx_dfg``, Q the texel count: a texel's solid angle is
                                                           sine weight x 2 pi^2 / Q, the shader sums without it
        colours = compose_microfacet(D, S0, S1, base_color, metallic, f0_dielectric) x (the normal is not zero)

    Differentiable with respect to the map (one transposed convolution and two gathers), the normals, the roughness (through
    the level and the table), the base colour and the metallic; positions and camera are constants.  It is the n = v = r
    approximation of the lobe: exact for a constant map up to the table's quadrature, approximate otherwise."""
    from .envmap_shader import _constant as _shader_constant, _shared_grid, compose_microfacet
    from .utils import get_directions, get_sineweight
    Wo = int(out_width)
    if Wo < 2 or Wo % 2:
        raise ValueError(f"out_width must be even and >= 2, got {out_width}")
    if not 0.0 < float(roughness_min) <= 1.0:
        raise ValueError("0 < roughness_min <= 1 is required")
    rho = _chain_roughness(chain_roughness)
    _shader_constant("the pixel positions", positions)
    _shader_constant("the camera centre", camera_center)
    _shader_constant("the light directions", envmap.directions)
    colors = envmap.environment_map
    ops._require_cuda(colors, normals, positions)
    if colors.dim() != 3:
        raise ValueError(f"shade_split_sum needs a map [B, H W, 3] on RENI's grid, got {tuple(colors.shape)}")
    W = _grid_width(colors)
    grid = _shared_grid(envmap.directions)
    if grid.dim() != 2 or grid.shape[0] != colors.shape[1]:
        raise ValueError("shade_split_sum needs one texel grid shared by the batch")
    dev = colors.device
    B, Q, K = colors.shape[0], colors.shape[1], len(rho)
    (odirs,) = _diffuse_device_tables(("reni_out", Wo), lambda: (get_directions(Wo)[0],), dev)
    gdirs, sinw = _diffuse_device_tables(("reni_sine", W), lambda: (get_directions(W)[0], get_sineweight(W)[0, :, 0]), dev)
    ones = torch.ones(Q, dtype=torch.float32, device=dev)
    lobes = [phong(1.0)] + [ggx(x) for x in rho]
    (den,) = _diffuse_device_tables(("split_sum_den", W, Wo) + rho, lambda: (ops.lobe_denominators(
        gdirs, sinw, odirs, ["ggx"] * K, [l.param for l in lobes[1:]]),), dev)
    chain = lobe_convolve(colors, grid, ones, odirs, lobes, normalise=False)  # [B, 1 + K, Po, 3]
    inv = torch.where(den > 0, 1.0 / den.clamp_min(1e-30), torch.zeros_like(den))
    scale = torch.cat([torch.ones(1, den.shape[1], device=dev), inv], 0)
    chain = (chain * scale[None, :, :, None]).view(B, 1 + K, Wo // 2, Wo, 3)
    NP = normals.shape[0]
    rough = torch.as_tensor(roughness, dtype=torch.float32, device=dev) if not isinstance(roughness, torch.Tensor) else roughness.float()
    if rough.numel() != 1 and tuple(rough.shape) != (NP,):
        raise ValueError(f"roughness must be a float, one value or [{NP}] (one per pixel), got {tuple(rough.shape)}")
    # only the pixels with a normal are sampled: the background's zero normals all name one texel, whose gradient the lookup's
    # gather would sum in one lane, and their colours and gradients are 0 whatever is sampled
    fg = (normals != 0).any(-1).nonzero().squeeze(1)
    NF = int(fg.shape[0])
    if NF == 0:
        return torch.zeros(B, NP, 3, dtype=torch.float32, device=dev) + colors.sum() * 0.0  # (still a function of the map)

    def pick(x, per_pixel_shape):  # a per-pixel input at the sampled pixels; a scalar or a colour stays as it is
        return x.index_select(0, fg) if NF < NP and isinstance(x, torch.Tensor) and tuple(x.shape) == per_pixel_shape else x

    pos = pick(positions, (NP, 3))
    n, r, _ = shading_dirs(pick(normals, (NP, 3)), pos, camera_center)
    cam = torch.as_tensor(camera_center, dtype=torch.float32).reshape(-1)[:3].to(dev)
    v = torch.nn.functional.normalize(cam[None] - pos.float(), p=2, dim=-1, eps=1e-6)
    nv = (n * v).sum(-1).clamp(0.0, 1.0)
    rc = pick(rough, (NP,)).reshape(-1).expand(NF).clamp(max(float(roughness_min), rho[0]), rho[-1])
    D = sample(chain, n, 0.0)
    Pm = sample(chain, r, roughness_level(rc, rho))
    table = ggx_dfg(int(dfg_size), float(roughness_min), dev)
    A0, A1 = dfg_lookup(table, nv, rc, float(roughness_min))
    measure = Q / (2.0 * math.pi ** 2)
    S0 = Pm * (A0 * measure)[None, :, None]
    S1 = Pm * (A1 * measure)[None, :, None]
    col = compose_microfacet(D, S0, S1, pick(base_color, (NP, 3)), pick(metallic, (NP,)), f0_dielectric)
    if NF == NP:
        return col
    return torch.zeros(B, NP, 3, dtype=col.dtype, device=dev).index_copy(1, fg, col)


class PrefilteredRenderer(torch.nn.Module):
    """``renderer(envmap=..., **kwargs) -> (colors [B, S, S, 3], pixel_normals [B, S, S, 3])`` -- the call shape
    ``RENI.set_renderer`` expects -- shading with ``shade_prefiltered`` instead of the per-pixel sum over texels, forward and
    backward.  The first argument is a ``mesh.MeshRasterizer`` (then the call takes ``meshes_world``, ``R``, ``T`` as
    ``mesh.HipMeshRenderer`` does, and the G-buffer is the rasteriser's cached one) or an ``envmap_shader.GBuffer``.

    ks defaults to 1 - kd.  camera_center defaults to what ``HipMeshRenderer`` uses -- the rasteriser's camera asked WITHOUT
    R and T, the reference's quirk -- or to the G-buffer's own; with kd = 1 the two renderers differ only by the lookup's
    interpolation on the out_width grid.

    ``materials=MicrofacetMaterials(...)`` / ``TexturedMicrofacetMaterials(...)``: the pixels are shaded with
    ``shade_split_sum`` (chain_roughness, dfg_size and out_width are its arguments; kd, ks and shininess are not used).  The
    values and, with a normal texture, the bent shading normals are fetched as ``mesh.HipMeshRenderer`` fetches them (a textured
    material needs a rasteriser), ``shader_cameras`` gives the camera centre as it does there, and the returned
    ``pixel_normals`` stay the geometry's.  The render is differentiable with respect to the map, the materials and the normal
    texture.  Shadows are not supported.  Without ``materials`` kd is required and nothing changes.  A mesh whose vertices
    require grad raises a ValueError (geometry gradients go through ``mesh.HipMeshRenderer``)."""

    def __init__(self, rasterizer_or_gbuffer, kd: float = None, shininess: float = 500.0, out_width: int = 64, ks=None,
                 camera_center=None, materials=None, chain_roughness=CHAIN_ROUGHNESS, dfg_size: int = 32, shader_cameras=None):
        super().__init__()
        from .envmap_shader import GBuffer, MicrofacetMaterials
        from .textures import TexturedMicrofacetMaterials
        self.gbuffer = rasterizer_or_gbuffer if isinstance(rasterizer_or_gbuffer, GBuffer) else None
        self.rasterizer = None if self.gbuffer is not None else rasterizer_or_gbuffer
        if self.gbuffer is None and not hasattr(self.rasterizer, "gbuffer"):
            raise ValueError("PrefilteredRenderer needs a mesh.MeshRasterizer or an envmap_shader.GBuffer")
        if materials is not None and not isinstance(materials, (MicrofacetMaterials, TexturedMicrofacetMaterials)):
            raise ValueError("materials must be a MicrofacetMaterials or a TexturedMicrofacetMaterials (or None: scalar "
                             "Blinn-Phong with kd, ks and shininess)")
        self.materials = materials
        self.textured = isinstance(materials, TexturedMicrofacetMaterials)
        if self.textured and self.rasterizer is None:
            raise ValueError("a TexturedMicrofacetMaterials is fetched through a mesh.MeshRasterizer, not a fixed GBuffer")
        if kd is None and materials is None:
            raise ValueError("kd is required unless materials is a MicrofacetMaterials or a TexturedMicrofacetMaterials")
        self.kd = 1.0 if kd is None else float(kd)
        self.ks = 1.0 - self.kd if ks is None else float(ks)
        self.shininess = float(shininess)
        self.out_width = int(out_width)
        if self.out_width < 2 or self.out_width % 2:
            raise ValueError(f"out_width must be even and >= 2, got {out_width}")
        self.chain_roughness = _chain_roughness(chain_roughness)
        self.dfg_size = int(dfg_size)
        if camera_center is None:
            if shader_cameras is not None:
                camera_center = shader_cameras.get_camera_center()
            else:
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
            if meshes_world.verts_packed().requires_grad and torch.is_grad_enabled():
                raise ValueError("PrefilteredRenderer cannot be rendered while the mesh's vertices require grad: the prefiltered "
                                 "lookup has no gradient with respect to geometry (detach the vertices, or use mesh.HipMeshRenderer)")
            _, nrm, pos = self.rasterizer.gbuffer(meshes_world, R, T)
            if nrm.requires_grad:
                raise ValueError("PrefilteredRenderer cannot be rendered while the camera (R, T or the fov) requires grad: the "
                                 "prefiltered lookup has no gradient with respect to geometry (detach the camera, or use "
                                 "mesh.HipMeshRenderer)")
            Hr = Wr = self.rasterizer.raster_settings.image_size
        B = envmap.environment_map.shape[0]
        if self.materials is not None:
            m = self.materials
            if m.roughness.device != nrm.device:
                m.to(nrm.device)
            shade_nrm = nrm
            if not self.textured:
                values = m.values()
            else:
                values = m.values(self.rasterizer, meshes_world, R, T)
                if m.normal is not None:  # the normal map bends the shading normals only
                    shade_nrm = m.shading_normals(self.rasterizer, meshes_world, R, T, nrm)
            colors = shade_split_sum(envmap, shade_nrm, pos, self.camera_center, *values, chain_roughness=self.chain_roughness,
                                     out_width=self.out_width, roughness_min=m.roughness_min, f0_dielectric=m.f0_dielectric,
                                     dfg_size=self.dfg_size)
        else:
            colors = shade_prefiltered(envmap, nrm, pos, self.camera_center, self.shininess, self.kd, self.ks, self.out_width)
        normals = torch.nn.functional.normalize(nrm, p=2, dim=-1, eps=1e-6).reshape(1, Hr, Wr, 3).repeat(B, 1, 1, 1)
        return colors.reshape(B, Hr, Wr, 3), normals
