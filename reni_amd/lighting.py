"""Environment maps as light sources without visiting every texel: importance-sampled light lists, on the device.

A map of H x W texels is H W point lights; an HDR map with a sun keeps nearly all of its energy in a handful of them.
``build_light_table`` turns a batch of maps into a luminance x solid-angle distribution, ``sample_lights`` draws S lights per
map from it by inverse-CDF sampling, and the result -- directions and colours [B, S, 3] -- feeds the two consumers:

    sampled_irradiance(samples, normals)      diffuse: scale sum_s max(0, n . d_s) colors_s       (reni_lights_irradiance)
    shade_sampled(samples, normals, ...)      Blinn-Phong: ``ops.envmap_shade`` with per-image light lists
    light_visibility(rasterizer, mesh, ...)   which pixels each sampled light reaches past the mesh (cast shadows)

All three steps are HIP calls of reni_tu_lights.hip (include/reni_hip.h has the definitions); nothing here touches a texel.

Definitions (omega_i the exact solid angle of a texel of row i, ``baselines.reni_grid_weights``; L the map's radiance):

    f    = max(0, 0.2126 r + 0.7152 g + 0.0722 b) omega_i mask             the importance of a texel, F = sum f
    pmf  = (1 - eps) f / F + eps omega_i / 4 pi                            eps = uniform_mix; F zero or not finite: eps = 1
    cond = the CDF along each row, marg = the CDF over the rows            (both end on exactly 1)
    row i    = #{marg <= u0}, column j = #{cond[i] <= u1}                  numpy's searchsorted(side="right")
    pdf      = pmf / omega_i                                               per steradian
    colors_s = L_s texel_weight_s / (S pmf_s)

so that ``sum_s colors_s g(d_s)`` estimates ``sum_t texel_weight_t L_t g(d_t)``: with texel_weight "solid_angle" that is the
irradiance integral (``baselines.irradiance_map``), with "sineweight" the sum the FIT_INVERSE shader forms over
``EnvironmentMap``'s pre-multiplied map.  ``jitter=True`` moves each direction uniformly in solid angle inside its texel, which
keeps ``pdf`` exact; RENI is a continuous field, so with a ``model`` the radiance is then re-evaluated at the moved directions.

Uniforms are drawn on the CPU generator and moved, so a seed fixes the samples on every machine.  There is no CPU fallback: a
CPU tensor raises ``RENILibraryError``; bad shapes and arguments raise ``ValueError`` before the library is touched.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

__all__ = ["LightTable", "LightSamples", "build_light_table", "uniforms", "texel_weights", "sample_lights", "sampled_irradiance", "shade_sampled", "light_visibility", "ambient_occlusion"]


@dataclass
class LightTable:
    """The sampling distribution of B maps: pmf, cond [B, H, W] and marg [B, H], float32 on the maps' device; ``space`` and
    ``minmax`` are what the maps were read with (``sample_lights`` reads them the same way)."""
    pmf: torch.Tensor
    cond: torch.Tensor
    marg: torch.Tensor
    H: int
    W: int
    space: str = "linear"
    minmax: Optional[Tuple[float, float]] = None


@dataclass
class LightSamples:
    """S lights per map: index [B, S] int32 (texel i W + j), dirs [B, S, 3], pdf [B, S] per steradian, radiance and colors
    [B, S, 3]."""
    index: torch.Tensor
    dirs: torch.Tensor
    pdf: torch.Tensor
    radiance: torch.Tensor
    colors: torch.Tensor


def build_light_table(maps, space: str = "linear", minmax=None, mask=None, uniform_mix: float = 0.0, size=None) -> LightTable:
    """The distribution sum-normalised luminance x solid angle of maps [B, H, W, 3], [B, H W, 3] (a model output; ``size`` =
    (H, W), default H x 2H) or planar [B, 3, H, W], read in place.  space "linear": the maps are stored normalised and
    ``minmax`` maps them back to radiance; "stored": they are radiance already.  mask (>= 0, anything that broadcasts to
    [B, H, W] or a [1 | B, H W, 3] mask) multiplies the importance only: a texel under 0 is never sampled.  uniform_mix in
    [0, 1] blends in the uniform-solid-angle distribution, which bounds colors by radiance 4 pi / (S uniform_mix)."""
    pmf, cond, marg = ops.light_table_build(maps, space, minmax, mask, uniform_mix, size)
    mm = None if space == "stored" else (float(minmax[0]), float(minmax[1]))
    return LightTable(pmf, cond, marg, int(pmf.shape[1]), int(pmf.shape[2]), space, mm)


def _stratum_sides(S: int):
    a = math.isqrt(S)
    while a >= 2 and S % a:
        a -= 1
    if a < 2:
        raise ValueError(f"a stratified set needs S = a b with a, b >= 2, and {S} has no such factorisation")
    return a, S // a


def uniforms(S: int, kind: str = "random", generator=None, device=None) -> torch.Tensor:
    """[S, 2] float32 in [0, 1).  "random": independent; "stratified": an a x b jittered grid with a b = S (a the largest
    divisor up to sqrt(S)), sample k in stratum (k // b, k % b) -- one sample per stratum, and every value stays inside it after
    rounding to float32.  Drawn from ``generator`` (a CPU generator; default: torch's global one) and then moved to ``device``."""
    S = int(S)
    if S < 1:
        raise ValueError(f"S must be >= 1, got {S}")
    if kind not in ("random", "stratified"):
        raise ValueError(f'kind must be "random" or "stratified", got {kind!r}')
    if generator is not None and generator.device.type != "cpu":
        raise ValueError("uniforms are drawn on a CPU generator, so that a seed gives the same samples on every machine")
    if kind == "stratified":
        a, b = _stratum_sides(S)
    r = torch.rand(S, 2, generator=generator, dtype=torch.float32)
    if kind == "stratified":
        k = np.arange(S)
        cell = np.stack([k // b, k % b], 1).astype(np.float64)
        n = np.asarray([a, b], np.float64)
        u = ((cell + r.numpy().astype(np.float64)) / n).astype(np.float32)
        over = u.astype(np.float64) >= (cell + 1) / n  # rounded up onto the next stratum's edge
        u[over] = np.nextafter(u[over], np.float32(0))
        r = torch.from_numpy(u)
    return r if device is None else r.to(device)


def texel_weights(kind: str, W: int, device=None) -> torch.Tensor:
    """[H W] float32 on ``device``: "solid_angle" (``baselines.reni_grid_weights``) or "sineweight" (``utils.get_sineweight``)."""
    if kind == "solid_angle":  # (the row table ``ops.light_grid`` keeps on the device, repeated there: no host copy per call)
        return ops.light_grid(int(W), "cpu" if device is None else device)[0].repeat_interleave(int(W))
    elif kind == "sineweight":
        from .utils import get_sineweight
        w = get_sineweight(int(W))[0, :, 0].to(torch.float32).contiguous()
    else:
        raise ValueError(f'texel_weight must be "solid_angle", "sineweight", None or a tensor, got {kind!r}')
    return w if device is None else w.to(device)


def sample_lights(table: LightTable, maps, u=None, n_samples=None, generator=None, jitter: bool = False,
                  texel_weight="solid_angle", model=None, latents=None) -> LightSamples:
    """S lights per map of ``maps`` (the maps ``table`` was built from, in any of its layouts) for uniforms ``u`` [S, 2]
    (shared by the maps) or [B, S, 2]; without ``u``, ``uniforms(n_samples, "random", generator)``.  texel_weight: what the
    estimated sum weights a texel by -- "solid_angle" (irradiance), "sineweight" (the FIT_INVERSE shader's sum), None (1) or a
    tensor [H W].  jitter: directions uniform in solid angle inside their texels instead of the texel centres; radiance and
    colors stay the texel's unless ``model`` (and ``latents``: the model's first argument, indices or latent codes of the B
    maps) is given, which is then evaluated at the moved directions -- its output is read in ``table.space``."""
    if not isinstance(table, LightTable):
        raise ValueError("table must be a LightTable (build_light_table)")
    v = ops.light_maps_view(maps, (table.H, table.W))
    B = v.shape[0]
    if tuple(v.shape[2:]) != (table.H, table.W) or tuple(table.pmf.shape) != (B, table.H, table.W):
        raise ValueError(f"the table is of {tuple(table.pmf.shape)} maps, the maps are {tuple(v.shape)}")
    if u is None:
        if n_samples is None:
            raise ValueError("pass the uniforms u or n_samples")
        u = uniforms(int(n_samples), "random", generator, v.device)
    elif n_samples is not None and isinstance(u, torch.Tensor) and u.dim() >= 2 and int(n_samples) != u.shape[-2]:
        raise ValueError(f"n_samples = {n_samples} but u holds {u.shape[-2]} samples")
    if (model is None) != (latents is None):
        raise ValueError("model and latents come together")
    if model is not None and not jitter:
        raise ValueError("a model re-evaluates the radiance at jittered directions: pass jitter=True")
    if isinstance(texel_weight, str):
        tw = texel_weights(texel_weight, table.W, v.device)
    else:
        tw = texel_weight
    out = LightSamples(*ops.light_sample(table.pmf, table.cond, table.marg, v, u, table.space, table.minmax, tw, jitter))
    if model is not None:
        S = out.index.shape[1]
        with torch.no_grad():
            rad = model(latents, out.dirs)
        if tuple(rad.shape) != (B, S, 3):
            raise ValueError(f"the model returned {tuple(rad.shape)} for directions [{B}, {S}, 3]")
        if table.space == "linear":
            rad = ops.unnormalise_srgb(rad.permute(0, 2, 1).unsqueeze(2), table.minmax, srgb=False)[:, :, 0].permute(0, 2, 1)
        idx = out.index.long()
        omega = ops.light_grid(table.W, v.device)[0][idx // table.W]
        gain = 1.0 / (S * out.pdf * omega)  # 1 / (S pmf)
        if tw is not None:
            gain = gain * tw.to(torch.float32)[idx]
        out.radiance = rad.contiguous()
        out.colors = out.radiance * gain.unsqueeze(-1)
    return out


def sampled_irradiance(samples: LightSamples, normals, scale: float = 1.0 / math.pi) -> torch.Tensor:
    """[B, P, 3] = scale sum_s max(0, n_p . dirs_s) colors_s for normals [P, 3] (shared) or [B, P, 3].  With samples of
    texel_weight "solid_angle" and the default scale this estimates ``baselines.irradiance_map`` at the normals."""
    if not isinstance(samples, LightSamples):
        raise ValueError("samples must be LightSamples (sample_lights)")
    return ops.lights_irradiance(normals, samples.dirs, samples.colors, scale)


def shade_sampled(samples: LightSamples, normals, positions, camera_center, shininess=None, kd=None, ks=None, visibility=None,
                  materials=None) -> torch.Tensor:
    """[B, NP, 3]: the Blinn-Phong environment-map shader (``ops.envmap_shade``) lit by the S sampled lights of each map
    instead of its H W texels; sample with texel_weight "sineweight" to estimate what the shader gives for the whole map.
    ``visibility``: the mask of ``light_visibility`` for these samples -- a light lights only the pixels that see it.
    ``materials``: an ``envmap_shader.SpatialMaterials`` of NP pixels instead of the scalars shininess, kd, ks (the shader's
    terms path with per-image light lists; differentiable with respect to ``samples.colors`` and the materials)."""
    if not isinstance(samples, LightSamples):
        raise ValueError("samples must be LightSamples (sample_lights)")
    if materials is not None:
        from .envmap_shader import SpatialMaterials, _shade_terms, compose_materials
        if not isinstance(materials, SpatialMaterials):
            raise ValueError("materials must be an envmap_shader.SpatialMaterials")
        albedo, ks_p, s_p = materials.values()
        D, S = _shade_terms(samples.colors, samples.dirs, normals, positions, camera_center, s_p, vis=visibility)
        return compose_materials(D, S, albedo, ks_p, s_p)
    if shininess is None or kd is None or ks is None:
        raise ValueError("shininess, kd and ks are required without materials")
    return ops.envmap_shade(normals, positions, camera_center, samples.dirs, samples.colors, shininess, kd, ks, vis=visibility)


def light_visibility(rasterizer, mesh, R, T, samples: LightSamples, t_min=None) -> torch.Tensor:
    """The visibility mask [B, NP, ceil(S/32)] of each map's S sampled lights over ``rasterizer``'s G-buffer of ``mesh`` seen
    with (R, T) (``mesh.MeshRasterizer.visibility`` with per-image direction lists): sampled point lights that cast shadows."""
    if not isinstance(samples, LightSamples):
        raise ValueError("samples must be LightSamples (sample_lights)")
    return rasterizer.visibility(mesh, R, T, samples.dirs, t_min=t_min)


def ambient_occlusion(vis, normals, dirs, weights) -> torch.Tensor:
    """[NP] = sum_j w_j max(0, n . d_j) vis(p, j) / sum_j w_j max(0, n . d_j), and 0 where the denominator is 0: the
    cosine-weighted share of the directions ``dirs`` [J, 3] (weights [J], e.g. solid angles) that pixel p sees past the mesh.
    vis is the mask [1, NP, ceil(J/32)] of a shared grid; normals [NP, 3] need not be normalised.  Two calls of the shader
    (kd = 1, ks = 0, colours w), masked and unmasked -- no kernel of its own."""
    if not isinstance(dirs, torch.Tensor) or dirs.dim() != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs must be [J, 3] (a shared grid)")
    J = dirs.shape[0]
    if not isinstance(normals, torch.Tensor) or normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError("normals must be [NP, 3]")
    if not isinstance(weights, torch.Tensor) or weights.numel() != J:
        raise ValueError(f"weights must hold {J} values")
    ops.check_visibility(vis, normals.shape[0], J, NB=1)
    w = weights.reshape(1, J, 1).to(torch.float32).expand(1, J, 3).contiguous()
    pos = torch.zeros_like(normals, dtype=torch.float32)
    cam = torch.tensor([0.0, 0.0, 1.0])
    num = ops.envmap_shade(normals, pos, cam, dirs, w, 1.0, 1.0, 0.0, vis=vis)[0, :, 0]
    den = ops.envmap_shade(normals, pos, cam, dirs, w, 1.0, 1.0, 0.0)[0, :, 0]
    return torch.where(den > 0, num / den.clamp_min(1e-30), torch.zeros_like(den))
