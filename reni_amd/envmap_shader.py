"""Environment-map Blinn-Phong shading for the FIT_INVERSE task -- host mirror of the reference's
``src/utils/pytorch3d_envmap_shader.py`` over ``reni_envmap_shade`` / ``reni_envmap_shade_backward``
(include/reni_hip.h).

Same names and argument meaning as the reference: ``EnvironmentMap`` (:33-44),
``blinn_phong_shading_env_map`` (:46-116), ``BlinnPhongShaderEnvMap`` (:119-174), ``build_renderer`` (:177-217).
The shading arithmetic runs in the HIP library (there is no torch fallback: a CPU tensor raises); the only
tensor that carries a gradient is ``EnvironmentMap.environment_map`` -- the mesh, the camera and the texel grid
are constants in the reference's use (RENI_module.py:386-396).

pytorch3d (rasteriser, ``Meshes``, cameras) is not part of this build.  The shading function is duck-typed over
what it touches -- ``meshes.verts_packed() / faces_packed() / verts_normals_packed()``,
``fragments.pix_to_face / bary_coords``, ``cameras.get_camera_center()``, ``materials.shininess`` -- so real
pytorch3d objects work when the package is present, and a fixed G-buffer works without it
(``GBuffer`` / ``blinn_phong_shading_gbuffer``).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops


class EnvironmentMap:
    """Lighting colours and directions (reference :33-44): the map is pre-multiplied by the sine weight."""

    def __init__(self, environment_map: torch.Tensor = None, directions: torch.Tensor = None,
                 sineweight: torch.Tensor = None) -> None:
        self.directions = directions
        self.environment_map = environment_map * sineweight

    def to(self, device):
        self.directions = self.directions.to(device)
        self.environment_map = self.environment_map.to(device)
        return self


def interpolate_face_attributes(pix_to_face: torch.Tensor, bary_coords: torch.Tensor, face_attrs: torch.Tensor):
    """Barycentric interpolation of per-face-vertex attributes (pytorch3d.ops.interpolate_face_attributes):
    pix_to_face [N,H,W,K] (-1 = background), bary_coords [N,H,W,K,3], face_attrs [F,3,D] -> [N,H,W,K,D]."""
    mask = pix_to_face < 0
    attrs = face_attrs[pix_to_face.clamp(min=0)]
    out = (bary_coords[..., None] * attrs).sum(dim=-2)
    return out.masked_fill(mask[..., None], 0.0)


class _ShadeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, light_colors, normals, positions, camera_center, light_dirs, shininess, kd, ks, vis=None):
        ctx.save_for_backward(normals, positions, camera_center, light_dirs)
        ctx.consts = (float(shininess), float(kd), float(ks))
        ctx.vis = vis  # a constant of (mesh, camera, directions): see _constant_mask
        return ops.envmap_shade(normals, positions, camera_center, light_dirs, light_colors, *ctx.consts, vis=vis)

    @staticmethod
    def backward(ctx, dcolors):
        normals, positions, camera_center, light_dirs = ctx.saved_tensors
        g = ops.envmap_shade_backward(normals, positions, camera_center, light_dirs, dcolors.contiguous(), *ctx.consts,
                                      vis=ctx.vis)
        return g, None, None, None, None, None, None, None, None


def _constant_mask(vis, NP, directions):
    """A visibility mask rides through the shader as a constant (it depends on the geometry alone, and gradients with
    respect to geometry are out of scope): one that requires grad is an error, not a silently dropped gradient."""
    if vis is None:
        return None
    ops.check_visibility(vis, NP, directions.shape[-2])
    return vis


def _shared_grid(directions: torch.Tensor) -> torch.Tensor:
    """[B,J,3] directions -> [J,3] when every image uses the same grid (the reference's directions.repeat(B,1,1),
    RENI_module.py:376): the shading coefficients are then evaluated once for the whole batch."""
    if directions.dim() == 2:
        return directions
    if directions.shape[0] == 1 or bool((directions == directions[:1]).all()):
        return directions[0]
    return directions


def blinn_phong_shading_gbuffer(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap,
                                shininess, kd, ks, vis=None) -> torch.Tensor:
    """colors [B, NP, 3] from interpolated (not normalised) normals / positions [NP, 3] (reference :75-115).  ``vis``: a
    visibility mask of the envmap's directions (``MeshRasterizer.visibility``) -- only the texels a pixel sees light it."""
    s = float(torch.as_tensor(shininess).reshape(-1)[0])
    cam = torch.as_tensor(camera_center, dtype=torch.float32).reshape(-1)[:3].cpu()
    dirs = _shared_grid(envmap.directions)
    return _ShadeFn.apply(envmap.environment_map, pixel_normals, pixel_positions, cam, dirs, s, kd, ks,
                          _constant_mask(vis, pixel_normals.shape[0], dirs))


class _ShadeTermsFn(torch.autograd.Function):
    """(D, S) of ``ops.envmap_shade_terms``.  Gradients: the light colours through the backward kernel, the shininess as
    ds_p = sum_{b,c} gS T with T = dS/ds_p from the forward kernel (computed only when the shininess needs a gradient)."""

    @staticmethod
    def forward(ctx, light_colors, shininess, normals, positions, camera_center, light_dirs, vis, need_ds):
        D, S, T = ops.envmap_shade_terms(normals, positions, camera_center, light_dirs, light_colors, shininess, vis=vis,
                                         need_ds=need_ds)
        ctx.save_for_backward(normals, positions, camera_center, light_dirs, shininess, T)
        ctx.vis = vis  # a constant of (mesh, camera, directions): see _constant_mask
        return D, S

    @staticmethod
    def backward(ctx, gD, gS):
        normals, positions, camera_center, light_dirs, shininess, T = ctx.saved_tensors
        gC = gs = None
        if ctx.needs_input_grad[0]:
            gC = ops.envmap_shade_terms_backward(normals, positions, camera_center, light_dirs, gD.contiguous(),
                                                 gS.contiguous(), shininess, vis=ctx.vis)
        if ctx.needs_input_grad[1] and T is not None:
            gs = (gS * T).sum(dim=(0, 2))
            gs = (gs.sum() if shininess.numel() == 1 else gs).reshape(shininess.shape).to(shininess.dtype)
        return gC, gs, None, None, None, None, None, None


def _constant(what, t):
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise ValueError(f"{what} are constants of the shader (gradients with respect to geometry and camera are out of "
                         "scope): they cannot require grad")
    return t


class _ShadeTermsNormalsFn(torch.autograd.Function):
    """``_ShadeTermsFn`` with one more differentiable input, the (un-normalised) pixel normals: their gradient comes from
    ``ops.envmap_shade_terms_dnormals``, and only when somebody asks for it.  The forward call is the same kernel."""

    @staticmethod
    def forward(ctx, light_colors, shininess, normals, positions, camera_center, light_dirs, vis, need_ds):
        D, S, T = ops.envmap_shade_terms(normals, positions, camera_center, light_dirs, light_colors, shininess, vis=vis,
                                         need_ds=need_ds)
        ctx.save_for_backward(normals, positions, camera_center, light_dirs, shininess, T, light_colors)
        ctx.vis = vis
        return D, S

    @staticmethod
    def backward(ctx, gD, gS):
        normals, positions, camera_center, light_dirs, shininess, T, light_colors = ctx.saved_tensors
        gC = gs = gn = None
        gD, gS = gD.contiguous(), gS.contiguous()
        if ctx.needs_input_grad[0]:
            gC = ops.envmap_shade_terms_backward(normals, positions, camera_center, light_dirs, gD, gS, shininess, vis=ctx.vis)
        if ctx.needs_input_grad[1] and T is not None:
            gs = (gS * T).sum(dim=(0, 2))
            gs = (gs.sum() if shininess.numel() == 1 else gs).reshape(shininess.shape).to(shininess.dtype)
        if ctx.needs_input_grad[2]:
            gn = ops.envmap_shade_terms_dnormals(normals, positions, camera_center, light_dirs, light_colors, gD, gS,
                                                 shininess, vis=ctx.vis).to(normals.dtype)
        return gC, gs, gn, None, None, None, None, None


def _shade_terms(light_colors, light_dirs, pixel_normals, pixel_positions, camera_center, shininess, vis=None,
                 differentiable_normals=False):
    if not differentiable_normals:
        _constant("the pixel normals", pixel_normals)
    _constant("the pixel positions", pixel_positions)
    _constant("the light directions", light_dirs)
    cam = torch.as_tensor(_constant("the camera centre", camera_center), dtype=torch.float32).reshape(-1)[:3].cpu()
    NP = pixel_normals.shape[0] if isinstance(pixel_normals, torch.Tensor) and pixel_normals.dim() == 2 else -1
    if not isinstance(shininess, torch.Tensor):
        shininess = torch.as_tensor(float(shininess), dtype=torch.float32, device=light_colors.device)
    if shininess.numel() != 1 and tuple(shininess.shape) != (NP,):
        raise ValueError(f"shininess must be a float, one value or [{NP}] (one per pixel), got {tuple(shininess.shape)}")
    dirs = _shared_grid(light_dirs)
    need_ds = bool(shininess.requires_grad and torch.is_grad_enabled())  # T = dS/ds only when somebody will ask for it
    fn = _ShadeTermsNormalsFn if differentiable_normals else _ShadeTermsFn
    return fn.apply(light_colors, shininess, pixel_normals, pixel_positions, cam, dirs, _constant_mask(vis, NP, dirs), need_ds)


def shade_terms(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, shininess, vis=None):
    """(D, S), each [B, NP, 3]: the diffuse sum D = sum_j nl C and the specular sum S = sum_j nh^s_p C of the shader, kept
    apart and without kd, ks and norm(s), for a shininess per pixel (a float, one value or [NP]; every value > 0).
    ``compose_materials`` turns them into colours.  Differentiable with respect to ``envmap.environment_map`` and
    ``shininess``; normals, positions, camera, directions and the mask are constants (one that requires grad raises)."""
    return _shade_terms(envmap.environment_map, envmap.directions, pixel_normals, pixel_positions, camera_center, shininess, vis)


def shade_terms_normals(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, shininess, vis=None):
    """``shade_terms`` whose ``pixel_normals`` may require grad (normal-mapped materials, ``textures.perturb_normals``): the
    same forward kernel and the same gradients for the map and the shininess, plus d loss / d pixel_normals through
    ``ops.envmap_shade_terms_dnormals`` (the normalisation's Jacobian included; strict gates, so a zero normal gets exactly
    0).  Positions, camera, directions and the mask stay constants."""
    return _shade_terms(envmap.environment_map, envmap.directions, pixel_normals, pixel_positions, camera_center, shininess, vis,
                        differentiable_normals=True)


def specular_norm(shininess: torch.Tensor) -> torch.Tensor:
    """norm(s) = (s + 2) / (4 (2 - exp(-s / 2))), the reference's energy normalisation of the lobe (:112-114)."""
    return (shininess + 2.0) / (4.0 * (2.0 - torch.exp(-shininess / 2.0)))


def compose_materials(D: torch.Tensor, S: torch.Tensor, albedo, ks, shininess) -> torch.Tensor:
    """colours [B, NP, 3] = albedo D + ks norm(s) S from the terms of ``shade_terms``.  albedo: a float, [3] or [NP, 3];
    ks and shininess: a float, one value or [NP].  Plain torch (any device, any float dtype): its autograd gives the
    gradients of albedo and ks and the norm'(s) part of the shininess's."""
    if not isinstance(D, torch.Tensor) or D.dim() != 3 or D.shape[-1] != 3 or S.shape != D.shape:
        raise ValueError("D and S must be [B, NP, 3]")
    NP = D.shape[1]

    def per_pixel(x, name):
        x = torch.as_tensor(x, dtype=D.dtype, device=D.device) if not isinstance(x, torch.Tensor) else x.to(D.dtype)
        if x.numel() == 1:
            return x.reshape(1, 1)
        if tuple(x.shape) != (NP,):
            raise ValueError(f"{name} must be a float, one value or [{NP}] (one per pixel), got {tuple(x.shape)}")
        return x.reshape(NP, 1)

    a = torch.as_tensor(albedo, dtype=D.dtype, device=D.device) if not isinstance(albedo, torch.Tensor) else albedo.to(D.dtype)
    if a.numel() != 1 and tuple(a.shape) not in ((3,), (NP, 3)):
        raise ValueError(f"albedo must be a float, [3] or [{NP}, 3], got {tuple(a.shape)}")
    if a.numel() == 1:
        a = a.reshape(1)
    return a * D + (per_pixel(ks, "ks") * specular_norm(per_pixel(shininess, "shininess"))) * S


def blinn_phong_shading_materials(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, albedo, ks,
                                  shininess, vis=None, differentiable_normals: bool = False) -> torch.Tensor:
    """colours [B, NP, 3] with a material per pixel: ``compose_materials(*shade_terms(...), albedo, ks, shininess)``.
    Differentiable with respect to the environment map, albedo, ks and shininess, and, with ``differentiable_normals``
    (``shade_terms_normals``), the pixel normals."""
    terms = shade_terms_normals if differentiable_normals else shade_terms
    D, S = terms(pixel_normals, pixel_positions, camera_center, envmap, shininess, vis=vis)
    return compose_materials(D, S, albedo, ks, shininess)


class SpatialMaterials(nn.Module):
    """A Blinn-Phong material per render pixel.  albedo: a float, [3], [NP, 3] or [S, S, 3]; ks and shininess: a float,
    [NP] or [S, S].  The names in ``learn`` become Parameters (the caller owns their optimiser), the others buffers.  The
    shininess is clamped to [shininess_min, shininess_max] before use, so an optimiser cannot walk it out of the kernels'
    precondition s > 0.  ``values()`` -> (albedo, ks, shininess) flattened over the pixels, as the shading functions take
    them.  A per-vertex albedo needs no more than ``interpolate_face_attributes(frags.pix_to_face, frags.bary_coords,
    vertex_albedo[faces])`` as the albedo of ``compose_materials``."""

    NAMES = ("albedo", "ks", "shininess")

    def __init__(self, albedo=1.0, ks=0.0, shininess=500.0, learn=(), shininess_min: float = 1.0, shininess_max: float = 2000.0):
        super().__init__()
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for name in learn:
            if name not in self.NAMES:
                raise ValueError(f"learn names must be among {self.NAMES}, got {name!r}")
        if not 0.0 < float(shininess_min) <= float(shininess_max):
            raise ValueError("0 < shininess_min <= shininess_max is required")
        self.shininess_min, self.shininess_max = float(shininess_min), float(shininess_max)
        a = torch.as_tensor(albedo, dtype=torch.float32).detach().clone()
        if a.dim() == 3 and a.shape[0] == a.shape[1] and a.shape[2] == 3:
            a = a.reshape(-1, 3)
        if a.dim() > 2 or (a.dim() == 1 and a.shape[0] != 3) or (a.dim() == 2 and a.shape[1] != 3):
            raise ValueError(f"albedo must be a float, [3], [NP, 3] or [S, S, 3], got {tuple(a.shape)}")
        vals = {"albedo": a}
        for name, x in (("ks", ks), ("shininess", shininess)):
            x = torch.as_tensor(x, dtype=torch.float32).detach().clone()
            if x.dim() == 2 and x.shape[0] == x.shape[1]:
                x = x.reshape(-1)
            if x.dim() > 1:
                raise ValueError(f"{name} must be a float, [NP] or [S, S], got {tuple(x.shape)}")
            vals[name] = x
        sizes = {a.shape[0]} if a.dim() == 2 else set()
        sizes |= {vals[k].shape[0] for k in ("ks", "shininess") if vals[k].numel() > 1}
        if len(sizes) > 1:
            raise ValueError(f"the per-pixel materials disagree about the number of pixels: {sorted(sizes)}")
        for name, x in vals.items():
            if name in learn:
                setattr(self, name, nn.Parameter(x))
            else:
                self.register_buffer(name, x)

    def values(self):
        return self.albedo, self.ks, self.shininess.clamp(self.shininess_min, self.shininess_max)


class _ShadeGgxFn(torch.autograd.Function):
    """(D, S0, S1) of ``ops.envmap_shade_ggx``.  Gradients: the light colours through the backward kernel; alpha and the
    (un-normalised) pixel normals through the dpixel kernel, which runs only when one of them is asked for and computes the
    normals' gradient only when that one is."""

    @staticmethod
    def forward(ctx, light_colors, alpha, normals, positions, camera_center, light_dirs, vis):
        ctx.save_for_backward(normals, positions, camera_center, light_dirs, alpha, light_colors)
        ctx.vis = vis  # a constant of (mesh, camera, directions): see _constant_mask
        return ops.envmap_shade_ggx(normals, positions, camera_center, light_dirs, light_colors, alpha, vis=vis)

    @staticmethod
    def backward(ctx, gD, gS0, gS1):
        normals, positions, camera_center, light_dirs, alpha, light_colors = ctx.saved_tensors
        gC = ga = gn = None
        gD, gS0, gS1 = gD.contiguous(), gS0.contiguous(), gS1.contiguous()
        if ctx.needs_input_grad[0]:
            gC = ops.envmap_shade_ggx_backward(normals, positions, camera_center, light_dirs, gD, gS0, gS1, alpha, vis=ctx.vis)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            ga, gn = ops.envmap_shade_ggx_dpixel(normals, positions, camera_center, light_dirs, light_colors, gD, gS0, gS1, alpha,
                                                 vis=ctx.vis, need_dn=ctx.needs_input_grad[2])
            if ctx.needs_input_grad[1]:
                ga = (ga.sum() if alpha.numel() == 1 else ga).reshape(alpha.shape).to(alpha.dtype)
            else:
                ga = None
            if gn is not None:
                gn = gn.to(normals.dtype)
        return gC, ga, gn, None, None, None, None


def shade_terms_ggx(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, alpha, vis=None):
    """(D, S0, S1), each [B, NP, 3]: the diffuse sum and the two specular sums of the microfacet (GGX) material -- S0 =
    sum_j k C, S1 = sum_j k f C with k the GGX lobe x separable Smith x nl and f Schlick's (1 - V.H)^5 -- for an alpha
    (= roughness^2) per pixel (a float, one value or [NP]; every value > 0).  ``compose_microfacet`` turns them into colours.
    Differentiable with respect to ``envmap.environment_map``, ``alpha`` and ``pixel_normals``; positions, camera, directions
    and the mask are constants (one that requires grad raises)."""
    _constant("the pixel positions", pixel_positions)
    _constant("the light directions", envmap.directions)
    cam = torch.as_tensor(_constant("the camera centre", camera_center), dtype=torch.float32).reshape(-1)[:3].cpu()
    NP = pixel_normals.shape[0] if isinstance(pixel_normals, torch.Tensor) and pixel_normals.dim() == 2 else -1
    light_colors = envmap.environment_map
    if not isinstance(alpha, torch.Tensor):
        alpha = torch.as_tensor(float(alpha), dtype=torch.float32, device=light_colors.device)
    if alpha.numel() != 1 and tuple(alpha.shape) != (NP,):
        raise ValueError(f"alpha must be a float, one value or [{NP}] (one per pixel), got {tuple(alpha.shape)}")
    dirs = _shared_grid(envmap.directions)
    return _ShadeGgxFn.apply(light_colors, alpha, pixel_normals, pixel_positions, cam, dirs, _constant_mask(vis, NP, dirs))


def compose_microfacet(D: torch.Tensor, S0: torch.Tensor, S1: torch.Tensor, base_color, metallic,
                       f0_dielectric: float = 0.04) -> torch.Tensor:
    """colours [B, NP, 3] = (1 - metallic) base_color D + F0 S0 + (1 - F0) S1 with F0 = f0_dielectric (1 - metallic) +
    base_color metallic, from the terms of ``shade_terms_ggx``.  base_color: a float, [3] or [NP, 3]; metallic: a float, one
    value or [NP].  Plain torch (any device, any float dtype): its autograd gives the gradients of both."""
    if not isinstance(D, torch.Tensor) or D.dim() != 3 or D.shape[-1] != 3 or S0.shape != D.shape or S1.shape != D.shape:
        raise ValueError("D, S0 and S1 must be [B, NP, 3]")
    NP = D.shape[1]
    c = torch.as_tensor(base_color, dtype=D.dtype, device=D.device) if not isinstance(base_color, torch.Tensor) else base_color.to(D.dtype)
    if c.numel() != 1 and tuple(c.shape) not in ((3,), (NP, 3)):
        raise ValueError(f"base_color must be a float, [3] or [{NP}, 3], got {tuple(c.shape)}")
    if c.numel() == 1:
        c = c.reshape(1)
    m = torch.as_tensor(metallic, dtype=D.dtype, device=D.device) if not isinstance(metallic, torch.Tensor) else metallic.to(D.dtype)
    if m.numel() != 1 and tuple(m.shape) != (NP,):
        raise ValueError(f"metallic must be a float, one value or [{NP}] (one per pixel), got {tuple(m.shape)}")
    m = m.reshape(1, 1) if m.numel() == 1 else m.reshape(NP, 1)
    F0 = float(f0_dielectric) * (1.0 - m) + c * m
    return ((1.0 - m) * c) * D + F0 * S0 + (1.0 - F0) * S1


def microfacet_shading_materials(pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, base_color,
                                 roughness, metallic, vis=None, roughness_min: float = 0.1,
                                 f0_dielectric: float = 0.04) -> torch.Tensor:
    """colours [B, NP, 3] of a base-colour / roughness / metallic material per pixel:
    ``compose_microfacet(*shade_terms_ggx(..., alpha = clamp(roughness, roughness_min, 1)^2), base_color, metallic)``.
    Differentiable with respect to the environment map, the three material inputs and the pixel normals."""
    if not float(roughness_min) > 0.0:
        raise ValueError("roughness_min must be > 0")
    if not isinstance(roughness, torch.Tensor):
        roughness = torch.as_tensor(float(roughness), dtype=torch.float32, device=envmap.environment_map.device)
    r = roughness.clamp(float(roughness_min), 1.0)
    D, S0, S1 = shade_terms_ggx(pixel_normals, pixel_positions, camera_center, envmap, r * r, vis=vis)
    return compose_microfacet(D, S0, S1, base_color, metallic, f0_dielectric)


class MicrofacetMaterials(nn.Module):
    """A base-colour / roughness / metallic material per render pixel.  base_color: a float, [3], [NP, 3] or [S, S, 3];
    roughness and metallic: a float, [NP] or [S, S].  The names in ``learn`` become Parameters (the caller owns their
    optimiser), the others buffers.  ``values()`` -> (base_color, roughness, metallic) flattened over the pixels, the
    roughness clamped to [roughness_min, 1] and the metallic to [0, 1], so an optimiser cannot walk them out of the kernels'
    precondition alpha = roughness^2 > 0."""

    NAMES = ("base_color", "roughness", "metallic")

    def __init__(self, base_color=0.8, roughness=0.5, metallic=0.0, learn=(), roughness_min: float = 0.1,
                 f0_dielectric: float = 0.04):
        super().__init__()
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        for name in learn:
            if name not in self.NAMES:
                raise ValueError(f"learn names must be among {self.NAMES}, got {name!r}")
        if not 0.0 < float(roughness_min) <= 1.0:
            raise ValueError("0 < roughness_min <= 1 is required")
        self.roughness_min, self.f0_dielectric = float(roughness_min), float(f0_dielectric)
        a = torch.as_tensor(base_color, dtype=torch.float32).detach().clone()
        if a.dim() == 3 and a.shape[0] == a.shape[1] and a.shape[2] == 3:
            a = a.reshape(-1, 3)
        if a.dim() > 2 or (a.dim() == 1 and a.shape[0] != 3) or (a.dim() == 2 and a.shape[1] != 3):
            raise ValueError(f"base_color must be a float, [3], [NP, 3] or [S, S, 3], got {tuple(a.shape)}")
        vals = {"base_color": a}
        for name, x in (("roughness", roughness), ("metallic", metallic)):
            x = torch.as_tensor(x, dtype=torch.float32).detach().clone()
            if x.dim() == 2 and x.shape[0] == x.shape[1]:
                x = x.reshape(-1)
            if x.dim() > 1:
                raise ValueError(f"{name} must be a float, [NP] or [S, S], got {tuple(x.shape)}")
            vals[name] = x
        sizes = {a.shape[0]} if a.dim() == 2 else set()
        sizes |= {vals[k].shape[0] for k in ("roughness", "metallic") if vals[k].numel() > 1}
        if len(sizes) > 1:
            raise ValueError(f"the per-pixel materials disagree about the number of pixels: {sorted(sizes)}")
        for name, x in vals.items():
            if name in learn:
                setattr(self, name, nn.Parameter(x))
            else:
                self.register_buffer(name, x)

    def values(self):
        return self.base_color, self.roughness.clamp(self.roughness_min, 1.0), self.metallic.clamp(0.0, 1.0)

    def shade(self, pixel_normals, pixel_positions, camera_center, envmap: EnvironmentMap, vis=None) -> torch.Tensor:
        """colours [B, NP, 3] of this material on a G-buffer (``microfacet_shading_materials`` with ``values()``)."""
        c, r, m = self.values()
        return microfacet_shading_materials(pixel_normals, pixel_positions, camera_center, envmap, c, r, m, vis=vis,
                                            roughness_min=self.roughness_min, f0_dielectric=self.f0_dielectric)


def blinn_phong_shading_env_map(device, meshes, fragments, envmap, cameras, materials, kd, ks):
    """Reference signature (:46-48).  Returns (colors [B,H,W,3], pixel_normals [B,H,W,3])."""
    verts = meshes.verts_packed()
    faces = meshes.faces_packed()
    vertex_normals = meshes.verts_normals_packed()
    pixel_positions = interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, verts[faces])
    pixel_normals = interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, vertex_normals[faces])
    if pixel_normals.shape[0] != 1 or pixel_normals.shape[3] != 1:
        raise ValueError("one mesh and one face per pixel, as in the reference (:80-81 'assume K = 1')")
    _, Hr, Wr, _, _ = pixel_normals.shape
    B = envmap.directions.shape[0]
    n_flat = pixel_normals[0, :, :, 0, :].reshape(Hr * Wr, 3).to(device)
    p_flat = pixel_positions[0, :, :, 0, :].reshape(Hr * Wr, 3).to(device)
    cam = cameras.get_camera_center().reshape(-1)[:3]
    envmap_dev = envmap
    if envmap.environment_map.device != torch.device(device) and str(envmap.environment_map.device) != str(device):
        envmap_dev = EnvironmentMap.__new__(EnvironmentMap)
        envmap_dev.directions = envmap.directions.to(device)
        envmap_dev.environment_map = envmap.environment_map.to(device)
    colors = blinn_phong_shading_gbuffer(n_flat, p_flat, cam, envmap_dev, materials.shininess, kd, ks)
    normals_out = torch.nn.functional.normalize(n_flat, p=2, dim=-1, eps=1e-6).reshape(1, Hr, Wr, 3).repeat(B, 1, 1, 1)
    return colors.reshape(B, Hr, Wr, 3), normals_out


class GBuffer:
    """A rasterised view held as data: what the reference's rasteriser + interpolation produce for its fixed mesh and
    camera (RENI_module.py:66-72).  Stands in for (meshes, fragments, cameras) where pytorch3d is absent."""

    def __init__(self, pixel_normals: torch.Tensor, pixel_positions: torch.Tensor, camera_center, image_size):
        Hr, Wr = (image_size, image_size) if isinstance(image_size, int) else image_size
        self.pixel_normals = pixel_normals.reshape(Hr * Wr, 3)
        self.pixel_positions = pixel_positions.reshape(Hr * Wr, 3)
        self.camera_center = torch.as_tensor(camera_center, dtype=torch.float32).reshape(-1)[:3]
        self.image_size = (Hr, Wr)

    def to(self, device):
        self.pixel_normals = self.pixel_normals.to(device)
        self.pixel_positions = self.pixel_positions.to(device)
        return self


class _Materials:
    def __init__(self, shininess=64.0):
        self.shininess = torch.as_tensor([float(shininess)])

    def to(self, device):
        return self


class BlinnPhongShaderEnvMap(nn.Module):
    """Per-pixel lighting by an environment map (reference :119-174)."""

    def __init__(self, device="cpu", cameras=None, envmap: EnvironmentMap = None, materials=None, kd=None, ks=None):
        super().__init__()
        self.envmap = envmap
        self.materials = materials if materials is not None else _Materials()
        self.cameras = cameras
        self.device = device
        self.kd = kd
        self.ks = ks

    def to(self, device):
        cameras = self.cameras
        if cameras is not None and hasattr(cameras, "to"):
            self.cameras = cameras.to(device)
        if hasattr(self.materials, "to"):
            self.materials = self.materials.to(device)
        if self.envmap is not None:
            self.envmap = self.envmap.to(device)
        self.device = device
        return self

    def forward(self, fragments, meshes, envmap: EnvironmentMap, **kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass of BlinnPhongShader")
        materials = kwargs.get("materials", self.materials)
        return blinn_phong_shading_env_map(device=self.device, meshes=meshes, fragments=fragments, envmap=envmap,
                                           cameras=cameras, materials=materials, kd=self.kd, ks=self.ks)


class GBufferRenderer(nn.Module):
    """``renderer(envmap=...) -> (render [B,Hr,Wr,3], pixel_normals)`` over a fixed G-buffer: the call shape of the
    reference's MeshRenderer in ``RENI.get_render`` (RENI_module.py:393-396) without the rasteriser."""

    def __init__(self, gbuffer: GBuffer, kd: float, shininess: float = 500.0):
        super().__init__()
        self.gbuffer = gbuffer
        self.kd = kd
        self.ks = 1.0 - kd               # :199
        self.shininess = shininess       # Materials(shininess=500), :186

    def forward(self, envmap: EnvironmentMap = None, **kwargs):
        g = self.gbuffer
        dev = envmap.environment_map.device
        if g.pixel_normals.device != dev:
            g.to(dev)
        B = envmap.environment_map.shape[0]
        Hr, Wr = g.image_size
        colors = blinn_phong_shading_gbuffer(g.pixel_normals, g.pixel_positions, g.camera_center, envmap, self.shininess,
                                             self.kd, self.ks)
        normals = torch.nn.functional.normalize(g.pixel_normals, p=2, dim=-1, eps=1e-6).reshape(1, Hr, Wr, 3).repeat(B, 1, 1, 1)
        return colors.reshape(B, Hr, Wr, 3), normals


def build_renderer(obj_path, obj_rotation, img_size, kd, device):
    """Same signature and return value as the reference's ``build_renderer`` (:177-217): ``(renderer, R, T, mesh)`` with
    ``renderer(meshes_world=mesh, R=R, T=T, envmap=...)`` -> ``(render, pixel_normals)``.  pytorch3d does the mesh
    loading and the one rasterisation; the shading is this module's HIP path.  Without pytorch3d use
    ``GBufferRenderer`` with a stored G-buffer."""
    try:
        import pytorch3d.renderer as p3r
        from pytorch3d.io import load_obj
        from pytorch3d.structures import Meshes
        from pytorch3d.transforms import RotateAxisAngle
    except ImportError as e:  # pytorch3d is absent from this image
        raise ImportError("build_renderer needs pytorch3d (mesh loading and rasterisation); with a stored G-buffer use "
                          "reni_amd.envmap_shader.GBufferRenderer instead") from e
    # pragma: no cover -- everything below needs pytorch3d
    verts, faces_idx, _ = load_obj(obj_path, load_textures=False, device=device)
    verts = RotateAxisAngle(obj_rotation, "Y", device=device).transform_points(verts).to(device)
    white = p3r.TexturesVertex(verts_features=torch.ones(1, verts.shape[0], 3, device=device))
    mesh = Meshes(verts=[verts], faces=[faces_idx.verts_idx.to(device)], textures=white)
    cameras = p3r.FoVPerspectiveCameras(device=device)
    shader = BlinnPhongShaderEnvMap(device=device, cameras=cameras, materials=p3r.Materials(shininess=500), kd=kd, ks=1.0 - kd)
    raster = p3r.MeshRasterizer(cameras=cameras, raster_settings=p3r.RasterizationSettings(
        image_size=img_size, blur_radius=0.0, faces_per_pixel=1, perspective_correct=False))
    R, T = p3r.look_at_view_transform(2.0, 0.0, 0.0, degrees=True, device=device)
    return p3r.MeshRenderer(rasterizer=raster, shader=shader), R, T, mesh
