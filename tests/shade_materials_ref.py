"""float64 reference of the shader's terms path (per-pixel albedo, ks and shininess), in plain torch: the three sums of
reni_envmap_shade_terms and the composition behind them, restated the way oracle.blinn_phong_gbuffer states the scalar
shader.  Its autograd is the reference for every gradient of the feature.

    D[b,p,:] = sum_j v(p,j) nl(p,j)                C[b,j,:]
    S[b,p,:] = sum_j v(p,j) nh(p,j)^s_p            C[b,j,:]
    T[b,p,:] = sum_j v(p,j) nh(p,j)^s_p ln nh(p,j) C[b,j,:]        (a pair with nh = 0 adds 0)
    colours  = albedo D + ks norm(s) S,   norm(s) = (s + 2) / (4 (2 - exp(-s / 2)))
"""
import torch


def pair_terms(pixel_normals, pixel_positions, camera_center, light_directions, dtype=torch.float64):
    """nl, nh [NB, NP, J] for light_directions [NB, J, 3] (NB = 1: a shared grid), normalise-then-dot as the shader."""
    N = torch.nn.functional.normalize(pixel_normals.to(dtype), p=2, dim=-1, eps=1e-6)
    V = torch.nn.functional.normalize(camera_center.to(dtype)[None] - pixel_positions.to(dtype), p=2, dim=-1, eps=1e-6)
    L = light_directions.to(dtype)
    nl = torch.einsum("pk,bjk->bpj", N, L).clamp(0.0, 1.0)
    Hv = torch.nn.functional.normalize(V[None, :, None, :] + L[:, None, :, :], p=2, dim=-1, eps=1e-6)
    nh = torch.einsum("pk,bpjk->bpj", N, Hv).clamp(0.0, 1.0)
    return nl, nh


def shade_terms_ref(pixel_normals, pixel_positions, camera_center, light_directions, light_colors, shininess, vis=None,
                    dtype=torch.float64):
    """-> (D, S, T), each [B, NP, 3].  light_directions [1 | B, J, 3], light_colors [B, J, 3], shininess a float, a 0-d
    tensor or [NP] (may require grad), vis None or booleans [1 | B, NP, J]."""
    nl, nh = pair_terms(pixel_normals, pixel_positions, camera_center, light_directions, dtype)
    s = torch.as_tensor(shininess, dtype=dtype)
    s = s.reshape(1, -1, 1) if s.numel() > 1 else s.reshape(1, 1, 1)
    spec = nh ** s
    dspec = torch.where(nh > 0, spec * torch.log(nh.clamp_min(1e-300)), torch.zeros_like(spec))
    if vis is not None:
        v = vis.to(dtype)
        nl, spec, dspec = nl * v, spec * v, dspec * v
    C = light_colors.to(dtype)
    B = C.shape[0]
    return tuple(torch.einsum("bjk,bpj->bpk", C, m.expand(B, -1, -1)) for m in (nl, spec, dspec))


def specular_norm_ref(s):
    return (s + 2) / (4 * (2 - torch.exp(-s / 2)))


def specular_norm_ds_ref(s):
    """d norm / d s."""
    e = torch.exp(-s / 2)
    return 1 / (4 * (2 - e)) - (s + 2) * e / (8 * (2 - e) ** 2)


def compose_ref(D, S, albedo, ks, shininess):
    """colours [B, NP, 3]; albedo a float, [3] or [NP, 3]; ks, shininess a float, a 0-d tensor or [NP]."""
    dt = D.dtype
    a = torch.as_tensor(albedo, dtype=dt)
    k = torch.as_tensor(ks, dtype=dt)
    s = torch.as_tensor(shininess, dtype=dt)
    k = k.reshape(-1, 1) if k.numel() > 1 else k.reshape(1, 1)
    s = s.reshape(-1, 1) if s.numel() > 1 else s.reshape(1, 1)
    return a * D + k * specular_norm_ref(s) * S


def shininess_grad_bound(g, ks, shininess, S, T):
    """[NP]: sum_{b,c} |g| ks (|norm'(s_p)| |S| + norm(s_p) |T|), the magnitude of the two parts of the composed shininess
    gradient before they cancel (norm'(s) S and norm(s) T have opposite signs): the scale its error is measured against."""
    dt = S.dtype
    k = torch.as_tensor(ks, dtype=dt).reshape(-1, 1)
    s = torch.as_tensor(shininess, dtype=dt).reshape(-1, 1)
    m = g.abs().to(dt) * k * (specular_norm_ds_ref(s).abs() * S.abs() + specular_norm_ref(s) * T.abs())
    return m.sum(dim=(0, 2))
