"""Rotations of environment maps, latents and masks (not in the reference, which rotates latents only, in its tests).

Convention.  An equirectangular map has H rows and W columns (W even; W = 2 H for the project's maps, and the grid is then
``utils.get_directions(W)``): pixel (r, c) has phi = pi (r + 1/2) / H, theta = pi ((c + 1/2) / (W / 2) - 1) and direction
d = (sin phi sin theta, cos phi, -sin phi cos theta).  ``rotate_envmap(img, R)`` is the map turned by R:

    out(d) = img(R^T d)

With this sign, turning the map is the same as turning the latent of an equivariant model:
f(rotate_latent(Z, R), D) = rotate_envmap(f(Z, D), R), and ``rotation_y(k 2 pi / W)`` rolls the columns by -k.  The device side
is reni_tu_rotate.hip (``ops.rotate_envmap``); include/reni_hip.h states the sampling rule (bilinear / nearest on the sphere:
columns wrap, a row beyond a pole is the same row seen from the other side).

Rotation matrices are built in float64 and returned as fp32 [n, 3, 3]; everything here works on CPU tensors and on the device
except the two functions that resample (``rotate_envmap``, ``rotate_mask``), which need the GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

GROUPS = ("SO2", "SO3")


def grid_trig(H: int, W: int):
    """(row_trig [H, 2] = (sin phi, cos phi), col_trig [W, 2] = (sin theta, cos theta)) of the grid above, float64."""
    phi = np.pi * (np.arange(H, dtype=np.float64) + 0.5) / H
    theta = np.pi * ((np.arange(W, dtype=np.float64) + 0.5) / (W / 2.0) - 1.0)
    return np.stack((np.sin(phi), np.cos(phi)), 1), np.stack((np.sin(theta), np.cos(theta)), 1)


def rotation_y(angle, dtype=torch.float32) -> torch.Tensor:
    """Ry(angle) = [[cos, 0, sin], [0, 1, 0], [-sin, 0, cos]]: the yaw the SO2 encoding is invariant to.  angle: a number
    ([3, 3]) or a tensor [n] ([n, 3, 3]); computed in float64."""
    a = torch.as_tensor(angle, dtype=torch.float64)
    c, s, z, o = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    return torch.stack((c, z, s, z, o, z, -s, z, c), -1).reshape(a.shape + (3, 3)).to(dtype)


def random_rotations(n: int, group: str = "SO3", generator=None, device=None) -> torch.Tensor:
    """n rotations [n, 3, 3] fp32 drawn from ``generator``: "SO2" = Ry(angle uniform in [0, 2 pi)), "SO3" = uniform on the
    group (a normalised Gaussian quaternion).  The draw happens on the generator's device (``device`` without a generator)
    with device ops only: a device generator forces no host synchronisation."""
    if group not in GROUPS:
        raise ValueError(f"group must be one of {GROUPS}, got {group!r}")
    if int(n) < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    dev = generator.device if generator is not None else (torch.device(device) if device is not None else torch.device("cpu"))
    if group == "SO2":
        return rotation_y(2.0 * math.pi * torch.rand(int(n), dtype=torch.float64, device=dev, generator=generator))
    q = torch.randn(int(n), 4, dtype=torch.float64, device=dev, generator=generator)
    w, x, y, z = (q / q.norm(dim=1, keepdim=True).clamp_min(1e-300)).unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1)
    return R.reshape(int(n), 3, 3).float()


def check_rotation(R: torch.Tensor, tol: float = 1e-5) -> torch.Tensor:
    """R as fp32 [3, 3] or [n, 3, 3], or ValueError: wrong shape, |R R^T - I| > tol (not orthogonal) or det < 0 (a reflection).
    Reads R back to the host."""
    if not isinstance(R, torch.Tensor):
        R = torch.as_tensor(np.asarray(R))
    if R.dim() not in (2, 3) or tuple(R.shape[-2:]) != (3, 3):
        raise ValueError(f"a rotation is [3, 3] or [n, 3, 3], got {tuple(R.shape)}")
    M = R.detach().double().cpu().reshape(-1, 3, 3)
    if not bool(torch.isfinite(M).all()):
        raise ValueError("rotation matrix has non-finite entries")
    dev = float((M @ M.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max())
    if dev > tol:
        raise ValueError(f"not a rotation: max |R R^T - I| = {dev:.3e} > {tol:g}")
    if float(torch.linalg.det(M).min()) <= 0:
        raise ValueError("not a rotation: det R < 0 (a reflection)")
    return R.float()


def rotate_latent(Z: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """Z R^T for latents Z [N, ND, 3] (or [ND, 3]): every latent point turned by R ([3, 3] shared, or [N, 3, 3] per row)."""
    if Z.shape[-1] != 3 or tuple(R.shape[-2:]) != (3, 3) or R.dim() not in (2, 3):
        raise ValueError(f"expected Z [..., 3] and R [3, 3] or [N, 3, 3], got {tuple(Z.shape)} and {tuple(R.shape)}")
    if R.dim() == 3 and (Z.dim() != 3 or R.shape[0] != Z.shape[0]):
        raise ValueError(f"per-row rotations {tuple(R.shape)} do not match latents {tuple(Z.shape)}")
    return torch.matmul(Z, R.to(Z.dtype).transpose(-1, -2))


def rotate_envmap(imgs: torch.Tensor, R: torch.Tensor, mode: str = "bilinear", layout: str = "auto") -> torch.Tensor:
    """The maps ``imgs`` ([B, C, H, W], [C, H, W], [H, W]; channel-last with layout="hwc") turned by R ([3, 3], or [B, 3, 3]
    per image): out(d) = img(R^T d).  R is checked first (ValueError for a reflection or a matrix that is not orthogonal to
    1e-5), which reads it back to the host; a loop that builds its own matrices calls ``ops.rotate_envmap`` directly.
    No bicubic mode: HDR maps with a sun go negative under it."""
    from . import ops
    R = check_rotation(R)
    return ops.rotate_envmap(imgs, R.to(imgs.device), mode=mode, layout=layout)


def rotate_mask(mask: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """An inpainting mask [1, P, 3] (utils.get_mask; P = H 2H) turned with the map it belongs to: nearest sampling, so a
    mask in {0, 1} stays in {0, 1}.  Returns [1, P, 3]."""
    if mask.dim() != 3 or mask.shape[-1] != 3:
        raise ValueError(f"expected a mask [1, P, 3], got {tuple(mask.shape)}")
    n, P, _ = mask.shape
    H = math.isqrt(P // 2)
    if 2 * H * H != P:
        raise ValueError(f"P = {P} is not H x 2H")
    out = rotate_envmap(mask.reshape(n, H, 2 * H, 3), R, mode="nearest", layout="hwc")  # [n, 3, H, W]
    return out.permute(0, 2, 3, 1).reshape(n, P, 3)
