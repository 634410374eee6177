"""Host-side tables of the device resampler and blur (reni_tu_resample.hip: reni_resample, reni_gaussian_blur).

The kernels know no interpolation mode: they gather through index / weight tables.  Everything that decides a result --
source coordinates, tap indices, weights -- is computed here in exact integers or float64 and rounded to fp32 once, as the
separable SH tables are (baselines.sh_tables).  Evaluating ``scale (d + 0.5) - 0.5`` in fp32 on the device would make the
weights depend on FMA contraction.

All four modes use half-pixel centres: the source coordinate of output sample d is

    x = (2 d + 1) n_in / (2 n_out) - 1/2 = num / den,    num = (2 d + 1) n_in - n_out,  den = 2 n_out    (exact integers)

  nearest    1 tap   index = min(floor(fp32(d) fp32(n_in / n_out)), n_in - 1), the product in fp32: torchvision's NEAREST as
                     utils.mask_from_array restates it (NOT the half-pixel formula, and not the exact integer floor either)
  bilinear   2 taps  num clamped to >= 0, upper index clamped: F.interpolate(mode="bilinear", align_corners=False) without
                     antialiasing, which is what custom_transforms.Resize computes
  bicubic    4 taps  offsets -1 .. +2, Keys kernel with A = -0.75, coordinate not clamped, indices clamped (replicated border),
                     no antialiasing when shrinking: cv2 INTER_CUBIC on float images, torch's bicubic
  lanczos4   8 taps  offsets -3 .. +4, sinc(t) sinc(t / 4) normalised to sum 1, replicated border: cv2 INTER_LANCZOS4
"""
from __future__ import annotations

import math

import numpy as np
import torch

MODES = ("nearest", "bilinear", "bicubic", "lanczos4")
TAPS = {"nearest": 1, "bilinear": 2, "bicubic": 4, "lanczos4": 8}
CUBIC_A = -0.75


def cubic_weights(t):
    """Keys' cubic convolution weights (A = -0.75) of the taps at offsets -1, 0, +1, +2 for the fraction t in [0, 1)."""
    A = CUBIC_A

    def near(x):  # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def far(x):  # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

    return np.asarray([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], np.float64)


def lanczos4_weights(t):
    """sinc(x) sinc(x / 4) at the taps' distances x = t + 3 - k (k = 0 .. 7, offsets -3 .. +4), normalised to sum 1.
    At t = 0 the vector is exactly (0, 0, 0, 1, 0, 0, 0, 0)."""
    if t == 0:
        w = np.zeros(8, np.float64)
        w[3] = 1.0
        return w
    x = float(t) + 3.0 - np.arange(8, dtype=np.float64)
    w = np.sin(np.pi * x) / (np.pi * x) * (np.sin(np.pi * x / 4.0) / (np.pi * x / 4.0))
    return w / w.sum()


def resample_tables(n_in: int, n_out: int, mode: str):
    """(indices int64 [n_out, taps], weights float64 [n_out, taps]) of one axis resampled from n_in to n_out samples."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample_tables: sizes must be >= 1, got {n_in} -> {n_out}")
    if mode not in MODES:
        raise ValueError(f"resample_tables: mode must be one of {MODES}, got {mode!r}")
    taps = TAPS[mode]
    idx = np.zeros((n_out, taps), np.int64)
    w = np.zeros((n_out, taps), np.float64)
    if mode == "nearest":
        prod = np.arange(n_out, dtype=np.float32) * np.float32(n_in / n_out)  # fp32 product, as torchvision's kernel has it
        idx[:, 0] = np.minimum(np.floor(prod).astype(np.int64), n_in - 1)
        w[:, 0] = 1.0
        return idx, w
    den = 2 * n_out
    for d in range(n_out):
        num = (2 * d + 1) * n_in - n_out
        if mode == "bilinear":
            num = max(num, 0)
        i0 = num // den  # floor, also below zero
        t = (num - i0 * den) / den
        if mode == "bilinear":
            idx[d] = (min(i0, n_in - 1), min(i0 + 1, n_in - 1))
            w[d] = (1.0 - t, t)
        elif mode == "bicubic":
            idx[d] = np.clip(i0 - 1 + np.arange(4), 0, n_in - 1)
            w[d] = cubic_weights(t)
        else:
            idx[d] = np.clip(i0 - 3 + np.arange(8), 0, n_in - 1)
            w[d] = lanczos4_weights(t)
    return idx, w


def gaussian_weights(sigma: float):
    """(weights float64 [2 r + 1], r) of scipy.ndimage.gaussian_filter's kernel: r = int(4 sigma + 0.5) (truncate = 4),
    exp(-x^2 / 2 sigma^2) normalised to sum 1."""
    sigma = float(sigma)
    if not sigma > 0 or not math.isfinite(sigma):
        raise ValueError(f"gaussian_weights: sigma must be positive and finite, got {sigma}")
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), r


def reflect_indices(n: int, r: int):
    """[n, 2 r + 1] source indices of the taps under scipy's `reflect` boundary (d c b a | a b c d | d c b a, period 2 n)."""
    i = np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :]
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


_DEVICE_TABLES = {}


def device_tables(n_in: int, n_out: int, mode: str, device):
    """(indices int32 [n_out, taps], weights fp32 [n_out, taps]) on ``device``, cached per (n_in, n_out, mode, device)."""
    device = torch.device(device)
    key = (int(n_in), int(n_out), mode, device)
    t = _DEVICE_TABLES.get(key)
    if t is None:
        idx, w = resample_tables(n_in, n_out, mode)
        t = (torch.from_numpy(idx.astype(np.int32)).to(device), torch.from_numpy(w.astype(np.float32)).to(device))
        if len(_DEVICE_TABLES) >= 256:  # a curriculum touches a handful; a stream of odd sizes must not grow without bound
            _DEVICE_TABLES.clear()
        _DEVICE_TABLES[key] = t
    return t
