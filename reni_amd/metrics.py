"""Scores of environment maps: error sums, PSNR and SSIM of a prediction against a target, on the device.

Everything that touches pixels is one of two fused HIP calls (reni_tu_metrics.hip): ``ops.pair_stats`` reads both images once
and returns eight sums per image, ``ops.ssim`` returns the mean SSIM per image.  Both read the images where they are -- a
dataset batch [B, 3, H, W], a model output [B, P, 3] -- and map them into the space a score is defined in while the numbers
are in registers:

    "stored"   the numbers as given (normalised log radiance for an HDR dataset: what the loss sees)
    "linear"   radiance, UnMinMaxNormlise(minmax)
    "srgb"     what a viewer shows: linear / exposure, clamped to [0, 1], the sRGB curve.  The exposure is the target's
               (``exposure``: the nested 0.98-quantile ``utils.sRGB`` divides by) and is applied to both images.

Definitions (w_i the pixel weight, p and t the mapped prediction and target, sums over pixels i and the 3 channels c):

    weighted_mse = sum w (p - t)^2 / (3 sum w)        mae = sum w |p - t| / (3 sum w)
    cosine       = sum w cos(p_i, t_i) / sum w        (the RGB-vector cosine of F.cosine_similarity, eps 1e-20)
    psnr         = 10 log10(peak^2 / weighted_mse)    peak: a number, "target_max" or "target_range" (max - min) of the mapped
                                                      target over the pixels with w > 0
    ssim         Wang et al. 2004, 11 x 11 Gaussian window (sigma 1.5), per channel, channels averaged.  sphere=True: windows
                 wrap in longitude and cross the poles by the rule of ``rotation.py``, weighted mean over all pixels;
                 sphere=False: the published image definition (windows inside the image, unweighted).

Equirectangular pixels are not equal areas: ``solid_angle_weight(H)`` is sin(phi) per row, an [H, 1] tensor that the kernels
broadcast through zero strides.  There is no CPU fallback: a CPU tensor raises ``RENILibraryError``; bad shapes and arguments
raise ``ValueError`` before the library is touched.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

SPACES = ("stored", "linear", "srgb")
SCORES = ("wmse_stored", "cosine_stored", "psnr_linear", "psnr_srgb", "ssim_srgb")
DEFAULT_PEAK = {"srgb": 1.0, "linear": "target_max", "stored": "target_range"}
_SIN_ROWS = {}  # (H, device) -> solid_angle_weight: a function of its key alone


def gaussian_window(size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The SSIM window's weights along one axis, float64, normalised to sum 1 (the library rounds them to fp32 once)."""
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def solid_angle_weight(H: int, device=None) -> torch.Tensor:
    """sin(phi) of the H pixel rows, [H, 1] float32 (float64 rounded once): the solid angle of a pixel up to a constant."""
    phi = np.pi * (np.arange(int(H), dtype=np.float64) + 0.5) / int(H)
    return torch.from_numpy(np.sin(phi).astype(np.float32)).reshape(int(H), 1).to(device if device is not None else "cpu")


def exposure(target: torch.Tensor, minmax=None, size=None) -> torch.Tensor:
    """[B]: the nested 0.98-quantile (channels, rows, columns) ``utils.sRGB`` divides the LINEAR target by.  minmax: the target
    is stored normalised and is un-normalised first (on the device through reni_unnormalise_srgb, so the numbers are the
    ones the kernels see); None: it is linear already."""
    t = ops._pair_args(target, target, None, size)[0]
    if minmax is not None:
        if t.is_cuda:
            t = ops.unnormalise_srgb(t, minmax, srgb=False)
        else:
            t = torch.exp(0.5 * (t + 1) * (float(minmax[1]) - float(minmax[0])) + float(minmax[0]))
    return torch.quantile(torch.quantile(torch.quantile(t, 0.98, dim=1), 0.98, dim=1), 0.98, dim=1)


def _peak(stats: torch.Tensor, peak) -> torch.Tensor:
    if isinstance(peak, str):
        if peak == "target_max":
            return stats[:, 4]
        if peak == "target_range":
            return stats[:, 4] - stats[:, 5]
        raise ValueError(f'peak must be a number, "target_max" or "target_range", got {peak!r}')
    if not float(peak) > 0:
        raise ValueError(f"peak must be > 0, got {peak}")
    return torch.full_like(stats[:, 0], float(peak))


def mse_from_stats(stats: torch.Tensor) -> torch.Tensor:
    return stats[:, 1] / (3.0 * stats[:, 0])


def psnr_from_stats(stats: torch.Tensor, peak) -> torch.Tensor:
    """10 log10(peak^2 / (SSE / (3 sum w))) from rows of ``ops.pair_stats`` [B, 8]; ``peak`` may also be a tensor [B]."""
    pk = peak if isinstance(peak, torch.Tensor) else _peak(stats, peak)
    return 10.0 * torch.log10(pk * pk / mse_from_stats(stats))


def _check_peak(peak, space):
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, got {space!r}")
    peak = DEFAULT_PEAK[space] if peak is None else peak
    if isinstance(peak, str):
        if peak not in ("target_max", "target_range"):
            raise ValueError(f'peak must be a number, "target_max" or "target_range", got {peak!r}')
    elif not float(peak) > 0:
        raise ValueError(f"peak must be > 0, got {peak}")
    return peak


def _stats(pred, target, space, minmax, weight, size=None, expo=None):
    if space == "srgb" and expo is None:
        if minmax is None:
            raise ValueError("space='srgb' maps the stored numbers back to radiance and needs minmax")
        ops._pair_args(pred, target, weight, size)  # shapes first: a bad pair raises before anything is computed
        expo = exposure(target, minmax, size)
    return ops.pair_stats(pred, target, weight, space, minmax, expo, size)


def weighted_mse(pred, target, space="stored", minmax=None, weight=None, size=None) -> torch.Tensor:
    """[B]: sum w (p - t)^2 / (3 sum w) in ``space``."""
    return mse_from_stats(_stats(pred, target, space, minmax, weight, size))


def mae(pred, target, space="stored", minmax=None, weight=None, size=None) -> torch.Tensor:
    """[B]: sum w |p - t| / (3 sum w) in ``space``."""
    s = _stats(pred, target, space, minmax, weight, size)
    return s[:, 2] / (3.0 * s[:, 0])


def cosine(pred, target, space="stored", minmax=None, weight=None, size=None) -> torch.Tensor:
    """[B]: the weighted mean of the RGB-vector cosine between prediction and target pixels."""
    s = _stats(pred, target, space, minmax, weight, size)
    return s[:, 3] / s[:, 0]


def psnr(pred, target, space="srgb", minmax=None, weight=None, peak=None, size=None) -> torch.Tensor:
    """[B]: 10 log10(peak^2 / weighted_mse).  peak: a number, "target_max" or "target_range"; default 1.0 in "srgb",
    "target_max" in "linear", "target_range" in "stored"."""
    peak = _check_peak(peak, space)
    return psnr_from_stats(_stats(pred, target, space, minmax, weight, size), peak)


def ssim(pred, target, space="srgb", minmax=None, weight=None, L=None, sphere=True, return_map=False, size=None):
    """[B] (and the map [B, H, W] with return_map): mean SSIM in ``space``.  L, the dynamic range of C1 = (0.01 L)^2 and
    C2 = (0.03 L)^2: default 1 in "srgb" and 2 in "stored" ([-1, 1]); "linear" has no natural range and needs one."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, got {space!r}")
    if L is None:
        if space == "linear":
            raise ValueError("space='linear' needs L, the dynamic range the SSIM constants are scaled by")
        L = 1.0 if space == "srgb" else 2.0
    expo = None
    if space == "srgb":
        if minmax is None:
            raise ValueError("space='srgb' maps the stored numbers back to radiance and needs minmax")
        p, _, w = ops._pair_args(pred, target, weight, size)
        if not sphere and w is not None:
            raise ValueError("the planar SSIM is the unweighted published definition: pass no weight (or sphere=True)")
        if sphere and p.shape[-1] % 2:
            raise ValueError(f"SSIM on the sphere needs an even width, got {p.shape[-1]}")
        expo = exposure(target, minmax, size)
    return ops.ssim(pred, target, weight, space, minmax, expo, L, sphere, return_map, size)


def _mask_hw(mask, B, H, W):
    """an inpainting mask ([1 | B, P, 3] of utils.get_mask, or anything that broadcasts to [B, H, W]) as a view [1 | B, H, W]"""
    m = mask if mask.dtype == torch.float32 else mask.float()
    if m.dim() == 3 and m.shape[2] == 3 and m.shape[1] == H * W and m.shape[0] in (1, B):
        return m[..., 0].unflatten(1, (H, W))
    try:
        torch.broadcast_to(m, (B, H, W))
    except RuntimeError:
        raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to [{B}, {H}, {W}]") from None
    return m


def score_maps(pred, target, minmax=None, mask=None, solid_angle=True, size=None) -> dict:
    """The evaluation's scores of every image, a dict of [B] float32 tensors:

        wmse_stored, cosine_stored            in the stored numbers (what the training loss measures)
        psnr_linear                           peak = the target's largest radiance           } only with ``minmax``
        psnr_srgb, ssim_srgb                  under the target's exposure, peak = L = 1      }

    solid_angle: weight pixels by sin(phi) (and take the SSIM on the sphere).  mask: 1 where the model saw the target, 0
    where it had to invent it ([1, P, 3] of ``utils.get_mask`` or anything that broadcasts to [B, H, W]); every score is then
    also reported over the seen pixels (``_seen``) and over the hidden ones (``_hidden``) -- the inpainting table.  The PSNR
    peaks of the two parts are the whole image's, so the three PSNRs differ by their errors alone.  The exposure is computed
    once, from the target: that writes ONE linear target image, which the three quantile passes of torch read (not the hot
    path).  Each space then costs one pass over the pair per weight, and the kernels write no mapped image."""
    p, t, _ = ops._pair_args(pred, target, None, size)
    B, _, H, W = p.shape
    if solid_angle and W % 2:
        raise ValueError(f"scores on the sphere need an even width, got {W}")
    dev = p.device
    base = None
    if solid_angle:
        base = _SIN_ROWS.get((H, str(dev)))
        if base is None:
            base = _SIN_ROWS.setdefault((H, str(dev)), solid_angle_weight(H, dev))
    weights = {"": base}
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise ValueError("mask must be a tensor")
        m = _mask_hw(mask.to(dev), B, H, W)
        if m.numel() and not bool(((m >= 0) & (m <= 1)).all()):  # the one read-back of a masked call; a NaN fails it too
            raise ValueError("mask values must lie in [0, 1]")
        weights["_seen"] = m * base if base is not None else m
        weights["_hidden"] = (1.0 - m) * base if base is not None else 1.0 - m
    out = {}
    expo = exposure(t, minmax) if minmax is not None else None
    whole = {}
    for suffix, w in weights.items():
        s = ops.pair_stats(p, t, w, "stored", check_weight=False)  # (sin >= 0, the mask is in [0, 1])
        out["wmse_stored" + suffix] = mse_from_stats(s)
        out["cosine_stored" + suffix] = s[:, 3] / s[:, 0]
        if minmax is None:
            continue
        for space in ("linear", "srgb"):
            s = ops.pair_stats(p, t, w, space, minmax, expo, check_weight=False)
            if suffix == "":
                whole[space] = s
            peak = 1.0 if space == "srgb" else whole[space][:, 4]
            out["psnr_" + space + suffix] = psnr_from_stats(s, peak)
        if solid_angle:
            out["ssim_srgb" + suffix] = ops.ssim(p, t, w, "srgb", minmax, expo, 1.0, sphere=True, check_weight=False)
        elif suffix == "":
            out["ssim_srgb"] = ops.ssim(p, t, None, "srgb", minmax, expo, 1.0, sphere=False)
    return out


def _dataset_info(dataset):
    if hasattr(dataset, "batch") and hasattr(dataset, "size"):
        H, W = dataset.size
    else:
        H, W = dataset[0][0].shape[-2:]
    un = getattr(dataset, "unnormalise", None)
    return int(H), int(W), getattr(un, "minmax", None)


def evaluate(model, dataset, idx=None, batch_size=16, mask=None, diffuse=False, minmax="dataset", glossy=None):
    """Score the model's reconstruction of dataset images: a forward pass at the dataset's resolution, ``score_maps`` against
    the dataset's images (``ResidentDataset.batch`` where the dataset is resident, ``dataset[i]`` otherwise).  idx: the
    images (default: all); latent i belongs to image i.  minmax: "dataset" takes ``dataset.unnormalise.minmax`` (None when
    the dataset has none: stored-space scores only).  diffuse=True adds ``diffuse_psnr``: psnr_linear (solid-angle weighted,
    peak = the target's largest irradiance) of ``baselines.irradiance_map`` of the linear prediction against that of the
    linear target.  glossy: a list of lobes (``glossy.phong / blinn / ggx``) adds ``glossy_psnr_<k>`` for lobe k, the same score
    of ``glossy.prefilter`` of the two.  Returns (table, means): dicts of [N] tensors and of 0-d tensors, on the model's device."""
    from .utils import get_directions
    H, W, ds_minmax = _dataset_info(dataset)
    if minmax == "dataset":
        minmax = ds_minmax
    if W != 2 * H:
        raise ValueError(f"the model is evaluated on its own H x 2H grid, the dataset is {H} x {W}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if diffuse and minmax is None:
        raise ValueError("diffuse=True compares irradiance, which needs linear radiance: no minmax to un-normalise with")
    glossy = list(glossy) if glossy is not None else []
    if glossy and minmax is None:
        raise ValueError("glossy= compares prefiltered radiance, which needs linear radiance: no minmax to un-normalise with")
    idx = list(range(len(dataset))) if idx is None else [int(i) for i in (idx.tolist() if isinstance(idx, torch.Tensor) else idx)]
    if not idx:
        raise ValueError("no images to evaluate")
    dev = next(model.parameters()).device
    ops._require_cuda(torch.empty(0, device=dev))
    D = get_directions(W).to(dev, torch.float32)
    rows = []
    with torch.no_grad():
        for k in range(0, len(idx), int(batch_size)):
            chunk = idx[k:k + int(batch_size)]
            sel = torch.tensor(chunk, dtype=torch.long, device=dev)
            if hasattr(dataset, "batch"):
                target = dataset.batch(chunk).to(dev)
            else:
                target = torch.stack([dataset[i][0] for i in chunk]).to(dev, torch.float32)
            pred = model(sel, D)  # [B, P, 3], scored in place
            row = score_maps(pred, target, minmax, mask, solid_angle=True, size=(H, W))
            if diffuse:
                from .baselines import irradiance_map
                lp = ops.unnormalise_srgb(pred.unflatten(1, (H, W)).permute(0, 3, 1, 2), minmax, srgb=False)
                lt = ops.unnormalise_srgb(target, minmax, srgb=False)
                ip = irradiance_map(lp.permute(0, 2, 3, 1).reshape(len(chunk), H * W, 3))
                it = irradiance_map(lt.permute(0, 2, 3, 1).reshape(len(chunk), H * W, 3))
                s = ops.pair_stats(ip, it, solid_angle_weight(H, dev), "stored", size=(H, W))
                row["diffuse_psnr"] = psnr_from_stats(s, "target_max")
            if glossy:
                from .glossy import prefilter
                lp = ops.unnormalise_srgb(pred.unflatten(1, (H, W)).permute(0, 3, 1, 2), minmax, srgb=False)
                lt = ops.unnormalise_srgb(target, minmax, srgb=False)
                gp = prefilter(lp.permute(0, 2, 3, 1).reshape(len(chunk), H * W, 3), glossy)  # [B, Lv, H W, 3]
                gt = prefilter(lt.permute(0, 2, 3, 1).reshape(len(chunk), H * W, 3), glossy)
                for j in range(len(glossy)):
                    s = ops.pair_stats(gp[:, j], gt[:, j], solid_angle_weight(H, dev), "stored", size=(H, W))
                    row[f"glossy_psnr_{j}"] = psnr_from_stats(s, "target_max")
            rows.append(row)
    table = {k: torch.cat([r[k] for r in rows]) for k in rows[0]}
    return table, {k: v.mean() for k, v in table.items()}


def equivariance_error(model, idx, R, mode="bilinear", width=64, minmax=None) -> dict:
    """How well turning the latent turns the map: ``score_maps(f(Z R^T, D), rotate_envmap(f(Z, D), R))`` for the latents of
    the images ``idx`` and one rotation R [3, 3] (checked; ``rotation.py`` states the convention) on the width/2 x width
    grid.  The turned prediction is the target.  With an exactly equivariant model what is left is the resampler's interpolation error (none for a
    whole-pixel yaw in "nearest" mode)."""
    from .rotation import check_rotation, rotate_latent
    from .utils import get_directions
    R = check_rotation(R)
    if R.dim() != 2:
        raise ValueError(f"one rotation [3, 3] is expected, got {tuple(R.shape)}")
    if int(width) < 10 or int(width) % 2:
        raise ValueError(f"width must be even and >= 10, got {width}")
    dev = next(model.parameters()).device
    ops._require_cuda(torch.empty(0, device=dev))
    sel = torch.as_tensor(idx, dtype=torch.long).reshape(-1).to(dev)
    Zt = getattr(model, "Z", None)
    Z = (Zt if Zt is not None else model.mu)[sel]
    with torch.no_grad():
        W = int(width)
        H = W // 2
        D = get_directions(W).to(dev, torch.float32)
        base = model(Z, D)
        turned = model(rotate_latent(Z, R.to(dev)), D)
        want = ops.rotate_envmap(base.unflatten(1, (H, W)), R.to(dev), mode, "hwc")
        return score_maps(turned, want, minmax, None, solid_angle=True, size=(H, W))
