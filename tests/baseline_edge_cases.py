"""Edge shapes of the SG, SH and diffuse kernels (reni_tu_baselines.hip, reni_tu_diffuse.hip): the case lists, the input
builders and the float64 references that tests/test_baseline_edges_cpu.py and tests/test_gpu_baseline_edges.py share.

Plain data on the CPU; nothing here touches a device.  Every builder is cached and deterministic: treat what it returns
as read-only.  A batch case of N maps is the first N maps of the builder's largest batch, so one float64 reference per
shape serves every N (the kernels' results are per map; the GPU file checks that separately)."""
import functools
import math

import numpy as np
import torch

from tests.test_baselines_cpu import np_sg_loss_grad, np_sg_render, np_sh_basis, np_solid_angle

# ---------------------------------------------------------------------------------------------- per-map error measures
def _blocks(a, b):
    return np.asarray(a, np.float64).reshape(len(b), -1), np.asarray(b, np.float64).reshape(len(b), -1)


def per_map_rel(a, b):
    """[N]: max |a - b| / max |b| of each map (tests/test_baselines_cpu.py's rel, map by map)"""
    a, b = _blocks(a, b)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-30)


def per_map_rel_l2(a, b):
    """[N]: ||a - b|| / ||b|| of each map (rel_l2, map by map)"""
    a, b = _blocks(a, b)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


def per_map_max_over_norm(a, b):
    """[N]: max |a - b| / ||b|| of each map (the SH projection's measure in tests/test_gpu_baselines.py)"""
    a, b = _blocks(a, b)
    return np.abs(a - b).max(axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


# ---------------------------------------------------------------------------------------------- spherical harmonics
# Q = H W = 2, 8, 18, 50, 162, 578, 2178: never a multiple of the reconstruction wave's 128 pixels, below and above it
SH_WIDTHS = (2, 4, 6, 10, 18, 34, 66)
# T = 1, 4, 25, 36, 64, 81, 121, 144, 256: full and nearly full MT = 1, 2 tiles, the first MT = 4 and MT = 8 shapes
SH_LMAX = (0, 1, 4, 5, 7, 8, 10, 11, 15)
# 3 N = 3, 30, 33, 63, 66: column blocks with 3, 30, 1 + 32, 31 + 32 and 2 + 64 live columns
SH_N = (1, 10, 11, 21, 22)
SH_CASES = tuple((W, lmax, N) for W in SH_WIDTHS for lmax in SH_LMAX for N in SH_N)
SH_NMAX = max(SH_N)


@functools.lru_cache(maxsize=None)
def sh_images(W):
    """[SH_NMAX, W / 2, W, 3] float32, all positive with a large DC term"""
    gen = torch.Generator().manual_seed(1000 + W)
    return torch.rand(SH_NMAX, W // 2, W, 3, generator=gen) * 3


@functools.lru_cache(maxsize=None)
def sh_coeffs(lmax):
    """[SH_NMAX, (lmax + 1)^2, 3] float32"""
    gen = torch.Generator().manual_seed(2000 + lmax)
    return torch.randn(SH_NMAX, (lmax + 1) ** 2, 3, generator=gen)


@functools.lru_cache(maxsize=None)
def sh_reference(W, lmax):
    """float64 (coeffs [SH_NMAX, T, 3] of sh_images(W), maps [SH_NMAX, W / 2, W, 3] of sh_coeffs(lmax))"""
    imgs, cs = sh_images(W).numpy().astype(np.float64), sh_coeffs(lmax).numpy().astype(np.float64)
    Y = np_sh_basis(W, lmax)  # np_sh_project and np_sh_reconstruct of every map, with the basis built once
    return np.einsum("nyxc,yxt,y->ntc", imgs, Y, np_solid_angle(W)), np.einsum("yxt,ntc->nyxc", Y, cs)


# ---------------------------------------------------------------------------------------------- spherical Gaussians
# (N, H, W, SGRow, SGCol)
SG_CASES = (
    (1, 1, 1, 1, 1),
    (5, 3, 5, 8, 8),
    (6, 7, 9, 7, 9),
    (3, 1, 65, 2, 6),
    (2, 13, 59, 1, 2),
    (5, 24, 32, 2, 6),      # 768 px: the last LDS shape
    (3, 1, 769, 1, 1),      # the first workspace shape
    (2049, 25, 31, 1, 2),   # 775 px, 513 groups over 512 workgroups: workgroup 0's second group has one live wave
)
SG_WEIGHT_KINDS = ("broadcast", "contiguous", "sliced")


@functools.lru_cache(maxsize=None)
def sg_inputs(case):
    """(raw [N, K, 6], env [N, 3, H, W]) float32, as test_sg_gradient_against_float64_autograd draws them"""
    N, H, W, R, C = case
    K = R * C
    gen = torch.Generator().manual_seed(3000 + SG_CASES.index(case))
    raw = torch.randn(N, K, 6, generator=gen) * 0.7
    raw[0, 0, 3], raw[-1, K - 1, 4], raw[0, K // 2, 3] = 3.0, -3.5, -2.5  # near tanh saturation
    raw[..., 5] += float(np.log(np.pi / R))
    env = torch.rand(N, 3, H, W, generator=gen) * 4
    return raw, env


@functools.lru_cache(maxsize=None)
def _sg_weight_base(case, kind):
    N, H, W, R, C = case
    gen = torch.Generator().manual_seed(4000 + 10 * SG_CASES.index(case) + SG_WEIGHT_KINDS.index(kind))
    shape = {"broadcast": (1, 1, H, W), "contiguous": (N, 3, H, W), "sliced": (N, 3, 2 * H, 3 * W + 1)}[kind]
    return torch.rand(*shape, generator=gen) + 0.1


def sg_weight(case, kind, device=None):
    """The case's weight as a [N, 3, H, W] view: a stride-0 broadcast of [1, 1, H, W], a contiguous tensor, or the slice
    [:, :, ::2, 1::3] of a larger one (strides (6 H (3 W + 1), 2 H (3 W + 1), 2 (3 W + 1), 3)).  The storage is moved to
    `device` before the view is taken, so the view keeps its strides there."""
    N, H, W, R, C = case
    base = _sg_weight_base(case, kind)
    if device is not None:
        base = base.to(device)
    if kind == "broadcast":
        return base.expand(N, 3, H, W)
    if kind == "sliced":
        base = base[:, :, ::2, 1::3]
    assert tuple(base.shape) == (N, 3, H, W)
    return base


@functools.lru_cache(maxsize=None)
def sg_reference(case, kind):
    """float64 (total, per-map loss [N], gradient [N, K, 6]) of the case with this weight kind"""
    N, H, W, R, C = case
    raw, env = sg_inputs(case)
    return np_sg_loss_grad(raw.numpy(), env.numpy(), sg_weight(case, kind).numpy(), R, C)


@functools.lru_cache(maxsize=None)
def sg_render_reference(case):
    """float64 render [N, 3, H, W]"""
    N, H, W, R, C = case
    return np_sg_render(sg_inputs(case)[0].numpy(), R, C, H, W)


# ---------------------------------------------------------------------------------------------- diffuse convolution
# Q = 1, 2, 3: the main loop runs 0, 1, 1 times, the odd tail 1, 0, 1 times; P = 1, 31: one workgroup with idle waves;
# 33: two output tiles of one wave; 257: a second workgroup with one live row.  4095 / 4096 / 4097: the split boundary
# (no split and an odd tail; two even chunks; chunks of 2050 and 2047)
DF_SHAPES = tuple((P, Q) for P in (1, 31, 33, 257) for Q in (1, 2, 3)) + ((1, 4095), (1, 4096), (33, 4097))
DF_N = (1, 10, 11, 21, 22)  # 3 N = 3, 30 (CT = 1); 33, 63, 66 (CT = 2, the second tile with 1 live column at 33 and 66)
DF_CASES = tuple((P, Q, N) for P, Q in DF_SHAPES for N in DF_N)
DF_NMAX = max(DF_N)


def _unit(gen, n):
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True)).float()


def np_clamped_cosine(src, in_dirs, w, out_dirs, scale=1.0 / math.pi):
    """E [N, P, 3] = scale sum_i max(0, out . in_i) w_i src[n, i, c] in float64 (tests/test_gpu_diffuse.py's _ref64)"""
    A = np.maximum(0.0, np.asarray(out_dirs, np.float64) @ np.asarray(in_dirs, np.float64).T) * np.asarray(w, np.float64)
    return np.einsum("pq,nqc->npc", A, np.asarray(src, np.float64)) * scale


@functools.lru_cache(maxsize=None)
def df_inputs(P, Q):
    """(src [DF_NMAX, Q, 3], in_dirs [Q, 3], in_weight [Q], out_dirs [P, 3]) float32 and the float64 result
    [DF_NMAX, P, 3].  Random unit directions, drawn again until every map's float64 maximum is positive (an
    all-back-facing draw, likely at P = 1, Q = 1, would leave a comparison with nothing to compare) and the first and
    the last texel each light some output at a cosine above 0.5: the last one is the odd tail's, and with P = 1 it faces away from the one
    output direction in every other draw, where a kernel that dropped it would go unnoticed."""
    for attempt in range(256):
        gen = torch.Generator().manual_seed(5000 + 97 * DF_SHAPES.index((P, Q)) + 7919 * attempt)
        in_dirs, out_dirs = _unit(gen, Q), _unit(gen, P)
        w = torch.rand(Q, generator=gen) * (4 * math.pi / Q)
        src = torch.rand(DF_NMAX, Q, 3, generator=gen) * 3
        ref = np_clamped_cosine(src.numpy(), in_dirs.numpy(), w.numpy(), out_dirs.numpy())
        cos = out_dirs.double().numpy() @ in_dirs.double().numpy()[[0, -1]].T  # [P, 2]
        if ref.reshape(DF_NMAX, -1).max(axis=1).min() > 0 and cos.max(axis=0).min() > 0.5:
            return src, in_dirs, w, out_dirs, ref
    raise AssertionError(f"no front-facing draw for P = {P}, Q = {Q}")
