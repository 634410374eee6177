"""CPU check of the edge-shape case list (tests/baseline_edge_cases.py): for every case, an fp32 evaluation of the
formula the HIP kernel computes must sit within a quarter of the bound tests/test_gpu_baseline_edges.py applies against the float64
restatement.  A case whose float64 reference is so ill-conditioned that plain fp32 arithmetic already uses up the bound
would make the GPU comparison say nothing about the kernel; it fails here first.

The fp32 evaluations: SH from the library's tables rounded to float32, every sum accumulated sequentially
(np.cumsum in float32), as the MFMA's k-ordered chain does; SG in torch float32 with the gradient by autograd; diffuse
in numpy float32 with pairwise sums over the texels."""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_edge_cases as E
from tests.test_baselines_cpu import np_sg_grid, rel, rel_l2

# the bounds of tests/test_gpu_baseline_edges.py
SH_PROJECT_TOL = 1e-5   # max |c - ref| / ||ref|| per map
SH_RECONSTRUCT_TOL = 1e-5  # rel per map
SG_LOSS_TOL = 1e-5      # relative, total and per map
SG_GRAD_TOL = 1e-5      # rel_l2, overall and per map
SG_RENDER_TOL = 2e-6    # rel
DIFFUSE_TOL = 1e-5      # rel per map

f32 = np.float32


def test_case_lists_hold_the_shapes_they_name():
    assert len(E.SH_CASES) == 7 * 9 * 5 and len(set(E.SH_CASES)) == len(E.SH_CASES)
    assert [W * (W // 2) for W in E.SH_WIDTHS] == [2, 8, 18, 50, 162, 578, 2178]
    assert [(l + 1) ** 2 for l in E.SH_LMAX] == [1, 4, 25, 36, 64, 81, 121, 144, 256]
    assert [3 * N for N in E.SH_N] == [3, 30, 33, 63, 66] == [3 * N for N in E.DF_N]
    assert len(E.SG_CASES) == 8 and [c[1] * c[2] for c in E.SG_CASES] == [1, 15, 63, 65, 767, 768, 769, 775]
    assert len(E.DF_SHAPES) == 15 and len(E.DF_CASES) == 75
    for case in E.SG_CASES:
        N, H, W, R, C = case
        want = {"broadcast": (0, 0, W, 1), "contiguous": (3 * H * W, H * W, W, 1),
                "sliced": (6 * H * (3 * W + 1), 2 * H * (3 * W + 1), 2 * (3 * W + 1), 3)}
        for kind in E.SG_WEIGHT_KINDS:
            w = E.sg_weight(case, kind)
            assert tuple(w.shape) == (N, 3, H, W)
            # the stride of a dimension of size 1 is never used
            assert [s for s, n in zip(w.stride(), w.shape) if n > 1] == [s for s, n in zip(want[kind], w.shape) if n > 1]


# ---------------------------------------------------------------------------------------------- spherical harmonics
@functools.lru_cache(maxsize=None)
def _sh_f32(W, lmax):
    """fp32 (coeffs, maps) of the largest batch: the basis as the product of the float32 tables, k-ordered sums"""
    from reni_amd import baselines
    imgs, cs = E.sh_images(W).numpy(), E.sh_coeffs(lmax).numpy()
    Q = W * (W // 2)
    row_s, col = baselines.sh_tables(W, lmax, True)
    row, _ = baselines.sh_tables(W, lmax, False)
    col = col.astype(f32)
    Ys = (row_s.astype(f32)[:, None, :] * col[None, :, :]).reshape(Q, -1)
    Y = (row.astype(f32)[:, None, :] * col[None, :, :]).reshape(Q, -1)
    coeffs = np.stack([np.cumsum(Ys[:, :, None] * im.reshape(Q, 1, 3), axis=0, dtype=f32)[-1] for im in imgs])
    maps = np.stack([np.cumsum(Y[:, :, None] * c[None, :, :], axis=1, dtype=f32)[:, -1].reshape(W // 2, W, 3) for c in cs])
    assert coeffs.dtype == f32 and maps.dtype == f32
    return coeffs, maps


@pytest.mark.parametrize("W", E.SH_WIDTHS)
def test_sh_cases_leave_room_for_the_kernel(W):
    for lmax in E.SH_LMAX:
        ref_c, ref_r = E.sh_reference(W, lmax)
        c, r = _sh_f32(W, lmax)
        err_c = E.per_map_max_over_norm(c, ref_c)
        err_r = E.per_map_rel(r, ref_r)
        for N in E.SH_N:  # a case of N maps is the first N of the largest batch
            assert (W, lmax, N) in E.SH_CASES
            assert err_c[:N].max() <= SH_PROJECT_TOL / 4, (W, lmax, N, err_c[:N].max())
            assert err_r[:N].max() <= SH_RECONSTRUCT_TOL / 4, (W, lmax, N, err_r[:N].max())


# ---------------------------------------------------------------------------------------------- spherical Gaussians
def _sg_rec_f32(raw, R, C, H, W):
    """renderSG in torch float32 from raw [N, K, 6] -> [N, 3, H W] (tests/test_gpu_baselines.py's torch_sg_loss)"""
    tc, pc, tr, pr, dirs = np_sg_grid(R, C, H, W)
    tc, pc, dirs = (torch.as_tensor(x, dtype=torch.float32) for x in (tc, pc, dirs))
    th = tr * torch.tanh(raw[..., 3]) + tc
    ph = pr * torch.tanh(raw[..., 4]) + pc
    axis = torch.stack([torch.sin(th) * torch.cos(ph), torch.sin(th) * torch.sin(ph), torch.cos(th)], -1)
    e = torch.exp(torch.exp(raw[..., 5])[..., None] * (axis @ dirs.T - 1))  # [N, K, P]
    return (torch.exp(raw[..., 0:3])[..., None] * e[:, :, None, :]).sum(1)


def sg_render_f32(raw, R, C, H, W):
    out = _sg_rec_f32(raw, R, C, H, W).view(len(raw), 3, H, W)
    assert out.dtype == torch.float32
    return out.numpy()


def sg_loss_grad_f32(raw, env, sw, R, C):
    """(total, per-map loss [N], gradient [N, K, 6]) in torch float32, the gradient by autograd"""
    N = len(raw)
    p = raw.clone().requires_grad_()
    rec = _sg_rec_f32(p, R, C, *env.shape[2:])
    per = ((torch.log(rec + 1) - torch.log(env + 1).view(N, 3, -1)) ** 2 * sw.reshape(N, 3, -1)).view(N, -1).mean(1)
    total = per.sum()
    total.backward()
    assert total.dtype == torch.float32 and p.grad.dtype == torch.float32
    return total.item(), per.detach().numpy(), p.grad.numpy()


@pytest.mark.parametrize("case", E.SG_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_sg_cases_leave_room_for_the_kernel(case):
    N, H, W, R, C = case
    raw, env = E.sg_inputs(case)
    r = sg_render_f32(raw, R, C, H, W)
    assert rel(r, E.sg_render_reference(case)) <= SG_RENDER_TOL / 4
    for kind in E.SG_WEIGHT_KINDS:
        total, per, grad = sg_loss_grad_f32(raw, env, E.sg_weight(case, kind), R, C)
        ref_total, ref_per, ref_grad = E.sg_reference(case, kind)
        assert abs(float(total) - ref_total) <= SG_LOSS_TOL / 4 * abs(ref_total), kind
        assert (np.abs(per - ref_per) <= SG_LOSS_TOL / 4 * np.abs(ref_per)).all(), kind
        assert rel_l2(grad, ref_grad) <= SG_GRAD_TOL / 4, kind
        assert E.per_map_rel_l2(grad, ref_grad).max() <= SG_GRAD_TOL / 4, (kind, E.per_map_rel_l2(grad, ref_grad).max())


# ---------------------------------------------------------------------------------------------- diffuse convolution
@pytest.mark.parametrize("P,Q", E.DF_SHAPES)
def test_diffuse_cases_leave_room_for_the_kernel(P, Q):
    src, in_dirs, w, out_dirs, ref = E.df_inputs(P, Q)
    src, in_dirs, w, out_dirs = (t.numpy() for t in (src, in_dirs, w, out_dirs))
    t = out_dirs[:, None, 0] * in_dirs[None, :, 0]
    t = t + out_dirs[:, None, 1] * in_dirs[None, :, 1]
    t = t + out_dirs[:, None, 2] * in_dirs[None, :, 2]
    A = np.maximum(t, f32(0)) * (w * f32(1 / np.pi))
    # [N, P, 3, Q] summed over its contiguous last axis: numpy adds pairwise there.  One sequential chain over all of
    # Q = 4097 (np.einsum) reaches 2.6e-6 on the worst map, which is summation order, not conditioning.
    out = (A[None, :, None, :] * np.ascontiguousarray(src.transpose(0, 2, 1))[:, None, :, :]).sum(-1, dtype=f32)
    assert out.dtype == f32
    assert ref.reshape(E.DF_NMAX, -1).max(axis=1).min() > 0
    for N in E.DF_N:
        assert (P, Q, N) in E.DF_CASES
        assert E.per_map_rel(out[:N], ref[:N]).max() <= DIFFUSE_TOL / 4, (P, Q, N, E.per_map_rel(out[:N], ref[:N]).max())
