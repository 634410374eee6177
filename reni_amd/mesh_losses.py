"""The mesh regularisers of SoftRas / pytorch3d.loss on the device: ``mesh_edge_loss``, ``mesh_laplacian_smoothing``,
``mesh_normal_consistency`` and the fused ``mesh_regularizer`` -- what keeps a mesh fitted through ``MeshRasterizer.gbuffer`` and
``MeshRasterizer.silhouette`` a surface (the photometric and the silhouette loss constrain only what the views see).

All four are autograd functions over ``ops.mesh_regularizers`` (reni_tu_meshreg.hip; include/reni_hip.h has the definitions
and where they deviate from pytorch3d).  They return 0-d tensors; the gradient accumulates into ``verts.grad`` beside the
renderer's and the silhouette's, and it is bit-reproducible: no float atomics, every sum in an order that depends on the
topology alone.  The kernel produces the gradient with the value (the objective is a scalar), so the backward is one multiply.
The topology lists are kept by the ``Meshes`` per in-place version of its faces; the values are computed anew at every call, so
an in-place optimiser step on the vertices is seen.  There is no CPU path: CPU tensors raise."""
import torch

from . import _lib, ops


class _MeshRegFn(torch.autograd.Function):
    """values[index] of ``ops.mesh_regularizers`` as a function of the vertices; the gradient is the one the call produced"""

    @staticmethod
    def forward(ctx, verts, faces, lists, weights, target_length, method, index, need):
        values, grad = ops.mesh_regularizers(verts.detach(), faces, *weights, target_length=target_length, method=method,
                                             lists=lists, need_grad=need)
        ctx.grad = grad
        return values[index].clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.grad is None:
            return (None,) * 8
        return (ctx.grad * g.to(ctx.grad.dtype),) + (None,) * 7


def _apply(mesh, weights, target_length, method, index):
    if method not in _lib.LAPLACIAN:
        raise ValueError(f"method must be one of {tuple(_lib.LAPLACIAN)}, got {method!r} (\"cotcurv\" is not implemented)")
    weights = tuple(float(w) for w in weights)
    target_length = float(target_length)
    for name, x in zip(("edge", "laplacian", "normal", "target_length"), weights + (target_length,)):
        if not (x >= 0.0) or x == float("inf"):
            raise ValueError(f"{name} must be >= 0 and finite, got {x}")
    verts, faces = mesh.verts_packed(), mesh.faces_packed()
    ops._require_cuda(verts, faces)
    need = verts.requires_grad and torch.is_grad_enabled()  # (under no_grad nobody can ask for the gradient: no gather)
    return _MeshRegFn.apply(verts, faces, mesh._edge_lists(), weights, target_length, method, index, need)


def mesh_edge_loss(mesh, target_length: float = 0.0) -> torch.Tensor:
    """(1 / E) sum over the unique edges of (|x_a - x_b| - target_length)^2; 0 for a mesh without edges"""
    return _apply(mesh, (1.0, 0.0, 0.0), target_length, "uniform", 1)


def mesh_laplacian_smoothing(mesh, method: str = "uniform") -> torch.Tensor:
    """(1 / V) sum_v |r_v|, r_v the uniform ("uniform") or cotangent-weighted ("cot") mean of v's neighbours minus x_v; the cot
    weights are constants of the gradient.  A vertex without neighbours has r_v = 0."""
    return _apply(mesh, (0.0, 1.0, 0.0), 0.0, method, 2)


def mesh_normal_consistency(mesh) -> torch.Tensor:
    """(1 / P) sum over the pairs of faces on one edge of 1 - cos of their normals; 0 for a mesh without such a pair"""
    return _apply(mesh, (0.0, 0.0, 1.0), 0.0, "uniform", 3)


def mesh_regularizer(mesh, edge: float = 0.0, laplacian: float = 0.0, normal: float = 0.0, target_length: float = 0.0,
                     method: str = "uniform") -> torch.Tensor:
    """edge * mesh_edge_loss + laplacian * mesh_laplacian_smoothing + normal * mesh_normal_consistency from ONE call of the
    kernels (a weight of 0 skips that term's work)"""
    return _apply(mesh, (edge, laplacian, normal), target_length, method, 0)
