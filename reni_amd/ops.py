"""Thin tensor-level wrappers over the C ABI: plans, workspace and the compute calls.

PyTorch is plumbing here (device memory, streams); all arithmetic happens in libreni_hip.so.
"""
from __future__ import annotations

import ctypes
import math
import types
from typing import Optional, Tuple

import torch

from . import _lib


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.RENILibraryError(
                "RENI HIP ops need tensors on a GPU device (got a CPU tensor); there is no CPU fallback")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _loss_views(target, weight, B, P):
    """target / weight as float32 [B,P,3] views (stride 0 broadcasts: nothing is materialised) and their stride arrays."""
    target = (target if target.dtype == torch.float32 else target.float()).expand(B, P, 3)
    weight = (weight if weight.dtype == torch.float32 else weight.float()).expand(B, P, 3)
    return target, weight, (ctypes.c_int64 * 3)(*target.stride()), (ctypes.c_int64 * 3)(*weight.stride())


def _sparse_flags(sparse_weight):
    if sparse_weight not in (False, True, None, "tiles", "pixels"):
        raise ValueError('sparse_weight must be False, True / "tiles", or "pixels"')
    return _lib.WEIGHT_COMPACT if sparse_weight == "pixels" else _lib.WEIGHT_SPARSE if sparse_weight else 0


def _call(fn, device, *args):
    """fn(*args, stream) with `device` current and its current stream as the last argument; raises on a library error."""
    with torch.cuda.device(device):
        _lib.check(fn(*args, torch.cuda.current_stream(device).cuda_stream))


def _ptr(t):
    """t's address, or None (the C ABI's NULL) for an optional tensor that is not given"""
    return None if t is None else t.data_ptr()


def _strides(t):
    """t's element strides as the C ABI's int64 array (None, like ``_ptr``, for an optional tensor that is not given)"""
    return None if t is None else (ctypes.c_int64 * t.dim())(*t.stride())


def _f32(t):
    """t as float32: t itself, strides and all, where it already is"""
    return t if t.dtype == torch.float32 else t.float()


def _ws256(nbytes, device):
    """-> (the uint8 tensor that owns a call's workspace, a 256-byte aligned pointer into it, the bytes behind that pointer: at
    least nbytes).  Every wrapper below takes its workspace here: the library wants the alignment, no allocator promises it."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    p = ws.data_ptr()
    ap = (p + 255) & ~255
    return ws, ap, ws.numel() - (ap - p)


class Plan:
    """Immutable kernel plan for one decoder architecture (reni_plan_create)."""

    def __init__(self, equivariance: str, ndims: int, hidden_features: int, hidden_layers: int,
                 out_features: int = 3, last_layer_linear: bool = True, output_activation=None,
                 first_omega_0: float = 30.0, hidden_omega_0: float = 30.0, dtype: str = "f32",
                 conditioning: str = "concat", mapping_layers: int = 0, mapping_features: int = 0):
        lib = _lib.load()
        if equivariance not in _lib.EQ:
            raise ValueError(f"equivariance {equivariance!r}")
        if output_activation not in _lib.ACT:
            raise ValueError(f"output_activation {output_activation!r}")
        self.desc = _lib.reni_desc(_lib.EQ[equivariance], ndims, hidden_features, hidden_layers, out_features,
                                   1 if last_layer_linear else 0, _lib.ACT[output_activation],
                                   float(first_omega_0), float(hidden_omega_0), _lib.DTYPE[dtype],
                                   {"concat": _lib.COND_CONCAT, "film": _lib.COND_FILM}[conditioning],
                                   int(mapping_layers), int(mapping_features))
        self.conditioning = conditioning
        self.hidden_features = hidden_features
        self.hidden_layers = hidden_layers
        self._h = ctypes.c_void_p()
        _lib.check(lib.reni_plan_create(ctypes.byref(self.desc), ctypes.byref(self._h)))
        self.lib = lib
        self.ndims = ndims
        self.dtype = dtype
        self.n_params = int(lib.reni_param_count(self._h))
        self.n_map_params = int(lib.reni_film_map_param_count(self._h))
        self.in_features = int(lib.reni_in_features(self._h))
        self.n_first = hidden_features * self.in_features + hidden_features   # W0 + b0: the head of the flat buffer
        self._ws = {}

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self.lib.reni_plan_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    # ---- workspace (a torch uint8 tensor, cached per device and size)
    def workspace(self, B: int, P: int, flags: int, device) -> torch.Tensor:
        n = int(self.lib.reni_workspace_bytes(self._h, B, P, flags))
        if n == 0:
            raise _lib.RENILibraryError("reni_workspace_bytes returned 0 (unsupported configuration)")
        key = (torch.device(device).index, )
        ws = self._ws.get(key)
        if ws is None or ws.numel() < n:
            ws = torch.empty(n + 256, dtype=torch.uint8, device=device)
            self._ws[key] = ws
        # Every hand-out counts: reni_train_step_rows keeps the NEXT batch's prologue (gathered rows, A_b, layer-0 operands, packed
        # weight images) in this buffer between two calls, and any other call on the plan -- a validation forward at another B, a
        # fused loss, a reallocation for a larger problem -- overwrites it at shifted offsets or abandons the buffer.  train_step
        # compares this counter with the one it saw at the end of the step that staged.
        self._ws_gen = getattr(self, "_ws_gen", 0) + 1
        return ws

    @staticmethod
    def _aligned_ptr(ws: torch.Tensor) -> Tuple[int, int]:
        p = ws.data_ptr()
        ap = (p + 255) & ~255
        return ap, ws.numel() - (ap - p)

    def _ws_args(self, B, P, flags, device):
        """(aligned workspace pointer, bytes behind it, current stream) of one call -- through workspace(): every hand-out counts."""
        wp, wn = self._aligned_ptr(self.workspace(B, P, flags, device))
        return wp, wn, torch.cuda.current_stream(device).cuda_stream

    def launch_info(self, B: int, P: int):
        info = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.reni_launch_info(self._h, B, P, info))
        return {"workgroups": info[0], "threads": info[1], "lds_bytes": info[2], "tiles": info[3]}

    def path_info(self, B: int, P: int, need_dw: bool = True, need_dz: bool = True):
        """Which kernels a backward call of this shape takes (reni_path_info): printed by bench.py so that an environment selector
        left set by accident shows on the line."""
        info = (ctypes.c_int32 * 8)()
        flags = (_lib.NEED_DW if need_dw else 0) | (_lib.NEED_DZ if need_dz else 0)
        _lib.check(self.lib.reni_path_info(self._h, B, P, flags, info))
        env = [n for b, n in ((1, "RENI_NO_PERSIST"), (2, "RENI_NO_SIDE_STREAM"), (4, "RENI_FRAG_WS_CAP_MB"), (8, "RENI_DW1_OLD"),
                              (16, "RENI_NO_L0X"), (32, "RENI_TRAIN_WG")) if info[6] & b]
        # (k_reni_l0_ring: layer 0's backward + dW_1 behind the L0X training instance -- given, in addition, WeightedMSE and no output image)
        return {"persistent_kernels": bool(info[0]), "dw1_kernel": ("none", "k_reni_dw1_ring", "k_reni_dw1", "k_reni_l0_ring")[info[1]],
                "side_stream": bool(info[2]), "images_per_chunk": info[3], "operand_stream": bool(info[4]),
                "fragment_stream": ("none", "bf16", "f32")[info[5]], "env_overrides": env, "workgroups": info[7]}

    # ---- compute
    def _grid_args(self, Z, D):
        B = Z.shape[0]
        if D.dim() == 2:
            D = D.unsqueeze(0)
        if D.shape[0] not in (1, B):
            raise ValueError(f"directions batch {D.shape[0]} does not match latent batch {B}")
        P = D.shape[1]
        dbs = 0 if D.shape[0] == 1 or D.stride(0) == 0 else P * 3
        if dbs == 0:
            D = D[:1]
        return B, P, _f32c(D), dbs

    def _check_zp(self, Z, params, map_params=None):
        """The C ABI takes bare pointers: a mis-shaped latent or parameter buffer would be read out of bounds."""
        if Z.dim() != 3 or tuple(Z.shape[1:]) != (self.ndims, 3):
            raise ValueError(f"Z must be [B,{self.ndims},3], got {tuple(Z.shape)}")
        if params.numel() != self.n_params:
            raise ValueError(f"params must hold {self.n_params} floats, got {params.numel()}")
        if map_params is not None and map_params.numel() != self.n_map_params:
            raise ValueError(f"map_params must hold {self.n_map_params} floats, got {map_params.numel()}")

    def forward(self, Z: torch.Tensor, D: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
        _require_cuda(Z, D, params)
        Z = _f32c(Z); params = _f32c(params)
        self._check_zp(Z, params)
        B, P, Dc, dbs = self._grid_args(Z, D)
        out = torch.empty(B, P, 3, dtype=torch.float32, device=Z.device)
        wp, wn, stream = self._ws_args(B, P, 0, Z.device)
        _lib.check(self.lib.reni_forward(self._h, B, P, Z.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(),
                                         out.data_ptr(), wp, wn, stream))
        return out

    def forward_loss_backward(self, Z, D, params, target, weight, loss_kind="mse", alpha=0.0, beta=0.0,
                              need_dw=True, need_dz=True, want_out=False, idx=None, sparse_weight=False):
        """target / weight: any strided [B,P,3] views (stride 0 broadcasts); returns
        (loss_terms[4] device tensor, dZ or None, dparams or None, out or None).
        idx (int64 device tensor [B]): Z is a latent TABLE and image b uses row idx[b] (gathered inside the prologue
        kernel: reni_forward_loss_backward_rows); dZ stays [B,ND,3] in batch order.  An index outside the table makes the
        call's loss and gradients NaN (no out-of-bounds read, no host synchronisation to check it).
        sparse_weight: the weight is zero over whole regions (an inpainting mask, RENI_module.py:92-94): RENI_WEIGHT_SPARSE --
        the frozen-decoder persistent kernels then leave out the tiles (and the statistics pass) that cannot change the result --
        bit-equal to the dense call.  sparse_weight="pixels": RENI_WEIGHT_COMPACT -- the pixels with weight are also packed into
        each image's first tiles (fewer tiles still; the sums are re-associated: equal to fp32 rounding)."""
        _require_cuda(Z, D, params, target, weight, idx)
        Z = _f32c(Z); params = _f32c(params)
        self._check_zp(Z, params)
        if idx is not None:
            if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1:
                raise ValueError("idx must be a non-empty 1-D int64 tensor")
            idx = idx.contiguous()
            B, P, Dc, dbs = self._grid_args(Z[:1].expand(idx.numel(), -1, -1), D)  # (the batch's shape; Z stays the table)
        else:
            B, P, Dc, dbs = self._grid_args(Z, D)
        target, weight, ts, wst = _loss_views(target, weight, B, P)
        flags = (_lib.NEED_DW if need_dw else 0) | (_lib.NEED_DZ if need_dz else 0) | _sparse_flags(sparse_weight)
        dev = Z.device
        loss_terms = torch.empty(4, dtype=torch.float32, device=dev)
        dZ = torch.empty(B, self.ndims, 3, dtype=torch.float32, device=dev) if need_dz else None
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev) if need_dw else None
        out = torch.empty(B, P, 3, dtype=torch.float32, device=dev) if want_out else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        kind = _lib.LOSS_KIND[loss_kind]
        tail = (Dc.data_ptr(), dbs, params.data_ptr(), target.data_ptr(), ts, weight.data_ptr(), wst, kind, float(alpha),
                float(beta), flags, out.data_ptr() if out is not None else None, loss_terms.data_ptr(),
                dZ.data_ptr() if dZ is not None else None, dparams.data_ptr() if dparams is not None else None, wp, wn, stream)
        if idx is not None:
            _lib.check(self.lib.reni_forward_loss_backward_rows(self._h, B, P, Z.data_ptr(), Z.shape[0], idx.data_ptr(), *tail))
        else:
            _lib.check(self.lib.reni_forward_loss_backward(self._h, B, P, Z.data_ptr(), *tail))
        return loss_terms, dZ, dparams, out

    def train_step(self, Z_table, idx, D, params, target, weight, m_dec, v_dec, m_lat, v_lat, step, lr, stage_state, idx_next=None,
                   loss_kind="mse", alpha=0.0, beta=0.0, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, comm=None, overlap=False):
        """reni_train_step_rows: fused fwd + loss + bwd on the rows `idx` of the latent TABLE, then torch.optim.Adam's update of
        `params` and of the whole table, IN PLACE -- the same results as forward_loss_backward(idx=...) + adam_step2, with Adam and
        the next batch's prologue (`idx_next`) scheduled beside the backward pass's last kernel.  stage_state: a ctypes.c_uint32
        the caller keeps between calls (zero it whenever params / the table / the shapes change behind the library's back).
        comm: a ``dist.RcclComm`` -- the data-parallel step (reni_train_step_rows_dp): the decoder gradient is summed over the
        communicator's ranks INSIDE the call (pass grad_scale = 1 / world); overlap: the early slice on the library's own stream.
        Returns (loss_terms[4], dZ [B,ND,3], dparams)."""
        _require_cuda(Z_table, D, params, target, weight, idx, idx_next, m_dec, v_dec, m_lat, v_lat)
        for t in (Z_table, params, m_dec, v_dec, m_lat, v_lat):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("train_step updates its buffers in place: contiguous float32 tensors only")
        self._check_zp(Z_table, params)
        for ix in (idx, idx_next):
            if ix is not None and (ix.dtype != torch.int64 or ix.dim() != 1 or ix.numel() != idx.numel() or not ix.is_contiguous()):
                raise ValueError("idx / idx_next must be contiguous 1-D int64 tensors of the same length")
        B, P, Dc, dbs = self._grid_args(Z_table[:1].expand(idx.numel(), -1, -1), D)
        target, weight, ts, wst = _loss_views(target, weight, B, P)
        dev = Z_table.device
        loss_terms = torch.empty(4, dtype=torch.float32, device=dev)
        dZ = torch.empty(B, self.ndims, 3, dtype=torch.float32, device=dev)
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev)
        # a staged prologue is only good if NOTHING took the plan's workspace since the call that staged it (see workspace())
        if stage_state.value & 1 and getattr(self, "_stage_gen", None) != (getattr(self, "_ws_gen", 0), dev.index):
            stage_state.value = 0
        wp, wn, stream = self._ws_args(B, P, _lib.NEED_DW | _lib.NEED_DZ, dev)
        self._stage_gen = (self._ws_gen, dev.index)
        kind = _lib.LOSS_KIND[loss_kind]
        head = (self._h, B, P, Z_table.data_ptr(), Z_table.shape[0], idx.data_ptr(), idx_next.data_ptr() if idx_next is not None else None,
                Dc.data_ptr(), dbs, params.data_ptr(), target.data_ptr(), ts, weight.data_ptr(), wst, kind, float(alpha), float(beta),
                m_dec.data_ptr(), v_dec.data_ptr(), m_lat.data_ptr(), v_lat.data_ptr(), float(lr), float(betas[0]), float(betas[1]),
                float(eps), int(step), float(grad_scale))
        tail = (ctypes.byref(stage_state), loss_terms.data_ptr(), dZ.data_ptr(), dparams.data_ptr(), wp, wn, stream)
        with torch.cuda.device(dev):
            if comm is not None:
                _lib.check(self.lib.reni_train_step_rows_dp(*head, comm._comm, 1 if overlap else 0, *tail))
            else:
                _lib.check(self.lib.reni_train_step_rows(*head, *tail))
        return loss_terms, dZ, dparams

    def weight_lists(self, B, P, weight, mode):
        """The tile / pixel lists of a masked weight (reni_weight_lists_build), built ONCE per (weight tensor, its version counter,
        shape, strides, mode) and kept on the plan: the inpainting mask of a FIT_LATENT run does not change over its epochs.
        weight: the [B, P, 3] (expanded) view the step passes; mode: _lib.WEIGHT_SPARSE or _lib.WEIGHT_COMPACT."""
        # CAVEAT: the key sees in-place writes only through torch's version counter -- a write through `weight.data`, a
        # custom kernel or ctypes does not bump it.  Whoever changes the mask that way calls invalidate_weight_lists() (or passes
        # cache_lists=False to latent_step).  Inference tensors have no version counter: they are never cached (-> None).
        try:
            version = weight._version
        except RuntimeError:
            return None
        key = (weight.data_ptr(), version, tuple(weight.shape), tuple(weight.stride()), int(B), int(P), int(mode), weight.device.index)
        cache = self.__dict__.setdefault("_wlists", {})
        hit = cache.get("key") == key
        if not hit:
            n = int(self.lib.reni_weight_lists_bytes(B, P))
            buf = cache.get("buf")
            if buf is None or buf.numel() < n + 256 or buf.device != weight.device:
                buf = torch.empty(n + 256, dtype=torch.uint8, device=weight.device)
            lp = (buf.data_ptr() + 255) & ~255
            wst = (ctypes.c_int64 * 3)(*weight.stride())
            summary = (ctypes.c_int32 * 3)()
            _call(self.lib.reni_weight_lists_build, weight.device, B, P, weight.data_ptr(), wst, int(mode), lp,
                  buf.numel() - (lp - buf.data_ptr()), summary)
            # (one synchronisation per mask: no image with a live cosine term -> the steps leave the statistics launches out)
            cache.update(key=key, buf=buf, ptr=lp, weight=weight, cos_constant=summary[2] == 0,   # (the weight is kept alive: its
                         summary=tuple(summary))                                                  #  data_ptr is part of the key)
        return cache["ptr"], (_lib.WEIGHT_COS_CONSTANT if cache["cos_constant"] else 0)

    def invalidate_weight_lists(self):
        """Forget the cached tile / pixel lists: the next latent_step(sparse_weight=...) rebuilds them from the weight it is given.  To be
        called after a write into the weight tensor that torch's version counter cannot see (``weight.data``, a custom kernel, ctypes)."""
        self.__dict__.pop("_wlists", None)

    def latent_step(self, Z_table, idx, D, params, target, weight, m_lat, v_lat, step, lr, loss_kind="test", alpha=0.0, beta=0.0,
                    betas=(0.9, 0.999), eps=1e-8, sparse_weight=False, cache_lists=True):
        """reni_latent_step_rows: one FIT_LATENT iteration (frozen decoder) -- forward_loss_backward(idx=..., need_dw=False) then
        adam_rows_step on the table, IN PLACE, as one library call.  Returns (loss_terms[4], dZ [B,ND,3])."""
        _require_cuda(Z_table, D, params, target, weight, idx, m_lat, v_lat)
        for t in (Z_table, m_lat, v_lat):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("latent_step updates its buffers in place: contiguous float32 tensors only")
        params = _f32c(params)
        self._check_zp(Z_table, params)
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1 or not idx.is_contiguous():
            raise ValueError("idx must be a non-empty contiguous 1-D int64 tensor")
        flags = _sparse_flags(sparse_weight)
        B, P, Dc, dbs = self._grid_args(Z_table[:1].expand(idx.numel(), -1, -1), D)
        target, weight, ts, wst = _loss_views(target, weight, B, P)
        dev = Z_table.device
        loss_terms = torch.empty(4, dtype=torch.float32, device=dev)
        dZ = torch.empty(B, self.ndims, 3, dtype=torch.float32, device=dev)
        wp, wn, stream = self._ws_args(B, P, _lib.NEED_DZ | flags, dev)
        kind = _lib.LOSS_KIND[loss_kind]
        head = (self._h, B, P, Z_table.data_ptr(), Z_table.shape[0], idx.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(),
                target.data_ptr(), ts, weight.data_ptr(), wst, kind, float(alpha), float(beta), flags)
        tail = (m_lat.data_ptr(), v_lat.data_ptr(), float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                loss_terms.data_ptr(), dZ.data_ptr(), wp, wn, stream)
        chunked = False
        if flags:  # (H = 256 problems that run in image chunks keep the rebuilding entry point; decided once per shape)
            cc = self.__dict__.setdefault("_chunk_cache", {})
            if (B, P) not in cc:
                cc[(B, P)] = self.path_info(B, P, need_dw=False)["images_per_chunk"] < B
            chunked = cc[(B, P)]
        if flags and cache_lists and not chunked:
            # the lists from the plan's cache (built once per mask: reni_weight_lists_build), the step without its list-building launches
            wl = self.weight_lists(B, P, weight, flags)
        else:
            wl = None
        if wl is not None:
            lptr, extra = wl
            _lib.check(self.lib.reni_latent_step_rows_cached(*head[:-1], flags | extra, lptr, *tail))
        else:
            _lib.check(self.lib.reni_latent_step_rows(*head, *tail))
        return loss_terms, dZ

    def backward(self, Z, D, params, dout, need_dw=True, need_dz=True):
        _require_cuda(Z, D, params, dout)
        Z = _f32c(Z); params = _f32c(params); dout = _f32c(dout)
        self._check_zp(Z, params)
        B, P, Dc, dbs = self._grid_args(Z, D)
        if tuple(dout.shape) != (B, P, 3):
            raise ValueError(f"dout must be [{B},{P},3], got {tuple(dout.shape)}")
        flags = (_lib.NEED_DW if need_dw else 0) | (_lib.NEED_DZ if need_dz else 0)
        dev = Z.device
        dZ = torch.empty_like(Z) if need_dz else None
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev) if need_dw else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        _lib.check(self.lib.reni_backward(
            self._h, B, P, Z.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(), dout.data_ptr(), flags,
            dZ.data_ptr() if dZ is not None else None, dparams.data_ptr() if dparams is not None else None,
            wp, wn, stream))
        return dZ, dparams


    # ---- FiLM conditioning: the per-sample core (per-image glue in reni_amd/film.py)
    def _film_args(self, A, film, D):
        B = A.shape[0]
        H, L = self.hidden_features, self.hidden_layers
        assert A.shape == (B, H, 8), f"A must be [B,{H},8], got {tuple(A.shape)}"
        assert film.shape == (B, L, 2, H), f"film must be [B,{L},2,{H}], got {tuple(film.shape)}"
        return self._grid_args(A, D)

    def film_forward(self, A, film, D, params):
        _require_cuda(A, film, D, params)
        A = _f32c(A); film = _f32c(film); params = _f32c(params)
        B, P, Dc, dbs = self._film_args(A, film, D)
        assert params.numel() == self.n_params
        out = torch.empty(B, P, 3, dtype=torch.float32, device=A.device)
        wp, wn, stream = self._ws_args(B, P, 0, A.device)
        _lib.check(self.lib.reni_film_forward(self._h, B, P, Dc.data_ptr(), dbs, A.data_ptr(), film.data_ptr(),
                                              params.data_ptr(), out.data_ptr(), wp, wn, stream))
        return out

    def film_forward_loss_backward(self, A, film, D, params, target, weight, loss_kind="mse", beta=0.0,
                                   need_dw=True, want_out=False):
        """-> (loss_terms[4], dA [B,H,8], dfilm [B,L,2,H], dparams or None, out or None)"""
        _require_cuda(A, film, D, params, target, weight)
        A = _f32c(A); film = _f32c(film); params = _f32c(params)
        B, P, Dc, dbs = self._film_args(A, film, D)
        target, weight, ts, wst = _loss_views(target, weight, B, P)
        flags = _lib.NEED_DW if need_dw else 0
        dev = A.device
        loss_terms = torch.empty(4, dtype=torch.float32, device=dev)
        dA = torch.empty_like(A)
        dfilm = torch.empty_like(film)
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev) if need_dw else None
        out = torch.empty(B, P, 3, dtype=torch.float32, device=dev) if want_out else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        kind = _lib.LOSS_KIND[loss_kind]
        _lib.check(self.lib.reni_film_forward_loss_backward(
            self._h, B, P, Dc.data_ptr(), dbs, A.data_ptr(), film.data_ptr(), params.data_ptr(), target.data_ptr(), ts,
            weight.data_ptr(), wst, kind, float(beta), flags, out.data_ptr() if out is not None else None,
            loss_terms.data_ptr(), dA.data_ptr(), dfilm.data_ptr(),
            dparams.data_ptr() if dparams is not None else None, wp, wn, stream))
        return loss_terms, dA, dfilm, dparams, out

    def film_backward(self, A, film, D, params, dout, need_dw=True):
        _require_cuda(A, film, D, params, dout)
        A = _f32c(A); film = _f32c(film); params = _f32c(params); dout = _f32c(dout)
        B, P, Dc, dbs = self._film_args(A, film, D)
        flags = _lib.NEED_DW if need_dw else 0
        dev = A.device
        dA = torch.empty_like(A)
        dfilm = torch.empty_like(film)
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev) if need_dw else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        _lib.check(self.lib.reni_film_backward(
            self._h, B, P, Dc.data_ptr(), dbs, A.data_ptr(), film.data_ptr(), params.data_ptr(), dout.data_ptr(), flags,
            dA.data_ptr(), dfilm.data_ptr(), dparams.data_ptr() if dparams is not None else None, wp, wn, stream))
        return dA, dfilm, dparams


    # ---- FiLM, whole model (per-image glue in HIP too): latents + mapping-network parameters in, their gradients out
    def film_model_forward(self, Z, D, params, map_params):
        _require_cuda(Z, D, params, map_params)
        Z = _f32c(Z); params = _f32c(params); map_params = _f32c(map_params)
        self._check_zp(Z, params, map_params)
        B, P, Dc, dbs = self._grid_args(Z, D)
        out = torch.empty(B, P, 3, dtype=torch.float32, device=Z.device)
        wp, wn, stream = self._ws_args(B, P, 0, Z.device)
        _lib.check(self.lib.reni_film_model_forward(self._h, B, P, Z.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(),
                                                    map_params.data_ptr(), out.data_ptr(), wp, wn, stream))
        return out

    def film_model_forward_loss_backward(self, Z, D, params, map_params, target, weight, loss_kind="mse", alpha=0.0,
                                         beta=0.0, need_dw=True, want_out=False):
        """-> (loss_terms[4], dZ, dparams or None, dmap_params or None, out or None).  The two gradients are the two halves
        of ONE buffer (dparams first), so an optimiser over [params | map_params] stored the same way takes it whole
        (``dparams._base``)."""
        _require_cuda(Z, D, params, map_params, target, weight)
        Z = _f32c(Z); params = _f32c(params); map_params = _f32c(map_params)
        self._check_zp(Z, params, map_params)
        B, P, Dc, dbs = self._grid_args(Z, D)
        target, weight, ts, wst = _loss_views(target, weight, B, P)
        flags = (_lib.NEED_DW if need_dw else 0) | _lib.NEED_DZ
        dev = Z.device
        loss_terms = torch.empty(4, dtype=torch.float32, device=dev)
        dZ = torch.empty_like(Z)
        gall = torch.empty(self.n_params + self.n_map_params, dtype=torch.float32, device=dev) if need_dw else None
        dparams = gall[:self.n_params] if need_dw else None
        dmap = gall[self.n_params:] if need_dw else None
        out = torch.empty(B, P, 3, dtype=torch.float32, device=dev) if want_out else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        kind = _lib.LOSS_KIND[loss_kind]
        _lib.check(self.lib.reni_film_model_forward_loss_backward(
            self._h, B, P, Z.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(), map_params.data_ptr(), target.data_ptr(), ts,
            weight.data_ptr(), wst, kind, float(alpha), float(beta), flags, out.data_ptr() if out is not None else None,
            loss_terms.data_ptr(), dZ.data_ptr(), dparams.data_ptr() if need_dw else None,
            dmap.data_ptr() if need_dw else None, wp, wn, stream))
        return loss_terms, dZ, dparams, dmap, out

    def film_model_backward(self, Z, D, params, map_params, dout, need_dw=True):
        _require_cuda(Z, D, params, map_params, dout)
        Z = _f32c(Z); params = _f32c(params); map_params = _f32c(map_params); dout = _f32c(dout)
        self._check_zp(Z, params, map_params)
        B, P, Dc, dbs = self._grid_args(Z, D)
        if tuple(dout.shape) != (B, P, 3):
            raise ValueError(f"dout must be [{B},{P},3], got {tuple(dout.shape)}")
        flags = (_lib.NEED_DW if need_dw else 0) | _lib.NEED_DZ
        dev = Z.device
        dZ = torch.empty_like(Z)
        dparams = torch.empty(self.n_params, dtype=torch.float32, device=dev) if need_dw else None
        dmap = torch.empty(self.n_map_params, dtype=torch.float32, device=dev) if need_dw else None
        wp, wn, stream = self._ws_args(B, P, flags, dev)
        _lib.check(self.lib.reni_film_model_backward(
            self._h, B, P, Z.data_ptr(), Dc.data_ptr(), dbs, params.data_ptr(), map_params.data_ptr(), dout.data_ptr(), flags,
            dZ.data_ptr(), dparams.data_ptr() if need_dw else None, dmap.data_ptr() if need_dw else None, wp, wn, stream))
        return dZ, dparams, dmap


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float,
              betas=(0.9, 0.999), eps: float = 1e-8, grad_scale: float = 1.0):
    """In-place torch.optim.Adam step on flat fp32 buffers (reni_adam_step)."""
    _require_cuda(p, g, m, v)
    lib = _lib.load()
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    stream = torch.cuda.current_stream(p.device).cuda_stream
    _lib.check(lib.reni_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr),
                                  float(betas[0]), float(betas[1]), float(eps), int(step), float(grad_scale), stream))


def adam_rows_step(table: torch.Tensor, g_rows: torch.Tensor, idx: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
                   lr: float, betas=(0.9, 0.999), eps: float = 1e-8, grad_scale: float = 1.0):
    """In-place dense Adam step on table [N, ...] with the gradient g_rows [B, ...] of rows idx (reni_adam_rows_step)."""
    _require_cuda(table, g_rows, idx, m, v)
    lib = _lib.load()
    assert table.is_contiguous() and g_rows.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    idx = idx.to(torch.int64).contiguous()
    n_rows = table.shape[0]
    row_len = table.numel() // max(n_rows, 1)
    assert g_rows.numel() == idx.numel() * row_len
    stream = torch.cuda.current_stream(table.device).cuda_stream
    _lib.check(lib.reni_adam_rows_step(table.data_ptr(), g_rows.data_ptr(), idx.data_ptr(), idx.numel(), row_len, m.data_ptr(),
                                       v.data_ptr(), n_rows, float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                       float(grad_scale), stream))


def adam_step2(p, g, m, v, table, g_rows, idx, tm, tv, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
               grad_scale: float = 1.0):
    """adam_step on the flat decoder buffer and adam_rows_step on the latent table in ONE launch (reni_adam_step2)."""
    _require_cuda(p, g, m, v, table, g_rows, idx, tm, tv)
    lib = _lib.load()
    for t in (p, g, m, v, table, g_rows, tm, tv):
        assert t.is_contiguous()
    idx = idx.to(torch.int64).contiguous()
    n_rows = table.shape[0]
    row_len = table.numel() // max(n_rows, 1)
    assert g_rows.numel() == idx.numel() * row_len
    _call(lib.reni_adam_step2, p.device, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), table.data_ptr(),
          g_rows.data_ptr(), idx.data_ptr(), idx.numel(), row_len, tm.data_ptr(), tv.data_ptr(), n_rows, float(lr), float(betas[0]),
          float(betas[1]), float(eps), int(step), float(grad_scale))


def selftest_layouts():
    lib = _lib.load()
    out = (ctypes.c_int32 * 2)()
    _lib.check(lib.reni_selftest_layouts(out, 2))
    return list(out)


def profile_enable(on: bool = True):
    """Record HIP events around every fused forward+backward kernel launch (reni_profile_enable)."""
    _lib.check(_lib.load().reni_profile_enable(1 if on else 0))


PROF_FWD_BWD, PROF_STATS, PROF_FWD, PROF_DW1, PROF_DWS, PROF_COMM, PROF_ALL = 0, 1, 2, 3, 4, 5, -1


def profile_minmax(kind: int = PROF_FWD_BWD):
    """-> (shortest, longest) launch in milliseconds of one kind since the last reset (reni_profile_minmax; call before the reset)."""
    lo, hi = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _lib.check(_lib.load().reni_profile_minmax(int(kind), ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def profile_read(reset: bool = True, kind: int = PROF_FWD_BWD):
    """-> (summed kernel milliseconds, number of launches) of one kind of launch since the last reset
    (kind: the fused forward+loss+backward pass, RENITestLoss's statistics pass, plain inference, or all)."""
    tot = ctypes.c_double(0.0)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().reni_profile_read_kind(int(kind), ctypes.byref(tot), ctypes.byref(n), 1 if reset else 0))
    return tot.value, n.value


def _dirs_dims(light_dirs, what="light_dirs"):
    if not isinstance(light_dirs, torch.Tensor) or light_dirs.dim() not in (2, 3) or light_dirs.shape[-1] != 3 or min(light_dirs.shape) < 1:
        raise ValueError(f"{what} must be [J, 3] (a shared grid) or [B, J, 3], got "
                         f"{tuple(light_dirs.shape) if isinstance(light_dirs, torch.Tensor) else type(light_dirs).__name__}")


def check_visibility(vis, NP: int, J: int, NB=None):
    """The checks every consumer of a visibility mask makes before the library is touched: int32 (the bit pattern of the
    header's uint32 words) [NB, NP, ceil(J/32)], a constant (no gradient).  NB None: any."""
    if isinstance(vis, torch.Tensor) and vis.requires_grad:
        raise ValueError("the visibility mask is a constant: it cannot require grad")
    if not isinstance(vis, torch.Tensor) or vis.dtype != torch.int32:
        raise ValueError(f"the visibility mask must be an int32 tensor (32 directions per word), got "
                         f"{vis.dtype if isinstance(vis, torch.Tensor) else type(vis).__name__}")
    JW = (int(J) + 31) // 32
    if vis.dim() != 3 or vis.shape[1] != NP or vis.shape[2] != JW or (NB is not None and vis.shape[0] != NB):
        raise ValueError(f"the visibility mask must be [{'NB' if NB is None else NB}, {NP}, {JW}] for {NP} pixels and {J} "
                         f"directions, got {tuple(vis.shape)}")


def _shade_inputs(normals, positions, camera_center, light_dirs, srcs, on_texels, vis, mat=None, mat_name=None, early=True):
    """The prologue the shader's calls share (include/reni_hip.h): the argument checks that come before the library is touched,
    the casts to contiguous fp32, B, NP, J and the direction stride, the sources' shapes, the camera and the mask.  normals,
    positions [NP,3]; light_dirs [J,3] (shared grid) or [B,J,3]; srcs[i] is [B,J,3] where on_texels[i], else [B,NP,3]; vis = None
    or the int32 mask [1,NP,JW] (shared grid; also accepted with per-image directions) / [B,NP,JW]; mat (named mat_name in the
    messages) = the per-pixel scalar: a float, a one-element tensor or [NP].  early False: the checks of light_dirs, the normals'
    rank and the mask are left to what follows.  -> a record: lib, dev, B, NP, J, srcs (the cast tensors), head (the calls'
    first ten arguments), vis (mask pointer, batch stride), mats (scalar pointer, stride, then vis); keep holds the cast tensors."""
    if early:
        _dirs_dims(light_dirs)
        if not isinstance(normals, torch.Tensor) or normals.dim() != 2:
            raise ValueError("normals and positions must be [NP, 3]")
        NP = normals.shape[0]
        if mat_name is not None:
            if isinstance(mat, torch.Tensor):
                if mat.numel() != 1 and tuple(mat.shape) != (NP,):
                    raise ValueError(f"{mat_name} must be a float, one value or [{NP}] (one per pixel), got {tuple(mat.shape)}")
            elif not isinstance(mat, (int, float)):
                raise ValueError(f"{mat_name} must be a float, one value or [{NP}] (one per pixel), got {type(mat).__name__}")
        if vis is not None:
            check_visibility(vis, NP, light_dirs.shape[-2])
            if vis.shape[0] != 1 and (light_dirs.dim() == 2 or vis.shape[0] != light_dirs.shape[0]):
                raise ValueError(f"a mask of {vis.shape[0]} images needs per-image directions [{vis.shape[0]}, J, 3]")
    _require_cuda(normals, positions, light_dirs, *srcs, vis, mat if isinstance(mat, torch.Tensor) else None)
    lib = _lib.load()
    f32 = torch.float32
    normals = normals.to(f32).contiguous(); positions = positions.to(f32).contiguous()
    light_dirs = light_dirs.to(f32).contiguous()
    srcs = [x.to(f32).contiguous() for x in srcs]
    dev = srcs[0].device
    NP = normals.shape[0]
    if normals.shape != (NP, 3) or positions.shape != (NP, 3):
        raise ValueError("normals and positions must be [NP, 3]")
    B = srcs[0].shape[0]
    if light_dirs.dim() == 2:
        J, stride = light_dirs.shape[0], 0
    else:
        if light_dirs.shape[0] != B:
            raise ValueError("light_dirs batch size must match the colours'")
        J, stride = light_dirs.shape[1], light_dirs.shape[1] * 3
    for x, texels in zip(srcs, on_texels):
        want = (B, J, 3) if texels else (B, NP, 3)
        if tuple(x.shape) != want:
            raise ValueError(f"expected a {want} tensor, got {tuple(x.shape)}")
    if isinstance(mat, torch.Tensor):
        mat = mat.detach().to(device=dev, dtype=f32).reshape(-1).contiguous()
    elif mat_name is not None:
        mat = torch.full((1,), float(mat), dtype=f32, device=dev)
    cam = [float(x) for x in torch.as_tensor(camera_center).reshape(-1)[:3].tolist()]
    vargs = (None, 0)
    if vis is not None:
        vis = vis.contiguous()
        vargs = (vis.data_ptr(), 0 if vis.shape[0] == 1 else NP * vis.shape[2])
    head = (B, NP, J, normals.data_ptr(), positions.data_ptr(), cam[0], cam[1], cam[2], light_dirs.data_ptr(), stride)
    mats = None if mat is None else (mat.data_ptr(), 0 if mat.numel() == 1 else 1, *vargs)
    return types.SimpleNamespace(lib=lib, dev=dev, B=B, NP=NP, J=J, srcs=srcs, head=head, vis=vargs, mats=mats,
                                 keep=(normals, positions, light_dirs, mat, vis))


def _shade_call(forward: bool, normals, positions, camera_center, light_dirs, src, shininess, kd, ks, vis=None):
    """reni_envmap_shade / reni_envmap_shade_backward and their _masked forms (include/reni_hip.h).  src = light colours [B,J,3]
    (forward) or d colours [B,NP,3] (backward).  Without a mask the checks of the mask's arguments are the library's."""
    p = _shade_inputs(normals, positions, camera_center, light_dirs, (src,), (forward,), vis, early=vis is not None)
    lib, f32 = p.lib, torch.float32
    out = torch.empty((p.B, p.NP, 3) if forward else (p.B, p.J, 3), dtype=f32, device=p.dev)
    ws, wp, wn = _ws256(int(lib.reni_envmap_shade_workspace_bytes(p.B, p.NP, p.J)), p.dev)
    head = (*p.head, p.srcs[0].data_ptr(), float(shininess), float(kd), float(ks))
    if vis is None:
        _call(lib.reni_envmap_shade if forward else lib.reni_envmap_shade_backward, p.dev, *head, out.data_ptr(), wp, wn)
    else:
        _call(lib.reni_envmap_shade_masked if forward else lib.reni_envmap_shade_masked_backward, p.dev, *head, *p.vis,
              out.data_ptr(), wp, wn)
    return out


def envmap_shade(normals, positions, camera_center, light_dirs, light_colors, shininess, kd, ks, vis=None):
    """colors [B,NP,3] of the Blinn-Phong environment-map shader (pytorch3d_envmap_shader.py:75-115); with ``vis`` (a mask of
    ``mesh_visibility``) only the directions a pixel sees count: cast shadows."""
    return _shade_call(True, normals, positions, camera_center, light_dirs, light_colors, shininess, kd, ks, vis)


def envmap_shade_backward(normals, positions, camera_center, light_dirs, dcolors, shininess, kd, ks, vis=None):
    """d loss / d light_colors [B,J,3] for an upstream d loss / d colors [B,NP,3] (``vis``: as in the forward call)."""
    return _shade_call(False, normals, positions, camera_center, light_dirs, dcolors, shininess, kd, ks, vis)


def _terms_call(forward: bool, normals, positions, camera_center, light_dirs, srcs, shininess, vis, need_ds=False):
    """reni_envmap_shade_terms / reni_envmap_shade_terms_backward (include/reni_hip.h) behind ``_shade_inputs``.
    srcs: (light colours [B,J,3],) forward, (gD, gS) [B,NP,3] backward; shininess: a float, a one-element tensor or [NP].
    forward None: reni_envmap_shade_terms_dnormals, srcs = (light colours, gD, gS)."""
    dnormals = forward is None
    on_texels = (True,) if forward else (True, False, False) if dnormals else (False, False)
    p = _shade_inputs(normals, positions, camera_center, light_dirs, srcs, on_texels, vis, shininess, "shininess")
    lib, f32, ptr = p.lib, torch.float32, [x.data_ptr() for x in p.srcs]
    if dnormals:
        ws, wp, wn = _ws256(int(lib.reni_envmap_shade_terms_dnormals_workspace_bytes(p.B, p.NP, p.J)), p.dev)
        out = torch.empty((p.NP, 3), dtype=f32, device=p.dev)
        _call(lib.reni_envmap_shade_terms_dnormals, p.dev, *p.head, ptr[0], *p.mats, ptr[1], ptr[2], out.data_ptr(), wp, wn)
        return out
    ws, wp, wn = _ws256(int(lib.reni_envmap_shade_terms_workspace_bytes(p.B, p.NP, p.J, _lib.SHADE_TERMS_DS if need_ds else 0)), p.dev)
    if forward:
        outs = [torch.empty((p.B, p.NP, 3), dtype=f32, device=p.dev) for _ in range(3 if need_ds else 2)]
        _call(lib.reni_envmap_shade_terms, p.dev, *p.head, ptr[0], *p.mats, outs[0].data_ptr(), outs[1].data_ptr(),
              outs[2].data_ptr() if need_ds else None, wp, wn)
        return outs[0], outs[1], (outs[2] if need_ds else None)
    out = torch.empty((p.B, p.J, 3), dtype=f32, device=p.dev)
    _call(lib.reni_envmap_shade_terms_backward, p.dev, *p.head, *p.mats, ptr[0], ptr[1], out.data_ptr(), wp, wn)
    return out


def envmap_shade_terms(normals, positions, camera_center, light_dirs, light_colors, shininess, vis=None, need_ds=False):
    """The shader's terms for per-pixel materials -> (D, S, T | None), each [B,NP,3]: D = sum_j nl C, S = sum_j nh^s_p C
    (no ks, no norm(s): ``envmap_shader.compose_materials`` applies the material) and, with need_ds, T = dS / ds_p =
    sum_j nh^s_p ln nh C.  shininess: a float, a one-element tensor or [NP]; every value must be > 0 (anything else gives
    unspecified values for that pixel).  ``vis``: as for ``envmap_shade``."""
    return _terms_call(True, normals, positions, camera_center, light_dirs, (light_colors,), shininess, vis, need_ds)


def envmap_shade_terms_backward(normals, positions, camera_center, light_dirs, gD, gS, shininess, vis=None):
    """d loss / d light_colors [B,J,3] for upstream gradients gD, gS [B,NP,3] of ``envmap_shade_terms``' D and S."""
    return _terms_call(False, normals, positions, camera_center, light_dirs, (gD, gS), shininess, vis)


def envmap_shade_terms_dnormals(normals, positions, camera_center, light_dirs, light_colors, gD, gS, shininess, vis=None):
    """d loss / d normals [NP,3] for upstream gradients gD, gS [B,NP,3] of ``envmap_shade_terms``' D and S, through
    F.normalize's Jacobian (the normals are given un-normalised).  Strict gates: a pixel with a zero normal gets exactly 0."""
    return _terms_call(None, normals, positions, camera_center, light_dirs, (light_colors, gD, gS), shininess, vis)


def _ggx_call(mode: str, normals, positions, camera_center, light_dirs, srcs, alpha, vis, need_dn=False):
    """reni_envmap_shade_ggx / _backward / _dpixel (include/reni_hip.h) behind ``_shade_inputs``.  mode "forward":
    srcs = (light colours [B,J,3],); "backward": (gD, gS0, gS1) [B,NP,3]; "dpixel": (light colours, gD, gS0, gS1).  alpha: a
    float, a one-element tensor or [NP]."""
    on_texels = {"forward": (True,), "backward": (False, False, False), "dpixel": (True, False, False, False)}[mode]
    p = _shade_inputs(normals, positions, camera_center, light_dirs, srcs, on_texels, vis, alpha, "alpha")
    lib, f32, ptr = p.lib, torch.float32, [x.data_ptr() for x in p.srcs]
    if mode == "dpixel":
        ws, wp, wn = _ws256(int(lib.reni_envmap_shade_ggx_dpixel_workspace_bytes(p.B, p.NP, p.J)), p.dev)
        d_alpha = torch.empty(p.NP, dtype=f32, device=p.dev)
        d_normals = torch.empty((p.NP, 3), dtype=f32, device=p.dev) if need_dn else None
        _call(lib.reni_envmap_shade_ggx_dpixel, p.dev, *p.head, ptr[0], *p.mats, ptr[1], ptr[2], ptr[3], d_alpha.data_ptr(),
              _ptr(d_normals), wp, wn)
        return d_alpha, d_normals
    ws, wp, wn = _ws256(int(lib.reni_envmap_shade_ggx_workspace_bytes(p.B, p.NP, p.J)), p.dev)
    if mode == "forward":
        outs = [torch.empty((p.B, p.NP, 3), dtype=f32, device=p.dev) for _ in range(3)]
        _call(lib.reni_envmap_shade_ggx, p.dev, *p.head, ptr[0], *p.mats, outs[0].data_ptr(), outs[1].data_ptr(),
              outs[2].data_ptr(), wp, wn)
        return tuple(outs)
    out = torch.empty((p.B, p.J, 3), dtype=f32, device=p.dev)
    _call(lib.reni_envmap_shade_ggx_backward, p.dev, *p.head, *p.mats, ptr[0], ptr[1], ptr[2], out.data_ptr(), wp, wn)
    return out


def envmap_shade_ggx(normals, positions, camera_center, light_dirs, light_colors, alpha, vis=None):
    """The microfacet shader's terms -> (D, S0, S1), each [B,NP,3]: D = sum_j nl C (``envmap_shade_terms``' bits), S0 =
    sum_j k C and S1 = sum_j k f C with k the GGX lobe x separable Smith x nl and f = (1 - V.H)^5 (include/reni_hip.h has
    the definition; ``envmap_shader.compose_microfacet`` applies the material).  alpha (= roughness^2): a float, a one-element
    tensor or [NP]; every value must be > 0 (anything else gives unspecified values for that pixel)."""
    return _ggx_call("forward", normals, positions, camera_center, light_dirs, (light_colors,), alpha, vis)


def envmap_shade_ggx_backward(normals, positions, camera_center, light_dirs, gD, gS0, gS1, alpha, vis=None):
    """d loss / d light_colors [B,J,3] for upstream gradients gD, gS0, gS1 [B,NP,3] of ``envmap_shade_ggx``' three terms."""
    return _ggx_call("backward", normals, positions, camera_center, light_dirs, (gD, gS0, gS1), alpha, vis)


def envmap_shade_ggx_dpixel(normals, positions, camera_center, light_dirs, light_colors, gD, gS0, gS1, alpha, vis=None,
                            need_dn=False):
    """(d loss / d alpha [NP], d loss / d normals [NP,3] | None) for upstream gradients of ``envmap_shade_ggx``' terms.  d alpha
    is per pixel also when one alpha serves all pixels (its gradient is then the sum); the normals' gradient goes through
    F.normalize's Jacobian with strict gates (a zero normal gets exactly 0) and is computed only with need_dn, which does not
    move d alpha's bits."""
    return _ggx_call("dpixel", normals, positions, camera_center, light_dirs, (light_colors, gD, gS0, gS1), alpha, vis, need_dn)


def _vertex_face_csr(faces: torch.Tensor, V: int):
    """The faces of every vertex as corner indices 3 f + k, ascending per vertex (a stable sort of the flattened index list on
    the device), and the [V+1] offsets into that list.  Corners whose index lies outside [0, V) are left out."""
    flat = faces.reshape(-1)
    corners = torch.arange(flat.numel(), device=flat.device, dtype=torch.int64)
    ok = (flat >= 0) & (flat < V)
    keys, corners = flat[ok], corners[ok]
    keys, order = torch.sort(keys, stable=True)
    offsets = torch.searchsorted(keys, torch.arange(V + 1, device=flat.device, dtype=torch.int64))
    return offsets.contiguous(), corners[order].contiguous()


def _mesh_shapes(verts, faces, a_tensor="a tensor "):
    """The shape rules of a mesh.  Asked first by the callers whose bad shape is a ValueError before any device is looked at
    (anything may arrive: the message says "a tensor"), and by ``_mesh_inputs`` on the cast tensors (``a_tensor=""``)."""
    for name, t, n in (("verts", verts, "V"), ("faces", faces, "F")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"{name} must be {a_tensor}[{n}, 3] with {n} >= 1, got {tuple(getattr(t, 'shape', ()))}")


def _mesh_inputs(verts, faces):
    _require_cuda(verts, faces)
    verts = verts.to(torch.float32).contiguous()
    faces = faces.to(torch.int64).contiguous()
    _mesh_shapes(verts, faces, "")
    if faces.device != verts.device:
        raise ValueError("verts and faces must be on the same device")
    return verts, faces


def _image_size(image_size) -> int:
    S = int(image_size)
    if S < 1:
        raise ValueError("image_size must be >= 1")
    return S


def _camera_arrays(R, T):
    """R ([1,3,3] or [3,3]) and T ([1,3] or [3]) as the C ABI's float[9] and float[3]."""
    Rv = [float(x) for x in torch.as_tensor(R).reshape(-1).tolist()]
    Tv = [float(x) for x in torch.as_tensor(T).reshape(-1).tolist()]
    if len(Rv) != 9 or len(Tv) != 3:
        raise ValueError("R must hold 9 values ([1,3,3] or [3,3]) and T 3 ([1,3] or [3])")
    return (ctypes.c_float * 9)(*Rv), (ctypes.c_float * 3)(*Tv)


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, vf=None) -> torch.Tensor:
    """reni_mesh_vertex_normals: Meshes.verts_normals_packed() of one mesh, [V, 3] -- the area-weighted sum of the adjacent
    faces' cross(v1 - v0, v2 - v0), normalised with max(|n|, 1e-6).  Deterministic (a gather in ascending face order).
    ``vf``: ``vertex_face_lists(faces, V)`` when the caller keeps it (the same lists, the same bits)."""
    verts, faces = _mesh_inputs(verts, faces)
    V, F = verts.shape[0], faces.shape[0]
    offsets, corners = _vf_lists(faces, V, vf)
    out = torch.empty(V, 3, dtype=torch.float32, device=verts.device)
    _call(_lib.load().reni_mesh_vertex_normals, verts.device, V, F, verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(),
          corners.data_ptr(), out.data_ptr())
    return out


def rasterize_mesh(verts: torch.Tensor, faces: torch.Tensor, vert_normals: torch.Tensor, R, T, image_size: int,
                   tan_half_fov: float = 0.5773502691896258):
    """reni_rasterize_mesh: one mesh seen by FoVPerspectiveCameras (default tan(fov/2) = tan 30 deg) with world-to-view
    p R + T, rasterised at image_size^2 with one face per pixel, and the shader's G-buffer.  Returns
    (pix_to_face [1,S,S,1] int64, zbuf [1,S,S,1], bary [1,S,S,1,3], dists [1,S,S,1], pixel_normals [S*S,3],
    pixel_positions [S*S,3]) -- the first four are pytorch3d's Fragments, the last two interpolate_face_attributes of the
    vertex normals / positions (not normalised)."""
    verts, faces = _mesh_inputs(verts, faces)
    _require_cuda(vert_normals)
    vert_normals = vert_normals.to(torch.float32).contiguous()
    if tuple(vert_normals.shape) != tuple(verts.shape):
        raise ValueError("vert_normals must be [V, 3] like verts")
    S = _image_size(image_size)
    Rh, Th = _camera_arrays(R, T)
    lib = _lib.load()
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    p2f = torch.empty(1, S, S, 1, dtype=torch.int64, device=dev)
    zbuf = torch.empty(1, S, S, 1, dtype=torch.float32, device=dev)
    bary = torch.empty(1, S, S, 1, 3, dtype=torch.float32, device=dev)
    dists = torch.empty(1, S, S, 1, dtype=torch.float32, device=dev)
    nrm = torch.empty(S * S, 3, dtype=torch.float32, device=dev)
    pos = torch.empty(S * S, 3, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_raster_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_rasterize_mesh, dev, V, F, verts.data_ptr(), faces.data_ptr(), vert_normals.data_ptr(), Rh, Th, float(tan_half_fov),
          S, S, p2f.data_ptr(), zbuf.data_ptr(), bary.data_ptr(), dists.data_ptr(), nrm.data_ptr(), pos.data_ptr(), wp, wn)
    return p2f, zbuf, bary, dists, nrm, pos


def vertex_face_lists(faces: torch.Tensor, V: int):
    """(offsets [V + 1], corners) int64: the faces of every vertex as corner indices 3 f + k, ascending per vertex -- what
    ``vertex_normals_backward`` and ``gbuffer_backward`` gather through (``vf=``).  It depends on the faces alone: a caller
    whose vertices move every step keeps it."""
    offsets, corners = _vertex_face_csr(faces.to(torch.int64).contiguous(), int(V))
    if corners.numel() == 0:
        corners = torch.zeros(1, dtype=torch.int64, device=faces.device)  # (never read: every vertex's range is empty)
    return offsets, corners


def _vf_lists(faces, V, vf):
    if vf is None:
        return vertex_face_lists(faces, V)
    offsets, corners = vf
    if (not isinstance(offsets, torch.Tensor) or not isinstance(corners, torch.Tensor) or tuple(offsets.shape) != (V + 1,)
            or corners.dim() != 1 or corners.numel() < 1 or offsets.dtype != torch.int64 or corners.dtype != torch.int64
            or offsets.device != faces.device or corners.device != faces.device):
        raise ValueError(f"vf must be vertex_face_lists(faces, {V}) on {faces.device}")
    return offsets.contiguous(), corners.contiguous()


def vertex_normals_backward(verts: torch.Tensor, faces: torch.Tensor, grad_normals: torch.Tensor, vf=None) -> torch.Tensor:
    """reni_mesh_vertex_normals_backward: grad_verts [V, 3] = d/d verts of sum_v grad_normals[v] . n_v for the normals of
    ``vertex_normals`` (the Jacobian of u / max(|u|, 1e-6), then the cross products to every vertex of every incident face).
    Deterministic: gathers in ascending face order, no atomics."""
    _mesh_shapes(verts, faces)
    if not isinstance(grad_normals, torch.Tensor) or tuple(grad_normals.shape) != tuple(verts.shape):
        raise ValueError(f"grad_normals must be [V, 3] like verts, got {tuple(getattr(grad_normals, 'shape', ()))}")
    verts, faces = _mesh_inputs(verts, faces)
    _require_cuda(grad_normals)
    grad_normals = _f32c(grad_normals)
    if grad_normals.device != verts.device:
        raise ValueError("grad_normals is not on the mesh's device")
    V, F = verts.shape[0], faces.shape[0]
    offsets, corners = _vf_lists(faces, V, vf)
    out = torch.empty(V, 3, dtype=torch.float32, device=verts.device)
    _call(_lib.load().reni_mesh_vertex_normals_backward, verts.device, V, F, verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(),
          corners.data_ptr(), grad_normals.data_ptr(), out.data_ptr())
    return out


def face_pixel_table(pix_to_face: torch.Tensor, F: int):
    """What ``gbuffer_backward`` walks a face's pixels through: (offsets [F + 1] int64, pixels [S*S] int64) from the
    rasteriser's pix_to_face -- a stable sort on the device and a searchsorted that bins the pixels per face, as
    ``texture_table`` does.  The background (-1) sorts in front of offsets[0], anything >= F behind offsets[F]."""
    keys, order = torch.sort(pix_to_face.reshape(-1), stable=True)
    offsets = torch.searchsorted(keys, torch.arange(int(F) + 1, device=keys.device, dtype=torch.int64))
    return offsets.contiguous(), order.contiguous()


def _gbuffer_backward_inputs(verts, faces, vert_normals, R, T, image_size, pix_to_face, grad_pixel_normals, grad_pixel_positions,
                             tan_half_fov, table, vf, need_lists):
    """What ``gbuffer_backward`` and ``gbuffer_backward_camera`` share: the checks, in their order, the casts, the pixel table
    and the vertex lists (not built, and NULL in the call, when not needed) -> (device, V, F, S, the arguments the two entry
    points have in common -- everything in front of grad_verts --, the tensors those point into)."""
    _mesh_shapes(verts, faces)
    S = _image_size(image_size)
    if not isinstance(vert_normals, torch.Tensor) or tuple(vert_normals.shape) != tuple(verts.shape):
        raise ValueError("vert_normals must be [V, 3] like verts")
    if not isinstance(pix_to_face, torch.Tensor) or pix_to_face.dtype != torch.int64 or pix_to_face.numel() != S * S:
        raise ValueError(f"pix_to_face must be an int64 tensor of {S * S} entries (the rasteriser's)")
    if grad_pixel_normals is None and grad_pixel_positions is None:
        raise ValueError("grad_pixel_normals and grad_pixel_positions cannot both be None")
    for name, g in (("grad_pixel_normals", grad_pixel_normals), ("grad_pixel_positions", grad_pixel_positions)):
        if g is not None and (not isinstance(g, torch.Tensor) or tuple(g.shape) != (S * S, 3)):
            raise ValueError(f"{name} must be [{S * S}, 3] or None, got {tuple(getattr(g, 'shape', ()))}")
    Rh, Th = _camera_arrays(R, T)
    verts, faces = _mesh_inputs(verts, faces)
    _require_cuda(vert_normals, pix_to_face, grad_pixel_normals, grad_pixel_positions)
    dev = verts.device
    vert_normals = _f32c(vert_normals)
    p2f = pix_to_face.reshape(-1).contiguous()
    gN = None if grad_pixel_normals is None else _f32c(grad_pixel_normals)
    gX = None if grad_pixel_positions is None else _f32c(grad_pixel_positions)
    if any(t is not None and t.device != dev for t in (vert_normals, p2f, gN, gX)):
        raise ValueError(f"the G-buffer and its gradients are not on {dev}")
    V, F = verts.shape[0], faces.shape[0]
    foff, flist = face_pixel_table(p2f, F) if table is None else table
    if (tuple(foff.shape) != (F + 1,) or tuple(flist.shape) != (S * S,) or foff.dtype != torch.int64 or flist.dtype != torch.int64
            or foff.device != dev or flist.device != dev):
        raise ValueError(f"the table is not one of {S * S} pixels over {F} faces on {dev}")
    foff, flist = foff.contiguous(), flist.contiguous()
    offsets, corners = _vf_lists(faces, V, vf) if need_lists else (None, None)
    head = (V, F, verts.data_ptr(), faces.data_ptr(), vert_normals.data_ptr(), Rh, Th, float(tan_half_fov), S, S, p2f.data_ptr(),
            foff.data_ptr(), flist.data_ptr(), _ptr(offsets), _ptr(corners), _ptr(gN), _ptr(gX))
    return dev, V, F, S, head, (verts, faces, vert_normals, p2f, foff, flist, offsets, corners, gN, gX)


def gbuffer_backward(verts: torch.Tensor, faces: torch.Tensor, vert_normals: torch.Tensor, R, T, image_size: int,
                     pix_to_face: torch.Tensor, grad_pixel_normals=None, grad_pixel_positions=None,
                     tan_half_fov: float = 0.5773502691896258, table=None, vf=None) -> torch.Tensor:
    """reni_gbuffer_backward: grad_verts [V, 3] = d/d verts of sum_p (gN_p . N_p + gX_p . X_p) for the G-buffer of
    ``rasterize_mesh`` (N = pixel_normals, X = pixel_positions) with pix_to_face held fixed: through the interpolation
    weights' dependence on the projected corners, the interpolated positions, and -- for gN -- the vertex normals
    (``vertex_normals``' chain included: vert_normals must be the normals of verts, and is a constant here).  Either upstream
    gradient ([S*S, 3]) may be None, not both.  ``table``: ``face_pixel_table(pix_to_face, F)``, ``vf``: ``vertex_face_lists(faces, V)``, when the caller keeps them.
    Deterministic, no atomics; no silhouette / occlusion gradient, the camera is a constant."""
    dev, V, F, S, head, keep = _gbuffer_backward_inputs(verts, faces, vert_normals, R, T, image_size, pix_to_face, grad_pixel_normals,
                                                        grad_pixel_positions, tan_half_fov, table, vf, True)
    lib = _lib.load()
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_gbuffer_backward_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_gbuffer_backward, dev, *head, out.data_ptr(), wp, wn)
    return out


def _camera_gradient(cam: torch.Tensor):
    """grad_camera [13] -> (gR [3,3], gT [3], g_tan [])"""
    return cam[:9].reshape(3, 3), cam[9:12], cam[12]


def gbuffer_backward_camera(verts: torch.Tensor, faces: torch.Tensor, vert_normals: torch.Tensor, R, T, image_size: int,
                            pix_to_face: torch.Tensor, grad_pixel_normals=None, grad_pixel_positions=None,
                            tan_half_fov: float = 0.5773502691896258, table=None, vf=None, need_verts: bool = True):
    """reni_gbuffer_backward_camera: ``gbuffer_backward`` with the camera's gradient beside the vertices' ->
    (g_verts [V,3] | None, gR [3,3], gT [3], g_tan []): d/d R, d/d T and d/d tan_half_fov of the same objective, through the
    barycentric weights alone (the vertex normals and the interpolated positions are world-space), pix_to_face held fixed; R is
    differentiated as nine free numbers.  g_verts has ``gbuffer_backward``'s bits.  ``need_verts=False``: the mesh is known and
    only the pose is fitted -- the vertex kernels are not launched, no vertex list is built, g_verts is None; the camera's bits
    do not move.  Deterministic, no atomics."""
    dev, V, F, S, head, keep = _gbuffer_backward_inputs(verts, faces, vert_normals, R, T, image_size, pix_to_face, grad_pixel_normals,
                                                        grad_pixel_positions, tan_half_fov, table, vf, need_verts)
    lib = _lib.load()
    out = torch.empty(V, 3, dtype=torch.float32, device=dev) if need_verts else None
    cam = torch.empty(13, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_gbuffer_backward_camera_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_gbuffer_backward_camera, dev, *head, _ptr(out), cam.data_ptr(), wp, wn)
    return (out,) + _camera_gradient(cam)


def _silhouette_scalars(sigma, blur_radius):
    sigma, blur_radius = float(sigma), float(blur_radius)
    if not (sigma > 0.0) or not math.isfinite(sigma):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    if not (blur_radius >= 0.0) or not math.isfinite(blur_radius):
        raise ValueError(f"blur_radius must be >= 0 and finite, got {blur_radius}")
    return sigma, blur_radius


def soft_silhouette(verts: torch.Tensor, faces: torch.Tensor, R, T, image_size: int, tan_half_fov: float, sigma: float,
                    blur_radius: float):
    """reni_soft_silhouette: (alpha [S*S], trans [S*S]) of one mesh under ``rasterize_mesh``'s camera and pixel grid -- the soft
    coverage alpha_p = 1 - prod_f (1 - prob_f(p)), prob = 1 / (1 + exp(sd / sigma)) with sd the signed squared NDC distance of
    the pixel centre to the face's boundary (negative inside), over every face with all view z > 0 that holds the pixel or lies
    within ``blur_radius`` (squared NDC units) of it, in ascending face order.  trans = 1 - alpha's product is what
    ``soft_silhouette_backward`` reads.  Deterministic, no atomics."""
    _mesh_shapes(verts, faces)
    S = _image_size(image_size)
    sigma, blur_radius = _silhouette_scalars(sigma, blur_radius)
    Rh, Th = _camera_arrays(R, T)
    verts, faces = _mesh_inputs(verts, faces)
    lib = _lib.load()
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    alpha = torch.empty(S * S, dtype=torch.float32, device=dev)
    trans = torch.empty(S * S, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_soft_silhouette_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_soft_silhouette, dev, V, F, verts.data_ptr(), faces.data_ptr(), Rh, Th, float(tan_half_fov), S, S, sigma,
          blur_radius, alpha.data_ptr(), trans.data_ptr(), wp, wn)
    return alpha, trans


def _silhouette_backward_inputs(verts, faces, R, T, image_size, tan_half_fov, sigma, blur_radius, trans, grad_alpha, vf, need_lists):
    """What ``soft_silhouette_backward`` and ``soft_silhouette_backward_camera`` share: the checks, in their order, the casts
    and the vertex lists (not built, and NULL in the call, when not needed) -> (device, V, F, S, the arguments the two entry
    points have in common -- everything in front of grad_verts --, the tensors those point into)."""
    _mesh_shapes(verts, faces)
    S = _image_size(image_size)
    sigma, blur_radius = _silhouette_scalars(sigma, blur_radius)
    for name, t in (("trans", trans), ("grad_alpha", grad_alpha)):
        if not isinstance(t, torch.Tensor) or t.numel() != S * S:
            raise ValueError(f"{name} must be a tensor of {S * S} entries, got {tuple(getattr(t, 'shape', ()))}")
    Rh, Th = _camera_arrays(R, T)
    verts, faces = _mesh_inputs(verts, faces)
    _require_cuda(trans, grad_alpha)
    dev = verts.device
    trans, grad_alpha = _f32c(trans).reshape(-1), _f32c(grad_alpha).reshape(-1)
    if trans.device != dev or grad_alpha.device != dev:
        raise ValueError(f"trans and grad_alpha are not on {dev}")
    V, F = verts.shape[0], faces.shape[0]
    offsets, corners = _vf_lists(faces, V, vf) if need_lists else (None, None)
    head = (V, F, verts.data_ptr(), faces.data_ptr(), Rh, Th, float(tan_half_fov), S, S, sigma, blur_radius, trans.data_ptr(),
            grad_alpha.data_ptr(), _ptr(offsets), _ptr(corners))
    return dev, V, F, S, head, (verts, faces, trans, grad_alpha, offsets, corners)


def soft_silhouette_backward(verts: torch.Tensor, faces: torch.Tensor, R, T, image_size: int, tan_half_fov: float, sigma: float,
                             blur_radius: float, trans: torch.Tensor, grad_alpha: torch.Tensor, vf=None) -> torch.Tensor:
    """reni_soft_silhouette_backward: grad_verts [V, 3] = d/d verts of sum_p grad_alpha_p alpha_p for the alpha of
    ``soft_silhouette`` (``trans`` as it returned it), with membership, inside / outside, the nearest edge and a clamped edge
    parameter held constant; the camera is a constant.  ``vf``: ``vertex_face_lists(faces, V)`` when the caller keeps it.
    Deterministic, no atomics."""
    dev, V, F, S, head, keep = _silhouette_backward_inputs(verts, faces, R, T, image_size, tan_half_fov, sigma, blur_radius, trans,
                                                           grad_alpha, vf, True)
    lib = _lib.load()
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_soft_silhouette_backward_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_soft_silhouette_backward, dev, *head, out.data_ptr(), wp, wn)
    return out


def soft_silhouette_backward_camera(verts: torch.Tensor, faces: torch.Tensor, R, T, image_size: int, tan_half_fov: float,
                                    sigma: float, blur_radius: float, trans: torch.Tensor, grad_alpha: torch.Tensor, vf=None,
                                    need_verts: bool = True):
    """reni_soft_silhouette_backward_camera: ``soft_silhouette_backward`` with the camera's gradient beside the vertices' ->
    (g_verts [V,3] | None, gR [3,3], gT [3], g_tan []): d/d R, d/d T and d/d tan_half_fov of sum_p grad_alpha_p alpha_p under
    the same constants (membership, inside / outside, the nearest edge, a clamped edge parameter, blur_radius); R is
    differentiated as nine free numbers.  g_verts has ``soft_silhouette_backward``'s bits.  ``need_verts=False``: the mesh is
    known and only the pose is fitted -- the vertex kernel is not launched, no vertex list is built, g_verts is None; the
    camera's bits do not move.  Deterministic, no atomics."""
    dev, V, F, S, head, keep = _silhouette_backward_inputs(verts, faces, R, T, image_size, tan_half_fov, sigma, blur_radius, trans,
                                                           grad_alpha, vf, need_verts)
    lib = _lib.load()
    out = torch.empty(V, 3, dtype=torch.float32, device=dev) if need_verts else None
    cam = torch.empty(13, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_soft_silhouette_backward_camera_workspace_bytes(V, F, S, S)), dev)
    _call(lib.reni_soft_silhouette_backward_camera, dev, *head, _ptr(out), cam.data_ptr(), wp, wn)
    return (out,) + _camera_gradient(cam)


_EDGE_LIST_NAMES = ("edges", "ef_offsets", "ef_corners", "ve_offsets", "ve_edges", "vf_offsets", "vf_corners", "corner_edges")


def _pad1(t: torch.Tensor) -> torch.Tensor:
    """an empty list as one never-read entry, so that it still has an address"""
    return t if t.numel() else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)


def mesh_edge_lists(faces: torch.Tensor, V: int) -> dict:
    """The topology lists of ``mesh_regularizers`` (``lists=``), all int64 and ascending, built by stable sorts on the faces'
    device.  A face takes part iff its indices lie in [0, V) and are pairwise different.

    ``edges`` [E, 2]: the unique undirected edges (a < b) of the faces taking part, in ascending (a, b);
    ``ef_offsets`` [E + 1] / ``ef_corners``: per edge the corners 3 f + k OPPOSITE it of the faces holding it, ascending (so an
    edge of multiplicity m has m entries and m (m - 1) / 2 pairs);  ``ve_offsets`` [V + 1] / ``ve_edges`` [2 E]: per vertex its
    edges, ascending;  ``vf_offsets`` / ``vf_corners``: ``vertex_face_lists``;  ``corner_edges`` [3 F]: the edge opposite each
    corner, -1 for a face that takes no part;  ``E``, ``H`` (half edges), ``NC`` (corners), ``P`` (pairs), ``V``, ``F``: ints.
    The lists depend on the faces alone: a caller whose vertices move every step keeps them."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"faces must be a tensor [F, 3] with F >= 1, got {tuple(getattr(faces, 'shape', ()))}")
    V = int(V)
    if V < 1:
        raise ValueError("V must be >= 1")
    faces = faces.to(torch.int64).contiguous()
    dev, F = faces.device, faces.shape[0]
    part = ((faces >= 0) & (faces < V)).all(dim=1)
    part = part & (faces[:, 0] != faces[:, 1]) & (faces[:, 0] != faces[:, 2]) & (faces[:, 1] != faces[:, 2])
    f = part.nonzero()[:, 0]
    tri = faces[f]
    # corner k of face f is opposite the edge of the other two corners
    p = torch.stack([tri[:, 1], tri[:, 0], tri[:, 0]], 1).reshape(-1)
    q = torch.stack([tri[:, 2], tri[:, 2], tri[:, 1]], 1).reshape(-1)
    corners = (3 * f[:, None] + torch.arange(3, device=dev, dtype=torch.int64)[None, :]).reshape(-1)
    keys, order = torch.sort(torch.minimum(p, q) * V + torch.maximum(p, q), stable=True)  # ascending (a, b), then corner
    ef_corners = corners[order]
    ukeys, counts = torch.unique_consecutive(keys, return_counts=True)
    E = int(ukeys.numel())
    edges = torch.stack([ukeys // V, ukeys % V], 1)
    ef_offsets = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    ef_offsets[1:] = torch.cumsum(counts, 0)
    corner_edges = torch.full((3 * F,), -1, dtype=torch.int64, device=dev)
    corner_edges[ef_corners] = torch.repeat_interleave(torch.arange(E, device=dev, dtype=torch.int64), counts)
    ends = edges.reshape(-1)  # entry 2 e + s names edge e
    vkeys, vorder = torch.sort(ends, stable=True)
    ve_edges = torch.div(vorder, 2, rounding_mode="floor")
    ve_offsets = torch.searchsorted(vkeys, torch.arange(V + 1, device=dev, dtype=torch.int64))
    vf_offsets, vf_corners = _vertex_face_csr(faces, V)
    NC = int(vf_corners.numel())
    P = int((counts * (counts - 1) // 2).sum()) if E else 0
    out = {"edges": _pad1(edges.contiguous()), "ef_offsets": ef_offsets, "ef_corners": _pad1(ef_corners.contiguous()),
           "ve_offsets": ve_offsets.contiguous(), "ve_edges": _pad1(ve_edges.contiguous()), "vf_offsets": vf_offsets,
           "vf_corners": _pad1(vf_corners), "corner_edges": corner_edges, "V": V, "F": F, "E": E, "H": int(ef_corners.numel()),
           "NC": NC, "P": P}
    return out


def _edge_lists(faces, V, lists):
    """``lists`` checked by shape, dtype and device (their CONTENT is checked on the device, entry by entry)"""
    if lists is None:
        return mesh_edge_lists(faces, V)
    F = faces.shape[0]
    try:
        E, H, NC = int(lists["E"]), int(lists["H"]), int(lists["NC"])
        t = {k: lists[k] for k in _EDGE_LIST_NAMES}
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"lists must be mesh_edge_lists(faces, {V})") from None
    want = {"edges": (max(E, 1), 2), "ef_offsets": (E + 1,), "ef_corners": (max(H, 1),), "ve_offsets": (V + 1,),
            "ve_edges": (max(2 * E, 1),), "vf_offsets": (V + 1,), "vf_corners": (max(NC, 1),), "corner_edges": (3 * F,)}
    ok = E >= 0 and 0 <= H <= 3 * F and 0 <= NC <= 3 * F and int(lists.get("V", V)) == V and int(lists.get("F", F)) == F
    for k in _EDGE_LIST_NAMES:
        x = t[k]
        ok = ok and isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.device == faces.device and tuple(x.shape) == want[k]
    if not ok:
        raise ValueError(f"lists must be mesh_edge_lists(faces, {V}) on {faces.device}")
    out = dict(lists)
    out.update({k: t[k].contiguous() for k in _EDGE_LIST_NAMES})
    return out


def mesh_regularizers(verts: torch.Tensor, faces: torch.Tensor, edge: float = 0.0, laplacian: float = 0.0, normal: float = 0.0,
                      target_length: float = 0.0, method: str = "uniform", lists=None, need_grad: bool = True):
    """reni_mesh_regularizers: (values [4] = (L, L_e, L_l, L_n), grad_verts [V, 3] | None) of
    L = edge L_e + laplacian L_l + normal L_n -- the edge-length, Laplacian-smoothing (``method`` "uniform" or "cot") and
    normal-consistency terms of SoftRas / pytorch3d.loss (include/reni_hip.h has the definitions) and d L / d verts, from one
    call.  A weight of 0 skips that term.  ``lists``: ``mesh_edge_lists(faces, V)`` when the caller keeps it (the same bits).
    ``need_grad=False``: the values alone (the same bits).  Deterministic, no atomics."""
    _mesh_shapes(verts, faces)
    if method not in _lib.LAPLACIAN:
        raise ValueError(f"method must be one of {tuple(_lib.LAPLACIAN)}, got {method!r}")
    w = [float(edge), float(laplacian), float(normal)]
    target_length = float(target_length)
    for name, x in (("edge", w[0]), ("laplacian", w[1]), ("normal", w[2]), ("target_length", target_length)):
        if not (x >= 0.0) or not math.isfinite(x):
            raise ValueError(f"{name} must be >= 0 and finite, got {x}")
    verts, faces = _mesh_inputs(verts, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    L = _edge_lists(faces, V, lists)
    lib = _lib.load()
    values = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty(V, 3, dtype=torch.float32, device=dev) if need_grad else None
    ws, wp, wn = _ws256(int(lib.reni_mesh_regularizers_workspace_bytes(V, F, L["E"])), dev)
    _call(lib.reni_mesh_regularizers, dev, V, F, L["E"], L["H"], L["NC"], verts.data_ptr(), faces.data_ptr(),
          *[L[k].data_ptr() for k in _EDGE_LIST_NAMES], w[0], w[1], w[2], target_length, _lib.LAPLACIAN[method], values.data_ptr(),
          _ptr(grad), wp, wn)
    return values, grad


def _cloud(t, name):
    """The shape rule of a point cloud, a ValueError before any device is looked at"""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{name} must be a tensor [N, 3] with N >= 1, got {tuple(getattr(t, 'shape', ()))}")


def _cloud_pair(x, y):
    _cloud(x, "x")
    _cloud(y, "y")
    _require_cuda(x, y)
    x, y = _f32c(x.detach()), _f32c(y.detach())
    if y.device != x.device:
        raise ValueError("x and y must be on the same device")
    return x, y


def nearest_points(x: torch.Tensor, y: torch.Tensor, slices: int = 0):
    """reni_nearest_points: (dist2 [N] float32, idx [N] int64) -- for every x_i the LOWEST index of the nearest y_j under
    d = fmaf(dz, dz, fmaf(dy, dy, dx dx)) and that d.  Brute force through LDS tiles, never an N x M matrix; ``slices`` cuts the
    target range over more workgroups (0: the library's choice) and never changes a bit of the result."""
    slices = int(slices)
    if slices < 0:
        raise ValueError("slices must be >= 0")
    x, y = _cloud_pair(x, y)
    N, M, dev = x.shape[0], y.shape[0], x.device
    lib = _lib.load()
    dist2 = torch.empty(N, dtype=torch.float32, device=dev)
    idx = torch.empty(N, dtype=torch.int64, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_nearest_points_workspace_bytes(N, M)), dev)
    _call(lib.reni_nearest_points, dev, N, M, x.data_ptr(), y.data_ptr(), slices, dist2.data_ptr(), idx.data_ptr(), wp, wn)
    return dist2, idx


def chamfer_table(idx_yx: torch.Tensor, N: int):
    """What ``chamfer_grad`` gathers its second term through: (order [M] int64, offsets [N + 1] int64) from idx_yx [M], the
    nearest x of every y -- a stable sort and a searchsorted, as ``texture_table``'s.  An entry outside [0, N) falls outside
    every range."""
    if not isinstance(idx_yx, torch.Tensor) or idx_yx.dim() != 1 or idx_yx.dtype != torch.int64 or idx_yx.numel() < 1:
        raise ValueError("idx_yx must be an int64 tensor [M] with M >= 1")
    N = int(N)
    if N < 1:
        raise ValueError("N must be >= 1")
    keys, order = torch.sort(idx_yx, stable=True)
    offsets = torch.searchsorted(keys, torch.arange(N + 1, device=idx_yx.device, dtype=torch.int64))
    return order.contiguous(), offsets.to(torch.int64).contiguous()


def chamfer_grad(x: torch.Tensor, y: torch.Tensor, idx_xy, table, weights=(1.0, 1.0), g=None) -> torch.Tensor:
    """reni_chamfer_grad: grad_x [N, 3] of L = (w_x / N) sum_i dist2_x[i] + (w_y / M) sum_j dist2_y[j] times the device scalar
    ``g`` (None: 1), with the matches held constant: idx_xy [N] is x's nearest y, table = ``chamfer_table(idx_yx, N)``.  A weight
    of 0 skips its term (its list may be None).  Deterministic, no atomics.  With x, y and the weights swapped it is grad_y."""
    _cloud(x, "x")
    _cloud(y, "y")
    wx, wy = (float(w) for w in weights)
    for name, w in (("w_x", wx), ("w_y", wy)):
        if not (w >= 0.0) or not math.isfinite(w):
            raise ValueError(f"{name} must be >= 0 and finite, got {w}")
    N, M = x.shape[0], y.shape[0]
    if wx > 0.0 and (not isinstance(idx_xy, torch.Tensor) or tuple(idx_xy.shape) != (N,) or idx_xy.dtype != torch.int64):
        raise ValueError(f"idx_xy must be an int64 tensor [{N}]")
    order = offsets = None
    if wy > 0.0:
        try:
            order, offsets = table
        except (TypeError, ValueError):
            raise ValueError(f"table must be chamfer_table(idx_yx, {N})") from None
        if (not isinstance(order, torch.Tensor) or not isinstance(offsets, torch.Tensor) or tuple(order.shape) != (M,)
                or tuple(offsets.shape) != (N + 1,) or order.dtype != torch.int64 or offsets.dtype != torch.int64):
            raise ValueError(f"table must be chamfer_table(idx_yx, {N}) of {M} points")
    if wx == 0.0:
        idx_xy = None
    x, y = _cloud_pair(x, y)
    dev = x.device
    _require_cuda(idx_xy, order, offsets, g)
    for t in (idx_xy, order, offsets, g):
        if t is not None and t.device != dev:
            raise ValueError(f"the lists and g must be on {dev}")
    if g is None:
        g = torch.ones(1, dtype=torch.float32, device=dev)
    elif not isinstance(g, torch.Tensor) or g.numel() != 1:
        raise ValueError("g must hold one value")
    g = _f32c(g.detach()).reshape(1)
    idx_xy, order, offsets = (None if t is None else t.contiguous() for t in (idx_xy, order, offsets))
    grad = torch.empty(N, 3, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_chamfer_grad, dev, N, M, x.data_ptr(), y.data_ptr(), _ptr(idx_xy), _ptr(order), _ptr(offsets), wx, wy,
          g.data_ptr(), grad.data_ptr())
    return grad


def mesh_sample_table(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """reni_mesh_sample_table: table [2, F] float32 -- the faces' areas (0 for a face that takes no part or has no finite area)
    and their CDF, ascending, flat over faces without area, ending on exactly 1 (all 0 for a mesh without area)."""
    _mesh_shapes(verts, faces)
    verts, faces = _mesh_inputs(verts.detach(), faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    lib = _lib.load()
    table = torch.empty(2, F, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_mesh_sample_table_workspace_bytes(F)), dev)
    _call(lib.reni_mesh_sample_table, dev, V, F, verts.data_ptr(), faces.data_ptr(), table.data_ptr(), wp, wn)
    return table


def mesh_sample_points(faces: torch.Tensor, table: torch.Tensor, u: torch.Tensor, V: int):
    """reni_mesh_sample_points: (tap_index [S, 8] int32, tap_weight [S, 8] float32, face_idx [S] int64) for u [S, 3] in [0, 1):
    the face by area from u[:, 0] through ``table = mesh_sample_table(verts, faces)``, pytorch3d's barycentrics from the other
    two.  The taps are the texture unit's: the points are ``texture_fetch(verts, tap_index, tap_weight)``."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"faces must be a tensor [F, 3] with F >= 1, got {tuple(getattr(faces, 'shape', ()))}")
    F, V = faces.shape[0], int(V)
    if V < 1:
        raise ValueError("V must be >= 1")
    if not isinstance(table, torch.Tensor) or tuple(table.shape) != (2, F) or table.dtype != torch.float32:
        raise ValueError(f"table must be mesh_sample_table(verts, faces): float32 [2, {F}]")
    if not isinstance(u, torch.Tensor) or u.dim() != 2 or u.shape[1] != 3 or u.shape[0] < 1:
        raise ValueError(f"u must be a tensor [S, 3] with S >= 1, got {tuple(getattr(u, 'shape', ()))}")
    _require_cuda(faces, table, u)
    faces, table, u = faces.to(torch.int64).contiguous(), table.contiguous(), _f32c(u)
    dev, S = faces.device, u.shape[0]
    if table.device != dev or u.device != dev:
        raise ValueError(f"table and u must be on {dev}")
    idx = torch.empty(S, 8, dtype=torch.int32, device=dev)
    wgt = torch.empty(S, 8, dtype=torch.float32, device=dev)
    face_idx = torch.empty(S, dtype=torch.int64, device=dev)
    _call(_lib.load().reni_mesh_sample_points, dev, V, F, S, faces.data_ptr(), table.data_ptr(), u.data_ptr(), idx.data_ptr(),
          wgt.data_ptr(), face_idx.data_ptr())
    return idx, wgt, face_idx


def _point_mesh(entry, points, verts, faces, slices):
    slices = int(slices)
    if slices < 0:
        raise ValueError("slices must be >= 0")
    _cloud(points, "points")
    _mesh_shapes(verts, faces)
    _require_cuda(points)
    points = _f32c(points.detach())
    verts, faces = _mesh_inputs(verts.detach(), faces)
    if verts.device != points.device:
        raise ValueError("points and the mesh must be on the same device")
    N, V, F, dev = points.shape[0], verts.shape[0], faces.shape[0], points.device
    lib = _lib.load()
    n = F if entry == "reni_faces_nearest_points" else N
    dist2 = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    # (fresh allocations: 16-byte aligned, as the library's row stores and the fetch want -- the library checks)
    tap_index = torch.empty(n, 8, dtype=torch.int32, device=dev)
    tap_weight = torch.empty(n, 8, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(getattr(lib, entry + "_workspace_bytes")(N, V, F)), dev)
    _call(getattr(lib, entry), dev, N, V, F, points.data_ptr(), verts.data_ptr(), faces.data_ptr(), slices, dist2.data_ptr(),
          idx.data_ptr(), tap_index.data_ptr(), tap_weight.data_ptr(), wp, wn)
    return dist2, idx, tap_index, tap_weight


def nearest_faces(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, slices: int = 0):
    """reni_nearest_faces: (dist2 [N] float32, face_idx [N] int64, tap_index [N, 8] int32, tap_weight [N, 8] float32) -- for every
    point the LOWEST index of the nearest triangle under the pair function of include/reni_hip.h, that squared distance, and
    the closest point as a tap row of the texture unit: the face's vertices and the barycentric weights, so the closest points
    are ``texture_fetch(verts, tap_index, tap_weight)``.  Where no face takes part: -1, +inf and zero taps.  Brute force through
    LDS tiles, never an N x F matrix; ``slices`` cuts the faces over more workgroups (0: the library's choice) and never changes
    a bit of the result."""
    return _point_mesh("reni_nearest_faces", points, verts, faces, slices)


def faces_nearest_points(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, slices: int = 0):
    """reni_faces_nearest_points: (dist2 [F] float32, point_idx [F] int64, tap_index [F, 8] int32, tap_weight [F, 8] float32) -- for
    every face the LOWEST index of the nearest point, that squared distance and the face's closest point to it as a tap row.  A
    face that takes no part: -1, +inf and zero taps.  ``slices`` cuts the points over more workgroups and never changes a bit."""
    return _point_mesh("reni_faces_nearest_points", points, verts, faces, slices)


KNN_MAX_K = 32  # the register budget of a lane's list (reni_tu_knn.hip)


def _knn_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be an int in [1, {KNN_MAX_K}], got {k!r}")
    return k


def knn_points(x: torch.Tensor, y: torch.Tensor, k: int, slices: int = 0):
    """reni_knn_points: (dist2 [N, k] float32, idx [N, k] int64) -- for every x_i the k smallest pairs (d, j) over the y_j in
    ascending lexicographic order (ties in d by ascending j), d = fmaf(dz, dz, fmaf(dy, dy, dx dx)) as ``nearest_points``
    computes it: column 0 has its bits.  A target at a NaN or +inf distance is never listed; slots left unfilled hold +inf and
    -1.  1 <= k <= 32: the lists live in registers.  Brute force through LDS tiles, never an N x M matrix; ``slices`` cuts the
    target range over more workgroups (0: the library's choice) and never changes a bit of the result."""
    k = _knn_k(k)
    slices = int(slices)
    if slices < 0:
        raise ValueError("slices must be >= 0")
    x, y = _cloud_pair(x, y)
    N, M, dev = x.shape[0], y.shape[0], x.device
    lib = _lib.load()
    dist2 = torch.empty(N, k, dtype=torch.float32, device=dev)
    idx = torch.empty(N, k, dtype=torch.int64, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_knn_points_workspace_bytes(N, M, k)), dev)
    _call(lib.reni_knn_points, dev, N, M, k, x.data_ptr(), y.data_ptr(), slices, dist2.data_ptr(), idx.data_ptr(), wp, wn)
    return dist2, idx


def cloud_normals(y: torch.Tensor, idx: torch.Tensor, viewpoint=None):
    """reni_cloud_normals: (normals [N, 3], eigenvalues [N, 3] ascending, >= 0) from the neighbour lists idx [N, k] int64 into
    y [M, 3] (``knn_points``' format; a slot of -1 is skipped): the unit eigenvector of the smallest eigenvalue of each
    neighbourhood's covariance, by cyclic Jacobi in fp32 (include/reni_hip.h has the order of operations).  With ``viewpoint``
    (three numbers or a tensor [3]) row i is point y_i and n . (viewpoint - y_i) >= 0; without, the component of largest
    magnitude is positive.  Fewer than 3 usable neighbours: exactly 0.  Never a NaN."""
    _cloud(y, "y")
    if (not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int64 or idx.shape[0] < 1
            or not 1 <= idx.shape[1] <= KNN_MAX_K):
        raise ValueError(f"idx must be an int64 tensor [N, k] with N >= 1 and 1 <= k <= {KNN_MAX_K}")
    N, K, M = idx.shape[0], idx.shape[1], y.shape[0]
    if viewpoint is not None:
        if not isinstance(viewpoint, torch.Tensor):
            viewpoint = torch.tensor([float(v) for v in viewpoint], dtype=torch.float32, device=y.device)
        if viewpoint.numel() != 3:
            raise ValueError("viewpoint must hold three values")
        if N > M:
            raise ValueError("with a viewpoint row i is point y_i: idx must not have more rows than y")
    _require_cuda(y, idx, viewpoint)
    y, idx = _f32c(y.detach()), idx.contiguous()
    dev = y.device
    if idx.device != dev or (viewpoint is not None and viewpoint.device != dev):
        raise ValueError(f"idx and viewpoint must be on {dev}")
    if viewpoint is not None:
        viewpoint = _f32c(viewpoint.detach()).reshape(3)
    normals = torch.empty(N, 3, dtype=torch.float32, device=dev)
    eig = torch.empty(N, 3, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_cloud_normals, dev, N, M, K, y.data_ptr(), idx.data_ptr(), _ptr(viewpoint), normals.data_ptr(),
          eig.data_ptr())
    return normals, eig


def _morton_order(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """A permutation of the faces that keeps neighbours together: the stable argsort of the 30-bit Morton codes of the
    centroids (10 bits per axis over the mesh's bounding box).  Faces with an index outside [0, V) sort last."""
    V = verts.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(dim=1)
    c = verts[faces.clamp(0, V - 1)].mean(dim=1)
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    g = ((c - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).clamp(0, 1023).to(torch.int64)

    def spread(x):  # 10 bits -> every third bit
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    code = spread(g[:, 0]) | (spread(g[:, 1]) << 1) | (spread(g[:, 2]) << 2)
    code = torch.where(ok, code, torch.full_like(code, 1 << 30))
    return torch.sort(code, stable=True).indices.contiguous()


def mesh_visibility_prepare(verts: torch.Tensor, faces: torch.Tensor, order=None) -> torch.Tensor:
    """reni_mesh_visibility_prepare: the acceleration record of one mesh for ``mesh_visibility`` -- a uint8 tensor (opaque;
    the faces in Morton order of their centroids unless ``order`` [F] int64 is given, and one inflated bounding box per
    cluster of 64).  One-off per mesh."""
    for name, t in (("verts", verts), ("faces", faces)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"{name} must be a tensor [N, 3] with N >= 1")
    verts, faces = _mesh_inputs(verts, faces)
    V, F = verts.shape[0], faces.shape[0]
    if order is None:
        order = _morton_order(verts, faces)
    else:
        if not isinstance(order, torch.Tensor) or tuple(order.shape) != (F,):
            raise ValueError(f"order must be an int64 tensor [{F}]")
        _require_cuda(order)
        order = order.to(torch.int64).contiguous()
    lib = _lib.load()
    nbytes = int(lib.reni_mesh_visibility_accel_bytes(F))
    if nbytes == 0:
        raise ValueError(f"too many faces ({F})")
    accel = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    _call(lib.reni_mesh_visibility_prepare, verts.device, V, F, verts.data_ptr(), faces.data_ptr(), order.data_ptr(),
          accel.data_ptr(), nbytes)
    return accel


def mesh_visibility(positions, pix_to_face, dirs, accel, t_min: float, no_cull: bool = False) -> torch.Tensor:
    """reni_mesh_visibility: which directions each pixel sees past the mesh.  positions [NP,3] and pix_to_face (NP int64
    entries, any shape: the rasteriser's) are the G-buffer, dirs [J,3] (shared) or [B,J,3], accel the record of
    ``mesh_visibility_prepare``, t_min >= 0 the distance below which a hit is the surface itself.  Returns the int32 mask
    [NB, NP, ceil(J/32)] (NB = 1 for shared directions, else B): bit j & 31 of word j >> 5 is 1 where direction j is
    unoccluded; background pixels and the bits at j >= J are 0.  ``no_cull`` runs the brute-force path (the same bits)."""
    _dirs_dims(dirs, "dirs")
    if not isinstance(positions, torch.Tensor) or positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] < 1:
        raise ValueError("positions must be [NP, 3]")
    NP = positions.shape[0]
    if not isinstance(pix_to_face, torch.Tensor) or pix_to_face.dtype != torch.int64 or pix_to_face.numel() != NP:
        raise ValueError(f"pix_to_face must hold {NP} int64 entries")
    if not isinstance(accel, torch.Tensor) or accel.dtype != torch.uint8 or accel.dim() != 1:
        raise ValueError("accel must be the uint8 tensor of mesh_visibility_prepare")
    t_min = float(t_min)
    if not (t_min >= 0.0 and t_min < float("inf")):
        raise ValueError("t_min must be finite and >= 0")
    _require_cuda(positions, pix_to_face, dirs, accel)
    positions, dirs = _f32c(positions), _f32c(dirs)
    p2f = pix_to_face.reshape(-1).contiguous()
    if dirs.dim() == 2:
        B, J, stride, NB = 1, dirs.shape[0], 0, 1
    else:
        B, J = dirs.shape[0], dirs.shape[1]
        stride, NB = 3 * J, B
    vis = torch.empty(NB, NP, (J + 31) // 32, dtype=torch.int32, device=positions.device)
    _call(_lib.load().reni_mesh_visibility, positions.device, B, NP, J, positions.data_ptr(), p2f.data_ptr(), dirs.data_ptr(),
          stride, accel.data_ptr(), t_min, _lib.VIS_NO_CULL if no_cull else 0, vis.data_ptr())
    return vis


def _sg_check(params, theta_c, phi_c, H, W):
    _require_cuda(params, theta_c, phi_c)
    if params.dim() != 3 or params.shape[2] != 6:
        raise ValueError(f"params must be [N, K, 6], got {tuple(params.shape)}")
    N, K = params.shape[0], params.shape[1]
    if tuple(theta_c.shape) != (K,) or tuple(phi_c.shape) != (K,):
        raise ValueError("theta_c and phi_c must be [K]")
    return _f32c(params), _f32c(theta_c), _f32c(phi_c), N, K, int(H), int(W)


def sg_render(params, theta_c, phi_c, theta_range: float, phi_range: float, H: int, W: int) -> torch.Tensor:
    """reni_sg_render: SGEnvOptim.renderSG of raw parameters [N, K, 6] -> rec [N, 3, H, W]."""
    params, theta_c, phi_c, N, K, H, W = _sg_check(params, theta_c, phi_c, H, W)
    dev = params.device
    rec = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_sg_render, dev, N, K, H, W, params.data_ptr(), theta_c.data_ptr(), phi_c.data_ptr(), float(theta_range),
          float(phi_range), rec.data_ptr())
    return rec


def sg_loss_grad(params, theta_c, phi_c, theta_range: float, phi_range: float, log_target, weight):
    """reni_sg_loss_grad: (loss_total [], loss_per_map [N], dparams [N, K, 6]) of WeightedMSE(log(rec + 1), log_target,
    weight) at raw parameters [N, K, 6].  log_target [N, 3, H, W]; weight any tensor that broadcasts to [N, 3, H, W] (it is
    read through its expanded strides, nothing is materialised)."""
    _require_cuda(log_target, weight)
    log_target = _f32c(log_target)
    if log_target.dim() != 4 or log_target.shape[1] != 3:
        raise ValueError(f"log_target must be [N, 3, H, W], got {tuple(log_target.shape)}")
    N, _, H, W = log_target.shape
    params, theta_c, phi_c, Np, K, H, W = _sg_check(params, theta_c, phi_c, H, W)
    if Np != N:
        raise ValueError("params and log_target disagree on N")
    weight = _f32(weight).expand(N, 3, H, W)
    dev = params.device
    loss_map = torch.empty(N, dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty(N, K, 6, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, wp, wn = _ws256(int(lib.reni_sg_workspace_bytes(N, K, H, W)), dev)
    _call(lib.reni_sg_loss_grad, dev, N, K, H, W, params.data_ptr(), theta_c.data_ptr(), phi_c.data_ptr(), float(theta_range),
          float(phi_range), log_target.data_ptr(), weight.data_ptr(), *[int(x) for x in weight.stride()], loss_map.data_ptr(),
          total.data_ptr(), grad.data_ptr(), wp, wn)
    return total, loss_map, grad


def _sh_call(project: bool, src, row_table, col_table, H: int, W: int, lmax: int):
    _require_cuda(src, row_table, col_table)
    src = _f32c(src)
    T = (lmax + 1) ** 2
    N = src.shape[0]
    dev = src.device
    out = torch.empty((N, T, 3) if project else (N, H, W, 3), dtype=torch.float32, device=dev)
    fn = _lib.load().reni_sh_project if project else _lib.load().reni_sh_reconstruct
    _call(fn, dev, N, H, W, lmax, src.data_ptr(), _f32c(row_table).data_ptr(), _f32c(col_table).data_ptr(), out.data_ptr())
    return out


def sh_project(imgs, row_table, col_table, lmax: int) -> torch.Tensor:
    """reni_sh_project: imgs [N, H, W, 3] -> coeffs [N, T, 3] against the separable basis tables (row_table [H, T] with
    the solid angle folded in, col_table [W, T]; reni_hip.h)."""
    if imgs.dim() != 4 or imgs.shape[3] != 3:
        raise ValueError(f"imgs must be [N, H, W, 3], got {tuple(imgs.shape)}")
    return _sh_call(True, imgs, row_table, col_table, imgs.shape[1], imgs.shape[2], int(lmax))


def sh_reconstruct(coeffs, row_table, col_table, H: int, W: int, lmax: int) -> torch.Tensor:
    """reni_sh_reconstruct: coeffs [N, T, 3] -> maps [N, H, W, 3] (row_table without the solid angle)."""
    if coeffs.dim() != 3 or coeffs.shape[1] != (int(lmax) + 1) ** 2 or coeffs.shape[2] != 3:
        raise ValueError(f"coeffs must be [N, (lmax + 1)^2, 3], got {tuple(coeffs.shape)}")
    return _sh_call(False, coeffs, row_table, col_table, int(H), int(W), int(lmax))


def _sphere_operands(in_dirs, in_weight, out_dirs):
    """in_dirs [Q, 3], in_weight [Q] and out_dirs [P, 3] of a convolution over the sphere as contiguous float32, checked, then
    P and Q."""
    in_dirs, in_weight, out_dirs = _f32c(in_dirs), _f32c(in_weight), _f32c(out_dirs)
    if in_dirs.dim() != 2 or in_dirs.shape[1] != 3 or out_dirs.dim() != 2 or out_dirs.shape[1] != 3:
        raise ValueError("in_dirs and out_dirs must be [Q, 3] and [P, 3]")
    Q, P = in_dirs.shape[0], out_dirs.shape[0]
    if tuple(in_weight.shape) != (Q,):
        raise ValueError(f"in_weight must be [Q] = [{Q}], got {tuple(in_weight.shape)}")
    return in_dirs, in_weight, out_dirs, P, Q


def _convolve_args(src, in_dirs, in_weight, out_dirs):
    """The operands the convolutions over the sphere share: (src float32, in_dirs, in_weight, out_dirs contiguous float32,
    N, P, Q, src's element strides (map, texel, channel)) for src [N, Q, 3] or channel-planar [N, 3, Q]."""
    in_dirs, in_weight, out_dirs, P, Q = _sphere_operands(in_dirs, in_weight, out_dirs)
    src = _f32(src)
    if src.dim() != 3:
        raise ValueError(f"src must be [N, Q, 3] or [N, 3, Q], got {tuple(src.shape)}")
    N = src.shape[0]
    if src.shape[1] == Q and src.shape[2] == 3:
        sn, si, sc = src.stride()
    elif src.shape[1] == 3 and src.shape[2] == Q:
        sn, sc, si = src.stride()
    else:
        raise ValueError(f"src must be [N, Q, 3] or [N, 3, Q] with Q = {Q}, got {tuple(src.shape)}")
    return src, in_dirs, in_weight, out_dirs, N, P, Q, sn, si, sc


def diffuse_convolve(src, in_dirs, in_weight, out_dirs, scale: float) -> torch.Tensor:
    """reni_diffuse_convolve: out [N, P, 3] = scale sum_i max(0, out_dirs[o] . in_dirs[i]) in_weight[i] src[n, i, c].
    src is [N, Q, 3] or channel-planar [N, 3, Q], read through its own strides (any float32 view of those shapes; at
    Q = 3 the two shapes coincide and src is taken as [N, Q, 3]);
    in_dirs [Q, 3], in_weight [Q], out_dirs [P, 3] are shared by the N maps."""
    _require_cuda(src, in_dirs, in_weight, out_dirs)
    src, in_dirs, in_weight, out_dirs, N, P, Q, sn, si, sc = _convolve_args(src, in_dirs, in_weight, out_dirs)
    dev = src.device
    out = torch.empty(N, P, 3, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, wp, wn = _ws256(int(lib.reni_diffuse_workspace_bytes(N, P, Q)), dev)
    _call(lib.reni_diffuse_convolve, dev, N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), in_weight.data_ptr(), src.data_ptr(),
          sn, si, sc, float(scale), out.data_ptr(), wp, wn)
    return out


def _per_map_operand(t, N):
    """(P, the map stride in elements) of an operand [P, 3] that N maps share (stride 0) or [N, P, 3] with one set per map;
    None when t is neither.  What it is called, and whether P = 0 is an error, is the caller's."""
    if t.dim() == 2 and t.shape[1] == 3:
        return t.shape[0], 0
    if t.dim() == 3 and t.shape[0] == N and t.shape[2] == 3:
        return t.shape[1], 3 * t.shape[1]
    return None


def sh_irradiance_l2(coeffs, normals) -> torch.Tensor:
    """reni_sh_irradiance_l2: shRenderL2 of coeffs [N, 9, 3] at normals [P, 3] (shared) or [N, P, 3] (per map) -> [N, P, 3]."""
    _require_cuda(coeffs, normals)
    coeffs, normals = _f32c(coeffs), _f32c(normals)
    if coeffs.dim() != 3 or coeffs.shape[1:] != (9, 3):
        raise ValueError(f"coeffs must be [N, 9, 3], got {tuple(coeffs.shape)}")
    N = coeffs.shape[0]
    shape = _per_map_operand(normals, N)
    if shape is None:
        raise ValueError(f"normals must be [P, 3] or [N, P, 3], got {tuple(normals.shape)}")
    P, stride = shape
    dev = coeffs.device
    out = torch.empty(N, P, 3, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_sh_irradiance_l2, dev, N, P, coeffs.data_ptr(), normals.data_ptr(), stride, out.data_ptr())
    return out


def _lobe_args(kinds, params):
    """(Lv, kinds as int32[Lv], params as float[Lv]) of a call's lobes, checked"""
    kinds, params = list(kinds), [float(p) for p in params]
    Lv = len(kinds)
    if not 1 <= Lv <= 16 or len(params) != Lv:
        raise ValueError(f"need 1..16 lobes and one parameter each, got {Lv} kinds and {len(params)} parameters")
    for k in kinds:
        if k not in _lib.LOBE_KIND:
            raise ValueError(f"lobe kind must be one of {tuple(_lib.LOBE_KIND)}, got {k!r}")
    return Lv, (ctypes.c_int32 * Lv)(*[_lib.LOBE_KIND[k] for k in kinds]), (ctypes.c_float * Lv)(*params)


def lobe_convolve(src, in_dirs, in_weight, out_dirs, kinds, params, normalise: bool = True, scale: float = 1.0) -> torch.Tensor:
    """reni_lobe_convolve: out [N, Lv, P, 3] = the maps convolved with Lv zonal lobes f_l(out_dirs[o] . in_dirs[i]) weighted
    by in_weight[i]; divided by sum_i f_l in_weight[i] when normalise (0 where that sum is not positive), else times scale.
    kinds: Lv names of _lib.LOBE_KIND ("phong": tc^n, "blinn": m^(s/2), "ggx": tc a^2 / (m (a^2 - 1) + 1)^2 with
    tc = clamp(t, 0, 1), m = clamp((1 + t) / 2, 0, 1)); params: their one parameter each (n, s, a).  src, in_dirs, in_weight,
    out_dirs as in ``diffuse_convolve``."""
    _require_cuda(src, in_dirs, in_weight, out_dirs)
    Lv, ck, cp = _lobe_args(kinds, params)
    src, in_dirs, in_weight, out_dirs, N, P, Q, sn, si, sc = _convolve_args(src, in_dirs, in_weight, out_dirs)
    dev = src.device
    out = torch.empty(N, Lv, P, 3, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, wp, wn = _ws256(int(lib.reni_lobe_workspace_bytes(N, P, Q, Lv)), dev)
    _call(lib.reni_lobe_convolve, dev, N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), in_weight.data_ptr(), src.data_ptr(),
          sn, si, sc, Lv, ck, cp, 1 if normalise else 0, float(scale), out.data_ptr(), wp, wn)
    return out


def _level_tensor(level):
    """level where it is a tensor of per-direction levels; None for None, a number or a 0-d tensor (one constant level)"""
    return level if isinstance(level, torch.Tensor) and level.dim() > 0 else None


def _lookup_dirs_level(N, dirs, level, dev):
    """The directions and the level of a lookup of N maps on dev, checked: (dirs float32 contiguous, P, the directions' map
    stride, the level tensor or None, its pointer or None, its map stride, the constant level)."""
    dirs = _f32c(dirs)
    shape = _per_map_operand(dirs, N)
    if shape is None:
        raise ValueError(f"dirs must be [P, 3] or [{N}, P, 3], got {tuple(dirs.shape)}")
    P, dn = shape
    if P < 1:
        raise ValueError("no directions")
    lp, ln, lc = None, 0, 0.0
    if _level_tensor(level) is not None:
        level = _f32c(level)
        if tuple(level.shape) == (P,):
            ln = 0
        elif tuple(level.shape) == (N, P):
            ln = P
        else:
            raise ValueError(f"level must be a number, [P] or [N, P], got {tuple(level.shape)}")
        if level.device != dev:
            raise ValueError(f"level is on {level.device}, the maps on {dev}")
        lp = level.data_ptr()
    elif level is not None:
        lc = float(level)
    if dirs.device != dev:
        raise ValueError(f"dirs are on {dirs.device}, the maps on {dev}")
    return dirs, P, dn, level if lp is not None else None, lp, ln, lc


def _lookup_maps(maps):
    """The maps of a lookup, [N, H, W, 3] or a chain [N, Lv, H, W, 3] with any strides, as a float32 view [N, Lv, H, W, 3],
    checked, then N, Lv, H, W."""
    maps = _f32(maps)
    if maps.dim() == 4:
        maps = maps.unsqueeze(1)
    if maps.dim() != 5 or maps.shape[4] != 3:
        raise ValueError(f"maps must be [N, H, W, 3] or [N, Lv, H, W, 3], got {tuple(maps.shape)}")
    N, Lv, H, W, _ = maps.shape
    if min(N, Lv, H, W) < 1 or W % 2:
        raise ValueError(f"expected non-empty maps of even width, got {tuple(maps.shape)}")
    return maps, N, Lv, H, W


def envmap_lookup(maps, dirs, level=None) -> torch.Tensor:
    """reni_envmap_lookup: the bilinear sample, on the sphere, of equirectangular maps [N, H, W, 3] or chains of maps
    [N, Lv, H, W, 3] (any strides, read in place) at directions dirs [P, 3] (shared) or [N, P, 3] (per map), which need not
    have unit length -> [N, P, 3].  level: None (level 0), a number, or a float tensor [P] / [N, P]; it is clamped to
    [0, Lv - 1] and the result mixes floor(level) and the next level linearly."""
    _require_cuda(maps, dirs, _level_tensor(level))
    maps, N, Lv, H, W = _lookup_maps(maps)
    dev = maps.device
    dirs, P, dn, level, lp, ln, lc = _lookup_dirs_level(N, dirs, level, dev)
    out = torch.empty(N, P, 3, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_envmap_lookup, dev, N, Lv, H, W, P, maps.data_ptr(), _strides(maps), dirs.data_ptr(), dn, lp, ln, lc,
          out.data_ptr())
    return out


def lobe_denominators(in_dirs, in_weight, out_dirs, kinds, params) -> torch.Tensor:
    """reni_lobe_denominators: den [Lv, P] = sum_i f_l(out_dirs[o] . in_dirs[i]) in_weight[i], the denominators
    ``lobe_convolve`` divides by when it normalises, bit for bit (the forward's own launch without maps)."""
    _require_cuda(in_dirs, in_weight, out_dirs)
    Lv, ck, cp = _lobe_args(kinds, params)
    in_dirs, in_weight, out_dirs, P, Q = _sphere_operands(in_dirs, in_weight, out_dirs)
    dev = in_dirs.device
    den = torch.empty(Lv, P, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, wp, wn = _ws256(int(lib.reni_lobe_denominators_workspace_bytes(P, Q, Lv)), dev)
    _call(lib.reni_lobe_denominators, dev, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), in_weight.data_ptr(), Lv, ck, cp,
          den.data_ptr(), wp, wn)
    return den


def lobe_convolve_backward(grad_out, in_dirs, in_weight, out_dirs, kinds, params, normalise: bool = True, scale: float = 1.0,
                           den=None, planar: bool = False) -> torch.Tensor:
    """reni_lobe_convolve_backward: d loss / d src of ``lobe_convolve`` for the upstream grad_out [N, Lv, P, 3] -- the
    transposed convolution, as [N, Q, 3] or, with planar, [N, 3, Q] (the same bits).  den: the [Lv, P] of
    ``lobe_denominators`` for these operands (computed here when None and normalising; not needed otherwise)."""
    _require_cuda(grad_out, in_dirs, in_weight, out_dirs, den)
    Lv, ck, cp = _lobe_args(kinds, params)
    in_dirs, in_weight, out_dirs, P, Q = _sphere_operands(in_dirs, in_weight, out_dirs)
    grad_out = _f32c(grad_out)
    if grad_out.dim() != 4 or tuple(grad_out.shape[1:]) != (Lv, P, 3) or grad_out.shape[0] < 1:
        raise ValueError(f"grad_out must be [N, {Lv}, {P}, 3], got {tuple(grad_out.shape)}")
    N = grad_out.shape[0]
    dev = grad_out.device
    dp = None
    if normalise:
        den = lobe_denominators(in_dirs, in_weight, out_dirs, kinds, params) if den is None else _f32c(den)
        if tuple(den.shape) != (Lv, P) or den.device != dev:
            raise ValueError(f"den must be [{Lv}, {P}] on {dev}, got {tuple(den.shape)} on {den.device}")
        dp = den.data_ptr()
    out = torch.empty((N, 3, Q) if planar else (N, Q, 3), dtype=torch.float32, device=dev)
    sn, si, sc = (3 * Q, 1, Q) if planar else (3 * Q, 3, 1)
    lib = _lib.load()
    ws, wp, wn = _ws256(int(lib.reni_lobe_backward_workspace_bytes(N, P, Q, Lv)), dev)
    _call(lib.reni_lobe_convolve_backward, dev, N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), in_weight.data_ptr(),
          grad_out.data_ptr(), Lv, ck, cp, 1 if normalise else 0, float(scale), dp, out.data_ptr(), sn, si, sc, wp, wn)
    return out


def envmap_lookup_table(N: int, Lv: int, H: int, W: int, dirs, level=None):
    """What ``envmap_lookup_backward`` gathers through, for a lookup of N maps [Lv, H, W, 3] at dirs / level (as in
    ``envmap_lookup``): (tap weights [T, P, 8], tap order [T, 8 P] int64, offsets [T, Lv H W + 1] int64) with T = 1 when
    directions and level are shared by the maps, else N.  reni_envmap_lookup_taps writes the 8 texels and weights of every
    direction; a stable sort of the texel indices and a searchsorted bin them per texel (as ``_vertex_face_csr`` does the
    faces of a vertex).  It depends on the directions and the level only: a caller whose geometry is fixed may keep it."""
    N, Lv, H, W = int(N), int(Lv), int(H), int(W)
    if min(N, Lv, H, W) < 1 or W % 2 or Lv * H * W >= 2 ** 31:
        raise ValueError(f"expected N, Lv, H, W >= 1, an even width and Lv H W < 2^31, got {(N, Lv, H, W)}")
    _require_cuda(dirs, _level_tensor(level))
    dev = dirs.device
    dirs, P, dn, level, lp, ln, lc = _lookup_dirs_level(N, dirs, level, dev)
    T = 1 if dn == 0 and ln == 0 else N
    idx = torch.empty(T, 8 * P, dtype=torch.int32, device=dev)
    wgt = torch.empty(T, P, 8, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_envmap_lookup_taps, dev, T, Lv, H, W, P, dirs.data_ptr(), dn, lp, ln, lc, idx.data_ptr(),
          wgt.data_ptr())
    keys, order = torch.sort(idx, dim=1, stable=True)
    bounds = torch.arange(Lv * H * W + 1, device=dev, dtype=torch.int32).expand(T, -1).contiguous()
    offsets = torch.searchsorted(keys, bounds)
    return wgt, order.contiguous(), offsets.contiguous()


def envmap_lookup_backward(grad_out, Lv: int, H: int, W: int, dirs=None, level=None, table=None) -> torch.Tensor:
    """reni_envmap_lookup_backward: d loss / d maps [N, Lv, H, W, 3] (contiguous; 0 where nobody sampled) of
    ``envmap_lookup`` for the upstream grad_out [N, P, 3] -- the scatter of the lookup's 8 weights per direction, done as a
    deterministic gather per texel.  table: ``envmap_lookup_table(N, Lv, H, W, dirs, level)`` (built here when None)."""
    _require_cuda(grad_out, dirs)
    grad_out = _f32c(grad_out)
    if grad_out.dim() != 3 or grad_out.shape[2] != 3 or grad_out.shape[0] < 1 or grad_out.shape[1] < 1:
        raise ValueError(f"grad_out must be [N, P, 3], got {tuple(grad_out.shape)}")
    N, P, _ = grad_out.shape
    Lv, H, W = int(Lv), int(H), int(W)
    if table is None:
        if dirs is None:
            raise ValueError("need the lookup's dirs (and level), or its table")
        table = envmap_lookup_table(N, Lv, H, W, dirs, level)
    wgt, order, offsets = table
    _require_cuda(wgt, order, offsets)
    T = wgt.shape[0]
    E = Lv * H * W
    if (T not in (1, N) or tuple(wgt.shape) != (T, P, 8) or tuple(order.shape) != (T, 8 * P) or tuple(offsets.shape) != (T, E + 1)
            or wgt.dtype != torch.float32 or order.dtype != torch.int64 or offsets.dtype != torch.int64):
        raise ValueError(f"the table is not one of {N} maps [{Lv}, {H}, {W}, 3] looked up at {P} directions")
    dev = grad_out.device
    if wgt.device != dev or order.device != dev or offsets.device != dev:
        raise ValueError(f"the table is not on {dev}")
    out = torch.empty(N, Lv, H, W, 3, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_envmap_lookup_backward, dev, N, Lv, H, W, P, grad_out.data_ptr(), T, wgt.contiguous().data_ptr(),
          order.contiguous().data_ptr(), offsets.contiguous().data_ptr(), out.data_ptr())
    return out


def envmap_lookup_dquery(maps, dirs, level, grad_out, need_dirs: bool = True, need_level: bool = False):
    """reni_envmap_lookup_dquery: (d loss / d dirs, d loss / d level) of ``envmap_lookup(maps, dirs, level)`` for the upstream
    grad_out [N, P, 3]; a half that is not needed is None and is not computed.  d dirs has the shape of dirs ([P, 3], the sum
    over the maps, or [N, P, 3]), d level the shape of the level tensor ([P] or [N, P]); need_level needs a level tensor.  The
    chain rule runs through the lookup's own coordinate chain: exact zeros at a pole direction, for the zero vector and for a
    level outside [0, Lv - 1]; at a knot the level's slope is the right-sided one, at Lv - 1 the left-sided one."""
    if not (need_dirs or need_level):
        raise ValueError("neither d dirs nor d level is asked for")
    _require_cuda(maps, dirs, grad_out, _level_tensor(level))
    maps, N, Lv, H, W = _lookup_maps(maps)
    dev = maps.device
    dirs, P, dn, level, lp, ln, lc = _lookup_dirs_level(N, dirs, level, dev)
    if need_level and lp is None:
        raise ValueError("d level needs the level as a tensor [P] or [N, P]")
    grad_out = _f32c(grad_out)
    if tuple(grad_out.shape) != (N, P, 3) or grad_out.device != dev:
        raise ValueError(f"grad_out must be [{N}, {P}, 3] on {dev}, got {tuple(grad_out.shape)} on {grad_out.device}")
    d_dirs = torch.empty_like(dirs) if need_dirs else None
    d_level = torch.empty_like(level) if need_level else None
    _call(_lib.load().reni_envmap_lookup_dquery, dev, N, Lv, H, W, P, maps.data_ptr(), _strides(maps), dirs.data_ptr(), dn, lp, ln, lc,
          grad_out.data_ptr(), _ptr(d_dirs), _ptr(d_level))
    return d_dirs, d_level


def ggx_dfg(size_v: int = 32, size_r: int = 32, roughness_min: float = 0.1, nodes_u: int = 128, nodes_phi: int = 128,
            device="cuda") -> torch.Tensor:
    """reni_ggx_dfg: the directional-albedo table [2, size_r, size_v] of the microfacet material -- A0 = int k d omega and
    A1 = int k f d omega (k, f of ``envmap_shade_ggx``) at N.V = i / (size_v - 1) and roughness = roughness_min +
    j (1 - roughness_min) / (size_r - 1) -- by the midpoint rule on nodes_u x nodes_phi nodes of GGX's inverse-CDF
    parametrisation of the half vector."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.RENILibraryError("RENI HIP ops need tensors on a GPU device (got a CPU device); there is no CPU fallback")
    size_v, size_r, nodes_u, nodes_phi = int(size_v), int(size_r), int(nodes_u), int(nodes_phi)
    if min(size_v, size_r) < 2 or min(nodes_u, nodes_phi) < 1:
        raise ValueError(f"need table sizes >= 2 and node counts >= 1, got {(size_v, size_r, nodes_u, nodes_phi)}")
    out = torch.empty(2, size_r, size_v, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_ggx_dfg, dev, size_v, size_r, float(roughness_min), nodes_u, nodes_phi, out.data_ptr())
    return out


def texture_levels(H0: int, W0: int, levels=None):
    """(L, E, sizes): the number of levels of an H0 x W0 texture's pyramid (``levels=None``: the full one, 1 + log2(max(H0, W0))
    for powers of two and 1 otherwise), the element count E = sum H_l W_l and the [(H_l, W_l)] list.  Raises on a pyramid
    include/reni_hip.h does not define (L > 1 on a size that is no power of two, L beyond the full pyramid, E >= 2^31)."""
    H0, W0 = int(H0), int(W0)
    if H0 < 1 or W0 < 1:
        raise ValueError(f"a texture needs H0, W0 >= 1, got {(H0, W0)}")
    pow2 = H0 & (H0 - 1) == 0 and W0 & (W0 - 1) == 0
    full = max(H0, W0).bit_length() if pow2 else 1
    L = full if levels is None else int(levels)
    if L < 1 or L > full:
        raise ValueError(f"levels must be 1..{full} for a {H0} x {W0} texture (more than one level needs powers of two), got {L}")
    sizes = [(max(1, H0 >> l), max(1, W0 >> l)) for l in range(L)]
    E = sum(h * w for h, w in sizes)
    if E >= 2 ** 31:
        raise ValueError(f"the pyramid has {E} elements, the limit is 2^31 - 1")
    return L, E, sizes


def mesh_pixel_uv(verts, faces, verts_uvs, faces_uvs, R, T, image_size: int, pix_to_face, bary,
                  tan_half_fov: float = 0.5773502691896258):
    """reni_mesh_pixel_uv: (uv [P, 2], jac [P, 4], pix_valid [P] int64) of the P = S^2 pixels of a G-buffer
    (``rasterize_mesh``'s pix_to_face and bary, any shape with S^2 / 3 S^2 elements): the interpolated texture coordinate, its
    constant per-face derivative (du/dcol, dv/dcol, du/drow, dv/drow) per pixel step, and the pixel's face, -1 where the pixel
    is background, its face has no UVs (a faces_uvs entry outside [0, Tn)) or its uv is not finite (then uv = jac = 0)."""
    verts, faces = _mesh_inputs(verts, faces)
    _require_cuda(verts_uvs, faces_uvs, pix_to_face, bary)
    dev = verts.device
    verts_uvs = verts_uvs.to(torch.float32).contiguous()
    faces_uvs = faces_uvs.to(torch.int64).contiguous()
    if verts_uvs.dim() != 2 or verts_uvs.shape[1] != 2 or verts_uvs.shape[0] < 1:
        raise ValueError(f"verts_uvs must be [Tn, 2] with Tn >= 1, got {tuple(verts_uvs.shape)}")
    if tuple(faces_uvs.shape) != tuple(faces.shape):
        raise ValueError(f"faces_uvs must be [F, 3] like faces, got {tuple(faces_uvs.shape)}")
    S = _image_size(image_size)
    p2f = pix_to_face.to(torch.int64).contiguous()
    bary = bary.to(torch.float32).contiguous()
    if p2f.numel() != S * S or bary.numel() != 3 * S * S:
        raise ValueError(f"pix_to_face and bary must hold {S * S} pixels (and 3 barycentrics each)")
    if any(t.device != dev for t in (verts_uvs, faces_uvs, p2f, bary)):
        raise ValueError("the mesh, its UVs and the G-buffer must be on the same device")
    Rh, Th = _camera_arrays(R, T)
    uv = torch.empty(S * S, 2, dtype=torch.float32, device=dev)
    jac = torch.empty(S * S, 4, dtype=torch.float32, device=dev)
    valid = torch.empty(S * S, dtype=torch.int64, device=dev)
    _call(_lib.load().reni_mesh_pixel_uv, dev, verts.shape[0], faces.shape[0], verts_uvs.shape[0], verts.data_ptr(), faces.data_ptr(),
          verts_uvs.data_ptr(), faces_uvs.data_ptr(), Rh, Th, float(tan_half_fov), S, p2f.data_ptr(), bary.data_ptr(), uv.data_ptr(),
          jac.data_ptr(), valid.data_ptr())
    return uv, jac, valid


def texture_taps(uv, size, levels=None, jac=None, pix_valid=None, wrap: str = "clamp", align_corners: bool = False,
                 lod_bias: float = 0.0):
    """reni_texture_taps: (tap_index int32 [P, 8], tap_weight [P, 8]) of a lookup at uv [P, 2] into a texture of
    ``size`` = (H0, W0) with ``levels`` levels (None: the full pyramid): the trilinear fetch's 8 element indices into the
    [E] pyramid and their weights.  jac [P, 4] (``mesh_pixel_uv``'s) chooses the level per pixel; without it every pixel
    uses clamp(lod_bias, 0, L - 1).  pix_valid [P] int64: < 0 marks a pixel that fetches exactly 0.  uv, jac and pix_valid
    are constants (one that requires grad raises)."""
    H0, W0 = (int(x) for x in size)
    L, _, _ = texture_levels(H0, W0, levels)
    if wrap not in _lib.TEX_WRAP:
        raise ValueError(f'wrap must be "clamp" or "repeat", got {wrap!r}')
    if align_corners and (L > 1 or wrap != "clamp"):
        raise ValueError('align_corners=True needs levels=1 and wrap="clamp"')
    lod_bias = float(lod_bias)
    if lod_bias != lod_bias or lod_bias in (float("inf"), float("-inf")):
        raise ValueError("lod_bias must be finite")
    if not isinstance(uv, torch.Tensor) or uv.dim() != 2 or uv.shape[1] != 2 or uv.shape[0] < 1:
        raise ValueError(f"uv must be [P, 2] with P >= 1, got {tuple(uv.shape) if isinstance(uv, torch.Tensor) else uv!r}")
    P = uv.shape[0]
    for name, t, shape in (("jac", jac, (P, 4)), ("pix_valid", pix_valid, (P,))):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be a tensor {list(shape)}")
    for name, t in (("uv", uv), ("jac", jac)):
        if t is not None and t.requires_grad:
            raise ValueError(f"{name} is a constant of the lookup and must not require grad (only the texture carries a gradient)")
    _require_cuda(uv, jac, pix_valid)
    dev = uv.device
    uv = _f32c(uv)
    jac = None if jac is None else _f32c(jac)
    pix_valid = None if pix_valid is None else pix_valid.to(torch.int64).contiguous()
    if any(t is not None and t.device != dev for t in (jac, pix_valid)):
        raise ValueError(f"jac and pix_valid must be on {dev}")
    idx = torch.empty(P, 8, dtype=torch.int32, device=dev)
    wgt = torch.empty(P, 8, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_texture_taps, dev, P, uv.data_ptr(), _ptr(jac), _ptr(pix_valid), L, H0, W0, lod_bias, _lib.TEX_WRAP[wrap],
          1 if align_corners else 0, idx.data_ptr(), wgt.data_ptr())
    return idx, wgt


def texture_table(tap_index, E: int, tap_weight=None):
    """What ``texture_fetch_backward`` gathers through: (tap_order [8 P] int64, offsets [E + 1] int64) from tap_index
    [P, 8] -- a stable sort of the element indices and a searchsorted that bins them per texel, as ``envmap_lookup_table``
    does.  With tap_weight [P, 8] the taps of weight 0 (the unused next level, every tap of an invalid pixel -- all of which
    name element 0) are sorted behind offsets[E], outside every texel's range: they add nothing, and a background of
    invalid pixels would otherwise make element 0's range the longest of the table.  It depends on the taps only: once per
    (scene, texture size)."""
    if not isinstance(tap_index, torch.Tensor) or tap_index.dim() != 2 or tap_index.shape[1] != 8 or tap_index.dtype != torch.int32:
        raise ValueError("tap_index must be an int32 tensor [P, 8]")
    E = int(E)
    if E < 1 or E >= 2 ** 31:
        raise ValueError(f"E must be in [1, 2^31), got {E}")
    keys = tap_index.reshape(-1).to(torch.int64)
    if tap_weight is not None:
        if not isinstance(tap_weight, torch.Tensor) or tuple(tap_weight.shape) != tuple(tap_index.shape) or tap_weight.device != tap_index.device:
            raise ValueError("tap_weight must be [P, 8] like tap_index, on its device")
        keys = torch.where(tap_weight.reshape(-1) == 0, torch.full_like(keys, E), keys)
    keys, order = torch.sort(keys, stable=True)
    bounds = torch.arange(E + 1, device=tap_index.device, dtype=keys.dtype)
    offsets = torch.searchsorted(keys, bounds)
    return order.contiguous(), offsets.to(torch.int64).contiguous()


def _texture_buffer(tex, L, H0, W0, what):
    if not isinstance(tex, torch.Tensor) or tex.dim() != 2 or tex.dtype != torch.float32 or not tex.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor [E, C]")
    L, E, _ = texture_levels(H0, W0, L)
    if tex.shape[0] != E or not 1 <= tex.shape[1] <= 8:
        raise ValueError(f"{what} must be [{E}, C] with 1 <= C <= 8 for {L} levels of {H0} x {W0}, got {tuple(tex.shape)}")
    _require_cuda(tex)
    return L


def texture_pyramid(tex, levels: int, H0: int, W0: int):
    """reni_texture_pyramid: fills levels 1 .. L - 1 of the pyramid buffer tex [E, C] from its level 0, IN PLACE (box rule);
    returns tex."""
    L = _texture_buffer(tex, levels, int(H0), int(W0), "tex")
    _call(_lib.load().reni_texture_pyramid, tex.device, L, int(H0), int(W0), tex.shape[1], tex.data_ptr())
    return tex


def texture_pyramid_backward(grad_tex, levels: int, H0: int, W0: int):
    """reni_texture_pyramid_backward: folds the gradients of levels L - 1 .. 1 of grad_tex [E, C] into level 0, IN PLACE;
    returns grad_tex, whose first H0 W0 rows are then d loss / d level 0."""
    L = _texture_buffer(grad_tex, levels, int(H0), int(W0), "grad_tex")
    _call(_lib.load().reni_texture_pyramid_backward, grad_tex.device, L, int(H0), int(W0), grad_tex.shape[1], grad_tex.data_ptr())
    return grad_tex


def _tap_pair(tap_index, tap_weight):
    if (not isinstance(tap_weight, torch.Tensor) or tap_weight.dim() != 2 or tap_weight.shape[1] != 8 or tap_weight.dtype != torch.float32):
        raise ValueError("tap_weight must be a float32 tensor [P, 8]")
    if tap_index is not None and (not isinstance(tap_index, torch.Tensor) or tap_index.dtype != torch.int32
                                  or tuple(tap_index.shape) != tuple(tap_weight.shape)):
        raise ValueError("tap_index must be an int32 tensor [P, 8] like tap_weight")
    return tap_weight.shape[0]


def texture_fetch(tex, tap_index, tap_weight) -> torch.Tensor:
    """reni_texture_fetch: out [P, C] = sum_k tap_weight[p, k] tex[tap_index[p, k]] for the pyramid buffer tex [E, C]."""
    P = _tap_pair(tap_index, tap_weight)
    if not isinstance(tex, torch.Tensor) or tex.dim() != 2 or not 1 <= tex.shape[1] <= 8 or tex.shape[0] < 1:
        raise ValueError("tex must be [E, C] with 1 <= C <= 8")
    _require_cuda(tex, tap_index, tap_weight)
    tex = _f32c(tex)
    dev = tex.device
    if tap_index.device != dev or tap_weight.device != dev:
        raise ValueError(f"the taps are not on {dev}")
    out = torch.empty(P, tex.shape[1], dtype=torch.float32, device=dev)
    _call(_lib.load().reni_texture_fetch, dev, P, tex.shape[0], tex.shape[1], tex.data_ptr(), tap_index.contiguous().data_ptr(),
          tap_weight.contiguous().data_ptr(), out.data_ptr())
    return out


def texture_fetch_backward(grad_out, tap_weight, table, E: int, plain: bool = False) -> torch.Tensor:
    """reni_texture_fetch_backward: grad_tex [E, C] (0 where nobody sampled) of ``texture_fetch`` for the upstream grad_out
    [P, C], gathered per texel through table = ``texture_table(tap_index, E, tap_weight)``.  Deterministic; a texel with a long range
    is summed by the lanes of a wave (plain=True: by one lane, kept for measurements)."""
    P = _tap_pair(None, tap_weight)
    if not isinstance(grad_out, torch.Tensor) or grad_out.dim() != 2 or grad_out.shape[0] != P or not 1 <= grad_out.shape[1] <= 8:
        raise ValueError(f"grad_out must be [{P}, C] with 1 <= C <= 8")
    order, offsets = table
    E = int(E)
    if (not isinstance(order, torch.Tensor) or not isinstance(offsets, torch.Tensor) or tuple(order.shape) != (8 * P,)
            or tuple(offsets.shape) != (E + 1,) or order.dtype != torch.int64 or offsets.dtype != torch.int64):
        raise ValueError(f"the table is not one of {P} pixels looked up in {E} elements")
    _require_cuda(grad_out, tap_weight, order, offsets)
    grad_out = _f32c(grad_out)
    dev = grad_out.device
    if tap_weight.device != dev or order.device != dev or offsets.device != dev:
        raise ValueError(f"the table is not on {dev}")
    out = torch.empty(E, grad_out.shape[1], dtype=torch.float32, device=dev)
    _call(_lib.load().reni_texture_fetch_backward, dev, P, E, grad_out.shape[1], grad_out.data_ptr(), tap_weight.contiguous().data_ptr(),
          order.contiguous().data_ptr(), offsets.contiguous().data_ptr(), 1 if plain else 0, out.data_ptr())
    return out


def unnormalise_srgb(img: torch.Tensor, minmax=None, srgb: bool = True, want_linear: bool = False):
    """reni_unnormalise_srgb: UnMinMaxNormlise(minmax) (skipped when minmax is None) -> sRGB view, on the device.
    img: [B,3,H,W] or [3,H,W], ANY strides (e.g. a model output viewed as ``out.view(B,H,W,3).permute(0,3,1,2)`` is read
    in place).  Returns the sRGB batch [B,3,H,W] (srgb=True), the linear HDR batch (srgb=False), or both (want_linear)."""
    _require_cuda(img)
    lib = _lib.load()
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"expected [B,3,H,W] or [3,H,W], got {tuple(img.shape)}")
    img = _f32(img)
    B, _, H, W = img.shape
    dev = img.device
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if srgb else None
    lin = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if (want_linear or not srgb) else None
    ws, wp, wn = _ws256(int(lib.reni_image_workspace_bytes(B, H, W)), dev) if srgb else (None, None, 0)
    m0, m1 = (float(minmax[0]), float(minmax[1])) if minmax is not None else (0.0, 1.0)
    _call(lib.reni_unnormalise_srgb, dev, B, H, W, img.data_ptr(), _strides(img), 0 if minmax is None else 1, m0, m1, 1 if srgb else 0,
          _ptr(out), _ptr(lin), wp, wn)
    if srgb and want_linear:
        return out, lin
    return out if srgb else lin


def minmax_normalise(img: torch.Tensor, minmax):
    """reni_minmax_normalise: MinMaxNormalise(minmax) of ONE image (any shape; the clip bounds are the image's own)."""
    _require_cuda(img)
    lib = _lib.load()
    x = _f32c(img)
    out = torch.empty_like(x)
    ws, wp, wn = _ws256(256, x.device)
    _call(lib.reni_minmax_normalise, x.device, x.numel(), x.data_ptr(), float(minmax[0]), float(minmax[1]), out.data_ptr(), wp, wn)
    return out


def minmax_normalise_batch(imgs: torch.Tensor, minmax, nan_to_num: bool = True):
    """reni_minmax_normalise_batch: MinMaxNormalise(minmax) of every image imgs[n] of a batch [N, ...] with its own clip
    bounds; imgs[n]'s result is bit-identical to ``minmax_normalise(imgs[n])``.  nan_to_num: torch.nan_to_num afterwards, as
    the HDR dataset applies it."""
    _require_cuda(imgs)
    if imgs.dim() < 2 or imgs.shape[0] < 1 or imgs[0].numel() < 1:
        raise ValueError(f"expected a batch [N, ...] of N >= 1 non-empty images, got {tuple(imgs.shape)}")
    lib = _lib.load()
    x = _f32c(imgs)
    out = torch.empty_like(x)
    N = x.shape[0]
    ws, wp, wn = _ws256(int(lib.reni_minmax_batch_workspace_bytes(N)), x.device)
    _call(lib.reni_minmax_normalise_batch, x.device, N, x[0].numel(), x.data_ptr(), float(minmax[0]), float(minmax[1]),
          1 if nan_to_num else 0, out.data_ptr(), wp, wn)
    return out


def _image_layout(img: torch.Tensor, layout: str):
    """(view [N, C, H, W] of img without copying, a function that gives a planar result the caller's rank).  layout: "chw"
    (planar [H,W], [C,H,W], [N,C,H,W]), "hwc" (channel-last [H,W,C], [N,H,W,C]) or "auto": 2 and 4 dimensions are planar, 3
    dimensions are channel-last when only the last axis is <= 4 long and planar when only the first is."""
    if layout not in ("auto", "chw", "hwc"):
        raise ValueError(f"layout must be 'auto', 'chw' or 'hwc', got {layout!r}")
    d = img.dim()
    if layout == "auto":
        if d == 3:
            first, last = img.shape[0] <= 4, img.shape[2] <= 4
            if first == last:
                raise ValueError(f"cannot tell whether {tuple(img.shape)} is [C,H,W] or [H,W,C]: pass layout='chw' or 'hwc'")
            layout = "hwc" if last else "chw"
        else:
            layout = "chw"
    if layout == "chw":
        if d == 2:
            return img[None, None], lambda o: o[0, 0]
        if d == 3:
            return img[None], lambda o: o[0]
        if d == 4:
            return img, lambda o: o
    else:
        if d == 3:
            return img.permute(2, 0, 1)[None], lambda o: o[0]
        if d == 4:
            return img.permute(0, 3, 1, 2), lambda o: o
    raise ValueError(f"expected an image or a batch of images, got {tuple(img.shape)} with layout {layout!r}")


def resample(src: torch.Tensor, size, mode: str = "bilinear", layout: str = "auto") -> torch.Tensor:
    """reni_resample: src resampled to size = (height, width) with mode "nearest" | "bilinear" | "bicubic" | "lanczos4"
    (conventions: reni_amd/resample.py).  src is read in place through its strides, planar ([H,W], [C,H,W], [N,C,H,W]) or
    channel-last ([H,W,C], [N,H,W,C] with layout="hwc"); the result is planar float32 of the same rank ([Hd,Wd], [C,Hd,Wd],
    [N,C,Hd,Wd]).  An image's result is bit-identical alone and inside a batch."""
    from .resample import TAPS, device_tables
    _require_cuda(src)
    if mode not in TAPS:
        raise ValueError(f"mode must be one of {tuple(TAPS)}, got {mode!r}")
    Hd, Wd = int(size[0]), int(size[1])
    if Hd < 1 or Wd < 1:
        raise ValueError(f"size must be (height >= 1, width >= 1), got {tuple(size)}")
    x, unview = _image_layout(_f32(src), layout)
    N, C, Hs, Ws = x.shape
    if min(N, C, Hs, Ws) < 1:
        raise ValueError(f"empty image {tuple(src.shape)}")
    dev = x.device
    ri, rw = device_tables(Hs, Hd, mode, dev)
    ci, cw = device_tables(Ws, Wd, mode, dev)
    out = torch.empty(N, C, Hd, Wd, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_resample, dev, N, C, Hs, Ws, Hd, Wd, x.data_ptr(), _strides(x), ri.data_ptr(), rw.data_ptr(), TAPS[mode],
          ci.data_ptr(), cw.data_ptr(), TAPS[mode], out.data_ptr())
    return unview(out)


def gaussian_blur(img: torch.Tensor, sigma: float, layout: str = "auto") -> torch.Tensor:
    """reni_gaussian_blur: scipy.ndimage.gaussian_filter(channel, sigma) of every channel of one image ([H,W], [H,W,C] or
    [C,H,W]; layout as in ``resample``): truncate 4, `reflect` boundary, rows first.  The result has the input's shape and
    layout, float32."""
    from .resample import gaussian_weights
    _require_cuda(img)
    if img.dim() not in (2, 3):
        raise ValueError(f"expected one image [H,W], [H,W,C] or [C,H,W], got {tuple(img.shape)}")
    w, r = gaussian_weights(sigma)
    x = _f32(img)
    out = torch.empty_like(x)
    if out.stride() != x.stride():
        x = x.contiguous()
        out = torch.empty_like(x)
    v, _ = _image_layout(x, layout)
    _, C, H, W = v.shape
    if min(C, H, W) < 1:
        raise ValueError(f"empty image {tuple(img.shape)}")
    dev = x.device
    lib = _lib.load()
    wt = torch.from_numpy(w.astype("float32")).to(dev)
    ws, wp, wn = _ws256(int(lib.reni_blur_workspace_bytes(C, H, W)), dev)
    _call(lib.reni_gaussian_blur, dev, C, H, W, x.data_ptr(), _strides(v[0]), wt.data_ptr(), r, out.data_ptr(), wp, wn)
    return out


_ROTATE_TRIG = {}


def _rotate_trig(H: int, W: int, device):
    """(row_trig [H, 2], col_trig [W, 2]) fp32 on ``device``: (sin, cos) of the grid's polar and azimuth angles (rotation.py)."""
    key = (H, W, device)
    t = _ROTATE_TRIG.get(key)
    if t is None:
        from .rotation import grid_trig
        t = tuple(torch.from_numpy(x.astype("float32")).to(device) for x in grid_trig(H, W))
        if len(_ROTATE_TRIG) >= 64:
            _ROTATE_TRIG.clear()
        _ROTATE_TRIG[key] = t
    return t


def rotate_envmap(src: torch.Tensor, rot: torch.Tensor, mode: str = "bilinear", layout: str = "auto", index=None) -> torch.Tensor:
    """reni_rotate_envmap: the equirectangular maps ``src`` turned by ``rot``, out(d) = src(R^T d), sampled on the sphere
    (wrap in longitude, pole crossings) with mode "bilinear" | "nearest" (conventions: reni_amd/rotation.py).  src is read in
    place through its strides, in the shapes ``resample`` accepts (a model output [B, P, 3]: ``out.view(B, H, W, 3)`` with
    layout="hwc"); the width must be even.  rot: [3, 3] shared, or [B, 3, 3] per image; it is NOT checked for orthogonality
    here (rotation.rotate_envmap does, at the price of a host synchronisation).  index: optional integer tensor [B]: image b
    of the result is src[index[b]] turned by rot[b] -- the gather and the rotation in one launch (src must be a batch).
    The result is planar float32 [B, C, H, W] ([C, H, W] / [H, W] for one image)."""
    _require_cuda(src, rot, index if isinstance(index, torch.Tensor) else None)
    if mode not in _lib.ROTATE_MODE:
        raise ValueError(f"mode must be one of {tuple(_lib.ROTATE_MODE)}, got {mode!r}")
    x, unview = _image_layout(_f32(src), layout)
    N, C, H, W = x.shape
    if min(N, C, H, W) < 1 or W % 2:
        raise ValueError(f"expected non-empty maps of even width, got {tuple(src.shape)}")
    dev = x.device
    if index is not None:
        if src.dim() != 4:
            raise ValueError(f"index= gathers from a batch of maps, got {tuple(src.shape)}")
        index = torch.as_tensor(index, dtype=torch.long).to(dev).contiguous()
        if index.dim() != 1 or index.numel() < 1:
            raise ValueError(f"index must be a non-empty 1-d integer tensor, got {tuple(index.shape)}")
    B = N if index is None else index.numel()
    rot = _f32c(rot)
    if rot.device != dev:
        raise ValueError(f"rot is on {rot.device}, the maps on {dev}")
    if tuple(rot.shape) == (3, 3):
        rot_stride = 0
    elif tuple(rot.shape) == (B, 3, 3):
        rot_stride = 9
    else:
        raise ValueError(f"rot must be [3, 3] or [{B}, 3, 3], got {tuple(rot.shape)}")
    rt, ct = _rotate_trig(H, W, dev)
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    _call(_lib.load().reni_rotate_envmap, dev, B, C, H, W, x.data_ptr(), _strides(x), _ptr(index), N,
          rot.data_ptr(), rot_stride, rt.data_ptr(), ct.data_ptr(), _lib.ROTATE_MODE[mode], out.data_ptr())
    return unview(out)


def _pair_args(pred, target, weight, size=None, check_weight=True):
    """(pred, target as float32 views [B, 3, H, W], weight as a float32 view [B, H, W] or None) without copying a pixel, or
    ValueError.  An image batch is [B, 3, H, W] with any strides or a model output [B, P, 3] (``size`` = (H, W); default: the
    other operand's, else P = H x 2H); the weight is anything that broadcasts to [B, H, W] (sin(phi) per row: [H, 1]) or a
    mask / sineweight [1 | B, P, 3] (channel 0 is read).  Negative weights raise (check_weight: one read-back per call)."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise ValueError("pred and target must be tensors")
    if size is None:
        for x in (pred, target):
            if x.dim() == 4:
                size = tuple(x.shape[-2:])
    views = []
    for name, x in (("pred", pred), ("target", target)):
        if x.dim() == 4 and x.shape[1] == 3:
            v = x
        elif x.dim() == 3 and x.shape[2] == 3:
            if size is None:
                H = math.isqrt(x.shape[1] // 2)
                if 2 * H * H != x.shape[1]:
                    raise ValueError(f"{name}: {x.shape[1]} pixels are not H x 2H; pass size=(H, W)")
                size = (H, 2 * H)
            if int(size[0]) * int(size[1]) != x.shape[1]:
                raise ValueError(f"{name}: {x.shape[1]} pixels are not {int(size[0])} x {int(size[1])}")
            v = x.unflatten(1, (int(size[0]), int(size[1]))).permute(0, 3, 1, 2)
        else:
            raise ValueError(f"{name} must be [B, 3, H, W] or a model output [B, P, 3], got {tuple(x.shape)}")
        views.append(_f32(v))
    p, t = views
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} are not the same batch of images")
    B, _, H, W = p.shape
    if min(B, H, W) < 1:
        raise ValueError(f"empty images {tuple(pred.shape)}")
    if p.device != t.device:
        raise ValueError(f"pred is on {p.device}, target on {t.device}")
    w = None
    if weight is not None:
        if not isinstance(weight, torch.Tensor):
            raise ValueError("weight must be a tensor or None")
        w = _f32(weight)
        if w.dim() == 3 and w.shape[2] == 3 and w.shape[1] == H * W and w.shape[0] in (1, B) and (H, W) != (H * W, 3):
            w = w[..., 0].unflatten(1, (H, W))
        try:
            w = torch.broadcast_to(w, (B, H, W))
        except RuntimeError:
            raise ValueError(f"weight {tuple(weight.shape)} does not broadcast to [{B}, {H}, {W}]") from None
        if w.device != p.device:
            raise ValueError(f"weight is on {w.device}, the images on {p.device}")
        if check_weight and not bool((weight >= 0).all()):  # (a read-back; callers that built the weight from checked parts skip it)
            raise ValueError("weights must be >= 0 (and not NaN)")
    return p, t, w


def _space_args(space, minmax, exposure, B, device):
    if space not in _lib.SPACE:
        raise ValueError(f"space must be one of {tuple(_lib.SPACE)}, got {space!r}")
    if space != "stored":
        if minmax is None:
            raise ValueError(f"space={space!r} maps the stored numbers back to radiance and needs minmax")
        if not float(minmax[1]) > float(minmax[0]):
            raise ValueError(f"minmax[1] must exceed minmax[0], got {tuple(minmax)}")
    if space == "srgb":
        if not isinstance(exposure, torch.Tensor) or tuple(exposure.shape) != (B,):
            raise ValueError(f"space='srgb' needs exposure, a tensor [{B}] (metrics.exposure(target, minmax))")
        if exposure.device != device:
            raise ValueError(f"exposure is on {exposure.device}, the images on {device}")
        exposure = _f32c(exposure)
    else:
        exposure = None
    m0, m1 = (float(minmax[0]), float(minmax[1])) if minmax is not None else (0.0, 1.0)
    return m0, m1, exposure


def _pair_call_head(p, t, w, space, m0, m1, exposure):
    B, _, H, W = p.shape
    return (B, H, W, p.data_ptr(), _strides(p), t.data_ptr(), _strides(t), _ptr(w), _strides(w),
            _lib.SPACE[space], m0, m1, _ptr(exposure))


def pair_stats(pred, target, weight=None, space: str = "stored", minmax=None, exposure=None, size=None,
               check_weight: bool = True) -> torch.Tensor:
    """reni_pair_stats: [B, 8] float32 = (sum w, sum w (p - t)^2, sum w |p - t|, sum w cos(p, t), max t, min t, sum w t^2,
    sum w t) per image, over pixels (weight w) and channels, of pred and target mapped into ``space`` ("stored" | "linear" |
    "srgb"; include/reni_hip.h) in registers.  Shapes, strides and weights as ``_pair_args`` takes them: nothing is copied,
    permuted or expanded.  "linear" and "srgb" need ``minmax``; "srgb" needs ``exposure`` [B].  check_weight=False skips the read-back that
    looks for negative weights (for a caller that built the weight from checked parts)."""
    p, t, w = _pair_args(pred, target, weight, size, check_weight)
    m0, m1, exposure = _space_args(space, minmax, exposure, p.shape[0], p.device)
    _require_cuda(p, t, w)
    lib = _lib.load()
    B, _, H, W = p.shape
    out = torch.empty(B, 8, dtype=torch.float32, device=p.device)
    ws, wp, wn = _ws256(int(lib.reni_pair_stats_workspace_bytes(B, H, W)), p.device)
    _call(lib.reni_pair_stats, p.device, *_pair_call_head(p, t, w, space, m0, m1, exposure), out.data_ptr(), wp, wn)
    return out


def ssim(pred, target, weight=None, space: str = "stored", minmax=None, exposure=None, L: float = 1.0, sphere: bool = True,
         return_map: bool = False, size=None, check_weight: bool = True):
    """reni_ssim: mean SSIM per image [B] (11 x 11 Gaussian window, sigma 1.5, dynamic range ``L``) of pred and target mapped
    into ``space``.  sphere=True: every pixel has a window, taken on the sphere (columns wrap, rows cross the poles; even
    width), and the mean is weighted; sphere=False: the published image definition (windows inside the image, no weight).
    return_map: also the per-pixel channel-mean map [B, H, W]."""
    p, t, w = _pair_args(pred, target, weight, size, check_weight)
    B, _, H, W = p.shape
    m0, m1, exposure = _space_args(space, minmax, exposure, B, p.device)
    if not float(L) > 0:
        raise ValueError(f"L must be > 0, got {L}")
    if sphere:
        if W % 2 or H < 5:
            raise ValueError(f"SSIM on the sphere needs an even width and H >= 5, got {H} x {W}")
    else:
        if w is not None:
            raise ValueError("the planar SSIM is the unweighted published definition: pass no weight (or sphere=True)")
        if H < 11 or W < 11:
            raise ValueError(f"the planar SSIM needs H, W >= 11, got {H} x {W}")
    _require_cuda(p, t, w)
    lib = _lib.load()
    out = torch.empty(B, dtype=torch.float32, device=p.device)
    smap = torch.empty(B, H, W, dtype=torch.float32, device=p.device) if return_map else None
    ws, wp, wn = _ws256(int(lib.reni_pair_stats_workspace_bytes(B, H, W)), p.device)
    _call(lib.reni_ssim, p.device, *_pair_call_head(p, t, w, space, m0, m1, exposure), float(L),
          _lib.SSIM_MODE["sphere" if sphere else "planar"], out.data_ptr(), _ptr(smap), wp, wn)
    return (out, smap) if return_map else out


LIGHT_MAX_WIDTH = 4096
_LIGHT_GRIDS = {}  # (W, device) -> light_grid's tables; the most recent LIGHT_GRIDS_KEPT keys only (a 4096-wide direction table is 100 MB)
LIGHT_GRIDS_KEPT = 2


def light_maps_view(maps, size=None):
    """maps as a float32 view [B, 3, H, W] on RENI's grid (W even, H = W / 2, W <= 4096) without copying a texel, or ValueError.
    maps: [B, H, W, 3], a model output [B, H W, 3] (``size`` = (H, W); default H x 2H) or planar [B, 3, H, W]."""
    if not isinstance(maps, torch.Tensor):
        raise ValueError("maps must be a tensor")
    if maps.dim() == 4 and maps.shape[3] == 3 and (maps.shape[1] != 3 or maps.shape[2] == 6):  # ([B, 3, 6, 3] is 3 x 6 texels: no planar map is 3 wide)
        maps = maps.permute(0, 3, 1, 2)
    elif not (maps.dim() == 4 and maps.shape[1] == 3) and not (maps.dim() == 3 and maps.shape[2] == 3):
        raise ValueError(f"maps must be [B, H, W, 3], a model output [B, H W, 3] or planar [B, 3, H, W], got {tuple(maps.shape)}")
    v = _pair_args(maps, maps, None, size)[0]
    H, W = int(v.shape[2]), int(v.shape[3])
    if W % 2 or H != W // 2 or W > LIGHT_MAX_WIDTH:
        raise ValueError(f"light tables live on RENI's grid: W even, H = W / 2 and W <= {LIGHT_MAX_WIDTH}, got {H} x {W}")
    if v.shape[0] > 65535:
        raise ValueError(f"at most 65535 maps per call, got {v.shape[0]}")
    return v


def _light_space(space, minmax):
    if space not in ("stored", "linear"):
        raise ValueError(f'space must be "stored" (the maps hold radiance) or "linear" (un-normalise with minmax), got {space!r}')
    return _space_args(space, minmax, None, 0, None)[:2]


def light_grid(W: int, device):
    """(solid_angle [H] float32, row_cos [H + 1] float64, dirs_table [H W, 3] float32) of the W / 2 x W grid on ``device``: the
    exact band solid angles of ``baselines.reni_grid_weights``, cos(i pi / H), and ``utils.get_directions(W)``."""
    import numpy as np
    from .baselines import reni_grid_weights
    from .utils import get_directions
    key = (int(W), str(device))
    if key in _LIGHT_GRIDS:
        _LIGHT_GRIDS[key] = _LIGHT_GRIDS.pop(key)  # (most recent last)
    else:
        while len(_LIGHT_GRIDS) >= LIGHT_GRIDS_KEPT:
            _LIGHT_GRIDS.pop(next(iter(_LIGHT_GRIDS)))
        H = int(W) // 2
        sa = torch.from_numpy(reni_grid_weights(W)[::int(W)].astype(np.float32))
        rc = torch.from_numpy(np.cos(np.arange(H + 1, dtype=np.float64) * np.pi / H))
        _LIGHT_GRIDS[key] = (sa.to(device), rc.to(device), get_directions(int(W))[0].to(device, torch.float32).contiguous())
    return _LIGHT_GRIDS[key]


def light_table_build(maps, space: str = "linear", minmax=None, mask=None, uniform_mix: float = 0.0, size=None):
    """reni_light_table_build: (pmf [B, H, W], cond [B, H, W], marg [B, H]) float32 of maps as ``light_maps_view`` takes them,
    read in place.  mask: anything ``_pair_args`` takes as a weight (broadcasts to [B, H, W], or [1 | B, H W, 3])."""
    v = light_maps_view(maps, size)
    m0, m1 = _light_space(space, minmax)
    if not 0.0 <= float(uniform_mix) <= 1.0:
        raise ValueError(f"uniform_mix must lie in [0, 1], got {uniform_mix}")
    w = _pair_args(v, v, mask, None, check_weight=False)[2]
    _require_cuda(v, w)
    lib = _lib.load()
    B, _, H, W = v.shape
    dev = v.device
    sa = light_grid(W, dev)[0]
    pmf = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    cond = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    marg = torch.empty(B, H, dtype=torch.float32, device=dev)
    ws, wp, wn = _ws256(int(lib.reni_light_table_workspace_bytes(B, H, W)), dev)
    _call(lib.reni_light_table_build, dev, B, H, W, v.data_ptr(), _strides(v), _ptr(w), _strides(w),
          _lib.SPACE[space], m0, m1,
          sa.data_ptr(), float(uniform_mix), pmf.data_ptr(), cond.data_ptr(), marg.data_ptr(), wp, wn)
    return pmf, cond, marg


def light_sample(pmf, cond, marg, maps, u, space: str = "linear", minmax=None, texel_weight=None, jitter: bool = False, size=None):
    """reni_light_sample: (index [B, S] int32, dirs [B, S, 3], pdf [B, S], radiance [B, S, 3], colors [B, S, 3]) for uniforms u
    [S, 2] (shared) or [B, S, 2]; texel_weight [H W] float32 or None (1)."""
    v = light_maps_view(maps, size)
    m0, m1 = _light_space(space, minmax)
    B, _, H, W = v.shape
    for name, t, shape in (("pmf", pmf, (B, H, W)), ("cond", cond, (B, H, W)), ("marg", marg, (B, H))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor {list(shape)} (the table of these maps)")
    if not isinstance(u, torch.Tensor) or u.dim() not in (2, 3) or u.shape[-1] != 2 or u.shape[-2] < 1 or (u.dim() == 3 and u.shape[0] != B):
        raise ValueError(f"u must be [S, 2] or [{B}, S, 2] with S >= 1, got {tuple(u.shape) if isinstance(u, torch.Tensor) else u!r}")
    S = int(u.shape[-2])
    if texel_weight is not None and (not isinstance(texel_weight, torch.Tensor) or tuple(texel_weight.shape) != (H * W,)):
        raise ValueError(f"texel_weight must be a tensor [{H * W}] or None")
    _require_cuda(v, pmf, cond, marg, u, texel_weight)
    pmf, cond, marg, u = pmf.contiguous(), cond.contiguous(), marg.contiguous(), _f32c(u)
    tw = None if texel_weight is None else _f32c(texel_weight)
    lib = _lib.load()
    dev = v.device
    sa, rc, dt = light_grid(W, dev)
    index = torch.empty(B, S, dtype=torch.int32, device=dev)
    dirs, radiance, colors = (torch.empty(B, S, 3, dtype=torch.float32, device=dev) for _ in range(3))
    pdf = torch.empty(B, S, dtype=torch.float32, device=dev)
    _call(lib.reni_light_sample, dev, B, H, W, S, pmf.data_ptr(), cond.data_ptr(), marg.data_ptr(), v.data_ptr(),
          _strides(v), _lib.SPACE[space], m0, m1, u.data_ptr(), 0 if u.dim() == 2 else 2 * S, dt.data_ptr(),
          sa.data_ptr(), rc.data_ptr(), _ptr(tw), 1 if jitter else 0, index.data_ptr(), dirs.data_ptr(),
          pdf.data_ptr(), radiance.data_ptr(), colors.data_ptr())
    return index, dirs, pdf, radiance, colors


def lights_irradiance(normals, dirs, colors, scale: float) -> torch.Tensor:
    """reni_lights_irradiance: out [B, P, 3] = scale sum_s max(0, normals[p] . dirs[b, s]) colors[b, s] for light lists dirs,
    colors [B, S, 3] and normals [P, 3] (shared) or [B, P, 3] (per map); no [B, P, S] tensor exists."""
    for name, t in (("dirs", dirs), ("colors", colors), ("normals", normals)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if dirs.dim() != 3 or dirs.shape[2] != 3 or dirs.shape != colors.shape or min(dirs.shape[:2]) < 1:
        raise ValueError(f"dirs and colors must both be [B, S, 3], got {tuple(dirs.shape)} and {tuple(colors.shape)}")
    B, S = int(dirs.shape[0]), int(dirs.shape[1])
    shape = _per_map_operand(normals, B)
    if shape is None or shape[0] < 1:
        raise ValueError(f"normals must be [P, 3] or [{B}, P, 3], got {tuple(normals.shape)}")
    P, stride = shape
    _require_cuda(normals, dirs, colors)
    normals, dirs, colors = _f32c(normals), _f32c(dirs), _f32c(colors)
    out = torch.empty(B, P, 3, dtype=torch.float32, device=dirs.device)
    _call(_lib.load().reni_lights_irradiance, dirs.device, B, P, S, normals.data_ptr(), stride, dirs.data_ptr(), colors.data_ptr(),
          float(scale), out.data_ptr())
    return out


def launch_count(reset: bool = False) -> int:
    """Kernel launches the library has issued so far in this process (reni_launch_count)."""
    return int(_lib.load().reni_launch_count(1 if reset else 0))
