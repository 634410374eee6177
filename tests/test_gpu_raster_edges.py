"""GPU tests of the mesh pipeline (reni_tu_raster.hip) at the shapes where its tile, chunk and block boundaries act: the
scenes of tests/raster_edge_cases.py against the float64 restatement of tests/test_raster_cpu.py through the _compare of
tests/test_gpu_raster.py (face, depth, barycentrics, distance, G-buffer, exact background), outputs carved between guard
bands, and vertex normals round the 256-vertex block.  tests/test_raster_edges_cpu.py shows that no case leaves the choice of
a face to rounding at more than AMB_CAP of its pixels."""
import ctypes

import numpy as np
import pytest
import torch

from tests import raster_edge_cases as E
from tests.test_gpu_baseline_edges import Carved, _dev, _lib, _stream, _workspace
from tests.test_gpu_raster import _compare
from tests.test_raster_cpu import np_vertex_normals

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _check_scene(key):
    verts, faces, R, T, S, winner = E.scene(*key)
    ref, n = _compare(verts, faces, R, T, S)
    assert ref["amb"].mean() <= E.AMB_CAP
    return ref, n, winner


@pytest.mark.parametrize("S", E.SIZES)
def test_image_sizes_round_the_tile(S):
    """a 60-face soup and one triangle over the whole view at S below, at and past one and two tiles"""
    ref, n, _ = _check_scene(("soup", S))
    assert n >= 1
    ref, n, _ = _check_scene(("cover", S))
    assert n == S * S and (ref["pix_to_face"] == 0).all()


@pytest.mark.parametrize("S", E.CARVED_SIZES)
def test_lanes_beyond_the_image_store_nothing(S):
    """every output of reni_rasterize_mesh between guard bands, the workspace poisoned: same bits as the ops call"""
    from reni_amd import ops
    for kind in ("soup", "cover"):
        verts, faces, R, T, _, _ = E.scene(kind, S)
        v, f = _t(verts), _t(faces)
        vn = ops.vertex_normals(v, f)
        want = ops.rasterize_mesh(v, f, vn, R, T, S)
        lib = _lib()
        outs = [Carved(1, S, S, 2), Carved(1, S, S, 1), Carved(1, S, S, 1, 3), Carved(1, S, S, 1), Carved(S * S, 3), Carved(S * S, 3)]
        ws, wp, wn = _workspace(int(lib.reni_raster_workspace_bytes(len(verts), len(faces), S, S)), 0xFF)
        Rh = (ctypes.c_float * 9)(*[float(x) for x in R.reshape(-1).tolist()])
        Th = (ctypes.c_float * 3)(*[float(x) for x in T.reshape(-1).tolist()])
        rc = lib.reni_rasterize_mesh(len(verts), len(faces), v.data_ptr(), f.data_ptr(), vn.data_ptr(), Rh, Th, 0.5773502691896258, S, S,
                                     *[o.ptr for o in outs], wp, wn, _stream())
        assert rc == 0, lib.reni_last_error()
        names = ("pix_to_face", "zbuf", "bary", "dists", "pixel_normals", "pixel_positions")
        for o, w, name in zip(outs, want, names):
            o.check(w.view(torch.int32).view(o.shape) if w.dtype == torch.int64 else w, f"{kind} S = {S}: {name}")


@pytest.mark.parametrize("order", E.ORDERS)
@pytest.mark.parametrize("F", E.STACK_F)
def test_full_chunks_round_the_chunk_boundary(F, order):
    """F screen-filling triangles: all 256 faces of a chunk land in the compaction list, and the nearest one is the first
    face of the first chunk or the last face of the last (partial) chunk"""
    ref, n, winner = _check_scene(("stack", F, order))
    assert n == E.STACK_S ** 2 and (ref["pix_to_face"] == winner).all() and winner == (0 if order == "increasing" else F - 1)


@pytest.mark.parametrize("order", E.ORDERS)
def test_waves_that_contribute_nothing(order):
    """waves 1 and 3 of every chunk find no face: wave 2's slots follow wave 0's directly"""
    ref, n, winner = _check_scene(("gaps", order))
    assert n == E.STACK_S ** 2 and (ref["pix_to_face"] == winner).all()


@pytest.mark.parametrize("what", E.EMPTY_KINDS)
def test_nothing_to_draw_is_all_background(what):
    from reni_amd import ops
    verts, faces, R, T, S, _ = E.scene("empty", what)
    ref, n, _ = _check_scene(("empty", what))  # (its background checks: -1, -1, -1 and zeros, exactly)
    assert n == 0 and (ref["pix_to_face"] == -1).all()
    v, f = _t(verts), _t(faces)
    p2f, zbuf, bary, dists, nrm, pos = ops.rasterize_mesh(v, f, ops.vertex_normals(v, f), R, T, S)
    assert bool((p2f == -1).all()) and bool((zbuf == -1).all()) and bool((bary == -1).all()) and bool((dists == -1).all())
    assert bool((nrm == 0).all()) and bool((pos == 0).all())


def test_a_face_much_larger_than_the_screen():
    ref, n, winner = _check_scene(("huge",))
    assert n == E.STACK_S ** 2 and (ref["pix_to_face"] == winner).all()


@pytest.mark.parametrize("case", E.NORMAL_CASES, ids=[E.scene_id(c) for c in E.NORMAL_CASES])
def test_vertex_normals_round_the_block_and_on_odd_meshes(case):
    from reni_amd import ops
    verts, faces, tol, zero = E.normals_mesh(*case)
    v, f = _t(verts), _t(faces)
    a, b = ops.vertex_normals(v, f), ops.vertex_normals(v, f)
    assert torch.equal(a, b) and a.shape == (len(verts), 3)
    err = np.abs(a.cpu().numpy() - np_vertex_normals(verts, faces))
    print(f"normals {E.scene_id(case)}: max error {float(err.max()):.2e} (tolerance {tol:.0e})")
    assert err.max() <= tol
    for k in zero:
        assert bool((a[k] == 0).all()), k  # no face: exactly zero, not the normalisation of rounding noise
    out = Carved(len(verts), 3)
    off, corners = ops._vertex_face_csr(f, len(verts))
    lib = _lib()
    rc = lib.reni_mesh_vertex_normals(len(verts), len(faces), v.data_ptr(), f.data_ptr(), off.data_ptr(), corners.data_ptr(), out.ptr,
                                      _stream())
    assert rc == 0, lib.reni_last_error()
    out.check(a, f"normals {E.scene_id(case)}")
