"""CPU tests of cast shadows: the float64 restatement of the visibility definition (tests/visibility_ref.py) on analytic
scenes, plain fp32 against float64 on every scene the GPU tests use, the mask's packing, and the argument checks and header
entries of the new calls (reni_tu_visibility.hip, the masked shader)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import visibility_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one large triangle in the plane z = 1 above the origin: it covers the directions within ~60 degrees of +z
BIG = np.array([[-4.0, -3.0, 1.0], [4.0, -3.0, 1.0], [0.0, 5.0, 1.0]])


def _ref(origins, own, dirs, verts, faces, t_min=1e-3):
    return VR.visibility_ref(np.atleast_2d(origins), np.atleast_1d(own), np.atleast_2d(dirs), verts, np.atleast_2d(faces), t_min)


def _unit(*d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_point_under_a_triangle_inside_and_outside_its_cone():
    dirs = _unit([0, 0, 1], [0.3, 0.2, 1], [-0.5, 0.4, 1], [0, 0, -1], [1, 0, 0], [5, 0, 1], [0, -4, 1], [0.3, 0.2, -1])
    occ, dec = _ref([0, 0, 0], [7], dirs, BIG, [0, 1, 2])
    assert occ[0].tolist() == [True, True, True, False, False, False, False, False]
    assert dec.all()
    # two-sided: the same triangle with the other winding, and seen from above
    occ2, _ = _ref([0, 0, 0], [7], dirs, BIG, [0, 2, 1])
    assert (occ2 == occ).all()
    occ3, _ = _ref([0, 0, 2], [7], dirs * [1, 1, -1], BIG, [0, 1, 2])
    assert (occ3 == occ).all()


def test_own_face_is_excluded():
    occ, dec = _ref([0, 0, 0], [0], _unit([0, 0, 1]), BIG, [0, 1, 2])
    assert not occ[0, 0] and dec[0, 0]
    occ, _ = _ref([0, 0, 0], [1], _unit([0, 0, 1]), BIG, [[0, 1, 2], [0, 1, 2]])  # a copy with another id still blocks
    assert occ[0, 0]


def test_hit_closer_than_t_min_is_ignored():
    d = _unit([0, 0, 1])
    assert _ref([0, 0, 0], [7], d, BIG, [0, 1, 2], t_min=0.5)[0][0, 0]
    occ, dec = _ref([0, 0, 0], [7], d, BIG, [0, 1, 2], t_min=1.5)
    assert not occ[0, 0] and dec[0, 0]
    occ, dec = _ref([0, 0, 0], [7], d, BIG, [0, 1, 2], t_min=1.0)  # t > t_min is strict, and this ray sits on the bound
    assert not occ[0, 0] and not dec[0, 0]
    # a hit behind the origin is never one
    assert not _ref([0, 0, 2], [7], d, BIG, [0, 1, 2], t_min=0.0)[0][0, 0]


def test_degenerate_faces_and_bad_indices_are_skipped():
    verts = np.concatenate([BIG, [[0.0, 0.0, 1.0]]])
    d = _unit([0, 0, 1])
    for face in ([0, 1, 1], [0, 0, 0], [3, 3, 0]):            # zero area: a == 0 for every ray
        occ, dec = _ref([0, 0, 0], [7], d, verts, face)
        assert not occ[0, 0] and dec[0, 0]
    for face in ([0, 1, -1], [0, 1, 4], [9, 1, 2]):           # an index outside [0, V)
        occ, dec = _ref([0, 0, 0], [7], d, verts, face)
        assert not occ[0, 0] and dec[0, 0]
    occ, _ = _ref([0, 0, 0], [7], d, verts, [[0, 1, -1], [0, 1, 1], [0, 1, 2]])
    assert occ[0, 0]                                          # ... and the valid face behind them still counts


def test_background_rows_and_edge_rays_are_marked():
    dirs = _unit([0, 0, 1], [4, -3, 1])                       # the second ray runs through a vertex: undecided
    occ, dec = _ref([[0, 0, 0], [0, 0, 0]], [7, -1], dirs, BIG, [0, 1, 2])
    assert occ[1].all() and dec[1].all()                      # background: every bit 0, nothing to decide
    assert occ[0, 0] and dec[0, 0] and not dec[0, 1]


def _fp32_against_fp64(sc, occ, dec):
    o32, _ = VR.visibility_ref(sc["origins"], sc["own"], sc["dirs"], sc["verts"], sc["faces"], sc["t_min"], dtype=np.float32)
    undecided = 1.0 - dec.mean()
    assert undecided <= VR.UNDECIDED_MAX, f"{undecided:.4f} of the rays are undecided"
    bad = (o32 != occ) & dec
    assert not bad.any(), f"fp32 differs from float64 on {int(bad.sum())} decided rays, first {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("F,NP,J", VR.SOUP_CASES)
def test_fp32_agrees_with_float64_on_decided_soup_rays(F, NP, J):
    sc, occ, dec = VR.soup_case(F, NP, J)
    assert sc["origins"].shape == (NP, 3) and sc["dirs"].shape == (J, 3) and len(sc["faces"]) == F
    if NP > 1:
        assert (sc["own"] < 0).any() and (sc["own"] >= 0).any()
    _fp32_against_fp64(sc, occ, dec)


def test_fp32_agrees_with_float64_on_decided_teapot_rays():
    sc, occ, dec = VR.teapot_case()
    fg = sc["own"] >= 0
    assert 150 < fg.sum() < 600 and sc["dirs"].shape == (128, 3)
    assert 0.3 < occ[fg].mean() < 0.8                         # the handle, spout and lid do cast shadows
    _fp32_against_fp64(sc, occ, dec)


def test_soups_exercise_both_answers():
    occ = np.concatenate([VR.soup_case(F, 257, 129)[1][VR.soup_case(F, 257, 129)[0]["own"] >= 0].reshape(-1) for F in (63, 64, 65, 130)])
    assert 0.15 < occ.mean() < 0.6


@pytest.mark.parametrize("J", [1, 31, 32, 33, 129])
def test_unpack_visibility_round_trips(J):
    from reni_amd.mesh import unpack_visibility
    rng = np.random.default_rng(J)
    vis = rng.random((2, 5, J)) < 0.5
    words = VR.pack_bits(vis)
    assert words.shape == (2, 5, (J + 31) // 32) and words.dtype == np.int32
    # the layout itself: bit j & 31 of word j >> 5
    for j in (0, J // 2, J - 1):
        assert (((words[..., j >> 5].astype(np.int64) >> (j & 31)) & 1).astype(bool) == vis[..., j]).all()
    back = unpack_visibility(torch.from_numpy(words), J)
    assert back.dtype == torch.bool and back.shape == (2, 5, J) and (back.numpy() == vis).all()
    ones = unpack_visibility(torch.full((1, 3, (J + 31) // 32), -1, dtype=torch.int32), J)  # every bit set, the sign bit too
    assert bool(ones.all())
    with pytest.raises(ValueError):
        unpack_visibility(torch.from_numpy(words), J + 32)
    with pytest.raises(ValueError):
        unpack_visibility(torch.from_numpy(words).to(torch.int64), J)


def test_argument_checks_come_before_the_library():
    """Bad masks and direction shapes raise ValueError on CPU tensors (nothing reaches the library); a well-formed call
    with CPU tensors raises RENILibraryError: there is no CPU path."""
    from reni_amd import _lib, lighting, ops
    from reni_amd.envmap_shader import EnvironmentMap, blinn_phong_shading_gbuffer
    NP, J = 6, 40
    nrm, pos, cam = torch.randn(NP, 3), torch.randn(NP, 3), torch.zeros(3)
    dirs, C = torch.randn(J, 3), torch.rand(2, J, 3)
    good = torch.zeros(1, NP, 2, dtype=torch.int32)
    for fn, src in ((ops.envmap_shade, C), (ops.envmap_shade_backward, torch.rand(2, NP, 3))):
        with pytest.raises(ValueError, match="int32"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=good.to(torch.int64))
        with pytest.raises(ValueError, match="int32"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=good.to(torch.float32))
        with pytest.raises(ValueError, match=r"\[NB, 6, 2\]"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=torch.zeros(1, NP, 3, dtype=torch.int32))   # wrong JW
        with pytest.raises(ValueError, match=r"\[NB, 6, 2\]"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=torch.zeros(1, NP + 1, 2, dtype=torch.int32))
        with pytest.raises(ValueError, match="require grad"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=torch.zeros(1, NP, 2, requires_grad=True))
        with pytest.raises(ValueError, match="per-image directions"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=torch.zeros(2, NP, 2, dtype=torch.int32))
        for bad_dirs in (torch.randn(J), torch.randn(J, 4), torch.randn(1, 2, J, 3)):
            with pytest.raises(ValueError, match=r"\[J, 3\]"):
                fn(nrm, pos, cam, bad_dirs, src, 10.0, 0.5, 0.5, vis=good)
        with pytest.raises(_lib.RENILibraryError, match="GPU"):
            fn(nrm, pos, cam, dirs, src, 10.0, 0.5, 0.5, vis=good)
    env = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3), sineweight=torch.ones(1, J, 1))
    with pytest.raises(ValueError, match="require grad"):
        blinn_phong_shading_gbuffer(nrm, pos, cam, env, 10.0, 0.5, 0.5, vis=torch.zeros(1, NP, 2, requires_grad=True))
    # the ray caster
    accel, p2f = torch.zeros(256, dtype=torch.uint8), torch.zeros(NP, dtype=torch.int64)
    for bad_dirs in (torch.randn(J), torch.randn(J, 2), torch.randn(1, 1, J, 3)):
        with pytest.raises(ValueError, match=r"\[J, 3\]"):
            ops.mesh_visibility(pos, p2f, bad_dirs, accel, 1e-3)
    with pytest.raises(ValueError, match="int64"):
        ops.mesh_visibility(pos, p2f.to(torch.int32), dirs, accel, 1e-3)
    with pytest.raises(ValueError, match="int64"):
        ops.mesh_visibility(pos, p2f[:-1], dirs, accel, 1e-3)
    with pytest.raises(ValueError, match="t_min"):
        ops.mesh_visibility(pos, p2f, dirs, accel, -1.0)
    with pytest.raises(ValueError, match="accel"):
        ops.mesh_visibility(pos, p2f, dirs, accel.to(torch.float32), 1e-3)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.mesh_visibility(pos, p2f, dirs, accel, 1e-3)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.mesh_visibility_prepare(torch.randn(4, 3), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.mesh_visibility_prepare(torch.randn(4, 2), torch.zeros(2, 3, dtype=torch.int64))
    # ambient occlusion: a shared grid and its mask
    with pytest.raises(ValueError):
        lighting.ambient_occlusion(good, nrm, dirs.expand(2, J, 3), torch.ones(J))
    with pytest.raises(ValueError):
        lighting.ambient_occlusion(torch.zeros(2, NP, 2, dtype=torch.int32), nrm, dirs, torch.ones(J))
    with pytest.raises(ValueError):
        lighting.ambient_occlusion(good, nrm, dirs, torch.ones(J + 1))
    with pytest.raises(ValueError):
        lighting.shade_sampled("samples", nrm, pos, cam, 10.0, 0.5, 0.5, visibility=good)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from reni_amd import _lib
    lib = _lib.load()
    assert lib.reni_mesh_visibility_accel_bytes(0) == 0 and lib.reni_mesh_visibility_accel_bytes(1 << 31) == 0
    # header + per cluster of 64 faces: a box (32 bytes) and 64 face records of 48 bytes
    assert lib.reni_mesh_visibility_accel_bytes(1) == 64 + 32 + 64 * 48
    assert lib.reni_mesh_visibility_accel_bytes(65) == 64 + 2 * (32 + 64 * 48)
    assert lib.reni_mesh_visibility_prepare(3, 1, None, None, None, None, 0, None) == -1 and b"NULL" in lib.reni_last_error()
    assert lib.reni_mesh_visibility_prepare(3, 0, 16, 16, None, 16, 1 << 20, None) == -1
    assert lib.reni_mesh_visibility_prepare(3, 1, 16, 16, None, 16, 8, None) == -2      # accel too small
    assert lib.reni_mesh_visibility(1, 4, 4, None, None, None, 0, None, 0.0, 0, None, None) == -1
    assert lib.reni_mesh_visibility(1, 0, 4, 16, 16, 16, 0, 16, 0.0, 0, 16, None) == -1
    assert lib.reni_mesh_visibility(1, 4, 4, 16, 16, 16, 0, 16, -1.0, 0, 16, None) == -1 and b"t_min" in lib.reni_last_error()
    assert lib.reni_mesh_visibility(1, 4, 4, 16, 16, 16, 0, 16, float("nan"), 0, 16, None) == -1
    assert lib.reni_mesh_visibility(1, 4, 4, 16, 16, 16, 0, 16, 0.0, 2, 16, None) == -1 and b"flag" in lib.reni_last_error()
    assert lib.reni_mesh_visibility(2, 4, 4, 16, 16, 16, 5, 16, 0.0, 0, 16, None) == -1  # a batch stride below 3 J
    for fn in (lib.reni_envmap_shade_masked, lib.reni_envmap_shade_masked_backward):
        head = (2, 4, 40, 16, 16, 0.0, 0.0, 0.0, 16)
        assert fn(*head, 0, 16, 10.0, 0.5, 0.5, None, 0, 16, None, 0, None) == -1 and b"mask" in lib.reni_last_error()
        assert fn(*head, 0, 16, 10.0, 0.5, 0.5, 16, 8, 16, None, 0, None) == -1      # per-image masks on a shared grid
        assert fn(*head, 120, 16, 10.0, 0.5, 0.5, 16, 7, 16, None, 0, None) == -1    # stride below NP JW


def test_header_binding_build_and_docs_name_the_new_entry_points():
    from reni_amd import _lib
    names = ("reni_mesh_visibility_accel_bytes", "reni_mesh_visibility_prepare", "reni_mesh_visibility",
             "reni_envmap_shade_masked", "reni_envmap_shade_masked_backward")
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in names:
        assert n in _lib.EXPORTS
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in integration, n
    assert re.search(r"#define\s+RENI_VIS_NO_CULL\s+1u", header) and _lib.VIS_NO_CULL == 1
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert re.search(r"for tu in [^;]*\bvisibility\b", build) and "_build/visibility.o" in build
