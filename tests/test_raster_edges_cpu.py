"""CPU check of the rasteriser's edge cases (tests/raster_edge_cases.py), from the float64 reference alone and from an fp32
restatement of the kernels: the stacks' depth order and the winner it implies, the share of ambiguous pixels per case (none at
all where the image has a handful of pixels), that fp32 arithmetic in the kernel's written order picks the reference's face at
every pixel that is not ambiguous, and that the vertex-normal meshes leave half of their tolerance to the kernel."""
import numpy as np
import pytest

from tests import raster_edge_cases as E
from tests.test_raster_cpu import np_project, np_vertex_normals, pixel_ndc

IDS = [E.scene_id(k) for k in E.SCENES]


def test_case_lists_hold_the_shapes_they_name():
    assert E.SIZES == (1, 2, 3, 15, 16, 17, 31, 33) and set(E.CARVED_SIZES) <= set(E.SIZES)
    assert E.STACK_F == (255, 256, 257, 512, 513) and E.STACK_S == 16
    assert len(E.SCENES) == len(set(E.SCENES)) == 2 * 8 + 2 * 5 + 2 + 4 + 1
    off = E.gap_faces()
    assert off.sum() == 256 and not off[:64].any() and off[64:128].all() and not off[128:192].any() and off[192:256].all()
    assert np.array_equal(off[:256], off[256:])
    assert E.normals_mesh("strip", 257)[0].shape == (257, 3) and E.normals_mesh("fan")[1].shape == (E.FAN, 3)


@pytest.mark.parametrize("order", E.ORDERS)
@pytest.mark.parametrize("F", E.STACK_F)
def test_stacks_are_ordered_in_depth_and_cover_every_pixel(F, order):
    """every face of a stack holds every pixel centre well inside (so every chunk's list is full: n = 256, or F mod 256 in
    the last), depths are 1e-3 apart in the stack's order, and no pixel is ambiguous: the winner is face 0 or face F - 1"""
    verts, faces, R, T, S, winner = E.scene("stack", F, order)
    x, y, z = np_project(verts, R[0].double().numpy(), T[0].double().numpy(), E.TANF)
    X, Y, Z = x[faces], y[faces], z[faces]
    assert np.abs(Z - Z[:, :1]).max() <= 1e-6  # each face at one depth
    step = np.diff(Z[:, 0])
    assert np.all(np.abs(np.abs(step) - E.DEPTH_STEP) <= 1e-6) and np.all(step > 0 if order == "increasing" else step < 0)
    assert winner == (0 if order == "increasing" else F - 1)
    assert X.min(axis=1).max() <= -3.9 and X.max(axis=1).min() >= 3.9 and Y.min(axis=1).max() <= -2.9 and Y.max(axis=1).min() >= 4.9
    assert len({tuple(np.round(t, 6)) for t in np.stack([X, Y], -1).reshape(F, -1)}) == F  # no two alike
    ref = E.reference(("stack", F, order))
    assert (ref["pix_to_face"] == winner).all() and not ref["amb"].any()
    assert ref["bary"].min() > 0.05  # every pixel well inside: no pixel on an edge, shared or not


@pytest.mark.parametrize("key", E.SCENES, ids=IDS)
def test_ambiguous_share_and_the_fp32_restatement_agree_with_the_reference(key):
    verts, faces, R, T, S, winner = E.scene(*key)
    ref = E.reference(key)
    amb, p2f = ref["amb"], ref["pix_to_face"]
    share = float(amb.mean())
    print(f"{E.scene_id(key)}: S {S}, F {len(faces)}, covered {int((p2f >= 0).sum())} of {S * S}, ambiguous {share:.4f}")
    assert share <= E.AMB_CAP
    if S <= 2:
        assert not amb.any()
    if winner is not None:
        assert (p2f == winner).all() and not amb.any()
    elif key[0] == "soup":
        assert (p2f >= 0).any()
    got = E.raster_fp32(verts, faces, R[0].numpy(), T[0].numpy(), S)
    bad = (got != p2f) & ~amb
    assert not bad.any(), np.argwhere(bad)[:5].tolist()


@pytest.mark.parametrize("order", E.ORDERS)
def test_empty_waves_case_moves_the_named_faces_off_screen(order):
    verts, faces, R, T, S, winner = E.scene("gaps", order)
    x, y, _ = np_project(verts, R[0].double().numpy(), T[0].double().numpy(), E.TANF)
    off = E.gap_faces()
    assert (x[faces].min(axis=1) > 40)[off].all() and (x[faces].min(axis=1) < -3.9)[~off].all()
    centre, _ = pixel_ndc(S)
    assert np.abs(centre).max() < 1  # the moved faces' boxes miss every tile
    assert winner == (0 if order == "increasing" else 447) and not off[winner]


def test_huge_face_covers_the_view_with_barycentrics_inside_its_band():
    verts, faces, R, T, S, winner = E.scene("huge")
    x, y, _ = np_project(verts, R[0].double().numpy(), T[0].double().numpy(), E.TANF)
    assert np.ptp(x[faces[1]]) > 1e4 and np.ptp(x[faces[0]]) < 2
    ref = E.reference(("huge",))
    assert (ref["pix_to_face"] == 1).all() and ref["wtol"].max() < 1e-4 and ref["bary"].min() > 0.3


@pytest.mark.parametrize("case", E.NORMAL_CASES, ids=[E.scene_id(c) for c in E.NORMAL_CASES])
def test_normal_meshes_leave_room_for_the_kernel(case):
    verts, faces, tol, zero = E.normals_mesh(*case)
    ref = np_vertex_normals(verts, faces)
    got = E.vertex_normals_fp32(verts, faces)
    err = float(np.abs(got - ref).max())
    print(f"{E.scene_id(case)}: V {len(verts)}, F {len(faces)}, fp32 restatement max error {err:.2e} (tolerance {tol:.0e})")
    assert err <= 0.5 * tol
    for v in zero:
        assert (ref[v] == 0).all() and (got[v] == 0).all()
    used = np.zeros(len(verts), bool)
    ok = np.all((faces >= 0) & (faces < len(verts)), axis=1)
    used[faces[ok].reshape(-1)] = True
    assert set(np.flatnonzero(~used)) <= set(zero)
    if case[0] == "fan":
        assert np.bincount(faces.reshape(-1))[0] == E.FAN
    if case[0] == "strip":  # well-shaped: no angle below 30 degrees
        p = verts[faces].astype(np.float64)
        for k in range(3):
            a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
            cos = (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)
            assert cos.max() < np.cos(np.radians(30))
