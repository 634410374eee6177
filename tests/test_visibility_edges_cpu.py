"""CPU side of the ray caster's edge cases (tests/visibility_edge_cases.py): every scene the GPU file uses stays within the
cap on its undecided share (a condition on the scenes, re-asserted here so that a scene that drifts fails without a GPU),
plain fp32 numpy agrees with float64 on every decided ray of each, the pinned directions and the holes mean what the GPU
file takes them to mean, and the float32 restatement of k_vis_prepare's boxes is checked against its definition."""
import numpy as np
import pytest

from tests import visibility_edge_cases as EC
from tests import visibility_ref as VR


def _fp32_against_fp64(name, sc, occ, dec, faces=None):
    o32, _ = VR.visibility_ref(sc["origins"], sc["own"], sc["dirs"], sc["verts"], sc["faces"] if faces is None else faces,
                               sc["t_min"], dtype=np.float32)
    rays, undecided, share, occluded = EC.shares(occ, dec, sc["own"])
    bad = (o32 != occ) & dec
    print(f"{name}: rays {rays}, undecided {undecided} ({100 * share:.3f} %), occluded {occluded:.3f} of the foreground, "
          f"fp32 vs float64: {int(bad.sum())} decided and {int(((o32 != occ) & ~dec).sum())} undecided rays differ")
    assert share <= VR.UNDECIDED_MAX, f"{share:.4f} of the rays are undecided"
    assert not bad.any(), f"fp32 differs from float64 on {int(bad.sum())} decided rays, first {np.argwhere(bad)[:3].tolist()}"


# ---------------------------------------------------------------------------------------------------------- A, B, E
@pytest.mark.parametrize("F,NP,J", EC.WIDE_CASES)
def test_wide_soups_are_within_the_cap_and_fp32_agrees(F, NP, J):
    sc, occ, dec = EC.wide_case(F, NP, J)
    assert sc["dirs"].shape == (J, 3) and (J + 255) // 256 >= 1
    _fp32_against_fp64(f"wide {F, NP, J}", sc, occ, dec)
    if NP > 3:
        fg = sc["own"] >= 0
        assert 0.02 < occ[fg].mean() < 0.9  # both answers
        # every 256-direction block has both answers too: a block read from the wrong place cannot pass by being constant
        for j0 in range(0, J - 1, 256):
            blk = occ[fg][:, j0:j0 + 256]
            assert blk.any() and not blk.all()
        # ... and no two blocks of a pixel's row are equal where they overlap
        if J > 256:
            n = J - 256
            assert (occ[fg][:, :n] != occ[fg][:, 256:256 + n]).any()


def test_per_image_lists_are_within_the_cap_and_differ():
    sc, dirs, refs = EC.per_image_case()
    assert dirs.shape == (EC.PER_IMAGE_B, EC.PER_IMAGE_J, 3)
    for b, (occ, dec) in enumerate(refs):
        one = dict(sc, dirs=dirs[b])
        _fp32_against_fp64(f"per-image list {b}", one, occ, dec)
    assert not (refs[0][0] == refs[1][0]).all() and not (refs[1][0] == refs[2][0]).all()
    buf, stride = EC.padded_rows(dirs)
    assert stride == 3 * EC.PER_IMAGE_J + EC.PER_IMAGE_GAP and buf.shape == (EC.PER_IMAGE_B * stride,)
    for b in range(EC.PER_IMAGE_B):
        row = buf[b * stride:(b + 1) * stride]
        assert (row[:3 * EC.PER_IMAGE_J].reshape(-1, 3) == dirs[b]).all() and np.isnan(row[3 * EC.PER_IMAGE_J:]).all()
    # a reader that took row b at b * 3 J would meet other numbers from image 1 on
    assert not np.array_equal(buf[3 * EC.PER_IMAGE_J:6 * EC.PER_IMAGE_J].reshape(-1, 3), dirs[1], equal_nan=True)


def test_t_min_zero_makes_the_own_face_exclusion_decisive():
    sc, occ, dec = EC.tmin0_case()
    assert sc["t_min"] == 0.0
    _fp32_against_fp64("t_min = 0", sc, occ, dec)
    # without the exclusion (own ids that match no face) a large share of the decided foreground rays changes: in fp32,
    # which is what a device without the comparison would compute
    fg = sc["own"] >= 0
    loose, _ = VR.visibility_ref(sc["origins"], np.where(fg, 130 + 5, -1), sc["dirs"], sc["verts"], sc["faces"], 0.0, dtype=np.float32)
    moved = ((loose != occ) & dec)[fg].mean()
    print(f"t_min = 0: {100 * moved:.1f} % of the foreground rays are decided and change when nothing is excluded")
    assert moved > 0.1


# --------------------------------------------------------------------------------------------------------------- C, D
def test_room_layout():
    sc = EC.room_scene()
    v, f = sc["verts"], sc["faces"]
    assert len(f) == EC.ROOM_F == 148 and sc["dirs"].shape == (127, 3) and sc["origins"].shape == (64, 3)
    tri = v[f]
    assert (tri[:64, :, 2] == 0.5).all() and (tri[64:136, :, 2] == 0.0).all()           # cluster 0 is the flat table top
    assert (tri[136:140, :, 0] == -1.0).all() and (tri[140:144, :, 0] == 1.0).all() and (tri[144:, :, 1] == 1.0).all()
    assert tri[136:, :, 2].min() == -0.5 and tri[136:, :, 2].max() == 1.0
    assert ((sc["own"] >= 64) & (sc["own"] < 136)).all() and (sc["origins"][:, 2] == 0.0).all()
    d = sc["dirs"]
    assert ((d[:26] == 0).any(axis=1)).sum() == 18  # all but the eight diagonals have a zero component
    assert np.allclose(np.linalg.norm(d[:122].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(d[122:], EC.PINNED, equal_nan=True)
    moved = EC.room_scene(EC.ROOM_OFFSETS[1])
    assert (moved["verts"] == (v + np.array(EC.ROOM_OFFSETS[1], np.float32))).all() and (moved["origins"][:, 2] == 5.0).all()


@pytest.mark.parametrize("offset", EC.ROOM_OFFSETS)
def test_room_is_within_the_cap_and_fp32_agrees(offset):
    sc, occ, dec = EC.room_case(offset)
    _fp32_against_fp64(f"room at {offset}", sc, occ, dec)
    # the pinned directions: zero, NaN and inf are visible from every pixel and decided; (0, 0, 7) and (0, 0, 1e-3) answer as +z
    assert not occ[:, 122:125].any() and dec[:, 122:125].all()
    up = int(np.flatnonzero((sc["dirs"][:26] == np.array([0, 0, 1], np.float32)).all(axis=1))[0])
    both = dec[:, up] & dec[:, 125] & dec[:, 126]
    assert both.sum() >= 48 and (occ[both, 125] == occ[both, up]).all() and (occ[both, 126] == occ[both, up]).all()
    assert occ[:, up].any() and not occ[:, up].all()  # some origins lie under the table, some do not
    # the rays inside the floor's plane meet the walls x = +-1 and y = 1 (decided) and nothing towards y = -1
    flat = np.flatnonzero(sc["dirs"][:26, 2] == 0)
    assert len(flat) == 8 and dec[:, flat].mean() > 0.95 and occ[:, flat].any() and not occ[:, flat].all()
    toward_open = int(np.flatnonzero((sc["dirs"][:26] == np.array([0, -1, 0], np.float32)).all(axis=1))[0])
    assert not occ[:, toward_open].any()


def test_room_answers_do_not_depend_on_the_offset():
    (a, occ_a, dec_a), (b, occ_b, dec_b) = (EC.room_case(o) for o in EC.ROOM_OFFSETS)
    both = dec_a & dec_b
    assert both.mean() > 0.98 and (occ_a[both] == occ_b[both]).all()


def test_cluster_boxes_follow_the_definition():
    for offset in EC.ROOM_OFFSETS:
        sc = EC.room_scene(offset)
        lo, hi, valid = EC.cluster_boxes(sc["verts"], sc["faces"])
        assert lo.dtype == np.float32 and lo.shape == (3, 3) and valid.all()
        for c in range(3):
            pts = sc["verts"][sc["faces"][c * 64:(c + 1) * 64].reshape(-1)].astype(np.float64)
            l, h = pts.min(axis=0), pts.max(axis=0)
            m = max((h - l).max(), np.abs(l).max(), np.abs(h).max()) / 1024.0
            # the definition in float64 to within a few float32 roundings of the largest number involved ...
            tol = 4 * 2.0 ** -24 * max(np.abs(l).max(), np.abs(h).max(), 1.0)
            assert np.abs(lo[c] - (l - m)).max() <= tol and np.abs(hi[c] - (h + m)).max() <= tol
            # ... and every face strictly inside, on every axis, the flat one included
            assert (lo[c] < l).all() and (hi[c] > h).all()
        off = np.asarray(offset, np.float64)
        assert lo[0, 2] < 0.5 + off[2] < hi[0, 2] and hi[0, 2] - lo[0, 2] < 0.02  # the table's box: zero thickness plus the margin
    # at the second offset the margin follows the position (5.5 / 1024), not the extent (1 / 1024)
    lo0, hi0, _ = EC.cluster_boxes(EC.room_scene(EC.ROOM_OFFSETS[0])["verts"], EC.room_scene()["faces"])
    lo1, hi1, _ = EC.cluster_boxes(EC.room_scene(EC.ROOM_OFFSETS[1])["verts"], EC.room_scene()["faces"])
    assert (hi1[0, 2] - lo1[0, 2]) > 4 * (hi0[0, 2] - lo0[0, 2])
    # slots: an order entry outside [0, F) and a face with a bad index take no part; a cluster of nothing else is invalid
    sc, _, _ = EC.holes_case("empty_cluster")
    lo, hi, valid = EC.cluster_boxes(sc["verts"], sc["faces"])
    assert valid.tolist() == [True, False, True] and not lo[1].any() and not hi[1].any()
    sc, _, _ = EC.holes_case("bad_order")
    a = EC.cluster_boxes(sc["verts"], sc["faces"], sc["order"])
    gone = np.where(np.isin(np.arange(130), sc["order"])[:, None], sc["faces"], -1)
    b = EC.cluster_boxes(sc["verts"], gone)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("offset", EC.ROOM_OFFSETS)
def test_probes_sit_on_the_box_planes_and_are_within_the_cap(offset):
    sc, occ, dec = EC.probe_case(offset)
    lo, hi, _ = EC.cluster_boxes(sc["verts"], sc["faces"])
    assert sc["origins"].shape == (18, 3) and (sc["own"] == EC.ROOM_F + 5).all()
    k = 0
    for c in range(3):
        for x in range(3):
            for plane in (lo[c, x], hi[c, x]):
                o = sc["origins"][k]
                assert o[x] == plane  # exactly: the slab test's numerator is 0 there
                others = [y for y in range(3) if y != x]
                assert (o[others] > lo[c, others]).all() and (o[others] < hi[c, others]).all()
                k += 1
    # each probe has rays parallel to its plane (0 * inf in the slab test of its own cluster's box)
    assert ((sc["dirs"][:26] == 0).sum(axis=0) == 8).all()
    _fp32_against_fp64(f"box-plane probes at {offset}", sc, occ, dec)
    assert occ.any() and not occ.all()


@pytest.mark.parametrize("offset", EC.ROOM_OFFSETS)
def test_a_nan_in_the_slab_test_skips_the_cluster_and_that_is_right(offset):
    """The kernel's slab test in float32 numpy (np.fmin / np.fmax drop a NaN as fminf / fmaxf do) on the rays of each probe
    that are parallel to the probe's plane: the quotient of that plane is 0 * inf = NaN, the pair's other quotient +inf (lo
    plane) or -inf (hi plane) takes its place, and the cluster is not touched.  In float64 none of those rays meets a face
    of that cluster, so skipping it loses nothing."""
    sc = EC.probe_scene(offset)
    lo, hi, _ = EC.cluster_boxes(sc["verts"], sc["faces"])
    dirs = sc["dirs"][:26]
    k = 0
    for c in range(3):
        only_c = np.where(((np.arange(EC.ROOM_F) // 64) == c)[:, None], sc["faces"], -1)
        for x in range(3):
            for side in ("lo", "hi"):
                o = sc["origins"][k]
                par = dirs[dirs[:, x] == 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    inv = np.float32(1.0) / par
                    q0, q1 = (lo[c] - o) * inv, (hi[c] - o) * inv
                assert np.isnan(q0[:, x] if side == "lo" else q1[:, x]).all()
                tn = np.fmax.reduce(np.fmin(q0, q1), axis=1)
                tf = np.fmin.reduce(np.fmax(q0, q1), axis=1)
                assert (tn == np.inf).all() if side == "lo" else (tf == -np.inf).all()
                with np.errstate(invalid="ignore"):
                    assert not ((tf >= 0) & (tf * np.float32(1.000002) >= tn)).any()
                occ, dec = VR.visibility_ref(o[None], [EC.ROOM_F + 5], par, sc["verts"], only_c, sc["t_min"])
                assert not occ.any() and dec.all()
                k += 1
    assert k == 18


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("kind", EC.HOLES_KINDS)
def test_holes_are_within_the_cap_and_mean_what_the_gpu_file_assumes(kind):
    sc, occ, dec = EC.holes_case(kind)
    fg = sc["own"] >= 0
    ref_faces = None
    if kind == "bad_order":
        ref_faces = np.where(np.isin(np.arange(130), sc["order"])[:, None], sc["faces"], -1)
        assert sorted(set(range(130)) - set(sc["order"].tolist())) == [3, 10, 70, 100]
        assert (sc["order"] == 11).sum() == 2 and -1 in sc["order"] and 130 in sc["order"] and (1 << 40) in sc["order"]
    if kind == "never_prepared":
        ref_faces = np.full_like(sc["faces"], -1)
    _fp32_against_fp64(f"holes, {kind}", sc, occ, dec, faces=ref_faces)
    if kind in ("one_bad_face", "never_prepared"):
        assert fg.any() and (~fg).any() and not occ[fg].any() and dec.all()  # every foreground bit 1
    if kind == "all_background":
        assert not fg.any() and occ.all()
    if kind == "own_ids":
        assert fg.all() and set(sc["own"].tolist()) >= {135, EC.OWN_PAST_INT32, EC.OWN_WRAPS_TO_A_FACE}
        # face 7, which an id truncated to 32 bits would exclude, does occlude decided rays of those rows
        rows = sc["own"] == EC.OWN_WRAPS_TO_A_FACE
        without, _ = VR.visibility_ref(sc["origins"][rows], np.full(int(rows.sum()), 7), sc["dirs"], sc["verts"], sc["faces"], sc["t_min"])
        print(f"own ids: excluding face 7 would change {int(((without != occ[rows]) & dec[rows]).sum())} decided rays")
    if kind in ("empty_cluster", "bad_order", "own_ids"):
        assert occ[fg].any() and not occ[fg].all()


# ------------------------------------------------------------------------------------------------------------------ G
def test_sphere_under_the_512_direction_grid_is_within_the_cap():
    sc, occ, dec = EC.sphere_case()
    fg = sc["own"] >= 0
    assert sc["dirs"].shape == (512, 3) and 40 < fg.sum() < 256
    _fp32_against_fp64("uv sphere 16 x 16, J = 512", sc, occ, dec)
    assert 0.35 < occ[fg].mean() < 0.65  # the directions below a pixel's horizon
