"""Edge shapes of the cast-shadow ray caster (reni_tu_visibility.hip: k_vis_prepare, k_mesh_visibility): direction counts that
need more than one 256-direction block of the grid's y axis, per-image lists with a padded row stride, an axis-aligned room
whose directions have zero components, origins exactly on the planes of the inflated cluster boxes, t_min = 0 (where the
own-face exclusion decides), and records with holes.  The case lists, the deterministic scene builders and a float32
restatement of k_vis_prepare's boxes, shared by tests/test_visibility_edges_cpu.py and tests/test_gpu_visibility_edges.py.

Plain data on the CPU; nothing here touches a device.  The float64 reference, its margin and the cap on the undecided share
are tests/visibility_ref.py's (visibility_ref, MARGIN, UNDECIDED_MAX); nothing of them is restated here."""
import functools

import numpy as np

from tests import visibility_ref as VR

CLUSTER = 64  # faces per cluster of the record
BOX_MARGIN = np.float32(1.0 / 1024.0)

# ---------------------------------------------------------------------------------------------------------- A. wide J
# (F, NP, J): y-blocks 0 .. 4 of the grid; 255 / 256 / 257 = one short of a block, a block, a block and one live lane (the
# second block's other three waves have no direction at all, and JW = 9 is odd: the last word is a wave's first); 513 and
# 1025 the same two and four blocks further on; F = 1 a record of one cluster with one face
WIDE_CASES = [(130, 17, 255), (130, 17, 256), (130, 17, 257), (65, 9, 513), (64, 5, 1025), (1, 3, 257)]


def wide_case(F, NP, J):
    """(scene, occluded, decided) of VR.soup_scene(F, NP, J), the reference computed once per process"""
    return VR.soup_case(F, NP, J)


def _ref(sc, own=None, dirs=None, faces=None):
    occ, dec = VR.visibility_ref(sc["origins"], sc["own"] if own is None else own, sc["dirs"] if dirs is None else dirs,
                                 sc["verts"], sc["faces"] if faces is None else faces, sc["t_min"])
    occ.setflags(write=False); dec.setflags(write=False)
    return occ, dec


# -------------------------------------------------------------------------------------------------- B. per-image lists
PER_IMAGE_B, PER_IMAGE_J, PER_IMAGE_GAP = 3, 257, 5  # row stride 3 J + 5 floats


@functools.lru_cache(maxsize=None)
def per_image_case():
    """-> (scene, dirs [B, J, 3] float32, [(occluded, decided)] per image): the soup (130, 17, 257) under B lists of its own"""
    sc = VR.soup_scene(130, 17, PER_IMAGE_J)
    rng = np.random.default_rng(57)
    dirs = np.stack([VR.unit_dirs(rng, PER_IMAGE_J) for _ in range(PER_IMAGE_B)])
    dirs.setflags(write=False)
    return sc, dirs, [_ref(sc, dirs=dirs[b]) for b in range(PER_IMAGE_B)]


def padded_rows(dirs, gap=PER_IMAGE_GAP):
    """dirs [B, J, 3] -> (flat float32 buffer, row stride in floats): row b at b * (3 J + gap), the gaps filled with NaN"""
    B, J, _ = dirs.shape
    stride = 3 * J + gap
    buf = np.full(B * stride, np.nan, np.float32)
    for b in range(B):
        buf[b * stride:b * stride + 3 * J] = dirs[b].reshape(-1)
    return buf, stride


# ------------------------------------------------------------------------------------------------------------ C. room
ROOM_OFFSETS = ((0.0, 0.0, 0.0), (3.0, -2.0, 5.0))
ROOM_F, ROOM_TABLE, ROOM_FLOOR = 148, 64, 72
ROOM_NP = 64
# the five pinned directions at the end of the list: zero, NaN and inf (no face can hit: a is 0, NaN, or every quotient is),
# and two vectors along +z that are not unit (t scales by 1 / |d|)
PINNED = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.inf, 0.0], [0.0, 0.0, 7.0], [0.0, 0.0, 1e-3]], np.float32)


def _quads(corner, du, dv, nu, nv):
    """the rectangle corner + [0, 1] du + [0, 1] dv as nu x nv quads of two triangles each -> [2 nu nv, 3, 3]"""
    corner, du, dv = (np.asarray(x, np.float64) for x in (corner, du, dv))
    tris = []
    for j in range(nv):
        for i in range(nu):
            p00 = corner + du * (i / nu) + dv * (j / nv)
            p10 = corner + du * ((i + 1) / nu) + dv * (j / nv)
            p01 = corner + du * (i / nu) + dv * ((j + 1) / nv)
            p11 = corner + du * ((i + 1) / nu) + dv * ((j + 1) / nv)
            tris += [[p00, p10, p11], [p00, p11, p01]]
    return np.array(tris)


def room_dirs():
    """the 26 normalised vectors with components in {-1, 0, 1}, 96 random unit vectors, the 5 pinned: [127, 3] float32"""
    axis = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    axis = (axis / np.linalg.norm(axis, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([axis, VR.unit_dirs(np.random.default_rng(26), 96), PINNED])


@functools.lru_cache(maxsize=None)
def room_scene(offset=(0.0, 0.0, 0.0)):
    """An axis-aligned room, its faces in the order the record is to keep (order = arange): the table top z = 0.5 over
    [-0.5, 0.5] x [-0.25, 0.25] (64 faces: cluster 0, flat), the floor z = 0 over [-1, 1]^2 (72 faces), the walls x = -1,
    x = 1, y = 1 over z in [-0.5, 1] (4 faces each: they stand through the floor's plane, so a ray inside that plane meets a
    wall inside a face).  64 origins on random floor faces (own = that face); the whole scene moved by ``offset`` in float32."""
    tris = np.concatenate([_quads([-0.5, -0.25, 0.5], [1, 0, 0], [0, 0.5, 0], 8, 4),
                           _quads([-1, -1, 0], [2, 0, 0], [0, 2, 0], 6, 6),
                           _quads([-1, -1, -0.5], [0, 2, 0], [0, 0, 1.5], 2, 1),
                           _quads([1, -1, -0.5], [0, 2, 0], [0, 0, 1.5], 2, 1),
                           _quads([-1, 1, -0.5], [2, 0, 0], [0, 0, 1.5], 2, 1)])
    assert len(tris) == ROOM_F
    verts = (tris.reshape(-1, 3).astype(np.float32) + np.asarray(offset, np.float32)).astype(np.float32)
    faces = np.arange(3 * ROOM_F, dtype=np.int64).reshape(ROOM_F, 3)
    rng = np.random.default_rng(148)
    own = ROOM_TABLE + rng.integers(0, ROOM_FLOOR, ROOM_NP)
    w = rng.dirichlet([2.0, 2.0, 2.0], ROOM_NP)
    origins = np.einsum("pk,pkd->pd", w, verts.astype(np.float64)[faces[own]]).astype(np.float32)
    return dict(verts=verts, faces=faces, origins=origins, own=own.astype(np.int64), dirs=room_dirs(),
                t_min=1e-4 * VR.bbox_diag(verts))


@functools.lru_cache(maxsize=None)
def room_case(offset=(0.0, 0.0, 0.0)):
    sc = room_scene(offset)
    return (sc,) + _ref(sc)


# ------------------------------------------------------------------------------------------------- D. box-plane probes
def cluster_boxes(verts, faces, order=None):
    """float32 restatement of k_vis_prepare's boxes: per cluster of 64 consecutive slots (slot k = face order[k]) the
    bounds of its valid faces, grown by m = max(extent, |lo|, |hi|) * 2^-10 over the three axes -> (lo [NC, 3], hi [NC, 3],
    valid [NC]) in float32; a cluster without a valid face has valid False and zeros"""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    V, F = len(verts), len(faces)
    order = np.arange(F) if order is None else np.asarray(order, np.int64)
    NC = (F + CLUSTER - 1) // CLUSTER
    lo, hi, valid = np.zeros((NC, 3), np.float32), np.zeros((NC, 3), np.float32), np.zeros(NC, bool)
    for c in range(NC):
        pts = []
        for f in order[c * CLUSTER:(c + 1) * CLUSTER]:
            if 0 <= f < F and np.all((faces[f] >= 0) & (faces[f] < V)):
                pts.append(verts[faces[f]])
        if not pts:
            continue
        pts = np.concatenate(pts)
        l, h = pts.min(axis=0), pts.max(axis=0)
        m = np.float32(max(np.max(h - l), np.max(np.abs(l)), np.max(np.abs(h)))) * BOX_MARGIN
        lo[c], hi[c], valid[c] = l - m, h + m, True
    return lo, hi, valid


PROBE_FRACTIONS = np.array([0.37, 0.61, 0.43], np.float32)
PROBE_OWN_PAST_F = 5


@functools.lru_cache(maxsize=None)
def probe_scene(offset=(0.0, 0.0, 0.0)):
    """The room with one origin per (cluster, axis, side) of its inflated boxes: that coordinate exactly on the plane, the
    other two at lo + (0.37, 0.61, 0.43)(hi - lo) of the same box; own = F + 5 (no face).  The direction list is the
    room's, so the rays parallel to the plane form 0 * inf in the slab test."""
    sc = dict(room_scene(offset))
    lo, hi, valid = cluster_boxes(sc["verts"], sc["faces"])
    assert valid.all()
    pts = []
    for c in range(len(lo)):
        inside = (lo[c] + PROBE_FRACTIONS * (hi[c] - lo[c])).astype(np.float32)
        for x in range(3):
            for plane in (lo[c, x], hi[c, x]):
                p = inside.copy()
                p[x] = plane
                pts.append(p)
    sc["origins"] = np.array(pts, np.float32)
    sc["own"] = np.full(len(pts), ROOM_F + PROBE_OWN_PAST_F, np.int64)
    return sc


@functools.lru_cache(maxsize=None)
def probe_case(offset=(0.0, 0.0, 0.0)):
    sc = probe_scene(offset)
    return (sc,) + _ref(sc)


# ------------------------------------------------------------------------------------------------------ E. t_min = 0
TMIN0_KEY = (130, 33, 129)


@functools.lru_cache(maxsize=None)
def tmin0_case():
    """The soup (130, 33, 129) with t_min = 0: the own face's t is a rounding error round 0, positive for about half the
    rays, and only the id comparison keeps it from occluding them."""
    sc = dict(VR.soup_scene(*TMIN0_KEY))
    sc["t_min"] = 0.0
    return (sc,) + _ref(sc)


# ------------------------------------------------------------------------------------------------ F. records with holes
HOLES_NP, HOLES_J = 17, 257
HOLES_KINDS = ("empty_cluster", "bad_order", "own_ids", "one_bad_face", "all_background", "never_prepared")
BAD_ORDER_SLOTS = {3: -1, 70: 130, 100: 1 << 40, 10: 11}  # slot -> entry: three outside [0, F), and face 11 named twice
OWN_PAST_INT32 = (1 << 31) + 1
OWN_WRAPS_TO_A_FACE = (1 << 32) + 7  # (its low 32 bits are face 7)


def _soup_with_rays(F, NP, J, seed, spoil=None, off_faces=False):
    """VR.soup(F) with ``spoil`` applied to its faces, and rays as VR.soup_scene makes them (origins on valid faces, one row
    in eight background); ``off_faces``: origins uniform in [-0.8, 0.8]^3 instead, every row foreground"""
    rng = np.random.default_rng([seed, F, NP, J])
    verts, faces = VR.soup(rng, F)
    if spoil is not None:
        spoil(faces, len(verts))
    V = len(verts)
    valid = np.flatnonzero(np.all((faces >= 0) & (faces < V), axis=1) & (faces[:, 1] != faces[:, 2]))
    if off_faces or len(valid) == 0:
        origins = rng.uniform(-0.8, 0.8, (NP, 3)).astype(np.float32)
        own = np.zeros(NP, np.int64)
    else:
        own = rng.choice(valid, NP)
        w = rng.dirichlet(np.ones(3), NP)
        origins = np.einsum("pk,pkd->pd", w, verts.astype(np.float64)[faces[own]]).astype(np.float32)
        bg = rng.random(NP) < 0.125
        own = np.where(bg, -1, own)
        origins[bg] = 0.0
    return dict(verts=verts, faces=faces, origins=origins, own=own.astype(np.int64), dirs=VR.unit_dirs(rng, J),
                t_min=1e-4 * VR.bbox_diag(verts))


@functools.lru_cache(maxsize=None)
def holes_case(kind):
    """-> (scene, occluded, decided).  The scene's extra keys: ``order`` (int64 [F], or None: the given order) for the
    record, ``prepare`` (False: the record is a zero-filled buffer the library never saw).  The reference sees the faces
    the record can hold: a face no slot names is given a bad index."""
    order, prepare, ref_faces = None, True, None
    if kind == "empty_cluster":      # faces 64 .. 127 all carry an index outside [0, V): cluster 1 has no valid face
        def spoil(faces, V):
            faces[np.arange(64, 128), np.arange(64) % 3] = np.resize([-1, V, V + 7, -(1 << 40)], 64)
        sc = _soup_with_rays(130, HOLES_NP, HOLES_J, 11, spoil)
        assert not np.all((sc["faces"][64:128] >= 0) & (sc["faces"][64:128] < len(sc["verts"])), axis=1).any()
    elif kind == "bad_order":
        sc = _soup_with_rays(130, HOLES_NP, HOLES_J, 12)
        order = np.arange(130, dtype=np.int64)
        for k, f in BAD_ORDER_SLOTS.items():
            order[k] = f
        named = np.isin(np.arange(130), order)
        assert (~named).sum() == 4
        ref_faces = np.where(named[:, None], sc["faces"], -1)
    elif kind == "own_ids":          # none of these is the id of a face the record holds: nothing is excluded
        sc = _soup_with_rays(130, HOLES_NP, HOLES_J, 13, off_faces=True)
        V = len(sc["verts"])
        bad = np.flatnonzero(~np.all((sc["faces"] >= 0) & (sc["faces"] < V), axis=1))
        assert len(bad) >= 1
        ids = [130 + 5, OWN_PAST_INT32, int(bad[0]), OWN_WRAPS_TO_A_FACE]
        sc["own"] = np.resize(np.array(ids, np.int64), HOLES_NP)
    elif kind == "one_bad_face":
        sc = _soup_with_rays(1, HOLES_NP, HOLES_J, 14)
        sc["faces"][0, 1] = 3
        sc["own"] = np.where(np.arange(HOLES_NP) % 4 == 3, -1, 0).astype(np.int64)
    elif kind == "all_background":
        sc = _soup_with_rays(130, 3, HOLES_J, 15)
        sc["own"] = np.full(3, -1, np.int64)
    elif kind == "never_prepared":   # the reference is the empty mesh: every face given a bad index
        sc = _soup_with_rays(130, HOLES_NP, HOLES_J, 16)
        prepare = False
        ref_faces = np.full_like(sc["faces"], -1)
    else:
        raise ValueError(kind)
    sc["order"], sc["prepare"] = order, prepare
    return (sc,) + _ref(sc, faces=ref_faces)


# ----------------------------------------------------------------------------------------------------- G. Python layer
SPHERE_S, SPHERE_W = 16, 32
SPHERE_VIEW = (2.7, 10.0, 25.0)  # look_at_view_transform(dist, elev, azim)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """tests.util.uv_sphere() rasterised at 16 x 16 by the float64 restatement of the rasteriser, under the 16 x 32 grid
    (J = 512): the CPU's stand-in for the G-buffer the GPU test takes from the device"""
    from reni_amd.mesh import look_at_view_transform
    from tests.test_raster_cpu import np_rasterize, np_vertex_normals
    from tests.util import uv_sphere
    v, f, _, _ = uv_sphere()
    verts, faces = v.numpy(), f.numpy()
    R, T = look_at_view_transform(*SPHERE_VIEW)
    r = np_rasterize(verts, faces, np_vertex_normals(verts, faces), R[0].double().numpy(), T[0].double().numpy(), SPHERE_S)
    return dict(verts=verts, faces=faces, origins=r["positions"].astype(np.float32),
                own=r["pix_to_face"].reshape(-1).astype(np.int64), dirs=VR.grid_dirs(SPHERE_W), t_min=1e-4 * VR.bbox_diag(verts))


@functools.lru_cache(maxsize=None)
def sphere_case():
    sc = sphere_scene()
    return (sc,) + _ref(sc)


def shares(occ, dec, own):
    """(rays, undecided, share of undecided rays, share of the foreground rays that are occluded)"""
    fg = np.asarray(own) >= 0
    return occ.size, int((~dec).sum()), float(1.0 - dec.mean()), float(occ[fg].mean()) if fg.any() else 0.0
