"""Edge shapes of the mesh pipeline (reni_tu_raster.hip): image sizes around the 16 x 16 tile, face counts around the 256-face
chunk, chunks whose compaction list is full or fed by two of the four waves only, scenes with nothing to draw, a face much
larger than the screen, and the meshes of the vertex-normal cases.  The case lists, the deterministic scene builders and an
fp32 restatement of k_face_setup plus the per-pixel test, shared by tests/test_raster_edges_cpu.py and
tests/test_gpu_raster_edges.py.

Plain data on the CPU; nothing here touches a device.  The float64 references are np_rasterize and np_vertex_normals of
tests/test_raster_cpu.py; nothing of them is restated here."""
import functools

import numpy as np

from tests.test_raster_cpu import TAN30

AMB_CAP = 0.05  # largest share of pixels whose winner fp32 arithmetic may legitimately change (np_rasterize's "amb")
TANF = float(np.float32(TAN30))  # the tangent as the library is given it
SIZES = (1, 2, 3, 15, 16, 17, 31, 33)  # S: below a tile, one short of / exactly / one past a tile and two tiles
CARVED_SIZES = (1, 15, 17)
# seed of the 60-face soup at each S: the first seed from 0 whose soup keeps the ambiguous share within AMB_CAP (none at all
# at S <= 3, where one pixel is more than the cap) and covers at least one pixel
SOUP_SEEDS = {1: 1, 2: 0, 3: 0, 15: 0, 16: 0, 17: 0, 31: 0, 33: 0}
STACK_S = 16
STACK_F = (255, 256, 257, 512, 513)  # one short of a chunk, a chunk, one past; two chunks, one past
ORDERS = ("increasing", "decreasing")
DEPTH0, DEPTH_STEP = 1.5, 1e-3  # view depth of face 0 of a stack and the step to the next (ZREL of the restatement is 1e-6)
EMPTY_KINDS = ("behind", "degenerate", "bad_index", "off_screen")
NORMAL_STRIPS = (255, 256, 257)  # V: one short of a block of k_vertex_normals, a block, one past
FAN = 300


def camera():
    """look_at_view_transform(2.0, 0, 0): R = diag(-1, 1, -1), T = (0, 0, 2), as torch tensors [1, 3, 3], [1, 3]"""
    from reni_amd.mesh import look_at_view_transform
    return look_at_view_transform(2.0, 0.0, 0.0)


def world_from_ndc(ndc, zview):
    """world points that camera() sees at NDC (x, y) and view depth zview: view = (-x, y, 2 - z) of the world point"""
    ndc = np.asarray(ndc, np.float64)
    zview = np.broadcast_to(np.asarray(zview, np.float64), ndc.shape[:-1])
    return np.stack([-ndc[..., 0] * zview * TAN30, ndc[..., 1] * zview * TAN30, 2.0 - zview], -1)


def cover_triangle(i=0):
    """NDC corners of a triangle that holds the whole view [-1, 1]^2 with every edge at least 1.5 away from it; i makes each
    one slightly larger than the last, so no two of a stack share an edge"""
    e = 1e-3 * i
    return np.array([[-4.0 - e, -3.0 - e], [4.0 + e, -3.0 - e], [0.0, 5.0 + e]])


def _mesh(tris):
    """[F, 3, 3] world corners -> (verts float32 [3 F, 3], faces int64 [F, 3])"""
    tris = np.asarray(tris, np.float64)
    return tris.reshape(-1, 3).astype(np.float32), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)


def stack_depths(F, order):
    z = DEPTH0 + DEPTH_STEP * np.arange(F)
    return z if order == "increasing" else z[::-1].copy()


def gap_faces(F=512):
    """the faces of the empty-waves case that are moved off screen: (f mod 256) in [64, 128) or [192, 256), the faces waves 1
    and 3 of the workgroup test in each chunk"""
    m = np.arange(F) % 256
    return ((m >= 64) & (m < 128)) | (m >= 192)


@functools.lru_cache(maxsize=None)
def scene(kind, *args):
    """-> (verts float32 [V, 3], faces int64 [F, 3], R, T, S, winner): winner is the face every pixel must show (-1: the whole
    frame is background), or None where the restatement decides"""
    R, T = camera()
    if kind == "soup":  # 60 random triangles and their own random camera (tests/test_gpu_raster.py::_soup)
        from tests.test_gpu_raster import _soup
        (S,) = args
        verts, faces, R, T = _soup(np.random.default_rng(SOUP_SEEDS[S]), 60)
        return verts, faces, R, T, S, None
    if kind == "cover":  # one triangle over the whole view
        (S,) = args
        return _mesh([world_from_ndc(cover_triangle(), 1.7)]) + (R, T, S, 0)
    if kind in ("stack", "gaps"):  # F screen-filling triangles 1e-3 apart in depth: every chunk's list is full
        F, order = args if kind == "stack" else (512,) + args
        z = stack_depths(F, order)
        tris = np.stack([world_from_ndc(cover_triangle(i), z[i]) for i in range(F)])
        winner = int(np.argmin(z))
        if kind == "gaps":
            off = gap_faces(F)
            shifted = np.stack([world_from_ndc(cover_triangle(i) + [50.0, 0.0], z[i]) for i in range(F)])
            tris[off] = shifted[off]
            winner = int(np.argmin(np.where(off, np.inf, z)))
        return _mesh(tris) + (R, T, STACK_S, winner)
    if kind == "empty":
        (what,) = args
        n = 5
        tris = np.stack([world_from_ndc(cover_triangle(i) * 0.2, 1.5 + 0.1 * i) for i in range(n)])
        verts, faces = _mesh(tris)
        if what == "behind":
            verts, faces = _mesh(np.stack([world_from_ndc(cover_triangle(i) * 0.2, -0.5 - 0.1 * i) for i in range(n)]))
        elif what == "degenerate":  # a repeated corner, or three corners on a line
            tris[::2, 2] = tris[::2, 1]
            tris[1::2, 2] = 0.5 * (tris[1::2, 0] + tris[1::2, 1])
            verts, faces = _mesh(tris)
        elif what == "bad_index":
            faces = faces.copy()
            faces[np.arange(n), np.arange(n) % 3] = [-1, 3 * n, 3 * n + 7, -5, 2 ** 40]
        elif what == "off_screen":
            verts, faces = _mesh([world_from_ndc(cover_triangle() * 0.2 + [3.0, 0.0], 1.5)])
        else:
            raise ValueError(what)
        return verts, faces, R, T, STACK_S, -1
    if kind == "huge":  # the nearer of two triangles spans about 1e4 NDC units; the farther one is of ordinary size
        tris = np.stack([world_from_ndc(cover_triangle() * 0.2, 1.9), world_from_ndc(cover_triangle() * 2.5e3, 1.2)])
        return _mesh(tris) + (R, T, STACK_S, 1)
    raise ValueError(kind)


SCENES = (tuple(("soup", S) for S in SIZES) + tuple(("cover", S) for S in SIZES)
          + tuple(("stack", F, o) for F in STACK_F for o in ORDERS) + tuple(("gaps", o) for o in ORDERS)
          + tuple(("empty", k) for k in EMPTY_KINDS) + (("huge",),))


def scene_id(key):
    return "-".join(str(k) for k in key)


@functools.lru_cache(maxsize=None)
def reference(key):
    """np_rasterize of a scene with the float64 vertex normals: computed once, read-only"""
    from tests.test_raster_cpu import np_rasterize, np_vertex_normals
    verts, faces, R, T, S, _ = scene(*key)
    return np_rasterize(verts, faces, np_vertex_normals(verts, faces), R[0].double().numpy(), T[0].double().numpy(), S,
                        tan_half=TANF)


# ------------------------------------------------------------------------------------------------ fp32 restatement
def raster_fp32(verts, faces, R, T, S, tan_half=TANF):
    """pix_to_face [S, S] of k_face_setup and k_raster_tile's per-pixel test restated in fp32, every operation rounded once in
    the written order (no contraction): world -> view -> NDC, the signed area, the skip rules, then per pixel the box test,
    the three edge functions over A + 1e-8, w > 0, the depth, pz >= 0 and strict < in ascending face order."""
    f = np.float32
    verts, faces = np.asarray(verts, f), np.asarray(faces, np.int64)
    Rm, Tv, th = np.asarray(R, f).reshape(3, 3), np.asarray(T, f).reshape(3), f(tan_half)
    V, F = len(verts), len(faces)
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    p = verts[np.where(ok[:, None], faces, 0)]  # [F, 3 corners, 3]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        vx = px * Rm[0, 0] + py * Rm[1, 0] + pz * Rm[2, 0] + Tv[0]
        vy = px * Rm[0, 1] + py * Rm[1, 1] + pz * Rm[2, 1] + Tv[1]
        vz = px * Rm[0, 2] + py * Rm[1, 2] + pz * Rm[2, 2] + Tv[2]
        w = vz * th
        x, y, z = vx / w, vy / w, vz

        def edge(qx, qy, ax, ay, bx, by):
            return (qx - ax) * (by - ay) - (qy - ay) * (bx - ax)

        area = edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
        valid = ok & ~(z.max(axis=1) < 0) & ~(np.abs(area) <= f(1e-8))
        i = np.arange(S, dtype=f)
        c = (f(-1) + (f(2) * (f(S - 1) - i) + f(1)) / f(S)).astype(f)
        PX = np.broadcast_to(c[None, :], (S, S)).reshape(-1)[None, :]
        PY = np.broadcast_to(c[:, None], (S, S)).reshape(-1)[None, :]
        x0, y0, x1, y1, x2, y2 = (a[:, None] for a in (x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2]))
        inbox = ~((PX > x.max(axis=1)[:, None]) | (PX < x.min(axis=1)[:, None]) | (PY > y.max(axis=1)[:, None])
                  | (PY < y.min(axis=1)[:, None]))
        A = edge(x2, y2, x0, y0, x1, y1) + f(1e-8)
        w0 = edge(PX, PY, x1, y1, x2, y2) / A
        w1 = edge(PX, PY, x2, y2, x0, y0) / A
        w2 = edge(PX, PY, x0, y0, x1, y1) / A
        depth = w0 * z[:, 0, None] + w1 * z[:, 1, None] + w2 * z[:, 2, None]
        assert depth.dtype == f
        hit = valid[:, None] & inbox & (w0 > 0) & (w1 > 0) & (w2 > 0) & (depth >= 0)
    zc = np.where(hit, depth, np.inf)
    best = np.argmin(zc, axis=0)  # the first minimum: strict < in ascending order
    return np.where(np.isfinite(zc[best, np.arange(S * S)]), best, -1).reshape(S, S)


# ------------------------------------------------------------------------------------------------ vertex normals
def strip_mesh(V):
    """a zigzag strip of V - 2 well-shaped triangles (legs 0.1 .. 0.13, no angle below 40 degrees) that undulates in z"""
    i = np.arange(V)
    verts = np.stack([0.06 * i, 0.1 * (i % 2), 0.03 * np.sin(0.9 * i)], 1)
    a = np.arange(V - 2)
    faces = np.stack([a, np.where(a % 2 == 0, a + 1, a + 2), np.where(a % 2 == 0, a + 2, a + 1)], 1)
    return verts.astype(np.float32), faces.astype(np.int64)


@functools.lru_cache(maxsize=None)
def normals_mesh(kind, *args):
    """-> (verts float32, faces int64, tolerance, vertices whose normal is exactly 0)"""
    if kind == "strip":
        return strip_mesh(*args) + (1e-6, ())
    if kind == "unused_vertex":  # a vertex in the middle of the strip's list that belongs to no face
        v, f = strip_mesh(64)
        k = 30
        return np.insert(v, k, [[7.0, 7.0, 7.0]], axis=0), np.where(f >= k, f + 1, f), 1e-6, (k,)
    if kind == "fan":  # FAN faces round vertex 0, each with a 60 degree angle there: the ring vertex i and the one 50 further
        t = 2 * np.pi * np.arange(FAN) / FAN
        ring = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], 1)
        verts = np.concatenate([[[0.0, 0.0, 0.3]], ring])
        i = np.arange(FAN)
        faces = np.stack([np.zeros(FAN, np.int64), 1 + i, 1 + (i + FAN // 6) % FAN], 1)
        return verts.astype(np.float32), faces.astype(np.int64), 1e-6, ()
    if kind == "repeated_index":  # faces (i, i, j) add a zero vector: vertex 9 belongs to such faces only
        v, f = strip_mesh(9)
        v = np.concatenate([v, [[0.3, 0.5, 0.2]]]).astype(np.float32)
        f = np.concatenate([f, [[9, 9, 2], [3, 9, 3], [4, 4, 4]]])
        return v, f, 1e-6, (9,)
    if kind == "bad_index":  # faces with an index outside [0, V) add nothing, to any of their vertices
        v, f = strip_mesh(40)
        f = np.concatenate([f, [[0, 1, 40], [-1, 5, 6], [7, 2 ** 40, 8], [39, 38, 37]]])
        return v, f, 1e-6, ()
    raise ValueError(kind)


NORMAL_CASES = tuple(("strip", V) for V in NORMAL_STRIPS) + (("unused_vertex",), ("fan",), ("repeated_index",), ("bad_index",))


def vertex_normals_fp32(verts, faces):
    """k_vertex_normals restated in fp32: each vertex adds cross(v1 - v0, v2 - v0) of its faces in ascending face order (a
    face twice where it names the vertex twice, as the corner list has it), then v / max(|v|, 1e-6)"""
    f = np.float32
    verts, faces = np.asarray(verts, f), np.asarray(faces, np.int64)
    V = len(verts)
    n = np.zeros((V, 3), f)
    for face in faces:
        if not np.all((face >= 0) & (face < V)):
            continue
        a, b = verts[face[1]] - verts[face[0]], verts[face[2]] - verts[face[0]]
        cr = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f)
        for k in range(3):
            n[face[k]] = n[face[k]] + cr
    length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    return n * (f(1) / np.maximum(length, f(1e-6)))[:, None]
