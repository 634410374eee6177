"""Float64 numpy restatement of the visibility definition of include/reni_hip.h ("cast shadows"), the margin that says which
rays fp32 arithmetic may legitimately decide the other way, and the scenes the CPU and GPU tests share.

Per (ray, face), with o the origin, d the direction and v0, v1, v2 the face (two-sided, no culling):

    e1 = v1 - v0, e2 = v2 - v0, h = d x e2, a = e1 . h;      |a| <= 1e-12: miss
    s = o - v0, u = (s . h) / a, q = s x e1, v = (d . q) / a, t = (e2 . q) / a
    hit  <=>  f != own face  and  u >= 0  and  v >= 0  and  u + v <= 1  and  t > t_min

A ray is occluded iff some face hits.  The four conditions are c = (u, v, 1 - u - v, (t - t_min) / diag) >= 0 (the last one
strictly); K = max(1, |s| |e1| |e2| / |a|) is the pair's conditioning (u, v and t are quotients by a).  With
m = min |c_i| / K a pair's margin:

    decided occluded : some face hits with m >= MARGIN
    decided visible  : no face hits, and no face is a near miss -- one whose worst violated condition is violated by less
                       than MARGIN K (a perturbation of that size would make it a hit)
    undecided        : everything else; an implementation may answer either way

Faces that are absent -- an index outside [0, V), the ray's own face, |a| <= 1e-12 -- neither hit nor nearly miss.
"""
import functools
import os

import numpy as np

MARGIN = 1e-4
A_EPS = 1e-12
UNDECIDED_MAX = 0.02  # a condition on the scenes: at most this share of a case's rays may be undecided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")


def bbox_diag(verts):
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def visibility_ref(origins, own, dirs, verts, faces, t_min, dtype=np.float64, margin=MARGIN, chunk_rays=4096):
    """origins [NP,3], own [NP] (face id; < 0: a background pixel), dirs [J,3], verts [V,3], faces [F,3] ->
    (occluded [NP,J] bool, decided [NP,J] bool).  Background rows come back occluded = True (their mask bits are 0) and
    decided.  ``dtype=np.float32`` evaluates the same formulas in single precision (``decided`` is then meaningless)."""
    verts = np.asarray(verts, dtype)
    faces = np.asarray(faces, np.int64)
    origins, dirs = np.asarray(origins, dtype), np.asarray(dirs, dtype)
    own = np.asarray(own, np.int64).reshape(-1)
    V, F = len(verts), len(faces)
    NP, J = len(origins), len(dirs)
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    fs = np.where(ok[:, None], faces, 0)
    v0 = verts[fs[:, 0]]
    e1, e2 = verts[fs[:, 1]] - v0, verts[fs[:, 2]] - v0
    diag = dtype(bbox_diag(verts)) if V else dtype(1)
    diag = diag if diag > 0 else dtype(1)
    ne = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    occluded = np.zeros((NP, J), bool)
    decided = np.ones((NP, J), bool)
    t_min = dtype(t_min)
    fid = np.arange(F)
    step = max(1, chunk_rays // max(J, 1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fg = np.flatnonzero(own >= 0)  # (background rows are never evaluated)
        for k0 in range(0, len(fg), step):
            rows = fg[k0:k0 + step]
            o = origins[rows]                                            # [n,3]
            s = o[:, None, :] - v0[None]                                 # [n,F,3]
            q = np.cross(s, e1[None])                                    # [n,F,3]
            tq = np.einsum("fk,nfk->nf", e2, q)                          # [n,F]
            h = np.cross(dirs[:, None, :], e2[None])                     # [J,F,3]
            a = np.einsum("fk,jfk->jf", e1, h)                           # [J,F]
            u = np.einsum("nfk,jfk->njf", s, h) / a[None]                # [n,J,F]
            v = np.einsum("jk,nfk->njf", dirs, q) / a[None]
            t = tq[:, None, :] / a[None]
            present = ok[None, None, :] & (np.abs(a) > A_EPS)[None] & (fid[None, None, :] != own[rows, None, None])
            hit = present & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min)
            occ = hit.any(axis=2)
            if dtype is np.float64:
                w, tt = 1 - u - v, (t - t_min) / diag                    # c = (u, v, w, tt) >= 0
                K = np.maximum(1.0, np.linalg.norm(s, axis=2)[:, None, :] * ne[None, None, :] / np.abs(a)[None])
                cmin = np.minimum(np.minimum(u, v), np.minimum(w, tt))
                m = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.minimum(np.abs(w), np.abs(tt))) / K
                sure_hit = (hit & (m >= margin)).any(axis=2)
                near = present & ~hit & (cmin > -margin * K)
                sure_clear = ~occ & ~near.any(axis=2)
                decided[rows] = sure_hit | sure_clear
            occluded[rows] = occ
    bg = own < 0
    occluded[bg] = True
    decided[bg] = True
    return occluded, decided


def pack_bits(visible):
    """bool [..., J] -> int32 words [..., ceil(J/32)]: bit j & 31 of word j >> 5 (numpy's packbits, little bit order)."""
    visible = np.asarray(visible, bool)
    J = visible.shape[-1]
    pad = (-J) % 32
    b = np.concatenate([visible, np.zeros(visible.shape[:-1] + (pad,), bool)], axis=-1)
    by = np.packbits(b, axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view("<u4").astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------- scenes
def soup(rng, F):
    """F random triangles round the origin, as tests/test_gpu_raster.py's _soup builds them (centres in [-0.8, 0.8]^3, sizes
    0.03 .. 0.35, overlapping, both windings) with ~3 % of the faces carrying an index outside [0, V) and ~3 % degenerate
    (a repeated vertex); float32 vertices."""
    centres = rng.uniform(-0.8, 0.8, (F, 1, 3))
    verts = centres + rng.normal(0.0, 1.0, (F, 3, 3)) * rng.uniform(0.03, 0.35, (F, 1, 1))
    verts = verts.reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    if F > 1:
        bad = rng.random(F) < 0.03
        faces[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([-1, 3 * F, 3 * F + 7], int(bad.sum()))
        deg = (rng.random(F) < 0.03) & ~bad
        faces[deg, 2] = faces[deg, 1]
    return verts, faces


def unit_dirs(rng, J):
    d = rng.normal(0.0, 1.0, (J, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def soup_scene(F, NP, J, seed=1):
    """-> dict(verts, faces, origins [NP,3] float32, own [NP] int64, dirs [J,3] float32, t_min): the origins lie on valid
    faces of the soup (a random barycentric point of a random face, which is the pixel's own); about one row in eight is a
    background pixel (own = -1, origin 0) when NP > 1."""
    rng = np.random.default_rng([seed, F, NP, J])  # (seed 1: every case of SOUP_CASES meets UNDECIDED_MAX, checked on the CPU)
    verts, faces = soup(rng, F)
    V = len(verts)
    valid = np.flatnonzero(np.all((faces >= 0) & (faces < V), axis=1) & (faces[:, 1] != faces[:, 2]))
    own = rng.choice(valid, NP)
    w = rng.dirichlet(np.ones(3), NP)
    origins = np.einsum("pk,pkd->pd", w, verts.astype(np.float64)[faces[own]]).astype(np.float32)
    if NP > 1:
        bg = rng.random(NP) < 0.125
        own = np.where(bg, -1, own)
        origins[bg] = 0.0
    return dict(verts=verts, faces=faces, origins=origins, own=own.astype(np.int64), dirs=unit_dirs(rng, J),
                t_min=1e-4 * bbox_diag(verts))


def grid_dirs(W):
    """The W/2 x W equirectangular grid of the package (reni_amd.utils.get_directions) as float32 [H W, 3]."""
    from reni_amd.utils import get_directions
    return get_directions(W)[0].numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def teapot_scene(S=32, W=16):
    """The teapot fixture rasterised at S x S by the float64 restatement of the rasteriser (tests/test_raster_cpu.py) from
    the default camera of build_hip_renderer, and the W/2 x W grid: the same keys as ``soup_scene`` plus normals."""
    from reni_amd.mesh import load_obj, look_at_view_transform
    from tests.test_raster_cpu import np_rasterize, np_vertex_normals
    v, f = load_obj(TEAPOT)
    verts, faces = v.numpy(), f.numpy()
    R, T = look_at_view_transform(2.0, 0.0, 0.0)
    r = np_rasterize(verts, faces, np_vertex_normals(verts, faces), R[0].double().numpy(), T[0].double().numpy(), S)
    return dict(verts=verts, faces=faces, origins=r["positions"].astype(np.float32), own=r["pix_to_face"].reshape(-1).astype(np.int64),
                normals=r["normals"].astype(np.float32), dirs=grid_dirs(W), t_min=1e-4 * bbox_diag(verts))


SOUP_CASES = [(F, NP, J) for F in (1, 63, 64, 65, 130) for NP in (1, 255, 257) for J in (1, 31, 32, 33, 129)]


@functools.lru_cache(maxsize=None)
def soup_case(F, NP, J):
    """The scene of one (F, NP, J) case and its float64 reference, computed once per process: (scene, occluded, decided)."""
    sc = soup_scene(F, NP, J)
    occ, dec = visibility_ref(sc["origins"], sc["own"], sc["dirs"], sc["verts"], sc["faces"], sc["t_min"])
    occ.setflags(write=False); dec.setflags(write=False)
    return sc, occ, dec


@functools.lru_cache(maxsize=None)
def teapot_case(S=32, W=16):
    sc = teapot_scene(S, W)
    occ, dec = visibility_ref(sc["origins"], sc["own"], sc["dirs"], sc["verts"], sc["faces"], sc["t_min"])
    occ.setflags(write=False); dec.setflags(write=False)
    return sc, occ, dec
