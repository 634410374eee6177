"""GPU tests of the mesh pipeline (reni_tu_raster.hip, reni_amd.mesh) against the float64 numpy restatement in
tests/test_raster_cpu.py or an analytic result, and FIT_INVERSE run end to end from a config without set_renderer()."""
import math

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from tests.test_raster_cpu import TEAPOT, np_rasterize, np_vertex_normals

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _close(a, b, tol):
    """True when every |a - b| <= tol * max(1, |b|); reports the worst element otherwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))
    if not ok.all():
        i = np.unravel_index(np.argmax(np.abs(a - b) / (tol * np.maximum(1.0, np.abs(b)))), a.shape)
        print(f"worst: {a[i]} vs {b[i]} (tolerance {np.broadcast_to(tol, a.shape)[i]:.3g})")
    return bool(ok.all())


def _soup(rng, F):
    """F random triangles round the origin seen from a random camera at distance 2: overlapping, both windings, ~6 % with
    one vertex behind the camera (view z in [-0.8, -0.1]: never 0), ~3 % with an index outside [0, V)."""
    from reni_amd.mesh import FoVPerspectiveCameras, look_at_view_transform
    R, T = look_at_view_transform(2.0, float(rng.uniform(-40, 40)), float(rng.uniform(-180, 180)))
    C = FoVPerspectiveCameras().get_camera_center(R, T)[0].double().numpy()
    axis = -C / np.linalg.norm(C)
    centres = rng.uniform(-0.8, 0.8, (F, 1, 3))
    verts = centres + rng.normal(0.0, 1.0, (F, 3, 3)) * rng.uniform(0.03, 0.35, (F, 1, 1))
    behind = rng.random(F) < 0.06
    zv = rng.uniform(-0.8, -0.1, F)
    vz = verts @ axis + 2.0  # view depth (the camera looks along axis from distance 2)
    verts += axis * np.maximum(0.25 - vz, 0.0)[..., None]  # every other vertex at least 0.25 in front of the camera
    lat = rng.normal(0.0, 0.1, (int(behind.sum()), 3))
    lat -= (lat @ axis)[:, None] * axis  # sideways only: the depth stays zv
    verts[behind, 0] = C + axis * zv[behind, None] + lat
    verts = verts.reshape(-1, 3).astype(np.float32)
    # pin the behind-camera vertices' view depth away from 0 after the float32 rounding
    vz = verts.astype(np.float64) @ R[0].double().numpy()[:, 2] + float(T[0, 2])
    assert np.all(np.abs(vz) > 0.05)
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    bad = rng.random(F) < 0.03
    faces[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([-1, 3 * F, 3 * F + 7], int(bad.sum()))
    return verts, faces, R, T


def _gpu_raster(verts, faces, R, T, S):
    from reni_amd import ops
    v = torch.from_numpy(np.asarray(verts, np.float32)).to(DEV)
    f = torch.from_numpy(np.asarray(faces, np.int64)).to(DEV)
    vn = ops.vertex_normals(v, f)
    out = ops.rasterize_mesh(v, f, vn, R, T, S)
    return vn, [t.cpu() for t in out]


def _compare(verts, faces, R, T, S):
    """GPU fragments + G-buffer vs the numpy restatement; -> (numpy result, pixels compared)."""
    vn, (p2f, zbuf, bary, dists, nrm, pos) = _gpu_raster(verts, faces, R, T, S)
    ref = np_rasterize(verts, faces, np_vertex_normals(verts, faces), R[0].double().numpy(), T[0].double().numpy(), S,
                       tan_half=float(np.float32(math.tan(math.pi / 6))))
    assert p2f.shape == (1, S, S, 1) and bary.shape == (1, S, S, 1, 3) and nrm.shape == (S * S, 3)
    g = p2f[0, :, :, 0].numpy()
    amb = ref["amb"]
    bad = (g != ref["pix_to_face"]) & ~amb
    assert not bad.any(), f"pix_to_face differs at {np.argwhere(bad)[:5].tolist()}: gpu {g[bad][:5]} ref {ref['pix_to_face'][bad][:5]}"
    same = (g == ref["pix_to_face"])
    hit = same & (g >= 0)
    # 1e-5, widened on ill-conditioned faces (slivers, faces reaching behind the camera) to their fp32 error band
    wt = ref["wtol"][same]
    zsum = np.zeros((S, S))
    vsum = np.zeros(S * S)
    if hit.any():
        fi = np.asarray(faces)[ref["pix_to_face"][hit]]
        zv = np.asarray(verts, np.float64) @ R[0].double().numpy()[:, 2] + float(T[0, 2])
        zsum[hit] = np.abs(zv[fi]).sum(1)
        vsum[hit.reshape(-1)] = np.abs(np.asarray(verts, np.float64)[fi]).sum(axis=(1, 2))
    zs, vs = zsum[same], vsum[same.reshape(-1)]
    assert _close(zbuf[0, :, :, 0].numpy()[same], ref["zbuf"][same], np.maximum(1e-5, wt * zs))
    assert _close(bary[0, :, :, 0].numpy()[same], ref["bary"][same], np.maximum(1e-5, wt)[:, None])
    assert _close(dists[0, :, :, 0].numpy()[same], ref["dists"][same], 1e-5)
    sf = same.reshape(-1)
    assert _close(nrm.numpy()[sf], ref["normals"][sf], np.maximum(1e-5, 3 * wt)[:, None])
    assert _close(pos.numpy()[sf], ref["positions"][sf], np.maximum(1e-5, wt * vs)[:, None])
    bg = (g < 0).reshape(-1)
    assert (zbuf.reshape(-1)[bg] == -1).all() and (bary.reshape(-1, 3)[bg] == -1).all() and (dists.reshape(-1)[bg] == -1).all()
    assert (nrm[bg] == 0).all() and (pos[bg] == 0).all()
    return ref, int(hit.sum())


@pytest.mark.parametrize("F,S,seed", [(1, 16, 0), (7, 16, 1), (60, 64, 2), (400, 64, 3), (2000, 64, 4), (300, 129, 5),
                                      (2000, 129, 6)])
def test_triangle_soups_match_the_restatement(F, S, seed):
    rng = np.random.default_rng(seed)
    for _ in range(3):
        verts, faces, R, T = _soup(rng, F)
        ref, n = _compare(verts, faces, R, T, S)
        if F >= 60:
            assert n > S * S // 20 and ref["amb"].mean() < 0.05


def test_exact_depth_tie_goes_to_the_lower_face_index():
    """Identical triangles have bit-identical depths: the lower index wins everywhere (strict <, ascending scan), also
    across the kernel's 256-face chunks."""
    from reni_amd.mesh import look_at_view_transform
    R, T = look_at_view_transform(2.0, 0.0, 0.0)
    tri = np.array([[0.3, -0.3, 0.0], [-0.3, -0.2, 0.1], [0.0, 0.4, -0.1]], np.float32)
    other = tri + np.float32(5.0)  # off screen
    verts = np.concatenate([other] * 300 + [tri] * 3)
    faces = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
    faces[[7, 299, 300, 301, 302]] = faces[[300, 300, 301, 302, 300]]  # duplicates at 7, 299, 300, 301, 302 (chunk edges)
    _, (p2f, *_rest) = _gpu_raster(verts, faces, R, T, 64)
    cov = p2f.reshape(-1) >= 0
    assert cov.sum() > 100 and (p2f.reshape(-1)[cov] == 7).all()


def test_vertex_normals_match_and_are_deterministic():
    from reni_amd import ops
    from reni_amd.mesh import load_obj
    v, f = load_obj(TEAPOT)
    rng = np.random.default_rng(9)
    sv, sf, _, _ = _soup(rng, 500)
    # (the soup's slivers are ill-conditioned: an fp32 cross product of near-parallel edges is good to ~1e-5 there)
    for (verts, faces), tol in (((v.numpy(), f.numpy()), 1e-6), (_icosphere(3), 1e-6), ((sv, sf), 1e-5)):
        vd = torch.from_numpy(np.asarray(verts, np.float32)).to(DEV)
        fd = torch.from_numpy(np.asarray(faces, np.int64)).to(DEV)
        a, b = ops.vertex_normals(vd, fd), ops.vertex_normals(vd, fd)
        assert torch.equal(a, b)
        ref = np_vertex_normals(np.asarray(verts, np.float32), faces)
        np.testing.assert_allclose(a.cpu().numpy(), ref, atol=tol, rtol=0)


def _icosphere(levels, radius=0.5):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
         [9, 8, 1]]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


def test_analytic_sphere():
    from reni_amd.mesh import look_at_view_transform
    verts, faces = _icosphere(3)
    R, T = look_at_view_transform(2.0, 0.0, 0.0)
    S = 64
    _, (p2f, zbuf, bary, dists, nrm, pos) = _gpu_raster(verts, faces, R, T, S)
    r_disc = 0.5 / (math.sqrt(4 - 0.25) * math.tan(math.pi / 6))
    c = -1.0 + (2.0 * (S - 1 - np.arange(S)) + 1.0) / S
    rr = np.sqrt(c[None, :] ** 2 + c[:, None] ** 2)
    ring = np.abs(rr - r_disc) < 2.0 / S
    cov = p2f[0, :, :, 0].numpy() >= 0
    assert (cov == (rr < r_disc))[~ring].all()
    centre = (rr <= rr.min() + 1e-9).reshape(-1)
    assert centre.sum() == 4
    np.testing.assert_allclose(nrm.numpy()[centre], np.tile([0.0, 0.0, 1.0], (4, 1)), atol=3e-2)
    np.testing.assert_allclose(pos.numpy()[centre][:, 2], 0.5, atol=3e-3)
    # every pixel well inside the disc against the analytic sphere: the view ray through the pixel centre meets the sphere
    # (centre at view (0, 0, 2)) at depth t; world = (-x_view, y_view, 2 - z_view) for R = diag(-1, 1, -1), T = (0, 0, 2)
    inner = (rr < 0.8 * r_disc).reshape(-1)
    d = np.stack([np.broadcast_to(c[None, :], (S, S)) * math.tan(math.pi / 6),
                  np.broadcast_to(c[:, None], (S, S)) * math.tan(math.pi / 6), np.ones((S, S))], -1).reshape(-1, 3)
    dd, dc = (d * d).sum(1), d[:, 2] * 2.0
    t = (dc - np.sqrt(np.maximum(dc * dc - dd * (4.0 - 0.25), 0.0))) / dd
    pv = d * t[:, None]
    pw = np.stack([-pv[:, 0], pv[:, 1], 2.0 - pv[:, 2]], 1)
    # (the 1 280 flat faces lie up to 3e-3 inside the sphere along a ray; interpolated normals are within 1.1e-2 of its normal)
    np.testing.assert_allclose(zbuf[0, :, :, 0].numpy().reshape(-1)[inner], pv[inner, 2], atol=5e-3)
    np.testing.assert_allclose(pos.numpy()[inner], pw[inner], atol=5e-3)
    np.testing.assert_allclose(nrm.numpy()[inner], pw[inner] / 0.5, atol=2e-2)
    # and the whole view against the restatement
    _compare(verts, faces, R, T, S)


def _envmap(B, seed):
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    g = torch.Generator().manual_seed(seed)
    D, Sw = get_directions(32), get_sineweight(32)
    C = torch.rand(B, D.shape[1], 3, generator=g) * 4.0
    env = EnvironmentMap(environment_map=C.to(DEV), directions=D.expand(B, -1, -1).to(DEV), sineweight=Sw.to(DEV))
    return env, D, (C * Sw).double()


@pytest.mark.parametrize("kd", [1.0, 0.5])
def test_teapot_render_against_the_oracle(kd):
    from reni_amd.mesh import build_hip_renderer, load_obj
    renderer, R, T, mesh = build_hip_renderer(TEAPOT, 0, 64, kd, "cuda")
    env, D, Cw = _envmap(2, 3)
    col, normals = renderer(meshes_world=mesh, R=R, T=T, envmap=env)
    assert col.shape == (2, 64, 64, 3) and normals.shape == (2, 64, 64, 3)
    v, f = load_obj(TEAPOT)
    ref, n = _compare(v.numpy(), f.numpy(), R.cpu(), T.cpu(), 64)
    assert n > 400
    ok = ~ref["amb"].reshape(-1)
    refcol = O.blinn_phong_gbuffer(torch.from_numpy(ref["normals"]), torch.from_numpy(ref["positions"]), torch.zeros(3),
                                   D.expand(2, -1, -1), Cw, 500.0, kd, 1.0 - kd)
    err = (col.reshape(2, -1, 3).cpu().double() - refcol)[:, torch.from_numpy(ok)].abs().max()
    assert float(err) <= 2e-4 * float(refcol.abs().max())
    # a second build renders the same bits
    renderer2, R2, T2, mesh2 = build_hip_renderer(TEAPOT, 0, 64, kd, "cuda")
    col2, normals2 = renderer2(meshes_world=mesh2, R=R2, T=T2, envmap=env)
    assert torch.equal(col, col2) and torch.equal(normals, normals2)
    # the G-buffer is cached: a second call does not rasterise again and gives the same bits
    frag1 = renderer.rasterizer(mesh, R=R, T=T)
    frag2 = renderer.rasterizer(mesh, R=R, T=T)
    assert frag1 is frag2
    assert torch.equal(renderer(meshes_world=mesh, R=R, T=T, envmap=env)[0], col)


def test_teapot_rotation_equals_pre_rotated_vertices():
    from reni_amd.mesh import (FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, Meshes, RasterizationSettings,
                               build_hip_renderer, load_obj, rotate_axis_angle_y)
    renderer, R, T, mesh = build_hip_renderer(TEAPOT, 90, 64, 0.5, "cuda")
    v, f = load_obj(TEAPOT)
    m2 = Meshes(verts=[rotate_axis_angle_y(v, 90).to(DEV)], faces=[f.to(DEV)])
    r2 = HipMeshRenderer(MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=64)), kd=0.5)
    env, _, _ = _envmap(1, 5)
    a = renderer(meshes_world=mesh, R=R, T=T, envmap=env)[0]
    b = r2(meshes_world=m2, R=R, T=T, envmap=env)[0]
    assert torch.equal(a, b)
    c = build_hip_renderer(TEAPOT, 0, 64, 0.5, "cuda")
    a0 = c[0](meshes_world=c[3], R=c[1], T=c[2], envmap=env)[0]
    assert not torch.equal(a, a0)  # the rotation did something


def _inverse_cfg(obj_path, kd=1.0):
    from tests.test_gpu_workflows import _config, _task
    cfg = _config("VariationalAutoDecoder")
    cfg.RENI.FIT_INVERSE = _task(BATCH_SIZE=2, LR_START=1e-2, LR_END=1e-2, COSINE_SIMILARITY_WEIGHT=1e-4,
                                 OBJECT_PATH=obj_path, RENDER_RESOLUTION=32, KD_VALUE=kd)
    return cfg


def test_fit_inverse_end_to_end_from_the_config():
    """trainer.fit on FIT_INVERSE with no set_renderer(): on_fit_start builds the HIP renderer from the config; the loss
    falls; every step equals, bit for bit, the same step through GBufferRenderer on the rasteriser's G-buffer."""
    from reni_amd import trainer
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.envmap_shader import GBuffer, GBufferRenderer
    from reni_amd.lightning_module import RENI
    from reni_amd.mesh import HipMeshRenderer
    ds = SyntheticEnvMapDataset(4, 16, 32)
    torch.manual_seed(0)
    m = RENI(_inverse_cfg(TEAPOT), "FIT_INVERSE", dataset=ds)
    hist = trainer.fit(m, max_epochs=8, device=DEV)
    assert isinstance(m.renderer, HipMeshRenderer)
    assert m.gt_renders.shape == (4, 32, 32, 3)
    frag = m.renderer.rasterizer(**{k: m.render_kwargs[k] for k in ("meshes_world", "R", "T")})
    obj = (frag.pix_to_face[0, :, :, 0] >= 0)
    assert obj.sum() > 50 and (~obj).sum() > 50
    assert bool((m.gt_renders[:, obj].abs().sum(-1) > 0).all()) and float(m.gt_renders[:, ~obj].abs().max()) == 0.0
    assert hist[-1]["loss"] < hist[0]["loss"]

    # step-by-step equality with a stored G-buffer
    for kd in (1.0, 0.5):
        torch.manual_seed(1)
        a = RENI(_inverse_cfg(TEAPOT, kd), "FIT_INVERSE", dataset=ds)
        a.setup()
        a.on_fit_start()
        a.to(DEV)
        _, nrm, pos = a.renderer.rasterizer.gbuffer(a.render_kwargs["meshes_world"], a.render_kwargs["R"], a.render_kwargs["T"])
        b = RENI(_inverse_cfg(TEAPOT + ".not_read", kd), "FIT_INVERSE", dataset=ds)
        b.setup()
        b.to(DEV)
        with torch.no_grad():
            for pa, pb in zip(a.model.parameters(), b.model.parameters()):
                pb.copy_(pa)
        b.set_renderer(GBufferRenderer(GBuffer(nrm.clone(), pos.clone(), (0.0, 0.0, 0.0), 32), kd=kd))
        assert torch.equal(a.gt_renders, b.gt_renders)
        oa, ob = a.configure_optimizers()["optimizer"], b.configure_optimizers()["optimizer"]
        for step, idx in enumerate(([0, 1], [2, 3], [1, 2], [0, 3])):
            idx = torch.tensor(idx)
            imgs = torch.stack([ds[int(i)][0] for i in idx]).to(DEV)
            res = []
            for mod, opt in ((a, oa), (b, ob)):
                opt.zero_grad(set_to_none=True)
                out = mod.training_step((imgs, idx.to(DEV)), step)
                out["loss"].backward()
                res.append((out["loss"].detach().clone(), mod.model.mu.grad.clone()))
                opt.step()
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
            assert float(res[0][1][idx.to(DEV)].abs().max()) > 0


def test_set_renderer_by_hand_keeps_priority():
    """A renderer handed in before fit() is used (the config's OBJ path is never read) and survives fit()'s setup()."""
    from reni_amd import trainer
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.envmap_shader import GBuffer, GBufferRenderer
    from reni_amd.lightning_module import RENI
    ds = SyntheticEnvMapDataset(2, 16, 32)
    m = RENI(_inverse_cfg("/nonexistent/model.obj"), "FIT_INVERSE", dataset=ds)
    m.setup()
    g = torch.Generator().manual_seed(4)
    nrm, pos = torch.randn(16 * 16, 3, generator=g), torch.randn(16 * 16, 3, generator=g) * 0.3
    r = GBufferRenderer(GBuffer(nrm, pos, (0.0, 0.0, 2.0), 16), kd=1.0)
    m.set_renderer(r)
    trainer.fit(m, max_epochs=1, device=DEV)
    assert m.renderer is r and m.gt_renders.shape == (2, 16, 16, 3)


def test_errors():
    from reni_amd import _lib, ops
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.lightning_module import RENI
    from reni_amd.mesh import build_hip_renderer
    m = RENI(_inverse_cfg("/nonexistent/model.obj"), "FIT_INVERSE", dataset=SyntheticEnvMapDataset(2, 16, 32))
    m.setup()
    with pytest.raises(FileNotFoundError, match="OBJECT_PATH"):
        m.on_fit_start()
    with pytest.raises(_lib.RENILibraryError):
        build_hip_renderer(TEAPOT, 0, 32, 1.0, "cpu")
    v = torch.rand(3, 3, device=DEV)
    f = torch.tensor([[0, 1, 2]], device=DEV)
    with pytest.raises(_lib.RENILibraryError):
        ops.rasterize_mesh(v.cpu(), f.cpu(), v.cpu(), torch.eye(3), torch.zeros(3), 8)
    with pytest.raises(ValueError):
        ops.rasterize_mesh(v, f, v[:2], torch.eye(3), torch.zeros(3), 8)
    with pytest.raises(ValueError):
        ops.rasterize_mesh(v, f, v, torch.eye(2), torch.zeros(3), 8)
