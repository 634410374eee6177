"""What ops.launch_count() rises by for one call of each utility entry point (the twelve units behind reni_tu_host.inc), at
the smallest shapes they accept.  The counter does not count every launch (DESIGN 4.4i has the table and why): shade, raster,
baselines, diffuse, resample and rotate count nothing, and in the glossy unit only the denominators do.  The numbers were
read from the code as it stood before the units shared one host path, and confirmed by running this test on that library
(profiles/tu_host_refactor.md); the image calls stay pinned in tests/test_gpu_image.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

B, H, W = 2, 8, 16          # 2 maps of 8 x 16
P, S = 64, 16               # directions, samples
KINDS, PARAMS = ("phong", "blinn", "ggx"), (8.0, 16.0, 0.5)   # three lobes, one of each kind
PRESENT = len(set(KINDS))


def _unit(g, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1).to(DEV)


def test_launch_count_increment_of_every_utility_entry_point():
    from reni_amd import ops
    g = torch.Generator().manual_seed(0)
    rose = {}

    def call(name, fn, *args, **kw):
        before = ops.launch_count()
        out = fn(*args, **kw)
        rose[name] = ops.launch_count() - before
        return out

    # ---- metrics, lights
    pred = torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.rand(B, 3, H, W, generator=g).to(DEV)
    call("pair_stats", ops.pair_stats, pred, target)
    call("ssim", ops.ssim, pred, target)
    maps = torch.rand(B, H, W, 3, generator=g).to(DEV)
    pmf, cond, marg = call("light_table_build", ops.light_table_build, maps, space="stored")
    u = torch.rand(S, 2, generator=g).to(DEV)
    _, ldirs, _, _, lcol = call("light_sample", ops.light_sample, pmf, cond, marg, maps, u, space="stored")
    normals = _unit(g, P)
    call("lights_irradiance", ops.lights_irradiance, normals, ldirs, lcol, 1.0)

    # ---- a four-face mesh at 16 x 16: raster, visibility, the four shader calls
    verts = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]).to(DEV) * 0.5
    faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=torch.int64).to(DEV)
    vn = call("vertex_normals", ops.vertex_normals, verts, faces)
    p2f, _, _, _, pnrm, ppos = call("rasterize_mesh", ops.rasterize_mesh, verts, faces, vn, torch.eye(3), torch.tensor([0.0, 0.0, 3.0]), 16)
    accel = call("mesh_visibility_prepare", ops.mesh_visibility_prepare, verts, faces)
    sdirs = _unit(g, P)
    vis = call("mesh_visibility", ops.mesh_visibility, ppos, p2f, sdirs, accel, 1e-3)
    NP = ppos.shape[0]
    cam = torch.tensor([0.0, 0.0, 3.0])
    colors = torch.rand(B, P, 3, generator=g).to(DEV)
    dcol = torch.rand(B, NP, 3, generator=g).to(DEV)
    call("envmap_shade", ops.envmap_shade, pnrm, ppos, cam, sdirs, colors, 50.0, 0.5, 0.5)
    call("envmap_shade_backward", ops.envmap_shade_backward, pnrm, ppos, cam, sdirs, dcol, 50.0, 0.5, 0.5)
    call("envmap_shade_masked", ops.envmap_shade, pnrm, ppos, cam, sdirs, colors, 50.0, 0.5, 0.5, vis=vis)
    call("envmap_shade_masked_backward", ops.envmap_shade_backward, pnrm, ppos, cam, sdirs, dcol, 50.0, 0.5, 0.5, vis=vis)

    # ---- baselines, diffuse
    K = 4
    raw = torch.randn(B, K, 6, generator=g).to(DEV) * 0.1
    tc, pc = torch.rand(K, generator=g).to(DEV), torch.rand(K, generator=g).to(DEV)
    call("sg_render", ops.sg_render, raw, tc, pc, 0.5, 0.5, H, W)
    call("sg_loss_grad", ops.sg_loss_grad, raw, tc, pc, 0.5, 0.5, torch.rand(B, 3, H, W, generator=g).to(DEV),
         torch.ones(1, 1, H, 1, device=DEV))
    lmax = 2
    T = (lmax + 1) ** 2
    row_t, col_t = torch.rand(H, T, generator=g).to(DEV), torch.rand(W, T, generator=g).to(DEV)
    coeffs = call("sh_project", ops.sh_project, maps, row_t, col_t, lmax)
    call("sh_reconstruct", ops.sh_reconstruct, coeffs, row_t, col_t, H, W, lmax)
    Q = H * W
    in_dirs, in_w, out_dirs = _unit(g, Q), torch.rand(Q, generator=g).to(DEV), _unit(g, P)
    src = maps.reshape(B, Q, 3)
    call("diffuse_convolve", ops.diffuse_convolve, src, in_dirs, in_w, out_dirs, 1.0)
    call("sh_irradiance_l2", ops.sh_irradiance_l2, coeffs, normals)

    # ---- glossy and its backward
    call("lobe_convolve", ops.lobe_convolve, src, in_dirs, in_w, out_dirs, KINDS, PARAMS)
    den = call("lobe_denominators", ops.lobe_denominators, in_dirs, in_w, out_dirs, KINDS, PARAMS)
    gout = torch.rand(B, len(KINDS), P, 3, generator=g).to(DEV)
    call("lobe_convolve_backward", ops.lobe_convolve_backward, gout, in_dirs, in_w, out_dirs, KINDS, PARAMS, den=den)
    call("envmap_lookup", ops.envmap_lookup, maps, out_dirs)
    table = call("envmap_lookup_taps", ops.envmap_lookup_table, B, 1, H, W, out_dirs)
    call("envmap_lookup_backward", ops.envmap_lookup_backward, torch.rand(B, P, 3, generator=g).to(DEV), 1, H, W, table=table)

    # ---- resample, blur, rotate
    call("resample", ops.resample, pred, (4, 8))
    call("gaussian_blur", ops.gaussian_blur, pred[0], 1.0)
    call("rotate_envmap", ops.rotate_envmap, pred, torch.eye(3, device=DEV))
    torch.cuda.synchronize()

    want = {
        "pair_stats": 2, "ssim": 2, "light_table_build": 3, "light_sample": 1, "lights_irradiance": 1,
        "mesh_visibility_prepare": 1, "mesh_visibility": 1,
        "lobe_denominators": PRESENT + 1, "lobe_convolve_backward": PRESENT + 2,
        "envmap_lookup_taps": 1, "envmap_lookup_backward": 1,
        "envmap_shade": 0, "envmap_shade_backward": 0, "envmap_shade_masked": 0, "envmap_shade_masked_backward": 0,
        "vertex_normals": 0, "rasterize_mesh": 0, "sg_render": 0, "sg_loss_grad": 0, "sh_project": 0, "sh_reconstruct": 0,
        "diffuse_convolve": 0, "sh_irradiance_l2": 0, "lobe_convolve": 0, "envmap_lookup": 0,
        "resample": 0, "gaussian_blur": 0, "rotate_envmap": 0,
    }
    print(rose)
    assert rose == want
