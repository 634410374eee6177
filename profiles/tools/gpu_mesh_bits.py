"""Diagnostic: the raw bits of every output of the mesh family's entry points (ops.vertex_normals, rasterize_mesh,
vertex_normals_backward, gbuffer_backward, mesh_pixel_uv), for comparing two builds of the library.

  RENI_HIP_LIB=<library A> python profiles/tools/gpu_mesh_bits.py run a.npz      (one process per library)
  RENI_HIP_LIB=<library B> python profiles/tools/gpu_mesh_bits.py run b.npz
  python profiles/tools/gpu_mesh_bits.py compare a.npz b.npz                     (no GPU: numpy.array_equal on the raw words)

Inputs: the tests' own catalogues -- raster_edge_cases.SCENES and NORMAL_CASES, gbuffer_grad_ref.CASES x VARIANTS, the malformed
tables of test_gpu_gbuffer_grad.py::test_malformed_tables_add_nothing, and tests.util.uv_sphere (whole and with texture
coordinates missing) at S = 1, 15, 17, 33 for mesh_pixel_uv."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np


def run(path):
    import torch
    from reni_amd import ops
    from reni_amd.mesh import look_at_view_transform
    from tests import gbuffer_grad_ref as G
    from tests import raster_edge_cases as E
    from tests.util import uv_sphere
    dev = torch.device("cuda:0")
    out = {}

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            a = t.detach().cpu().contiguous().numpy()
            out[f"{key}/{i}"] = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)

    for key in E.SCENES:
        v, f, R, T, S, _ = E.scene(*key)
        v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        vn = ops.vertex_normals(v, f)
        put(f"scene/{E.scene_id(key)}", vn, *ops.rasterize_mesh(v, f, vn, R, T, S, E.TANF))
    for key in E.NORMAL_CASES:
        v, f = E.normals_mesh(*key)[:2]
        v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        put(f"normals/{E.scene_id(key)}", ops.vertex_normals(v, f))
        gn = torch.randn(v.shape, generator=torch.Generator().manual_seed(7)).to(dev)
        put(f"normals_bwd/{E.scene_id(key)}", ops.vertex_normals_backward(v, f, gn))

    def rastered(key):
        v, f, R, T, S = G.case(*key)
        v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        vn = ops.vertex_normals(v, f)
        return v, f, vn, R, T, S, ops.rasterize_mesh(v, f, vn, R, T, S, E.TANF)

    def to_dev(g):
        return None if g is None else g.float().to(dev)

    for key in G.CASES:
        v, f, vn, R, T, S, frag = rastered(key)
        put(f"grad/{G.case_id(key)}/forward", vn, *frag)
        put(f"grad/{G.case_id(key)}/normals_bwd", ops.vertex_normals_backward(v, f, G.normals_upstream(key).float().to(dev)))
        for variant in G.VARIANTS:
            gN, gX = (to_dev(g) for g in G.upstream(key, variant))
            put(f"grad/{G.case_id(key)}/{variant}", ops.gbuffer_backward(v, f, vn, R, T, S, frag[0], gN, gX, tan_half_fov=E.TANF))

    key = ("ico", 17)  # the malformed tables
    v, f, vn, R, T, S, frag = rastered(key)
    p2f, F = frag[0], f.shape[0]
    gN, gX = (to_dev(g) for g in G.upstream(key, "both"))
    off, lst = ops.face_pixel_table(p2f, F)
    dropped = lst[int(off[0])::3]
    p2f_kept, p2f_bad, bad_list, off_wide = p2f.reshape(-1).clone(), p2f.reshape(-1).clone(), lst.clone(), off.clone()
    p2f_kept[dropped] = -1
    bad_list[int(off[0])::3] = torch.tensor([-1, S * S, 2 ** 40], device=dev).repeat(dropped.numel() // 3 + 1)[:dropped.numel()]
    p2f_bad[dropped] = torch.tensor([F, F + 3, -7], device=dev).repeat(dropped.numel() // 3 + 1)[:dropped.numel()]
    off_wide[0], off_wide[F] = -5, S * S + 7
    for name, p, table in (("kept", p2f_kept, (off, lst)), ("bad_list", p2f, (off, bad_list)), ("bad_p2f", p2f_bad, (off, lst)),
                           ("wide_offsets", p2f, (off_wide, lst))):
        put(f"malformed/{name}", ops.gbuffer_backward(v, f, vn, R, T, S, p, gN, gX, tan_half_fov=E.TANF, table=table))

    R, T = look_at_view_transform(2.7, 20.0, 35.0, device=dev)
    for which in ("sphere", "sphere_missing"):
        v, f, vt, ft = uv_sphere()
        if which == "sphere_missing":  # as test_gpu_texture.py: every third face loses a coordinate, one keeps an index past Tn
            ft = ft.clone()
            ft[::3, 1] = -1
            ft[1, 2] = vt.shape[0]
        v, f, vt, ft = (t.to(dev) for t in (v, f, vt, ft))
        vn = ops.vertex_normals(v, f)
        for S in (1, 15, 17, 33):
            frag = ops.rasterize_mesh(v, f, vn, R, T, S)
            put(f"uv/{which}/{S}", *frag, *ops.mesh_pixel_uv(v, f, vt, ft, R, T, S, frag[0], frag[2]))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path} (library {os.environ.get('RENI_HIP_LIB', 'in-tree')})")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two files hold different arrays"
    differ = [k for k in a.files if not np.array_equal(a[k], b[k])]
    for k in differ:
        print(f"DIFFERS {k}: {int((a[k] != b[k]).sum())} of {a[k].size} words")
    print(f"{len(a.files)} arrays compared, {len(a.files) - len(differ)} bit-equal")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
