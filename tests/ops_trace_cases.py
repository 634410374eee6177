"""What the wrappers of ``reni_amd.ops`` below ``class Plan`` hand to the library, recorded on CPU tensors without a device.

``Recorder`` stands in for three names of ``ops``: ``_require_cuda`` (accepts anything), ``_call`` (records the entry point and
its arguments instead of calling) and ``_lib.load`` (a proxy that logs every ``*_bytes`` query, a pure host function, and
hands everything else through).  ``trace(install, uninstall)`` runs every case and returns the lines of tests/golden/ops_trace.txt and
the workspace pointers it saw; tests/test_ops_trace_cpu.py compares.  Nothing is launched.

A success line is ``case :: entry point | normalised arguments``: None stays None, a ctypes array is its values, floats are
written by repr, ints as they are, and a pointer becomes its role -- ``in:<name>`` (an input of ``I`` below, passed through
uncopied), ``out:<i>`` (the i-th returned tensor; only in the wrapper's last call, where every buffer is alive at once) or
``buf`` (tables, casts).  A pointer followed by a size_t that is no input or output is the workspace: ``ws:covers`` when the
bytes behind it are at least the result of the case's last ``*_bytes`` query (256 where the wrapper asks none); the byte
count itself moves with the allocator's alignment and is not recorded.  ``case :: -> ...`` gives the returned dtypes and
shapes.  An error line is ``case [cpu] :: Type: message`` with the real ``ops`` and CPU tensors (which checks come before the
device check) or ``case [traced] :: ...`` behind the recorder (the checks behind it).

Shapes: a 4-vertex, 4-face tetrahedron at 4 x 4 pixels, 2 maps of 4 x 8, 8 directions (SSIM needs 6 x 8 and 12 x 12).

To record (from the PARENT's reni_amd, never from the code under test): ``python -m tests.ops_trace_cases OUT`` in a tree
that holds the parent's package, its built library and this file.

Left out: adam_step and adam_rows_step ask torch for the stream outside ``_call`` (only their device check is recorded);
ggx_dfg checks its device argument itself (likewise); selftest_layouts, profile_enable, profile_minmax, profile_read and
launch_count take no tensors and call the library directly; check_visibility, texture_levels, light_maps_view and
light_grid never reach the library."""
import ctypes
import types

import torch

from reni_amd import _lib, ops


# ---------------------------------------------------------------------------------------------------------------- inputs
def _inputs():
    g = torch.Generator().manual_seed(0)

    def rnd(*s):
        return torch.rand(*s, generator=g)

    def unit(*s):
        return torch.nn.functional.normalize(torch.randn(*s, 3, generator=g), dim=-1).contiguous()

    I = types.SimpleNamespace()
    I.verts = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.5
    I.faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=torch.int64)
    I.vn, I.R, I.T = unit(4), torch.eye(3), torch.tensor([0.0, 0.0, 3.0])
    I.p2f = torch.tensor([-1, 0, 0, 1, 0, 0, 1, 1, 2, 2, 3, 3, -1, 2, 3, -1], dtype=torch.int64)
    I.gN, I.gX, I.trans, I.galpha = rnd(16, 3), rnd(16, 3), rnd(16), rnd(16)
    I.vf = ops.vertex_face_lists(I.faces, 4)
    I.table = ops.face_pixel_table(I.p2f, 4)
    I.lists = ops.mesh_edge_lists(I.faces, 4)
    I.order = torch.tensor([3, 1, 0, 2], dtype=torch.int64)
    I.accel = torch.zeros(64, dtype=torch.uint8)
    # the shader: 16 pixels, 8 directions, 2 images
    I.pnrm, I.ppos, I.cam = unit(16), rnd(16, 3), torch.tensor([0.0, 0.0, 3.0])
    I.dirs, I.dirs2 = unit(8), unit(2, 8)
    I.colors, I.dcol, I.gD, I.gS, I.gS1 = rnd(2, 8, 3), rnd(2, 16, 3), rnd(2, 16, 3), rnd(2, 16, 3), rnd(2, 16, 3)
    I.vis1, I.vis2 = torch.ones(1, 16, 1, dtype=torch.int32), torch.ones(2, 16, 1, dtype=torch.int32)
    I.shin, I.shin1, I.alpha = rnd(16) + 1.0, torch.tensor([20.0]), rnd(16) * 0.5 + 0.1
    # baselines, convolutions, lookups: 2 maps of 4 x 8 (32 texels)
    I.sg, I.tc, I.pc = rnd(2, 3, 6), rnd(3), rnd(3)
    I.logt, I.roww = rnd(2, 3, 4, 8), rnd(1, 1, 4, 1)
    I.maps, I.chain, I.planar = rnd(2, 4, 8, 3), rnd(2, 2, 4, 8, 3), rnd(2, 3, 4, 8)
    I.row_t, I.col_t, I.coeffs = rnd(4, 9), rnd(8, 9), rnd(2, 9, 3)
    I.src, I.srcp, I.in_dirs, I.in_w = rnd(2, 32, 3), rnd(2, 3, 32), unit(32), rnd(32)
    I.level, I.level2 = rnd(8), rnd(2, 8)
    I.gout, I.globe, I.den = rnd(2, 8, 3), rnd(2, 2, 8, 3), rnd(2, 8) + 0.5
    I.ltable = (rnd(1, 8, 8), torch.zeros(1, 64, dtype=torch.int64), torch.zeros(1, 33, dtype=torch.int64))
    # textures: 4 x 4 with the full pyramid (3 levels, 21 elements), 16 pixels
    I.verts_uvs, I.bary, I.uv, I.jac = rnd(4, 2), rnd(16, 3), rnd(16, 2), rnd(16, 4)
    I.pix_valid = torch.tensor([0, -1] * 8, dtype=torch.int64)
    I.tex, I.gtex = rnd(21, 3), rnd(16, 3)
    I.tap_index, I.tap_weight = torch.randint(0, 21, (16, 8), generator=g, dtype=torch.int32), rnd(16, 8)
    I.ttable = ops.texture_table(I.tap_index, 21, I.tap_weight)
    # images and scores
    I.img, I.img3, I.hwc, I.gray, I.model = rnd(2, 3, 4, 8), rnd(3, 4, 8), rnd(4, 8, 3), rnd(4, 8), rnd(2, 32, 3)
    I.pred, I.target, I.hw, I.mask, I.expo = rnd(2, 3, 4, 8), rnd(2, 3, 4, 8), rnd(4, 1), rnd(1, 32, 3), rnd(2) + 0.5
    I.pred6, I.target6, I.pred12, I.target12 = rnd(2, 3, 6, 8), rnd(2, 3, 6, 8), rnd(2, 3, 12, 12), rnd(2, 3, 12, 12)
    I.rot, I.rot2, I.index = torch.eye(3), torch.eye(3).repeat(2, 1, 1), torch.tensor([1, 0], dtype=torch.int64)
    # lights
    I.pmf, I.cond, I.marg, I.u, I.u2, I.texw = rnd(2, 4, 8), rnd(2, 4, 8), rnd(2, 4), rnd(3, 2), rnd(2, 3, 2), rnd(32)
    I.normals, I.normals2, I.ldirs, I.lcol = unit(8), unit(2, 8), unit(2, 3), rnd(2, 3, 3)
    # the optimiser
    I.p, I.g, I.m, I.v = rnd(10), rnd(10), rnd(10), rnd(10)
    I.tab, I.grows, I.idx, I.tm, I.tv = rnd(3, 4), rnd(2, 4), torch.tensor([2, 0], dtype=torch.int64), rnd(3, 4), rnd(3, 4)
    return I


I = _inputs()


def _named(prefix, x, out):
    if isinstance(x, torch.Tensor):
        out.setdefault(x.data_ptr(), prefix)
    elif isinstance(x, (tuple, list)):
        for i, y in enumerate(x):
            _named(f"{prefix}[{i}]", y, out)
    elif isinstance(x, dict):
        for k in sorted(x):
            _named(f"{prefix}.{k}", x[k], out)
    return out


IN_ROLES = {}
for _name in sorted(vars(I)):
    _named("in:" + _name, getattr(I, _name), IN_ROLES)


# ---------------------------------------------------------------------------------------------------------------- cases
CASES = []   # (function of ops, keyword arguments of the first success case, further success cases, error cases, modes)


def W(fn, base, ok=(), bad=(), modes=("cpu", "traced"), trace=True):
    CASES.append((fn, base, list(ok), list(bad), modes, trace))


def c(label, **overrides):
    return label, overrides


BAD_VF = (torch.zeros(4, dtype=torch.int64), torch.zeros(12, dtype=torch.int64))
BAD_TABLE = (torch.zeros(5, dtype=torch.int64), torch.zeros(15, dtype=torch.int64))
BAD_LISTS = {**I.lists, "edges": torch.zeros(5, 2, dtype=torch.int64)}

W("adam_step", dict(p=I.p, g=I.g, m=I.m, v=I.v, step=1, lr=1e-3), modes=("cpu",), trace=False)
W("adam_rows_step", dict(table=I.tab, g_rows=I.grows, idx=I.idx, m=I.tm, v=I.tv, step=1, lr=1e-3), modes=("cpu",), trace=False)
W("adam_step2", dict(p=I.p, g=I.g, m=I.m, v=I.v, table=I.tab, g_rows=I.grows, idx=I.idx, tm=I.tm, tv=I.tv, step=3, lr=1e-3,
                     betas=(0.5, 0.75), eps=1e-6, grad_scale=0.5),
  bad=[c("g_rows-length", g_rows=I.grows[:1])])

_shade = dict(normals=I.pnrm, positions=I.ppos, camera_center=I.cam, light_dirs=I.dirs, shininess=50.0, kd=0.5, ks=0.25)
_shade_bad = [c("normals-trailing", normals=I.pnrm[:, :2]), c("light_dirs-batch", light_dirs=I.dirs2.repeat(2, 1, 1)[:3]),
              c("vis-dtype", vis=I.vis1.float()), c("vis-shape", vis=I.vis1[:, :15]), c("vis-images-shared-dirs", vis=I.vis2),
              c("vis-requires-grad", vis=I.vis1.float().requires_grad_())]
W("envmap_shade", dict(_shade, light_colors=I.colors),
  ok=[c("masked", vis=I.vis1), c("per-image", light_dirs=I.dirs2, vis=I.vis2)],
  bad=_shade_bad + [c("light_colors-shape", light_colors=I.colors[:, :7])])
W("envmap_shade_backward", dict(_shade, dcolors=I.dcol),
  ok=[c("masked", vis=I.vis1), c("per-image", light_dirs=I.dirs2, vis=I.vis2)],
  bad=_shade_bad + [c("dcolors-shape", dcolors=I.dcol[:, :15])])

_terms = dict(normals=I.pnrm, positions=I.ppos, camera_center=I.cam, light_dirs=I.dirs)
_mat_bad = [c("normals-rank", normals=I.pnrm[None]), c("light_dirs-trailing", light_dirs=I.dirs[:, :2]),
            c("positions-trailing", positions=I.ppos[:, :2]), c("vis-dtype", vis=I.vis1.float())]
_shin_bad = [c("shininess-type", shininess="x"), c("shininess-length", shininess=I.shin[:5])]
W("envmap_shade_terms", dict(_terms, light_colors=I.colors, shininess=50.0),
  ok=[c("ds-masked-per-pixel", shininess=I.shin, vis=I.vis1, need_ds=True), c("one-value-per-image", shininess=I.shin1,
                                                                               light_dirs=I.dirs2, vis=I.vis2)],
  bad=_mat_bad + _shin_bad + [c("light_colors-shape", light_colors=I.colors[:1, :7])])
W("envmap_shade_terms_backward", dict(_terms, gD=I.gD, gS=I.gS, shininess=I.shin),
  ok=[c("masked-float", shininess=20.0, vis=I.vis1)], bad=_mat_bad + _shin_bad + [c("gS-shape", gS=I.gS[:, :15])])
W("envmap_shade_terms_dnormals", dict(_terms, light_colors=I.colors, gD=I.gD, gS=I.gS, shininess=I.shin),
  ok=[c("masked-float", shininess=20.0, vis=I.vis1)], bad=_mat_bad + _shin_bad + [c("gD-shape", gD=I.gD[:, :15])])
_alpha_bad = [c("alpha-type", alpha=None), c("alpha-length", alpha=I.alpha[:5])]
W("envmap_shade_ggx", dict(_terms, light_colors=I.colors, alpha=0.25),
  ok=[c("masked-per-pixel", alpha=I.alpha, vis=I.vis1)], bad=_mat_bad + _alpha_bad)
W("envmap_shade_ggx_backward", dict(_terms, gD=I.gD, gS0=I.gS, gS1=I.gS1, alpha=I.alpha),
  ok=[c("masked-float", alpha=0.25, vis=I.vis1)], bad=_mat_bad + _alpha_bad + [c("gS1-shape", gS1=I.gS1[:, :15])])
W("envmap_shade_ggx_dpixel", dict(_terms, light_colors=I.colors, gD=I.gD, gS0=I.gS, gS1=I.gS1, alpha=I.alpha),
  ok=[c("masked-float-dn", alpha=0.25, vis=I.vis1, need_dn=True)], bad=_mat_bad + _alpha_bad)

_mesh = dict(verts=I.verts, faces=I.faces)
_mesh_bad = [c("verts-trailing", verts=I.verts[:, :2]), c("faces-rank", faces=I.faces[0]), c("verts-none", verts=None)]
_cam_bad = [c("R-length", R=torch.eye(3)[:2]), c("image_size-zero", image_size=0)]
W("vertex_normals", _mesh, ok=[c("vf", vf=I.vf)], bad=_mesh_bad + [c("vf-malformed", vf=BAD_VF)])
W("rasterize_mesh", dict(_mesh, vert_normals=I.vn, R=I.R, T=I.T, image_size=4), ok=[c("fov", tan_half_fov=0.25)],
  bad=_mesh_bad + _cam_bad + [c("vert_normals-shape", vert_normals=I.vn[:3])])
W("vertex_normals_backward", dict(_mesh, grad_normals=I.gN[:4].contiguous()), ok=[c("vf", vf=I.vf)],
  bad=_mesh_bad + [c("grad_normals-shape", grad_normals=I.gN[:3]), c("grad_normals-none", grad_normals=None),
                   c("vf-malformed", vf=BAD_VF)])
_gb = dict(_mesh, vert_normals=I.vn, R=I.R, T=I.T, image_size=4, pix_to_face=I.p2f, grad_pixel_normals=I.gN,
           grad_pixel_positions=I.gX)
_gb_ok = [c("gX-only-table-vf", grad_pixel_normals=None, table=I.table, vf=I.vf, tan_half_fov=0.25),
          c("gN-only", grad_pixel_positions=None)]
_gb_bad = _mesh_bad + _cam_bad + [
    c("vert_normals-none", vert_normals=None), c("vert_normals-shape", vert_normals=I.vn[:3]),
    c("pix_to_face-dtype", pix_to_face=I.p2f.int()), c("pix_to_face-length", pix_to_face=I.p2f[:15]),
    c("both-none", grad_pixel_normals=None, grad_pixel_positions=None), c("gN-shape", grad_pixel_normals=I.gN[:15]),
    c("gX-rank", grad_pixel_positions=I.gX[0]), c("table-malformed", table=BAD_TABLE), c("vf-malformed", vf=BAD_VF)]
W("gbuffer_backward", _gb, ok=_gb_ok, bad=_gb_bad)
W("gbuffer_backward_camera", _gb, ok=_gb_ok + [c("pose-only", need_verts=False), c("pose-only-vf-ignored", need_verts=False, vf=I.vf)],
  bad=_gb_bad)
_sil = dict(_mesh, R=I.R, T=I.T, image_size=4, tan_half_fov=0.5, sigma=1e-2, blur_radius=1e-3)
_sil_bad = _mesh_bad + _cam_bad + [c("sigma-zero", sigma=0.0), c("sigma-inf", sigma=float("inf")), c("sigma-nan", sigma=float("nan")),
                                   c("blur_radius-negative", blur_radius=-1.0), c("blur_radius-inf", blur_radius=float("inf"))]
W("soft_silhouette", _sil, ok=[c("no-blur", blur_radius=0.0)], bad=_sil_bad)
_silb = dict(_sil, trans=I.trans, grad_alpha=I.galpha)
_silb_bad = _sil_bad + [c("trans-length", trans=I.trans[:15]), c("grad_alpha-none", grad_alpha=None), c("vf-malformed", vf=BAD_VF)]
W("soft_silhouette_backward", _silb, ok=[c("vf", vf=I.vf)], bad=_silb_bad)
W("soft_silhouette_backward_camera", _silb, ok=[c("vf", vf=I.vf), c("pose-only", need_verts=False)], bad=_silb_bad)
W("mesh_regularizers", dict(_mesh, edge=1.0, laplacian=0.5, normal=0.25, target_length=0.125),
  ok=[c("cot-lists-values-only", method="cot", lists=I.lists, need_grad=False), c("defaults", edge=0.0, laplacian=0.0, normal=0.0,
                                                                                   target_length=0.0)],
  bad=_mesh_bad + [c("method", method="x"), c("edge-negative", edge=-1.0), c("laplacian-nan", laplacian=float("nan")),
                   c("normal-inf", normal=float("inf")), c("target_length-negative", target_length=-1.0),
                   c("lists-key", lists={"E": 6}), c("lists-shape", lists=BAD_LISTS), c("lists-type", lists=3)])
W("mesh_visibility_prepare", _mesh, ok=[c("order", order=I.order)],
  bad=_mesh_bad + [c("order-length", order=I.order[:3]), c("order-type", order=[3, 1, 0, 2])])
W("mesh_visibility", dict(positions=I.ppos, pix_to_face=I.p2f, dirs=I.dirs, accel=I.accel, t_min=1e-3),
  ok=[c("per-image-no-cull", dirs=I.dirs2, no_cull=True)],
  bad=[c("dirs-trailing", dirs=I.dirs[:, :2]), c("dirs-rank", dirs=I.dirs[0]), c("positions-trailing", positions=I.ppos[:, :2]),
       c("pix_to_face-dtype", pix_to_face=I.p2f.int()), c("pix_to_face-length", pix_to_face=I.p2f[:15]),
       c("accel-dtype", accel=I.accel.float()), c("t_min-negative", t_min=-1.0), c("t_min-inf", t_min=float("inf"))])

W("sg_render", dict(params=I.sg, theta_c=I.tc, phi_c=I.pc, theta_range=0.5, phi_range=0.25, H=4, W=8),
  bad=[c("params-trailing", params=I.sg[:, :, :5]), c("theta_c-length", theta_c=I.tc[:2])])
W("sg_loss_grad", dict(params=I.sg, theta_c=I.tc, phi_c=I.pc, theta_range=0.5, phi_range=0.25, log_target=I.logt, weight=I.roww),
  bad=[c("log_target-channels", log_target=I.logt[:, :2]), c("params-batch", params=I.sg[:1]), c("phi_c-length", phi_c=I.pc[:2])])
W("sh_project", dict(imgs=I.maps, row_table=I.row_t, col_table=I.col_t, lmax=2), bad=[c("imgs-trailing", imgs=I.maps[..., :2])])
W("sh_reconstruct", dict(coeffs=I.coeffs, row_table=I.row_t, col_table=I.col_t, H=4, W=8, lmax=2),
  bad=[c("coeffs-length", coeffs=I.coeffs[:, :8])])
_conv = dict(in_dirs=I.in_dirs, in_weight=I.in_w, out_dirs=I.dirs)
_conv_bad = [c("in_dirs-trailing", in_dirs=I.in_dirs[:, :2]), c("out_dirs-rank", out_dirs=I.dirs[0]),
             c("in_weight-length", in_weight=I.in_w[:31])]
_src_bad = [c("src-rank", src=I.src[0]), c("src-texels", src=I.src[:, :31])]
W("diffuse_convolve", dict(_conv, src=I.src, scale=0.5), ok=[c("planar", src=I.srcp)], bad=_conv_bad + _src_bad)
W("sh_irradiance_l2", dict(coeffs=I.coeffs, normals=I.normals), ok=[c("per-map", normals=I.normals2)],
  bad=[c("coeffs-length", coeffs=I.coeffs[:, :8]), c("normals-batch", normals=I.normals2[:1].repeat(3, 1, 1)),
       c("normals-trailing", normals=I.normals[:, :2])])
_lobes = dict(kinds=("phong", "ggx"), params=(8.0, 0.5))
_lobe_bad = [c("kind", kinds=("phong", "x")), c("no-lobes", kinds=(), params=()), c("params-length", params=(8.0,))]
W("lobe_convolve", dict(_conv, **_lobes, src=I.src), ok=[c("planar-scaled", src=I.srcp, normalise=False, scale=0.5)],
  bad=_conv_bad + _src_bad + _lobe_bad)
_maps_bad = [c("maps-trailing", maps=I.maps[..., :2]), c("maps-odd-width", maps=I.maps[:, :, :7]), c("maps-rank", maps=I.maps[0, 0])]
_dirs_bad = [c("dirs-trailing", dirs=I.dirs[:, :2]), c("dirs-batch", dirs=I.dirs2[:1].repeat(3, 1, 1)), c("level-length", level=I.level[:7]),
             c("level-rank", level=I.level2[None])]
W("envmap_lookup", dict(maps=I.maps, dirs=I.dirs),
  ok=[c("chain-number-per-map", maps=I.chain, dirs=I.dirs2, level=0.5), c("chain-level", maps=I.chain, level=I.level),
      c("chain-level-per-map", maps=I.chain, level=I.level2), c("strided", maps=I.planar.permute(0, 2, 3, 1))],
  bad=_maps_bad + _dirs_bad)
W("lobe_denominators", dict(_conv, **_lobes), bad=_conv_bad + _lobe_bad)
W("lobe_convolve_backward", dict(_conv, **_lobes, grad_out=I.globe),
  ok=[c("den-planar", den=I.den, planar=True), c("scaled", normalise=False, scale=0.5), c("scaled-den-ignored", normalise=False, den=I.den)],
  bad=_conv_bad + _lobe_bad + [c("grad_out-lobes", grad_out=I.globe[:, :1]), c("grad_out-rank", grad_out=I.globe[0]),
                               c("den-shape", den=I.den[:, :7])])
W("envmap_lookup_table", dict(N=2, Lv=2, H=4, W=8, dirs=I.dirs), ok=[c("per-map-level", level=I.level2), c("number", level=1.0)],
  bad=[c("odd-width", W=7), c("no-maps", N=0)] + _dirs_bad)
W("envmap_lookup_backward", dict(grad_out=I.gout, Lv=1, H=4, W=8, dirs=I.dirs),
  ok=[c("table", dirs=None, table=I.ltable), c("level", Lv=2, level=I.level)],
  bad=[c("grad_out-trailing", grad_out=I.gout[..., :2]), c("no-dirs-no-table", dirs=None), c("table-shape", table=I.ltable, H=5),
       c("table-dtype", table=(I.ltable[0], I.ltable[1].int(), I.ltable[2]))])
W("envmap_lookup_dquery", dict(maps=I.maps, dirs=I.dirs, level=None, grad_out=I.gout),
  ok=[c("level-only", maps=I.chain, level=I.level, need_dirs=False, need_level=True),
      c("both-per-map", maps=I.chain, dirs=I.dirs2, level=I.level2, need_level=True)],
  bad=_maps_bad + _dirs_bad + [c("neither", need_dirs=False), c("level-number", level=0.5, need_level=True),
                               c("grad_out-shape", grad_out=I.gout[:, :7])])
W("ggx_dfg", dict(device="cpu"), modes=("cpu",), trace=False)

W("mesh_pixel_uv", dict(_mesh, verts_uvs=I.verts_uvs, faces_uvs=I.faces, R=I.R, T=I.T, image_size=4, pix_to_face=I.p2f, bary=I.bary),
  bad=_mesh_bad + _cam_bad + [c("verts_uvs-trailing", verts_uvs=I.verts), c("faces_uvs-shape", faces_uvs=I.faces[:3]),
                              c("bary-length", bary=I.bary[:15])])
W("texture_taps", dict(uv=I.uv, size=(4, 4)),
  ok=[c("jac-valid-repeat", jac=I.jac, pix_valid=I.pix_valid, wrap="repeat", lod_bias=0.5),
      c("one-level-corners", levels=1, align_corners=True)],
  bad=[c("wrap", wrap="x"), c("align_corners-levels", align_corners=True), c("lod_bias-nan", lod_bias=float("nan")),
       c("lod_bias-inf", lod_bias=float("inf")), c("uv-trailing", uv=I.bary), c("jac-length", jac=I.jac[:15]),
       c("pix_valid-rank", pix_valid=I.pix_valid[None]), c("levels", levels=9), c("uv-requires-grad", uv=I.uv.clone().requires_grad_())])
_tex_bad = [c("dtype", tex=I.tex.double()), c("elements", tex=I.tex[:20]), c("strided", tex=I.tex.t().contiguous().t()),
            c("levels", levels=4)]
W("texture_pyramid", dict(tex=I.tex, levels=3, H0=4, W0=4), bad=_tex_bad)
W("texture_pyramid_backward", dict(grad_tex=I.tex, levels=3, H0=4, W0=4),
  bad=[(label, {("grad_tex" if k == "tex" else k): v for k, v in o.items()}) for label, o in _tex_bad])
W("texture_fetch", dict(tex=I.tex, tap_index=I.tap_index, tap_weight=I.tap_weight),
  bad=[c("tap_weight-dtype", tap_weight=I.tap_weight.double()), c("tap_index-dtype", tap_index=I.tap_index.long()),
       c("tap_index-shape", tap_index=I.tap_index[:15]), c("tex-channels", tex=I.tex.repeat(1, 3))])
W("texture_fetch_backward", dict(grad_out=I.gtex, tap_weight=I.tap_weight, table=I.ttable, E=21), ok=[c("plain", plain=True)],
  bad=[c("grad_out-length", grad_out=I.gtex[:15]), c("table-elements", E=20), c("table-dtype", table=(I.ttable[0].int(), I.ttable[1])),
       c("tap_weight-rank", tap_weight=I.tap_weight[0])])

W("unnormalise_srgb", dict(img=I.img),
  ok=[c("minmax-both", minmax=(-1.0, 2.0), want_linear=True), c("linear-only", img=I.img3, minmax=(-1.0, 2.0), srgb=False),
      c("model-output", img=I.model.view(2, 4, 8, 3).permute(0, 3, 1, 2))],
  bad=[c("channels", img=I.maps), c("rank", img=I.gray)])
W("minmax_normalise", dict(img=I.img3, minmax=(-1.0, 2.0)))
W("minmax_normalise_batch", dict(imgs=I.img, minmax=(-1.0, 2.0)), ok=[c("keep-nan", nan_to_num=False)],
  bad=[c("rank", imgs=I.in_w), c("empty", imgs=I.img[:0])])
W("resample", dict(src=I.img, size=(2, 4)),
  ok=[c("channel-last-nearest", src=I.hwc, layout="hwc", mode="nearest"), c("model-output-bicubic", src=I.model.view(2, 4, 8, 3), layout="hwc", mode="bicubic"),
      c("gray-lanczos", src=I.gray, mode="lanczos4", size=(8, 16)), c("planar-one", src=I.img3), c("auto-channel-last", src=I.pred6[0].permute(1, 2, 0))],
  bad=[c("mode", mode="x"), c("size-zero", size=(0, 4)), c("layout", layout="x"), c("ambiguous", src=I.img3[:, :, :3]),
       c("rank", src=I.in_w), c("empty", src=I.img[:0])])
W("gaussian_blur", dict(img=I.gray, sigma=1.0), ok=[c("channel-last", img=I.hwc, sigma=0.5, layout="hwc"), c("planar", img=I.img3, sigma=0.5),
                                                    c("strided-auto", img=I.pred6[0].permute(1, 2, 0), sigma=0.5)],
  bad=[c("sigma-zero", sigma=0.0), c("sigma-nan", sigma=float("nan")), c("rank", img=I.img), c("layout", layout="x")])
W("rotate_envmap", dict(src=I.img, rot=I.rot),
  ok=[c("per-image-nearest", rot=I.rot2, mode="nearest"), c("index", rot=I.rot2, index=I.index),
      c("model-output", src=I.model.view(2, 4, 8, 3), layout="hwc"), c("one-map", src=I.img3)],
  bad=[c("mode", mode="x"), c("odd-width", src=I.img[..., :7]), c("rot-shape", rot=I.rot[:2, :2]),
       c("rot-batch", rot=I.rot2[:1].repeat(3, 1, 1)), c("index-no-batch", src=I.img3, index=I.index),
       c("index-rank", index=I.index[None]), c("layout", layout="x")])
_pair = dict(pred=I.pred, target=I.target)
_pair_bad = [c("space", space="x"), c("linear-no-minmax", space="linear"), c("minmax-order", space="linear", minmax=(1.0, 1.0)),
             c("srgb-no-exposure", space="srgb", minmax=(0.0, 1.0)), c("exposure-length", space="srgb", minmax=(0.0, 1.0), exposure=I.expo[:1]),
             c("pred-channels", pred=I.planar[:, :2]), c("pred-none", pred=None), c("target-batch", target=I.target[:1]),
             c("pixels-not-hx2h", pred=I.model[:, :31], target=I.model[:, :31]), c("size-mismatch", pred=I.model, target=I.model, size=(4, 7)),
             c("weight-negative", weight=-I.hw), c("weight-shape", weight=I.in_w[:5]), c("weight-type", weight=1.0)]
W("pair_stats", _pair,
  ok=[c("rows-linear", weight=I.hw, space="linear", minmax=(-1.0, 2.0)),
      c("model-output-srgb-mask", pred=I.model, target=I.model, weight=I.mask, space="srgb", minmax=(-1.0, 2.0), exposure=I.expo,
        size=(4, 8), check_weight=False),
      c("model-output-default-size", pred=I.model, target=I.img)],
  bad=_pair_bad)
W("ssim", dict(pred=I.pred6, target=I.target6),
  ok=[c("map-weight-srgb", weight=I.hw[:1].expand(6, 1), space="srgb", minmax=(-1.0, 2.0), exposure=I.expo, L=2.0, return_map=True),
      c("planar", pred=I.pred12, target=I.target12, sphere=False)],
  bad=_pair_bad[:4] + [c("L-zero", L=0.0), c("sphere-rows", pred=I.pred, target=I.target),
                       c("planar-weight", pred=I.pred12, target=I.target12, sphere=False, weight=I.target12[:, 0]),
                       c("planar-small", sphere=False)])
_light_bad = [c("space", space="srgb"), c("linear-no-minmax", minmax=None), c("maps-grid", maps=I.maps[:, :, :6]),
              c("maps-rank", maps=I.gray), c("maps-type", maps=None)]
W("light_table_build", dict(maps=I.maps, minmax=(-1.0, 2.0)),
  ok=[c("stored-mask-mix", space="stored", minmax=None, mask=I.hw, uniform_mix=0.5), c("model-output-mask", maps=I.model, mask=I.mask),
      c("planar-size", maps=I.planar, size=(4, 8))],
  bad=_light_bad + [c("uniform_mix", uniform_mix=1.5), c("mask-shape", mask=I.in_w[:5])])
W("light_sample", dict(pmf=I.pmf, cond=I.cond, marg=I.marg, maps=I.maps, u=I.u, minmax=(-1.0, 2.0)),
  ok=[c("per-map-weight-jitter", u=I.u2, space="stored", minmax=None, texel_weight=I.texw, jitter=True)],
  bad=_light_bad + [c("pmf-shape", pmf=I.pmf[:1]), c("marg-dtype", marg=I.marg.double()), c("u-trailing", u=I.lcol[0]),
                    c("u-batch", u=I.u2[:1].repeat(3, 1, 1)), c("texel_weight-length", texel_weight=I.texw[:31])])
W("lights_irradiance", dict(normals=I.normals, dirs=I.ldirs, colors=I.lcol, scale=0.5), ok=[c("per-map", normals=I.normals2)],
  bad=[c("colors-shape", colors=I.lcol[:, :2]), c("normals-batch", normals=I.normals2[:1].repeat(3, 1, 1)), c("normals-none", normals=None),
       c("dirs-rank", dirs=I.ldirs[0], colors=I.lcol[0])])

# the pure-torch builders: checked through what they return
BUILDERS = [
    ("vertex_face_lists", dict(faces=I.faces, V=4), [c("no-face-in-range", V=0)], []),
    ("face_pixel_table", dict(pix_to_face=I.p2f, F=4), [c("image", pix_to_face=I.p2f.view(1, 4, 4, 1))], []),
    ("mesh_edge_lists", dict(faces=I.faces, V=4), [c("degenerate-face", faces=I.faces.clone().index_fill_(0, torch.tensor([3]), 1))],
     [c("faces-trailing", faces=I.faces[:, :2]), c("faces-none", faces=None), c("V-zero", V=0)]),
    ("texture_table", dict(tap_index=I.tap_index, E=21), [c("weights", tap_weight=I.tap_weight)],
     [c("tap_index-dtype", tap_index=I.tap_index.long()), c("E-zero", E=0), c("tap_weight-shape", tap_weight=I.tap_weight[:15])]),
]


# ---------------------------------------------------------------------------------------------------------------- recorder
class Recorder:
    """The three stand-ins (see the module docstring); ``events`` holds what one wrapper call did."""

    def __init__(self, lib):
        self._real = lib
        self.events = []

    def load(self):
        return self

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.endswith("_bytes"):
            return fn

        def query(*args):
            result = fn(*args)
            self.events.append(("query", name, args, int(result)))
            return result
        return query

    def require_cuda(self, *tensors):
        pass

    def call(self, fn, device, *args):
        assert len(args) == len(fn.argtypes) - 1, f"{fn.__name__}: {len(args)} arguments and a stream for {len(fn.argtypes)} parameters"
        self.events.append(("call", fn.__name__, fn.argtypes[:-1], args))


def _describe(x):
    if isinstance(x, torch.Tensor):
        return f"{str(x.dtype)[6:]}{list(x.shape)}"
    if isinstance(x, (tuple, list)):
        return "(" + ", ".join(_describe(y) for y in x) + ")"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}: {_describe(x[k])}" for k in sorted(x)) + "}"
    return repr(x)


def _format(events, result, workspaces):
    out_roles = {}
    for i, t in enumerate(result if isinstance(result, (tuple, list)) else (result,)):
        if isinstance(t, torch.Tensor):
            out_roles.setdefault(t.data_ptr(), f"out:{i}")
    last = max((i for i, e in enumerate(events) if e[0] == "call"), default=-1)
    lines, need = [], 256
    for n, (kind, name, a, b) in enumerate(events):
        if kind == "query":
            lines.append(f"{name}({', '.join(repr(x) for x in a)}) -> {b}")
            need = b
            continue
        types_, args, cells, i = a, b, [], 0
        while i < len(args):
            ty, x = types_[i], args[i]
            if ty is ctypes.c_void_p and x is not None:
                role = IN_ROLES.get(x) or (out_roles.get(x) if n == last else None)
                if role is None and i + 1 < len(args) and types_[i + 1] is ctypes.c_size_t:
                    workspaces.append((name, x))
                    cells.append("ws:covers" if args[i + 1] >= need else f"ws:short({args[i + 1]} < {need})")
                    i += 2
                    continue
                cells.append(role or "buf")
            elif isinstance(x, ctypes.Array):
                cells.append("[" + ", ".join(repr(y) for y in x) + "]")
            else:
                cells.append(repr(x))
            i += 1
        lines.append(f"{name} | " + " | ".join(cells))
        need = 256
    return lines


def trace(install, uninstall):
    """Every case -> (the golden's lines, [(entry point, workspace pointer)]).  install(recorder) puts the three stand-ins
    into ``ops``, uninstall() takes them out again (the [cpu] lines run the real ``ops``)."""
    lines, workspaces = [], []
    rec = Recorder(_lib.load())

    def run(fn, kw, traced):
        rec.events = []
        if traced:
            install(rec)
        try:
            result = getattr(ops, fn)(**kw)
        except Exception as e:  # noqa: BLE001 -- the line IS the exception
            return None, f"{type(e).__name__}: {e}".replace("\n", " / ")
        finally:
            if traced:
                uninstall()
        return result, None

    for fn, base, ok, bad, modes, traced in CASES:
        for label, over in ([("base", {})] + ok if traced else []):
            result, err = run(fn, {**base, **over}, True)
            head = f"{fn}/{label} :: "
            if err is not None:
                lines.append(head + "FAILED " + err)
                continue
            lines += [head + x for x in _format(rec.events, result, workspaces)]
            lines.append(head + "-> " + _describe(result))
        for label, over in ([] if traced else [("base", {})]) + bad:
            for mode in modes:
                result, err = run(fn, {**base, **over}, mode == "traced")
                lines.append(f"{fn}/{label} [{mode}] :: " + (err if err is not None else "no error"))
    for fn, base, ok, bad in BUILDERS:
        for label, over in [("base", {})] + ok:
            lines.append(f"{fn}/{label} :: -> " + _describe(getattr(ops, fn)(**{**base, **over})))
        for label, over in bad:
            result, err = run(fn, {**base, **over}, False)
            lines.append(f"{fn}/{label} :: " + (err if err is not None else "no error"))
    return lines, workspaces


if __name__ == "__main__":
    import sys
    saved = (ops._require_cuda, ops._call, _lib.load)

    def _install(rec):
        ops._require_cuda, ops._call, _lib.load = rec.require_cuda, rec.call, rec.load

    def _uninstall():
        ops._require_cuda, ops._call, _lib.load = saved

    got, ws = trace(_install, _uninstall)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(got) + "\n")
    print(f"{len(got)} lines; {sum(p % 256 != 0 for _, p in ws)} of {len(ws)} workspace pointers off 256-byte alignment")
