"""GPU tests of the soft silhouette (reni_tu_silhouette.hip, ops.soft_silhouette, ops.soft_silhouette_backward,
MeshRasterizer.silhouette) against the float64 reference of tests/silhouette_ref.py.

Bounds: max(K 2^-23 sum |terms|, 2e-5 max |ref|) per element, sum |terms| accumulated by the reference, K = 4 x the worst
ratio of the float32 CPU evaluation over the same cases and settings (K_ALPHA, K_GVERTS of the case file; DESIGN 4.4r has
the measured figures, the device's among them).  alpha and trans must lie within the bound of the interval
[reference_lo, reference_hi] (the undecided pairs taken either way); the gradient, evaluated by the reference with the
device's own trans, within the bound of reference_lo widened per element by |reference_hi - reference_lo|.  Every test
prints its figure before it asserts."""
import pytest
import torch

from tests import raster_edge_cases as E
from tests import silhouette_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMBOS = tuple((key, name) for key in R.CASES for name in R.SETTINGS)


def _combo_id(c):
    return R.case_id(c[0]) + "-" + c[1]


def _dev(key):
    v, f, Rm, T, S = R.case(*key)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), Rm, T, S


def _forward(key, name):
    from reni_amd import ops
    v, f, Rm, T, S = _dev(key)
    sigma, r = R.setting(name, S)
    return (v, f, Rm, T, S, sigma, r) + ops.soft_silhouette(v, f, Rm, T, S, E.TANF, sigma, r)


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_forward_matches_the_float64_reference(combo):
    from reni_amd import ops
    key, name = combo
    v, f, Rm, T, S, sigma, r, alpha, trans = _forward(key, name)
    lo, hi = R.reference_lo(key, name), R.reference_hi(key, name)
    n, u = R.count_pairs(key, name)
    ra = R.error_ratio(alpha, lo["alpha"], hi["alpha"], lo["terms_alpha"], False)
    rt = R.error_ratio(trans, lo["trans"], hi["trans"], lo["terms_alpha"], False)
    oa = R.over_bound(alpha, lo["alpha"], hi["alpha"], lo["terms_alpha"], R.K_ALPHA, False)
    ot = R.over_bound(trans, lo["trans"], hi["trans"], lo["terms_alpha"], R.K_ALPHA, False)
    print(f"alpha {_combo_id(combo)}: error / (2^-23 sum |terms|) = {ra:.4g} (trans {rt:.4g}), error / bound = {oa:.4g} "
          f"(trans {ot:.4g}), pairs {n}, undecided {u}")
    assert alpha.shape == (S * S,) and trans.shape == (S * S,) and torch.isfinite(alpha).all() and torch.isfinite(trans).all()
    assert oa <= 1.0 and ot <= 1.0
    # a pixel no face takes part at, under either choice: exactly 0 / 1
    v64, f64, R64, T64, _, tanh = R.inputs(key)
    with torch.no_grad():
        _, x, y, _ = R.taking_part(v64, f64, R64, T64, tanh)
        background = ~R.pairs(x, y, S, r)["either"].any(dim=1).to(DEV)
    assert (alpha[background] == 0).all() and (trans[background] == 1).all()
    if key[0] == "behind":
        assert bool(background.all())
    # two calls give equal bits
    alpha2, trans2 = ops.soft_silhouette(v, f, Rm, T, S, E.TANF, sigma, r)
    assert torch.equal(alpha, alpha2) and torch.equal(trans, trans2)


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_backward_matches_the_float64_reference(combo):
    from reni_amd import ops
    key, name = combo
    v, f, Rm, T, S, sigma, r, alpha, trans = _forward(key, name)
    gA = R.upstream(key, name)
    gA_dev = gA.float().to(DEV)
    got = ops.soft_silhouette_backward(v, f, Rm, T, S, E.TANF, sigma, r, trans, gA_dev)
    t64 = trans.double().cpu()
    lo, hi = R.reference_lo(key, name, gA, t64), R.reference_hi(key, name, gA, t64)
    terms = torch.maximum(lo["terms_g"], hi["terms_g"])
    print(f"g_verts {_combo_id(combo)}: error / (2^-23 sum |terms|) = {R.error_ratio(got, lo['g'], hi['g'], terms, True):.4g}, "
          f"error / bound = {R.over_bound(got, lo['g'], hi['g'], terms, R.K_GVERTS, True):.4g}, "
          f"max |ref| = {float(lo['g'].abs().max()):.4g}, max |hi - lo| = {float((hi['g'] - lo['g']).abs().max()):.4g}")
    assert got.shape == lo["g"].shape and torch.isfinite(got).all()
    assert R.over_bound(got, lo["g"], hi["g"], terms, R.K_GVERTS, True) <= 1.0  # no case and no vertex left out
    # exact zeros
    assert (ops.soft_silhouette_backward(v, f, Rm, T, S, E.TANF, sigma, r, trans, torch.zeros_like(gA_dev)) == 0).all()
    if key[0] == "unreferenced":
        assert (got[R.UNREFERENCED] == 0).all() and (got != 0).any()
    if key[0] == "behind":
        assert (got == 0).all()
    if key[0] == "cover" and name != "wide":  # alpha = 1: trans = 0 everywhere
        assert (trans == 0).all() and (alpha == 1).all() and (got == 0).all()
    # two calls give equal bits; lists passed in by the caller give the same bits as lists built inside
    assert torch.equal(got, ops.soft_silhouette_backward(v, f, Rm, T, S, E.TANF, sigma, r, trans, gA_dev))
    vf = ops.vertex_face_lists(f, v.shape[0])
    assert torch.equal(got, ops.soft_silhouette_backward(v, f, Rm, T, S, E.TANF, sigma, r, trans, gA_dev, vf=vf))


def test_gradient_is_exactly_zero_where_trans_is_zero():
    """cover-33, wide: an upstream that lives only on the pixels whose trans is 0 gives exactly 0 (no division by 1 - prob);
    and on the sharp settings, where trans is 0 everywhere, any upstream does"""
    from reni_amd import ops
    key = ("cover", 33)
    for name in R.SETTINGS:
        v, f, Rm, T, S, sigma, r, alpha, trans = _forward(key, name)
        gA = R.upstream(key, name).float().to(DEV)
        gA = torch.where(trans == 0, gA, torch.zeros_like(gA))
        got = ops.soft_silhouette_backward(v, f, Rm, T, S, E.TANF, sigma, r, trans, gA)
        print(f"cover-33 {name}: {int((trans == 0).sum())} of {S * S} pixels with trans = 0")
        assert (got == 0).all()


def test_malformed_input_adds_nothing():
    """ico-17: bad face indices, vertex-list entries outside [0, 3F) and offsets outside the list are skipped: the results
    are those of the well-formed entries alone"""
    from reni_amd import ops
    key, name = ("ico", 17), "sharp"
    v, f, Rm, T, S, sigma, r, alpha, trans = _forward(key, name)
    V, F = v.shape[0], f.shape[0]
    gA = R.upstream(key, name).float().to(DEV)
    off, lst = ops.vertex_face_lists(f, V)

    def run(faces, tr, vf):
        return ops.soft_silhouette_backward(v, faces, Rm, T, S, E.TANF, sigma, r, tr, gA, vf=vf)

    good = run(f, trans, None)
    assert torch.equal(good, run(f, trans, (off, lst)))
    # bad face indices: every fifth face gets one; the mesh without those faces gives the same alpha and the same gradient
    bad = f.clone()
    junk = torch.tensor([-1, V, 2 ** 40, -7, V + 3], device=DEV)
    rows = torch.arange(0, F, 5, device=DEV)
    bad[rows, rows % 3] = junk.repeat(rows.numel() // 5 + 1)[:rows.numel()]
    keep = torch.ones(F, dtype=torch.bool, device=DEV)
    keep[rows] = False
    a_bad, t_bad = ops.soft_silhouette(v, bad, Rm, T, S, E.TANF, sigma, r)
    a_kept, t_kept = ops.soft_silhouette(v, f[keep], Rm, T, S, E.TANF, sigma, r)
    assert torch.equal(a_bad, a_kept) and torch.equal(t_bad, t_kept) and not torch.equal(a_bad, alpha)
    g_bad = run(bad, t_bad, None)
    g_kept = ops.soft_silhouette_backward(v, f[keep], Rm, T, S, E.TANF, sigma, r, t_kept, gA)
    assert torch.equal(g_bad, g_kept) and torch.isfinite(g_bad).all()
    # list entries outside [0, 3F): every third entry replaced; the same as the list with those entries naming no vertex
    bad_list = lst.clone()
    bad_list[::3] = torch.tensor([-1, 3 * F, 2 ** 40], device=DEV).repeat(lst.numel() // 9 + 1)[:bad_list[::3].numel()]
    dropped = run(f, trans, (off, bad_list))
    assert (dropped != good).any() and torch.isfinite(dropped).all()
    # (the reference for "dropped": the corners behind the replaced entries contribute nothing -- the same gather without them)
    kept_list = lst.clone()
    kept_list[::3] = -1
    assert torch.equal(dropped, run(f, trans, (off, kept_list)))
    # offsets outside the list are clamped into it: vertex 0's range starts in front of the list, the last vertex's ends beyond it
    off_wide = off.clone()
    off_wide[0], off_wide[V] = -5, 3 * F + 7
    assert torch.equal(good, run(f, trans, (off_wide, lst)))
    off_wide[1] = 3 * F + 7  # vertex 0 is offered the whole list: the entries that do not name it add nothing; vertex 1's range is empty
    wide = run(f, trans, (off_wide, lst))
    assert torch.equal(wide[0], good[0]) and (wide[1] == 0).all() and torch.equal(wide[2:], good[2:])


def _mesh_and_rasterizer(key, requires_grad, S=None):
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings
    v, f, Rm, T, S0 = _dev(key)
    v = v.clone().requires_grad_(requires_grad)
    mesh = Meshes(verts=[v], faces=[f])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=S or S0))
    return v, f, Rm.to(DEV), T.to(DEV), mesh, rast


def test_autograd_through_the_rasterizer():
    import math
    from reni_amd import ops
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, RasterizationSettings, look_at_view_transform
    key = ("ico", 16)
    v, f, Rm, T, mesh, rast = _mesh_and_rasterizer(key, True)
    S = 16
    sigma = R.setting("sharp", S)[0]
    tanf = rast.cameras.tan_half_fov()
    w = torch.randn(S, S, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    alpha = rast.silhouette(mesh, Rm, T, sigma=sigma)
    assert alpha.shape == (S, S) and alpha.requires_grad
    r = math.log(1.0 / 1e-4 - 1.0) * sigma  # the default blur_radius
    a_ops, t_ops = ops.soft_silhouette(v.detach(), f, Rm, T, S, tanf, sigma, r)
    assert torch.equal(alpha.detach().reshape(-1), a_ops)
    (alpha * w).sum().backward()
    g1 = ops.soft_silhouette_backward(v.detach(), f, Rm, T, S, tanf, sigma, r, t_ops, w.reshape(-1))
    assert (g1 != 0).any() and torch.equal(v.grad, g1)
    # two views accumulate
    R2, T2 = look_at_view_transform(2.0, 20.0, 40.0, device=DEV)
    rast2 = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=17))
    w2 = torch.randn(17, 17, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    sigma2 = R.setting("sharp", 17)[0]
    (g2,) = torch.autograd.grad((rast2.silhouette(mesh, R2, T2, sigma=sigma2) * w2).sum(), v)
    v.grad = None
    ((rast.silhouette(mesh, Rm, T, sigma=sigma) * w).sum() + (rast2.silhouette(mesh, R2, T2, sigma=sigma2) * w2).sum()).backward()
    assert (g2 != 0).any() and torch.equal(v.grad, g1 + g2)
    # the cache: reused while nothing changed, a node per call, dropped after an in-place vertex update or another sigma
    a1, a2 = rast.silhouette(mesh, Rm, T, sigma=sigma), rast.silhouette(mesh, Rm, T, sigma=sigma)
    assert a1 is not a2 and a1.data_ptr() == a2.data_ptr() == alpha.data_ptr()
    with torch.no_grad():
        cached = rast.silhouette(mesh, Rm, T, sigma=sigma)
        assert not cached.requires_grad and rast.silhouette(mesh, Rm, T, sigma=sigma) is cached
    other = rast.silhouette(mesh, Rm, T, sigma=2 * sigma)
    assert not torch.equal(other.detach(), alpha.detach())
    with torch.no_grad():
        v.mul_(0.9)
        moved = rast.silhouette(mesh, Rm, T, sigma=sigma)
    assert torch.equal(moved.reshape(-1), ops.soft_silhouette(v.detach(), f, Rm, T, S, tanf, sigma, r)[0])
    assert not torch.equal(moved, alpha.detach())
    # nothing requires grad: no node, the cached tensor itself
    v0, f0, _, _, mesh0, rast0 = _mesh_and_rasterizer(key, False)
    b1 = rast0.silhouette(mesh0, Rm, T, sigma=sigma, blur_radius=r)
    assert not b1.requires_grad and b1.grad_fn is None and rast0.silhouette(mesh0, Rm, T, sigma=sigma, blur_radius=r) is b1
    assert torch.equal(b1.reshape(-1), a_ops)
    # the hard rasteriser's outputs are untouched by a silhouette call on the same rasteriser
    frags = rast0(mesh0, R=Rm, T=T)
    direct = ops.rasterize_mesh(v0, f0, ops.vertex_normals(v0, f0), Rm, T, S, tanf)
    assert torch.equal(frags.pix_to_face, direct[0]) and torch.equal(frags.zbuf, direct[1])


def test_a_silhouette_fit_grows_the_sphere():
    """40 Adam steps on the icosphere scaled by 0.8, at S = 32 with the sharp setting and the soft IoU alone: the hard IoU of
    the rasterised result against the target's hard coverage rises, the loss falls, and the device closes at least half the
    gap the float64 CPU loop closes (its start and end IoU are recorded in the case file)."""
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings, silhouette_iou
    target_v, start_v, f, Rm, T = R.fit_meshes()
    S = R.FIT_S
    sigma, r = R.setting(R.FIT_SETTING, S)
    faces = torch.from_numpy(f).to(DEV)
    Rm, T = Rm.to(DEV), T.to(DEV)

    def hard(verts):
        rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=S))
        with torch.no_grad():
            return rast(Meshes(verts=[verts.detach()], faces=[faces]), R=Rm, T=T).pix_to_face.reshape(-1) >= 0

    mask = hard(torch.from_numpy(target_v).to(DEV))
    verts = torch.from_numpy(start_v).to(DEV).requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[faces])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=S))
    iou0 = R.hard_iou(hard(verts).cpu(), mask.cpu())
    opt = torch.optim.Adam([verts], lr=R.FIT_LR)
    losses = []
    for _ in range(R.FIT_STEPS + 1):
        loss = silhouette_iou(rast.silhouette(mesh, Rm, T, sigma=sigma, blur_radius=r), mask.reshape(S, S))
        losses.append(float(loss.detach()))
        if len(losses) > R.FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    iou1 = R.hard_iou(hard(verts).cpu(), mask.cpu())
    gap = R.FIT_IOU_END - R.FIT_IOU_START
    print(f"silhouette fit: hard IoU {iou0:.4f} -> {iou1:.4f} (float64 reference {R.FIT_IOU_START:.4f} -> {R.FIT_IOU_END:.4f}), "
          f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert gap > 0.1
    assert iou1 > iou0 and losses[-1] < losses[0]
    assert iou1 - iou0 >= 0.5 * gap
