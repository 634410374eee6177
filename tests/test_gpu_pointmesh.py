"""GPU tests of the point-against-mesh unit (reni_tu_pointmesh.hip; ops.nearest_faces, ops.faces_nearest_points;
mesh_losses.nearest_surface, point_mesh_distance, geometry_scores(surface=True)) against the float64 reference of
tests/pointmesh_ref.py.

Bounds.  dist2 within K_D 2^-23 s of the reference's distance for the pair the device names, s = |p - a|^2 + |ab|^2 + |ac|^2 of
that face.  The named target is never compared with == in general (a point nearest a shared edge or vertex ties between the
adjacent faces): its reference distance must be within the two pairs' bounds of the reference's smallest, for EVERY query.  The
tap row names the face's vertices, its weights are within K_W 2^-23 s^2 / |ab x ac|^2 of the reference's for that pair.  Ties
that are exact in fp32 are compared with ==.  point_mesh_distance's value and gradients: max(K 2^-23 sum |terms|, 2e-5 max |ref|)
against the closed form at the device's matches and weights.  Every K is 4 x the worst ratio of the reference's float32 CPU
evaluation (R.K_*; DESIGN 4.4v has the device's figures).  Every test prints its figure before it asserts."""
import pytest
import torch

from tests import pointmesh_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
M = R.M


def _one(t):
    return torch.as_tensor(t).detach().reshape(1)


def _mesh_dev(v, f, grad=False):
    from reni_amd.mesh import Meshes
    return Meshes(verts=[v.to(DEV).clone().requires_grad_(grad)], faces=[f.to(DEV)])


def _run(by_face, p, v, f, **kw):
    from reni_amd import ops
    fn = ops.faces_nearest_points if by_face else ops.nearest_faces
    return tuple(t.cpu() for t in fn(p.to(DEV), v.to(DEV), f.to(DEV), **kw))


def _pairs(by_face, idx):
    """(point of every query, face of every query) from the device's idx"""
    q = torch.arange(idx.numel())
    return (idx, q) if by_face else (q, idx)


def _check_rows(by_face, p, v, f, got, label, weights=True):
    """what holds for every query that found a target: the tap row, the distance bound, the weight bound -> the reference's
    rows of the device's pairs"""
    d, idx, ti, tw = got
    T = p.shape[0] if by_face else f.shape[0]
    assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < T
    pi, fi = _pairs(by_face, idx)
    assert R.take_part(f, v.shape[0])[fi].all()
    row = R.pair_rows(p, v, f, pi, fi)
    assert torch.equal(ti[:, :3].long(), f[fi]) and (ti[:, 3:] == 0).all() and (tw[:, 3:] == 0).all()
    w = tw[:, :3].double()
    assert (tw >= 0).all() and float((w.sum(1) - 1).abs().max()) <= 4 * R.U
    rd = float(((d.double() - row["d"]).abs() / (R.U * row["s"]).clamp_min(1e-300)).max())
    ref_w = torch.stack([row["u"], row["v"], row["w"]], dim=1)
    rw = float(((w - ref_w).abs() / R.weight_bound(row, 1.0)[:, None]).max())
    print(f"{label}: worst |dist2 - d_ref| / (2^-23 s) = {rd:.4g} (K_D {R.K_D}); worst weight error / (2^-23 s^2 / |ab x ac|^2) = {rw:.4g} "
          f"(K_W {R.K_W})")
    assert torch.isfinite(d).all() and ((d.double() - row["d"]).abs() <= R.dist_bound(row)).all()
    if weights:
        assert ((w - ref_w).abs() <= R.weight_bound(row)[:, None]).all()
    return row


def _check_search(by_face, p, v, f, got, ref, label):
    row = _check_rows(by_face, p, v, f, got, label)
    assert (ref["idx"] >= 0).all()
    slack = row["d"] - ref["d"] - R.dist_bound(row) - R.dist_bound(ref)  # the named target is as near as the nearest, within the bounds
    differ = got[1] != ref["idx"]
    print(f"{label}: {int(differ.sum())} of {differ.numel()} named targets differ from the reference's; worst excess over the bounds "
          f"{float(slack.max()):.3g}")
    assert (slack <= 0).all()


# ----------------------------------------------------------------------------------------------------------- the searches
@pytest.mark.parametrize("key", R.SEARCH_CASES, ids=R.case_id)
def test_searches_match_the_float64_reference(key):
    p, v, f = R.search_inputs(key)
    by_face = key[1] == "fp"
    got = _run(by_face, p, v, f)
    _check_search(by_face, p, v, f, got, R.search_of(key), R.case_id(key))
    again = _run(by_face, p, v, f)
    assert all(torch.equal(a, b) for a, b in zip(got, again))  # two calls give identical bits


def test_all_seven_regions():
    p, v, f = R.region_case()
    ref = R.nearest_faces(p, v, f)
    for side in (p[:, 2] > 0, p[:, 2] < 0):
        assert sorted(set(ref["region"][side].tolist())) == list(range(7))  # the test cannot pass with a region left out
    got = _run(False, p, v, f)
    _check_search(False, p, v, f, got, ref, "regions")
    d, idx, ti, tw = got
    u, vv, w = tw[:, 0], tw[:, 1], tw[:, 2]
    reg = ref["region"]  # (the grid and the triangle are exact in fp32: the device is in the region the reference names)
    print("regions:", {R.REGIONS[k]: int((reg == k).sum()) for k in range(7)})
    assert (idx == 0).all()
    assert (u[reg == 0] == 1).all() and (vv[reg == 1] == 1).all() and (w[reg == 3] == 1).all()
    assert (w[reg == 2] == 0).all() and (vv[reg == 4] == 0).all() and (u[reg == 5] <= 4 * R.U).all()
    assert torch.equal(d.double(), ref["d"])  # quarter steps against a unit triangle: every distance is exact
    # the other direction on the same pairs: one face, its nearest grid point
    gf = _run(True, p, v, f)
    _check_search(True, p, v, f, gf, R.faces_nearest_points(p, v, f), "regions, by face")


def test_exact_ties_take_the_lowest_index():
    p = R.tie_points()
    want = torch.tensor([z * z + (2.0 if x == 3.0 else 0.0) for x, z in zip(p[:, 0].tolist(), p[:, 2].tolist())])
    for swapped in (False, True):
        for repeat in (1, 3000):
            f = R.tie_faces(swapped, repeat)
            if repeat == 1:  # both candidates give equal bits in the float32 CPU evaluation: the case is a tie
                rows = [R.pair_rows(p, R.SQUARE, f, torch.arange(12), torch.full((12,), k), R.F32)["d"] for k in (0, 1)]
                assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], want)
            d, idx, ti, tw = _run(False, p, R.SQUARE, f)
            print(f"split square, swapped {swapped}, x {repeat}: {int((idx != 0).sum())} of 12 points name another face than 0")
            assert torch.equal(d, want) and (idx == 0).all() and torch.equal(ti[:, :3].long(), f[:1].expand(12, 3))
    # the other direction: the cloud repeated, every face ties between the copies of four points at distance 0.25
    cloud = p.repeat(500, 1)
    for repeat in (1, 3000):
        f = R.tie_faces(False, repeat)
        cpu = R.faces_nearest_points(cloud, R.SQUARE, f[:2], R.F32)
        assert (cpu["idx"] == 2).all() and (cpu["d"] == 0.25).all()
        d, idx, ti, tw = _run(True, cloud, R.SQUARE, f)
        print(f"repeated cloud, {f.shape[0]} faces: {int((idx != 2).sum())} faces name another point than 2")
        assert (d == 0.25).all() and (idx == 2).all()


def test_slicing_never_changes_a_bit():
    from reni_amd import ops
    cases = [("big 64 x 20000", False) + R.search_inputs(("big", "pf", 64, 20000, 1.0)),
             ("big 64 x 20000 by face", True) + R.search_inputs(("big", "fp", 64, 20000, 1.0)),
             ("square x 3000", False, R.tie_points(), R.SQUARE, R.tie_faces(False, 3000)),
             ("cloud x 500 by face", True, R.tie_points().repeat(500, 1), R.SQUARE, R.tie_faces(False, 1))]
    for label, by_face, p, v, f in cases:
        fn = ops.faces_nearest_points if by_face else ops.nearest_faces
        p, v, f = p.to(DEV), v.to(DEV), f.to(DEV)
        got = {}
        for s in (1, 3, 7, 0, 10 ** 6):
            before = ops.launch_count()
            got[s] = fn(p, v, f, slices=s)
            launches = ops.launch_count() - before
            print(f"{label}: slices = {s}: {launches} launches")
            assert launches == (1 if s == 1 else 2)  # (every case here has more than one tile of targets)
        for s in (3, 7, 0, 10 ** 6):
            assert all(torch.equal(a, b) for a, b in zip(got[1], got[s])), (label, s)
    before = ops.launch_count()  # one tile of targets is not cut by the library
    ops.nearest_faces(p[:64], v, f[:2])
    ops.faces_nearest_points(p[:200], v, f)
    assert ops.launch_count() - before == 2


def test_faces_that_take_no_part_are_never_named():
    p, v, f = R.search_inputs(("big", "pf", 300, R.TILE + 1, 1.0))
    v, f = v.clone(), f.clone()
    V = v.shape[0]
    f[3, 1] = V            # out of range
    f[40, 0] = -1
    f[100, 2] = 2 ** 40
    f[7, 2] = f[7, 0]      # a repeated index
    f[R.TILE, 1] = f[R.TILE, 2]
    v[f[11]] = float("nan")            # a face of NaN vertices takes part by the rule and wins no comparison
    v[f[12, 0], 1] = float("inf")
    out = torch.tensor([3, 40, 100, 7, R.TILE, 11, 12])
    for s in (1, 5):
        got = _run(False, p, v, f, slices=s)
        assert not torch.isin(got[1], out).any()
        _check_search(False, p, v, f, got, R.nearest_faces(p, v, f), f"bad faces, slices = {s}")
        d, idx, ti, tw = _run(True, p, v, f, slices=s)
        assert (idx[out] == -1).all() and torch.isinf(d[out]).all() and (ti[out] == 0).all() and (tw[out] == 0).all()
        keep = torch.ones(f.shape[0], dtype=torch.bool)
        keep[out] = False
        ref = R.faces_nearest_points(p, v, f)
        assert (ref["idx"][out] == -1).all()
        sub = tuple(t[keep] for t in (d, idx, ti, tw))
        row = _check_rows(True, p, v, f[keep], sub, f"bad faces by face, slices = {s}")
        assert (row["d"] - ref["d"][keep] - R.dist_bound(row) - R.dist_bound({"s": ref["s"][keep]}) <= 0).all()
    # a NaN point finds no face, and no face names it
    q = p.clone()
    q[5, 2] = float("nan")
    d, idx, ti, tw = _run(False, q, v, f)
    assert int(idx[5]) == -1 and torch.isinf(d[5]) and (ti[5] == 0).all() and (tw[5] == 0).all() and (idx[torch.arange(300) != 5] >= 0).all()
    assert not (_run(True, q, v, f)[1] == 5).any()
    # nobody takes part: -1, +inf, zero taps, in both directions and through the combine kernel
    none = torch.tensor([[0, 0, 1], [V, 1, 2], [-1, 2, 3]]).repeat(200, 1)
    for by_face in (False, True):
        for s in (1, 4):
            d, idx, ti, tw = _run(by_face, p, v, none, slices=s)
            assert (idx == -1).all() and torch.isinf(d).all() and (d > 0).all() and (ti == 0).all() and (tw == 0).all()


def test_needles_and_faces_without_area_give_valid_weights():
    v, f = R.degenerate_mesh()
    p = R.cloud(400, 8)
    ref = R.nearest_faces(p, v, f)
    d, idx, ti, tw = _run(False, p, v, f)
    row = R.pair_rows(p, v, f, torch.arange(400), idx)
    print(f"degenerate mesh: faces named {sorted(set(idx.tolist()))}; worst dist2 - d_ref = {float((d.double() - ref['d']).max()):.3g}, "
          f"least {float((d.double() - ref['d']).min()):.3g}")
    assert (idx >= 0).all() and torch.isfinite(d).all() and (tw >= 0).all() and torch.isfinite(tw).all()
    assert float((tw[:, :3].double().sum(1) - 1).abs().max()) <= 4 * R.U and torch.equal(ti[:, :3].long(), f[idx])
    assert (d.double() >= ref["d"] - R.dist_bound(row)).all()
    for k in range(f.shape[0]):  # each face alone, so that every degenerate one is named: valid weights, a finite distance
        d, idx, ti, tw = _run(False, p[:64], v, f[k:k + 1])
        one = R.nearest_faces(p[:64], v, f[k:k + 1])
        row = R.pair_rows(p[:64], v, f[k:k + 1], torch.arange(64), torch.zeros(64, dtype=torch.int64))
        assert (idx == 0).all() and torch.isfinite(d).all() and (tw >= 0).all() and float((tw.double().sum(1) - 1).abs().max()) <= 4 * R.U
        assert (d.double() >= one["d"] - R.dist_bound(row)).all(), k
        fd, fi, fti, ftw = _run(True, p[:64], v, f[k:k + 1])
        assert int(fi[0]) >= 0 and torch.isfinite(fd).all() and (ftw >= 0).all() and abs(float(ftw.double().sum()) - 1) <= 4 * R.U


def test_nearest_surface():
    from reni_amd import mesh_losses
    p, v, f = R.pmd_inputs("ico1")
    mesh = _mesh_dev(v, f, grad=True)
    d, idx, bary, closest = mesh_losses.nearest_surface(p.to(DEV).requires_grad_(True), mesh)
    assert not d.requires_grad and not closest.requires_grad and tuple(bary.shape) == (300, 3) and tuple(closest.shape) == (300, 3)
    row = R.pair_rows(p, v, f, torch.arange(300), idx.cpu())
    err = (closest.cpu().double() - row["q"]).abs().max(1).values
    # three weights within their budget, each on a corner no farther than sqrt(s) from the others, and the fetch's roundings
    scale = 3 * R.weight_bound(row) * row["s"].sqrt() + 4 * R.U * v.abs().max().double()
    print(f"nearest_surface: worst closest-point error {float(err.max()):.3g}, worst / budget {float((err / scale).max()):.3g}")
    assert (err <= scale).all() and torch.equal(bary.cpu(), _run(False, p, v, f)[3][:, :3])


# ----------------------------------------------------------------------------------------------------- point_mesh_distance
def _pmd_dev(name, weights, up=1.0):
    from reni_amd import mesh_losses
    p, v, f = R.pmd_inputs(name)
    P = p.to(DEV).requires_grad_(True)
    mesh = _mesh_dev(v, f, grad=True)
    L = mesh_losses.point_mesh_distance(P, mesh, weights)
    (L * up).backward()
    return L.detach(), P.grad, mesh.verts_packed().grad


@pytest.mark.parametrize("weights", R.WEIGHTS, ids=lambda w: f"w{w[0]:g}-{w[1]:g}")
@pytest.mark.parametrize("name", R.PMD_CASES)
def test_point_mesh_distance_value_and_gradients_match_the_float64_reference(name, weights):
    p, v, f = R.pmd_inputs(name)
    L, gp, gv = _pmd_dev(name, weights, R.G_UP)
    by_point, by_face = _run(False, p, v, f), _run(True, p, v, f)  # the forward's own searches: the same bits
    part = R.take_part(f, v.shape[0])
    assert (by_point[1] >= 0).all() and torch.equal(by_face[1] >= 0, part)
    ref = R.value_and_grads(p, v, f, weights, (by_point[1], by_face[1]), (by_point[3][:, :3], by_face[3][:, :3]))
    rv = M.error_ratio(_one(L), _one(ref["value"]), _one(ref["value_terms"]))
    ov = M.over_bound(_one(L), _one(ref["value"]), _one(ref["value_terms"]), R.K_VALUE)
    rp = M.error_ratio(gp, R.G_UP * ref["gp"], R.G_UP * ref["gp_terms"])
    op = M.over_bound(gp, R.G_UP * ref["gp"], R.G_UP * ref["gp_terms"], R.K_GP)
    rg = M.error_ratio(gv, R.G_UP * ref["gv"], R.G_UP * ref["gv_terms"])
    og = M.over_bound(gv, R.G_UP * ref["gv"], R.G_UP * ref["gv_terms"], R.K_GV)
    print(f"{name} {weights}: value error / (2^-23 sum |terms|) = {rv:.4g}, / bound = {ov:.4g}; points.grad {rp:.4g}, / bound = {op:.4g}; "
          f"verts.grad {rg:.4g}, / bound = {og:.4g}")
    assert torch.isfinite(gp).all() and torch.isfinite(gv).all() and L.dim() == 0 and gp.shape == p.shape and gv.shape == v.shape
    assert ov <= 1.0 and op <= 1.0 and og <= 1.0
    if name == "on_vertices" or weights == (0.0, 0.0):
        assert float(L) == 0.0 and (gp == 0).all() and (gv == 0).all()  # exactly 0
    if name.startswith("star") and weights[1] > 0:
        assert (by_face[1] == 0).all()  # every face on point 0: a range of F entries in the gather
    L2, gp2, gv2 = _pmd_dev(name, weights, R.G_UP)
    assert torch.equal(L, L2) and torch.equal(gp, gp2) and torch.equal(gv, gv2)  # two calls give identical bits


def test_point_mesh_distance_gradient_only_for_what_requires_it_and_launch_counts():
    """a search is 1 launch, 2 when sliced; the forward is its two searches; the backward counts one chamfer_grad
    per input that requires grad when weights[1] > 0 (the fetches and the vertex gather are the texture unit's: not counted)"""
    from reni_amd import mesh_losses, ops
    p, v, f = R.pmd_inputs("teapot")  # 1000 points, 2464 faces: both searches are sliced
    counts = {}
    for label, grad_p, grad_v, weights in (("both", True, True, (1.0, 1.0)), ("points", True, False, (1.0, 1.0)),
                                           ("verts", False, True, (1.0, 1.0)), ("first term", True, True, (1.0, 0.0))):
        P = p.to(DEV).requires_grad_(grad_p)
        mesh = _mesh_dev(v, f, grad=grad_v)
        before = ops.launch_count()
        L = mesh_losses.point_mesh_distance(P, mesh, weights)
        fwd = ops.launch_count() - before
        L.backward()
        counts[label] = (fwd, ops.launch_count() - before - fwd)
        assert (P.grad is not None) == grad_p and (mesh.verts_packed().grad is not None) == grad_v
    print("point_mesh_distance launches (forward, backward):", counts)
    assert counts == {"both": (4, 2), "points": (4, 1), "verts": (4, 1), "first term": (2, 0)}
    with torch.no_grad():
        assert not mesh_losses.point_mesh_distance(p.to(DEV), _mesh_dev(v, f), (1.0, 1.0)).requires_grad
    small = R.pmd_inputs("ico1")  # 80 faces are one tile of targets: 1 launch; 300 points are two: the library slices, 2 launches
    before = ops.launch_count()
    mesh_losses.point_mesh_distance(small[0].to(DEV), _mesh_dev(*small[1:]))
    assert ops.launch_count() - before == 3


def test_verts_grad_accumulates_beside_the_regulariser_and_the_chamfer_distance():
    from reni_amd import mesh_losses
    p, v, f = R.pmd_inputs("ico1")
    P = p.to(DEV)
    u = torch.rand(500, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
    cloud = R.cloud(400, 9).to(DEV)

    def terms(mesh):
        return (mesh_losses.point_mesh_distance(P, mesh), mesh_losses.mesh_regularizer(mesh, edge=1.0, laplacian=0.5),
                mesh_losses.chamfer_distance(mesh_losses.sample_points_from_meshes(mesh, 500, u=u), cloud))

    alone = []
    for k in range(3):
        mesh = _mesh_dev(v, f, grad=True)
        terms(mesh)[k].backward()
        alone.append(mesh.verts_packed().grad.clone())
    mesh = _mesh_dev(v, f, grad=True)
    sum(terms(mesh)).backward()
    both = mesh.verts_packed().grad
    a, b, c = alone
    assert any(torch.equal(both, s) for s in ((a + b) + c, (a + c) + b, (b + c) + a))  # the three gradients' bits, in autograd's order


# ---------------------------------------------------------------------------------------------------------- geometry scores
def test_geometry_scores_by_samples_are_unchanged():
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    n = 1000
    pred, true = _mesh_dev(*R.ico(2)), ico_sphere(3, DEV)
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    for kw in ({}, {"surface": False}):
        s = mesh_losses.geometry_scores(pred, true, n=n, u=u, **kw)
        a, b = mesh_losses.sample_points_from_meshes(pred, n, u=u), mesh_losses.sample_points_from_meshes(true, n, u=u)
        d_p, d_t = ops.nearest_points(a, b)[0], ops.nearest_points(b, a)[0]
        assert torch.equal(s["chamfer_pred"], d_p.mean()) and torch.equal(s["chamfer_true"], d_t.mean())
        assert torch.equal(s["chamfer"], d_p.mean() + d_t.mean())
        assert torch.equal(s["precision@0.01"], (d_p.sqrt() <= 0.01).float().mean()) and torch.equal(s["recall@0.02"], (d_t.sqrt() <= 0.02).float().mean())
    gens = [torch.Generator(device=DEV).manual_seed(4) for _ in range(2)]
    s1, s2 = mesh_losses.geometry_scores(pred, true, n=n, generator=gens[0]), mesh_losses.geometry_scores(pred, true, n=n, generator=gens[1], surface=False)
    assert s1.keys() == s2.keys() and all(torch.equal(s1[k], s2[k]) for k in s1)


def test_geometry_scores_against_the_surface():
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    n = 2000
    unit = ico_sphere(3, DEV)
    v, f = unit.verts_packed().cpu(), unit.faces_packed().cpu()
    # a mesh against itself, independent sample sets: the sample-based score has the sampling term, the surface-based none
    twin = torch.Generator(device=DEV).manual_seed(4)
    u1, u2 = torch.rand(n, 3, device=DEV, generator=twin), torch.rand(n, 3, device=DEV, generator=twin)
    by_samples = mesh_losses.geometry_scores(unit, unit, n=n, generator=torch.Generator(device=DEV).manual_seed(4))
    s = mesh_losses.geometry_scores(unit, unit, n=n, generator=torch.Generator(device=DEV).manual_seed(4), surface=True)
    assert s.keys() == by_samples.keys() and not any(t.requires_grad for t in s.values())
    limit = 0.0
    for uu in (u1, u2):  # the samples the call drew, and the bound of each against the nearest face
        pts = mesh_losses.sample_points_from_meshes(unit, n, u=uu).cpu()
        ref = R.nearest_faces(pts, v, f)
        limit += float((ref["d"] + R.dist_bound(ref)).mean())
    limit *= 1 + n * 2.0 ** -24  # (the float32 mean of n terms)
    print(f"unit sphere against itself, n = {n}: chamfer by samples {float(by_samples['chamfer']):.4g}, against the surface "
          f"{float(s['chamfer']):.4g} (at most the summed distance bounds {limit:.4g})")
    assert 0.0 <= float(s["chamfer"]) <= limit < 1e-3 * float(by_samples["chamfer"])  # the sampling term is what is removed
    assert float(by_samples["chamfer"]) > 1e-4 and float(s["fscore@0.01"]) == 1.0 and float(s["precision@0.02"]) == 1.0
    # against the sphere grown by 1.05: the float64 reference on the same samples
    grown = Meshes(verts=[unit.verts_packed() * 1.05], faces=[unit.faces_packed()])
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    s = mesh_losses.geometry_scores(unit, grown, n=n, thresholds=(0.01, 0.3), u=u, surface=True)
    gv = grown.verts_packed().cpu()
    for key, pts, tv in (("chamfer_pred", mesh_losses.sample_points_from_meshes(unit, n, u=u).cpu(), gv),
                         ("chamfer_true", mesh_losses.sample_points_from_meshes(grown, n, u=u).cpu(), v)):
        ref = R.nearest_faces(pts, tv, f)
        want, bound = float(ref["d"].mean()), float(R.dist_bound(ref).mean()) + n * 2.0 ** -24 * float(ref["d"].mean())
        print(f"{key}: {float(s[key]):.8g}, float64 {want:.8g}, |difference| / bound = {abs(float(s[key]) - want) / bound:.3g}")
        assert abs(float(s[key]) - want) <= bound and 0.04 ** 2 < want < 0.06 ** 2
    assert abs(float(s["chamfer"]) - float(s["chamfer_pred"]) - float(s["chamfer_true"])) <= 1e-6 * float(s["chamfer"])
    assert float(s["fscore@0.01"]) == 0.0 and float(s["precision@0.01"]) == 0.0 and float(s["recall@0.01"]) == 0.0
    assert float(s["fscore@0.3"]) == 1.0


# ------------------------------------------------------------------------------------------------------------------ a fit
def test_a_sphere_is_pulled_onto_a_scan():
    """a level-2 sphere of radius 0.5 towards samples of DESIGN 4.4u's ellipsoid with point_mesh_distance alone: no resampling"""
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    target = ico_sphere(3, DEV)
    cloud = mesh_losses.sample_points_from_meshes(
        Meshes(verts=[target.verts_packed() * torch.tensor(R.ELLIPSOID, device=DEV)], faces=[target.faces_packed()]), R.FIT_POINTS,
        generator=torch.Generator(device=DEV).manual_seed(0))
    start = ico_sphere(2, DEV)
    mesh = Meshes(verts=[(start.verts_packed() * 0.5).clone().requires_grad_(True)], faces=[start.faces_packed()])
    verts = mesh.verts_packed()
    opt = torch.optim.Adam([verts], lr=R.FIT_LR)
    first = None
    for step in range(R.FIT_STEPS):
        loss = mesh_losses.point_mesh_distance(cloud, mesh)
        first = float(loss) if first is None else first
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"fit: point_mesh_distance {first:.5f} -> {float(loss):.5f}")
    assert float(loss) < 0.5 * first and torch.isfinite(verts).all()  # (the 1/2 tells descent from none)
