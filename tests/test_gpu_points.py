"""GPU tests of the point-cloud unit (reni_tu_points.hip; ops.nearest_points, chamfer_grad, mesh_sample_table,
mesh_sample_points; reni_amd/mesh_losses.py) against the float64 reference of tests/points_ref.py.

Bounds.  dist2 within 4 * 2^-23 d_ref (five roundings of relative 2^-24 on a sum of non-negative terms); idx equal to the
reference's except at undecided queries (best and second best within 8 * 2^-23 d_second), where any j inside that margin may
be named -- the random cases have none.  Ties that are exact in fp32 are compared with ==.  The chamfer value and gradients,
the sampled points and their vertex gradient: max(K 2^-23 sum |terms|, 2e-5 max |ref|), K = 4 x the worst ratio of the
reference's float32 CPU evaluation (P.K_*; DESIGN 4.4u has the device's figures).  Rows that touch an undecided match or sample
are left out of the bound and checked finite.  Every test prints its figure before it asserts."""
import pytest
import torch

from tests import points_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
M = P.M


def _one(t):
    return torch.as_tensor(t).detach().reshape(1)


# ---------------------------------------------------------------------------------------------------------- nearest points
def _check_nearest(x, y, d, i, ref, label):
    d, i = d.cpu().double(), i.cpu()
    assert d.shape == ref["d"].shape and i.dtype == torch.int64 and int(i.min()) >= 0 and int(i.max()) < y.shape[0]
    err = ((d - ref["d"]).abs() / ref["d"].clamp_min(1e-300)).max() / P.U if float(ref["d"].max()) > 0 else 0.0
    wrong = i != ref["idx"]
    print(f"{label}: worst |dist2 - ref| / (2^-23 ref) = {float(err):.4g} (bound {P.DIST_K}); {int(wrong.sum())} indices differ, "
          f"{int(ref['und'].sum())} queries undecided")
    assert ((d - ref["d"]).abs() <= P.DIST_K * P.U * ref["d"]).all()
    assert not (wrong & ~ref["und"]).any()
    if wrong.any():  # an undecided query may name any j within the margin
        dj = ((x.double()[wrong] - y.double()[i[wrong]]) ** 2).sum(1)
        assert (dj - ref["d"][wrong] <= P.MARGIN_K * P.U * ref["d2"][wrong]).all()


@pytest.mark.parametrize("key", P.NN_CASES, ids=P.case_id)
def test_nearest_points_match_the_float64_reference(key):
    from reni_amd import ops
    x, y = P.nn_clouds(key)
    d, i = ops.nearest_points(x.to(DEV), y.to(DEV))
    _check_nearest(x, y, d, i, P.nearest_of(key), P.case_id(key))
    d2, i2 = ops.nearest_points(x.to(DEV), y.to(DEV))
    assert torch.equal(d, d2) and torch.equal(i, i2)


def test_exact_ties_take_the_lowest_index():
    from reni_amd import ops
    x, y = P.lattice()
    ref = P.nearest(x, y)
    d, i = ops.nearest_points(x.to(DEV), y.to(DEV))
    print(f"lattice: {int((i.cpu() != ref['idx']).sum())} of {x.shape[0]} indices differ from the lowest of the tied ones")
    assert (d.cpu() == 0.75).all() and torch.equal(i.cpu(), ref["idx"])
    # y holds copies of x among other points: distance exactly 0, and the named point is the copy
    a, b = P.cloud("cube", 700, 31), P.cloud("cube", 1500, 32)
    yy = torch.cat([b[:900], a, b[900:]])
    d, i = ops.nearest_points(a.to(DEV), yy.to(DEV))
    assert (d == 0).all() and torch.equal(yy[i.cpu()], a) and torch.equal(i.cpu(), 900 + torch.arange(700))
    # the same copy twice: the lower index
    d, i = ops.nearest_points(a.to(DEV), torch.cat([a, a]).to(DEV))
    assert (d == 0).all() and torch.equal(i.cpu(), torch.arange(700))
    # x is y
    z = a.to(DEV)
    d, i = ops.nearest_points(z, z)
    assert (d == 0).all() and torch.equal(i.cpu(), torch.arange(700))


def test_slicing_never_changes_a_bit():
    from reni_amd import ops
    for label, (x, y) in (("64x20000", P.nn_clouds(("cube", 64, 20000, 1.0))), ("lattice", P.lattice())):
        x, y = x.to(DEV), y.to(DEV)
        got = {}
        for s in (1, 7, 0, 3, 10 ** 6):
            before = ops.launch_count()
            got[s] = ops.nearest_points(x, y, slices=s)
            launches = ops.launch_count() - before
            print(f"{label}: slices = {s}: {launches} launches")
            # (the lattice's 729 targets are less than one tile: the library's own choice is one slice)
            assert launches == (1 if s == 1 or (s == 0 and label == "lattice") else 2)
        for s in (7, 0, 3, 10 ** 6):
            assert torch.equal(got[1][0], got[s][0]) and torch.equal(got[1][1], got[s][1]), (label, s)
    # the library slices (64, 20000) by itself; one tile of targets is not cut
    before = ops.launch_count()
    ops.nearest_points(x[:64], y[:100])
    assert ops.launch_count() - before == 1


def test_nan_and_infinite_coordinates_fall_back_to_index_zero():
    from reni_amd import ops
    x = P.cloud("cube", 70, 41).clone()
    y = P.cloud("cube", 1500, 42).clone()
    x[3, 1] = float("nan")
    y[7] = float("nan")       # a NaN target wins no comparison
    y[1200, 0] = float("inf")
    ref = P.nearest(x[torch.arange(70) != 3], y[torch.isfinite(y).all(1)])
    for s in (1, 5):
        d, i = ops.nearest_points(x.to(DEV), y.to(DEV), slices=s)
        d, i = d.cpu(), i.cpu()
        assert int(i[3]) == 0 and torch.isnan(d[3])  # what d(3, 0) computes
        keep = torch.arange(70) != 3
        assert not (i[keep] == 7).any() and not (i[keep] == 1200).any() and torch.isfinite(d[keep]).all()
        assert ((d[keep].double() - ref["d"]).abs() <= P.DIST_K * P.U * ref["d"]).all()
    big = torch.full((5, 3), 3e38)
    d, i = ops.nearest_points(big.to(DEV), (-big).to(DEV))  # every d overflows to +inf: no comparison succeeds
    assert (i == 0).all() and torch.isinf(d).all()


# ----------------------------------------------------------------------------------------------------------------- chamfer
def _chamfer_dev(name, weights, up=1.0):
    from reni_amd import mesh_losses
    x, y = P.ch_clouds(name)
    X, Y = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    L = mesh_losses.chamfer_distance(X, Y, weights)
    (L * up).backward()
    return L.detach(), X.grad, Y.grad


@pytest.mark.parametrize("weights", P.WEIGHTS, ids=lambda w: f"w{w[0]:g}-{w[1]:g}")
@pytest.mark.parametrize("name", P.CH_CASES)
def test_chamfer_value_and_gradients_match_the_float64_reference(name, weights):
    ref = P.chamfer_of(name, weights)
    L, gx, gy = _chamfer_dev(name, weights, P.G_UP)
    kx, ky = ~ref["und_x"], ~ref["und_y"]
    rv = M.error_ratio(_one(L), _one(ref["value"]), _one(ref["value_terms"]))
    ov = M.over_bound(_one(L), _one(ref["value"]), _one(ref["value_terms"]), P.K_VALUE)
    rx = M.error_ratio(gx, P.G_UP * ref["gx"], P.G_UP * ref["gx_terms"], kx)
    ry = M.error_ratio(gy, P.G_UP * ref["gy"], P.G_UP * ref["gy_terms"], ky)
    ox = M.over_bound(gx, P.G_UP * ref["gx"], P.G_UP * ref["gx_terms"], P.K_GRAD, kx)
    oy = M.over_bound(gy, P.G_UP * ref["gy"], P.G_UP * ref["gy_terms"], P.K_GRAD, ky)
    print(f"{name} {weights}: value error / (2^-23 sum |terms|) = {rv:.4g}, / bound = {ov:.4g}; grad_x {rx:.4g}, / bound = {ox:.4g}; "
          f"grad_y {ry:.4g}, / bound = {oy:.4g}; undecided rows {int((~kx).sum())} + {int((~ky).sum())}")
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all() and L.dim() == 0
    assert ov <= 1.0 and ox <= 1.0 and oy <= 1.0
    if name == "coincident" or weights == (0.0, 0.0):
        assert float(L) == 0.0 and (gx == 0).all() and (gy == 0).all()  # exactly 0
    L2, gx2, gy2 = _chamfer_dev(name, weights, P.G_UP)
    assert torch.equal(L, L2) and torch.equal(gx, gx2) and torch.equal(gy, gy2)  # two calls give identical bits


def test_chamfer_gradient_only_for_what_requires_it_and_with_g_one():
    from reni_amd import mesh_losses, ops
    x, y = (t.to(DEV) for t in P.ch_clouds("r129"))
    ref = P.chamfer_of("r129")
    X = x.clone().requires_grad_(True)
    before = ops.launch_count()
    L = mesh_losses.chamfer_distance(X, y)
    fwd = ops.launch_count() - before
    L.backward()
    bwd = ops.launch_count() - before - fwd
    print(f"chamfer_distance r129: {fwd} launches forward, {bwd} backward for one cloud")
    assert fwd == 2 and bwd == 1  # two searches (one slice each here); one gather for the one cloud that requires grad
    assert M.over_bound(X.grad, ref["gx"], ref["gx_terms"], P.K_GRAD) <= 1.0
    with torch.no_grad():
        assert not mesh_losses.chamfer_distance(x, y).requires_grad
    d, i = mesh_losses.nearest_points(X, y)
    assert not d.requires_grad and torch.equal(i.cpu(), ref["matches"][0]["idx"])
    # ops.chamfer_grad with the roles swapped is grad_y
    nx, ny = ref["matches"]
    gy = ops.chamfer_grad(y, x, ny["idx"].to(DEV), ops.chamfer_table(nx["idx"].to(DEV), y.shape[0]), (1.0, 1.0))
    assert M.over_bound(gy, ref["gy"], ref["gy_terms"], P.K_GRAD) <= 1.0
    # a malformed table adds nothing and is never an address
    order, offsets = ops.chamfer_table(ny["idx"].to(DEV), x.shape[0])
    bad_order = order.clone()
    bad_order[::3] = 10 ** 12
    bad_order[1::3] = -5
    bad_off = offsets.clone()
    bad_off[5] = -10 ** 12
    bad_off[9] = 10 ** 12
    g = ops.chamfer_grad(x, y, torch.full((x.shape[0],), 10 ** 12, dtype=torch.int64, device=DEV), (bad_order, bad_off), (1.0, 1.0))
    assert torch.isfinite(g).all()


# ---------------------------------------------------------------------------------------------------------------- sampling
def _mesh_dev(key, grad=False):
    from reni_amd.mesh import Meshes
    v, f = P.sample_mesh(key)
    return Meshes(verts=[v.to(DEV).requires_grad_(grad)], faces=[f.to(DEV)])


@pytest.mark.parametrize("key", P.SAMPLE_MESHES, ids=P.case_id)
def test_samples_match_the_float64_reference(key):
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh_losses import mesh_regularizer
    v, f = P.sample_mesh(key)
    u = P.sample_u()
    up = P.sample_upstream(u.shape[0])
    ref = P.sample(v, f, u, up)
    table = ops.mesh_sample_table(v.to(DEV), f.to(DEV)).cpu()
    area, cdf = table[0].double(), table[1]
    assert ((area - ref["area"]).abs() <= 8 * P.U * ref["area"]).all() and ((area > 0) == (ref["area"] > 0)).all()
    assert (cdf[1:] >= cdf[:-1]).all() and float(cdf[-1]) == 1.0 and float((cdf.double() - ref["cdf"]).abs().max()) <= P.CDF_BUDGET
    flat = torch.cat([cdf[:1] == 0, cdf[1:] == cdf[:-1]])
    assert flat[area == 0].all()  # a face without area is a flat step: never chosen
    mesh = _mesh_dev(key, grad=True)
    pts, face = mesh_losses.sample_points_from_meshes(mesh, u.shape[0], u=u.to(DEV), return_faces=True)
    idx, wgt, face2 = ops.mesh_sample_points(f.to(DEV), table.to(DEV), u.to(DEV), v.shape[0])
    face, wgt, idx = face.cpu(), wgt.cpu(), idx.cpu()
    assert torch.equal(face, face2.cpu())
    wrong = face != ref["face"]
    print(f"{P.case_id(key)}: {int(wrong.sum())} faces differ, {int(ref['und'].sum())} of {u.shape[0]} samples undecided")
    assert not (wrong & ~ref["und"]).any() and float(ref["und"].float().mean()) <= P.UNDECIDED_CAP
    assert (area[face] > 0).all() and ref["part"][face].all()
    assert torch.equal(idx[:, :3].long(), f[face]) and (idx[:, 3:] == 0).all() and (wgt[:, 3:] == 0).all()
    assert float((wgt[:, :3].double() - ref["w"]).abs().max()) <= P.WEIGHT_BOUND and (wgt >= 0).all()
    keep = ~wrong
    rp = M.error_ratio(pts, ref["points"], ref["points_terms"], keep)
    op = M.over_bound(pts, ref["points"], ref["points_terms"], P.K_POINTS, keep)
    (pts * up.to(DEV)).sum().backward()
    g1 = mesh.verts_packed().grad.clone()
    rows = ~ref["und_rows"] if wrong.any() else torch.ones(v.shape[0], dtype=torch.bool)
    rg = M.error_ratio(g1, ref["gv"], ref["gv_terms"], rows)
    og = M.over_bound(g1, ref["gv"], ref["gv_terms"], P.K_VGRAD, rows)
    print(f"{P.case_id(key)}: points error / (2^-23 sum |terms|) = {rp:.4g}, / bound = {op:.4g}; verts.grad {rg:.4g}, / bound = {og:.4g}")
    assert op <= 1.0 and og <= 1.0 and torch.isfinite(g1).all()
    # a second call: identical bits; and beside the regulariser's gradient in one backward
    mesh2 = _mesh_dev(key, grad=True)
    pts2 = mesh_losses.sample_points_from_meshes(mesh2, u.shape[0], u=u.to(DEV))
    reg = mesh_regularizer(mesh2, edge=1.0, laplacian=0.5)
    ((pts2 * up.to(DEV)).sum() + reg).backward()
    assert torch.equal(pts, pts2)
    mesh3 = _mesh_dev(key, grad=True)
    mesh_regularizer(mesh3, edge=1.0, laplacian=0.5).backward()
    both = mesh2.verts_packed().grad
    assert torch.equal(both, g1 + mesh3.verts_packed().grad) or torch.equal(both, mesh3.verts_packed().grad + g1)


def test_sample_table_across_chunks_and_tiles():
    """F past one chunk of 1024 faces, and past 256 chunks (the second tile of the chunk scan): the CDF against float64"""
    from reni_amd import ops
    from reni_amd.mesh import ico_sphere
    g = torch.Generator().manual_seed(5)
    for label, (v, f) in (("ico4", (ico_sphere(4).verts_packed(), ico_sphere(4).faces_packed())),
                          ("soup", (torch.rand(3 * 263169, 3, generator=g), torch.arange(3 * 263169).reshape(-1, 3)))):
        f = f.clone()
        f[100] = torch.tensor([0, 0, 1])         # takes no part
        f[f.shape[0] - 1] = torch.tensor([5, 6, 5])
        f[2048] = -1
        a, part = P.areas(v, f)
        ref = torch.cumsum(a, 0) / a.sum()
        table = ops.mesh_sample_table(v.to(DEV), f.to(DEV)).cpu()
        cdf = table[1]
        err = float((cdf.double() - ref).abs().max())
        print(f"{label}: F = {f.shape[0]}, worst |cdf - float64| = {err:.3g} (budget {P.CDF_BUDGET:.3g})")
        assert (cdf[1:] >= cdf[:-1]).all() and float(cdf[-1]) == 1.0 and err <= P.CDF_BUDGET
        assert ((table[0] > 0) == (a > 0)).all() and cdf[100] == cdf[99] and cdf[2048] == cdf[2047]
        last = int((a > 0).nonzero().max())
        assert (cdf[last:] == 1.0).all() and cdf[last - 1] < 1.0
        u = torch.rand(4096, 3, generator=g)
        u[0, 0], u[1, 0] = 0.0, 1.0 - 2.0 ** -24
        idx, wgt, face = ops.mesh_sample_points(f.to(DEV), table.to(DEV), u.to(DEV), v.shape[0])
        face = face.cpu()
        # A step of this CDF is narrower than (ico4: comparable to) the budget, so the face is checked against the definition
        # on the DEVICE'S OWN table -- the number of its entries <= u0 -- which is exact; the table itself is bounded above.
        want = torch.searchsorted(cdf, u[:, 0].contiguous(), right=True).clamp_max(f.shape[0] - 1)
        assert torch.equal(face, want) and (a[face] > 0).all() and int(face[0]) == int((a > 0).nonzero().min()) and int(face[1]) == last
        t2 = ops.mesh_sample_table(v.to(DEV), f.to(DEV)).cpu()
        assert torch.equal(table, t2)


def test_a_mesh_without_area_gives_exact_zeros():
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh import Meshes
    v = torch.tensor([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [float("nan"), 0, 0]])
    f = torch.tensor([[0, 1, 2], [1, 2, 3], [0, 0, 1], [0, 1, 9], [0, 1, 4]])  # collinear, repeated, out of range, not finite
    table = ops.mesh_sample_table(v.to(DEV), f.to(DEV))
    assert (table == 0).all()
    m = Meshes(verts=[v.to(DEV).requires_grad_(True)], faces=[f.to(DEV)])
    pts, face = mesh_losses.sample_points_from_meshes(m, 300, generator=torch.Generator(device=DEV).manual_seed(1), return_faces=True)
    assert (pts == 0).all() and (face == 0).all() and pts.shape == (300, 3)
    pts.sum().backward()
    assert (m.verts_packed().grad == 0).all()


def test_the_area_table_follows_the_vertices():
    from reni_amd import mesh_losses
    mesh = _mesh_dev(("two", 0))
    first = mesh._sample_table()
    assert mesh._sample_table() is first
    u = P.sample_u().to(DEV)
    a = mesh_losses.sample_points_from_meshes(mesh, u.shape[0], u=u)
    with torch.no_grad():
        mesh.verts_packed()[3:] *= 0.01   # the second face shrinks in place: areas 1 : 0.0003
    assert mesh._sample_table() is not first
    pts, face = mesh_losses.sample_points_from_meshes(mesh, u.shape[0], u=u, return_faces=True)
    assert float((face == 0).float().mean()) > 0.99 and not torch.equal(a, pts)
    gen = torch.Generator(device=DEV).manual_seed(3)
    p1 = mesh_losses.sample_points_from_meshes(mesh, 64, generator=gen)
    p2 = mesh_losses.sample_points_from_meshes(mesh, 64, generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(p1, p2) and p1.shape == (64, 3)
    p3 = mesh_losses.sample_points_from_meshes(mesh, 64, generator=torch.Generator().manual_seed(3))  # a CPU generator draws on the CPU
    assert p3.device == p1.device


# ---------------------------------------------------------------------------------------------------------- geometry scores
def test_geometry_scores():
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    n = 2000
    unit = ico_sphere(3, DEV)
    grown = Meshes(verts=[unit.verts_packed() * 1.05], faces=[unit.faces_packed()])
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    s = mesh_losses.geometry_scores(unit, unit, n=n, u=u)
    print({k: float(v) for k, v in s.items()})
    assert float(s["chamfer"]) == 0.0 and float(s["chamfer_pred"]) == 0.0 and float(s["chamfer_true"]) == 0.0
    for t in ("0.01", "0.02"):
        assert float(s[f"fscore@{t}"]) == 1.0 and float(s[f"precision@{t}"]) == 1.0 and float(s[f"recall@{t}"]) == 1.0
    # independent samples of both: the reference's sampling term is the chamfer of two sample sets of the SAME surface
    gen = torch.Generator(device=DEV).manual_seed(4)
    twin = torch.Generator(device=DEV).manual_seed(4)
    u1, u2 = torch.rand(n, 3, device=DEV, generator=twin).cpu(), torch.rand(n, 3, device=DEV, generator=twin).cpu()
    v, f = unit.verts_packed().cpu(), unit.faces_packed().cpu()
    p1, p2 = P.sample(v, f, u1)["points"], P.sample(v, f, u2)["points"]
    D = P.dist_matrix(p1, p2)
    sampling = float(D.min(1).values.mean() + D.min(0).values.mean())
    s = mesh_losses.geometry_scores(unit, grown, n=n, thresholds=(0.01, 0.02, 0.3), generator=gen)
    lo, hi = 0.05 ** 2 * 2 * 0.9, 0.05 ** 2 * 2 * 1.1 + sampling
    print({k: float(v) for k, v in s.items()}, f"bounds {lo:.6g} .. {hi:.6g} (sampling term {sampling:.6g})")
    assert lo <= float(s["chamfer"]) <= hi
    assert abs(float(s["chamfer"]) - float(s["chamfer_pred"]) - float(s["chamfer_true"])) <= 1e-6 * float(s["chamfer"])
    assert float(s["fscore@0.01"]) == 0.0 and float(s["precision@0.01"]) == 0.0 and float(s["recall@0.01"]) == 0.0
    assert float(s["fscore@0.3"]) == 1.0
    assert not any(v.requires_grad for v in s.values())
    # the same u for both: every sample has its scaled twin, so no sampling term
    s = mesh_losses.geometry_scores(unit, grown, n=n, u=u)
    assert lo <= float(s["chamfer"]) <= 0.05 ** 2 * 2 * 1.1


def test_a_sphere_is_pulled_towards_a_cloud():
    """the README's loop in small: an icosphere towards the samples of a larger one, with the regulariser beside the chamfer"""
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    target = ico_sphere(3, DEV)
    cloud = mesh_losses.sample_points_from_meshes(
        Meshes(verts=[target.verts_packed() * torch.tensor([1.5, 1.0, 0.7], device=DEV)], faces=[target.faces_packed()]), 3000,
        generator=torch.Generator(device=DEV).manual_seed(0))
    start = ico_sphere(2, DEV)
    verts = (start.verts_packed() * 0.5).clone().requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[start.faces_packed()])
    verts = mesh.verts_packed()
    opt = torch.optim.Adam([verts], lr=0.02)
    gen = torch.Generator(device=DEV).manual_seed(1)
    first = None
    for step in range(60):
        pts = mesh_losses.sample_points_from_meshes(mesh, 2000, generator=gen)
        chamfer = mesh_losses.chamfer_distance(pts, cloud)
        loss = chamfer + mesh_losses.mesh_regularizer(mesh, edge=0.1, laplacian=0.1)
        first = float(chamfer) if first is None else first
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"fit: chamfer {first:.5f} -> {float(chamfer):.5f}")
    # a fit that works at all halves the distances (a quarter of the squared ones) on the way from radius 0.5 to the ellipsoid
    assert float(chamfer) < 0.25 * first and torch.isfinite(verts).all()


# ------------------------------------------------------------------------------------------------------------ launch counts
def test_launch_counts_are_the_header_s():
    from reni_amd import ops
    x, y = (t.to(DEV) for t in P.ch_clouds("cube"))
    v, f = (t.to(DEV) for t in P.sample_mesh(("ico", 16)))
    rose = {}

    def call(name, fn, *args, **kw):
        before = ops.launch_count()
        out = fn(*args, **kw)
        rose[name] = ops.launch_count() - before
        return out

    _, ixy = call("nearest_points_one_slice", ops.nearest_points, x, y, slices=1)
    call("nearest_points_sliced", ops.nearest_points, x, y, slices=4)
    _, iyx = ops.nearest_points(y, x)
    call("chamfer_grad", ops.chamfer_grad, x, y, ixy, ops.chamfer_table(iyx, x.shape[0]))
    table = call("mesh_sample_table", ops.mesh_sample_table, v, f)
    call("mesh_sample_points", ops.mesh_sample_points, f, table, P.sample_u().to(DEV), v.shape[0])
    print(rose)
    assert rose == {"nearest_points_one_slice": 1, "nearest_points_sliced": 2, "chamfer_grad": 1, "mesh_sample_table": 3,
                    "mesh_sample_points": 1}
