"""GPU tests of the cloud-neighbourhood unit (reni_tu_knn.hip; ops.knn_points, ops.cloud_normals) and of the normals in
reni_amd/mesh_losses.py (knn_points, estimate_normals, sample_points_from_meshes(return_normals=True),
chamfer_distance(x_normals=, y_normals=), geometry_scores(normals=True)) against the float64 reference of
tests/cloud_normals_ref.py.

Bounds.  dist2 within DIST_K 2^-23 d_ref (points_ref's constant: the same expression); idx equal to the reference's except in
rows where two consecutive reference distances among the first K + 1 lie within MARGIN_K 2^-23 of each other, which may
permute inside that margin.  Ties that are exact in fp32 are compared with ==.  Eigenvalues, evaluated by the reference on the
DEVICE'S OWN neighbour lists, within K_E 2^-23 l2; the angle to the reference normal within K_N 2^-23 l2 / (l1 - l0); a point
with (l1 - l0) / l2 < 1e-3 may be left out (capped at 1 %).  Sampled normals, the chamfer normal term and their gradients:
max(K 2^-23 sum |terms|, 2e-5 max |ref|).  Every K is 4 x the worst ratio of the reference's float32 CPU evaluation (C.K_*).
Every test prints its figure before it asserts."""
import math

import pytest
import torch

from tests import cloud_normals_ref as C
from tests import points_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
M = P.M
U = C.U


def _one(t):
    return torch.as_tensor(t).detach().reshape(1)


# ------------------------------------------------------------------------------------------------------------------- k-NN
def _check_knn(x, y, K, d, i, ref, label):
    d, i = d.cpu().double(), i.cpu()
    rd, ri = ref["d"][:, :K], ref["idx"][:, :K]
    assert tuple(d.shape) == (x.shape[0], K) == tuple(i.shape) and i.dtype == torch.int64
    assert int(i.min()) >= -1 and int(i.max()) < y.shape[0]
    filled = ri >= 0
    err = float(((d - rd).abs() / rd.clamp_min(1e-300))[filled].max()) / U if filled.any() else 0.0
    wrong = (i != ri).any(1)
    print(f"{label}: worst |dist2 - ref| / (2^-23 ref) = {err:.4g} (bound {C.DIST_K}); {int(wrong.sum())} rows differ, "
          f"{int(ref['und'].sum())} of {wrong.numel()} rows undecided")
    assert torch.equal(i >= 0, filled) and torch.isinf(d[~filled]).all() and (d[~filled] > 0).all()
    assert ((d - rd).abs() <= C.DIST_K * U * rd)[filled].all()
    assert not (wrong & ~ref["und"]).any()
    if wrong.any():  # an undecided row may permute inside the margin
        own = ((x.double()[wrong][:, None, :] - y.double()[i[wrong].clamp_min(0)]) ** 2).sum(-1)
        ok = ((own - rd[wrong]).abs() <= C.MARGIN_K * U * torch.maximum(own, rd[wrong])) | ~filled[wrong]
        assert ok.all()


@pytest.mark.parametrize("key", C.KNN_CASES, ids=C.case_id)
def test_knn_points_match_the_float64_reference(key):
    from reni_amd import ops
    x, y = C.knn_clouds(key)
    K = key[3]
    X, Y = x.to(DEV), y.to(DEV)
    d, i = ops.knn_points(X, Y, K)
    _check_knn(x, y, K, d, i, C.knn_of(key), C.case_id(key))
    d2, i2 = ops.knn_points(X, Y, K)
    assert torch.equal(d, d2) and torch.equal(i, i2)  # two calls give identical bits
    # column 0 has reni_nearest_points' bits wherever slot 0 is filled (here: everywhere)
    d1, i1 = ops.nearest_points(X, Y)
    assert (i[:, 0] >= 0).all() and torch.equal(d[:, 0], d1) and torch.equal(i[:, 0], i1)


def test_exact_ties_go_by_the_lowest_index():
    from reni_amd import ops
    x, y = C.lattice()
    ref = C.knn(x, y, 8)
    d, i = ops.knn_points(x.to(DEV), y.to(DEV), 8)
    print(f"lattice: {int((i.cpu() != ref['idx'][:, :8]).sum())} of {i.numel()} indices differ from the lexicographic order")
    assert torch.equal(d.cpu().double(), ref["d"][:, :8]) and torch.equal(i.cpu(), ref["idx"][:, :8])
    d1, i1 = ops.nearest_points(x.to(DEV), y.to(DEV))
    assert torch.equal(d[:, 0], d1) and torch.equal(i[:, 0], i1)
    # the same cloud twice: every point finds itself at slots 0 and 1, the lower index first
    a = P.cloud("cube", 700, 31)
    for K in (2, 5):
        d, i = ops.knn_points(a.to(DEV), torch.cat([a, a]).to(DEV), K)
        d, i = d.cpu(), i.cpu()
        assert (d[:, :2] == 0).all() and torch.equal(i[:, 0], torch.arange(700)) and torch.equal(i[:, 1], torch.arange(700) + 700)
        if K > 2:  # then its other neighbours in pairs of equal distance, the lower index first
            assert torch.equal(d[:, 2], d[:, 3]) and torch.equal(i[:, 2] + 700, i[:, 3]) and (d[:, 2] > 0).all()
    # K = 1 is reni_nearest_points
    for key in (("cube", 513, 4097, 1.0), ("spheres", 257, 1023, 1e3)):
        x, y = (t.to(DEV) for t in P.nn_clouds(key))
        d, i = ops.knn_points(x, y, 1)
        d1, i1 = ops.nearest_points(x, y)
        assert torch.equal(d[:, 0], d1) and torch.equal(i[:, 0], i1)


def test_slicing_never_changes_a_bit():
    from reni_amd import ops
    for label, (x, y), K in (("64x20000", C.knn_clouds(("cube", 64, 20000, 32, 1.0)), 32), ("lattice", C.lattice(), 8)):
        x, y = x.to(DEV), y.to(DEV)
        got = {}
        for s in (1, 3, 7, 0, 10 ** 6):
            before = ops.launch_count()
            got[s] = ops.knn_points(x, y, K, slices=s)
            launches = ops.launch_count() - before
            print(f"{label}: slices = {s}: {launches} launches")
            # (the lattice's 729 targets are less than one tile: the library's own choice is one slice)
            assert launches == (1 if s == 1 or (s == 0 and label == "lattice") else 2)
        for s in (3, 7, 0, 10 ** 6):
            assert torch.equal(got[1][0], got[s][0]) and torch.equal(got[1][1], got[s][1]), (label, s)


def test_nan_and_infinite_coordinates_are_never_listed():
    from reni_amd import ops
    x = P.cloud("cube", 70, 41).clone()
    y = P.cloud("cube", 1500, 42).clone()
    x[3, 1] = float("nan")
    y[7] = float("nan")
    y[1200, 0] = float("inf")
    keep = torch.arange(70) != 3
    ref = C.knn(x[keep], y, 8)
    for s in (1, 5):
        d, i = ops.knn_points(x.to(DEV), y.to(DEV), 8, slices=s)
        d, i = d.cpu(), i.cpu()
        print(f"slices = {s}: the NaN query's row {i[3].tolist()}")
        assert (i[3] == -1).all() and torch.isinf(d[3]).all()
        assert not (i == 7).any() and not (i == 1200).any() and torch.isfinite(d[keep]).all()
        assert torch.equal(i[keep], ref["idx"][:, :8])
    big = torch.full((5, 3), 3e38)
    for s in (1, 3):
        d, i = ops.knn_points(big.to(DEV), (-big).to(DEV), 4, slices=s)  # every d overflows to +inf
        assert (i == -1).all() and torch.isinf(d).all()


# ----------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("key", C.NORMAL_CASES, ids=C.case_id)
def test_cloud_normals_match_the_float64_reference(key):
    from reni_amd import mesh_losses, ops
    kind, n, k = key
    y = C.normal_cloud(kind, n)
    Y = y.to(DEV)
    _, idx = ops.knn_points(Y, Y, k)
    nrm, eig = ops.cloud_normals(Y, idx)
    ref = C.normals(y, idx.cpu())  # on the device's own neighbour lists
    re, ra, left_out, gap = C.normal_ratios(nrm.cpu(), eig.cpu(), ref)
    same = float((idx.cpu() == C.normal_case(key)[1]).all(1).float().mean())
    print(f"{C.case_id(key)}: eigenvalue error / (2^-23 l2) = {re:.4g} (bound {C.K_E}); angle / (2^-23 l2 / (l1 - l0)) = {ra:.4g} "
          f"(bound {C.K_N}); left out {100 * left_out:.2f} %, smallest gap ratio {gap:.4g}; {100 * same:.1f} % of the lists are "
          f"the reference's")
    assert torch.isfinite(nrm).all() and torch.isfinite(eig).all()
    assert float((nrm.double().norm(dim=1) - 1).abs().max()) <= 4 * U
    assert (eig[:, 0] >= 0).all() and (eig[:, 0] <= eig[:, 1]).all() and (eig[:, 1] <= eig[:, 2]).all()
    assert re <= C.K_E and ra <= C.K_N and left_out <= C.UNDECIDED_CAP
    # the sign rule without a viewpoint: the component of largest magnitude is positive, the lowest index on ties
    top = nrm.abs().argmax(dim=1)
    assert (nrm.gather(1, top[:, None]) > 0).all()
    n2, e2 = mesh_losses.estimate_normals(Y, k, return_eigenvalues=True)
    assert torch.equal(nrm, n2) and torch.equal(eig, e2)  # the same calls; two calls give identical bits
    assert torch.equal(mesh_losses.estimate_normals(Y, k), nrm)


def test_an_exact_plane_and_the_sign_rules():
    from reni_amd import mesh_losses, ops
    g = torch.Generator().manual_seed(7)
    y = torch.rand(1200, 3, generator=g) * 2 - 1
    y[:, 2] = 0.25
    Y = y.to(DEV)
    _, idx = ops.knn_points(Y, Y, 16)
    nrm, eig = ops.cloud_normals(Y, idx)
    ref = C.normals(y, idx.cpu())
    e = ref["eig"]
    bound = C.K_N * U * e[:, 2] / (e[:, 1] - e[:, 0])
    ang = C.angle(nrm.cpu(), torch.tensor([[0.0, 0.0, 1.0]]).expand(1200, 3))
    print(f"plane z = 0.25: worst angle to (0, 0, 1) = {float(ang.max()):.3g} (smallest bound {float(bound.min()):.3g})")
    assert (ang <= bound).all() and (nrm[:, 2] > 0).all()  # the no-viewpoint rule makes it +
    below = mesh_losses.estimate_normals(Y, 16, viewpoint=(0.0, 0.0, -3.0))
    assert (below[:, 2] < 0).all() and torch.equal(below, -nrm)
    # a sphere seen from inside: every normal points inwards; from outside and far away: the definition, point by point
    s = C.normal_cloud("sphere", 1500)
    S = s.to(DEV)
    free = mesh_losses.estimate_normals(S, 16)
    inner = mesh_losses.estimate_normals(S, 16, viewpoint=torch.zeros(3, device=DEV))
    dots = (inner * S).sum(1)
    print(f"sphere from inside: largest n . (y - viewpoint) = {float(dots.max()):.3g}")
    assert (dots <= 0).all() and float(dots.max()) < -0.5
    vp = torch.tensor([0.3, -40.0, 55.0])
    outer = mesh_losses.estimate_normals(S, 16, viewpoint=vp.to(DEV))
    side = (outer.cpu().double() * (vp.double() - s.double())).sum(1)
    assert (side >= 0).all()
    flip = (outer != free).any(1)
    assert torch.equal(outer[flip], -free[flip]) and torch.equal(outer[~flip], free[~flip])
    want = (free.cpu().double() * (vp.double() - s.double())).sum(1) < 0
    margin = (free.cpu().double() * (vp.double() - s.double())).sum(1).abs() > 1e-4  # (away from the rounding of the dot product)
    assert torch.equal(flip.cpu()[margin], want[margin])


def test_degenerate_neighbourhoods():
    from reni_amd import mesh_losses, ops
    line = torch.zeros(64, 3)
    line[:, 0] = torch.arange(64) * 0.125
    line[:, 1] = 0.5
    n, e = mesh_losses.estimate_normals(line.to(DEV), 8, return_eigenvalues=True)
    print(f"collinear: normals {n[0].tolist()} .., eigenvalues {e[0].tolist()}")
    assert torch.isfinite(n).all() and float((n.norm(dim=1) - 1).abs().max()) <= 4 * U
    assert (e[:, :2] == 0).all() and (e[:, 2] > 0).all() and (n[:, 0].abs() <= 4 * U).all()  # orthogonal to the line
    same = torch.full((50, 3), 0.25)
    n, e = mesh_losses.estimate_normals(same.to(DEV), 8, return_eigenvalues=True)
    assert (e == 0).all() and torch.equal(n.cpu(), torch.tensor([[1.0, 0.0, 0.0]]).expand(50, 3))  # what the header says
    y = C.normal_cloud("sphere", 1500).to(DEV)
    n, e = mesh_losses.estimate_normals(y, 2, return_eigenvalues=True)  # fewer than 3 neighbours: exactly 0
    assert (n == 0).all() and (e == 0).all()
    idx = torch.tensor([[0, 1, 2, -1], [0, 1, -1, -1], [5, 1500, 7, 9], [-1, -1, -1, -1]], device=DEV)
    n, e = ops.cloud_normals(y, idx)
    assert (n[1] == 0).all() and (n[3] == 0).all() and (e[1] == 0).all() and torch.isfinite(n).all()
    assert abs(float(n[0].norm()) - 1) <= 4 * U and abs(float(n[2].norm()) - 1) <= 4 * U  # a slot out of range is skipped
    ref = C.normals(y.cpu(), idx.cpu())
    assert float(C.angle(n[[0, 2]].cpu(), ref["normal"][[0, 2]]).max()) <= 1e-5  # (three points: the plane through them)
    big = torch.full((8, 3), 3e38)
    big[::2] *= -1
    n, e = ops.cloud_normals(big.to(DEV), torch.arange(8, device=DEV).repeat(8, 1))  # moments that overflow
    assert torch.isfinite(n).all() and torch.isfinite(e).all() and float((n.norm(dim=1) - 1).abs().max()) <= 4 * U


# --------------------------------------------------------------------------------------------------------- sampled normals
def _mesh_dev(key, grad=False):
    from reni_amd.mesh import Meshes
    v, f = P.sample_mesh(key)
    return Meshes(verts=[v.to(DEV).requires_grad_(grad)], faces=[f.to(DEV)])


@pytest.mark.parametrize("key", C.FN_MESHES, ids=C.case_id)
def test_sampled_normals_match_the_float64_reference(key):
    from reni_amd import mesh_losses
    from reni_amd.mesh_losses import mesh_regularizer
    v, f, u, up, s, ref = C.fn_case(key)
    mesh = _mesh_dev(key, grad=True)
    pts, nrm, face = mesh_losses.sample_points_from_meshes(mesh, u.shape[0], u=u.to(DEV), return_faces=True, return_normals=True)
    plain = mesh_losses.sample_points_from_meshes(_mesh_dev(key), u.shape[0], u=u.to(DEV))
    assert torch.equal(pts, plain)  # without return_normals the points keep their bits
    wrong = face.cpu() != s["face"]
    keep = ~wrong
    rn = M.error_ratio(nrm, ref["n"], ref["n_terms"], keep)
    on = M.over_bound(nrm, ref["n"], ref["n_terms"], C.K_FN, keep)
    (nrm * up.to(DEV)).sum().backward()
    g1 = mesh.verts_packed().grad.clone()
    rows = ~s["und_rows"] if wrong.any() else torch.ones(v.shape[0], dtype=torch.bool)
    rg = M.error_ratio(g1, ref["gv"], ref["gv_terms"], rows)
    og = M.over_bound(g1, ref["gv"], ref["gv_terms"], C.K_FNG, rows)
    print(f"{C.case_id(key)}: normals error / (2^-23 sum |terms|) = {rn:.4g}, / bound = {on:.4g}; verts.grad {rg:.4g}, / bound = "
          f"{og:.4g}; {int(wrong.sum())} faces differ, {int(s['und'].sum())} samples undecided")
    assert not (wrong & ~s["und"]).any()
    assert on <= 1.0 and og <= 1.0 and torch.isfinite(g1).all() and torch.isfinite(nrm).all()
    assert float((nrm.detach().norm(dim=1) - 1).abs().max()) <= 4 * U
    # a second backward: identical bits; and beside the regulariser's gradient in one backward
    mesh2 = _mesh_dev(key, grad=True)
    _, nrm2 = mesh_losses.sample_points_from_meshes(mesh2, u.shape[0], u=u.to(DEV), return_normals=True)
    (nrm2 * up.to(DEV)).sum().backward()
    assert torch.equal(nrm, nrm2) and torch.equal(mesh2.verts_packed().grad, g1)
    mesh3 = _mesh_dev(key, grad=True)
    _, nrm3 = mesh_losses.sample_points_from_meshes(mesh3, u.shape[0], u=u.to(DEV), return_normals=True)
    ((nrm3 * up.to(DEV)).sum() + mesh_regularizer(mesh3, edge=1.0, laplacian=0.5)).backward()
    mesh4 = _mesh_dev(key, grad=True)
    mesh_regularizer(mesh4, edge=1.0, laplacian=0.5).backward()
    both, reg = mesh3.verts_packed().grad, mesh4.verts_packed().grad
    assert torch.equal(both, g1 + reg) or torch.equal(both, reg + g1)


# ---------------------------------------------------------------------------------------------------- the chamfer normal term
G_N = 1.7  # the upstream factor of the normal term


def _normal_term_dev(name, weights, abs_cosine):
    from reni_amd import mesh_losses
    x, y = P.ch_clouds(name)
    nx, ny = C.nt_normals(name)
    X, Y, NX, NY = (t.to(DEV).requires_grad_(True) for t in (x, y, nx, ny))
    dist, term = mesh_losses.chamfer_distance(X, Y, weights, x_normals=NX, y_normals=NY, abs_cosine=abs_cosine)
    (dist * P.G_UP + term * G_N).backward()
    return dist.detach(), term.detach(), X.grad, Y.grad, NX.grad, NY.grad


@pytest.mark.parametrize("abs_cosine", (True, False), ids=("abs", "signed"))
@pytest.mark.parametrize("weights", C.NT_WEIGHTS, ids=lambda w: f"w{w[0]:g}-{w[1]:g}")
@pytest.mark.parametrize("name", C.NT_CASES)
def test_chamfer_normal_term_matches_the_float64_reference(name, weights, abs_cosine):
    from reni_amd import mesh_losses
    ref = C.nt_of(name, weights, abs_cosine)
    dist, term, gx, gy, gnx, gny = _normal_term_dev(name, weights, abs_cosine)
    rv = M.error_ratio(_one(term), _one(ref["value"]), _one(ref["value_terms"]))
    ov = M.over_bound(_one(term), _one(ref["value"]), _one(ref["value_terms"]), C.K_NT)
    rx = M.error_ratio(gnx, G_N * ref["gx"], G_N * ref["gx_terms"])
    ry = M.error_ratio(gny, G_N * ref["gy"], G_N * ref["gy_terms"])
    ox = M.over_bound(gnx, G_N * ref["gx"], G_N * ref["gx_terms"], C.K_NTG)
    oy = M.over_bound(gny, G_N * ref["gy"], G_N * ref["gy_terms"], C.K_NTG)
    print(f"{name} {weights} abs={abs_cosine}: term error / (2^-23 sum |terms|) = {rv:.4g}, / bound = {ov:.4g}; x_normals.grad "
          f"{rx:.4g}, / bound = {ox:.4g}; y_normals.grad {ry:.4g}, / bound = {oy:.4g}")
    assert term.dim() == 0 and torch.isfinite(gnx).all() and torch.isfinite(gny).all()
    assert ov <= 1.0 and ox <= 1.0 and oy <= 1.0
    # the distance and the position gradients are the bits of the call without normals
    x, y = P.ch_clouds(name)
    X, Y = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    L = mesh_losses.chamfer_distance(X, Y, weights)
    (L * P.G_UP).backward()
    assert torch.equal(L.detach(), dist) and torch.equal(X.grad, gx) and torch.equal(Y.grad, gy)
    again = _normal_term_dev(name, weights, abs_cosine)
    assert all(torch.equal(a, b) for a, b in zip(again, (dist, term, gx, gy, gnx, gny)))  # two calls give identical bits


def test_a_zero_normal_gives_a_finite_term_and_gradient():
    from reni_amd import mesh_losses
    x, y = P.ch_clouds("cube")
    nx, ny = (t.clone() for t in C.nt_normals("cube"))
    nx[0] = 0.0
    ny[5] = 0.0
    NX, NY = nx.to(DEV).requires_grad_(True), ny.to(DEV).requires_grad_(True)
    X = x.to(DEV).requires_grad_(True)
    dist, term = mesh_losses.chamfer_distance(X, y.to(DEV), x_normals=NX, y_normals=NY)
    term.backward()
    ch = P.chamfer_of("cube", (1.0, 1.0))
    ref = C.normal_term(nx, ny, ch["matches"][0]["idx"], ch["matches"][1]["idx"])
    print(f"zero normals: term {float(term):.6g} (reference {float(ref['value']):.6g})")
    assert torch.isfinite(term) and torch.isfinite(NX.grad).all() and torch.isfinite(NY.grad).all()
    assert M.over_bound(_one(term), _one(ref["value"]), _one(ref["value_terms"]), C.K_NT) <= 1.0
    assert X.grad is None or (X.grad == 0).all()  # the positions get no gradient from the normal term


# ------------------------------------------------------------------------------------------------------------------ scores
def test_normal_consistency_scores():
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    n = 2000
    unit = ico_sphere(3, DEV)
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(2))
    floor = C.max_dihedral_cos(unit.verts_packed().cpu(), unit.faces_packed().cpu())
    s = mesh_losses.geometry_scores(unit, unit, n=n, u=u.to(DEV), surface=True, normals=True)
    print({k: float(v) for k, v in s.items()}, f"cos of the largest dihedral angle {floor:.6f}")
    for k in ("normal_consistency_pred", "normal_consistency_true", "normal_consistency"):
        assert floor <= float(s[k]) <= 1.0 + 4 * U
    assert float(s["chamfer"]) <= 1e-10
    # against the cube, sample to sample: the reference on the same samples, within the summed bounds
    # and surface to surface: the face normal of the nearest triangle by the float64 pair function
    vu, fu = unit.verts_packed().cpu(), unit.faces_packed().cpu()
    mean = 4 * U  # (the mean of n float32 values near 1)
    for h in (0.6, 1.2):  # the cube cuts the unit sphere (many samples nearest to an edge: ties), and encloses it
        vc, fc = C.cube_mesh(h)
        cube = Meshes(verts=[vc.to(DEV)], faces=[fc.to(DEV)])
        for surface in (False, True):
            if surface:
                (rp, bp, tp), (rt, bt, tt) = C.consistency_surface(vu, fu, vc, fc, u)
            else:
                ((rp, bp), (rt, bt)), tp, tt = C.consistency(vu, fu, vc, fc, u), 0.0, 0.0
            s = mesh_losses.geometry_scores(unit, cube, n=n, u=u.to(DEV), surface=surface, normals=True)
            old = mesh_losses.geometry_scores(unit, cube, n=n, u=u.to(DEV), surface=surface)
            print(f"cube {h} surface={surface}:", {k: float(v) for k, v in s.items() if k.startswith("normal")},
                  f"reference {rp:.6f} +- {bp:.3g}, {rt:.6f} +- {bt:.3g}; tied rows {100 * tp:.1f} %, {100 * tt:.1f} %")
            assert set(s) == set(old) | {"normal_consistency_pred", "normal_consistency_true", "normal_consistency"}
            assert all(torch.equal(s[k], old[k]) for k in old)  # the old keys keep their bits
            assert abs(float(s["normal_consistency"]) - 0.5 * (float(s["normal_consistency_pred"]) + float(s["normal_consistency_true"]))) <= 2 * U
            assert not any(v.requires_grad for v in s.values())
            assert abs(float(s["normal_consistency_pred"]) - rp) <= bp + mean
            assert abs(float(s["normal_consistency_true"]) - rt) <= bt + mean


# ------------------------------------------------------------------------------------------------------------------- a fit
def test_a_sphere_is_pulled_towards_a_scan_with_estimated_normals():
    """the README's loop in small: scan -> estimate_normals -> chamfer + 0.1 normal term -> normal consistency"""
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes, ico_sphere
    target = ico_sphere(3, DEV)
    ellipsoid = Meshes(verts=[target.verts_packed() * torch.tensor([1.5, 1.0, 0.7], device=DEV)], faces=[target.faces_packed()])
    scan = mesh_losses.sample_points_from_meshes(ellipsoid, 3000, generator=torch.Generator(device=DEV).manual_seed(0))
    scan_normals = mesh_losses.estimate_normals(scan, 16)
    start = ico_sphere(2, DEV)
    verts = (start.verts_packed() * 0.5).clone().requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[start.faces_packed()])
    verts = mesh.verts_packed()
    u = torch.rand(2000, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    before = mesh_losses.geometry_scores(mesh, ellipsoid, n=2000, u=u, surface=True, normals=True)
    opt = torch.optim.Adam([verts], lr=0.02)
    gen = torch.Generator(device=DEV).manual_seed(1)
    first = None
    for step in range(60):
        pts, nrm = mesh_losses.sample_points_from_meshes(mesh, 2000, generator=gen, return_normals=True)
        chamfer, normal = mesh_losses.chamfer_distance(pts, scan, x_normals=nrm, y_normals=scan_normals)
        first = (float(chamfer), float(normal)) if first is None else first
        opt.zero_grad()
        (chamfer + 0.1 * normal).backward()
        opt.step()
    after = mesh_losses.geometry_scores(mesh, ellipsoid, n=2000, u=u, surface=True, normals=True)
    print(f"fit: chamfer {first[0]:.5f} -> {float(chamfer):.5f}, normal term {first[1]:.5f} -> {float(normal):.5f}, "
          f"normal consistency {float(before['normal_consistency']):.5f} -> {float(after['normal_consistency']):.5f}, "
          f"chamfer to the surface {float(before['chamfer']):.5f} -> {float(after['chamfer']):.5f}")
    assert torch.isfinite(verts).all()
    assert float(chamfer) < first[0] and float(normal) < first[1]
    assert float(after["normal_consistency"]) > float(before["normal_consistency"])


# ------------------------------------------------------------------------------------------------------------ launch counts
def test_launch_counts_are_the_header_s():
    from reni_amd import ops
    x, y = (t.to(DEV) for t in P.ch_clouds("cube"))
    rose = {}

    def call(name, fn, *args, **kw):
        before = ops.launch_count()
        out = fn(*args, **kw)
        rose[name] = ops.launch_count() - before
        return out

    call("knn_points_one_slice", ops.knn_points, x, y, 8, slices=1)
    _, idx = call("knn_points_sliced", ops.knn_points, y, y, 8, slices=4)
    call("cloud_normals", ops.cloud_normals, y, idx)
    call("cloud_normals_viewpoint", ops.cloud_normals, y, idx, (0.0, 0.0, 5.0))
    print(rose)
    assert rose == {"knn_points_one_slice": 1, "knn_points_sliced": 2, "cloud_normals": 1, "cloud_normals_viewpoint": 1}
    assert math.isfinite(float(idx.sum()))
