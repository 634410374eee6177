"""GPU tests of the mesh regularisers (reni_tu_meshreg.hip, ops.mesh_regularizers, reni_amd/mesh_losses.py) against the float64
reference of tests/mesh_reg_ref.py.

Bounds: max(K 2^-23 sum |terms|, 2e-5 max |ref|) per element, sum |terms| accumulated by the reference's closed form, K = 4 x
the worst ratio of its float32 CPU evaluation over the same cases (M.K; DESIGN 4.4t has the measured figures, the device's
among them).  Undecided elements (M.closed_form's und_rows / und_value) are left out of the bound and checked for finiteness
and equal bits only; no parity case has any but the cot ones, and "bad_faces" under cot, whose collinear face reaches more than
the cap, is bounded on "bad_faces_cot".  Every test prints its figure before it asserts."""
import pytest
import torch

from tests import mesh_reg_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMBOS = tuple((key, loss) for loss in M.LOSSES for key in M.parity_cases(loss))
WEIGHTS = {"edge": (1.0, 0.0, 0.0), "uniform": (0.0, 1.0, 0.0), "cot": (0.0, 1.0, 0.0), "normal": (0.0, 0.0, 1.0)}
INDEX = {"edge": 1, "uniform": 2, "cot": 2, "normal": 3}


def _combo_id(c):
    return M.case_id(c[0]) + "-" + c[1]


def _dev(key):
    v, f = M.mesh(key)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)


def _method(loss):
    return "cot" if loss == "cot" else "uniform"


def _run(key, loss, **kw):
    from reni_amd import ops
    v, f = _dev(key)
    return ops.mesh_regularizers(v, f, *WEIGHTS[loss], target_length=M.target_of(loss), method=_method(loss), **kw)


def _one(t):
    return torch.as_tensor(t).reshape(1)


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_value_and_gradient_match_the_float64_reference(combo):
    from reni_amd import ops
    key, loss = combo
    ref = M.scales(key, loss)
    values, g = _run(key, loss)
    kv, kg = M.K[loss]
    keep = ~ref["und_rows"]
    val = values[INDEX[loss]]
    rv = M.error_ratio(_one(val), _one(ref["value"]), _one(ref["value_terms"]))
    ov = M.over_bound(_one(val), _one(ref["value"]), _one(ref["value_terms"]), kv)
    rg = M.error_ratio(g, ref["g"], ref["g_terms"], keep)
    og = M.over_bound(g, ref["g"], ref["g_terms"], kg, keep)
    print(f"{_combo_id(combo)}: value error / (2^-23 sum |terms|) = {rv:.4g}, / bound = {ov:.4g}; grad_verts {rg:.4g}, / bound = {og:.4g}; "
          f"undecided rows {int((~keep).sum())}")
    assert g.shape == ref["g"].shape and torch.isfinite(g).all() and torch.isfinite(values).all()
    if not ref["und_value"]:
        assert ov <= 1.0
    assert og <= 1.0
    # the weighted total of a single loss of weight 1 is the loss; the other two are skipped: exactly 0
    assert float(values[0]) == float(val)
    for other in (1, 2, 3):
        if other != INDEX[loss]:
            assert float(values[other]) == 0.0
    # equal bits: a second call, caller-kept lists, and the values alone (grad_verts = NULL)
    values2, g2 = _run(key, loss)
    assert torch.equal(values, values2) and torch.equal(g, g2)
    v, f = _dev(key)
    values3, g3 = _run(key, loss, lists=ops.mesh_edge_lists(f, v.shape[0]))
    assert torch.equal(values, values3) and torch.equal(g, g3)
    values4, g4 = _run(key, loss, need_grad=False)
    assert g4 is None and torch.equal(values, values4)


@pytest.mark.parametrize("combo", tuple((key, m) for m in ("uniform", "cot") for key in M.parity_cases(m)), ids=_combo_id)
def test_fused_call_matches_the_reference_and_the_separate_calls(combo):
    from reni_amd import ops
    key, method = combo
    lap = method
    v, f = _dev(key)
    we, wl, wn = M.FUSED
    values, g = ops.mesh_regularizers(v, f, we, wl, wn, target_length=M.target_of("edge"), method=method)
    parts = {loss: M.scales(key, loss) for loss in ("edge", lap, "normal")}
    w = {"edge": we, lap: wl, "normal": wn}
    # the bound of the weighted sum: max(2^-23 sum_k w_k K_k sum |terms_k|, 2e-5 max |ref|), each loss under its own K
    ref_g = sum(w[k] * parts[k]["g"] for k in parts)
    kterms_g = sum(w[k] * M.K[k][1] * parts[k]["g_terms"] for k in parts)
    ref_v = sum(w[k] * parts[k]["value"] for k in parts)
    kterms_v = sum(w[k] * M.K[k][0] * parts[k]["value_terms"] for k in parts)
    keep = ~(parts["edge"]["und_rows"] | parts[lap]["und_rows"] | parts["normal"]["und_rows"])
    und_value = any(parts[k]["und_value"] for k in parts)
    ov = M.over_bound(_one(values[0]), _one(ref_v), _one(kterms_v), 1.0)
    og = M.over_bound(g, ref_g, kterms_g, 1.0, keep)
    # the separate calls, on the device
    sep_g, sep_v = torch.zeros_like(g).double(), 0.0
    for loss in parts:
        vals, gs = _run(key, loss)
        sep_g += w[loss] * gs.double()
        sep_v += w[loss] * float(vals[INDEX[loss]])
        # each value of the fused call within its own bound
        o = M.over_bound(_one(values[INDEX[loss]]), _one(parts[loss]["value"]), _one(parts[loss]["value_terms"]), M.K[loss][0])
        assert parts[loss]["und_value"] or o <= 1.0, (loss, o)
    os_ = M.over_bound(g, sep_g.cpu(), kterms_g, 1.0, keep)  # the same bound, about the separate calls' weighted sum
    osv = M.over_bound(_one(values[0]), _one(torch.tensor(sep_v, dtype=torch.float64)), _one(kterms_v), 1.0)
    print(f"fused {M.case_id(key)}-{method}: total error / bound = {ov:.4g}, grad_verts {og:.4g}, against the separate calls {os_:.4g} (total {osv:.4g})")
    assert torch.isfinite(g).all() and torch.isfinite(values).all()
    assert und_value or ov <= 1.0
    assert og <= 1.0 and os_ <= 1.0
    assert osv <= 1.0
    values2, g2 = ops.mesh_regularizers(v, f, we, wl, wn, target_length=M.target_of("edge"), method=method)
    assert torch.equal(values, values2) and torch.equal(g, g2)


def test_exact_zeros():
    from reni_amd import ops
    for loss in M.LOSSES:  # an isolated vertex: r = 0, gradient 0 exactly
        values, g = _run(("unreferenced", 16), loss)
        assert (g[M.G.UNREFERENCED] == 0).all() and (g != 0).any(), loss
    values, g = _run(("cover", 33), "normal")  # one face: no pair
    assert float(values[3]) == 0.0 and float(values[0]) == 0.0 and (g == 0).all()
    values, g = _run(("soup", 17), "normal")
    assert float(values[3]) == 0.0 and (g == 0).all()
    values, g = _run(("hinge", 0), "normal")  # a flat pair
    assert float(values[3]) == 0.0
    values, _ = _run(("double", 0), "normal")  # a repeated face
    assert abs(float(values[3]) - 2.0) <= 4 * M.U
    # vertex 43 of "bad_faces" is the exact midpoint of its two neighbours: r_43 = 0 and its own share -u_43 of the Laplacian
    # gradient is exactly 0.  The reference's terms of row 43 then hold the neighbours' share alone, so a share that is not 0
    # (a unit vector over V) would leave the bound by orders of magnitude
    key = ("bad_faces", 16)
    v, f = _dev(key)
    values, g = _run(key, "uniform")
    ref = M.scales(key, "uniform")
    row = torch.zeros(v.shape[0], dtype=torch.bool)
    row[43] = True
    o43 = M.over_bound(g, ref["g"], ref["g_terms"], M.K["uniform"][1], row)
    print(f"bad_faces row 43: error / bound = {o43:.4g}, |g_43| = {float(g[43].norm()):.4g}, 1 / V = {1 / v.shape[0]:.4g}")
    assert o43 <= 1.0
    # a weight of 0: that loss's value is exactly 0 and it adds exactly 0 to the gradient -- the single-loss call's gradient
    # is not moved by what the skipped losses would have added: the isolated vertex and, for the normal loss on a mesh
    # without a pair, every row stay exactly 0 (above); here the value
    a = ops.mesh_regularizers(v, f, 0.7, 1.3, 0.0, target_length=0.05)
    assert float(a[0][3]) == 0.0 and float(a[0][1]) != 0.0 and float(a[0][2]) != 0.0
    b = ops.mesh_regularizers(v, f, 0.0, 0.0, 0.0)
    assert (b[0] == 0).all() and (b[1] == 0).all()


def test_bad_faces_under_cot_is_finite_and_reproducible():
    """its collinear face sits at the area floor (undecided by construction): finite, equal bits, and the rows it does not reach
    within the bound"""
    key = ("bad_faces", 16)
    ref = M.scales(key, "cot")
    values, g = _run(key, "cot")
    values2, g2 = _run(key, "cot")
    keep = ~ref["und_rows"]
    og = M.over_bound(g, ref["g"], ref["g_terms"], M.K["cot"][1], keep)
    print(f"bad_faces-16-cot: grad_verts of the decided rows, error / bound = {og:.4g}; value {float(values[2]):.6g}")
    assert torch.isfinite(values).all() and torch.isfinite(g).all()
    assert torch.equal(values, values2) and torch.equal(g, g2)
    assert og <= 1.0


def _lists(key):
    from reni_amd import ops
    v, f = _dev(key)
    return v, f, ops.mesh_edge_lists(f, v.shape[0])


def test_malformed_lists_add_nothing_and_nothing_faults():
    from reni_amd import ops
    key = ("ico", 16)
    v, f, L = _lists(key)
    good = ops.mesh_regularizers(v, f, *M.FUSED, lists=L)

    def run(**changed):
        bad = dict(L)
        bad.update(changed)
        values, g = ops.mesh_regularizers(v, f, *M.FUSED, method="cot", lists=bad)
        torch.cuda.synchronize()
        assert torch.isfinite(values).all() and torch.isfinite(g).all(), tuple(changed)
        return values, g

    # every edge turned round (a > b): no edge is valid, nothing is added anywhere
    values, g = run(edges=L["edges"].flip(1).contiguous())
    assert (values == 0).all() and (g == 0).all()
    # edges out of range
    values, g = run(edges=L["edges"] + v.shape[0])
    assert (values == 0).all() and (g == 0).all()
    # offsets far outside their lists, negative, decreasing: clamped
    big = torch.iinfo(torch.int64).max
    for name in ("ef_offsets", "ve_offsets", "vf_offsets"):
        n = L[name].numel()
        run(**{name: torch.full((n,), big, dtype=torch.int64, device=DEV)})
        run(**{name: torch.full((n,), -big, dtype=torch.int64, device=DEV)})
        run(**{name: L[name].flip(0).contiguous()})
    whole = torch.zeros_like(L["ef_offsets"])
    whole[1::2] = L["H"]  # every other edge is handed the whole list
    run(ef_offsets=whole)
    values, g = run(ve_offsets=torch.zeros_like(L["ve_offsets"]))  # no vertex has an edge: no Laplacian, no end-point gradient
    assert float(values[2]) == 0.0
    # entries outside their ranges, and entries that name the wrong face / edge / vertex
    gen = torch.Generator().manual_seed(5)
    for name in ("ef_corners", "ve_edges", "vf_corners", "corner_edges"):
        x = L[name]
        run(**{name: torch.randint(-2 ** 62, 2 ** 62, x.shape, generator=gen).to(DEV)})
        run(**{name: x.roll(1).contiguous()})
        run(**{name: torch.full_like(x, -1)})
    values, g = run(ef_corners=torch.full_like(L["ef_corners"], -1))  # no edge has a face: no pair, no cot weight
    assert float(values[3]) == 0.0
    # shapes, dtypes and devices are checked on the host
    for bad in (dict(edges=L["edges"][:-1]), dict(ef_offsets=L["ef_offsets"].int()), dict(ve_edges=L["ve_edges"].cpu()),
                dict(E=L["E"] + 1), dict(corner_edges=L["corner_edges"][:-1])):
        changed = dict(L)
        changed.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_regularizers(v, f, *M.FUSED, lists=changed)
    # a face tensor with bad and repeated indices needs no help from the lists
    values, g = _run(("bad_faces", 16), "normal")
    assert torch.isfinite(g).all()
    again = ops.mesh_regularizers(v, f, *M.FUSED, lists=L)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])


def test_autograd_functions():
    import math
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings
    from tests import raster_edge_cases as E
    key = ("ico", 16)
    v0, f = _dev(key)
    v = v0.clone().requires_grad_(True)
    mesh = Meshes(verts=[v], faces=[f])
    target = 0.05
    # the four functions are the op's values, 0-d, and their backward its gradient
    fns = {"edge": lambda: mesh_losses.mesh_edge_loss(mesh, target), "uniform": lambda: mesh_losses.mesh_laplacian_smoothing(mesh),
           "cot": lambda: mesh_losses.mesh_laplacian_smoothing(mesh, method="cot"), "normal": lambda: mesh_losses.mesh_normal_consistency(mesh)}
    for loss, fn in fns.items():
        values, g = ops.mesh_regularizers(v.detach(), f, *WEIGHTS[loss], target_length=target, method=_method(loss))
        out = fn()
        assert out.dim() == 0 and out.requires_grad and float(out.detach()) == float(values[INDEX[loss]])
        (got,) = torch.autograd.grad(out, v)
        assert torch.equal(got, g), loss
    # upstream scalar != 1
    values, g = ops.mesh_regularizers(v.detach(), f, *M.FUSED, target_length=target)
    out = mesh_losses.mesh_regularizer(mesh, *M.FUSED, target_length=target)
    assert float(out.detach()) == float(values[0])
    (got,) = torch.autograd.grad(out * 2.5, v)
    assert torch.equal(got, g * 2.5)
    # accumulation beside a silhouette loss on the same vertices
    Rm, T = E.camera()
    Rm, T = Rm.to(DEV), T.to(DEV)
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=16))
    w = torch.randn(16, 16, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    (gs,) = torch.autograd.grad((rast.silhouette(mesh, Rm, T, sigma=1e-3) * w).sum(), v)
    v.grad = None
    ((rast.silhouette(mesh, Rm, T, sigma=1e-3) * w).sum() + mesh_losses.mesh_regularizer(mesh, *M.FUSED, target_length=target)).backward()
    assert (gs != 0).any() and torch.equal(v.grad, gs + g)
    # an in-place step: the topology lists are kept, the value is renewed
    lists = mesh._edge_lists()
    with torch.no_grad():
        v.mul_(0.9)
    moved = mesh_losses.mesh_regularizer(mesh, *M.FUSED, target_length=target)
    assert mesh._edge_lists() is lists
    want = ops.mesh_regularizers(v.detach(), f, *M.FUSED, target_length=target)[0][0]
    assert float(moved.detach()) == float(want) and float(moved.detach()) != float(out.detach())
    assert torch.equal(mesh.edges_packed().cpu(), M.topology(key).edges)
    # nothing requires grad: a plain value, no node
    plain = mesh_losses.mesh_regularizer(Meshes(verts=[v0], faces=[f]), *M.FUSED, target_length=target)
    assert not plain.requires_grad and plain.dim() == 0
    with torch.no_grad():
        assert not mesh_losses.mesh_edge_loss(mesh).requires_grad
    assert math.isfinite(float(plain))


def test_regulariser_only_fit_reaches_half_the_reference_gain():
    from reni_amd import mesh_losses
    from reni_amd.mesh import Meshes
    _, start, f, target = M.fit_mesh()
    v = torch.from_numpy(start).to(DEV).requires_grad_(True)
    mesh = Meshes(verts=[v], faces=[torch.from_numpy(f).to(DEV)])
    opt = torch.optim.Adam([v], lr=M.FIT_LR)
    losses = []
    for step in range(M.FIT_STEPS + 1):
        loss = mesh_losses.mesh_regularizer(mesh, target_length=target, **M.FIT_WEIGHTS)
        losses.append(float(loss.detach()))
        if step == M.FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    gain, ref_gain = losses[0] - losses[-1], M.FIT_START - M.FIT_END
    print(f"fit: device loss {losses[0]:.6f} -> {losses[-1]:.6f} (gain {gain:.6f}); float64 reference {M.FIT_START:.6f} -> "
          f"{M.FIT_END:.6f} (gain {ref_gain:.6f})")
    assert abs(losses[0] - M.FIT_START) <= 1e-5 * M.FIT_START
    assert gain >= 0.5 * ref_gain
