"""GPU side of the ray caster's edge cases (tests/visibility_edge_cases.py; reni_tu_visibility.hip: k_vis_prepare,
k_mesh_visibility) against the float64 restatement of tests/visibility_ref.py: direction counts beyond one 256-direction
block, per-image lists with a padded row stride, the axis-aligned room (zero, NaN and inf direction components, flat
clusters), origins exactly on the planes of the inflated boxes, t_min = 0, records with holes behind guard bands, and the
Python layer at J = 512.

The rule is tests/test_gpu_visibility.py's: the device agrees with float64 on EVERY decided ray, and at most
VR.UNDECIDED_MAX of a case's rays are undecided (a condition on the scenes, re-asserted on the CPU by
tests/test_visibility_edges_cpu.py).  Every case also asserts that two calls are bit-equal and that RENI_VIS_NO_CULL gives
the same bits on all rays, decided or not."""
import numpy as np
import pytest
import torch

from tests import visibility_edge_cases as EC
from tests import visibility_ref as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 4096                    # bytes of guard band on each side of a carved buffer
VIS_SENTINEL = 0x5A5A5A5A       # in the bands round the mask; the mask itself is prefilled with 0xFFFFFFFF
ACCEL_SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------------------ helpers
def _t(x):
    return torch.from_numpy(np.array(x)).to(DEV)  # (a copy: the shared scenes are read-only)


def _prepare(sc, order="morton"):
    """the record of the scene's mesh: the package's Morton order, or order = arange ("given"), or an int64 array"""
    from reni_amd import ops
    v, f = _t(sc["verts"]), _t(sc["faces"])
    if isinstance(order, str) and order == "morton":
        return ops.mesh_visibility_prepare(v, f)
    o = torch.arange(f.shape[0], device=DEV) if isinstance(order, str) else _t(order)
    return ops.mesh_visibility_prepare(v, f, order=o)


def _cast(sc, accel, no_cull=False, dirs=None, own=None):
    from reni_amd import ops
    vis = ops.mesh_visibility(_t(sc["origins"]), _t(sc["own"] if own is None else own), _t(sc["dirs"] if dirs is None else dirs),
                              accel, sc["t_min"], no_cull=no_cull)
    return vis.cpu()


def _cast_three_ways(sc, accel, **kw):
    """the mask, after asserting that a second call and the brute-force path give the same bits on all rays"""
    a = _cast(sc, accel, **kw)
    assert torch.equal(a, _cast(sc, accel, **kw)), "two calls differ"
    assert torch.equal(a, _cast(sc, accel, no_cull=True, **kw)), "RENI_VIS_NO_CULL moves a bit"
    return a


def _agree(name, words, own, J, occ, dec):
    """words: one image's mask [NP, JW] (int32 tensor on the host) against the reference (occluded, decided) [NP, J]"""
    from reni_amd.mesh import unpack_visibility
    NP = len(own)
    assert words.dtype == torch.int32 and tuple(words.shape) == (NP, (J + 31) // 32) and occ.shape == (NP, J)
    visible = unpack_visibility(words[None], J)[0].numpy()
    differ = visible != ~occ
    bad = differ & dec
    share = 1.0 - dec.mean()
    print(f"{name}: rays {NP * J}, undecided {int((~dec).sum())} ({100 * share:.3f} %), GPU vs float64: "
          f"{int(bad.sum())} decided and {int((differ & ~dec).sum())} undecided rays differ")
    assert share <= VR.UNDECIDED_MAX
    assert not bad.any(), f"{int(bad.sum())} decided rays differ, first (pixel, direction) {np.argwhere(bad)[:4].tolist()}"
    w = words.numpy().view(np.uint32)
    if J % 32:
        assert not (w[:, -1] >> np.uint32(J % 32)).any(), "padding bits at j >= J must be 0"
    assert not w[np.asarray(own) < 0].any(), "background rows must be 0"


class _Carved:
    """``count`` elements of ``dtype`` in the middle of a larger buffer whose two guard bands hold ``sentinel``"""

    def __init__(self, count, dtype, sentinel, fill):
        self.g = GUARD // torch.empty(0, dtype=dtype).element_size()
        self.count, self.sentinel = count, sentinel
        self.big = torch.full((2 * self.g + count,), sentinel, dtype=dtype, device=DEV)
        self.view = self.big[self.g:self.g + count]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.big[:self.g] == self.sentinel).all()) and bool((self.big[self.g + self.count:] == self.sentinel).all())


# ----------------------------------------------------------------------------------------------------------- A. wide J
@pytest.mark.parametrize("F,NP,J", EC.WIDE_CASES)
def test_every_block_of_directions_matches_float64(F, NP, J):
    sc, occ, dec = EC.wide_case(F, NP, J)
    vis = _cast_three_ways(sc, _prepare(sc))
    assert tuple(vis.shape) == (1, NP, (J + 31) // 32)
    _agree(f"wide {F, NP, J}", vis[0], sc["own"], J, occ, dec)


# --------------------------------------------------------------------------------------------------- B. per-image lists
def test_per_image_lists_with_a_padded_row_stride():
    from reni_amd import _lib, ops
    lib = _lib.load()
    sc, dirs, refs = EC.per_image_case()
    B, J, NP = EC.PER_IMAGE_B, EC.PER_IMAGE_J, len(sc["own"])
    JW = (J + 31) // 32
    buf, stride = EC.padded_rows(dirs)
    accel = _prepare(sc)
    pos, p2f, dbuf = _t(sc["origins"]), _t(sc["own"]), _t(buf)
    stream = torch.cuda.current_stream().cuda_stream
    raw = []
    for flags in (0, 0, _lib.VIS_NO_CULL):
        out = _Carved(B * NP * JW, torch.int32, VIS_SENTINEL, -1)
        rc = lib.reni_mesh_visibility(B, NP, J, pos.data_ptr(), p2f.data_ptr(), dbuf.data_ptr(), stride, accel.data_ptr(),
                                      sc["t_min"], flags, out.view.data_ptr(), stream)
        assert rc == 0 and out.intact()
        raw.append(out.view.reshape(B, NP, JW).cpu())
    assert torch.equal(raw[0], raw[1]) and torch.equal(raw[0], raw[2])
    # the same lists, packed (row stride 3 J), through the Python entry
    packed = _cast_three_ways(sc, accel, dirs=dirs)
    assert tuple(packed.shape) == (B, NP, JW) and torch.equal(packed, raw[0])
    for b in range(B):
        one = _cast(sc, accel, dirs=dirs[b])
        assert tuple(one.shape) == (1, NP, JW) and torch.equal(raw[0][b], one[0]), f"image {b} is not the shared call on its row"
        _agree(f"per-image list {b}, row stride 3 J + {EC.PER_IMAGE_GAP}", raw[0][b], sc["own"], J, *refs[b])
    assert not torch.equal(raw[0][0], raw[0][1]) and not torch.equal(raw[0][1], raw[0][2])


# -------------------------------------------------------------------------------------------------------------- C. room
@pytest.mark.parametrize("offset", EC.ROOM_OFFSETS)
def test_axis_aligned_room_and_pinned_directions(offset):
    sc, occ, dec = EC.room_case(offset)
    J = len(sc["dirs"])
    given = _cast_three_ways(sc, _prepare(sc, "given"))
    _agree(f"room at {offset}, given order", given[0], sc["own"], J, occ, dec)
    # (0,0,0), (NaN,0,1), (0,inf,0): visible from every pixel (each is decided, so the line above has held them already)
    from reni_amd.mesh import unpack_visibility
    assert bool(unpack_visibility(given, J)[0, :, 122:125].all())
    morton = _cast_three_ways(sc, _prepare(sc, "morton"))
    assert torch.equal(given, morton), "the order of the faces inside the record moves a bit"


# ----------------------------------------------------------------------------------------------- D. box-plane probes
@pytest.mark.parametrize("offset", EC.ROOM_OFFSETS)
def test_origins_on_the_planes_of_the_inflated_boxes(offset):
    """For every cluster, axis and side one origin whose coordinate is the float32 plane of the box the record holds (the
    restatement EC.cluster_boxes, checked against the definition on the CPU): the slab test of a ray parallel to that plane
    forms 0 * inf = NaN.  fminf / fmaxf return the other operand, +-inf, so such a ray SKIPS the cluster (tn = +inf on a lo
    plane, tf = -inf on a hi plane), which is right because every face lies strictly inside the inflated box; culled and
    brute force must agree on all rays."""
    sc, occ, dec = EC.probe_case(offset)
    vis = _cast_three_ways(sc, _prepare(sc, "given"))
    _agree(f"box-plane probes at {offset}", vis[0], sc["own"], len(sc["dirs"]), occ, dec)


# --------------------------------------------------------------------------------------------------------- E. t_min = 0
def test_t_min_zero_leaves_the_own_face_to_the_id_comparison():
    sc, occ, dec = EC.tmin0_case()
    vis = _cast_three_ways(sc, _prepare(sc))
    _agree("t_min = 0", vis[0], sc["own"], len(sc["dirs"]), occ, dec)


# ------------------------------------------------------------------------------------------------ F. records with holes
@pytest.mark.parametrize("kind", EC.HOLES_KINDS)
def test_records_with_holes_behind_guard_bands(kind):
    """Raw library calls: the record and the mask are carved out of larger buffers with 4096-byte guard bands that must be
    intact after every call, and the mask is prefilled with 0xFFFFFFFF, so a word the kernel does not write shows as set
    padding bits, a set background row or a visible ray that float64 says is occluded."""
    from reni_amd import _lib
    lib = _lib.load()
    sc, occ, dec = EC.holes_case(kind)
    V, F, NP, J = len(sc["verts"]), len(sc["faces"]), len(sc["own"]), len(sc["dirs"])
    JW = (J + 31) // 32
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = int(lib.reni_mesh_visibility_accel_bytes(F))
    accel = _Carved(nbytes, torch.uint8, ACCEL_SENTINEL, 0)
    verts, faces, pos, p2f, dirs = (_t(sc[k]) for k in ("verts", "faces", "origins", "own", "dirs"))
    order = None if sc["order"] is None else _t(sc["order"])
    if sc["prepare"]:
        rc = lib.reni_mesh_visibility_prepare(V, F, verts.data_ptr(), faces.data_ptr(), None if order is None else order.data_ptr(),
                                              accel.view.data_ptr(), nbytes, stream)
        assert rc == 0 and accel.intact()
    got = []
    for flags in (0, 0, _lib.VIS_NO_CULL):
        out = _Carved(NP * JW, torch.int32, VIS_SENTINEL, -1)
        rc = lib.reni_mesh_visibility(1, NP, J, pos.data_ptr(), p2f.data_ptr(), dirs.data_ptr(), 0, accel.view.data_ptr(),
                                      sc["t_min"], flags, out.view.data_ptr(), stream)
        assert rc == 0 and out.intact() and accel.intact()
        got.append(out.view.reshape(NP, JW).cpu())
    assert torch.equal(got[0], got[1]), "two calls differ"
    assert torch.equal(got[0], got[2]), "RENI_VIS_NO_CULL moves a bit"
    _agree(f"holes, {kind}", got[0], sc["own"], J, occ, dec)
    words = got[0].numpy().view(np.uint32)
    fg = sc["own"] >= 0
    if kind in ("one_bad_face", "never_prepared"):   # nothing to hit: every foreground bit below J is 1
        full = VR.pack_bits(np.ones((1, J), bool)).view(np.uint32)[0]
        assert fg.any() and (~fg).any() and (words[fg] == full[None]).all()
    if kind == "all_background":
        assert not words.any()
    if kind == "bad_order":  # a face named twice changes nothing: the same record with the duplicate's slot left empty
        twice = sc["order"].copy()
        twice[10] = -1
        accel2 = _Carved(nbytes, torch.uint8, ACCEL_SENTINEL, 0)
        o2 = _t(twice)
        assert lib.reni_mesh_visibility_prepare(V, F, verts.data_ptr(), faces.data_ptr(), o2.data_ptr(), accel2.view.data_ptr(),
                                                nbytes, stream) == 0 and accel2.intact()
        out = _Carved(NP * JW, torch.int32, VIS_SENTINEL, -1)
        assert lib.reni_mesh_visibility(1, NP, J, pos.data_ptr(), p2f.data_ptr(), dirs.data_ptr(), 0, accel2.view.data_ptr(),
                                        sc["t_min"], 0, out.view.data_ptr(), stream) == 0 and out.intact()
        assert torch.equal(out.view.reshape(NP, JW).cpu(), got[0])


# ------------------------------------------------------------------------------------------------------ G. Python layer
def _sphere_view():
    from reni_amd.mesh import FoVPerspectiveCameras, Meshes, MeshRasterizer, RasterizationSettings, look_at_view_transform
    from tests.util import uv_sphere
    v, f, _, _ = uv_sphere()
    mesh = Meshes(verts=[v.to(DEV)], faces=[f.to(DEV)])
    R, T = look_at_view_transform(*EC.SPHERE_VIEW, device=DEV)
    ras = MeshRasterizer(cameras=FoVPerspectiveCameras(device=DEV), raster_settings=RasterizationSettings(image_size=EC.SPHERE_S))
    return mesh, R, T, ras, v.numpy(), f.numpy()


def _device_gbuffer_ref(ras, mesh, R, T, verts, faces, dirs):
    """float64 on the device's own G-buffer (its origins and pix_to_face), as the teapot test's restatement does on the CPU's"""
    frag, _, pos = ras.gbuffer(mesh, R, T)
    own = frag.pix_to_face.reshape(-1).cpu().numpy()
    occ, dec = VR.visibility_ref(pos.cpu().numpy(), own, dirs, verts, faces, 1e-4 * VR.bbox_diag(verts))
    return own, occ, dec


def test_rasterizer_visibility_at_512_directions():
    from reni_amd.utils import get_directions
    mesh, R, T, ras, verts, faces = _sphere_view()
    D = get_directions(EC.SPHERE_W)[0].to(DEV)
    J = D.shape[0]
    assert J == 512
    vis = ras.visibility(mesh, R, T, D)
    assert ras.visibility(mesh, R, T, D) is vis, "the second call must return the cached mask"
    assert tuple(vis.shape) == (1, EC.SPHERE_S ** 2, 16) and vis.dtype == torch.int32
    own, occ, dec = _device_gbuffer_ref(ras, mesh, R, T, verts, faces, D.cpu().numpy())
    fg = own >= 0
    assert 40 < fg.sum() < 256 and 0.35 < occ[fg].mean() < 0.65  # about half the directions lie below a pixel's horizon
    _agree("uv sphere 16 x 16 under the 16 x 32 grid", vis[0].cpu(), own, J, occ, dec)
    assert torch.equal(vis, ras.visibility(mesh, R, T, D, no_cull=True))


def test_light_visibility_with_lists_of_257():
    from reni_amd import lighting
    mesh, R, T, ras, verts, faces = _sphere_view()
    B, S = 2, 257
    rng = np.random.default_rng(257)
    dirs = _t(np.stack([VR.unit_dirs(rng, S) for _ in range(B)]))
    colors = torch.ones(B, S, 3, device=DEV)
    samples = lighting.LightSamples(index=torch.zeros(B, S, dtype=torch.int32, device=DEV), dirs=dirs,
                                    pdf=torch.ones(B, S, device=DEV), radiance=colors, colors=colors)
    vis = lighting.light_visibility(ras, mesh, R, T, samples)
    assert tuple(vis.shape) == (B, EC.SPHERE_S ** 2, 9) and vis.dtype == torch.int32
    for b in range(B):
        row = dirs[b].contiguous()
        assert torch.equal(vis[b], ras.visibility(mesh, R, T, row)[0]), f"list {b} is not the shared call on its row"
        own, occ, dec = _device_gbuffer_ref(ras, mesh, R, T, verts, faces, row.cpu().numpy())
        _agree(f"light list {b} of {S}", vis[b].cpu(), own, S, occ, dec)
    assert not torch.equal(vis[0], vis[1])
