"""GPU tests of the SG, SH and diffuse kernels (reni_tu_baselines.hip, reni_tu_diffuse.hip) at the shapes where their
guards, tails and dispatch thresholds act: the cases of tests/baseline_edge_cases.py against the float64 restatements of
tests/test_baselines_cpu.py, batch independence, guard bands around every output, and poisoned workspaces.
tests/test_baseline_edges_cpu.py shows that plain fp32 arithmetic reaches a quarter of each bound at every case.

Each parity test prints its worst figure before it asserts (pytest -s or -rA shows them)."""
import numpy as np
import pytest
import torch

from tests import baseline_edge_cases as E
from tests.test_baselines_cpu import rel, rel_l2

pytestmark = pytest.mark.gpu

# the bounds of the project's existing tests of the same quantities (tests/test_gpu_baselines.py, tests/test_gpu_diffuse.py)
SH_PROJECT_TOL = 1e-5      # max |c - ref| / ||ref|| per map
SH_RECONSTRUCT_TOL = 1e-5  # rel per map
SG_LOSS_TOL = 1e-5         # relative, total and per map
SG_GRAD_TOL = 1e-5         # rel_l2, overall and per map
SG_RENDER_TOL = 2e-6       # rel
DIFFUSE_TOL = 1e-5         # rel per map

SENTINEL = 0x5A17C0DE  # a finite float32 (1.07e16) no kernel here produces
GUARD = 4096           # sentinel words on either side of a carved output
SG_IDS = ["x".join(str(v) for v in c) for c in E.SG_CASES]


def _dev():
    return torch.device("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from reni_amd import _lib
    return _lib.load()


class Carved:
    """n float32 words in the middle of one allocation filled with SENTINEL, the output included: a stray store on either
    side lands in the same allocation (it faults nothing) and shows; a word the kernel leaves unwritten shows as well."""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((2 * GUARD + self.n,), SENTINEL, dtype=torch.int32, device=_dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def values(self):
        return self.buf[GUARD:GUARD + self.n].view(torch.float32).view(self.shape)

    def check(self, expected, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENTINEL).all()), f"{what}: a store below the output"
        assert bool((self.buf[GUARD + self.n:] == SENTINEL).all()), f"{what}: a store above the output"
        assert not bool((self.buf[GUARD:GUARD + self.n] == SENTINEL).any()), f"{what}: a word of the output was never written"
        assert torch.equal(self.values().view(torch.int32), expected.contiguous().view(torch.int32)), f"{what}: values"


def _workspace(nbytes, fill):
    """(keep-alive tensor, 256-byte aligned pointer, bytes) with every byte set to `fill`"""
    ws = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device=_dev())
    p = (ws.data_ptr() + 255) & ~255
    return ws, p, ws.numel() - (p - ws.data_ptr())


def _sh_tables(W, lmax, solid_angle):
    from reni_amd import baselines
    row, col = baselines.sh_tables(W, lmax, solid_angle)
    return (torch.from_numpy(row.astype(np.float32)).to(_dev()), torch.from_numpy(col.astype(np.float32)).to(_dev()))


def c_sh(project, src, W, lmax, out_ptr):
    """reni_sh_project / reni_sh_reconstruct through the C entry point, the output wherever out_ptr says"""
    row, col = _sh_tables(W, lmax, project)
    lib = _lib()
    fn = lib.reni_sh_project if project else lib.reni_sh_reconstruct
    assert src.is_contiguous() and src.dtype == torch.float32
    rc = fn(src.shape[0], W // 2, W, lmax, src.data_ptr(), row.data_ptr(), col.data_ptr(), out_ptr, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()


def _sg_operands(case):
    from reni_amd import baselines
    N, H, W, R, C = case
    raw, env = (t.to(_dev()) for t in E.sg_inputs(case))
    tc, pc, tr, pr = baselines.sg_lobe_centres(R, C, _dev())
    return raw, torch.log(env + 1), tc, pc, tr, pr


def c_sg_loss_grad(case, raw, lt, tc, pc, tr, pr, weight, per_ptr, total_ptr, grad_ptr, ws_fill=0):
    N, H, W, R, C = case
    lib = _lib()
    ws, wp, wn = _workspace(int(lib.reni_sg_workspace_bytes(N, R * C, H, W)), ws_fill)
    assert raw.is_contiguous() and lt.is_contiguous() and tuple(weight.shape) == (N, 3, H, W)
    rc = lib.reni_sg_loss_grad(N, R * C, H, W, raw.data_ptr(), tc.data_ptr(), pc.data_ptr(), float(tr), float(pr), lt.data_ptr(),
                               weight.data_ptr(), *[int(s) for s in weight.stride()], per_ptr, total_ptr, grad_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()
    return int(lib.reni_sg_workspace_bytes(N, R * C, H, W))


def c_diffuse(src, in_dirs, w, out_dirs, out_ptr, ws_fill=0, planar=False):
    """reni_diffuse_convolve through the C entry point: src [N, Q, 3], or [N, 3, Q] when planar"""
    N, Q, P = src.shape[0], in_dirs.shape[0], out_dirs.shape[0]
    lib = _lib()
    ws, wp, wn = _workspace(int(lib.reni_diffuse_workspace_bytes(N, P, Q)), ws_fill)
    assert tuple(src.shape) == ((N, 3, Q) if planar else (N, Q, 3))
    sn, si, sc = (int(s) for s in src.stride())
    if planar:
        si, sc = sc, si
    rc = lib.reni_diffuse_convolve(N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), w.data_ptr(), src.data_ptr(), sn, si, sc,
                                   float(1 / np.pi), out_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()
    return int(lib.reni_diffuse_workspace_bytes(N, P, Q))


def _df_operands(P, Q):
    src, in_dirs, w, out_dirs, ref = E.df_inputs(P, Q)
    return src.to(_dev()), in_dirs.to(_dev()), w.to(_dev()), out_dirs.to(_dev()), ref


# ---------------------------------------------------------------------------------------------- parity with float64
@pytest.mark.parametrize("W", E.SH_WIDTHS)
def test_sh_edge_shapes_match_float64(W):
    """Q = W^2 / 2 never a multiple of 128 (qok, the q < Q store guard), every tile count with its first and fullest T
    (t < T in operand and store), 3 N = 3 .. 66 (cok with 1, 2, 30, 31 live columns in a block)."""
    from reni_amd import baselines
    imgs = E.sh_images(W).to(_dev())
    worst_c = worst_r = 0.0
    for lmax in E.SH_LMAX:
        ref_c, ref_r = E.sh_reference(W, lmax)
        cs = E.sh_coeffs(lmax).to(_dev())
        for N in E.SH_N:
            assert (W, lmax, N) in E.SH_CASES
            c = baselines.sh_project(imgs[:N], lmax)
            r = baselines.sh_reconstruct(cs[:N], W)
            assert c.shape == (N, (lmax + 1) ** 2, 3) and r.shape == (N, W // 2, W, 3)
            err_c = E.per_map_max_over_norm(c.cpu().numpy(), ref_c[:N]).max()
            err_r = E.per_map_rel(r.cpu().numpy(), ref_r[:N]).max()
            worst_c, worst_r = max(worst_c, err_c), max(worst_r, err_r)
            assert err_c <= SH_PROJECT_TOL, (W, lmax, N, err_c)
            assert err_r <= SH_RECONSTRUCT_TOL, (W, lmax, N, err_r)
    print(f"sh W={W}: projection max|c - ref| / ||ref|| {worst_c:.3e}  reconstruction rel {worst_r:.3e}")


@pytest.mark.parametrize("case", E.SG_CASES, ids=SG_IDS)
def test_sg_edge_shapes_match_float64(case):
    """k_sg_loss_grad on both sides of SG_LDS_MAX_PIX (767, 768 | 769, 775 pixels), with a second map group per workgroup
    (2049 maps), the weight read through a broadcast's, a contiguous tensor's and a sliced view's strides."""
    from reni_amd import ops
    N, H, W, R, C = case
    raw, lt, tc, pc, tr, pr = _sg_operands(case)
    assert (int(_lib().reni_sg_workspace_bytes(N, R * C, H, W)) > 0) == (H * W > 768)
    for kind in E.SG_WEIGHT_KINDS:
        weight = E.sg_weight(case, kind, _dev())
        assert weight.stride() == E.sg_weight(case, kind).stride()
        total, per, grad = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, weight)
        ref_total, ref_per, ref_grad = E.sg_reference(case, kind)
        e_total = abs(total.item() - ref_total) / abs(ref_total)
        e_per = (np.abs(per.cpu().numpy() - ref_per) / np.abs(ref_per)).max()
        e_grad = rel_l2(grad.cpu().numpy(), ref_grad)
        e_grad_map = E.per_map_rel_l2(grad.cpu().numpy(), ref_grad).max()
        print(f"sg {case} {kind}: loss {e_total:.3e}  per-map loss {e_per:.3e}  grad rel_l2 {e_grad:.3e}  per-map {e_grad_map:.3e}")
        assert e_total <= SG_LOSS_TOL and e_per <= SG_LOSS_TOL, (case, kind, e_total, e_per)
        assert e_grad <= SG_GRAD_TOL and e_grad_map <= SG_GRAD_TOL, (case, kind, e_grad, e_grad_map)


@pytest.mark.parametrize("case", E.SG_CASES, ids=SG_IDS)
def test_sg_render_edge_shapes_match_float64(case):
    """k_sg_render against float64 beyond the two golden shapes, at the golden test's 2e-6 (measured on an MI355X: 4.6e-7
    at worst, the 2049-map case; torch float32 on the host gives 4.3e-7 there)."""
    from reni_amd import ops
    N, H, W, R, C = case
    raw, _, tc, pc, tr, pr = _sg_operands(case)
    rec = ops.sg_render(raw, tc, pc, tr, pr, H, W)
    assert rec.shape == (N, 3, H, W)
    err = rel(rec.cpu().numpy(), E.sg_render_reference(case))
    print(f"sg render {case}: rel {err:.3e}")
    assert err <= SG_RENDER_TOL, (case, err)


@pytest.mark.parametrize("P,Q", E.DF_SHAPES)
def test_diffuse_edge_shapes_match_float64(P, Q):
    """Q = 1, 2, 3 (the odd tail with and without a main loop), P < 32 and P = 33, 257 (idle waves, masked rows), 3 N = 33
    and 66 (a column pair whose second tile holds one or two live columns), and the split boundary 4095 | 4096 | 4097; the
    interleaved [N, Q, 3] and planar [N, 3, Q] layouts give the same bits."""
    from reni_amd import baselines
    src, in_dirs, w, out_dirs, ref = _df_operands(P, Q)
    assert (int(_lib().reni_diffuse_workspace_bytes(1, P, Q)) > 0) == (Q >= 4096)
    worst = 0.0
    for N in E.DF_N:
        assert (P, Q, N) in E.DF_CASES
        out = baselines.diffuse_convolve(src[:N], in_dirs, w, out_dirs)
        assert out.shape == (N, P, 3)
        o = out.cpu().numpy()
        # every map has something lit: a comparison of zeros with zeros would pass whatever the kernel did
        assert ref[:N].reshape(N, -1).max(axis=1).min() > 0 and o.reshape(N, -1).max(axis=1).min() > 0
        err = E.per_map_rel(o, ref[:N]).max()
        worst = max(worst, err)
        assert err <= DIFFUSE_TOL, (P, Q, N, err)
        planar = src[:N].permute(0, 2, 1).contiguous()  # [N, 3, Q]
        got = Carved(N, P, 3)
        c_diffuse(planar, in_dirs, w, out_dirs, got.ptr, planar=True)
        got.check(out, f"planar {(P, Q, N)}")
        if Q != 3:  # the wrapper tells the layouts apart by shape: it reads [N, 3, 3] as [N, Q, 3]
            assert torch.equal(baselines.diffuse_convolve(planar, in_dirs, w, out_dirs), out), (P, Q, N)
    print(f"diffuse P={P} Q={Q}: rel {worst:.3e}")


# ---------------------------------------------------------------------------------------------- batch independence
def test_sg_maps_of_the_second_group_are_batch_independent():
    """2049 maps of 775 pixels: map 2047 (the last wave of workgroup 511's only group), map 2048 (the one live wave of
    workgroup 0's second group) and map 0 give, run alone, the bits they have in the batch."""
    from reni_amd import ops
    case = E.SG_CASES[-1]
    N, H, W, R, C = case
    assert N == 2049 and H * W == 775
    raw, lt, tc, pc, tr, pr = _sg_operands(case)
    rec = ops.sg_render(raw, tc, pc, tr, pr, H, W)
    for kind in E.SG_WEIGHT_KINDS:
        weight = E.sg_weight(case, kind, _dev())
        total, per, grad = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, weight)
        again = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, weight)
        assert torch.equal(again[0], total) and torch.equal(again[1], per) and torch.equal(again[2], grad)
        for n in (0, 2047, 2048):
            t1, p1, g1 = ops.sg_loss_grad(raw[n:n + 1], tc, pc, tr, pr, lt[n:n + 1], weight[n:n + 1])
            assert torch.equal(p1[0], per[n]) and torch.equal(t1, per[n]), (kind, n)
            assert torch.equal(g1[0], grad[n]), (kind, n)
    for n in (0, 2047, 2048):
        assert torch.equal(ops.sg_render(raw[n:n + 1], tc, pc, tr, pr, H, W)[0], rec[n]), n


@pytest.mark.parametrize("W", [6, 66])
def test_sh_maps_are_batch_independent_at_ragged_column_blocks(W):
    """N = 11 and 22: the second column block holds one and two live columns, and a map straddles the two blocks."""
    from reni_amd import baselines
    imgs = E.sh_images(W).to(_dev())
    for lmax in E.SH_LMAX:
        cs = E.sh_coeffs(lmax).to(_dev())
        for N in (11, 22):
            c = baselines.sh_project(imgs[:N], lmax)
            r = baselines.sh_reconstruct(cs[:N], W)
            for n in (0, 10, N - 1):
                assert torch.equal(baselines.sh_project(imgs[n:n + 1], lmax)[0], c[n]), (W, lmax, N, n)
                assert torch.equal(baselines.sh_reconstruct(cs[n:n + 1], W)[0], r[n]), (W, lmax, N, n)


def test_diffuse_maps_are_batch_independent_across_the_split():
    from reni_amd import baselines
    P, Q = 33, 4097
    src, in_dirs, w, out_dirs, _ = _df_operands(P, Q)
    for N in (11, 22):
        out = baselines.diffuse_convolve(src[:N], in_dirs, w, out_dirs)
        assert torch.equal(baselines.diffuse_convolve(src[:N], in_dirs, w, out_dirs), out)
        for n in (0, 10, N - 1):
            assert torch.equal(baselines.diffuse_convolve(src[n:n + 1], in_dirs, w, out_dirs)[0], out[n]), (N, n)


# ---------------------------------------------------------------------------------------------- guard bands
def test_sh_outputs_stay_inside_their_buffers():
    """W = 6 (18 pixels of a 128-pixel wave), lmax 11 (T = 144: three of eight tiles wholly masked), N = 11 (one live
    column in the second block)."""
    from reni_amd import baselines
    W, lmax, N = 6, 11, 11
    imgs, cs = E.sh_images(W)[:N].to(_dev()), E.sh_coeffs(lmax)[:N].to(_dev())
    coeffs = Carved(N, (lmax + 1) ** 2, 3)
    c_sh(True, imgs, W, lmax, coeffs.ptr)
    coeffs.check(baselines.sh_project(imgs, lmax), "sh_project")
    maps = Carved(N, W // 2, W, 3)
    c_sh(False, cs, W, lmax, maps.ptr)
    maps.check(baselines.sh_reconstruct(cs, W), "sh_reconstruct")


@pytest.mark.parametrize("case", [(3, 1, 769, 1, 1), (5, 3, 5, 8, 8)], ids=["3x1x769x1x1", "5x3x5x8x8"])
def test_sg_outputs_stay_inside_their_buffers(case):
    from reni_amd import ops
    assert case in E.SG_CASES
    N, H, W, R, C = case
    raw, lt, tc, pc, tr, pr = _sg_operands(case)
    for kind in E.SG_WEIGHT_KINDS:
        weight = E.sg_weight(case, kind, _dev())
        per, total, grad = Carved(N), Carved(1), Carved(N, R * C, 6)
        c_sg_loss_grad(case, raw, lt, tc, pc, tr, pr, weight, per.ptr, total.ptr, grad.ptr)
        want = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, weight)
        total.check(want[0].view(1), f"sg total {kind}")
        per.check(want[1], f"sg loss_per_map {kind}")
        grad.check(want[2], f"sg dparams {kind}")
    rec = Carved(N, 3, H, W)
    lib = _lib()
    rc = lib.reni_sg_render(N, R * C, H, W, raw.data_ptr(), tc.data_ptr(), pc.data_ptr(), float(tr), float(pr), rec.ptr, _stream())
    assert rc == 0, lib.reni_last_error()
    rec.check(ops.sg_render(raw, tc, pc, tr, pr, H, W), "sg rec")


def test_diffuse_output_stays_inside_its_buffer():
    """P = 33 (the second output tile holds one live row), Q = 3 (odd tail), N = 11 (one live column in the second tile)"""
    from reni_amd import baselines
    P, Q, N = 33, 3, 11
    src, in_dirs, w, out_dirs, _ = _df_operands(P, Q)
    out = Carved(N, P, 3)
    c_diffuse(src[:N], in_dirs, w, out_dirs, out.ptr)
    out.check(baselines.diffuse_convolve(src[:N], in_dirs, w, out_dirs), "diffuse out")


# ---------------------------------------------------------------------------------------------- poisoned workspace
@pytest.mark.parametrize("case", [(3, 1, 769, 1, 1), (2049, 25, 31, 1, 2)], ids=["3x1x769x1x1", "2049x25x31x1x2"])
def test_sg_workspace_path_with_a_poisoned_workspace(case):
    """Every byte of the workspace 0xFF (NaN floats) before the call: the directions and g that k_sg_loss_grad<false>
    keeps there must all be written before they are read, in the second map group as in the first."""
    assert case in E.SG_CASES
    N, H, W, R, C = case
    raw, lt, tc, pc, tr, pr = _sg_operands(case)
    weight = E.sg_weight(case, "contiguous", _dev())
    runs = []
    for fill in (0x00, 0xFF):
        per, total, grad = Carved(N), Carved(1), Carved(N, R * C, 6)
        assert c_sg_loss_grad(case, raw, lt, tc, pc, tr, pr, weight, per.ptr, total.ptr, grad.ptr, ws_fill=fill) > 0
        runs.append((per, total, grad))
    for clean, dirty, what in zip(runs[0], runs[1], ("loss_per_map", "loss_total", "dparams")):
        assert bool(torch.isfinite(dirty.values()).all()), what
        dirty.check(clean.values(), what)


def test_diffuse_split_with_a_poisoned_workspace():
    """(33, 4097): two chunks (2050 + 2047) whose partial sums go through the workspace; k_diffuse_reduce must read only
    what k_diffuse_convolve wrote."""
    P, Q = 33, 4097
    src, in_dirs, w, out_dirs, _ = _df_operands(P, Q)
    for N in E.DF_N:
        runs = []
        for fill in (0x00, 0xFF):
            out = Carved(N, P, 3)
            assert c_diffuse(src[:N], in_dirs, w, out_dirs, out.ptr, ws_fill=fill) > 0
            runs.append(out)
        assert bool(torch.isfinite(runs[1].values()).all()), N
        runs[1].check(runs[0].values(), f"diffuse N={N}")


# ---------------------------------------------------------------------------------------------- wrapper inputs
def test_sh_project_takes_a_channel_planar_view():
    """A [N, H, W, 3] view of a [N, 3, H, W] tensor projects to the bits of its contiguous copy."""
    from reni_amd import baselines
    for W, lmax, N in ((6, 11, 11), (34, 8, 22)):
        imgs = E.sh_images(W)[:N].to(_dev())
        view = imgs.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
        assert not view.is_contiguous() and torch.equal(view, imgs)
        assert torch.equal(baselines.sh_project(view, lmax), baselines.sh_project(imgs, lmax)), (W, lmax, N)
