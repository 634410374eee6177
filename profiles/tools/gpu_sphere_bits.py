"""Diagnostic: the raw bits of every output of the sphere family's entry points (ops.diffuse_convolve, lobe_convolve,
lobe_denominators, lobe_convolve_backward, envmap_lookup, envmap_lookup_table, envmap_lookup_backward, envmap_lookup_dquery,
rotate_envmap), for comparing two builds of the library.

  RENI_HIP_LIB=<library A> python profiles/tools/gpu_sphere_bits.py run a.npz    (one process per library)
  RENI_HIP_LIB=<library B> python profiles/tools/gpu_sphere_bits.py run b.npz
  python profiles/tools/gpu_sphere_bits.py compare a.npz b.npz                   (no GPU: numpy.array_equal on the raw words)

Inputs: the tests' own catalogues -- baseline_edge_cases.DF_CASES; glossy_edge_cases.fwd_case / bwd_case over FWD_SHAPES /
BWD_SHAPES x LOBE_SETS x LB_N, normalised and not (the 16-lobe sets on the operands of the shape's nine-lobe case, with an
upstream of their own, and on the tests' own SIXTEEN cases); LOOKUP_CASES with shared and per-map directions and levels, a level
array or a constant (0, a knot, a fraction, out of range) and one strided source; map_edge_cases' rotations, channel counts,
non-finite matrices and carved input, each with index= as well -- and one shape of the timing tools per entry point, where more
than one workgroup column and more than one split run."""
import math
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np


def run(path):
    import torch
    from reni_amd import ops
    from tests import baseline_edge_cases as B
    from tests import glossy_edge_cases as G
    from tests import map_edge_cases as M
    dev = torch.device("cuda:0")
    out = {}

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            if t is None:
                continue
            a = t.detach().cpu().contiguous().numpy()
            out[f"{key}/{i}"] = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])

    def kp(lobes):
        return [l.kind for l in lobes], [l.param for l in lobes]

    # ---- diffuse convolve
    for P, Q, N in B.DF_CASES:
        src, in_dirs, w, out_dirs, _ = (x.to(dev) if isinstance(x, torch.Tensor) else x for x in B.df_inputs(P, Q))
        put(f"diffuse/{P}x{Q}/{N}", ops.diffuse_convolve(src[:N], in_dirs, w, out_dirs, 1.0 / math.pi))

    # ---- lobe convolve, denominators, backward
    def lobe_forward(key, c, lobes):
        src, in_dirs, w, out_dirs = (x.to(dev) for x in (c.src, c.in_dirs, c.w, c.out_dirs))
        k, p = kp(lobes)
        put(f"{key}/den", ops.lobe_denominators(in_dirs, w, out_dirs, k, p))
        for N in G.LB_N:
            put(f"{key}/{N}", ops.lobe_convolve(src[:N], in_dirs, w, out_dirs, k, p, True),
                ops.lobe_convolve(src[:N], in_dirs, w, out_dirs, k, p, False, G.SCALE))

    def lobe_backward(key, c, lobes, g):
        g, in_dirs, w, out_dirs = (x.to(dev) for x in (g, c.in_dirs, c.w, c.out_dirs))
        k, p = kp(lobes)
        den = ops.lobe_denominators(in_dirs, w, out_dirs, k, p)
        for N in G.LB_N:
            gN = g[:N].contiguous()
            put(f"{key}/{N}", ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, k, p, True, den=den),
                ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, k, p, False, G.SCALE),
                ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, k, p, True, den=den, planar=True))

    for name, lobes in G.LOBE_SETS.items():
        for P, Q in G.FWD_SHAPES:
            lobe_forward(f"lobe/{name}/{P}x{Q}", G.fwd_case(P, Q), lobes)
        for P, Q in G.BWD_SHAPES:
            c = G.bwd_case(P, Q)
            g = c.g if name == "nine" else torch.randn(G.NMAX, len(lobes), P, 3, generator=torch.Generator().manual_seed(P + Q))
            lobe_backward(f"lobe_bwd/{name}/{P}x{Q}", c, lobes, g)
        if name != "nine":
            lobe_forward(f"lobe/{name}/sixteen", G.fwd_case(*G.SIXTEEN_FWD, name), lobes)
            c = G.bwd_case(*G.SIXTEEN_BWD, name)
            lobe_backward(f"lobe_bwd/{name}/sixteen", c, lobes, c.g)

    # ---- lookup, its table, its backward and its query derivative
    for case in G.LOOKUP_CASES:
        H, W, Lv, P = case
        c = G.lookup_case(*case)
        key = "lookup/" + "x".join(str(v) for v in case)
        chain = torch.from_numpy(c.chain).to(dev)
        wide = torch.zeros(G.LOOKUP_MAPS, Lv + 1, H + 2, 2 * W, 4, device=dev)
        strided = wide[:, 1:, 1:H + 1, ::2, :3]  # every stride its own
        strided.copy_(chain)
        dirs, per = torch.from_numpy(c.dirs).to(dev), torch.from_numpy(c.per_map).to(dev)
        level, level_np = torch.from_numpy(c.level).to(dev), torch.from_numpy(c.level_np).to(dev)
        up = torch.randn(G.LOOKUP_MAPS, P, 3, generator=torch.Generator().manual_seed(P)).to(dev)
        consts = (None, 0.0, float(Lv - 1), 0.5 * (Lv - 1) + 0.25, -3.0, Lv + 2.0)
        for dname, d in (("shared", dirs), ("per_map", per)):
            for lname, lv in [("array", level), ("array_per_map", level_np)] + [(f"const{v}", v) for v in consts]:
                k = f"{key}/{dname}/{lname}"
                put(f"{k}/lookup", ops.envmap_lookup(chain, d, lv))
                put(f"{k}/table", *ops.envmap_lookup_table(G.LOOKUP_MAPS, Lv, H, W, d, lv))
                put(f"{k}/backward", ops.envmap_lookup_backward(up, Lv, H, W, d, lv))
                if isinstance(lv, torch.Tensor):
                    for nd, nl in ((True, True), (True, False), (False, True)):
                        put(f"{k}/dquery{int(nd)}{int(nl)}", *ops.envmap_lookup_dquery(chain, d, lv, up, nd, nl))
                else:
                    put(f"{k}/dquery10", *ops.envmap_lookup_dquery(chain, d, lv, up, True, False))
            put(f"{key}/{dname}/strided", ops.envmap_lookup(strided, d, level),
                *ops.envmap_lookup_dquery(strided, d, level, up, True, True))

    # ---- rotate
    def rot(R):
        return torch.from_numpy(np.ascontiguousarray(R, np.float32)).to(dev)

    def rotate(key, x, R, mode):
        B_ = x.shape[0]
        idx = torch.tensor(M.INDEX_B7, device=dev)
        put(key, ops.rotate_envmap(x, R, mode), ops.rotate_envmap(x, R if R.dim() == 2 else R[idx], mode, index=idx))
        assert B_ == 2

    for H, W in M.ROTATE_SHAPES:
        x = torch.tensor(M.rotate_input(H, W)).to(dev)
        for name, R32, _ in M.bilinear_rotations(H, W):
            rotate(f"rotate/{H}x{W}/bilinear/{name}", x, rot(R32), "bilinear")
        for name, R in M.nearest_rotations():
            rotate(f"rotate/{H}x{W}/nearest/{name}", x, rot(R), "nearest")
        for name, R, _ in M.nearest_exact_cases(M.rotate_input(H, W)):
            rotate(f"rotate/{H}x{W}/nearest_exact/{name}", x, rot(R), "nearest")
    for H, W in M.NONFINITE_SHAPES:
        x = torch.tensor(M.rotate_input(H, W)).to(dev)
        for mode in ("bilinear", "nearest"):
            for name, R in M.NONFINITE:
                rotate(f"rotate/{H}x{W}/{mode}/nonfinite {name}", x, rot(R), mode)
    H, W = M.ROTATE_CHANNEL_SHAPE
    for C in (1, 5):
        x = torch.tensor(M.rotate_input(H, W, C)).to(dev)
        for mode in ("bilinear", "nearest"):
            for name, R32, _ in M.bilinear_rotations(H, W):
                rotate(f"rotate/{H}x{W}/C{C}/{mode}/{name}", x, rot(R32), mode)
    H, W = M.ROTATE_CARVED_SHAPE
    x = torch.tensor(M.rotate_input(H, W)).to(dev)
    wide = torch.zeros(2, 4, H + 3, 2 * W, device=dev)
    carved = wide[:, :3, 2:H + 2, 1::2]
    carved.copy_(x)
    from tests.test_rotate_cpu import rotation_list
    Rs = torch.stack([rot(R) for _, R in rotation_list()[:7]])
    for mode in ("bilinear", "nearest"):
        rotate(f"rotate/{H}x{W}/{mode}/carved", carved, Rs[:2], mode)
        rotate(f"rotate/{H}x{W}/{mode}/hwc", x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), Rs[:2], mode)
        put(f"rotate/{H}x{W}/{mode}/index7", ops.rotate_envmap(x, Rs, mode, index=torch.tensor(M.INDEX_B7, device=dev)))

    # ---- one shape of the timing tools per entry point
    from reni_amd import glossy
    from reni_amd.baselines import reni_grid_weights
    from reni_amd.rotation import random_rotations
    from reni_amd.utils import get_directions
    g = torch.Generator().manual_seed(0)
    envs = (torch.rand(64, 64 * 128, 3, generator=g) * 2).to(dev)
    d128 = get_directions(128)[0].to(dev)
    w128 = torch.as_tensor(reni_grid_weights(128), dtype=torch.float32).to(dev)
    put("timing/diffuse 64 x 64x128", ops.diffuse_convolve(envs, d128, w128, d128, 1.0 / math.pi))
    mixed = [glossy.phong(64), glossy.blinn(20), glossy.ggx(0.6), glossy.phong(8)]
    k, p = kp(mixed)
    den = ops.lobe_denominators(d128, w128, d128, k, p)
    up = torch.randn(64, len(mixed), d128.shape[0], 3, generator=g).to(dev)
    put("timing/lobes 64 x 64x128", den, ops.lobe_convolve(envs, d128, w128, d128, k, p, True),
        ops.lobe_convolve_backward(up, d128, w128, d128, k, p, True, den=den))
    del envs, up
    chain = torch.rand(64, 5, 64, 128, 3, generator=g).to(dev)
    dirs = torch.randn(64, 16384, 3, generator=g).to(dev)
    level = (torch.rand(64, 16384, generator=g) * 4).to(dev)
    up = torch.randn(64, 16384, 3, generator=g).to(dev)
    for name, d, lv in (("shared", dirs[0], level[0].contiguous()), ("per_map", dirs, level)):
        put(f"timing/lookup 64 x 16384 {name}", ops.envmap_lookup(chain, d, lv), *ops.envmap_lookup_dquery(chain, d, lv, up, True, True))
    # (table and gather at split_sum_time.py's query shape: at 64 x 16384 the table alone is 120 MB)
    put("timing/lookup table 1 x 16384", *ops.envmap_lookup_table(1, 5, 64, 128, dirs[0], level[0].contiguous()),
        ops.envmap_lookup_backward(up[:1], 5, 64, 128, dirs[0], level[0].contiguous()))
    del chain, dirs, level, up
    gd = torch.Generator(device=dev).manual_seed(0)
    maps = torch.rand(200, 3, 64, 128, device=dev, generator=gd)
    idx = torch.randperm(200, device=dev, generator=gd)[:100]
    R = random_rotations(100, "SO3", gd)
    for mode in ("bilinear", "nearest"):
        put(f"timing/rotate 100 x 3 x 64x128 {mode}", ops.rotate_envmap(maps, R, mode, "chw", index=idx))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
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
