"""Diagnostic: the raw bits of every output of the env-map shader's entry points, for comparing two builds of the library.

  RENI_HIP_LIB=<library A> python profiles/tools/gpu_shade_bits.py run a.npz      (one process per library)
  RENI_HIP_LIB=<library B> python profiles/tools/gpu_shade_bits.py run b.npz
  python profiles/tools/gpu_shade_bits.py compare a.npz b.npz                     (no GPU: numpy.array_equal on uint32 views)

Shapes: tests/test_gpu_shade_materials.py::SHAPES; every entry point through reni_amd.ops, without a mask and with a random
one, with a per-pixel and with a single shininess / alpha; fixed seeds."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np

SHAPES = [(1, 300, 200, False), (3, 1000, 515, False), (5, 257, 1030, False), (9, 64, 129, False), (2, 130, 512, False),
          (2, 500, 300, True), (3, 1, 1, False)]


def run(path):
    import torch
    from reni_amd import ops
    dev = torch.device("cuda:0")
    out = {}

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{key}/{i}"] = t.detach().cpu().contiguous().numpy().view(np.uint32)

    for si, (B, NP, J, per_image) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(1000 + si)
        nrm = torch.randn(NP, 3, generator=g) * 0.7
        pos = torch.randn(NP, 3, generator=g) * 0.4
        bg = torch.rand(NP, generator=g) < 0.2
        nrm[bg] = 0.0
        pos[bg] = 0.0
        cam = torch.tensor([0.0, 0.0, 2.0])
        L = torch.nn.functional.normalize(torch.randn((B, J, 3) if per_image else (J, 3), generator=g), dim=-1)
        C = torch.exp(torch.randn(B, J, 3, generator=g)) * torch.rand(1, J, 1, generator=g)
        G = [torch.randn(B, NP, 3, generator=g) for _ in range(3)]
        shin = torch.rand(NP, generator=g) * 200.0 + 1.0
        alpha = torch.rand(NP, generator=g) * 0.9 + 0.05
        JW = (J + 31) // 32
        mask = torch.randint(-2 ** 31, 2 ** 31, (B if per_image else 1, NP, JW), generator=g, dtype=torch.int64).to(torch.int32)
        nrm, pos, L, C, shin, alpha, mask = (t.to(dev) for t in (nrm, pos, L, C, shin, alpha, mask))
        G = [t.to(dev) for t in G]
        for vname, vis in (("plain", None), ("masked", mask)):
            k = f"s{si}/{vname}"
            put(f"{k}/shade", ops.envmap_shade(nrm, pos, cam, L, C, 500.0, 0.5, 0.5, vis))
            put(f"{k}/shade_bwd", ops.envmap_shade_backward(nrm, pos, cam, L, G[0], 20.0, 0.3, 0.7, vis))
            for mname, s, a in (("pp", shin, alpha), ("one", 20.0, 0.3)):
                put(f"{k}/{mname}/terms", *ops.envmap_shade_terms(nrm, pos, cam, L, C, s, vis))
                put(f"{k}/{mname}/terms_ds", *ops.envmap_shade_terms(nrm, pos, cam, L, C, s, vis, need_ds=True))
                put(f"{k}/{mname}/terms_bwd", ops.envmap_shade_terms_backward(nrm, pos, cam, L, G[0], G[1], s, vis))
                put(f"{k}/{mname}/terms_dn", ops.envmap_shade_terms_dnormals(nrm, pos, cam, L, C, G[0], G[1], s, vis))
                put(f"{k}/{mname}/ggx", *ops.envmap_shade_ggx(nrm, pos, cam, L, C, a, vis))
                put(f"{k}/{mname}/ggx_bwd", ops.envmap_shade_ggx_backward(nrm, pos, cam, L, G[0], G[1], G[2], a, vis))
                put(f"{k}/{mname}/ggx_da", *ops.envmap_shade_ggx_dpixel(nrm, pos, cam, L, C, G[0], G[1], G[2], a, vis))
                put(f"{k}/{mname}/ggx_da_dn", *ops.envmap_shade_ggx_dpixel(nrm, pos, cam, L, C, G[0], G[1], G[2], a, vis, need_dn=True))
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
