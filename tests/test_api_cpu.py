"""CPU-only tests: host-side API parity with the reference's module surface, the C-ABI library
(loads, exports every declared symbol, validates arguments; no compute without a GPU), grids."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from reni_amd import _lib, utils
from reni_amd.models import RENIAutoDecoder, RENIVariationalAutoDecoder, get_model
from tests.util import load_golden


def load_golden_sd(g):
    return {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    declared = set(re.findall(r"\b(reni_[a-z_0-9]+)\s*\(", header))
    declared -= {"reni_desc", "reni_plan"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None


def test_binding_argtypes_are_the_headers_prototypes():
    """Every prototype of include/reni_hip.h against the ctypes binding, position by position: ctypes converts what it is given to
    the declared argtypes and checks nothing against the library, so a drifted list passes a pointer where a float belongs."""
    import ctypes
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    protos = re.findall(r"^([a-z_0-9 ]+?\*?)\s*\b(reni_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert {name for _, name, _ in protos} == set(_lib.EXPORTS) and len(protos) == len(_lib.EXPORTS)
    scalars = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
               "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}

    def agrees(ctype, decl, is_param):
        if "*" in decl or "[" in decl:
            return isinstance(ctype, type) and issubclass(ctype, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p))
        words = [w for w in decl.split() if w != "const"]
        base = " ".join(words[:-1] if is_param else words)   # (a parameter's last word is its name)
        return ctype is None if base == "void" else ctype is scalars[base]

    bad = []
    for ret, name, params in protos:
        fn = getattr(lib, name)
        want = [] if params.strip() == "void" else [x.strip() for x in params.split(",")]
        if fn.argtypes is None or len(fn.argtypes) != len(want):
            bad.append(f"{name}: argtypes {fn.argtypes!r} for {len(want)} parameters")
            continue
        bad += [f"{name}: parameter {i} `{d}` bound as {t.__name__}" for i, (t, d) in enumerate(zip(fn.argtypes, want))
                if not agrees(t, d, True)]
        if not agrees(fn.restype, ret.strip(), False):
            bad.append(f"{name}: returns `{ret.strip()}`, restype {fn.restype!r}")
    assert not bad, "\n".join(bad)


def test_binding_constants_are_the_headers():
    """The flag / enum values the Python binding passes are the ones include/reni_hip.h defines (a drifted constant would select
    another behaviour silently: RENI_WEIGHT_SPARSE is a bit of the same word as RENI_NEED_DW / RENI_NEED_DZ)."""
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(RENI_[A-Z_0-9]+)\s+(\d+u?)\b", header)}
    assert defs["RENI_NEED_DW"] == _lib.NEED_DW and defs["RENI_NEED_DZ"] == _lib.NEED_DZ and defs["RENI_WEIGHT_SPARSE"] == _lib.WEIGHT_SPARSE
    assert defs["RENI_WEIGHT_COMPACT"] == _lib.WEIGHT_COMPACT
    bits = [_lib.NEED_DW, _lib.NEED_DZ, _lib.WEIGHT_SPARSE, _lib.WEIGHT_COMPACT]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == 4   # four distinct bits of one word
    assert defs["RENI_LOSS_MSE"] == _lib.LOSS_MSE and defs["RENI_LOSS_TEST"] == _lib.LOSS_TEST


def test_plan_validation_and_counts():
    from reni_amd.ops import Plan
    p = Plan("SO2", 36, 128, 5, 3, True, "tanh", 30.0, 30.0, "bf16")
    assert p.n_params == 258435 and p.in_features == 1370
    p1 = Plan("SO2", 9, 64, 3, 3, True, None)
    assert p1.n_params == 19203 and p1.in_features == 101
    assert Plan("SO3", 49, 128, 5).in_features == 2450
    assert Plan("None", 9, 64, 3).in_features == 36
    assert Plan("SO2", 36, 256, 5).n_params == 256 * 1370 + 256 + 5 * (256 * 256 + 256) + 3 * 256 + 3  # reference default width
    assert p.lib.reni_workspace_bytes(p._h, 4, 32768, 3) > 0
    with pytest.raises(_lib.RENILibraryError, match="hidden_features"):
        Plan("SO2", 9, 100, 3)
    with pytest.raises(_lib.RENILibraryError, match="out_features"):
        Plan("SO2", 9, 64, 3, out_features=4)
    lib = _lib.load()
    assert lib.reni_plan_create(None, None) < 0 and b"NULL" in lib.reni_last_error()


def test_null_and_size_checks_without_gpu():
    from reni_amd.ops import Plan
    p = Plan("SO2", 9, 64, 3)
    lib = p.lib
    rc = lib.reni_forward(p._h, 1, 128, None, None, 0, None, None, None, 0, None)
    assert rc == -1 and b"non-NULL" in lib.reni_last_error()
    rc = lib.reni_forward(p._h, 0, 128, 8, 8, 0, 8, 8, 256, 0, None)
    assert rc == -1
    rc = lib.reni_adam_step(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None)
    assert rc == -1


def test_cpu_tensors_fail_loudly():
    m = RENIAutoDecoder(2, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        m(0, torch.zeros(1, 16, 3))


@pytest.mark.parametrize("mt,cls", [("AD", RENIAutoDecoder), ("VAD", RENIVariationalAutoDecoder)])
@pytest.mark.parametrize("eq", ["SO2", "SO3", "None"])
def test_state_dict_keys_shapes_and_seed_parity(golden, mt, cls, eq):
    g = golden("g9_api.npz")
    torch.manual_seed(9)
    m = cls(3, 9, eq, 64, 3, 3, True, "tanh", 30, 30, False)
    sd = m.state_dict()
    assert list(sd.keys()) == list(g[f"keys_{mt}_{eq}"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g[f"shapes_{mt}_{eq}"])
    assert m.in_features == int(g[f"infeat_{mt}_{eq}"])
    if mt == "AD" and eq == "SO2":  # same seed -> same initial weights as the reference, bit for bit
        for k, v in sd.items():
            assert np.array_equal(v.numpy(), g["sd." + k]), k


def test_flat_parameter_storage_and_reflatten():
    m = RENIAutoDecoder(2, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    flat = m._flat_params()
    assert flat.numel() == 19203
    ps = list(m.net.parameters())
    assert ps[0].data_ptr() == flat.data_ptr()
    with torch.no_grad():
        ps[1].add_(1.0)
    o = ps[0].numel()
    assert torch.equal(flat[o:o + 64], ps[1].detach())
    m2 = m.double().float()  # _apply re-flattens
    f2 = m2._flat_params()
    assert list(m2.net.parameters())[2].data_ptr() == f2.data_ptr() + 4 * (ps[0].numel() + ps[1].numel())


def test_load_state_dict_remap():
    torch.manual_seed(1)
    trained = RENIVariationalAutoDecoder(5, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    ckpt = {"model." + k: v.clone() for k, v in trained.state_dict().items()}
    frozen = RENIVariationalAutoDecoder(3, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, True)
    frozen.load_state_dict(ckpt)  # fixed decoder: only net.* is loaded, latents stay zero (RENI.py:196-201)
    assert float(frozen.mu.abs().sum()) == 0.0
    assert all(not p.requires_grad for p in frozen.net.parameters()) and not frozen.log_var.requires_grad
    for (k1, v1), (k2, v2) in zip(trained.net.state_dict().items(), frozen.net.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    full = RENIVariationalAutoDecoder(5, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    full.load_state_dict(ckpt)
    assert torch.equal(full.mu, trained.mu) and torch.equal(full.log_var, trained.log_var)
    assert torch.equal(full._flat_params(), trained._flat_params())


def _cfg(**over):
    r = dict(CONDITIONING="Cond-by-Concat", MODEL_TYPE="AutoDecoder", EQUIVARIANCE="SO2", LATENT_DIMENSION=9,
             HIDDEN_LAYERS=3, HIDDEN_FEATURES=64, OUT_FEATURES=3, LAST_LAYER_LINEAR=True, OUTPUT_ACTIVATION="tanh",
             FIRST_OMEGA_0=30.0, HIDDEN_OMEGA_0=30.0, MAPPING_LAYERS=3, MAPPING_FEATURES=64)
    r.update(over)
    return types.SimpleNamespace(RENI=types.SimpleNamespace(**r))


def test_get_model_factory():
    m = get_model(_cfg(), 7, "FIT_DECODER")
    assert isinstance(m, RENIAutoDecoder) and not m.fixed_decoder and m.Z.shape == (7, 9, 3)
    m = get_model(_cfg(MODEL_TYPE="VariationalAutoDecoder"), 7, "FIT_LATENT")
    assert isinstance(m, RENIVariationalAutoDecoder) and m.fixed_decoder
    assert float(m.mu.abs().sum()) == 0.0
    from reni_amd.film import RENIAutoDecoderFiLM, RENIVariationalAutoDecoderFiLM
    m = get_model(_cfg(CONDITIONING="FiLM"), 7, "FIT_DECODER")
    assert isinstance(m, RENIAutoDecoderFiLM) and len(m.net) == 3 and m.mapping_network.network[0].in_features == 90
    m = get_model(_cfg(CONDITIONING="FiLM", MODEL_TYPE="VariationalAutoDecoder"), 7, "FIT_INVERSE")
    assert isinstance(m, RENIVariationalAutoDecoderFiLM) and m.fixed_decoder
    assert not any(p.requires_grad for p in list(m.net.parameters()) + list(m.mapping_network.parameters()))


@pytest.mark.parametrize("tag", ["so2_ad", "so3_vad", "so2_one"])
def test_film_state_dict_seed_parity_and_glue(golden, tag):
    """FiLM modules: the reference's state-dict keys and, for the same torch seed, bit-identical initial values
    (RENI.py:563-596 RNG order); the per-image glue reproduces the reference's frequencies / phase shifts and the
    first layer's angle."""
    from reni_amd.film import RENIAutoDecoderFiLM, RENIVariationalAutoDecoderFiLM
    g = golden(f"g11_film_{tag}.npz")
    eq, nd, H, nF, mf, ml, act = [int(x) for x in g["cfg"]]
    cls = RENIVariationalAutoDecoderFiLM if "sd.mu" in g else RENIAutoDecoderFiLM
    torch.manual_seed(111)
    m = cls(2, nd, {1: "SO2", 2: "SO3"}[eq], H, nF, mf, ml, 3, {0: None, 1: "tanh", 2: "exp"}[act], False)
    sd = m.state_dict()
    want = load_golden_sd(g)
    assert sorted(sd) == sorted(want)
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    # flat storage: net.* then final_layer.* back the C ABI's `params`
    flat = m._flat_params()
    assert flat.numel() == sum(p.numel() for p in m._net_params()) and m.net[0].layer.weight.data_ptr() == flat.data_ptr()
    Z = torch.from_numpy(g["Z"])
    A, film = m._glue(Z)
    assert A.shape == (2, H, 8) and film.shape == (2, nF - 1, 2, H)
    fr = torch.from_numpy(g["freq_raw"]) * 15 + 30
    ph = torch.from_numpy(g["phase"])
    if nF > 1:
        assert float((film[:, :, 0].reshape(2, -1) - fr[:, H:]).abs().max()) <= 1e-5
        assert float((film[:, :, 1].reshape(2, -1) - ph[:, H:]).abs().max()) <= 1e-6
    si = torch.from_numpy(g["siren_input_head"])
    th_ref = fr[:, None, :H] * (si @ sd["net.0.layer.weight"].t() + sd["net.0.layer.bias"]) + ph[:, None, :H]
    D = utils.get_directions(int(g["W"]))[0, :8]
    x5 = torch.stack([D[:, 0], D[:, 1], D[:, 2], torch.sqrt(D[:, 0] ** 2 + D[:, 2] ** 2), torch.ones(8)], -1)
    assert float((torch.einsum("bhk,pk->bph", A[:, :, :5], x5) - th_ref).abs().max()) <= 2e-5
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        m(Z, D[None].repeat(2, 1, 1))


def test_film_plan_validation():
    from reni_amd.film import RENIAutoDecoderFiLM
    from reni_amd.ops import Plan
    p = Plan("SO2", 9, 64, 2, 3, True, "tanh", dtype="bf16", conditioning="film")
    assert p.in_features == 11 and p.n_params == 64 * 11 + 64 + 2 * (64 * 64 + 64) + 3 * 64 + 3
    assert Plan("SO3", 9, 64, 0, conditioning="film").in_features == 9
    with pytest.raises(_lib.RENILibraryError, match="None"):
        Plan("None", 9, 64, 2, conditioning="film")
    lib = p.lib
    assert lib.reni_forward(p._h, 1, 128, 8, 8, 0, 8, 8, 256, 0, None) == -1 and b"reni_film" in lib.reni_last_error()
    assert lib.reni_film_forward(p._h, 1, 128, 8, 0, None, 8, 8, 8, 256, 0, None) == -1
    m = RENIAutoDecoderFiLM(2, 9, "None", 64, 2, 32, 1, 3, None, False)  # constructible, as in the reference ...
    with pytest.raises(NotImplementedError):
        m._plan()                                                          # ... but never runnable


def test_vad_sample_latent_matches_reference_stream(golden):
    g = golden("g8_vad.npz")
    m = RENIVariationalAutoDecoder(3, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    m.load_state_dict({"model." + k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")})
    torch.manual_seed(80)
    Z, mu, lv = m.sample_latent(torch.from_numpy(g["idx"]))
    np.testing.assert_allclose(Z.detach().numpy(), g["Z"], atol=1e-7)


def test_grids_bitwise(golden):
    g = golden("g1_grids.npz")
    for W in (32, 64):
        assert np.array_equal(utils.get_directions(W).numpy(), g[f"dir_{W}"])
        assert np.array_equal(utils.get_sineweight(W).numpy(), g[f"sw_{W}"])
    d = utils.get_directions(256)
    assert np.array_equal(d[0, -64:].numpy(), g["dir_256_tail"])


def test_get_mask(tmp_path, golden):
    from PIL import Image
    g = golden("g7_latent_opt.npz")
    src = g["mask_src"]
    Image.fromarray(np.stack([src] * 3, -1)).save(tmp_path / "m.png")
    m = utils.get_mask(64, str(tmp_path / "m.png"))
    assert m.shape == (1, 32 * 64, 3)
    assert np.array_equal(m.numpy(), g["mask"])
    assert abs(float(m.mean()) - 0.188) < 0.01  # Mask-3 keeps ~18.8 % of the pixels


@pytest.mark.parametrize("W", [64, 100, 128, 256])
def test_get_mask_is_the_tensor_nearest_resize(tmp_path, golden, W):
    """utils.get_mask against what torchvision 0.11's tensor path of Resize(NEAREST) calls -- torch.nn.functional.interpolate(
    mode="nearest") on the ToTensor-equivalent CHW tensor (utils.py:81-91; the G7 golden's mask is generated the same way since
    round 3): the fixture's Mask-3, random binary 512 x 256 masks (the index rule at a non-integer ratio too), and the reference's
    five mask files (their pixels travel in tests/golden/masks.npz)."""
    from PIL import Image
    srcs = {"mask3": golden("g7_latent_opt.npz")["mask_src"]}
    rng = np.random.default_rng(W)
    srcs["rand"] = (rng.random((256, 512)) > 0.5).astype(np.uint8) * 255
    srcs.update(golden("masks.npz"))
    assert len(srcs) == 7
    for name, src in srcs.items():
        arr = src if src.ndim == 3 else np.stack([src] * 3, -1)
        path = tmp_path / f"{name}.png"
        Image.fromarray(arr).save(path)
        got = utils.get_mask(W, str(path))
        chw = torch.from_numpy(arr[..., :3].astype(np.float32) / 255.0).permute(2, 0, 1)
        want = torch.nn.functional.interpolate(chw[None], size=(W // 2, W), mode="nearest")[0].permute(1, 2, 0).reshape(1, -1, 3)
        assert torch.equal(got, want), name


def test_hdr_transforms_match_reference(golden):
    """MinMaxNormalise / UnMinMaxNormlise / UnNormalise / sRGB against the reference's outputs (G12)."""
    from reni_amd.custom_transforms import MinMaxNormalise, UnMinMaxNormlise, UnNormalise, transform_builder
    g = golden("g12_transforms.npz")
    img = torch.from_numpy(g["img"])
    minmax = [float(g["minmax"][0]), float(g["minmax"][1])]
    n = MinMaxNormalise(minmax)(img.clone())
    assert np.array_equal(n.numpy(), g["normalised"])
    assert np.array_equal(transform_builder([("minmaxnormalise", minmax)])(img.clone()).numpy(), g["normalised"])
    u = UnMinMaxNormlise(minmax)(n.clone())
    assert np.array_equal(u.numpy(), g["unnormalised"])
    un = UnNormalise([0.1, 0.2, 0.3], [1.5, 2.5, 3.5])(torch.from_numpy(g["batch"]).clone())
    assert np.array_equal(un.numpy(), g["unnorm_batch"])
    np.testing.assert_allclose(utils.sRGB(u.clone()).numpy(), g["srgb1"], rtol=0, atol=1e-6)
    x2 = torch.rand(2, 3, 8, 16, generator=torch.Generator().manual_seed(13)) * 3.0
    np.testing.assert_allclose(utils.sRGB(x2).numpy(), g["srgb2"], rtol=0, atol=1e-6)
    # resize restates torchvision's tensor path (bilinear, align_corners=False, no antialias); the random augmentations raise
    r = transform_builder([("resize", [4, 8])])(x2[0])
    assert torch.equal(r, torch.nn.functional.interpolate(x2[:1], size=(4, 8), mode="bilinear", align_corners=False)[0])
    with pytest.raises(NotImplementedError, match="torchvision"):
        transform_builder([("randomcrop", 8)])


def test_envmap_shader_surface():
    """reni_amd.envmap_shader mirrors src/utils/pytorch3d_envmap_shader.py: EnvironmentMap pre-multiplies the sine
    weight (:41), the interpolation matches the oracle's, the shading itself has no CPU path, build_renderer needs
    pytorch3d."""
    import pytest
    from oracle import reni_oracle as O
    from reni_amd import _lib
    from reni_amd import envmap_shader as es
    g = torch.Generator().manual_seed(0)
    env, sw, D = torch.rand(2, 8, 3, generator=g), torch.rand(2, 8, 3, generator=g), torch.randn(2, 8, 3, generator=g)
    em = es.EnvironmentMap(environment_map=env, directions=D, sineweight=sw)
    assert torch.equal(em.environment_map, env * sw) and em.directions is D
    p2f = torch.randint(-1, 5, (1, 4, 3, 1), generator=g)
    bary = torch.rand(1, 4, 3, 1, 3, generator=g)
    attrs = torch.randn(5, 3, 3, generator=g)
    assert torch.equal(es.interpolate_face_attributes(p2f, bary, attrs), O.interpolate_face_attributes(p2f, bary, attrs))
    with pytest.raises(_lib.RENILibraryError):
        es.blinn_phong_shading_gbuffer(torch.randn(5, 3), torch.randn(5, 3), torch.tensor([0.0, 0.0, 2.0]), em, 500.0, 0.5, 0.5)
    with pytest.raises(ImportError):
        es.build_renderer("teapot.obj", 90, 128, 0.5, "cpu")
    r = es.GBufferRenderer(es.GBuffer(torch.randn(16, 3), torch.randn(16, 3), [0.0, 0.0, 2.0], 4), kd=0.3)
    assert abs(r.ks - 0.7) < 1e-12 and r.shininess == 500.0 and r.gbuffer.image_size == (4, 4)


def test_mask3_geometry_behind_the_sparse_weight_records():
    """The figures bench.py's config-4 records and DESIGN.md quote for the notebook's Mask-3 at 128 x 256 (examples.ipynb cell 4;
    resized by get_mask's nearest rule, utils.py:81-91): rows 20-93 x columns 81-164 kept = 19.0 % of the pixels, pixel 0 masked (so
    RENITestLoss's cosine term, which carries pixel 0's weight, is a constant), 148 of the 256 tiles of 128 consecutive pixels touched
    (RENI_WEIGHT_SPARSE) and 49 tiles' worth of pixels (RENI_WEIGHT_COMPACT)."""
    import bench
    m = bench.mask3(256)
    assert tuple(m.shape) == (1, 128 * 256, 3) and set(m.unique().tolist()) == {0.0, 1.0}
    g = m.view(128, 256, 3)[..., 0]
    rows, cols = g.any(1).nonzero().flatten(), g.any(0).nonzero().flatten()
    assert (int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())) == (20, 93, 81, 164)
    assert float(g[0, 0]) == 0.0 and abs(float(g.mean()) - 0.1897) < 1e-4
    live = g.reshape(-1) != 0
    assert int(live.view(-1, 128).any(1).sum()) == 148 and (int(live.sum()) + 127) // 128 == 49


def test_pmc_traffic_record_belongs_to_the_committed_kernel_sources():
    """bench.py's `roofline.traffic` comes from profiles/pmc_traffic.json and is printed only when the record's source hash equals
    the hash of reni_amd/csrc -- a kernel edit without a new PMC pass (profiles/tools/gpu_profile_round.sh) must not go unnoticed."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    rec = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    sha = bench.kernel_src_sha()
    # (round 5: the L0X instance and k_reni_l0_ring are what config 2 runs; the H = 256 chain's three forms have entries of their own)
    for kernel in ("k_reni_train_bf16<128,true,L0X>", "k_reni_l0_ring", "k_reni_train_bf16<128,false>", "k_reni_main<f32,H=128,FWD>",
                   "k_reni_wide256<0>", "k_reni_wide256<1>", "k_reni_wide256<2>"):
        assert rec[kernel]["src_sha256"] == sha, f"{kernel}: PMC record is of another source state"
        assert bench.pmc_record(kernel).get("hbm_bytes_per_launch"), kernel


def test_bench_contract_line_stays_short_and_last(capsys):
    """round 5's 24 KB contract line (14 sub-records inside it) did not parse on the driver's side.  bench.py now prints the
    sub-records on `also <name> {json}` lines and ends with ONE contract line of at most bench.LINE_MAX = 6144 bytes that keeps
    [value, ms_per_step, frac_step] of each -- checked here on a synthetic record with every field at full width."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    roof = {"bound": "mfma+valu_issue", "achieved": 820.1723456789, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.3280691234, "frac_step": 0.2758141234,
            "frac_issued": 0.2827861234, "traffic": 2924134400, "kernel": "k_reni_train_bf16<128,true,L0X>", "kernel_avg_ms": 1.336741234,
            "kernel_min_ms": 1.281171234, "kernel_max_ms": 1.466891234, "kernel_launches": 20, "work_kernels_ms_per_step": 1.51441234, "flop_per_sample": 522784,
            "kernels": [{"kernel": "k_reni_train_bf16<128,true,L0X>", "avg_ms": 1.336741234, "frac_issued": 0.282786, "traffic": 2924134400},
                        {"kernel": "k_reni_l0_ring", "avg_ms": 0.1776661234, "min_ms": 0.171234, "max_ms": 0.181234, "launches": 20, "traffic": 557608960,
                         "frac_issued": 0.4061291234, "hbm_frac": 0.3923161234}],
            "valu_per_mfma": 7.221, "trans_per_mfma": 2.1, "issue_limited_frac": 0.6186431234}
    paths = {"persistent_kernels": True, "dw1_kernel": "k_reni_l0_ring", "side_stream": True, "images_per_chunk": 64, "operand_stream": False,
             "fragment_stream": "none", "env_overrides": ["RENI_NO_L0X", "RENI_FRAG_WS_CAP_MB"], "workgroups": 256}
    rec = {"value": 1318971234.5678, "ms_per_step": 1.589991234, "steps": 20, "warmup": 5, "dtype": "bf16", "launches_per_step": 6.0,
           "config": {"workload": "BASELINE config 2: 615-image set, 128x256 equirect, ND=36, 5x128 SIREN, SO2, tanh, AutoDecoder, RENITrainLoss; "
                                  "full training step (fwd+loss+bwd, grad all-reduce, Adam)", "images_per_gpu_per_step": 64, "global_batch_images": 512,
                      "directions_per_image": 32768, "parallelism": "dp8", "result_check": 0.7507611234, "paths": paths,
                      "step_call": "reni_train_step_rows_dp (one call: fwd+loss+bwd, RCCL all-reduce inside, Adam, next prologue)"},
           "roofline": roof,
           "exchange": {"kind": "inside reni_train_step_rows_dp (librccl, the library's communicator)", "avg_us_on_compute_stream": 41.51234,
                        "comm_fallback": "x" * 200}}
    names = ("c4", "c4_dense", "c4_pixels", "c4_f32", "c5", "film", "c2_b100", "c2_curric_16x32", "c2_curric_32x64", "c2_curric_64x128", "c2_h256",
             "c4_h256", "c4_h256_dense", "fwd_h256", "film_h256")
    also = {n: {"value": 1234567890.1234, "ms_per_step": 0.4645531234, "roofline": dict(roof), "workload": "w" * 300, "paths": paths} for n in names}
    also["film"] = {"error": "RuntimeError: " + "e" * 300}
    sustained = {"value": 1351431234.5, "ms_per_step": 1.55181234, "kernel_avg_ms": 1.301341234, "frac": 0.3369941234, "frac_step": 0.281234, "steps": 20,
                 "warmup": 5, "note": "the same W+K steps again behind the sub-records (sustained clocks); not `value`"}
    cpu = {"value": 46525.81234, "unit": "samples/s", "cores": 128, "kind": "port", "port_b1": 46525.81234, "port_b4": 40755.81234, "factored": 66715.71234,
           "factored_b1": 66715.71234, "factored_b4": 54558.61234, "sample": "s" * 260}
    line = bench.contract_line(bench.METRIC_TRAIN, rec, 1, also, sustained, cpu)
    bench.emit(line, also)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == len(names) + 1 and all(ln.startswith("also ") for ln in out[:-1]) and out[-1].startswith("{")
    assert len(out[-1]) <= bench.LINE_MAX == 6144, len(out[-1])
    got = json.loads(out[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "sustained", "step_call", "also"):
        assert key in got, key
    assert got["config"]["workload"].startswith("BASELINE config 2") and "model" not in got["config"]
    assert set(got["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "frac_step", "frac_issued", "traffic", "kernel", "kernels"}
    assert got["also"]["c4"] == [1234570000.0, 0.464553, 0.275814] and "error" in got["also"]["film"]
    assert got["step_call"].startswith("reni_train_step_rows_dp") and set(got["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    sub = json.loads(out[0].split(" ", 2)[2])
    assert out[0].split(" ", 2)[1] == "c4" and sub["roofline"]["kernel"] == roof["kernel"]


def test_bench_dump_outputs_stays_within_its_budget(tmp_path):
    """bench.py --dump-outputs: every array as float32 .npy; small ones whole, one larger than its share of 64 MB replaced by a seeded
    sample of its elements -- the same positions in every run, so two builds' dumps compare element for element."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    big = torch.arange(16 * 524288 * 3, dtype=torch.float32).view(16, 524288, 3)   # 100 MB: config 5's output at 16 images
    terms = torch.tensor([0.5, 0.25, 0.125, 0.0625], dtype=torch.float64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"output": big, "loss_terms": terms})
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert [p.name for p in files] == ["loss_terms.npy", "output.npy"] and sum(p.stat().st_size for p in files) <= 64e6
    t, o = np.load(tmp_path / "a" / "loss_terms.npy"), np.load(tmp_path / "a" / "output.npy")
    assert t.dtype == np.float32 and np.array_equal(t, terms.numpy().astype(np.float32))
    assert o.dtype == np.float32 and 15e6 < o.size < big.numel() and np.all(np.diff(o) >= 0)   # positions in order
    assert np.array_equal(o, np.load(tmp_path / "b" / "output.npy"))


def test_rocpd_summary_finds_the_training_instance_by_prefix(tmp_path):
    """profiles/summarize_rocpd.py: the headline / sustained window lines must exist for the CURRENT name of the training instance (it
    gained a template argument in round 5 and the summary, matching the round-4 name exactly, silently printed no window lines for a
    whole round) and for the ring kernel."""
    import sqlite3
    import subprocess
    import sys
    db = tmp_path / "k.db"
    c = sqlite3.connect(db)
    c.execute("create table kernels (name text, start integer, end integer)")
    t = 0
    for i in range(30):
        for name, dur in (("void reni::k_reni_train_bf16<128, true, false, false, true, true>(reni::MainArgs)", 1300000 + 1000 * i),
                          ("void reni::k_reni_l0_ring<128>(reni::MainArgs)", 170000 + 100 * i)):
            c.execute("insert into kernels values (?, ?, ?)", (name, t, t + dur))
            t += dur + 5000
    c.commit(); c.close()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "summarize_rocpd.py"), str(db), str(tmp_path / "o.md"), "20", "5"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "window" in ln]
    assert len(lines) == 4, out
    assert "launches 5..24" in lines[0] and "avg 1314.5 us" in lines[0], lines[0]     # mean of 1305 .. 1324
    assert "k_reni_l0_ring" in lines[2] and "avg 171.4 us" in lines[2], lines[2]


def test_isa_audit_lists_functions_with_mfma_even_without_near_accesses():
    from tests import isa_audit
    text = "\n".join(["_Zfoo:", "\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]"] + ["\ts_nop 7"] * 8 + ["\ts_endpgm", "_Zbar:", "\tv_add_f32 v0, v1, v2", "\ts_endpgm"])
    assert isa_audit.mfma_functions(text) == {"_Zfoo"}
    assert not any(f == "_Zfoo" for f, _ in isa_audit.audit(text))      # (no access within the horizon: audit() alone does not list it)
