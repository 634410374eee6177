"""The device-resident dataset (reni_amd.data.ResidentDataset): its levels against the wrapped dataset's own pipeline
evaluated in float64, one decode per file over a whole fit, loss histories bit-equal to the same tensors fed from the host,
FIT_LATENT / FIT_INVERSE through ``__getitem__``, and the memory it keeps."""
import math
import types

import numpy as np
import pytest
import torch

from tests.test_gpu_workflows import _config, _task

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24


def _write_exr_dir(d, n, h=128, w=256, seed=0):
    """n half-float ZIP EXR files: a positive sky and a sun, a different one per file"""
    from reni_amd import exr
    d.mkdir(parents=True, exist_ok=True)
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i in range(n):
        sky = np.exp(2.0 * np.cos(np.pi * yy / h) + 0.3 * i)[:, :, None] * np.array([0.6, 0.8, 1.0])
        sky = sky * (0.9 + 0.2 * g.random((h, w, 1)))
        sun = 500.0 * np.exp(-((yy - h // 5 - i) ** 2 + (xx - w // 3 - 5 * i) ** 2) / (h / 5.0))[:, :, None]
        exr.write_exr(str(d / f"env{i + 1}.exr"), (sky + sun).astype(np.float32), pixel_type="half", compression="zip")


def _hdr_dataset(path, size, minmax=()):
    from reni_amd.custom_transforms import transform_builder
    from reni_amd.data import RENIDatasetHDR
    return RENIDatasetHDR(str(path), transform_builder([["resize", list(size)], ["minmaxnormalise", list(minmax)]]))


def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23)


class _HostLevels(torch.utils.data.Dataset):
    """a plain host dataset holding copies of a resident dataset's level tensors"""

    def __init__(self, levels, unnormalise):
        self.levels, self.level, self.unnormalise = [t.cpu().clone() for t in levels], 0, unnormalise

    def __len__(self):
        return self.levels[0].shape[0]

    def __getitem__(self, i):
        return self.levels[self.level][i].clone(), i

    def double_resolution(self):
        self.level += 1


def test_levels_equal_the_float64_pipeline_of_the_wrapped_hdr_dataset(tmp_path):
    """★ Resize on .double(), then the MinMaxNormalise formula, against the device levels 16 x 32 .. 128 x 256 and one
    upsampled level (256 x 512).  Bound: (16 2^-24 + 2 ulp32(max|log|)) 2 / (m1 - m0) + 2^-23 -- the interpolation's rounding
    (relative in the linear domain = absolute in the log domain), the fp32 logf and its subtraction, the final affine map."""
    from reni_amd.custom_transforms import MinMaxNormalise, Resize
    from reni_amd.data import ResidentDataset
    _write_exr_dir(tmp_path / "hdr", 6)
    ds = _hdr_dataset(tmp_path / "hdr", (16, 32))
    m0, m1 = ds.transforms.transforms[1].minmax  # from the data (calculate_minmax)
    rd = ResidentDataset(ds, levels=4, device=DEV)
    assert len(rd) == 6 and rd.sizes == [(16, 32), (32, 64), (64, 128), (128, 256), (256, 512)]
    assert rd.unnormalise is ds.unnormalise and rd.img_names == ds.img_names and rd.transforms is ds.transforms
    bound = (16 * EPS32 + 2 * _ulp32(max(abs(m0), abs(m1)))) * 2 / (m1 - m0) + 2.0 ** -23
    print(f"minmax {m0:.4f} {m1:.4f}: bound {bound:.3e}")
    worst = 0.0
    for j, size in enumerate(rd.sizes):
        for i in range(6):
            got, idx = rd[i]
            assert idx == i and got.is_cuda and got.dtype == torch.float32 and got.shape == (3,) + size
            src = ds.get_image(i).double()
            ref = torch.nan_to_num(MinMaxNormalise((m0, m1))(Resize(size)(src)))
            err = float((got.double().cpu() - ref).abs().max())
            worst = max(worst, err)
            assert err <= bound, (j, i, err, bound)
        b = rd.batch([5, 0, 3])
        assert b.shape == (3, 3) + size and torch.equal(b[0], rd[5][0]) and torch.equal(b[1], rd[0][0])
        assert torch.equal(rd.batch(torch.tensor([5, 0, 3])), b)
        if j + 1 < len(rd.sizes):
            rd.double_resolution()
            assert tuple(ds.transforms.transforms[0].size) == rd.sizes[j + 1]  # the wrapped Resize follows
    print(f"largest error over 5 levels x 6 files: {worst:.3e} ({worst / bound:.2f} of the bound)")
    # beyond the last level: rebuilt from the files at twice the size
    rd.double_resolution()
    assert rd.size == (512, 1024) and rd[2][0].shape == (3, 512, 1024)


def test_non_dyadic_target_and_mixed_file_sizes_against_float64(tmp_path):
    from reni_amd import exr
    from reni_amd.custom_transforms import MinMaxNormalise, Resize
    from reni_amd.data import ResidentDataset
    _write_exr_dir(tmp_path / "hdr", 2, 128, 256)
    g = np.random.default_rng(4)
    exr.write_exr(str(tmp_path / "hdr" / "env9.exr"), (0.1 + g.random((50, 100, 3))).astype(np.float32), pixel_type="half",
                  compression="zip")
    ds = _hdr_dataset(tmp_path / "hdr", (24, 48))
    m0, m1 = ds.transforms.transforms[1].minmax
    rd = ResidentDataset(ds, levels=1, device=DEV)
    bound = (16 * EPS32 + 2 * _ulp32(max(abs(m0), abs(m1)))) * 2 / (m1 - m0) + 2.0 ** -23
    for j, size in enumerate(((24, 48), (48, 96))):
        for i in range(3):
            ref = torch.nan_to_num(MinMaxNormalise((m0, m1))(Resize(size)(ds.get_image(i).double())))
            assert float((rd[i][0].double().cpu() - ref).abs().max()) <= bound
        rd.double_resolution()


def test_ldr_directory_against_float64(tmp_path):
    """PNG through PIL, ToTensor, Resize, Normalize.  Bound: the interpolation's 8 2^-24 max|x| and the subtraction's and
    division's roundings, over the smallest std, plus one rounding of the result."""
    from PIL import Image
    from reni_amd.custom_transforms import Normalize, Resize, transform_builder
    from reni_amd.data import RENIDatasetLDR, ResidentDataset
    d = tmp_path / "ldr"
    d.mkdir()
    g = np.random.default_rng(8)
    for i in range(3):
        a = (g.random((64, 128, 4 if i == 1 else 3)) * 255).astype(np.uint8)  # one file with an alpha channel
        Image.fromarray(a).save(d / f"img{i}.png")
    mean, std = [0.5, 0.4, 0.3], [0.25, 0.2, 0.3]
    ds = RENIDatasetLDR(str(d), transform_builder([["resize", [16, 32]], ["normalize", [mean, std]]]))
    rd = ResidentDataset(ds, levels=2, device=DEV)
    assert rd.unnormalise is ds.unnormalise
    for size in ((16, 32), (32, 64), (64, 128)):
        for i in range(3):
            ref = Normalize(mean, std)(Resize(size)(ds.get_image(i)[:3].double()))
            got = rd[i][0]
            assert got.shape == (3,) + size
            bound = (8 + 2) * EPS32 / min(std) + 2.0 ** -23 * float(ref.abs().max())
            assert float((got.double().cpu() - ref).abs().max()) <= bound
        rd.double_resolution()


def test_unsupported_transforms_are_named(tmp_path):
    from reni_amd.custom_transforms import CenterCrop, MinMaxNormalise, Resize, _Compose
    from reni_amd.data import RENIDatasetHDR, ResidentDataset
    _write_exr_dir(tmp_path / "hdr", 1, 16, 32)
    with pytest.raises(ValueError, match="CenterCrop"):
        ResidentDataset(RENIDatasetHDR(str(tmp_path / "hdr"), _Compose([Resize((8, 16)), CenterCrop(8), MinMaxNormalise((-1.0, 3.0))])),
                        device=DEV)
    with pytest.raises(ValueError, match="Resize"):
        ResidentDataset(RENIDatasetHDR(str(tmp_path / "hdr"), _Compose([MinMaxNormalise((-1.0, 3.0))])), device=DEV)
    with pytest.raises(ValueError):
        ResidentDataset(torch.utils.data.TensorDataset(torch.zeros(2, 3)), device=DEV)


def _fit_cfg(path, minmax, resident):
    cfg = _config(LR_START=1e-2, LR_END=1e-3, SCHEDULER_TYPE="exponential", EPOCHS=6, BATCH_SIZE=2,
                  MULTI_RES_TRAINING=True, INITAL_RESOLUTION=[16, 32], FINAL_RESOLUTION=[32, 64], CURRICULUM=[3])
    cfg.DATASET = types.SimpleNamespace(NAME="RENI_HDR", RENI_HDR=types.SimpleNamespace(
        PATH=str(path), TRANSFORMS=[["minmaxnormalise", list(minmax)]], IS_HDR=True))
    if resident:
        cfg.DATASET.RESIDENT = True
    return cfg


def test_fit_decodes_every_file_once_and_equals_the_injected_tensor_fit(tmp_path, monkeypatch):
    """★ the curriculum of test_fit_decoder_from_exr_files_on_disk with DATASET.RESIDENT = True"""
    from reni_amd import exr, trainer
    from reni_amd.data import RENIDatasetHDR, ResidentDataset
    from reni_amd.lightning_module import RENI
    _write_exr_dir(tmp_path / "hdr" / "Train", 4, 32, 64)
    minmax = _hdr_dataset(tmp_path / "hdr" / "Train", (16, 32)).transforms.transforms[1].minmax  # from the data
    calls = []
    real = exr.read_exr

    def counted(path, *a, **k):
        calls.append(str(path))
        return real(path, *a, **k)

    monkeypatch.setattr(exr, "read_exr", counted)
    torch.manual_seed(0)
    mod = RENI(_fit_cfg(tmp_path / "hdr", minmax, True), "FIT_DECODER")
    hist = trainer.fit(mod, max_epochs=6, device=DEV)
    rd = mod.dataset
    assert isinstance(rd, ResidentDataset) and isinstance(rd.dataset, RENIDatasetHDR)
    assert len(calls) == 4 and len(set(calls)) == 4, calls  # once per file over six epochs and one doubling
    assert mod.cur_res == [32, 64] and rd.sizes == [(16, 32), (32, 64)] and rd.level == 1
    assert rd[0][0].shape == (3, 32, 64) and rd.batch([0, 1]).shape == (2, 3, 32, 64) and len(calls) == 4
    assert rd.level_tensor(0).shape == (4, 3, 16, 32) and rd.level_tensor(1).shape == (4, 3, 32, 64)
    losses = [h["loss"] for h in hist]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]

    # the default path reads every file every epoch
    del calls[:]
    torch.manual_seed(0)
    plain = RENI(_fit_cfg(tmp_path / "hdr", minmax, False), "FIT_DECODER")
    hist_plain = trainer.fit(plain, max_epochs=6, device=DEV)
    assert isinstance(plain.dataset, RENIDatasetHDR) and len(calls) >= 6 * 4
    monkeypatch.undo()

    # the same tensors from a plain host dataset: the same loss history, bit for bit
    host = _HostLevels([rd.level_tensor(0), rd.level_tensor(1)], rd.unnormalise)
    torch.manual_seed(0)
    inj = RENI(_fit_cfg(tmp_path / "hdr", minmax, False), "FIT_DECODER", dataset=host)
    hist_host = trainer.fit(inj, max_epochs=6, device=DEV)
    assert hist_host == hist
    assert host.level == 1 and inj.cur_res == [32, 64]
    # (the host pipeline's own fp32 images differ from the device's by rounding: its history is close, not equal)
    print("resident", losses, "host pipeline", [h["loss"] for h in hist_plain])


def test_fit_latent_with_a_mask_on_a_resident_dataset(tmp_path):
    from PIL import Image
    from reni_amd import trainer
    from reni_amd.data import ResidentDataset
    from reni_amd.lightning_module import RENI
    _write_exr_dir(tmp_path / "hdr", 3, 32, 64)
    m = np.zeros((64, 128, 3), np.uint8)
    m[:, :80] = 255
    Image.fromarray(m).save(tmp_path / "mask.png")
    rd = ResidentDataset(_hdr_dataset(tmp_path / "hdr", (16, 32)), levels=0, device=DEV)
    hists = []
    for ds in (rd, None):
        ds = ds if ds is not None else _HostLevels([rd.level_tensor(0)], rd.unnormalise)
        cfg = _config(LR_START=1e-1, LR_END=1e-1, BATCH_SIZE=3, APPLY_MASK=True, MASK_PATH=str(tmp_path / "mask.png"), EPOCHS=4)
        torch.manual_seed(1)
        mod = RENI(cfg, "FIT_LATENT", dataset=ds)
        hists.append(trainer.fit(mod, max_epochs=3, device=DEV))
        assert mod.mask is not None
    assert all(np.isfinite(h["loss"]) for h in hists[0]) and hists[0] == hists[1]


def test_fit_inverse_renders_and_steps_on_a_resident_dataset(tmp_path):
    from reni_amd.data import ResidentDataset
    from reni_amd.envmap_shader import GBuffer, GBufferRenderer
    from reni_amd.lightning_module import RENI
    from tests.test_gpu_shader import _problem
    _write_exr_dir(tmp_path / "hdr", 4, 32, 64)
    rd = ResidentDataset(_hdr_dataset(tmp_path / "hdr", (16, 32)), levels=0, device=DEV)
    nrm, pos, cam, _, _ = _problem(1, 400, 4, seed=11)
    res = []
    for ds in (rd, None):
        ds = ds if ds is not None else _HostLevels([rd.level_tensor(0)], rd.unnormalise)  # (copied once the first pass has filled it)
        cfg = _config("VariationalAutoDecoder")
        cfg.RENI.FIT_INVERSE = _task(BATCH_SIZE=3, COSINE_SIMILARITY_WEIGHT=1e-3)
        torch.manual_seed(2)
        m = RENI(cfg, "FIT_INVERSE", dataset=ds)
        m.setup()
        m.model.to(DEV)
        with torch.no_grad():
            m.model.mu.normal_()
        m.set_renderer(GBufferRenderer(GBuffer(nrm, pos, cam, 20), kd=0.5))  # generate_gt_renders goes through __getitem__
        idx = torch.tensor([0, 2, 3])
        imgs = torch.stack([ds[int(i)][0] for i in idx]).to(DEV)
        out = m.training_step((imgs, idx.to(DEV)), 0)
        out["loss"].backward()
        assert torch.isfinite(out["loss"]) and bool(torch.isfinite(m.model.mu.grad).all())
        res.append((m.gt_renders.clone(), out["loss"].detach().clone()))
    assert res[0][0].shape == (4, 20, 20, 3) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_no_source_image_stays_on_the_device(tmp_path):
    from reni_amd.data import ResidentDataset
    _write_exr_dir(tmp_path / "hdr", 5, 256, 512)
    ds = _hdr_dataset(tmp_path / "hdr", (16, 32), minmax=(-3.0, 8.0))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    rd = ResidentDataset(ds, levels=2, device=DEV)
    rd.fill()
    assert rd.batch([0, 1, 2, 3, 4]).shape == (5, 3, 16, 32)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated(DEV) - before
    level_bytes = sum(5 * 3 * h * w * 4 for h, w in rd.sizes)
    source = 3 * 256 * 512 * 4
    print(f"allocated grew by {grown} bytes; levels {level_bytes}, one source {source}")
    assert grown <= level_bytes + source + (1 << 20)
    assert grown < 5 * source  # five retained sources would be 7.5 MB
