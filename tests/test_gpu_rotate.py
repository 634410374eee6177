"""GPU tests of the environment-map rotation (reni_tu_rotate.hip through ops.rotate_envmap, reni_amd/rotation.py and
ResidentDataset's augmentation) against the float64 oracle and the derived bound of tests/test_rotate_cpu.py.

Largest err / bound of the bilinear kernel, measured on an MI355X over the thirteen rotations and both maps
(test_bilinear_against_the_float64_oracle prints one line per rotation): 0.111 at 16 x 32, 0.155 at 64 x 128, 0.180 at
128 x 256, 0.165 at 512 x 1024; at most 32, 112, 188 and 200 pixels left out."""
import math

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from tests.test_gpu_resident import _fit_cfg, _hdr_dataset, _write_exr_dir
from tests.test_rotate_cpu import (FLIP_X, FLIP_Y, FLIP_Z, Ry, np_rotate_envmap, rotate_bound, rotation_list, sky_maps)
from tests.util import flat_params, load_golden, make_plan, sd_from

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(R):
    return torch.from_numpy(np.asarray(R, np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------ 5. bilinear against the oracle
@pytest.mark.parametrize("size", [(16, 32), (64, 128), (128, 256), (512, 1024)])
def test_bilinear_against_the_float64_oracle(size):
    from reni_amd import ops
    H, W = size
    x = sky_maps(2, H, W, H + W)
    xd = torch.from_numpy(x).to(DEV)
    worst, most_left = 0.0, 0
    for name, R in rotation_list():
        R32 = R.astype(np.float32)  # the oracle turns by the very numbers the kernel is given
        got = ops.rotate_envmap(xd, _t(R32)).double().cpu().numpy()
        ref = np_rotate_envmap(x, R32)
        bound, keep = rotate_bound(x, R32)
        err = np.abs(got - ref)
        ratio = float((err / bound)[..., keep].max())
        left = int((~keep).sum())
        print(f"{H}x{W} {name}: max err {float(err[..., keep].max()):.3e}, largest err / bound {ratio:.3f}, left out {left} of {H * W}")
        worst, most_left = max(worst, ratio), max(most_left, left)
        assert got.shape == ref.shape
        assert left * H <= 2 * H * W  # at most 2 / H of the map
        assert ratio <= 1.0
        # every pixel, the caps included: finite, and a convex combination of source pixels
        assert np.isfinite(got).all()
        for n in range(2):
            assert got[n].min() >= x[n].min() and got[n].max() <= x[n].max()
    print(f"{H}x{W}: largest err / bound over all rotations {worst:.3f}, most pixels left out {most_left}")


# ------------------------------------------------------------------------------------------ 6. nearest: exact
@pytest.mark.parametrize("size", [(16, 32), (128, 256)])
def test_nearest_half_turns_and_pixel_yaws_are_flips_and_rolls(size):
    from reni_amd import ops
    H, W = size
    x = torch.from_numpy(sky_maps(2, H, W, 7)).to(DEV)
    assert torch.equal(ops.rotate_envmap(x, _t(np.eye(3)), "nearest"), x)
    assert torch.equal(ops.rotate_envmap(x, _t(FLIP_Y), "nearest"), torch.roll(x, W // 2, -1))
    assert torch.equal(ops.rotate_envmap(x, _t(FLIP_Z), "nearest"), x.flip(-1, -2))
    assert torch.equal(ops.rotate_envmap(x, _t(FLIP_X), "nearest"), torch.roll(x.flip(-1, -2), W // 2, -1))
    for k in (1, 3, -5, W // 4 + 1, W - 2):
        assert torch.equal(ops.rotate_envmap(x, _t(Ry(k * 2 * math.pi / W)), "nearest"), torch.roll(x, -k, -1)), k


def test_rotate_mask_on_the_golden_masks(golden):
    from reni_amd import rotation
    from reni_amd.utils import mask_from_array
    masks = golden("masks.npz")
    assert len(masks) >= 5
    W = 128
    for name, m in masks.items():
        mask = mask_from_array(W, m).to(DEV)  # [1, P, 3]
        assert set(torch.unique(mask).tolist()) <= {0.0, 1.0}
        for rname, R in rotation_list():
            out = rotation.rotate_mask(mask, _t(R))
            assert out.shape == mask.shape and set(torch.unique(out).tolist()) <= {0.0, 1.0}, (name, rname)
        for k in (1, 9, -20):
            out = rotation.rotate_mask(mask, rotation.rotation_y(k * 2 * math.pi / W).to(DEV))
            want = torch.roll(mask.reshape(1, W // 2, W, 3), -k, 2).reshape(1, -1, 3)
            assert torch.equal(out, want), (name, k)
        ref = np_rotate_envmap(mask[0].cpu().numpy().reshape(W // 2, W, 3).transpose(2, 0, 1), rotation_list()[1][1].astype(np.float32), "nearest")
        got = rotation.rotate_mask(mask, _t(rotation_list()[1][1]))[0].cpu().numpy().reshape(W // 2, W, 3).transpose(2, 0, 1)
        # a nearest tap can differ from the oracle's only where the coordinate falls within the kernel's error of a pixel edge
        assert float((got != ref).mean()) <= 1e-3, name


# ------------------------------------------------------------------------------------------ 7. bit-equality
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_same_bits_across_calls_batches_layouts_and_index(mode):
    from reni_amd import ops
    H, W = 64, 128
    x = torch.from_numpy(sky_maps(5, H, W, 11)).to(DEV)
    Rs = torch.stack([_t(R) for _, R in rotation_list()[:5]])
    full = ops.rotate_envmap(x, Rs, mode)
    assert full.shape == (5, 3, H, W) and full.dtype == torch.float32
    assert torch.equal(full, ops.rotate_envmap(x, Rs, mode))  # two calls
    for n in (0, 3, 4):  # alone, as a batch of one, through index=
        assert torch.equal(ops.rotate_envmap(x[n], Rs[n], mode), full[n])
        assert torch.equal(ops.rotate_envmap(x[n:n + 1], Rs[n:n + 1], mode)[0], full[n])
        assert torch.equal(ops.rotate_envmap(x[n, 1], Rs[n], mode), full[n, 1])  # [H, W]
    idx = torch.tensor([4, 0, 0, 2], device=DEV)
    via = ops.rotate_envmap(x, Rs[idx], mode, index=idx)
    assert via.shape == (4, 3, H, W) and torch.equal(via, full[idx])
    assert torch.equal(ops.rotate_envmap(x, Rs[[4, 0, 0, 2]], mode, index=[4, 0, 0, 2]), via)
    last = x.permute(0, 2, 3, 1).contiguous()  # channel-last [N, H, W, 3]
    assert torch.equal(ops.rotate_envmap(last, Rs, mode, layout="hwc"), full)
    assert torch.equal(ops.rotate_envmap(last[2], Rs[2], mode), full[2])  # [H, W, 3] -> [3, H, W]
    model_out = last.reshape(5, H * W, 3)  # a model output [B, P, 3] read in place
    assert torch.equal(ops.rotate_envmap(model_out.view(5, H, W, 3), Rs, mode, layout="hwc"), full)
    shared = ops.rotate_envmap(x, Rs[1], mode)  # one [3, 3] for the batch against the same matrix per image
    assert torch.equal(shared, ops.rotate_envmap(x, Rs[1].expand(5, 3, 3), mode))
    assert torch.equal(shared[1], full[1])
    with pytest.raises(ValueError):
        ops.rotate_envmap(x, Rs[:3], mode)
    with pytest.raises(ValueError):
        ops.rotate_envmap(x[..., :W - 1], Rs, mode)  # odd width
    with pytest.raises(ValueError):
        ops.rotate_envmap(x, Rs, "bicubic")


# ------------------------------------------------------------------------------------------ 8. equivariance on the device
def _psnr(a, b):
    return 10.0 * math.log10(float(np.abs(b).max()) ** 2 / max(float(((a - b) ** 2).mean()), 1e-300))


@pytest.mark.parametrize("eq", ["SO2", "SO3"])
def test_turning_the_map_is_turning_the_latent_on_the_device(eq):
    from reni_amd import rotation
    g = load_golden("g10_equivariance.npz")
    spec = O.DecoderSpec(49, eq, 128, 5, 3, True, "tanh")
    plan = make_plan(spec, "f32")
    fp = flat_params(spec, sd_from(g, f"sd_{eq}.")).to(DEV)
    H, W = 64, 128
    Z = torch.from_numpy(g[f"Z_{eq}"]).to(DEV)
    D = O.get_directions(W).to(DEV)
    base = plan.forward(Z, D, fp)  # [1, P, 3]
    base64 = base[0].double().cpu().numpy().reshape(H, W, 3).transpose(2, 0, 1)

    def turned(R):
        out = plan.forward(rotation.rotate_latent(Z, _t(R)), D, fp)
        return out[0].double().cpu().numpy().reshape(H, W, 3).transpose(2, 0, 1)

    def rotated(R):
        out = rotation.rotate_envmap(base.view(1, H, W, 3), _t(R), layout="hwc")  # the model output read in place
        return out[0].double().cpu().numpy()

    for k in (3, -17):  # pixel centres land on pixel centres: the model identity's tolerance plus the kernel's bound
        R = Ry(k * 2 * math.pi / W).astype(np.float32)
        bound, keep = rotate_bound(base64, R)
        err = np.abs(rotated(R) - turned(R))
        print(f"{eq} Ry({k} 2 pi / {W}): max err {err.max():.3e} (2e-5 + bound, bound <= {bound.max():.1e})")
        assert keep.all() and np.all(err <= 2e-5 + bound)
    between = [("Ry(0.7)", g["Ry"])] + ([("R3", g["R3"])] if eq == "SO3" else [])
    for name, R in between:  # between pixels: no worse than the float64 oracle on the same device output, plus the bound
        R = R.astype(np.float32)
        want = turned(R)
        bound, keep = rotate_bound(base64, R)
        e_dev, e_ref = np.abs(rotated(R) - want), np.abs(np_rotate_envmap(base64, R) - want)
        print(f"{eq} {name}: kernel max {e_dev[:, keep].max():.3e} rms {np.sqrt((e_dev ** 2).mean()):.3e} PSNR {_psnr(rotated(R), want):.1f} dB; "
              f"float64 oracle max {e_ref[:, keep].max():.3e} PSNR {_psnr(np_rotate_envmap(base64, R), want):.1f} dB")
        assert np.all((e_dev <= e_ref + bound)[:, keep])
        assert (~keep).sum() * H <= 2 * H * W


# ------------------------------------------------------------------------------------------ 9. ResidentDataset
def test_resident_dataset_rotations(tmp_path):
    from reni_amd import ops, rotation
    from reni_amd.data import ResidentDataset
    _write_exr_dir(tmp_path / "hdr", 6, 64, 128)

    def make(**kw):
        return ResidentDataset(_hdr_dataset(tmp_path / "hdr", (16, 32), (-3.0, 8.0)), levels=1, device=DEV, **kw)

    rd = make()
    idx = [4, 1, 1, 5]
    plain = rd.batch(idx)
    assert torch.equal(plain, rd.level_tensor()[idx])  # rotate=None: today's tensors
    R = rotation.random_rotations(4, "SO3", torch.Generator(device=DEV).manual_seed(1))
    assert R.is_cuda
    got = rd.batch(idx, rotations=R)
    assert got.shape == (4, 3, 16, 32) and torch.equal(got, ops.rotate_envmap(plain, R))
    assert not torch.equal(got, plain)
    assert torch.equal(rd.batch(torch.tensor(idx), rotations=R.cpu()), got)

    a, b, other_rank, other_seed = make(rotate="SO2", rotate_seed=7, rotate_rank=0), make(rotate="SO2", rotate_seed=7, rotate_rank=0), \
        make(rotate="SO2", rotate_seed=7, rotate_rank=1), make(rotate="SO2", rotate_seed=8, rotate_rank=0)
    a1, a2 = a.batch(idx), a.batch(idx)
    assert torch.equal(a1, b.batch(idx)) and torch.equal(a2, b.batch(idx))  # same seed: same batches, call by call
    assert not torch.equal(a1, a2)  # a fresh draw per call
    assert not torch.equal(a1[1], a1[2])  # ... and per image: the same source twice in one batch
    assert not torch.equal(a1, other_rank.batch(idx)) and not torch.equal(a1, other_seed.batch(idx))
    assert not torch.equal(a1, plain) and bool(torch.isfinite(a1).all())
    # a yaw keeps every row's content in its row, and its column weights sum to one around the circle: the row sums agree to
    # W x (the row coordinate's error A_ROW H 2^-24 = 7e-6 pixels x a row difference <= 2) = 5e-4 and the sums' own rounding
    assert torch.allclose(a1.sum(-1), plain.sum(-1), rtol=1e-5, atol=1e-3)
    # explicit rotations win over the configured draw and do not advance its stream
    assert torch.equal(a.batch(idx, rotations=R), got)
    assert torch.equal(a.batch(idx), b.batch(idx))
    # __getitem__ is never rotated
    for i in (0, 4):
        assert torch.equal(a[i][0], rd[i][0]) and torch.equal(a[i][0], a.level_tensor()[i])
    # after double_resolution the rotations apply at the new level
    for d in (rd, a, b):
        d.double_resolution()
    assert rd.size == (32, 64)
    big = rd.batch(idx, rotations=R)
    assert big.shape == (4, 3, 32, 64) and torch.equal(big, ops.rotate_envmap(rd.level_tensor(1)[idx], R))
    a3 = a.batch(idx)
    assert a3.shape == (4, 3, 32, 64) and torch.equal(a3, b.batch(idx)) and not torch.equal(a3, rd.batch(idx))
    so3 = make(rotate="SO3", rotate_seed=7, rotate_rank=0).batch(idx)
    assert not torch.allclose(so3.sum(-1), plain.sum(-1), rtol=1e-5, atol=1e-3)  # a general rotation mixes the rows
    with pytest.raises(ValueError):
        make(rotate="SO4")


# ------------------------------------------------------------------------------------------ 10. the augmented fit
def test_fit_decoder_with_rotation_augmentation(tmp_path, monkeypatch):
    from reni_amd import exr, trainer
    from reni_amd.data import ResidentDataset
    from reni_amd.lightning_module import RENI
    _write_exr_dir(tmp_path / "hdr" / "Train", 4, 32, 64)
    minmax = _hdr_dataset(tmp_path / "hdr" / "Train", (16, 32)).transforms.transforms[1].minmax
    calls = []
    real = exr.read_exr

    def counted(path, *a, **k):
        calls.append(str(path))
        return real(path, *a, **k)

    monkeypatch.setattr(exr, "read_exr", counted)

    def run(augment):
        del calls[:]
        cfg = _fit_cfg(tmp_path / "hdr", minmax, True)
        if augment is not None:
            cfg.DATASET.ROTATE_AUGMENT = augment
        torch.manual_seed(0)
        mod = RENI(cfg, "FIT_DECODER")
        hist = trainer.fit(mod, max_epochs=6, device=DEV)
        assert isinstance(mod.dataset, ResidentDataset) and mod.dataset.rotate == augment
        assert len(calls) == 4 and len(set(calls)) == 4, calls  # one decode per file over six epochs and one doubling
        assert mod.cur_res == [32, 64] and mod.dataset.level == 1
        return [h["loss"] for h in hist]

    plain, so2, so2_again, so3 = run(None), run("SO2"), run("SO2"), run("SO3")
    print("plain", plain, "SO2", so2, "SO3", so3)
    assert all(np.isfinite(so2)) and all(np.isfinite(so3))
    assert so2 == so2_again  # same seed, same history
    assert so2 != plain and so3 != plain and so3 != so2
    cfg = _fit_cfg(tmp_path / "hdr", minmax, False)
    cfg.DATASET.ROTATE_AUGMENT = "SO2"
    with pytest.raises(ValueError, match="RESIDENT"):
        RENI(cfg, "FIT_DECODER").setup_dataset()
