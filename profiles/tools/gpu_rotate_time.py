"""Rotation timings, one JSON line per measurement.

  python profiles/tools/gpu_rotate_time.py write DIR        64 synthetic 256 x 512 half / ZIP EXR files under DIR/Train (8 distinct
        maps, each copied 8 times); the other modes read them
  python profiles/tools/gpu_rotate_time.py kernel           ops.rotate_envmap on one augmented batch, per-image SO(3), bilinear,
        gathered from a level tensor through index= (64 x 3 x 128 x 256 and 100 x 3 x 64 x 128): call time from device events,
        next to index_select alone and to the byte bound (read + write 2 B 3 H W 4 bytes over 6.3 TB/s)
  python profiles/tools/gpu_rotate_time.py trace 0|1        thirty such calls of the first / second shape and nothing else: the body
        for `rocprofv3 --kernel-trace --stats -- python profiles/tools/gpu_rotate_time.py trace 0`
  python profiles/tools/gpu_rotate_time.py fit DIR [AUGMENT] [--root TREE]   device time per epoch of the resident fit of
        gpu_resident_time.py (64 maps at 64 x 128, B = 64, bf16, H = 128, 5 layers, latent 36), 14 epochs, events at every epoch
        end, DATASET.ROTATE_AUGMENT = AUGMENT (SO2 | SO3) or off.  --root: import reni_amd from another checkout (the parent
        commit, built), so that "off" is what users have today."""
import json
import os
import shutil
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TREE = "this"
if "--root" in sys.argv:
    k = sys.argv.index("--root")
    ROOT, TREE = os.path.abspath(sys.argv[k + 1]), "parent"
    del sys.argv[k:k + 2]
sys.path.insert(0, ROOT)

N_FILES, SRC, SIZE, BATCH, EPOCHS = 64, (256, 512), (64, 128), 64, 14
MINMAX = [-4.0, 8.0]
HBM_TB_S = 6.3


def out(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def write_files(d):
    from reni_amd import exr
    os.makedirs(os.path.join(d, "Train"))
    h, w = SRC
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    g = np.random.default_rng(0)
    for i in range(8):
        sky = np.exp(2.0 * np.cos(np.pi * yy / h) + 0.2 * i)[:, :, None] * np.array([0.6, 0.8, 1.0])
        sky = sky * (0.9 + 0.2 * g.random((h, w, 1)))
        sun = 500.0 * np.exp(-((yy - h // 5 - 2 * i) ** 2 + (xx - w // 3 - 10 * i) ** 2) / 20.0)[:, :, None]
        p = os.path.join(d, "Train", f"env{i}.exr")
        exr.write_exr(p, (sky + sun).astype(np.float32), pixel_type="half", compression="zip")
        for k in range(1, N_FILES // 8):
            shutil.copy(p, os.path.join(d, "Train", f"env{i + 8 * k}.exr"))
    out(what="files written", files=N_FILES, size=list(SRC))


def events(fn, warmup=10, iters=100):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def batches():
    from reni_amd.rotation import random_rotations
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    for n_src, B, H, W in ((1694, 64, 128, 256), (1694, 100, 64, 128)):
        level = torch.rand(n_src, 3, H, W, device=dev, generator=g)
        idx = torch.randperm(n_src, device=dev, generator=g)[:B]
        yield level, idx, random_rotations(B, "SO3", g), (B, H, W)


def mode_kernel():
    from reni_amd import ops
    for level, idx, R, (B, H, W) in batches():
        bound_us = 2 * B * 3 * H * W * 4 / (HBM_TB_S * 1e12) * 1e6
        rot = events(lambda: ops.rotate_envmap(level, R, "bilinear", "chw", index=idx))
        near = events(lambda: ops.rotate_envmap(level, R, "nearest", "chw", index=idx))
        sel = events(lambda: level.index_select(0, idx))
        out(what="one augmented batch, per-image SO(3), gathered through index=", shape=[B, 3, H, W],
            rotate_bilinear_call_us=round(rot, 1), rotate_nearest_call_us=round(near, 1), index_select_call_us=round(sel, 1),
            byte_bound_us=round(bound_us, 2))


def mode_trace(which):
    from reni_amd import ops
    level, idx, R, _ = list(batches())[which]
    for _ in range(30):
        ops.rotate_envmap(level, R, "bilinear", "chw", index=idx)
    torch.cuda.synchronize()


def config(path, augment):
    task = types.SimpleNamespace(
        LR_START=1e-4, LR_END=1e-5, OPTIMIZER="adam", OPTIMIZER_BETA_1=0.0, OPTIMIZER_BETA_2=0.9, SCHEDULER_TYPE="none",
        SCHEDULER_STEP_SIZE=1, SCHEDULER_GAMMA=1.0, BATCH_SIZE=BATCH, EPOCHS=EPOCHS + 1, MULTI_RES_TRAINING=False,
        INITAL_RESOLUTION=list(SIZE), FINAL_RESOLUTION=list(SIZE), CURRICULUM=[1], KLD_WEIGHTING=1e-4,
        COSINE_SIMILARITY_WEIGHT=1e-1, PRIOR_LOSS_WEIGHT=1e-7, APPLY_MASK=False, MASK_PATH="")
    reni = types.SimpleNamespace(
        CONDITIONING="Cond-by-Concat", MODEL_TYPE="AutoDecoder", EQUIVARIANCE="SO2", LATENT_DIMENSION=36, HIDDEN_LAYERS=5,
        HIDDEN_FEATURES=128, OUT_FEATURES=3, LAST_LAYER_LINEAR=True, OUTPUT_ACTIVATION="tanh", FIRST_OMEGA_0=30.0,
        HIDDEN_OMEGA_0=30.0, MAPPING_LAYERS=3, MAPPING_FEATURES=128, COMPUTE_DTYPE="bf16", FIT_DECODER=task)
    ds = types.SimpleNamespace(NAME="RENI_HDR", RESIDENT=True, RENI_HDR=types.SimpleNamespace(
        PATH=path, TRANSFORMS=[["minmaxnormalise", MINMAX]], IS_HDR=True))
    if augment:
        ds.ROTATE_AUGMENT = augment
    return types.SimpleNamespace(RENI=reni, DATASET=ds, TRAINER=types.SimpleNamespace(LOGGER=types.SimpleNamespace(NUMBER_OF_IMAGES=2)))


def mode_fit(path, augment):
    from reni_amd import trainer
    from reni_amd.lightning_module import RENI
    torch.manual_seed(0)
    mod = RENI(config(path, augment), "FIT_DECODER")
    marks = [torch.cuda.Event(enable_timing=True)]
    end = mod.training_epoch_end

    def timed_end(outs):
        end(outs)
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)

    mod.training_epoch_end = timed_end
    marks[0].record()
    hist = trainer.fit(mod, max_epochs=EPOCHS)
    torch.cuda.synchronize()
    ms = [round(a.elapsed_time(b), 3) for a, b in zip(marks[:-1], marks[1:])]
    later = ms[4:]
    out(what="resident fit, device ms per epoch of 64 maps", tree=TREE, augment=augment or "off",
        has_rotation=hasattr(mod.dataset, "rotate"), epoch_ms=ms, epochs_5_on_median=round(float(np.median(later)), 3),
        epochs_5_on_min=min(later), epochs_5_on_max=max(later), last_loss=hist[-1]["loss"])


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "write":
        return write_files(sys.argv[2])
    if mode == "kernel":
        return mode_kernel()
    if mode == "trace":
        return mode_trace(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    if mode == "fit":
        return mode_fit(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    raise SystemExit(f"unknown mode {mode!r}")


if __name__ == "__main__":
    main()
