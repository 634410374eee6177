"""Resident-dataset timings, one JSON line per measurement.

  python profiles/tools/gpu_resident_time.py fit [rounds]   wall time per epoch of trainer.fit, DATASET.RESIDENT against the
        host path, alternating the two on the same box: 64 synthetic 1024 x 2048 half / ZIP EXR files at 64 x 128, B = 64, bf16
        training (H = 128, 5 layers, latent 36), 4 epochs per fit, device-synchronised host clocks at every epoch end
  python profiles/tools/gpu_resident_time.py build          the cache build of those 64 files split into decode (host),
        upload (host to device) and kernels (resample + normalise, CUDA events); then batch(idx) at B = 64
  python profiles/tools/gpu_resident_time.py resize         ops.resample 4096 x 2048 -> 1000 x 500 bicubic and 32 x 16 -> 600 x 300
        Lanczos (kernel alone, CUDA events) and baselines.resizeImage around them (with the copies), and k_resample's time
        against its output size (what bounds it)
  python profiles/tools/gpu_resident_time.py kernels        a few cache builds and resizes and nothing else: the body for
        `rocprofv3 --kernel-trace --stats -- python profiles/tools/gpu_resident_time.py kernels`

The files are written to a temporary directory (8 distinct maps, each copied 8 times: decoding costs the same)."""
import json
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import baselines, exr, ops, trainer  # noqa: E402
from reni_amd.custom_transforms import transform_builder  # noqa: E402
from reni_amd.data import RENIDatasetHDR, ResidentDataset  # noqa: E402
from reni_amd.lightning_module import RENI  # noqa: E402

N_FILES, SRC, SIZE, BATCH, EPOCHS = 64, (1024, 2048), (64, 128), 64, 4
MINMAX = [-4.0, 8.0]


def out(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def write_files(d):
    os.makedirs(os.path.join(d, "Train"))
    h, w = SRC
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    g = np.random.default_rng(0)
    t0 = time.perf_counter()
    for i in range(8):
        sky = np.exp(2.0 * np.cos(np.pi * yy / h) + 0.2 * i)[:, :, None] * np.array([0.6, 0.8, 1.0])
        sky = sky * (0.9 + 0.2 * g.random((h, w, 1)))
        sun = 500.0 * np.exp(-((yy - h // 5 - 9 * i) ** 2 + (xx - w // 3 - 40 * i) ** 2) / 300.0)[:, :, None]
        p = os.path.join(d, "Train", f"env{i}.exr")
        exr.write_exr(p, (sky + sun).astype(np.float32), pixel_type="half", compression="zip")
        for k in range(1, N_FILES // 8):
            shutil.copy(p, os.path.join(d, "Train", f"env{i + 8 * k}.exr"))
    out(what="files written", files=N_FILES, seconds=round(time.perf_counter() - t0, 2),
        mb_per_file=round(os.path.getsize(p) / 1e6, 2))


def config(path, resident):
    task = types.SimpleNamespace(
        LR_START=1e-4, LR_END=1e-5, OPTIMIZER="adam", OPTIMIZER_BETA_1=0.0, OPTIMIZER_BETA_2=0.9, SCHEDULER_TYPE="none",
        SCHEDULER_STEP_SIZE=1, SCHEDULER_GAMMA=1.0, BATCH_SIZE=BATCH, EPOCHS=EPOCHS + 1, MULTI_RES_TRAINING=False,
        INITAL_RESOLUTION=list(SIZE), FINAL_RESOLUTION=list(SIZE), CURRICULUM=[1], KLD_WEIGHTING=1e-4,
        COSINE_SIMILARITY_WEIGHT=1e-1, PRIOR_LOSS_WEIGHT=1e-7, APPLY_MASK=False, MASK_PATH="")
    reni = types.SimpleNamespace(
        CONDITIONING="Cond-by-Concat", MODEL_TYPE="AutoDecoder", EQUIVARIANCE="SO2", LATENT_DIMENSION=36, HIDDEN_LAYERS=5,
        HIDDEN_FEATURES=128, OUT_FEATURES=3, LAST_LAYER_LINEAR=True, OUTPUT_ACTIVATION="tanh", FIRST_OMEGA_0=30.0,
        HIDDEN_OMEGA_0=30.0, MAPPING_LAYERS=3, MAPPING_FEATURES=128, COMPUTE_DTYPE="bf16", FIT_DECODER=task)
    ds = types.SimpleNamespace(NAME="RENI_HDR", RESIDENT=resident, RENI_HDR=types.SimpleNamespace(
        PATH=path, TRANSFORMS=[["minmaxnormalise", MINMAX]], IS_HDR=True))
    return types.SimpleNamespace(RENI=reni, DATASET=ds, TRAINER=types.SimpleNamespace(LOGGER=types.SimpleNamespace(NUMBER_OF_IMAGES=2)))


def one_fit(path, resident):
    torch.manual_seed(0)
    mod = RENI(config(path, resident), "FIT_DECODER")
    marks = []
    end = mod.training_epoch_end

    def timed_end(outs):
        end(outs)
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    mod.training_epoch_end = timed_end
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = trainer.fit(mod, max_epochs=EPOCHS)
    ts = [t0] + marks
    return [round(b - a, 4) for a, b in zip(ts[:-1], ts[1:])], hist[-1]["loss"]


def mode_fit(path, rounds):
    for r in range(rounds):
        for resident in (True, False):
            ep, loss = one_fit(path, resident)
            out(what="fit", round=r, variant="resident" if resident else "host", epoch_seconds=ep,
                later_epochs_mean=round(float(np.mean(ep[1:])), 4), last_loss=loss)


def dataset(path):
    return RENIDatasetHDR(os.path.join(path, "Train"), transform_builder([["resize", list(SIZE)], ["minmaxnormalise", MINMAX]]))


def mode_build(path):
    ds = dataset(path)
    dev = torch.device("cuda", torch.cuda.current_device())
    # the three stages by hand, one file after the other (what ResidentDataset._build does)
    rd = ResidentDataset(ds, levels=3, device=dev, workers=1)
    rd.fill([0])  # tables, library load
    torch.cuda.synchronize()
    dec = up = 0.0
    ev = []
    for i in range(1, 17):
        t0 = time.perf_counter()
        img = rd._source(i)
        t1 = time.perf_counter()
        src = img.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for j, (h, w) in enumerate(rd.sizes):
            rd._store[j][i].copy_(rd._finish(ops.resample(src[None], (h, w), "bilinear"))[0])
        b.record()
        ev.append((a, b))
        dec += t1 - t0
        up += t2 - t1
    torch.cuda.synchronize()
    out(what="cache build per file, 4 levels 64x128..512x1024 from 1024x2048", files=16, decode_ms=round(dec / 16 * 1e3, 2),
        upload_ms=round(up / 16 * 1e3, 3), kernels_ms=round(sum(a.elapsed_time(b) for a, b in ev) / 16, 3))
    for workers in (1, 8, 16):
        rd = ResidentDataset(ds, levels=0, device=dev, workers=workers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd.fill()
        torch.cuda.synchronize()
        out(what="fill 64 files, one level", workers=workers, seconds=round(time.perf_counter() - t0, 3))
    idx = list(range(BATCH))
    for _ in range(10):
        rd.batch(idx)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        x = rd.batch(idx)
    torch.cuda.synchronize()
    out(what="batch(idx), B = 64 at 64x128, all cached", us_per_call=round((time.perf_counter() - t0) / 200 * 1e6, 1),
        shape=list(x.shape))


def events(fn, warmup=5, iters=30):
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


def mode_resize():
    g = np.random.default_rng(1)
    dev = torch.device("cuda")
    for (hs, ws), (hd, wd), interp, mode in (((2048, 4096), (500, 1000), baselines.INTER_CUBIC, "bicubic"),
                                             ((16, 32), (300, 600), baselines.INTER_LANCZOS4, "lanczos4")):
        img = (g.random((hs, ws, 3)) + 0.1).astype(np.float32)
        t = torch.from_numpy(img).to(dev)
        us = events(lambda: ops.resample(t, (hd, wd), mode, layout="hwc"))
        t0 = time.perf_counter()
        for _ in range(5):
            baselines.resizeImage(img, wd, hd, interp)
        wall = (time.perf_counter() - t0) / 5
        taps = 16 if mode == "bicubic" else 64
        out(what=f"resize {ws}x{hs} -> {wd}x{hd} {mode}", kernel_call_us=round(us, 1), resizeImage_ms=round(wall * 1e3, 2),
            source_mb=round(img.nbytes / 1e6, 1), gathered_gb_per_s=round(hd * wd * 3 * taps * 4 / us / 1e3, 1))
    # what bounds k_resample: bilinear from one 1024 x 2048 planar source to growing outputs, call time against output pixels
    src = torch.from_numpy((g.random((1, 3, 1024, 2048)) + 0.1).astype(np.float32)).to(dev)
    for hd, wd in ((16, 32), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 2048), (2048, 4096)):
        us = events(lambda: ops.resample(src, (hd, wd), "bilinear"))
        out(what="k_resample bilinear 1024x2048 ->", size=[hd, wd], call_us=round(us, 1),
            out_gb_per_s=round(3 * hd * wd * 4 / us / 1e3, 2))
    empty = events(lambda: torch.empty(1, 3, 64, 128, device=dev))
    out(what="torch.empty alone (the allocator's share of a call)", us=round(empty, 1))


def mode_kernels(path):
    ds = dataset(path)
    rd = ResidentDataset(ds, levels=3, device=torch.device("cuda", torch.cuda.current_device()), workers=8)
    rd.fill(range(16))
    img = torch.rand(2048, 4096, 3, device="cuda") + 0.1
    for _ in range(5):
        ops.resample(img, (500, 1000), "bicubic", layout="hwc")
        ops.resample(img[:16, :32], (300, 600), "lanczos4", layout="hwc")
        ops.gaussian_blur(img[:300, :600].contiguous(), 5.0, layout="hwc")
    torch.cuda.synchronize()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "fit"
    if mode == "resize":
        return mode_resize()
    d = tempfile.mkdtemp(prefix="reni_resident_")
    try:
        write_files(d)
        if mode == "fit":
            mode_fit(d, int(sys.argv[2]) if len(sys.argv) > 2 else 2)
        elif mode == "build":
            mode_build(d)
        elif mode == "kernels":
            mode_kernels(d)
        else:
            raise SystemExit(f"unknown mode {mode!r}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
