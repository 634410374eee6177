#!/usr/bin/env python
"""bench.py -- BASELINE.json's headline metric on the fused HIP path.

    python bench.py --gpus N --steps K --warmup W [--config c2|c4|c5|film|c2_curric|c2_h256] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run measures the headline alone: set-up, W warm-up steps, K timed steps, the line.  --full adds everything else the
benchmark measures (the sub-records, `sustained`, `cpu_baseline`; see Headline below).  --dump-outputs DIR writes what the last
timed step computed (the step's return value and the state it updates) as DIR/<name>.npy; the inputs are seeded, so two builds
run with the same arguments can be compared array for array.

Metric  : directional samples / second (one sample = one (image, direction) pair through encoding -> SIREN ->
          loss -> gradients).
Workload: --config c2 (default, the configuration BASELINE.json's metric is quoted on): a 615-image training set,
          128x256 equirect (P = 32768), ND = 36, 5x128 SIREN, SO2, tanh, AutoDecoder, RENITrainLoss, bf16 MFMA;
          per-GPU batch = 64 images (the largest power of two that 8 ranks can each draw from their 76-77 owned images);
          one step = fused forward+loss+backward (decoder and latent gradients) -> [N > 1: ONE RCCL all-reduce of the
          flat decoder gradient] -> Adam on decoder + latents.
          --config c4 (BASELINE config 4): test-time latent optimisation -- 21 held-out maps, frozen decoder, masked
          RENITestLoss(1e-7, 1e-4) with the cosine term, per-image latent Adam (lr 0.1); one step = statistics pass +
          latent forward/backward + Adam on the latent rows.  No collective (every rank: its own 21 maps).
          --config film: config 2's training step with the reference's DEFAULT conditioning (configs/default.py:9: FiLM,
                         5 FiLM layers x 128, mapping network 3 x 128) -- not a BASELINE config, reported beside it.
          --config c5 (BASELINE config 5): fp32 inference at 512x1024 directions, ND = 49, 4 images per step (SO2; the record also
                         carries the SO3 model of SURVEY 8(d) C5 as `so3`).
          --config c2_curric: config 2's step in the reference's REAL schedule (configs/experiment.yaml:29-34, callbacks.py:11-29):
                         B = 100 at 16x32, 32x64 and 64x128 (the headline: 64x128; --full: one record per resolution) -- a step
                         there is its dependent launches.
          --config c2_h256: config 2's step at the width the reference's shipped configs use (configs/default.py:13: 5 x 256).
          Synthetic images / random-init weights (seed 42).
Scaling : weak (per-GPU batch fixed; images and their latent rows sharded round-robin over ranks).
Launch  : with WORLD_SIZE / RANK in the environment (torchrun) this process is one rank.  Without them and --gpus N > 1
          it spawns N rank processes itself -- BEFORE anything touches the GPU -- and returns the worst exit code.

Headline: `value` / `ms_per_step` / `roofline` are ONE measurement -- W warm-up steps, barrier, exactly K timed steps, barrier --
          taken FIRST, right behind the set-up, identically with and without --full and the sub-records (`--no-also`).  A GPU that
          has been idle needs ~30 ms of load to reach its sustained clocks, so with a short warm-up that window
          reads ~4 % below what a training run sees; with --full the same W + K steps measured again behind the sub-records are
          reported beside it as `sustained` (a side field, never `value`).
Rank 0 prints ONE JSON line including `roofline` (dominant kernel, timed live with HIP events on its own stream) and, with --full
at N = 1, `cpu_baseline` (the CPU oracle timed on the host's cores on a bounded sample: B = 1 and B = 4 images, 3 warm-up +
10 timed steps each, reference-shaped and factored -- SURVEY.md 8d).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# algorithmic work per sample, factored form (SURVEY.md 8d / BASELINE.md section 4)
FLOP_TRAIN, FLOP_FROZEN, FLOP_FWD_ND49 = 522784, 348448, 177860
# --config film: SURVEY 8(d)'s formulas with L = 4 hidden FiLM layers behind the folded first one (ND = 36, H = 128):
# F = (ND+2) H + 2 ND + L H^2 + 3 H = 70 856 MAC, Bt = 2 (L H^2 + 3 H) + (ND+2) H + ND H + 2 ND = 141 384 MAC; 2 FLOP / MAC
FLOP_FILM = 2 * (70856 + 141384)
PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}   # dense MFMA peaks, MI355X_MICROARCH.md
PMC_TRAFFIC = os.path.join(ROOT, "profiles", "pmc_traffic.json")  # {"<kernel>": {"hbm_bytes_per_launch": .., "src_sha256": ..}}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=["c2", "c4", "c5", "film", "c2_curric", "c2_h256"])
    ap.add_argument("--batch", type=int, default=None,
                    help="images per GPU per step (c2: 64, <= 615/8 so that 8 ranks can own them; c4: 21; c5: 4)")
    ap.add_argument("--dtype", default=None, choices=["bf16", "f32"], help="c2 / c4: bf16, c5: f32")
    ap.add_argument("--res", default=None, help="c2 only: HxW of the equirect grid (e.g. 16x32: one stage of the curriculum on its own)")
    ap.add_argument("--hidden", type=int, default=128, choices=[128, 256],
                    help="c4 / c5: the SIREN's width (256: the reference's shipped width -- the sub-records c4_h256 / fwd_h256 on their own, "
                         "for the counter passes of profiles/tools/gpu_profile_round.sh; c5 then runs in bf16)")
    ap.add_argument("--dense", action="store_true", help="c4: RENI_WEIGHT_SPARSE off (every tile, and the statistics pass)")
    ap.add_argument("--pixels", action="store_true", help="c4: RENI_WEIGHT_COMPACT (pixels with weight packed into each image's first tiles)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the sub-records (`also`), the `sustained` re-run and the CPU "
                         "baseline; a plain run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float32, "
                         "at most 64 MB in all: a fixed, seeded sample of a larger array)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--no-also", action="store_true", help="--full: skip the sub-records of the c2 line")
    ap.add_argument("--no-fused-step", action="store_true",
                    help="the training step as two library calls (fwd+loss+bwd, then Adam) instead of reni_train_step_rows")
    ap.add_argument("--comm", default=None, choices=["torch", "capi"],
                    help="the step's exchange (decoder-gradient all-reduce).  capi: an RCCL communicator the library owns -- the step is "
                         "then reni_train_step_rows_dp, the SAME fused call N = 1 runs with the all-reduce inside it (the default at "
                         "N > 1 on the nccl backend; if the communicator cannot be created the line says so in `comm_fallback`).  "
                         "torch: torch.distributed's collective between forward_loss_backward_rows and adam_step2 (three calls; the "
                         "opt-out, and what a gloo job gets).  N = 1 default: no communicator at all")
    return ap.parse_args()


EXIT_RENDEZVOUS = 75  # a rank that could not join the process group (main() exits with it): the one failure spawn_ranks retries


def spawn_ranks(n):
    """python bench.py --gpus N without a launcher: start N rank processes (children of this one, which has not
    touched the GPU and never will) with the environment torchrun would give them; rank 0's stdout is ours.
    The children are polled: the first one to fail takes its siblings down with it (they would otherwise sit in
    init_process_group / the all-reduce until the process-group timeout).  ONLY a failed rendezvous (EXIT_RENDEZVOUS: the port,
    picked by bind-and-close, was taken by a concurrent run) is retried, once, on a fresh port -- any other failure is
    deterministic and running it twice would at best print a second line."""
    def launch():
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
        return procs

    rc = 0
    for attempt in range(2):
        procs = launch()
        rc = 0
        while True:
            codes = [p.poll() for p in procs]
            bad = [c for c in codes if c not in (None, 0)]
            if bad:
                rc = EXIT_RENDEZVOUS if EXIT_RENDEZVOUS in bad else bad[0]
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                for p in procs:
                    try:
                        p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        p.wait()
                break
            if all(c == 0 for c in codes):
                return 0
            time.sleep(0.2)
        if not (attempt == 0 and rc == EXIT_RENDEZVOUS):
            return rc
    return rc


def _median_step_s(fn, warm, n):
    ts = []
    for i in range(warm + n):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def cpu_baseline(n_steps):
    """the CPU oracle on the config-2 shape, fp32, all host threads, B = 1 and B = 4 images per step,
    3 warm-up + n_steps timed forward+loss+backward steps each (median), in two forms: "port" = reference-shaped
    (materialised 1370-column encoding, linear + sin, autograd: the op sequence of src/models/RENI.py:31-53,86-87) and
    "factored" (the algebra the kernels implement, per-image constants folded into an affine map).  `value` is the
    reference-shaped figure at the better of the two batch sizes."""
    import torch
    from oracle import reni_oracle as O
    spec = O.DecoderSpec(36, "SO2", 128, 5, 3, True, "tanh")
    g = torch.Generator().manual_seed(42)
    params = O.init_params(spec, g)
    D = O.get_directions(256); S = O.get_sineweight(256)
    P = D.shape[1]
    res = {}
    for B in (1, 4):
        Z = torch.randn(B, 36, 3, generator=g)
        T = O.synthetic_images(list(range(B)), 128, 256).permute(0, 2, 3, 1).reshape(B, -1, 3)
        Db, Sb = D.expand(B, -1, 3), S.expand(B, -1, 3)
        res[f"port_b{B}"] = B * P / _median_step_s(lambda: O.fwd_loss_bwd(spec, params, Z, Db, T, Sb), 3, n_steps)
        res[f"factored_b{B}"] = B * P / _median_step_s(lambda: O.factored_torch_fwd_loss_bwd(spec, params, Z, D, T, Sb), 3, n_steps)
    return {"value": max(res["port_b1"], res["port_b4"]), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "port_b1": res["port_b1"], "port_b4": res["port_b4"],
            "factored": max(res["factored_b1"], res["factored_b4"]), "factored_b1": res["factored_b1"], "factored_b4": res["factored_b4"],
            "sample": f"config-2 shape (128x256, ND=36, 5x128, fp32), B=1 and B=4 images/step, 3 warm-up + {n_steps} timed fwd+loss+bwd "
                      f"steps each, median; port = reference-shaped (1370-column encoding + autograd), factored = per-image affine first layer"}


def kernel_src_sha():
    """sha256 over the kernel sources (reni_amd/csrc/*.inc, *.h, *.hip in name order): profiles/pmc_traffic.json carries it."""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "reni_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.inc")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.hip"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def pmc_record(kernel):
    """Counters of one kernel from the PMC passes (profiles/tools/gpu_profile_round.sh -> profiles/pmc_traffic.json): HBM-side
    bytes per launch and, for the training kernel, the instruction mix.  Valid only for the kernel sources they were measured
    on: the file carries kernel_src_sha(), and a stale entry reads as nothing (`traffic: null`)."""
    try:
        rec = json.load(open(PMC_TRAFFIC)).get(kernel)
        if rec and rec.get("src_sha256") == kernel_src_sha():
            return rec
    except Exception:  # noqa: BLE001
        pass
    return {}


def issue_ceiling(valu_per_mfma, trans_per_mfma):
    """Fraction of the MFMA peak a lone wave per SIMD can reach when it must also issue `valu_per_mfma` VALU instructions
    (`trans_per_mfma` of them transcendental) per MFMA: slot costs measured on this kernel's exact MFMA form
    (profiles/r02_mfma_shadow.md: 33.6 cycles per 32x32x16 bf16 MFMA, of which ~13.3 block the issue port; 4.4 cycles a plain
    VALU, 8.8 a transcendental)."""
    issue = 13.3 + 4.4 * (valu_per_mfma - trans_per_mfma) + 8.8 * trans_per_mfma
    return 33.6 / max(33.6, issue)


def flop_train(nd, H, L):
    """SURVEY.md 8(d)'s per-sample work of one fwd+bwd training step, factored form (2 FLOP per MAC): forward
    F = (ND+2) H + 2 ND + L H^2 + 3 H, backward Bt = 2 (L H^2 + 3 H) + (ND+2) H + ND H + 2 ND.  (ND=36, H=128, L=5: 522 784.)"""
    F = (nd + 2) * H + 2 * nd + L * H * H + 3 * H
    Bt = 2 * (L * H * H + 3 * H) + (nd + 2) * H + nd * H + 2 * nd
    return 2 * (F + Bt)


def flop_film(nd, H, L):
    """--config film: SURVEY 8(d)'s formulas with L hidden FiLM layers behind the folded first one: F = (ND+2) H + 2 ND + L H^2 + 3 H,
    Bt = 2 (L H^2 + 3 H) + (ND+2) H + ND H + 2 ND; 2 FLOP / MAC.  (ND=36, H=128, L=4: 424 480.)"""
    F = (nd + 2) * H + 2 * nd + L * H * H + 3 * H
    Bt = 2 * (L * H * H + 3 * H) + (nd + 2) * H + nd * H + 2 * nd
    return 2 * (F + Bt)


def flop_fwd(nd, H, L):
    """forward only: 2 x ((ND+2) H + 2 ND + L H^2 + 3 H)  (ND=49, H=128, L=5: 177 860)"""
    return 2 * ((nd + 2) * H + 2 * nd + L * H * H + 3 * H)


def flop_frozen(nd, H, L):
    """forward + the backward pass of a frozen decoder (dX GEMMs, the first layer's ND H + 2 ND): ND=36, H=128, L=5: 348 448"""
    return flop_fwd(nd, H, L) + 2 * (L * H * H + 3 * H + nd * H + 2 * nd)


_IMG_CACHE = {}
_COMM = {}   # the library-owned RCCL communicator of this process (one per process: every configuration of a run shares it)


def _want_capi(args, world):
    """--comm capi, or no --comm at N > 1: the fused data-parallel step on the library's own communicator (whatever backend the torch
    group runs on -- the group only carries the 128-byte unique id and the barriers)."""
    if args.comm is not None:
        return args.comm == "capi"
    return world > 1


def _rccl_comm(args, rank, world, dev):
    """The communicator, created once.  A failure here is collective (ncclCommInitRank fails or hangs on every rank alike), and every
    rank must take the same branch: the ranks agree through the torch group, and on a fallback the line carries `comm_fallback`."""
    import torch
    from reni_amd import dist as rdist
    if "comm" not in _COMM:
        comm, err = None, None
        try:
            comm = rdist.RcclComm(rank, world)
            # one small all-reduce through it, checked against the sum every rank can compute: a communicator that comes up but does
            # not reduce (or a library that is not the one torch talks to) must not reach the timed steps
            probe = torch.full((1024,), float(rank + 1), device=dev)
            comm.allreduce_(probe, 1.0)
            torch.cuda.synchronize(dev)
            want = world * (world + 1) / 2.0
            if not bool((probe == want).all()):
                raise RuntimeError(f"probe all-reduce gave {float(probe[0])}, expected {want}")
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"[:200]
            if comm is not None:
                try:
                    comm.close()
                except Exception:  # noqa: BLE001
                    pass
                comm = None
        if world > 1:
            ok = torch.tensor([0 if comm is None else 1], device=dev)
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
            if int(ok) == 0 and comm is not None:
                comm.close()
                comm, err = None, "another rank could not create the communicator"
        if comm is None and args.comm == "capi":
            raise RuntimeError(f"--comm capi: {err}")
        _COMM["comm"], _COMM["error"] = comm, err
        if comm is None:
            print(f"bench.py: the library's RCCL communicator could not be created ({err}); falling back to torch.distributed's "
                  "all-reduce between forward_loss_backward_rows and adam_step2", file=sys.stderr, flush=True)
    return _COMM["comm"]


def _resident_images(n_images, h, w, owned, dev):
    """This rank's shard of the synthetic set, resident in HBM (shared by the configurations of one process that use the same set)."""
    import torch
    from reni_amd.data import SyntheticEnvMapDataset
    key = (n_images, h, w, len(owned), owned[0] if owned else -1, str(dev))
    if key not in _IMG_CACHE:
        ds = SyntheticEnvMapDataset(n_images, h, w)
        _IMG_CACHE[key] = torch.stack([ds.make(i) for i in owned]).to(dev)      # [n_local,3,H,W]
    return _IMG_CACHE[key]


def mask3(sidelen):
    """The reference's data/Masks/Mask-3.png (examples.ipynb cell 4) at this resolution: its 256 x 512 source travels as plain
    data in tests/golden/g7_latent_opt.npz (`mask_src`); resized exactly as utils.get_mask does (utils.py:81-91)."""
    import numpy as np
    from reni_amd.utils import mask_from_array
    src = np.load(os.path.join(ROOT, "tests", "golden", "g7_latent_opt.npz"))["mask_src"]
    return mask_from_array(sidelen, src)


def run_config(cfg, args, rank, world, dev, batch=None, steps=None, warmup=None, defer=False, res=None, hidden=128, eq="SO2", dense=False,
               pixels=False, force_dtype=None):
    """One bench configuration in this process: build the model / engine, warm up, time `steps` steps between barriers.
    Returns the record (value, ms_per_step, roofline ...) on every rank; timing is the MAX over ranks.
    res = (height, width) of the c2 step's images (the multi-resolution curriculum), hidden = the SIREN's width."""
    import torch
    from reni_amd import dist as rdist
    from reni_amd import ops
    from reni_amd.engine import TrainEngine
    from reni_amd.models import RENIAutoDecoder
    from reni_amd.utils import get_directions, get_sineweight

    torch.cuda.empty_cache()  # (what the previous configuration of this process left in the caching allocator)
    steps = steps or args.steps
    warmup = args.warmup if warmup is None else warmup
    dtype = force_dtype or args.dtype or ("f32" if cfg == "c5" else "bf16")
    torch.manual_seed(42)
    if cfg == "c2":
        N_IMAGES, (H_IMG, W_IMG), ND, B = 615, res or (128, 256), 36, batch or 64
        owned = rdist.owned_indices(N_IMAGES, rank, world)
        model = RENIAutoDecoder(N_IMAGES, ND, "SO2", hidden, 5, 3, True, "tanh", 30.0, 30.0, False)
    elif cfg == "film":
        from reni_amd.film import RENIAutoDecoderFiLM
        N_IMAGES, H_IMG, W_IMG, ND, B = 615, 128, 256, 36, batch or 64
        owned = rdist.owned_indices(N_IMAGES, rank, world)
        model = RENIAutoDecoderFiLM(N_IMAGES, ND, "SO2", hidden, 5, hidden, 3, 3, "tanh", False)   # (hidden = 256: the reference's default model, configs/default.py:9-13)
    elif cfg == "c4":
        N_IMAGES, H_IMG, W_IMG, ND, B = 21, 128, 256, 36, batch or 21
        owned = list(range(N_IMAGES))  # every rank optimises its own 21 held-out maps (no shared state, no collective)
        model = RENIAutoDecoder(N_IMAGES, ND, "SO2", hidden, 5, 3, True, "tanh", 30.0, 30.0, True)
        with torch.no_grad():
            model.Z.normal_()  # (fixed_decoder starts the latents at zero; any start costs the same)
    else:
        N_IMAGES, H_IMG, W_IMG, ND, B = 4, 512, 1024, 49, batch or 4
        owned = list(range(N_IMAGES))
        model = RENIAutoDecoder(N_IMAGES, ND, eq, hidden, 5, 3, True, "tanh", 30.0, 30.0, True)
        with torch.no_grad():
            model.Z.normal_()
    model.set_compute_dtype(dtype)
    with torch.no_grad():  # this rank keeps only the latent rows of the images it owns
        model.Z = torch.nn.Parameter(model.Z[owned].clone(), requires_grad=model.Z.requires_grad)
    model.to(dev)
    if world > 1:
        rdist.broadcast_(model._all_flat() if cfg == "film" else model._flat_params(), 0)
    n_local = len(owned)
    assert n_local >= B, f"per-GPU batch {B} exceeds the {n_local} images this rank owns"
    directions = get_directions(W_IMG).to(dev)
    sineweight = get_sineweight(W_IMG).to(dev)
    P = directions.shape[1]
    idx_all = torch.arange(n_local, device=dev)  # (the loader's indices: resident like the images)
    eng = None

    if cfg in ("c2", "c4", "film"):
        imgs = _resident_images(N_IMAGES, H_IMG, W_IMG, owned, dev)  # resident in HBM before the timed region; ~0.39 MB per image
        comm = None
        if _want_capi(args, world) and cfg in ("c2", "film"):  # the exchange step inside the library (reni_train_step_rows_dp / reni_allreduce_grads)
            comm = _rccl_comm(args, rank, world, dev)
        if cfg in ("c2", "film"):
            eng = TrainEngine(model, lr=1e-5, comm=comm, fused_step=not args.no_fused_step)
            weight = sineweight
        else:
            # the notebook's inpainting mask (examples.ipynb cell 4: data/Masks/Mask-3.png, rows 20-93 x columns 81-164 of 128 x 256
            # kept = 18.8 % of the pixels), multiplied into the sine weight (RENI_module.py:92-94)
            weight = sineweight * mask3(W_IMG).to(dev)
            # sparse_weight: what RENI.training_step passes whenever a mask is configured (lightning_module.py) -- RENI_WEIGHT_SPARSE:
            # tiles whose 128 pixels all have zero weight, and the statistics pass of images whose pixel-0 weight is zero, cannot
            # change the result and are left out (on the device, from the weight, every call).  dense=True: the flag off.
            # pixels=True: RENI_WEIGHT_COMPACT -- the pixels with weight are also packed into each image's first tiles (equal to rounding)
            eng = TrainEngine(model, lr=1e-1, loss_kind="test", alpha=1e-7, beta=1e-4, sparse_weight=("pixels" if pixels else not dense))
            wz = (weight.reshape(-1, 3) != 0).any(1)                                  # (host-side bookkeeping for the record only)
            cos_live = bool(wz[0])
            tiles = torch.nn.functional.pad(wz, (0, (-wz.numel()) % 128)).view(-1, 128).any(1)
            n_live = int(wz.sum())
            sparsity = {"flag": "RENI_WEIGHT_COMPACT" if pixels else "RENI_WEIGHT_SPARSE" if not dense else "off",
                        "pixels_with_weight": float(wz.float().mean()), "tiles_with_weight": float(tiles.float().mean()),
                        "cosine_term_live": cos_live,
                        "tiles_visited": 1.0 if (dense or cos_live) else (((n_live + 127) // 128) / tiles.numel() if pixels
                                                                           else float(tiles.float().mean())),
                        "statistics_pass": "run" if (dense or cos_live) else "skipped on the device (pixel-0 weight is zero: the term is a constant)"}

        def step(s):
            """B consecutive owned images; targets are the reference's permute+view of [B,3,H,W]
            (RENI_module.py:83-84): a channel-planar strided view, never copied."""
            start = (s * B) % (n_local - B + 1)
            nstart = ((s + 1) * B) % (n_local - B + 1)   # (the loader is one batch ahead: the fused step stages that batch's prologue)
            return eng.step(idx_all[start:start + B], imgs[start:start + B].permute(0, 2, 3, 1).view(B, P, 3), weight, directions,
                            next_idx=idx_all[nstart:nstart + B])
    else:
        def step(s):
            with torch.no_grad():
                return model(idx_all[:B], directions)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    shape = {"cfg": cfg, "B": B, "P": P, "ND": ND, "hidden": hidden, "res": (H_IMG, W_IMG), "eq": eq,
             "sparsity": sparsity if cfg == "c4" else None}
    try:
        paths = model._plan().path_info(B, P, need_dw=cfg in ("c2", "film"))
    except Exception as e:  # noqa: BLE001  (diagnostics only)
        paths = {"error": str(e)[:100]}

    final = {}

    def measure():
        rec, final["last"] = _measure(shape, args, world, dev, dtype, step, barrier, steps, warmup, eng, paths)
        return rec

    def outputs():
        """What a caller of the timed path holds after the last measured step: the step's return value and, for the optimising
        configurations, the state the step updates in place (parameters, latent rows, Adam moments)."""
        last = final["last"]
        if eng is None:   # c5: the forward pass's images
            return {"output": last}
        out = {"loss_terms": last, "latents": eng.latent.data, "adam_m_latents": eng.m_lat, "adam_v_latents": eng.v_lat}
        if eng.train_decoder:
            out.update({"decoder_params": eng.flat, "adam_m_decoder": eng.m_dec, "adam_v_decoder": eng.v_dec})
        return out

    measure.outputs = outputs
    # defer: the caller decides when the measurement runs (the headline: first; again behind the sub-records as `sustained`)
    return measure if defer else measure()


def _measure(shape, args, world, dev, dtype, step, barrier, steps, warmup, eng, paths):
    """W untimed warm-up steps, barrier + synchronize, EXACTLY K timed steps, barrier + synchronize (the driver's contract)."""
    import torch
    from reni_amd import ops
    cfg, B, P = shape["cfg"], shape["B"], shape["P"]
    for s in range(warmup):
        step(s)
    barrier()
    ops.profile_enable(True)
    ops.profile_read(reset=True, kind=ops.PROF_ALL)
    ops.launch_count(reset=True)
    if eng is not None:
        eng.time_comm(True)
    t0 = time.perf_counter()
    last = None
    for s in range(steps):
        last = step(warmup + s)
    barrier()
    dt = time.perf_counter() - t0
    launches = ops.launch_count(reset=True)
    kind = ops.PROF_FWD if cfg == "c5" else ops.PROF_FWD_BWD
    kern_ms, kern_n = ops.profile_read(reset=False, kind=kind)
    kern_min, kern_max = ops.profile_minmax(kind)
    dw1_ms, dw1_n = ops.profile_read(reset=False, kind=ops.PROF_DW1)
    dw1_min, dw1_max = ops.profile_minmax(ops.PROF_DW1) if dw1_n else (None, None)
    dws_ms, dws_n = ops.profile_read(reset=False, kind=ops.PROF_DWS)
    stats_ms, stats_n = ops.profile_read(reset=False, kind=ops.PROF_STATS)
    comm_us = eng.time_comm(False) if eng is not None else None   # (the fused data-parallel step: the library's PROF_COMM pairs)
    ops.profile_read(reset=True, kind=ops.PROF_ALL)
    ops.profile_enable(False)
    check = float(last[0]) if cfg != "c5" else float(last.abs().max())
    assert check == check and abs(check) < 1e6, f"non-finite result {check}"

    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax)
    value = world * B * P * steps / dt

    kavg_ms = kern_ms / max(kern_n, 1)
    H = shape["hidden"]
    if cfg == "c2":
        flop = flop_train(shape["ND"], H, 5)
        assert H != 128 or flop == FLOP_TRAIN
        l0x = isinstance(paths, dict) and paths.get("dw1_kernel") == "k_reni_l0_ring"   # (round 5: the L0X instance + k_reni_l0_ring)
        wide = dtype == "bf16" and H == 256 and isinstance(paths, dict) and paths.get("persistent_kernels")  # (round 5: k_reni_wide256<2> feeds k_dw_frag)
        kernel = (("k_reni_train_bf16<128,true,L0X>" if l0x else "k_reni_train_bf16<128,true>") if (dtype == "bf16" and H == 128)
                  else "k_reni_wide256<2>" if wide else f"k_reni_main<{dtype},H={H},FWD_BWD>")
        workload = (f"BASELINE config 2: 615-image set, {shape['res'][0]}x{shape['res'][1]} equirect, ND=36, 5x{H} SIREN, SO2, tanh, "
                    "AutoDecoder, RENITrainLoss; full training step (fwd+loss+bwd, grad all-reduce, Adam)")
    elif cfg == "film":
        flop = flop_film(shape["ND"], H, 4)
        assert H != 128 or flop == FLOP_FILM
        kernel = (("k_reni_train_bf16<128,true,false,true>" if H == 128 else "k_reni_wide256<2,FILM>") if dtype == "bf16"
                  else f"k_reni_main<f32,H={H},FWD_BWD,FILM>")
        workload = (f"config 2's set and step with the reference's default conditioning: RENIAutoDecoderFiLM, SO2, ND=36, 5 FiLM "
                    f"layers x {H}, mapping network 3 x {H}, tanh; full training step (mapping network, fwd+loss+bwd, glue "
                    "backward, grad all-reduce, Adam over decoder + mapping network + latents)")
    elif cfg == "c4":
        flop = flop_frozen(shape["ND"], H, 5)
        assert H != 128 or flop == FLOP_FROZEN
        kernel = ("k_reni_wide256<1>" if H == 256 else "k_reni_train_bf16<128,false>") if dtype == "bf16" else f"k_reni_main<f32,H={H},FWD_BWD>"
        workload = (f"BASELINE config 4: test-time latent optimisation, 21 held-out maps, 128x256 equirect, ND=36, 5x{H} SIREN, "
                    "frozen decoder, the reference's Mask-3 (18.8 % kept), RENITestLoss(1e-7,1e-4) with the cosine term, per-image "
                    "latent Adam lr 0.1; full step (statistics pass where the cosine term is live + latent fwd/bwd + Adam)")
    else:
        flop = flop_fwd(shape["ND"], H, 5)
        assert H != 128 or flop == FLOP_FWD_ND49
        kernel = f"k_reni_main<f32,H={H},FWD>" if dtype == "f32" else ("k_reni_wide256<0>" if H == 256 else "k_reni_train_bf16<128,false,true>")
        workload = f"BASELINE config 5: inference, 512x1024 directions, ND=49, 5x{H} SIREN, {shape['eq']}, 4 images per step"
    # achieved = the algorithmic FLOPs of the timed steps / the dominant kernel's total run time in them (HIP events on its stream):
    # per launch this is flop x samples per launch / average launch duration, also when a step is several launches (H = 256: chunks)
    # (c4 with RENI_WEIGHT_SPARSE: only the tiles the kernel visits are counted -- `value` counts every direction of the images, as the
    # reference evaluates them all for the same result)
    visited = shape["sparsity"]["tiles_visited"] if shape.get("sparsity") else 1.0
    step_flops = visited * B * P * steps * flop
    # `frac`: the algorithmic FLOPs of the timed steps over the SUMMED run time of the kernels that perform them -- the chain
    # kernel plus whatever finishes the backward pass behind it (k_reni_l0_ring / k_reni_dw1*: PROF_DW1; k_dw_frag / k_dw_stream /
    # k_wide_head_dw: PROF_DWS), each timed with HIP events on its own stream.  Moving work from one kernel into another cannot raise it.
    #   frac_step   the same FLOPs over the whole step's wall time (every kernel, every gap)
    #   frac_issued per kernel: the MFMA FLOPs it issues (SQ_INSTS_MFMA of the PMC passes x FLOP per instruction) over its own time
    work_ms = kern_ms + dw1_ms + dws_ms
    achieved = step_flops / (max(work_ms, 1e-9) * 1e-3) / 1e12
    pmc = pmc_record(kernel)
    peak = PEAK_TFLOPS[dtype]
    mfma_flop = 32768.0 if dtype == "bf16" else 4096.0   # v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x2_f32

    def issued(rec, avg_ms):
        return (rec["mfma_per_launch"] * mfma_flop / (avg_ms * 1e-3) / 1e12 / peak) if rec.get("mfma_per_launch") and avg_ms > 0 else None

    roof = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
            "frac": achieved / peak, "frac_step": step_flops / dt / 1e12 / peak, "frac_issued": issued(pmc, kavg_ms),
            "traffic": pmc.get("hbm_bytes_per_launch"), "kernel": kernel,
            "kernel_avg_ms": kavg_ms, "kernel_min_ms": kern_min, "kernel_max_ms": kern_max, "kernel_launches": kern_n,
            "work_kernels_ms_per_step": work_ms / steps, "flop_per_sample": flop}
    kernels = [{"kernel": kernel, "avg_ms": kavg_ms, "frac_issued": roof["frac_issued"], "traffic": pmc.get("hbm_bytes_per_launch")}]
    if dw1_n:
        # (named from the kernel the call LAUNCHED -- reni_path_info answers for the plan, the L0X form also needs WeightedMSE,
        #  no output image and 16-byte aligned target / weight rows; bench's step meets them, and the PROF_DW1 pairs exist only if it ran)
        k2 = paths.get("dw1_kernel", "k_reni_dw1") if isinstance(paths, dict) else "k_reni_dw1"
        p2 = pmc_record(k2)
        a2 = dw1_ms / dw1_n
        kernels.append({"kernel": k2, "avg_ms": a2, "min_ms": dw1_min, "max_ms": dw1_max, "launches": dw1_n,
                        "traffic": p2.get("hbm_bytes_per_launch"), "frac_issued": issued(p2, a2),
                        "hbm_frac": (p2["hbm_bytes_per_launch"] / (a2 * 1e-3) / 8e12) if p2.get("hbm_bytes_per_launch") else None})
    if dws_n:
        kernels.append({"kernel": "k_dw_frag + k_wide_head_dw" if H == 256 and dtype == "bf16" else "k_dw_frag32" if H == 256 else "k_dw_stream",
                        "ms_per_step": dws_ms / steps, "launches": dws_n})
    if len(kernels) > 1:
        roof["kernels"] = kernels
    if pmc.get("valu_per_mfma"):
        # the co-bound: one wave per SIMD issues the SIREN's activation / epilogue VALU through the same port as its
        # MFMAs; `issue_limited_frac` is the MFMA-peak fraction that instruction mix allows even with perfect overlap
        vpm, tpm = pmc["valu_per_mfma"], pmc.get("trans_per_mfma", 2.1)
        roof.update({"bound": "mfma+valu_issue", "valu_per_mfma": vpm, "trans_per_mfma": tpm, "issue_limited_frac": issue_ceiling(vpm, tpm)})
    if stats_n:
        roof["stats_pass_avg_ms"] = stats_ms / stats_n
    rec = {"value": value, "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup, "dtype": dtype,
           "launches_per_step": launches / steps,
           "config": {"workload": workload, "images_per_gpu_per_step": B, "global_batch_images": world * B,
                      "directions_per_image": P, "parallelism": f"dp{world}", "result_check": check, "paths": paths},
           "roofline": roof}
    if shape.get("sparsity"):
        rec["config"]["weight_sparsity"] = shape["sparsity"]
    fused_dp = eng is not None and eng.comm is not None and eng._stage is not None
    if eng is not None and cfg == "c4":
        rec["config"]["step_call"] = "reni_latent_step_rows (one call: statistics pass where live + fwd + loss + bwd, Adam on the latent table)"
    if eng is not None and cfg == "c2":
        rec["config"]["step_call"] = ("reni_train_step_rows_dp (one call: fwd+loss+bwd, RCCL all-reduce inside, Adam, next prologue)" if fused_dp
                                      else "reni_train_step_rows (one call: fwd+loss+bwd, Adam, next prologue)" if eng._stage is not None
                                      else "reni_forward_loss_backward_rows + all-reduce + reni_adam_step2 (three calls)" if (world > 1 or eng.comm is not None)
                                      else "reni_forward_loss_backward_rows + reni_adam_step2")
    if eng is not None and cfg == "film":
        rec["config"]["step_call"] = "reni_film_model_forward_loss_backward + all-reduce + reni_adam_step"
    if (world > 1 or (eng is not None and eng.comm is not None)) and cfg in ("c2", "film"):
        rec["exchange"] = {"kind": ("inside reni_train_step_rows_dp (librccl, the library's communicator)" if fused_dp
                                    else "reni_allreduce_grads (C ABI, librccl)" if eng.comm is not None
                                    else f"torch.distributed all_reduce ({torch.distributed.get_backend()})"),
                           "avg_us_on_compute_stream": comm_us}
        if _COMM.get("error"):
            rec["exchange"]["comm_fallback"] = _COMM["error"]
    return rec, last


METRIC_FWD = "directional-samples/sec (fwd), 512x1024 equirect, ND=49 latent"
METRIC_TRAIN = "directional-samples/sec (fwd+bwd), 128x256 equirect, ND=36 latent"
CURRIC = ((16, 32), (32, 64), (64, 128))   # configs/experiment.yaml:31-33: INITAL_RESOLUTION doubled at CURRICULUM's epochs


def sub_record(name, args, rank, world, dev):
    """One sub-record of the default line (same process): two windows of 20 timed steps behind 10 warm-up steps each, the faster one
    reported (`ms_per_step_windows` lists both)."""
    kw = dict(steps=20, warmup=10, defer=True)
    if name == "c2_b100":     # config 2 at the shipped experiment.yaml's batch of 100 images
        m = run_config("c2", args, rank, world, dev, batch=100, **kw)
    elif name.startswith("c2_curric_"):   # the reference's real schedule: B = 100 at 16x32 / 32x64 / 64x128
        h, w = (int(x) for x in name[len("c2_curric_"):].split("x"))
        m = run_config("c2", args, rank, world, dev, batch=100, res=(h, w), **kw)
    elif name == "c4_dense":  # config 4 with RENI_WEIGHT_SPARSE off: every tile, and the statistics pass (the figure of rounds 1-3)
        m = run_config("c4", args, rank, world, dev, dense=True, **kw)
    elif name == "c4_pixels":  # config 4 with RENI_WEIGHT_COMPACT: the pixels with weight packed into each image's first tiles
        m = run_config("c4", args, rank, world, dev, pixels=True, **kw)
    elif name == "c4_f32":    # config 4 on the fp32 (parity-grade) kernels, RENI_WEIGHT_SPARSE: the arithmetic to use when the LATENTS, not
        m = run_config("c4", args, rank, world, dev, force_dtype="f32", **kw)   # only the loss curve, must track the reference
    elif name == "c2_h256":   # the width of the reference's shipped configs (configs/default.py:13)
        m = run_config("c2", args, rank, world, dev, hidden=256, **kw)
    elif name == "c4_h256":   # config 4's step at that width (k_reni_wide256: round 5), RENI_WEIGHT_SPARSE as RENI.training_step passes it
        m = run_config("c4", args, rank, world, dev, hidden=256, **kw)
    elif name == "c4_h256_dense":
        m = run_config("c4", args, rank, world, dev, hidden=256, dense=True, **kw)
    elif name == "film_h256":  # the reference's DEFAULT model at its shipped width (configs/default.py:9,13): FiLM, 5 x 256, mapping 3 x 256
        m = run_config("film", args, rank, world, dev, hidden=256, **kw)
    elif name == "fwd_h256":  # config 5's shape (4 x 524 288 directions, ND = 49) forward at H = 256 in bf16
        m = run_config("c5", args, rank, world, dev, hidden=256, force_dtype="bf16", **kw)
    else:
        m = run_config(name, args, rank, world, dev, **kw)
    # Two windows of W + K steps, the faster one reported and both listed: a sub-millisecond step is several host calls, and on a
    # shared host a window now and then stalls on the CPU side (seen: 1.6 ms per step around 0.45 ms of kernels whose own times were
    # unchanged; profiles/tools/gpu_c4_twice.py).  Sub-records only -- the headline is its one contract window.
    wins = [m(), m()]
    r = min(wins, key=lambda x: x["ms_per_step"])
    out = {"metric": METRIC_FWD if name in ("c5", "fwd_h256") else METRIC_TRAIN.replace("128x256", "%dx%d" % tuple(int(x) for x in name[10:].split("x")))
           if name.startswith("c2_curric_") else METRIC_TRAIN,
           "value": r["value"] / (world if name in ("c4", "c4_dense", "c4_pixels", "c4_f32", "c5", "c4_h256", "c4_h256_dense", "fwd_h256") else 1), "unit": "samples/s",
           "ms_per_step": r["ms_per_step"], "ms_per_step_windows": [w_["ms_per_step"] for w_ in wins],
           "ms_per_step_mean": sum(w_["ms_per_step"] for w_ in wins) / len(wins),   # (not only the faster window)
           "steps": r["steps"], "launches_per_step": r["launches_per_step"],
           "dtype": r["dtype"], "workload": r["config"]["workload"],
           "images_per_gpu_per_step": r["config"]["images_per_gpu_per_step"], "paths": r["config"]["paths"], "roofline": r["roofline"]}
    if "weight_sparsity" in r["config"]:
        out["weight_sparsity"] = r["config"]["weight_sparsity"]
        # with RENI_WEIGHT_SPARSE / _COMPACT `value` counts EVERY direction of the images -- what the reference evaluates for the same
        # result -- although the kernels visit only the tiles that can change it: label it, and print what was visited beside it.
        # The figure to compare with BASELINE config 4 and with rounds 1-3 is `c4_dense`.
        vis = r["config"]["weight_sparsity"]["tiles_visited"]
        out["value_kind"] = "effective_samples_per_s" if vis < 1.0 else "samples_per_s"
        out["visited_samples_per_s"] = out["value"] * vis
    if name == "c5":  # SURVEY 8(d) C5 names both invariances: the SO3 model through the same kernel
        r3 = run_config("c5", args, rank, world, dev, eq="SO3", **kw)()
        out["so3"] = {"value": r3["value"] / world, "ms_per_step": r3["ms_per_step"], "frac": r3["roofline"]["frac"],
                      "kernel_avg_ms": r3["roofline"]["kernel_avg_ms"]}
    if world > 1:
        out["note"] = "per GPU (independent replicas)"
    return out


LINE_MAX = 6144   # bytes of the contract line (round 5's 24 KB line did not parse on the driver's side)


def _r(x, sig=6):
    """floats to `sig` significant digits (the line is read by people and by a parser with a size limit)"""
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def contract_line(metric, rec, world, also, sustained, cpu):
    """THE line: the contract's fields, the headline's roofline (with both kernels of the backward pass), `sustained`, `cpu_baseline`, and
    for every sub-record only [value, ms_per_step, frac_step] -- the sub-records themselves are printed on the lines above it."""
    import torch
    cfgd = dict(rec["config"])
    paths = cfgd.pop("paths", None)
    if isinstance(paths, dict):   # the facts that name the code path, not the whole diagnostic record (that one is on the `also` lines)
        cfgd["paths"] = {k: paths[k] for k in ("persistent_kernels", "dw1_kernel", "side_stream", "env_overrides", "workgroups", "error") if k in paths}
    line = {
        "metric": metric, "value": rec["value"], "unit": "samples/s", "n_gpus": world, "steps": rec["steps"], "warmup": rec["warmup"],
        "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": rec["dtype"], "data": "synthetic",
        "n_ranks_seen": torch.distributed.get_world_size() if world > 1 else 1,
        "dist_backend": torch.distributed.get_backend() if world > 1 else None,
        "launches_per_step": rec["launches_per_step"], "step_call": cfgd.pop("step_call", None),
        "config": cfgd, "roofline": rec["roofline"],
    }
    if "exchange" in rec:
        line["exchange"] = rec["exchange"]
    if sustained is not None:
        line["sustained"] = sustained
    if cpu is not None:
        line["cpu_baseline"] = cpu
    if also is not None:
        line["also"] = {k: ([v["value"], v["ms_per_step"], v["roofline"]["frac_step"]] if "error" not in v else {"error": v["error"][:80]})
                        for k, v in also.items()}
        line["also_fields"] = ["value (samples/s)", "ms_per_step", "roofline.frac_step"]
    return _r(line)


DUMP_BYTES = 64 * 10 ** 6   # --dump-outputs: at most this many bytes of arrays in all


def dump_outputs(d, arrays):
    """--dump-outputs DIR: every array as DIR/<name>.npy in float32.  The smaller arrays go whole; one that does not fit its share of
    DUMP_BYTES is replaced by a fixed, seeded sample of its flattened elements (the same positions in every run at the same arguments),
    so that two builds can be compared output for output."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    left = DUMP_BYTES
    items = sorted(arrays.items(), key=lambda kv: kv[1].nbytes)
    for i, (name, a) in enumerate(items):
        share = left // (len(items) - i) - 256   # (room for the .npy header)
        if a.nbytes > share:
            keep = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[keep]
        np.save(os.path.join(d, name + ".npy"), a)
        left -= a.nbytes + 256


_OUT = None   # the process's REAL stdout once main() has parked fd 1 on stderr (see own_stdout)


def own_stdout():
    """Keep stdout for this program's lines alone: librccl prints a version banner through C stdio on fd 1 when a communicator is created
    (seen on the GPU box: flushed at process exit, i.e. BEHIND the contract line, which must be the last line of stdout), and so may any
    other native library.  fd 1 is duplicated for emit() and then pointed at stderr, in every rank."""
    global _OUT
    if _OUT is None:
        sys.stdout.flush()
        _OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def _say(text):
    out = _OUT or sys.stdout
    out.write(text + "\n")
    out.flush()


def emit(line, also):
    """stdout: one `also <name> {json}` line per sub-record (full record, 7 significant digits), then THE contract line, last and alone
    on its line, at most LINE_MAX bytes."""
    for k, v in (also or {}).items():
        _say("also " + k + " " + json.dumps(_r(v, 7), separators=(",", ":")))
    out = json.dumps(line)
    if len(out) > LINE_MAX:   # (cannot happen with today's fields: drop the optional ones rather than print a line nobody can parse)
        for k in ("also_fields", "exchange", "sustained"):
            line.pop(k, None)
        line["roofline"].pop("kernels", None)
        out = json.dumps(line)
    assert len(out) <= LINE_MAX, len(out)
    _say(out)


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    own_stdout()
    import torch
    from reni_amd import dist as rdist
    try:
        rank, world, local = rdist.init_from_env()
    except Exception as e:  # noqa: BLE001  (a failed rendezvous is the one failure spawn_ranks retries: say so with a code of its own)
        print(f"bench.py: rendezvous failed: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
        sys.exit(EXIT_RENDEZVOUS)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:  # create the RCCL communicator outside the timed region even with --warmup 0
        torch.distributed.all_reduce(torch.zeros(1, device=dev))

    cfg = args.config
    also, sustained = None, None
    if cfg == "c2_curric":   # the line's headline = the curriculum's final resolution; --full: all three in `also`
        if args.full:
            also = {f"c2_curric_{h}x{w}": sub_record(f"c2_curric_{h}x{w}", args, rank, world, dev) for h, w in CURRIC}
        head = run_config("c2", args, rank, world, dev, batch=args.batch or 100, res=CURRIC[-1], defer=True)
    elif cfg == "c2_h256":
        head = run_config("c2", args, rank, world, dev, batch=args.batch, hidden=256, defer=True)
    else:
        res = tuple(int(x) for x in args.res.split("x")) if (args.res and cfg == "c2") else None
        wide = args.hidden == 256 and cfg in ("c4", "c5")
        head = run_config(cfg, args, rank, world, dev, batch=args.batch, res=res, defer=True, dense=args.dense, pixels=args.pixels,
                          hidden=256 if wide else 128, force_dtype="bf16" if (wide and cfg == "c5") else None)  # set-up only
    # THE headline: W warm-up + K timed steps, first, identically with and without the sub-records
    rec = head()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, head.outputs())
    if args.full and cfg == "c2" and not args.no_also:
        # The other BASELINE configurations, the reference's default conditioning, its shipped batch / schedule / width, measured in the
        # same process behind the headline: sub-records, each with its own ms_per_step / launches / roofline.  N > 1: only the two
        # configurations whose ranks are independent (c4, c5: rank 0's own replica).
        also = {}
        user_dtype = args.dtype
        names = (("c4", "c4_dense", "c4_pixels", "c4_f32", "c5", "film", "c2_b100") + tuple(f"c2_curric_{h}x{w}" for h, w in CURRIC) + ("c2_h256", "c4_h256", "c4_h256_dense", "fwd_h256", "film_h256")) if world == 1 else ("c4", "c5")
        for c in names:
            args.dtype = None
            try:
                also[c] = sub_record(c, args, rank, world, dev)
            except Exception as e:  # a sub-record must not cost the headline its line (one process only: with ranks, fail together)
                if world > 1:
                    raise
                also[c] = {"error": f"{type(e).__name__}: {e}"[:300]}
        args.dtype = user_dtype
        # the headline's W + K steps once more, now behind ~0.3 s of load: the clocks a training run sees (side field)
        r1 = head()
        sustained = {"value": r1["value"], "ms_per_step": r1["ms_per_step"], "kernel_avg_ms": r1["roofline"]["kernel_avg_ms"],
                     "frac": r1["roofline"]["frac"], "frac_step": r1["roofline"]["frac_step"], "steps": r1["steps"], "warmup": r1["warmup"],
                     "note": "the same W+K steps again behind the sub-records (sustained clocks); not `value`"}
    metric = METRIC_FWD if cfg == "c5" else METRIC_TRAIN.replace("128x256", "64x128") if cfg == "c2_curric" else METRIC_TRAIN
    if rank == 0:
        emit(contract_line(metric, rec, world, also, sustained,
                           cpu_baseline(args.cpu_steps) if (args.full and world == 1 and not args.no_cpu_baseline) else None), also)
    if _COMM.get("comm") is not None:
        _COMM["comm"].close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
