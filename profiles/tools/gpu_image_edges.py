"""The image epilogue at its edges and on the clock; both modes use whichever library RENI_HIP_LIB names (a
library built from another commit, for a before / after in alternating processes) or the tree's own.  From the repository root:

  python profiles/tools/gpu_image_edges.py probe    what the library returns for the inputs of tests/test_gpu_image.py's NaN,
        zero-exposure and -0.0 cases: counts of NaN and 0.0 and the value range, no verdicts
  python profiles/tools/gpu_image_edges.py time     ms per call of ops.unnormalise_srgb (8 x 3 x 512 x 1024, a model output read
        in place), ops.minmax_normalise (the 12.6 M values as one image) and ops.minmax_normalise_batch (as 8 images): device
        events around 30 calls, best of 5, after 5 warm-up calls"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from reni_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
MM = [-18.0536, 11.4633]


def randexp(seed, *shape):
    return torch.exp(2 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def probe():
    for c in range(3):
        x = randexp(40 + c, 2, 3, 9, 14)
        clean = ops.unnormalise_srgb(x.to(DEV), None, srgb=True).cpu()
        x[0, c, 4, 6] = float("nan")
        out = ops.unnormalise_srgb(x.to(DEV), None, srgb=True).cpu()
        print(f"NaN in channel {c}: image 0 has {int(torch.isnan(out[0]).sum())} NaN and {int((out[0] == 0).sum())} zeros of "
              f"{out[0].numel()}; the NaN pixel reads {float(out[0, c, 4, 6])}; largest change elsewhere in image 0 against the "
              f"clean image {float(torch.nan_to_num(out[0] - clean[0], nan=float('inf')).abs().max()):.3g}; image 1 changed: "
              f"{not torch.equal(out[1], clean[1])}")
    x = torch.zeros(2, 3, 101, 4)
    x[0, :, 99:, :] = randexp(60, 3, 2, 4)
    out = ops.unnormalise_srgb(x.to(DEV), None, srgb=True).cpu()
    dark = out[0, :, :99]
    print(f"q == 0: lit pixels {float(out[0, :, 99:].min())} .. {float(out[0, :, 99:].max())}; zero pixels: {int(torch.isnan(dark).sum())} "
          f"NaN, {int((dark == 0).sum())} zeros of {dark.numel()}; all-zero image: {int(torch.isnan(out[1]).sum())} NaN, "
          f"{int((out[1] == 0).sum())} zeros of {out[1].numel()}")
    x = randexp(70, 3, 5, 7)
    x.view(-1)[17] = -0.0
    one = ops.minmax_normalise(x.to(DEV), MM).cpu()
    raw = ops.minmax_normalise_batch(x[None].to(DEV), MM, nan_to_num=False).cpu()
    num = ops.minmax_normalise_batch(x[None].to(DEV), MM, nan_to_num=True).cpu()
    print(f"-0.0 among positive values: minmax_normalise {float(one.min())} .. {float(one.max())}; batch {float(raw.min())} .. "
          f"{float(raw.max())}; batch with nan_to_num {float(num.min())} .. {float(num.max())}")


def time_calls():
    x = (torch.rand(8, 512 * 1024, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    x = x.view(8, 512, 1024, 3).permute(0, 3, 1, 2)
    lin = ops.unnormalise_srgb(x, MM, srgb=False)

    def ms(f, n=30):
        for _ in range(5):
            f()
        best = float("inf")
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                f()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / n)
        return best

    print(f"sRGB view 8x3x512x1024 {ms(lambda: ops.unnormalise_srgb(x, MM, srgb=True)):.4f} ms  "
          f"minmax_normalise 12.6M {ms(lambda: ops.minmax_normalise(lin, MM)):.4f} ms  "
          f"minmax_normalise_batch 8 images {ms(lambda: ops.minmax_normalise_batch(lin, MM)):.4f} ms")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("probe", "time"):
        sys.exit(__doc__)
    print("library:", "RENI_HIP_LIB" if os.environ.get("RENI_HIP_LIB") else "the tree's", os.path.basename(_lib.LIB_PATH))
    probe() if mode == "probe" else time_calls()
