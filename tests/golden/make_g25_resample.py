"""G25: Gaussian blur of environment maps (src/models/spherical_harmonics.py: blurIBL), by IMPORTING the reference.

Run where the reference checkout and scipy are available (make_golden.py puts the reference on sys.path):

    python tests/golden/make_g25_resample.py

The reference module imports cv2, imageio, scipy.ndimage and matplotlib at module top; whichever is absent is stubbed as
make_g24_diffuse.py does.  scipy must be the real one here: blurIBL is scipy.ndimage.gaussian_filter per channel, and the
script refuses to run on a stub.
Recorded: blurIBL at sigma in {1, 3, 5} of two small float32 maps -- a random positive 16 x 32 map, and a 12 x 24 sky
gradient with one bright texel (sigma 5 has radius 20, beyond both maps' height: the reflect boundary wraps more than once).
Output: tests/golden/g25_resample.npz (plain arrays, well under 500 KB)."""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (stubs gdown / torchvision, puts the reference on sys.path)

import scipy.ndimage  # noqa: E402,F401  (the real one, or this golden means nothing)

for name in ("cv2", "imageio", "matplotlib", "matplotlib.pyplot", "matplotlib.colors"):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib.colors"].__dict__.setdefault("LinearSegmentedColormap", object)
sys.modules["matplotlib"].__dict__.setdefault("pyplot", sys.modules["matplotlib.pyplot"])
sys.modules["cv2"].__dict__.setdefault("INTER_CUBIC", 2)
sys.modules["cv2"].__dict__.setdefault("INTER_LANCZOS4", 4)

from src.models import spherical_harmonics as ref_sh  # noqa: E402

SIGMAS = (1, 3, 5)


def maps():
    g = np.random.default_rng(250)
    rnd = (0.05 + g.random((16, 32, 3))).astype(np.float32)
    H, W = 12, 24
    yy = np.linspace(0, 1, H)[:, None, None]
    sky = (0.2 + 0.8 * (1 - yy)) * np.asarray([0.4, 0.6, 1.0]) + 0.05 * yy * np.asarray([1.0, 0.8, 0.5])
    sky = np.broadcast_to(sky, (H, W, 3)).copy()
    sky[H // 4, (3 * W) // 5] = (60.0, 50.0, 40.0)
    return [rnd, sky.astype(np.float32)]


def main():
    out = {}
    for k, img in enumerate(maps()):
        out[f"blur_img{k}"] = img
        for s in SIGMAS:
            out[f"blur_img{k}_s{s}"] = ref_sh.blurIBL(img, amount=s)
    np.savez_compressed(os.path.join(HERE, "g25_resample.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
