"""G24: diffuse irradiance of environment maps (src/models/spherical_harmonics.py), by IMPORTING the reference.

Run where the reference checkout is available (make_golden.py puts it on sys.path):

    python tests/golden/make_g24_diffuse.py

The reference module imports cv2, imageio, scipy.ndimage and matplotlib at module top.  Whichever is absent is stubbed as
make_g22_baselines.py does, and three stubs are always installed:
  - cv2.resize is the identity when the size is unchanged and raises otherwise (no cv2 arithmetic enters the golden);
  - imageio.imread returns an array from a dict keyed by a fake file name (getDiffuseMap reads its map by name);
  - np.math is a shim whose factorial accepts floats with integral values.  getDiffuseCoefficients calls
    np.math.factorial(l / 2), which numpy 2 and Python >= 3.10 reject; this is the only change to the reference's arithmetic.
Recorded (float64 numpy unless the reference casts):
  getDiffuseMap at (W, widthLowRes) in {(32, 16), (64, 32), (64, 16)} with outputWidth = widthLowRes, for a random positive
  map and a structured one (a single bright texel over a sky gradient); getSolidAngleMap at W in {32, 64};
  getDiffuseCoefficients for lmax 0..15; shRender at lmax in {0, 1, 2, 5} and W in {16, 32, 64}; getNormalMap and
  shReconstructDiffuseMap on 9 coefficients at W in {16, 32, 64}; shReconstructDiffuseNormalMap on random unit normals;
  findWindowingFactor / applyWindowing on one coefficient set below the target (factor 0) and two above it.
Output: tests/golden/g24_diffuse.npz (plain arrays, well under 500 KB)."""
import math
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (stubs gdown / torchvision, puts the reference on sys.path)

for name in ("cv2", "imageio", "scipy", "scipy.ndimage", "matplotlib", "matplotlib.pyplot", "matplotlib.colors"):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib.colors"].__dict__.setdefault("LinearSegmentedColormap", object)
sys.modules["scipy"].__dict__.setdefault("ndimage", sys.modules["scipy.ndimage"])
sys.modules["matplotlib"].__dict__.setdefault("pyplot", sys.modules["matplotlib.pyplot"])

cv2 = sys.modules["cv2"]
cv2.INTER_CUBIC, cv2.INTER_LANCZOS4 = 2, 4


def _resize(img, size, interpolation=None):
    if (img.shape[1], img.shape[0]) != tuple(size):
        raise RuntimeError(f"cv2.resize stub: {img.shape[:2]} -> {size} would resample")
    return img


cv2.resize = _resize
IMAGES = {}
sys.modules["imageio"].imread = lambda name, *args, **kw: IMAGES[name]


class _NpMath:
    @staticmethod
    def factorial(x):
        if float(x) != int(x):
            raise ValueError(f"factorial of a non-integral {x}")
        return math.factorial(int(x))


np.math = _NpMath()

from src.models import spherical_harmonics as ref_sh  # noqa: E402

DM_SHAPES = ((32, 16), (64, 32), (64, 16))
SR_LMAX = (0, 1, 2, 5)
SR_WIDTHS = (16, 32, 64)


def maps(W, seed):
    """[2, W/2, W, 3] float32: a random positive map, and one bright texel over a sky gradient"""
    H = W // 2
    g = np.random.default_rng(seed)
    rnd = (0.05 + g.random((H, W, 3))).astype(np.float32)
    yy = np.linspace(0, 1, H)[:, None, None]
    sky = (0.2 + 0.8 * (1 - yy)) * np.asarray([0.4, 0.6, 1.0]) + 0.05 * yy * np.asarray([1.0, 0.8, 0.5])
    sky = np.broadcast_to(sky, (H, W, 3)).copy()
    sky[H // 4, (3 * W) // 5] = (60.0, 50.0, 40.0)
    return np.stack([rnd, sky.astype(np.float32)])


def main():
    out = {}
    for W in sorted({w for w, _ in DM_SHAPES}):
        out[f"dm_w{W}_imgs"] = maps(W, 240 + W)
        out[f"sa_w{W}"] = ref_sh.getSolidAngleMap(W)
    for W, wl in DM_SHAPES:
        res = []
        for k, img in enumerate(out[f"dm_w{W}_imgs"]):
            IMAGES[f"map{k}.exr"] = img
            res.append(ref_sh.getDiffuseMap(f"map{k}.exr", width=W, widthLowRes=wl, outputWidth=wl))
        out[f"dm_w{W}_l{wl}"] = np.stack(res)
    for lmax in range(16):
        out[f"dc_l{lmax}"] = ref_sh.getDiffuseCoefficients(lmax)
    g = np.random.default_rng(241)
    for lmax in SR_LMAX:
        c = g.normal(size=(ref_sh.shTerms(lmax), 3))
        c[0] += 2.0
        out[f"sr_l{lmax}_coeffs"] = c
        for W in SR_WIDTHS:
            out[f"sr_l{lmax}_w{W}"] = ref_sh.shRender(c.copy(), W)
    c9 = out["sr_l2_coeffs"]
    for W in SR_WIDTHS:
        out[f"nm_w{W}"] = ref_sh.getNormalMap(W)
        out[f"srd_w{W}"] = ref_sh.shReconstructDiffuseMap(c9.copy(), W)
    n = g.normal(size=(8, 12, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    out["srn_normals"] = n
    out["srn_out"] = ref_sh.shReconstructDiffuseNormalMap(c9.copy(), n)
    win = [0.01 * g.normal(size=(9, 3)),                # below the target: factor 0, coefficients unchanged
           0.5 + g.random((9, 3)),                      # above it
           0.2 + g.random((36, 3))]                     # above it, lmax 5
    for k, c in enumerate(win):
        out[f"win{k}_coeffs"] = c
        f = ref_sh.findWindowingFactor(c.copy())
        out[f"win{k}_factor"] = np.float64(f)
        out[f"win{k}_applied"] = ref_sh.applyWindowing(c.copy(), f)
        out[f"win{k}_applied_auto"] = ref_sh.applyWindowing(c.copy())
    np.savez_compressed(os.path.join(HERE, "g24_diffuse.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
