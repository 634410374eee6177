"""Spherical-Gaussian and spherical-harmonic environment-map baselines on the GPU: what RENI is compared against.

Restates the reference's src/models/spherical_gaussians.py (SGEnvOptim) and src/models/spherical_harmonics.py with the
same call shapes: the projection / reconstruction part, and the diffuse irradiance part (getDiffuseMap's brute-force
clamped-cosine convolution, the Ramamoorthi-Hanrahan SH irradiance shRender / shRenderL2, Sloan's ringing window).  The
arithmetic runs in libreni_hip.so (reni_tu_baselines.hip, reni_tu_diffuse.hip); torch supplies device memory and, for
SGEnvOptim, its own LBFGS.  The small float64 helpers (grids, solid angles, diffuse coefficients, the windowing factor)
stay on the host.  There is no CPU fallback.

Differences from the reference, all deliberate:
  - SGEnvOptim.optimize(envmap, sineweight=None) treats sineweight=None as a weight of 1 everywhere (the reference
    crashes on None).
  - getCoefficientsFromImage's resizeWidth / filterAmount (cv2 / scipy) raise NotImplementedError, and a map wider than
    1000 pixels -- which the reference silently resizes to 1000 x 500 -- raises ValueError.
    resizeImage (bicubic / Lanczos) and blurIBL below are the device restatements to do that with; the wrappers themselves
    keep refusing, so nothing is resampled behind the caller's back.
  - resizeImage has no "max_pooling" option (skimage), and cv2 is on no machine this was developed on: bicubic is pinned
    against torch's float64 bicubic, Lanczos against its closed form, not against cv2 itself.
  - The SH maps are read as float32 on the device; coefficients come back as float64 arrays, as in the reference.
  - getDiffuseCoefficients uses the integer (l // 2)!.  The reference calls np.math.factorial(l / 2), which cannot run
    here (numpy 2 has no np.math, and Python >= 3.10 rejects a float factorial); the integer form is the formula it
    intends.
  - getDiffuseMap(ibl, ...) accepts an array, a tensor, or a path read with reni_amd.exr.read_exr.  The reference always
    resizes the map to `width` with cv2 (bicubic) and, when widthLowRes < outputWidth, upsamples the result with cv2
    (Lanczos); both raise NotImplementedError here unless they are identities (the map is already width x width / 2 and
    widthLowRes >= outputWidth).  The reference's prints and timing are dropped.
  - shRender, shRenderL2 and getDiffuseMap compute in float32 on the device (the reference: float64 on the host).
Kept on purpose (the golden pins them): getDiffuseMap's own grid (directions at pixel corners, v flipped, solid angles of
the row centres, output pixel (x, y) looking along input pixel (int(x / wL W), int(y / hL H))), findWindowingFactor's
m in range(-1, l + 1) and unsquared mean, and shReconstructDiffuseMap's L2 closed form for exactly 9 coefficients.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib, ops

# ----------------------------------------------------------------------------------------------- spherical Gaussians


def sg_lobe_centres(SGRow: int, SGCol: int, device=None):
    """(theta_c [K], phi_c [K], theta_range, phi_range) as SGEnvOptim builds them (:29-39): lobe k = row * SGCol + col,
    centres computed in float64 and rounded to float32."""
    phi = ((np.arange(SGCol) + 0.5) / SGCol - 0.5) * np.pi * 2
    theta = (np.arange(SGRow) + 0.5) / SGRow * np.pi / 2.0
    phi, theta = np.meshgrid(phi, theta)
    tc = torch.from_numpy(theta.reshape(-1).astype(np.float32))
    pc = torch.from_numpy(phi.reshape(-1).astype(np.float32))
    if device is not None:
        tc, pc = tc.to(device), pc.to(device)
    return tc, pc, (np.pi / 2 / SGRow) * 1.5, (2 * np.pi / SGCol) * 1.5


def _raw(params, K=None):
    N = params.shape[0]
    K = params.numel() // (6 * N) if K is None else K
    return params.reshape(N, K, 6)


def sg_render(params: torch.Tensor, SGRow: int, SGCol: int, envHeight: int, envWidth: int) -> torch.Tensor:
    """renderSG of the reparametrised raw parameters: params [N, K * 6] or [N, K, 6] (per lobe w~0..2, theta~, phi~,
    lambda~) -> rec [N, 3, envHeight, envWidth].  Not differentiable (see sg_loss)."""
    tc, pc, tr, pr = sg_lobe_centres(SGRow, SGCol, params.device)
    return ops.sg_render(_raw(params.detach(), SGRow * SGCol), tc, pc, tr, pr, envHeight, envWidth)


class _SGLoss(torch.autograd.Function):
    """WeightedMSE(log(renderSG(params) + 1), log_target, weight) with the fused kernel's gradient."""

    @staticmethod
    def forward(ctx, params, theta_c, phi_c, theta_range, phi_range, log_target, weight):
        total, _, grad = ops.sg_loss_grad(_raw(params.detach(), theta_c.numel()), theta_c, phi_c, theta_range, phi_range,
                                          log_target, weight)
        ctx.save_for_backward(grad)
        ctx.shape = params.shape
        return total

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape), None, None, None, None, None, None


def sg_loss(params: torch.Tensor, log_target: torch.Tensor, weight, SGRow: int, SGCol: int) -> torch.Tensor:
    """Scalar loss sum_n mean_(c, p) weight (log(rec + 1) - log_target)^2, differentiable with respect to params
    ([N, K * 6] or [N, K, 6]).  log_target [N, 3, H, W] = log(env + 1); weight broadcasts to [N, 3, H, W] (None: 1)."""
    tc, pc, tr, pr = sg_lobe_centres(SGRow, SGCol, params.device)
    if weight is None:
        weight = torch.ones(1, 1, 1, 1, device=params.device)
    return _SGLoss.apply(params, tc, pc, tr, pr, log_target, weight)


class SGEnvOptim:
    """SGEnvOptim (src/models/spherical_gaussians.py) on the fused HIP kernel: fits SGRow x SGCol spherical Gaussians to
    each of envNum environment maps with torch's LBFGS(lr 0.2, max_iter 100), niter outer steps."""

    def __init__(self, isCuda=True, gpuId=0, niter=10, envNum=19200, envWidth=32, envHeight=16, SGRow=2, SGCol=6, ch=3):
        if not isCuda:
            raise _lib.RENILibraryError("SGEnvOptim runs on a GPU device (isCuda=True); there is no CPU fallback")
        if ch != 3:
            raise ValueError(f"SGEnvOptim supports ch == 3 only, got {ch}")
        self.SGNum = int(SGRow * SGCol)
        if not 1 <= self.SGNum <= 64:
            raise ValueError(f"SGRow * SGCol must be in [1, 64], got {self.SGNum}")
        self.envNum, self.niter, self.ch = envNum, niter, ch
        self.envHeight, self.envWidth = envHeight, envWidth
        self.SGRow, self.SGCol = SGRow, SGCol
        self.isCuda, self.gpuId = isCuda, gpuId
        self.iterCount = 0
        self.device = torch.device("cuda", gpuId)
        self.thetaCenter, self.phiCenter, self.thetaRange, self.phiRange = sg_lobe_centres(SGRow, SGCol, self.device)
        weight = torch.zeros(envNum, self.SGNum, 3)
        theta = torch.zeros(envNum, self.SGNum, 1)
        phi = torch.zeros(envNum, self.SGNum, 1)
        lamb = torch.log(torch.ones(envNum, self.SGNum, 1) * np.pi / SGRow)
        self.param = torch.cat([weight, theta, phi, lamb], dim=2).view(envNum, self.SGNum * 6).to(self.device)
        self.param.requires_grad = True
        self.optEnv = torch.optim.LBFGS([self.param], lr=0.2, max_iter=100)
        self.loss = None

    def deparameterize(self):
        """(theta, phi, weight, lamb) [N, K, 1 | 1 | 3 | 1] after the reparametrisation of optimize's closure."""
        p = self.param.detach().view(self.envNum, self.SGNum, 6)
        theta = self.thetaRange * torch.tanh(p[:, :, 3:4]) + self.thetaCenter.view(1, -1, 1)
        phi = self.phiRange * torch.tanh(p[:, :, 4:5]) + self.phiCenter.view(1, -1, 1)
        return theta, phi, torch.exp(p[:, :, 0:3]), torch.exp(p[:, :, 5:6])

    def renderSG(self):
        """The current parameters' maps [envNum, 3, envHeight, envWidth]."""
        return ops.sg_render(self.param.detach().view(self.envNum, self.SGNum, 6), self.thetaCenter, self.phiCenter,
                             self.thetaRange, self.phiRange, self.envHeight, self.envWidth)

    def optimize(self, envmap, sineweight=None):
        """-> (thetaBest [N, K, 1], phiBest [N, K, 1], lambBest [N, K, 1], weightBest [N, K, 3], recImageBest [N, 3, H, W]),
        float32 numpy arrays of the best outer step (all None if the first step's loss is not below 2e20 or is NaN)."""
        assert (envmap.shape[0] == self.envNum and envmap.shape[1] == self.ch and envmap.shape[2] == self.envHeight
                and envmap.shape[3] == self.envWidth)
        env = torch.as_tensor(envmap).to(self.device, torch.float32)
        log_target = torch.log(env + 1).contiguous()
        if sineweight is None:
            weight = torch.ones(1, 1, 1, 1, device=self.device)
        else:
            weight = torch.as_tensor(sineweight).to(self.device, torch.float32)
        minLoss = 2e20
        recImageBest = thetaBest = phiBest = weightBest = lambBest = None
        self.loss = None
        for _ in range(self.niter):

            def closure():
                loss = _SGLoss.apply(self.param, self.thetaCenter, self.phiCenter, self.thetaRange, self.phiRange,
                                     log_target, weight)
                self.loss = loss
                self.optEnv.zero_grad()
                loss.backward()
                self.iterCount += 1
                return loss

            self.optEnv.step(closure)
            loss = float(self.loss.item())
            if loss < minLoss:
                if torch.isnan(torch.sum(self.param)):
                    break
                theta, phi, weight_, lamb = self.deparameterize()
                recImageBest = self.renderSG().cpu().numpy()
                thetaBest = theta.cpu().numpy().reshape(self.envNum, self.SGNum, 1)
                phiBest = phi.cpu().numpy().reshape(self.envNum, self.SGNum, 1)
                lambBest = lamb.cpu().numpy().reshape(self.envNum, self.SGNum, 1)
                weightBest = weight_.cpu().numpy().reshape(self.envNum, self.SGNum, 3)
                minLoss = loss
            else:
                break
        return thetaBest, phiBest, lambBest, weightBest, recImageBest


# ----------------------------------------------------------------------------------------------- spherical harmonics


def shTerms(lmax):
    return (lmax + 1) * (lmax + 1)


def shIndex(l, m):
    return l * l + l + m


def sh_lmax_from_terms(terms):
    return int(np.sqrt(terms) - 1)


def calc_num_sh_coeffs(order):
    return sum(2 * i + 1 for i in range(order + 1))


def get_sh_order(ndims):
    order = 0
    while calc_num_sh_coeffs(order) < ndims:
        order += 1
    return order


def _legendre(l, m, x):
    """associated Legendre P_l^m(x) by the reference's recursion (spherical_harmonics.py P, :45-68), float64"""
    pmm = np.ones_like(x)
    if m > 0:
        somx2 = np.sqrt((1.0 - x) * (1.0 + x))
        fact = 1.0
        for _ in range(1, m + 1):
            pmm = pmm * (-fact) * somx2
            fact += 2.0
    if l == m:
        return pmm
    pmmp1 = x * (2.0 * m + 1.0) * pmm
    if l == m + 1:
        return pmmp1
    pll = np.zeros_like(x)
    for ll in range(m + 2, l + 1):
        pll = ((2.0 * ll - 1.0) * x * pmmp1 - (ll + m - 1.0) * pmm) / (ll - m)
        pmm, pmmp1 = pmmp1, pll
    return pll


def _knorm(l, m):
    return np.sqrt(((2 * l + 1) * float(math.factorial(l - m))) / (4 * np.pi * float(math.factorial(l + m))))


def sh_tables(width: int, lmax: int, solid_angle: bool):
    """The separable basis of getCoefficientsMatrix(width, lmax) in float64: row [H, T] (K P, sqrt 2 for m != 0; times
    getSolidAngle of the row when solid_angle) and col [W, T] (cos(m phi), 1, sin(|m| phi)); Y_t(y, x) = row[y, t] col[x, t].
    Angles of the pixel's top-left corner: theta = y pi / H, phi = x 2 pi / W."""
    W = int(width)
    H = W // 2
    T = shTerms(lmax)
    theta = np.arange(H) / (float(H) / np.pi)
    phi = np.arange(W) / (float(W) / (np.pi * 2))
    ct = np.cos(theta)
    row = np.zeros((H, T))
    col = np.zeros((W, T))
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            t = shIndex(l, m)
            if m == 0:
                row[:, t] = _knorm(l, 0) * _legendre(l, 0, ct)
                col[:, t] = 1.0
            elif m > 0:
                row[:, t] = np.sqrt(2.0) * _knorm(l, m) * _legendre(l, m, ct)
                col[:, t] = np.cos(m * phi)
            else:
                row[:, t] = np.sqrt(2.0) * _knorm(l, -m) * _legendre(l, -m, ct)
                col[:, t] = np.sin(-m * phi)
    if solid_angle:
        th = (1.0 - ((np.arange(H) + 0.5) / H)) * np.pi
        row *= ((np.pi * 2) / W * (np.cos(th - (np.pi / H / 2.0)) - np.cos(th + (np.pi / H / 2.0))))[:, None]
    return row, col


_TABLES = {}


def _device_tables(width, lmax, solid_angle, device):
    key = (int(width), int(lmax), bool(solid_angle), str(device))
    if key not in _TABLES:
        row, col = sh_tables(width, lmax, solid_angle)
        _TABLES[key] = (torch.from_numpy(row.astype(np.float32)).to(device),
                        torch.from_numpy(col.astype(np.float32)).to(device))
    return _TABLES[key]


def _check_sh(width, lmax):
    if not 0 <= int(lmax) <= 15:
        raise ValueError(f"lmax must be in [0, 15], got {lmax}")
    if int(width) < 2 or int(width) % 2:
        raise ValueError(f"the map width must be even and >= 2, got {width}")


def sh_project(imgs: torch.Tensor, lmax: int) -> torch.Tensor:
    """getCoefficientsFromImage for a batch: imgs [N, W/2, W, 3] on the GPU -> coeffs [N, (lmax + 1)^2, 3] float32."""
    if imgs.dim() != 4 or imgs.shape[3] != 3 or 2 * imgs.shape[1] != imgs.shape[2]:
        raise ValueError(f"imgs must be [N, W/2, W, 3], got {tuple(imgs.shape)}")
    _check_sh(imgs.shape[2], lmax)
    ops._require_cuda(imgs)
    row, col = _device_tables(imgs.shape[2], lmax, True, imgs.device)
    return ops.sh_project(imgs, row, col, int(lmax))


def sh_reconstruct(coeffs: torch.Tensor, width: int) -> torch.Tensor:
    """shReconstructSignal for a batch: coeffs [N, T, 3] on the GPU (T a square) -> maps [N, width/2, width, 3] float32."""
    if coeffs.dim() != 3 or coeffs.shape[2] != 3:
        raise ValueError(f"coeffs must be [N, T, 3], got {tuple(coeffs.shape)}")
    lmax = sh_lmax_from_terms(coeffs.shape[1])
    if shTerms(lmax) != coeffs.shape[1]:
        raise ValueError(f"the number of SH terms must be a square, got {coeffs.shape[1]}")
    _check_sh(width, lmax)
    ops._require_cuda(coeffs)
    row, col = _device_tables(width, lmax, False, coeffs.device)
    return ops.sh_reconstruct(coeffs, row, col, int(width) // 2, int(width), lmax)


def _gpu():
    if not torch.cuda.is_available():
        raise _lib.RENILibraryError("the SH baselines run on a GPU device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def getCoefficientsFromImage(ibl, lmax=2, resizeWidth=None, filterAmount=None):
    """SH coefficients [(lmax + 1)^2, 3] float64 of an equirectangular map [W/2, W, >= 3] (numpy or tensor)."""
    if resizeWidth is not None:
        raise NotImplementedError("getCoefficientsFromImage(resizeWidth=...) needs cv2's bicubic resize; resize the map first")
    if filterAmount is not None:
        raise NotImplementedError("getCoefficientsFromImage(filterAmount=...) needs scipy's gaussian_filter; blur the map first")
    img = torch.as_tensor(np.asarray(ibl) if not isinstance(ibl, torch.Tensor) else ibl)
    if img.shape[1] > 1000:
        raise ValueError(f"map width {img.shape[1]} > 1000: the reference silently resizes it to 1000 x 500 with cv2; "
                         "resize the map first")
    img = img[..., :3].to(_gpu(), torch.float32)
    return sh_project(img.unsqueeze(0), lmax)[0].cpu().numpy().astype(np.float64)


INTER_CUBIC, INTER_LANCZOS4 = 2, 4  # cv2's constants, as the reference passes them
_INTERPOLATION = {INTER_CUBIC: "bicubic", INTER_LANCZOS4: "lanczos4"}


def resizeImage(img, width, height, interpolation=INTER_CUBIC):
    """The map [H, W, C] or [H, W] (numpy or tensor) resampled to [height, width, C] float32 numpy on the GPU, with cv2's
    conventions for INTER_CUBIC (default) and INTER_LANCZOS4 on float images: half-pixel centres, replicated border, no
    antialiasing when shrinking (reni_amd/resample.py).  This is the "resize the map first" that getCoefficientsFromImage and
    getDiffuseMap ask for.  The reference's "max_pooling" option (skimage block_reduce) is not restated and raises."""
    if isinstance(interpolation, str):
        raise NotImplementedError(f"resizeImage(interpolation={interpolation!r}) is not supported; use INTER_CUBIC or INTER_LANCZOS4")
    if interpolation not in _INTERPOLATION:
        raise ValueError(f"interpolation must be INTER_CUBIC ({INTER_CUBIC}) or INTER_LANCZOS4 ({INTER_LANCZOS4}), got {interpolation!r}")
    t = torch.as_tensor(np.asarray(img) if not isinstance(img, torch.Tensor) else img)
    if t.dim() not in (2, 3):
        raise ValueError(f"img must be [H, W] or [H, W, C], got {tuple(t.shape)}")
    t = t.to(_gpu(), torch.float32)
    out = ops.resample(t, (int(height), int(width)), _INTERPOLATION[interpolation], layout="hwc" if t.dim() == 3 else "chw")
    return (out.permute(1, 2, 0) if t.dim() == 3 else out).contiguous().cpu().numpy()


def blurIBL(ibl, amount=5):
    """scipy.ndimage.gaussian_filter(channel, sigma=amount) of every channel of the map [H, W, C] (numpy or tensor), on the
    GPU: float32 numpy of the same shape.  This is the "blur the map first" that getCoefficientsFromImage asks for."""
    t = torch.as_tensor(np.asarray(ibl) if not isinstance(ibl, torch.Tensor) else ibl)
    if t.dim() != 3:
        raise ValueError(f"ibl must be [H, W, C], got {tuple(t.shape)}")
    t = t.to(_gpu(), torch.float32)
    return ops.gaussian_blur(t, float(amount), layout="hwc").cpu().numpy()


def shReconstructSignal(coeffs, sh_basis_matrix=None, width=600):
    """The map [width/2, width, 3] float32 of SH coefficients [T, 3]."""
    if sh_basis_matrix is not None:
        raise NotImplementedError("shReconstructSignal(sh_basis_matrix=...) is not supported; pass width instead")
    c = torch.as_tensor(np.asarray(coeffs) if not isinstance(coeffs, torch.Tensor) else coeffs)
    c = c.to(_gpu(), torch.float32)
    return sh_reconstruct(c.unsqueeze(0), width)[0].cpu().numpy()


def get_spherical_harmonic_representation(img, nBands):
    """The SH reconstruction of img [H, W, 3] with lmax = nBands (as the reference passes it), a float32 torch tensor."""
    coeffs = getCoefficientsFromImage(img, nBands)
    return torch.from_numpy(shReconstructSignal(coeffs, width=img.shape[1]))


# ----------------------------------------------------------------------------------------------- diffuse irradiance


def l_from_idx(idx):
    return int(np.sqrt(idx))


def getSolidAngle(y, width, is3D=False):
    """Solid angle of row y of a width x width / 2 map (the row centre's band)."""
    height = int(width / 2)
    pi2OverWidth = (np.pi * 2) / width
    piOverHeight = np.pi / height
    theta = (1.0 - ((y + 0.5) / height)) * np.pi
    return pi2OverWidth * (np.cos(theta - (piOverHeight / 2.0)) - np.cos(theta + (piOverHeight / 2.0)))


def getSolidAngleMap(width):
    height = int(width / 2)
    return np.repeat(getSolidAngle(np.arange(0, height), width)[:, np.newaxis], width, axis=1)


def xy2ll(x, y, width, height):
    """(latitude y pi / height, longitude x 2 pi / width) as an object array, like the reference."""
    return np.asarray([y / (float(height) / np.pi), x / (float(width) / (np.pi * 2))], dtype=object)


def spherical2Cartesian2(theta, phi):
    phi = phi + np.pi
    x = np.sin(theta) * np.cos(phi)
    y = np.cos(theta)
    z = np.sin(theta) * np.sin(phi)
    if not np.isscalar(x):
        y = np.repeat(y, x.shape[1], axis=1)
    return np.moveaxis(np.asarray([x, z, y]), 0, 2)


def getNormalMap(width):
    """[width / 2, width, 3] float64 normals at the pixels' top-left corners (the SH basis grid)."""
    height = int(width / 2)
    x = np.arange(0, width)
    y = np.arange(0, height).reshape(height, 1)
    latLon = xy2ll(x, y, width, height)
    return spherical2Cartesian2(latLon[0], latLon[1])


def getDiffuseCoefficients(lmax):
    """Ramamoorthi & Hanrahan's clamped-cosine band factors A_l / pi, l = 0..lmax, float64."""
    diffuseCoeffs = [np.pi, (2 * np.pi) / 3]
    for l in range(2, lmax + 1):
        if l % 2 == 0:
            a = (-1.0) ** ((l / 2.0) - 1.0)
            b = (l + 2.0) * (l - 1.0)
            c = float(math.factorial(l)) / (2**l * math.factorial(l // 2) ** 2)
            diffuseCoeffs.append(2 * np.pi * (a / b) * c)
        else:
            diffuseCoeffs.append(0)
    return np.asarray(diffuseCoeffs) / np.pi


def findWindowingFactor(coeffs, maxLaplacian=10.0):
    """Sloan's windowing factor (http://www.ppsloan.org/publications/StupidSH36.pdf) by Newton's method, as the reference
    computes it: m in range(-1, l + 1), the plain mean of the coefficients, at most 1e7 iterations."""
    coeffs = np.asarray(coeffs)
    lmax = sh_lmax_from_terms(coeffs.shape[0])
    tableL = np.zeros((lmax + 1))
    tableB = np.zeros((lmax + 1))
    for l in range(1, lmax + 1):
        tableL[l] = float((l * l) * ((l + 1) * (l + 1)))
        B = 0.0
        for m in range(-1, l + 1):
            B += np.mean(coeffs[shIndex(l, m), :])
        tableB[l] = B
    squaredLaplacian = 0.0
    for l in range(1, lmax + 1):
        squaredLaplacian += tableL[l] * tableB[l]
    targetSquaredLaplacian = maxLaplacian * maxLaplacian
    if squaredLaplacian <= targetSquaredLaplacian:
        return 0.0
    windowingFactor = 0.0
    for _ in range(0, 10000000):
        f = 0.0
        fd = 0.0
        for l in range(1, lmax + 1):
            f += tableL[l] * tableB[l] / ((1.0 + windowingFactor * tableL[l]) * (1.0 + windowingFactor * tableL[l]))
            d = 1.0 + windowingFactor * tableL[l]
            fd += (2.0 * (tableL[l] * tableL[l]) * tableB[l]) / (d * d * d)
        f = targetSquaredLaplacian - f
        delta = -f / fd
        windowingFactor += delta
        if abs(delta) < 0.0000001:
            break
    return windowingFactor


def applyWindowing(coeffs, windowingFactor=None, verbose=False):
    """Scales band l of coeffs [T, 3] by 1 / (1 + f l^2 (l + 1)^2) in place (f <= 0: unchanged) and returns it."""
    lmax = sh_lmax_from_terms(coeffs.shape[0])
    if windowingFactor is None:
        windowingFactor = findWindowingFactor(coeffs)
    if windowingFactor <= 0:
        if verbose:
            print("No windowing applied")
        return coeffs
    if verbose:
        print("Using windowingFactor: %s" % (windowingFactor))
    for l in range(0, lmax + 1):
        s = 1.0 / (1.0 + windowingFactor * l * l * (l + 1.0) * (l + 1.0))
        for m in range(-l, l + 1):
            coeffs[shIndex(l, m), :] *= s
    return coeffs


def diffuse_map_tables(width, widthLowRes):
    """getDiffuseMap's grid in float64: (in_dirs [H W, 3], in_weight [H W] (the row's solid angle), out_dirs [hL wL, 3]).
    Pixel (x, y) looks along (cos phi sin theta, sin phi, cos phi cos theta), phi = pi ((1 - y / H) - 0.5),
    theta = 2 pi (1 - x / W); output pixel (x, y) along input pixel (int(x / wL W), int(y / hL H))."""
    width, widthLowRes = int(width), int(widthLowRes)
    height, heightLowRes = int(width / 2), int(widthLowRes / 2)
    uv_x = np.tile(np.arange(float(width)) / width, (height, 1))
    uv_y = 1 - np.tile(np.arange(float(height)) / height, (width, 1)).transpose()
    phi = np.pi * (uv_y - 0.5)
    theta = 2 * np.pi * (1 - uv_x)
    cos_phi = np.cos(phi)
    d = np.stack([cos_phi * np.sin(theta), np.sin(phi), cos_phi * np.cos(theta)], -1)  # [H, W, 3]
    xs = [int((float(x) / widthLowRes) * width) for x in range(widthLowRes)]
    ys = [int((float(y) / heightLowRes) * height) for y in range(heightLowRes)]
    out = d[np.asarray(ys)[:, None], np.asarray(xs)[None, :]]
    return d.reshape(-1, 3), getSolidAngleMap(width).reshape(-1), out.reshape(-1, 3)


def reni_grid_weights(width):
    """The exact band solid angles of RENI's width x width / 2 grid, [H W] float64: row k covers polar angles
    [k pi / H, (k + 1) pi / H], so each pixel gets (2 pi / W)(cos(k pi / H) - cos((k + 1) pi / H))."""
    W = int(width)
    H = W // 2
    k = np.arange(H, dtype=np.float64)
    band = (2 * np.pi / W) * (np.cos(k * np.pi / H) - np.cos((k + 1) * np.pi / H))
    return np.repeat(band, W)


_DTABLES = {}


def _diffuse_device_tables(key, make, device):
    key = key + (str(device),)
    if key not in _DTABLES:
        _DTABLES[key] = tuple(torch.as_tensor(np.asarray(t, np.float32) if isinstance(t, np.ndarray) else t)
                              .to(device, torch.float32).contiguous() for t in make())
    return _DTABLES[key]


def diffuse_convolve(src: torch.Tensor, in_dirs: torch.Tensor, in_weight: torch.Tensor, out_dirs: torch.Tensor,
                     scale: float = 1.0 / np.pi) -> torch.Tensor:
    """E[n, o, c] = scale sum_i max(0, out_dirs[o] . in_dirs[i]) in_weight[i] src[n, i, c] on the GPU, without a [P, Q]
    tensor.  src [N, Q, 3] or channel-planar [N, 3, Q] (any strides); in_dirs [Q, 3], in_weight [Q], out_dirs [P, 3]
    -> [N, P, 3] float32."""
    return ops.diffuse_convolve(src, in_dirs, in_weight, out_dirs, scale)


def irradiance_map(envmaps: torch.Tensor, out_width=None) -> torch.Tensor:
    """Diffuse irradiance (/ pi: a constant map of 1 gives 1) of maps on RENI's own grid (reni_amd.utils.get_directions):
    envmaps [N, H W, 3] or [N, H, W, 3] on the GPU -> the same layout at out_width (default: the input width)."""
    from .utils import get_directions
    if envmaps.dim() == 4 and envmaps.shape[3] == 3 and 2 * envmaps.shape[1] == envmaps.shape[2]:
        W = int(envmaps.shape[2])
        src = envmaps.reshape(envmaps.shape[0], -1, 3)
    elif envmaps.dim() == 3 and envmaps.shape[2] == 3:
        W = int(round(math.sqrt(2 * envmaps.shape[1])))
        if W * (W // 2) != envmaps.shape[1] or W % 2:
            raise ValueError(f"[N, H W, 3] maps need H W = W^2 / 2 for an even W, got {envmaps.shape[1]} pixels")
        src = envmaps
    else:
        raise ValueError(f"envmaps must be [N, H W, 3] or [N, W/2, W, 3], got {tuple(envmaps.shape)}")
    Wo = W if out_width is None else int(out_width)
    if Wo < 2 or Wo % 2:
        raise ValueError(f"out_width must be even and >= 2, got {out_width}")
    ops._require_cuda(envmaps)
    dirs, w = _diffuse_device_tables(("reni", W), lambda: (get_directions(W)[0], reni_grid_weights(W)), envmaps.device)
    (odirs,) = _diffuse_device_tables(("reni_out", Wo), lambda: (get_directions(Wo)[0],), envmaps.device)
    out = ops.diffuse_convolve(src, dirs, w, odirs, 1.0 / np.pi)
    return out.view(envmaps.shape[0], Wo // 2, Wo, 3) if envmaps.dim() == 4 else out


def sh_irradiance(coeffs: torch.Tensor, width: int) -> torch.Tensor:
    """shReconstructDiffuseMap for a batch: coeffs [N, T, 3] on the GPU -> [N, width / 2, width, 3] float32; the L2
    closed form (shRenderL2) when T == 9, otherwise shRender (the SH reconstruction of the coefficients scaled by
    getDiffuseCoefficients)."""
    if coeffs.dim() != 3 or coeffs.shape[2] != 3:
        raise ValueError(f"coeffs must be [N, T, 3], got {tuple(coeffs.shape)}")
    lmax = sh_lmax_from_terms(coeffs.shape[1])
    if shTerms(lmax) != coeffs.shape[1]:
        raise ValueError(f"the number of SH terms must be a square, got {coeffs.shape[1]}")
    _check_sh(width, lmax)
    ops._require_cuda(coeffs)
    W = int(width)
    if coeffs.shape[1] == 9:
        (nrm,) = _diffuse_device_tables(("normals", W), lambda: (getNormalMap(W).reshape(-1, 3),), coeffs.device)
        return ops.sh_irradiance_l2(coeffs, nrm).view(coeffs.shape[0], W // 2, W, 3)
    (band,) = _diffuse_device_tables(("band", lmax), lambda: (_band_scale(lmax),), coeffs.device)
    return sh_reconstruct(coeffs * band.view(1, -1, 1), W)


def _band_scale(lmax):
    """getDiffuseCoefficients(lmax)[l] per term t, float64"""
    d = getDiffuseCoefficients(lmax)
    return np.asarray([d[l_from_idx(t)] for t in range(shTerms(lmax))])


def _host_coeffs(iblCoeffs):
    c = iblCoeffs.detach().cpu().numpy() if isinstance(iblCoeffs, torch.Tensor) else np.asarray(iblCoeffs)
    return c.astype(np.float64)


def shRender(iblCoeffs, width=600):
    """Diffuse render [width / 2, width, 3] (float64 array of the float32 result) of SH coefficients [T, 3]: the
    reconstruction of the coefficients scaled by getDiffuseCoefficients(lmax)[l] on the host."""
    c = _host_coeffs(iblCoeffs)
    lmax = sh_lmax_from_terms(c.shape[0])
    scaled = torch.from_numpy((c * _band_scale(lmax)[:, None]).astype(np.float32))
    return sh_reconstruct(scaled.to(_gpu()).unsqueeze(0), width)[0].cpu().numpy().astype(np.float64)


def shRenderL2(iblCoeffs, normalMap):
    """shRenderL2 of coefficients [9+, 3] at normals [..., 3] -> [..., 3] (float64 array of the float32 result)."""
    c = _host_coeffs(iblCoeffs)[:9]
    n = normalMap.detach() if isinstance(normalMap, torch.Tensor) else torch.from_numpy(np.asarray(normalMap, np.float64))
    shape = tuple(n.shape)
    if shape[-1] != 3:
        raise ValueError(f"normalMap must be [..., 3], got {shape}")
    dev = _gpu()
    out = ops.sh_irradiance_l2(torch.from_numpy(c.astype(np.float32)).to(dev).unsqueeze(0),
                               n.reshape(-1, 3).to(dev, torch.float32))
    return out[0].cpu().numpy().astype(np.float64).reshape(shape)


def shReconstructDiffuseMap(iblCoeffs, width=600):
    """The diffuse map [width / 2, width, 3] float32 of SH coefficients [T, 3]: shRenderL2 on getNormalMap(width) when
    T == 9, shRender otherwise."""
    c = _host_coeffs(iblCoeffs)
    if c.shape[0] == 9:
        return shRenderL2(c, getNormalMap(width)).astype(np.float32)
    return shRender(c, width).astype(np.float32)


def shReconstructDiffuseNormalMap(iblCoeffs, normal_map):
    return shRenderL2(iblCoeffs, normal_map).astype(np.float32)


def _read_ibl(ibl):
    if isinstance(ibl, (str, bytes, os.PathLike)):
        from .exr import read_exr
        return torch.from_numpy(np.ascontiguousarray(read_exr(ibl)))
    return ibl if isinstance(ibl, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ibl))


def getDiffuseMap(ibl_name, width=600, widthLowRes=32, outputWidth=None):
    """The ground-truth diffuse map [widthLowRes / 2, widthLowRes, 3] float32 of an equirectangular map [width / 2, width,
    >= 3] (array, tensor or EXR path): the brute-force clamped-cosine convolution / pi on getDiffuseMap's own grid."""
    if outputWidth is None:
        outputWidth = width
    height = int(width / 2)
    img = _read_ibl(ibl_name)
    if img.dim() != 3 or img.shape[2] < 3:
        raise ValueError(f"the map must be [H, W, >= 3], got {tuple(img.shape)}")
    if tuple(img.shape[:2]) != (height, width):
        raise NotImplementedError(f"getDiffuseMap resizes a {tuple(img.shape[:2])} map to ({height}, {width}) with cv2's "
                                  "bicubic resize; resize the map first")
    if widthLowRes < outputWidth:
        raise NotImplementedError(f"getDiffuseMap upsamples the {widthLowRes}-wide result to {outputWidth} with cv2's "
                                  "Lanczos resize; pass outputWidth=widthLowRes")
    dev = _gpu()
    dirs, w, odirs = _diffuse_device_tables(("ref", int(width), int(widthLowRes)),
                                            lambda: diffuse_map_tables(width, widthLowRes), dev)
    src = img[..., :3].to(dev, torch.float32).reshape(1, -1, 3)
    out = ops.diffuse_convolve(src, dirs, w, odirs, 1.0 / np.pi)
    return out.view(int(widthLowRes / 2), int(widthLowRes), 3).cpu().numpy()
