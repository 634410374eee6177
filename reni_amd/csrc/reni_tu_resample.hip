// translation unit of libreni_hip.so: image resampling and Gaussian blur, the device side of the resident dataset
// (reni_amd/data.py: ResidentDataset) and of baselines.resizeImage / blurIBL.
//
// Reference: torchvision Resize (bilinear, src/data/datasets.py via custom_transforms), get_mask's NEAREST (src/utils/utils.py:81-91),
// cv2.resize INTER_CUBIC / INTER_LANCZOS4 (src/models/spherical_harmonics.py:274-279) and scipy.ndimage.gaussian_filter
// (blurIBL :564-569).  fp32 throughout, no atomics: every sum runs in a fixed order that depends on the tap counts only, so two
// calls give identical bits and an image's result does not depend on the batch around it.
//
//   k_resample       out[n][c][y][x] = sum_j row_w[y][j] ( sum_k col_w[x][k] src(n, c, row_idx[y][j], col_idx[x][k]) ): a separable
//                    gather through host-built tables.  The kernel knows no interpolation mode: every coordinate and weight was
//                    computed on the host in float64 / exact integers and rounded to fp32 once (reni_amd/resample.py), as the
//                    separable SH tables are.  One thread per output pixel, (c, n) on the grid; the inner sum is an fmaf chain
//                    over k ascending from 0, the outer one over j ascending from 0.
//   k_blur_axis      one axis of scipy's separable gaussian_filter with the `reflect` boundary (d c b a | a b c d | d c b a,
//                    period 2 n, so a radius beyond the image still works): an fmaf chain over the 2 r + 1 taps, ascending.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#define DEV __device__ __forceinline__

namespace reni {

struct RsArgs {
  const float* src;  // element (n, c, y, x) at src[n sn + c sc + y sy + x sx]
  int64_t sn, sc, sy, sx;
  float* out;  // [N][C][Hd][Wd]
  const int* row_idx;  // [Hd][ty]
  const float* row_w;  // [Hd][ty]
  const int* col_idx;  // [Wd][tx]
  const float* col_w;  // [Wd][tx]
  int Hs, Ws, Hd, Wd, ty, tx;
};

// TX > 0: the column taps are held in registers; TX == 0: any 1 <= tx <= 8, read per row.  Same fmaf order either way.  The
// register instances are what the four modes use: where the work is large the per-row table reads of the generic instance
// cost 2 x (bilinear to 2048 x 4096, bicubic 4096 x 2048 -> 1000 x 500) to 10 x (Lanczos 32 x 16 -> 600 x 300), DESIGN 4.6b.
template <int TX>
__global__ void __launch_bounds__(256) k_resample(const RsArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;  // Hd Wd < 2^30
  if (p >= a.Hd * a.Wd) return;
  const int y = p / a.Wd, x = p - y * a.Wd;
  const float* base = a.src + (int64_t)blockIdx.z * a.sn + (int64_t)blockIdx.y * a.sc;
  const int tx = TX > 0 ? TX : a.tx;
  const int* ci = a.col_idx + (int64_t)x * tx;
  const float* cw = a.col_w + (int64_t)x * tx;
  const int* ri = a.row_idx + (int64_t)y * a.ty;
  const float* rw = a.row_w + (int64_t)y * a.ty;
  int64_t coff[TX > 0 ? TX : 1];
  float cwv[TX > 0 ? TX : 1];
  if (TX > 0) {
#pragma unroll
    for (int k = 0; k < TX; ++k) {
      coff[k] = (int64_t)min(max(ci[k], 0), a.Ws - 1) * a.sx;  // (a table is trusted for weights, never for addresses)
      cwv[k] = cw[k];
    }
  }
  float acc = 0.f;
  for (int j = 0; j < a.ty; ++j) {
    const float* row = base + (int64_t)min(max(ri[j], 0), a.Hs - 1) * a.sy;
    float s = 0.f;
    if (TX > 0) {
#pragma unroll
      for (int k = 0; k < TX; ++k) s = fmaf(cwv[k], row[coff[k]], s);
    } else {
      for (int k = 0; k < tx; ++k) s = fmaf(cw[k], row[(int64_t)min(max(ci[k], 0), a.Ws - 1) * a.sx], s);
    }
    acc = fmaf(rw[j], s, acc);
  }
  a.out[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * a.Hd * a.Wd + p] = acc;
}

DEV int reflect_index(int i, int n) {  // scipy's `reflect`: period 2 n, the edge sample is repeated
  const int per = 2 * n;
  int m = i % per;
  if (m < 0) m += per;
  return m < n ? m : per - 1 - m;
}

// one axis of the blur: element (c, y, x) of in at c ic + y iy + x ix, of out at c oc + y oy + x ox; axis 0 runs along y
__global__ void __launch_bounds__(256) k_blur_axis(const float* __restrict__ in, int64_t ic, int64_t iy, int64_t ix,
                                                   float* __restrict__ out, int64_t oc, int64_t oy, int64_t ox, int H, int W,
                                                   int axis, const float* __restrict__ w, int radius) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const float* base = in + (int64_t)blockIdx.y * ic;
  float s = 0.f;
  if (axis == 0) {
    base += (int64_t)x * ix;
    for (int t = -radius; t <= radius; ++t) s = fmaf(w[t + radius], base[(int64_t)reflect_index(y + t, H) * iy], s);
  } else {
    base += (int64_t)y * iy;
    for (int t = -radius; t <= radius; ++t) s = fmaf(w[t + radius], base[(int64_t)reflect_index(x + t, W) * ix], s);
  }
  out[(int64_t)blockIdx.y * oc + (int64_t)y * oy + (int64_t)x * ox] = s;
}

}  // namespace reni

namespace {

using reni::reni_set_error;
constexpr int64_t RS_MAX_PIXELS = 0x3fffffff;
constexpr int64_t RS_MAX_RADIUS = 1 << 20;

bool blur_shape_ok(int64_t C, int64_t H, int64_t W) {
  return C >= 1 && C <= 65535 && H >= 1 && W >= 1 && H <= RS_MAX_PIXELS / W && C <= RS_MAX_PIXELS / (H * W);
}

}  // namespace

extern "C" {

int reni_resample(int64_t N, int64_t C, int64_t Hs, int64_t Ws, int64_t Hd, int64_t Wd, const float* src,
                  const int64_t src_strides[4], const int32_t* row_idx, const float* row_w, int32_t row_taps,
                  const int32_t* col_idx, const float* col_w, int32_t col_taps, float* out, void* stream) {
  if (N < 1 || C < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return reni_set_error(RENI_EINVAL, "resample: sizes must be >= 1");
  if (N > 65535 || C > 65535 || Hs > RS_MAX_PIXELS / Ws || Hd > RS_MAX_PIXELS / Wd || N * C > RS_MAX_PIXELS / (Hd * Wd))
    return reni_set_error(RENI_EINVAL, "resample: need N, C <= 65535, Hs Ws < 2^30 and N C Hd Wd < 2^30");
  if (row_taps < 1 || row_taps > 8 || col_taps < 1 || col_taps > 8)
    return reni_set_error(RENI_EINVAL, "resample: taps per axis must be 1..8");
  if (!src || !src_strides || !row_idx || !row_w || !col_idx || !col_w || !out)
    return reni_set_error(RENI_EINVAL, "resample: NULL argument");
  if (int rc = tu_check_strides("resample", "src strides", src_strides, 4)) return rc;
  reni::RsArgs a = {};
  a.src = src; a.sn = src_strides[0]; a.sc = src_strides[1]; a.sy = src_strides[2]; a.sx = src_strides[3];
  a.out = out; a.row_idx = row_idx; a.row_w = row_w; a.col_idx = col_idx; a.col_w = col_w;
  a.Hs = (int)Hs; a.Ws = (int)Ws; a.Hd = (int)Hd; a.Wd = (int)Wd; a.ty = row_taps; a.tx = col_taps;
  const dim3 grid((unsigned)((Hd * Wd + 255) / 256), (unsigned)C, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  switch (col_taps) {
    case 1: return tu_launch(TU_PLAIN, reni::k_resample<1>, grid, dim3(256), 0, s, a);
    case 2: return tu_launch(TU_PLAIN, reni::k_resample<2>, grid, dim3(256), 0, s, a);
    case 4: return tu_launch(TU_PLAIN, reni::k_resample<4>, grid, dim3(256), 0, s, a);
    case 8: return tu_launch(TU_PLAIN, reni::k_resample<8>, grid, dim3(256), 0, s, a);
    default: return tu_launch(TU_PLAIN, reni::k_resample<0>, grid, dim3(256), 0, s, a);
  }
}

size_t reni_blur_workspace_bytes(int64_t C, int64_t H, int64_t W) {
  if (!blur_shape_ok(C, H, W)) return 0;
  return (size_t)C * H * W * sizeof(float) + 256;
}

int reni_gaussian_blur(int64_t C, int64_t H, int64_t W, const float* src, const int64_t strides[3], const float* weights,
                       int32_t radius, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!blur_shape_ok(C, H, W)) return reni_set_error(RENI_EINVAL, "blur: need C, H, W >= 1, C <= 65535 and C H W < 2^30");
  if (radius < 0 || radius > RS_MAX_RADIUS) return reni_set_error(RENI_EINVAL, "blur: radius must be 0..2^20");
  if (!src || !strides || !weights || !out) return reni_set_error(RENI_EINVAL, "blur: NULL argument");
  if (int rc = tu_check_strides("blur", "strides", strides, 3)) return rc;
  if (int rc = tu_check_ws("blur", ws, ws_bytes, (size_t)C * H * W * sizeof(float))) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* mid = (float*)ws;  // [C][H][W]
  const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)C);
  if (int rc = tu_launch(TU_PLAIN, reni::k_blur_axis, grid, dim3(256), 0, s, src, strides[0], strides[1], strides[2], mid, H * W, W,
                         (int64_t)1, (int)H, (int)W, 0, weights, (int)radius))
    return rc;
  return tu_launch(TU_PLAIN, reni::k_blur_axis, grid, dim3(256), 0, s, mid, H * W, W, (int64_t)1, out, strides[0], strides[1],
                   strides[2], (int)H, (int)W, 1, weights, (int)radius);
}

}  // extern "C"
