// translation unit of libreni_hip.so: rotation of equirectangular environment maps (reni_amd/rotation.py, the rotation
// augmentation of reni_amd/data.py: ResidentDataset).  No reference counterpart: the reference rotates latents only.
//
//   k_rotate_envmap  out[b](d) = src[b](R_b^T d) for every pixel direction d of the H x W grid (utils.get_directions when W = 2 H):
//                    one lane per output pixel computes the source coordinate ONCE and serves all C channels with it; consecutive
//                    lanes are consecutive columns (coalesced stores, a wave's gathers fall into a few source rows).
//
// The chain of one pixel, fp32, every operation written out (contraction is off for the whole unit, so what is written is what
// runs):
//     d   = (sp st, cp, -(sp ct))                        sp, cp = row_trig[r], st, ct = col_trig[c]: host tables, float64 -> fp32
//     s_j = fma(R[2][j], d.z, fma(R[1][j], d.y, R[0][j] d.x))                                                       (s = R^T d)
//     phi = atan2f(sqrtf(fma(s.z, s.z, s.x s.x)), s.y)   theta = atan2f(s.x, -s.z)
//     row = fma(phi, fp32(H / pi), -1/2)                 col = fma(theta, fp32(W / 2 pi), W/2 - 1/2)
// then the taps of the sphere (a row beyond a pole is the same row seen from the other side: column + W/2; columns modulo W):
//     bilinear  i = floor(row), fr = row - i (exact), likewise j, fc;  top = fma(fc, t01, (1 - fc) t00), bot likewise,
//               out = fma(fr, bot, (1 - fr) top)
//     nearest   the tap at floor(row + 1/2), floor(col + 1/2)
// This is the one place where the project's rule "everything that decides a result is computed on the host in float64"
// (reni_amd/resample.py) does not hold: a fresh rotation per image and step would make host tables the bottleneck.  Only the
// trigonometry of the OUTPUT grid is tabulated; sqrtf and two atan2f per pixel run on the device and are amortised over
// C x taps loads.  The error this costs is bounded in tests/test_rotate_cpu.py (rotate_bound) from the chain above.
// No atomics, no workspace, nothing but the launch on the stream: two calls give identical bits, and an image's result does
// not depend on the batch around it or on how it is addressed (strides, src_index).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#include "reni_sphere.inc"  // direction -> (row, col), the taps and the three constants: shared with the lookup (reni_tu_glossy.hip)

namespace reni {

struct RotArgs {
  const float* src;  // element (n, c, y, x) at src[n sn + c sc + y sy + x sx]
  int64_t sn, sc;
  int sy, sx;  // (< 2^31, checked: index x stride is then one 32 x 32 -> 64 bit multiply instead of a 64-bit product per tap)
  const int64_t* src_index;  // optional [B]
  int64_t n_src;
  const float* rot;  // image b's R at rot + b rot_stride, row-major
  int64_t rot_stride;
  const float* row_trig;  // [H][2]
  const float* col_trig;  // [W][2]
  float* out;  // [B][C][H][W]
  int C, H, W;
  float row_scale, col_scale, col_bias;  // fp32(H / pi), fp32(W / 2 pi), W/2 - 1/2
};

template <bool BILINEAR>
__global__ void __launch_bounds__(256) k_rotate_envmap(const RotArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;  // H W < 2^30
  if (p >= a.H * a.W) return;
  const int r = p / a.W, c = p - r * a.W;
  const int b = (int)blockIdx.y;
  const float* R = a.rot + (int64_t)b * a.rot_stride;
  const float sp = a.row_trig[2 * r], cp = a.row_trig[2 * r + 1];
  const float st = a.col_trig[2 * c], ct = a.col_trig[2 * c + 1];
  const float dx = sp * st, dy = cp, dz = -(sp * ct);
  const float sx = fmaf(R[6], dz, fmaf(R[3], dy, R[0] * dx));
  const float sy = fmaf(R[7], dz, fmaf(R[4], dy, R[1] * dx));
  const float sz = fmaf(R[8], dz, fmaf(R[5], dy, R[2] * dx));
  float row, col;
  sph_rowcol(sx, sy, sz, a.H, a.W, a.row_scale, a.col_scale, a.col_bias, row, col);
  int64_t n = b;
  if (a.src_index) n = min(max(a.src_index[b], (int64_t)0), a.n_src - 1);
  const float* base = a.src + n * a.sn;
  float* o = a.out + (int64_t)b * a.C * a.H * a.W + p;
  if (BILINEAR) {
    const SphTaps t = sph_taps(row, col, a.H, a.W);
    const float fr = t.fr, gr = t.gr, fc = t.fc, gc = t.gc;
    const int64_t r0 = (int64_t)t.i0 * (int64_t)a.sy, r1 = (int64_t)t.i1 * (int64_t)a.sy;
    const int64_t o00 = r0 + (int64_t)t.j00 * (int64_t)a.sx, o01 = r0 + (int64_t)t.j01 * (int64_t)a.sx;
    const int64_t o10 = r1 + (int64_t)t.j10 * (int64_t)a.sx, o11 = r1 + (int64_t)t.j11 * (int64_t)a.sx;
    for (int ch = 0; ch < a.C; ++ch, base += a.sc, o += (int64_t)a.H * a.W) {
      const float top = fmaf(fc, base[o01], gc * base[o00]);
      const float bot = fmaf(fc, base[o11], gc * base[o10]);
      *o = fmaf(fr, bot, gr * top);
    }
  } else {
    const SphTaps t = sph_taps(row + 0.5f, col + 0.5f, a.H, a.W);  // the one-tap case: its first tap
    const int64_t o00 = (int64_t)t.i0 * (int64_t)a.sy + (int64_t)t.j00 * (int64_t)a.sx;
    for (int ch = 0; ch < a.C; ++ch, base += a.sc, o += (int64_t)a.H * a.W) *o = base[o00];
  }
}

}  // namespace reni

extern "C" int reni_rotate_envmap(int64_t B, int64_t C, int64_t H, int64_t W, const float* src, const int64_t src_strides[4],
                                  const int64_t* src_index, int64_t n_src, const float* rot, int64_t rot_stride,
                                  const float* row_trig, const float* col_trig, int32_t mode, float* out, void* stream) {
  using reni::reni_set_error;
  if (B < 1 || C < 1 || H < 1 || W < 1) return reni_set_error(RENI_EINVAL, "rotate: sizes must be >= 1");
  if (W & 1) return reni_set_error(RENI_EINVAL, "rotate: W must be even (the far side of a pole is W / 2 columns away)");
  if (B > 65535 || C > 65535 || H > 0x3fffffff / W) return reni_set_error(RENI_EINVAL, "rotate: need B, C <= 65535 and H W < 2^30");
  if (!src || !src_strides || !rot || !row_trig || !col_trig || !out) return reni_set_error(RENI_EINVAL, "rotate: NULL argument");
  if (int rc = tu_check_strides("rotate", "src strides", src_strides, 4)) return rc;
  if (src_strides[2] > 0x7fffffff || src_strides[3] > 0x7fffffff)
    return reni_set_error(RENI_EINVAL, "rotate: the row and column strides must be < 2^31 elements");
  if (rot_stride != 0 && rot_stride != 9) return reni_set_error(RENI_EINVAL, "rotate: rot_stride must be 9 (per image) or 0 (shared)");
  if (mode != RENI_ROTATE_NEAREST && mode != RENI_ROTATE_BILINEAR) return reni_set_error(RENI_EINVAL, "rotate: unknown mode");
  if (src_index && n_src < 1) return reni_set_error(RENI_EINVAL, "rotate: src_index needs n_src >= 1");
  reni::RotArgs a = {};
  a.src = src; a.sn = src_strides[0]; a.sc = src_strides[1]; a.sy = (int)src_strides[2]; a.sx = (int)src_strides[3];
  a.src_index = src_index; a.n_src = n_src; a.rot = rot; a.rot_stride = rot_stride;
  a.row_trig = row_trig; a.col_trig = col_trig; a.out = out;
  a.C = (int)C; a.H = (int)H; a.W = (int)W;
  sph_scales(H, W, a.row_scale, a.col_scale, a.col_bias);
  const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  const auto k = mode == RENI_ROTATE_BILINEAR ? reni::k_rotate_envmap<true> : reni::k_rotate_envmap<false>;
  return tu_launch(TU_PLAIN, k, grid, dim3(256), 0, s, a);
}
