// translation unit of libreni_hip.so: scores of environment-map pairs (reni_amd/metrics.py) -- weighted error sums and SSIM.
// No reference counterpart: the reference's evaluation notebooks compose these from tensor operations.
//
//   k_pair_stats   one pass over a (prediction, target) pair: every pixel is read once through the caller's strides, mapped into
//                  the call's space IN REGISTERS (reni_dev_image.inc: the expressions reni_unnormalise_srgb writes out), and folded
//                  into eight per-image quantities (include/reni_hip.h lists them).  A workgroup owns PS_CHUNK consecutive pixels
//                  of one image; a thread adds its PS_PPT pixels in pixel order, the 64 lanes of a wave combine in a butterfly, the
//                  four waves in wave order: the partial of a workgroup is a function of (H, W) and the pixels alone.
//   k_ssim         mean SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5) of one 32 x 32 tile of one image.  Per
//                  channel: the tile plus a halo of 5 of BOTH images goes to LDS already mapped (on the sphere: columns wrap, a row
//                  beyond a pole is the same row seen from the other side, the rule of reni_rotate_envmap); a horizontal pass
//                  forms the five windowed moments p, t, p^2, t^2, p t of every row; a vertical pass finishes them for four output
//                  rows per thread and turns them into the SSIM value, which goes straight into the thread's sum.  No moment
//                  image leaves the chip.  LDS: 2 x 42 x 42 + 5 x 42 x 32 floats = 41 KB, three workgroups per CU.
//                  Both passes address LDS with consecutive lanes on consecutive dwords (lanes 0..31 one row, 32..63 the next):
//                  no bank conflicts without padding.
//   k_finish       the partials of one image, added in DOUBLE in a fixed order (eight interleaved strands, then the strands in
//                  order) and rounded to fp32 once.
// fp32 on the device, no float atomics, no host synchronisation, launches on `stream` only: two calls give identical bits, and an
// image's result does not depend on the batch around it or on how it is addressed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_dev_image.inc"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__

namespace reni {

constexpr int PS_PPT = 8;                // pixels per thread
constexpr int PS_CHUNK = 256 * PS_PPT;   // pixels per workgroup
constexpr int SS_T = 32;                 // output tile (rows and columns)
constexpr int SS_R = 5;                  // window radius
constexpr int SS_IN = SS_T + 2 * SS_R;   // tile plus halo
constexpr int SS_ROWS = 4;               // output rows per thread in the vertical pass

struct PairImg {
  const float* p;  // element (b, c, h, w) at p[b s[0] + c s[1] + h s[2] + w s[3]]
  int64_t s[4];
};

struct MetArgs {
  PairImg pred, target;
  const float* weight;  // element (b, h, w) at weight[b ws[0] + h ws[1] + w ws[2]]; NULL: 1
  int64_t ws[3];
  const float* exposure;  // [B], RENI_SPACE_SRGB only
  float range, m0;        // (float)(m1 - m0), (float)m0
  int H, W;
  int nblk;      // workgroups (partials) per image
  float* part;   // [B][nblk][NE]
  // SSIM
  int planar, tiles_x;
  float g[2 * SS_R + 1];
  float C1, C2;
  float* map_out;  // [B][H][W] or NULL
};

template <int SPACE>
DEV float map_value(float x, float range, float m0, float q) {
  if (SPACE == RENI_SPACE_STORED) return x;
  const float y = img_unnormalise(x, range, m0);
  if (SPACE == RENI_SPACE_LINEAR) return y;
  return img_srgb(y, q);
}

DEV float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
DEV float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}
DEV float wave_min(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
  return v;
}

template <int SPACE>
__global__ void __launch_bounds__(256) k_pair_stats(const MetArgs a) {
  __shared__ float red[4][8];
  const int b = (int)blockIdx.y;
  const int npix = a.H * a.W;
  const float q = SPACE == RENI_SPACE_SRGB ? a.exposure[b] : 1.f;
  const float* pb = a.pred.p + (int64_t)b * a.pred.s[0];
  const float* tb = a.target.p + (int64_t)b * a.target.s[0];
  const float* wb = a.weight ? a.weight + (int64_t)b * a.ws[0] : nullptr;
  float s_w = 0.f, s_se = 0.f, s_ae = 0.f, s_cos = 0.f, s_t2 = 0.f, s_t1 = 0.f;
  float t_max = -INFINITY, t_min = INFINITY;
  // every load of the thread's PS_PPT pixels is issued before the first value is used (a pixel beyond the image re-reads the last one
  // with weight 0)
  float xp[PS_PPT][3], xt[PS_PPT][3], xw[PS_PPT];
#pragma unroll
  for (int k = 0; k < PS_PPT; ++k) {
    const int at = (int)blockIdx.x * PS_CHUNK + k * 256 + (int)threadIdx.x;  // H W < 2^30
    const int pix = min(at, npix - 1);
    const int h = pix / a.W, w = pix - h * a.W;
    const float* pp = pb + (int64_t)h * a.pred.s[2] + (int64_t)w * a.pred.s[3];
    const float* tp = tb + (int64_t)h * a.target.s[2] + (int64_t)w * a.target.s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xp[k][c] = pp[c * a.pred.s[1]];
      xt[k][c] = tp[c * a.target.s[1]];
    }
    const float wt = wb ? wb[(int64_t)h * a.ws[1] + (int64_t)w * a.ws[2]] : 1.f;
    xw[k] = at < npix ? wt : 0.f;
  }
#pragma unroll
  for (int k = 0; k < PS_PPT; ++k) {
    const float wt = xw[k];
    float se = 0.f, ae = 0.f, t2 = 0.f, t1 = 0.f, pt = 0.f, p2 = 0.f, tmx = -INFINITY, tmn = INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p = map_value<SPACE>(xp[k][c], a.range, a.m0, q);
      const float t = map_value<SPACE>(xt[k][c], a.range, a.m0, q);
      const float d = p - t;
      se = fmaf(d, d, se);
      ae += fabsf(d);
      t2 = fmaf(t, t, t2);
      t1 += t;
      pt = fmaf(p, t, pt);
      p2 = fmaf(p, p, p2);
      tmx = fmaxf(tmx, t);
      tmn = fminf(tmn, t);
    }
    // F.cosine_similarity(dim = channel, eps = 1e-20): each norm is held at eps or above
    const float cs = pt / (fmaxf(sqrtf(p2), 1e-20f) * fmaxf(sqrtf(t2), 1e-20f));
    if (wt != 0.f) {  // a pixel of weight 0 is not there: whatever it holds (an overflow, a NaN) stays out of every entry
      s_w += wt;
      s_se = fmaf(wt, se, s_se);
      s_ae = fmaf(wt, ae, s_ae);
      s_cos = fmaf(wt, cs, s_cos);
      s_t2 = fmaf(wt, t2, s_t2);
      s_t1 = fmaf(wt, t1, s_t1);
    }
    if (wt > 0.f) {
      t_max = fmaxf(t_max, tmx);
      t_min = fminf(t_min, tmn);
    }
  }
  float v[8] = {wave_sum(s_w), wave_sum(s_se), wave_sum(s_ae), wave_sum(s_cos), wave_max(t_max), wave_min(t_min),
                wave_sum(s_t2), wave_sum(s_t1)};
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][e] = v[e];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int e = threadIdx.x;
    float r;
    if (e == 4) r = fmaxf(fmaxf(red[0][e], red[1][e]), fmaxf(red[2][e], red[3][e]));
    else if (e == 5) r = fminf(fminf(red[0][e], red[1][e]), fminf(red[2][e], red[3][e]));
    else r = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    a.part[((int64_t)b * a.nblk + blockIdx.x) * 8 + e] = r;
  }
}

template <int SPACE>
__global__ void __launch_bounds__(256) k_ssim(const MetArgs a) {
  __shared__ float sp[SS_IN][SS_IN], st[SS_IN][SS_IN];
  __shared__ float mom[5][SS_IN][SS_T];
  __shared__ float red[4][2];
  const int b = (int)blockIdx.y;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const int r0 = ty * SS_T, c0 = tx * SS_T;
  const int rlast = min(r0 + SS_T, a.H) - 1 + SS_R, clast = min(c0 + SS_T, a.W) - 1 + SS_R;  // last row / column any window needs
  const int half = a.W >> 1;
  const float q = SPACE == RENI_SPACE_SRGB ? a.exposure[b] : 1.f;
  const float* pb = a.pred.p + (int64_t)b * a.pred.s[0];
  const float* tb = a.target.p + (int64_t)b * a.target.s[0];
  const int col_l = (int)threadIdx.x & 31, rg = (int)threadIdx.x >> 5;
  float chan[SS_ROWS];
#pragma unroll
  for (int o = 0; o < SS_ROWS; ++o) chan[o] = 0.f;

  for (int c = 0; c < 3; ++c) {
    // tile + halo of both images, mapped
    for (int idx = threadIdx.x; idx < SS_IN * SS_IN; idx += 256) {
      const int i = idx / SS_IN, j = idx - i * SS_IN;
      int row = r0 - SS_R + i, col = c0 - SS_R + j;
      bool ok = row <= rlast && col <= clast;
      if (a.planar) {
        ok = ok && row >= 0 && row < a.H && col >= 0 && col < a.W;
      } else {
        if (row < 0) { row = -1 - row; col += half; }
        else if (row >= a.H) { row = 2 * a.H - 1 - row; col += half; }
        col %= a.W;
        if (col < 0) col += a.W;
      }
      float p = 0.f, t = 0.f;
      if (ok) {
        row = min(max(row, 0), a.H - 1);  // (a no-op for H >= 5, which the entry point checks: an address stays inside whatever comes)
        p = map_value<SPACE>(pb[c * a.pred.s[1] + (int64_t)row * a.pred.s[2] + (int64_t)col * a.pred.s[3]], a.range, a.m0, q);
        t = map_value<SPACE>(tb[c * a.target.s[1] + (int64_t)row * a.target.s[2] + (int64_t)col * a.target.s[3]], a.range, a.m0, q);
      }
      sp[i][j] = p;
      st[i][j] = t;
    }
    __syncthreads();
    // horizontal pass: five moments of every row of the tile + halo
    for (int idx = threadIdx.x; idx < SS_IN * SS_T; idx += 256) {
      const int i = idx >> 5, j = idx & 31;
      float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
      for (int k = 0; k <= 2 * SS_R; ++k) {
        const float p = sp[i][j + k], t = st[i][j + k];
        const float gp = a.g[k] * p, gt = a.g[k] * t;
        m0 += gp;
        m1 += gt;
        m2 = fmaf(gp, p, m2);
        m3 = fmaf(gt, t, m3);
        m4 = fmaf(gp, t, m4);
      }
      mom[0][i][j] = m0; mom[1][i][j] = m1; mom[2][i][j] = m2; mom[3][i][j] = m3; mom[4][i][j] = m4;
    }
    __syncthreads();
    // vertical pass: SS_ROWS output rows of one column per thread
    float acc[5][SS_ROWS];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      float v[SS_ROWS + 2 * SS_R];
#pragma unroll
      for (int i = 0; i < SS_ROWS + 2 * SS_R; ++i) v[i] = mom[m][rg * SS_ROWS + i][col_l];
#pragma unroll
      for (int o = 0; o < SS_ROWS; ++o) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * SS_R; ++k) s = fmaf(a.g[k], v[o + k], s);
        acc[m][o] = s;
      }
    }
#pragma unroll
    for (int o = 0; o < SS_ROWS; ++o) {
      const float mp = acc[0][o], mt = acc[1][o];
      const float mp2 = mp * mp, mt2 = mt * mt, mpt = mp * mt;
      const float vp = acc[2][o] - mp2, vt = acc[3][o] - mt2, cov = acc[4][o] - mpt;
      const float num = (2.f * mpt + a.C1) * (2.f * cov + a.C2);
      const float den = ((mp2 + mt2) + a.C1) * ((vp + vt) + a.C2);
      chan[o] += num / den;
    }
    // (the next channel's loads wait at the barrier behind them for every thread to leave this pass)
  }

  float s_ws = 0.f, s_w = 0.f;
#pragma unroll
  for (int o = 0; o < SS_ROWS; ++o) {
    const int row = r0 + rg * SS_ROWS + o, col = c0 + col_l;
    if (row >= a.H || col >= a.W) continue;
    const bool inside = !a.planar || (row >= SS_R && row < a.H - SS_R && col >= SS_R && col < a.W - SS_R);
    const float s = inside ? chan[o] / 3.f : 0.f;
    if (a.map_out) a.map_out[((int64_t)b * a.H + row) * a.W + col] = s;
    if (!inside) continue;
    const float wt = a.weight ? a.weight[(int64_t)b * a.ws[0] + (int64_t)row * a.ws[1] + (int64_t)col * a.ws[2]] : 1.f;
    if (wt != 0.f) {
      s_ws = fmaf(wt, s, s_ws);
      s_w += wt;
    }
  }
  s_ws = wave_sum(s_ws);
  s_w = wave_sum(s_w);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = s_ws; red[wave][1] = s_w; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int e = threadIdx.x;
    a.part[((int64_t)b * a.nblk + blockIdx.x) * 2 + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

// out[b]: the nblk partials of image b in double, strand s = partials s, s + 8, ... in order, then the strands in order.
// NE = 8: the eight entries of reni_pair_stats (4: max, 5: min);  NE = 2: out[b] = sum / weight (reni_ssim)
template <int NE>
__global__ void __launch_bounds__(64) k_finish(const float* __restrict__ part, int nblk, float* __restrict__ out) {
  __shared__ double red[8][8];
  const int b = (int)blockIdx.x, e = (int)threadIdx.x & 7, s = (int)threadIdx.x >> 3;
  const bool is_max = NE == 8 && e == 4, is_min = NE == 8 && e == 5;
  double v = is_max ? -(double)INFINITY : is_min ? (double)INFINITY : 0.0;
  if (e < NE) {
    const float* pp = part + (int64_t)b * nblk * NE + e;
    for (int j = s; j < nblk; j += 8) {
      const double x = (double)pp[(int64_t)j * NE];
      v = is_max ? fmax(v, x) : is_min ? fmin(v, x) : v + x;
    }
  }
  red[s][e] = v;
  __syncthreads();
  if (threadIdx.x < 8) {
    double r = red[0][e];
    for (int k = 1; k < 8; ++k) r = is_max ? fmax(r, red[k][e]) : is_min ? fmin(r, red[k][e]) : r + red[k][e];
    red[0][e] = r;
  }
  __syncthreads();
  if (NE == 8) {
    if (threadIdx.x < 8) out[(int64_t)b * 8 + e] = (float)red[0][e];
  } else {
    if (threadIdx.x == 0) out[b] = (float)(red[0][0] / red[0][1]);
  }
}

}  // namespace reni

namespace {

using reni::reni_set_error;

int64_t ps_blocks(int64_t H, int64_t W) { return (H * W + reni::PS_CHUNK - 1) / reni::PS_CHUNK; }
int64_t ss_tiles(int64_t n) { return (n + reni::SS_T - 1) / reni::SS_T; }

bool met_shape_ok(int64_t B, int64_t H, int64_t W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 0x3fffffff / W; }

// the checks both entry points share; `what` prefixes the message
int met_check(const char* what, int64_t B, int64_t H, int64_t W, const float* pred, const int64_t* ps, const float* target,
              const int64_t* ts, const float* weight, const int64_t* wst, int32_t space, double m0, double m1,
              const float* exposure, const void* out) {
  if (!met_shape_ok(B, H, W)) return tu_fail(RENI_EINVAL, what, "need 1 <= B <= 65535, H, W >= 1 and H W < 2^30");
  if (!pred || !ps || !target || !ts || !out) return tu_fail(RENI_EINVAL, what, "NULL argument");
  if (weight && !wst) return tu_fail(RENI_EINVAL, what, "NULL argument (a weight needs its strides)");
  if (int rc = tu_check_strides(what, "image strides", ps, 4)) return rc;
  if (int rc = tu_check_strides(what, "image strides", ts, 4)) return rc;
  if (int rc = tu_check_strides(what, "weight strides", wst, weight ? 3 : 0)) return rc;
  if (space != RENI_SPACE_STORED && space != RENI_SPACE_LINEAR && space != RENI_SPACE_SRGB)
    return tu_fail(RENI_EINVAL, what, "unknown space");
  if (space != RENI_SPACE_STORED && !(m1 > m0)) return tu_fail(RENI_EINVAL, what, "minmax[1] must exceed minmax[0] in a mapped space");
  if (space == RENI_SPACE_SRGB && !exposure) return tu_fail(RENI_EINVAL, what, "NULL argument (RENI_SPACE_SRGB needs the exposures)");
  return RENI_OK;
}

void met_fill(reni::MetArgs& a, int64_t H, int64_t W, const float* pred, const int64_t* ps, const float* target, const int64_t* ts,
              const float* weight, const int64_t* wst, double m0, double m1, const float* exposure) {
  a.pred.p = pred; a.target.p = target;
  for (int k = 0; k < 4; ++k) { a.pred.s[k] = ps[k]; a.target.s[k] = ts[k]; }
  a.weight = weight;
  for (int k = 0; k < 3; ++k) a.ws[k] = weight ? wst[k] : 0;
  a.exposure = exposure;
  a.range = (float)(m1 - m0); a.m0 = (float)m0;
  a.H = (int)H; a.W = (int)W;
}

}  // namespace

extern "C" {

size_t reni_pair_stats_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  if (!met_shape_ok(B, H, W)) return 0;
  const int64_t stats = ps_blocks(H, W) * 8, ssim = ss_tiles(H) * ss_tiles(W) * 2;
  return (size_t)(B * (stats > ssim ? stats : ssim)) * sizeof(float) + 256;
}

int reni_pair_stats(int64_t B, int64_t H, int64_t W, const float* pred, const int64_t pred_strides[4], const float* target,
                    const int64_t target_strides[4], const float* weight, const int64_t weight_strides[3], int32_t space,
                    double minmax0, double minmax1, const float* exposure, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = met_check("pair stats", B, H, W, pred, pred_strides, target, target_strides, weight, weight_strides, space,
                         minmax0, minmax1, exposure, out))
    return rc;
  const int64_t nblk = ps_blocks(H, W);
  if (int rc = tu_check_ws("pair stats", ws, ws_bytes, (size_t)(B * nblk * 8) * sizeof(float))) return rc;
  reni::MetArgs a = {};
  met_fill(a, H, W, pred, pred_strides, target, target_strides, weight, weight_strides, minmax0, minmax1, exposure);
  a.nblk = (int)nblk;
  a.part = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  auto k = reni::k_pair_stats<RENI_SPACE_STORED>;
  if (space == RENI_SPACE_LINEAR) k = reni::k_pair_stats<RENI_SPACE_LINEAR>;
  if (space == RENI_SPACE_SRGB) k = reni::k_pair_stats<RENI_SPACE_SRGB>;
  if (int rc = tu_launch(TU_COUNTED, k, grid, dim3(256), 0, s, a)) return rc;
  return tu_launch(TU_COUNTED, reni::k_finish<8>, dim3((unsigned)B), dim3(64), 0, s, a.part, a.nblk, out);
}

int reni_ssim(int64_t B, int64_t H, int64_t W, const float* pred, const int64_t pred_strides[4], const float* target,
              const int64_t target_strides[4], const float* weight, const int64_t weight_strides[3], int32_t space,
              double minmax0, double minmax1, const float* exposure, float L, int32_t mode, float* out, float* map_out, void* ws,
              size_t ws_bytes, void* stream) {
  if (int rc = met_check("ssim", B, H, W, pred, pred_strides, target, target_strides, weight, weight_strides, space, minmax0,
                         minmax1, exposure, out))
    return rc;
  if (mode != RENI_SSIM_SPHERE && mode != RENI_SSIM_PLANAR) return reni_set_error(RENI_EINVAL, "ssim: unknown mode");
  if (!(L > 0.f)) return reni_set_error(RENI_EINVAL, "ssim: the dynamic range L must be > 0");
  const int win = 2 * reni::SS_R + 1;
  if (mode == RENI_SSIM_SPHERE) {
    if (W & 1) return reni_set_error(RENI_EINVAL, "ssim: W must be even on the sphere (the far side of a pole is W / 2 columns away)");
    if (H < reni::SS_R) return reni_set_error(RENI_EINVAL, "ssim: H must be >= 5 on the sphere (a window crosses a pole once)");
  } else {
    if (weight) return reni_set_error(RENI_EINVAL, "ssim: the planar mode is the unweighted published definition: weight must be NULL");
    if (H < win || W < win) return reni_set_error(RENI_EINVAL, "ssim: the planar mode needs H, W >= 11 (one whole window)");
  }
  const int64_t tx = ss_tiles(W), nblk = tx * ss_tiles(H);
  if (int rc = tu_check_ws("ssim", ws, ws_bytes, (size_t)(B * nblk * 2) * sizeof(float))) return rc;
  reni::MetArgs a = {};
  met_fill(a, H, W, pred, pred_strides, target, target_strides, weight, weight_strides, minmax0, minmax1, exposure);
  a.nblk = (int)nblk;
  a.tiles_x = (int)tx;
  a.part = (float*)ws;
  a.planar = mode == RENI_SSIM_PLANAR ? 1 : 0;
  a.map_out = map_out;
  // the window: exp(-x^2 / 2 sigma^2), sigma = 1.5, normalised in float64 and rounded once
  double g[2 * reni::SS_R + 1], sum = 0.0;
  for (int k = 0; k < win; ++k) {
    const double x = (double)(k - reni::SS_R);
    g[k] = exp(-x * x / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < win; ++k) a.g[k] = (float)(g[k] / sum);
  a.C1 = (float)((0.01 * (double)L) * (0.01 * (double)L));
  a.C2 = (float)((0.03 * (double)L) * (0.03 * (double)L));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  auto k = reni::k_ssim<RENI_SPACE_STORED>;
  if (space == RENI_SPACE_LINEAR) k = reni::k_ssim<RENI_SPACE_LINEAR>;
  if (space == RENI_SPACE_SRGB) k = reni::k_ssim<RENI_SPACE_SRGB>;
  if (int rc = tu_launch(TU_COUNTED, k, grid, dim3(256), 0, s, a)) return rc;
  return tu_launch(TU_COUNTED, reni::k_finish<2>, dim3((unsigned)B), dim3(64), 0, s, a.part, a.nblk, out);
}

}  // extern "C"
