// translation unit of libreni_hip.so: environment maps as importance-sampled light lists (reni_amd/lighting.py) -- the sampling
// distribution of a map, inverse-CDF sampling, and the diffuse consumer of per-map light lists.
// No reference counterpart: the reference sums every texel of a map wherever it uses one as a light source.
//
//   k_lt_rows      one workgroup per (row, image): every texel is read once through the caller's strides, mapped into the call's
//                  space IN REGISTERS (reni_dev_image.inc), and turned into its importance f = max(0, luminance) omega_row mask --
//                  formed in double and rounded to fp32 once.  f goes to the pmf array (k_lt_cdf overwrites it in place), the
//                  row's sum of the rounded f, in double, to the workspace.
//   k_lt_image     one workgroup per image: F = sum of the row sums, Omega = sum_i W omega_i, the effective uniform mix (1 when F
//                  is 0 or not finite), and the marginal CDF over rows -- a workgroup-wide scan in double, divided by its own
//                  value at the last row with mass and rounded once (row_cdf).
//   k_lt_cdf       one workgroup per (row, image): pmf = (1 - eps) f / F + eps omega / Omega in double, the same scan along the row;
//                  a row without mass gets (j + 1) / W.
//   k_light_sample one thread per (sample, image): two upper-bound binary searches (entries <= u, clamped), then gathers; with
//                  jitter the direction is uniform in solid angle inside the texel (double: near a pole cos(phi) differs from 1
//                  by less than an fp32 ulp resolves).
//   k_lights_irradiance  out[b][p] = scale sum_s max(0, n_p . d_bs) colors_bs: one thread per output, the image's lights staged in
//                  LDS LI_CHUNK at a time and read as broadcasts, summed in ascending s with one fmaf chain per channel.
// A scan is Hillis-Steele inside a wave, the waves' totals added in wave order, the 256-entry tiles in ascending order: its order
// of additions depends on the row length only, but it is not the sequential order, so a CDF is made ascending, and flat over
// entries without mass, by a running maximum behind the division (row_cdf).  fp32 storage, no float atomics, no host synchronisation, launches on `stream`
// only: two calls give identical bits, and image b's results do not depend on the batch around it or on how it is addressed.
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

constexpr int LT_MAX_W = 4096;
constexpr int LT_TILES = LT_MAX_W / 256;  // tiles of a row scan (a thread keeps one prefix per tile in registers)
constexpr int LI_CHUNK = 1024;            // lights staged in LDS at a time (24 KB)

struct LtArgs {
  const float* img;  // element (b, c, h, w) at img[b s[0] + c s[1] + h s[2] + w s[3]]
  int64_t s[4];
  const float* mask;  // element (b, h, w) at mask[b ms[0] + h ms[1] + w ms[2]]; NULL: 1
  int64_t ms[3];
  const float* solid_angle;  // [H]
  float range, m0;           // (float)(m1 - m0), (float)m0
  double eps;
  int H, W;
  float* pmf;    // [B][H][W]
  float* cond;   // [B][H][W]
  float* marg;   // [B][H]
  double* rowf;  // [B][H]   sum_j f
  double* par;   // [B][4]   F, Omega, effective eps
};

struct LsArgs {
  const float *pmf, *cond, *marg;
  const float* img;
  int64_t s[4];
  float range, m0;
  const float* u;  // sample k of image b at u[b ub + 2 k]
  int64_t ub;
  const float* dirs_table;    // [H W][3]
  const float* solid_angle;   // [H]
  const double* row_cos;      // [H + 1] cos(i pi / H), jitter only
  const float* texel_weight;  // [H W] or NULL
  int H, W, S, jitter;
  int* index;
  float *dirs, *pdf, *radiance, *colors;
};

template <int SPACE>
DEV float lt_map(float x, float range, float m0) {
  return SPACE == RENI_SPACE_STORED ? x : img_unnormalise(x, range, m0);
}

DEV double wave_sum_d(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// sum over the workgroup's 256 threads (lanes in a butterfly, the four waves in order), the same value in every thread
DEV double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}

// inclusive scan of one value per thread over the workgroup's 256 threads
DEV double block_scan_d(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  if (lane == 63) red[wave] = v;
  __syncthreads();
  const double w0 = red[0], w1 = red[1], w2 = red[2];
  const double off = wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : (w0 + w1) + w2;
  __syncthreads();
  return wave == 0 ? v : off + v;
}

// Inclusive scan of n <= 256 LT_TILES values, entry k * 256 + thread in val[k]; returns the scan's value at entry `at` in every
// thread.
DEV double row_scan_d(double (&val)[LT_TILES], int n, int at, double* red, double* last) {
  double carry = 0.0;
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    if (k * 256 < n) {  // (uniform over the workgroup: the barriers inside are reached by all or by none)
      const double inc = block_scan_d(val[k], red);
      val[k] = k == 0 ? inc : carry + inc;
      if (threadIdx.x == 255) *last = val[k];
      if (k * 256 + (int)threadIdx.x == at) last[1] = val[k];
      __syncthreads();
      carry = *last;
    }
  }
  return last[1];
}

// largest value over the workgroup's 256 threads, the same in every thread (a maximum is exact: any order gives it)
DEV double block_max_d(double v, double* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return r;
}

// The CDF of n <= 256 LT_TILES masses (>= 0), entry k * 256 + thread in val[k], into cdf[k], float32.  The prefix sums are those of
// row_scan_d, divided by the scan's own value at the LAST ENTRY WITH MASS, which therefore is exactly 1.0f.  A parallel scan
// builds neighbouring prefixes by different association trees, so what makes the CDF ascending, and flat over an entry without
// mass, is not the sum but a running maximum behind it: an entry with mass gets the largest quotient up to itself, an entry
// without mass the value before it (0 in front of the first mass, 1.0f behind the last).  Without any mass: (j + 1) / n.
DEV void row_cdf(double (&val)[LT_TILES], float (&cdf)[LT_TILES], int n, double* red, double* last) {
  unsigned mass = 0;
  double top = -1.0;
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    const int j = k * 256 + (int)threadIdx.x;
    if (j < n && val[k] > 0.0) { mass |= 1u << k; top = (double)j; }
  }
  const int at = (int)block_max_d(top, red);  // the last entry with mass
  if (at < 0) {
#pragma unroll
    for (int k = 0; k < LT_TILES; ++k) cdf[k] = (float)((double)(k * 256 + (int)threadIdx.x + 1) / (double)n);
    return;
  }
  const double total = row_scan_d(val, n, at, red, last);
  float carry = 0.f;
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    if (k * 256 < n) {
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      float v = (mass >> k) & 1u ? (float)(val[k] / total) : 0.f;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(v, d, 64);
        if (lane >= d) v = fmaxf(v, t);
      }
      if (lane == 63) red[wave] = (double)v;
      __syncthreads();
      const float w0 = (float)red[0], w1 = (float)red[1], w2 = (float)red[2], w3 = (float)red[3];
      const float off = wave == 0 ? 0.f : wave == 1 ? w0 : wave == 2 ? fmaxf(w0, w1) : fmaxf(fmaxf(w0, w1), w2);
      __syncthreads();
      cdf[k] = fmaxf(fmaxf(v, off), carry);
      carry = fmaxf(carry, fmaxf(fmaxf(w0, w1), fmaxf(w2, w3)));
    }
  }
}

template <int SPACE>
__global__ void __launch_bounds__(256) k_lt_rows(const LtArgs a) {
  __shared__ double red[4];
  const int i = (int)blockIdx.x, b = (int)blockIdx.y;
  const float* ib = a.img + (int64_t)b * a.s[0] + (int64_t)i * a.s[2];
  const float* mb = a.mask ? a.mask + (int64_t)b * a.ms[0] + (int64_t)i * a.ms[1] : nullptr;
  const double om = (double)a.solid_angle[i];
  float* fo = a.pmf + ((int64_t)b * a.H + i) * a.W;
  double sum = 0.0;
  for (int j = threadIdx.x; j < a.W; j += 256) {
    const float* px = ib + (int64_t)j * a.s[3];
    const double r = (double)lt_map<SPACE>(px[0], a.range, a.m0);
    const double g = (double)lt_map<SPACE>(px[a.s[1]], a.range, a.m0);
    const double bl = (double)lt_map<SPACE>(px[2 * a.s[1]], a.range, a.m0);
    double f = (0.2126 * r + 0.7152 * g) + 0.0722 * bl;
    f *= om;
    if (mb) f *= (double)mb[(int64_t)j * a.ms[2]];
    const float ff = f > 0.0 ? (float)f : 0.f;  // (a NaN fails the comparison: such a texel has no importance)
    fo[j] = ff;
    sum += (double)ff;
  }
  sum = block_sum_d(sum, red);
  if (threadIdx.x == 0) a.rowf[(int64_t)b * a.H + i] = sum;
}

// the probability mass of a row from its f sum: what k_lt_cdf's scan of the row ends on, up to double rounding
DEV double lt_row_mass(double rowf, double om, double F, double Om, double eps, int W) {
  double m = eps * ((double)W * om) / Om;
  if (eps < 1.0) m += (1.0 - eps) * rowf / F;
  return m;
}

__global__ void __launch_bounds__(256) k_lt_image(const LtArgs a) {
  __shared__ double red[4];
  __shared__ double last[2];
  const int b = (int)blockIdx.x;
  const double* rf = a.rowf + (int64_t)b * a.H;
  double sf = 0.0, so = 0.0;
  for (int i = threadIdx.x; i < a.H; i += 256) {
    sf += rf[i];
    so += (double)a.W * (double)a.solid_angle[i];
  }
  const double F = block_sum_d(sf, red), Om = block_sum_d(so, red);
  const double eps = (F > 0.0 && F <= 1.7976931348623157e308) ? a.eps : 1.0;  // (a NaN or an infinite F fails the comparisons)
  if (threadIdx.x == 0) {
    double* p = a.par + (int64_t)b * 4;
    p[0] = F; p[1] = Om; p[2] = eps;
  }
  double val[LT_TILES];
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    const int i = k * 256 + (int)threadIdx.x;
    val[k] = i < a.H ? lt_row_mass(rf[i], (double)a.solid_angle[i], F, Om, eps, a.W) : 0.0;
  }
  float cdf[LT_TILES];
  row_cdf(val, cdf, a.H, red, last);
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    const int i = k * 256 + (int)threadIdx.x;
    if (i < a.H) a.marg[(int64_t)b * a.H + i] = cdf[k];
  }
}

__global__ void __launch_bounds__(256) k_lt_cdf(const LtArgs a) {
  __shared__ double red[4];
  __shared__ double last[2];
  const int i = (int)blockIdx.x, b = (int)blockIdx.y;
  const double* p = a.par + (int64_t)b * 4;
  const double F = p[0], Om = p[1], eps = p[2];
  const double om = (double)a.solid_angle[i];
  const double uni = eps * om / Om;
  float* po = a.pmf + ((int64_t)b * a.H + i) * a.W;
  float* co = a.cond + ((int64_t)b * a.H + i) * a.W;
  double val[LT_TILES];
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    const int j = k * 256 + (int)threadIdx.x;
    double m = 0.0;
    if (j < a.W) {
      m = uni;
      if (eps < 1.0) m += (1.0 - eps) * (double)po[j] / F;
      const float pf = (float)m;
      po[j] = pf;
      if (pf == 0.f) m = 0.0;  // (mass is what the stored pmf says: a texel whose pmf is 0 is never to be chosen)
    }
    val[k] = m;
  }
  float cdf[LT_TILES];
  row_cdf(val, cdf, a.W, red, last);
#pragma unroll
  for (int k = 0; k < LT_TILES; ++k) {
    const int j = k * 256 + (int)threadIdx.x;
    if (j < a.W) co[j] = cdf[k];
  }
}

// the number of entries of the ascending table t[0 .. n) that are <= u, at most n - 1
DEV int ls_upper(const float* __restrict__ t, int n, float u) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  return min(lo, n - 1);
}

// where u lies between the table entries around position k, in [0, 1]
DEV double ls_fraction(const float* __restrict__ t, int k, float u) {
  const double lo = k > 0 ? (double)t[k - 1] : 0.0, hi = (double)t[k];
  const double x = hi > lo ? ((double)u - lo) / (hi - lo) : 0.5;
  return fmin(fmax(x, 0.0), 1.0);
}

template <int SPACE>
__global__ void __launch_bounds__(256) k_light_sample(const LsArgs a) {
  const int k = (int)blockIdx.x * 256 + (int)threadIdx.x, b = (int)blockIdx.y;
  if (k >= a.S) return;
  const float u0 = a.u[(int64_t)b * a.ub + 2 * k], u1 = a.u[(int64_t)b * a.ub + 2 * k + 1];
  const float* mg = a.marg + (int64_t)b * a.H;
  const int i = ls_upper(mg, a.H, u0);
  const float* cd = a.cond + ((int64_t)b * a.H + i) * a.W;
  const int j = ls_upper(cd, a.W, u1);
  const int idx = i * a.W + j;
  const float pm = a.pmf[(int64_t)b * a.H * a.W + idx];
  const float om = a.solid_angle[i];
  const float tw = a.texel_weight ? a.texel_weight[idx] : 1.f;
  const float* px = a.img + (int64_t)b * a.s[0] + (int64_t)i * a.s[2] + (int64_t)j * a.s[3];
  const int64_t o = (int64_t)b * a.S + k;
  float d[3];
  if (a.jitter) {
    const double tr = ls_fraction(mg, i, u0), tc = ls_fraction(cd, j, u1);
    const double c0 = a.row_cos[i], c1 = a.row_cos[i + 1];
    const double cp = c0 - tr * (c0 - c1);
    const double sp = sqrt(fmax(1.0 - cp * cp, 0.0));
    double st, ct;  // of theta = 2 pi (j + t_c) / W - pi
    sincospi(2.0 * ((double)j + tc) / (double)a.W - 1.0, &st, &ct);
    d[0] = (float)(sp * st); d[1] = (float)cp; d[2] = (float)(-sp * ct);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = a.dirs_table[3 * (int64_t)idx + c];
  }
  const float g = tw / ((float)a.S * pm);
  a.index[o] = idx;
  a.pdf[o] = pm / om;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float rad = lt_map<SPACE>(px[c * a.s[1]], a.range, a.m0);
    a.dirs[3 * o + c] = d[c];
    a.radiance[3 * o + c] = rad;
    a.colors[3 * o + c] = rad * g;
  }
}

__global__ void __launch_bounds__(256) k_lights_irradiance(int P, int S, const float* __restrict__ normals, int64_t nstride,
                                                           const float* __restrict__ dirs, const float* __restrict__ colors,
                                                           float scale, float* __restrict__ out) {
  __shared__ float4 la[LI_CHUNK];  // direction, red
  __shared__ float2 lb[LI_CHUNK];  // green, blue
  const int b = (int)blockIdx.y;
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int pr = min(p, P - 1);  // (a thread beyond P computes the last output again and does not store it)
  const float* nv = normals + (int64_t)b * nstride + 3 * (int64_t)pr;
  const float nx = nv[0], ny = nv[1], nz = nv[2];
  const float* db = dirs + (int64_t)b * S * 3;
  const float* cb = colors + (int64_t)b * S * 3;
  float ar = 0.f, ag = 0.f, ab = 0.f;
  for (int s0 = 0; s0 < S; s0 += LI_CHUNK) {
    const int n = min(LI_CHUNK, S - s0);
    __syncthreads();  // the chunk before has been read by everyone
    for (int k = threadIdx.x; k < n; k += 256) {
      const float* dp = db + 3 * (int64_t)(s0 + k);
      const float* cp = cb + 3 * (int64_t)(s0 + k);
      la[k] = make_float4(dp[0], dp[1], dp[2], cp[0]);
      lb[k] = make_float2(cp[1], cp[2]);
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float4 l = la[k];
      const float2 c = lb[k];
      float t = nx * l.x;
      t = fmaf(ny, l.y, t);
      t = fmaf(nz, l.z, t);
      t = fmaxf(t, 0.f);
      ar = fmaf(t, l.w, ar);
      ag = fmaf(t, c.x, ag);
      ab = fmaf(t, c.y, ab);
    }
  }
  if (p < P) {
    float* op = out + ((int64_t)b * P + p) * 3;
    op[0] = scale * ar; op[1] = scale * ag; op[2] = scale * ab;
  }
}

}  // namespace reni

namespace {

using reni::reni_set_error;

constexpr int64_t LT_MAX_ELEMS = (int64_t)1 << 28;  // B S and B P stay below this (3 B S fits an int with room to spare)

bool lt_shape_ok(int64_t B, int64_t H, int64_t W) {
  return B >= 1 && B <= 65535 && W >= 2 && W <= reni::LT_MAX_W && (W & 1) == 0 && H == W / 2;
}

// the checks of an image argument that the table and the sampler share
int lt_check_image(const char* what, const float* img, const int64_t* st, int32_t space, double m0, double m1) {
  if (!img || !st) return tu_fail(RENI_EINVAL, what, "NULL argument");
  if (int rc = tu_check_strides(what, "image strides", st, 4)) return rc;
  if (space == RENI_SPACE_SRGB)
    return tu_fail(RENI_EINVAL, what, "RENI_SPACE_SRGB is a display space, not radiance: use RENI_SPACE_STORED or RENI_SPACE_LINEAR");
  if (space != RENI_SPACE_STORED && space != RENI_SPACE_LINEAR) return tu_fail(RENI_EINVAL, what, "unknown space");
  if (space == RENI_SPACE_LINEAR && !(m1 > m0)) return tu_fail(RENI_EINVAL, what, "minmax[1] must exceed minmax[0] in RENI_SPACE_LINEAR");
  return RENI_OK;
}

int64_t lt_ws_doubles(int64_t B, int64_t H) { return B * (H + 4); }

}  // namespace

extern "C" {

size_t reni_light_table_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  if (!lt_shape_ok(B, H, W)) return 0;
  return (size_t)lt_ws_doubles(B, H) * sizeof(double) + 256;
}

int reni_light_table_build(int64_t B, int64_t H, int64_t W, const float* img, const int64_t img_strides[4], const float* mask,
                           const int64_t mask_strides[3], int32_t space, double minmax0, double minmax1, const float* solid_angle,
                           double uniform_mix, float* pmf, float* cond, float* marg, void* ws, size_t ws_bytes, void* stream) {
  if (!lt_shape_ok(B, H, W))
    return reni_set_error(RENI_EINVAL, "light table: need 1 <= B <= 65535, W even, 2 <= W <= 4096 and H = W / 2");
  if (int rc = lt_check_image("light table", img, img_strides, space, minmax0, minmax1)) return rc;
  if (!solid_angle || !pmf || !cond || !marg) return reni_set_error(RENI_EINVAL, "light table: NULL argument");
  if (mask && !mask_strides) return reni_set_error(RENI_EINVAL, "light table: NULL argument (a mask needs its strides)");
  if (int rc = tu_check_strides("light table", "mask strides", mask_strides, mask ? 3 : 0)) return rc;
  if (!(uniform_mix >= 0.0 && uniform_mix <= 1.0)) return reni_set_error(RENI_EINVAL, "light table: uniform_mix must lie in [0, 1]");
  if (int rc = tu_check_ws("light table", ws, ws_bytes, (size_t)lt_ws_doubles(B, H) * sizeof(double))) return rc;
  reni::LtArgs a = {};
  a.img = img;
  for (int k = 0; k < 4; ++k) a.s[k] = img_strides[k];
  a.mask = mask;
  for (int k = 0; k < 3; ++k) a.ms[k] = mask ? mask_strides[k] : 0;
  a.solid_angle = solid_angle;
  a.range = (float)(minmax1 - minmax0); a.m0 = (float)minmax0;
  a.eps = uniform_mix;
  a.H = (int)H; a.W = (int)W;
  a.pmf = pmf; a.cond = cond; a.marg = marg;
  a.rowf = (double*)ws;
  a.par = a.rowf + B * H;
  hipStream_t s = (hipStream_t)stream;
  const dim3 rows((unsigned)H, (unsigned)B);
  const auto k = space == RENI_SPACE_STORED ? reni::k_lt_rows<RENI_SPACE_STORED> : reni::k_lt_rows<RENI_SPACE_LINEAR>;
  if (int rc = tu_launch(TU_COUNTED, k, rows, dim3(256), 0, s, a)) return rc;
  if (int rc = tu_launch(TU_COUNTED, reni::k_lt_image, dim3((unsigned)B), dim3(256), 0, s, a)) return rc;
  return tu_launch(TU_COUNTED, reni::k_lt_cdf, rows, dim3(256), 0, s, a);
}

int reni_light_sample(int64_t B, int64_t H, int64_t W, int64_t S, const float* pmf, const float* cond, const float* marg,
                      const float* img, const int64_t img_strides[4], int32_t space, double minmax0, double minmax1,
                      const float* u, int64_t u_stride_b, const float* dirs_table, const float* solid_angle,
                      const double* row_cos, const float* texel_weight, int32_t jitter, int32_t* index, float* dirs, float* pdf,
                      float* radiance, float* colors, void* stream) {
  if (!lt_shape_ok(B, H, W))
    return reni_set_error(RENI_EINVAL, "light sample: need 1 <= B <= 65535, W even, 2 <= W <= 4096 and H = W / 2");
  if (S < 1 || S >= LT_MAX_ELEMS || B * S >= LT_MAX_ELEMS)
    return reni_set_error(RENI_EINVAL, "light sample: need S >= 1 and B S < 2^28");
  if (int rc = lt_check_image("light sample", img, img_strides, space, minmax0, minmax1)) return rc;
  if (!pmf || !cond || !marg || !u || !dirs_table || !solid_angle || !index || !dirs || !pdf || !radiance || !colors)
    return reni_set_error(RENI_EINVAL, "light sample: NULL argument");
  if (u_stride_b != 0 && u_stride_b != 2 * S)
    return reni_set_error(RENI_EINVAL, "light sample: the uniforms' image stride must be 0 (shared) or 2 S (per image)");
  if (jitter != 0 && jitter != 1) return reni_set_error(RENI_EINVAL, "light sample: jitter must be 0 or 1");
  if (jitter && !row_cos) return reni_set_error(RENI_EINVAL, "light sample: NULL argument (jitter needs row_cos)");
  reni::LsArgs a = {};
  a.pmf = pmf; a.cond = cond; a.marg = marg;
  a.img = img;
  for (int k = 0; k < 4; ++k) a.s[k] = img_strides[k];
  a.range = (float)(minmax1 - minmax0); a.m0 = (float)minmax0;
  a.u = u; a.ub = u_stride_b;
  a.dirs_table = dirs_table; a.solid_angle = solid_angle; a.row_cos = row_cos; a.texel_weight = texel_weight;
  a.H = (int)H; a.W = (int)W; a.S = (int)S; a.jitter = jitter;
  a.index = index; a.dirs = dirs; a.pdf = pdf; a.radiance = radiance; a.colors = colors;
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  const auto k = space == RENI_SPACE_STORED ? reni::k_light_sample<RENI_SPACE_STORED> : reni::k_light_sample<RENI_SPACE_LINEAR>;
  return tu_launch(TU_COUNTED, k, grid, dim3(256), 0, s, a);
}

int reni_lights_irradiance(int64_t B, int64_t P, int64_t S, const float* normals, int64_t normals_stride_b, const float* dirs,
                           const float* colors, float scale, float* out, void* stream) {
  if (B < 1 || B > 65535 || P < 1 || S < 1 || P >= LT_MAX_ELEMS || S >= LT_MAX_ELEMS || B * P >= LT_MAX_ELEMS || B * S >= LT_MAX_ELEMS)
    return reni_set_error(RENI_EINVAL, "lights irradiance: need 1 <= B <= 65535, P, S >= 1 and B P, B S < 2^28");
  if (normals_stride_b != 0 && normals_stride_b != 3 * P)
    return reni_set_error(RENI_EINVAL, "lights irradiance: the normals' image stride must be 0 (shared) or 3 P (per image)");
  if (!normals || !dirs || !colors || !out) return reni_set_error(RENI_EINVAL, "lights irradiance: NULL argument");
  return tu_launch(TU_COUNTED, reni::k_lights_irradiance, dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0,
                   (hipStream_t)stream, (int)P, (int)S, normals, normals_stride_b, dirs, colors, scale, out);
}

}  // extern "C"
