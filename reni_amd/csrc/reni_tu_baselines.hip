// translation unit of libreni_hip.so: the spherical-Gaussian and spherical-harmonic environment-map baselines.
//
// Reference: src/models/spherical_gaussians.py (SGEnvOptim: renderSG :109-137, the reparametrisation :170-173, the loss
// WeightedMSE of src/utils/loss_functions.py:6-13) and src/models/spherical_harmonics.py (getCoefficientsFromImage
// :174-204, shReconstructSignal :433-437).  fp32 throughout, no float atomics: every sum runs in a fixed order, so two calls
// give identical bits and a map's results do not depend on the batch around it.
//
//   k_sg_loss_grad   one wave64 per map (four maps per 256-thread workgroup).  The lanes first turn the map's raw parameters
//                    into lobes (axis, lambda, weight) in LDS.  Pass 1, pixel-major: each lane renders its pixels over all
//                    K lobes, adds s (log(rec + 1) - log(env + 1))^2 to its loss partial and keeps g = dL/drec per pixel in
//                    LDS.  Pass 2, lobe-major: the exponential is recomputed and the 7 sums of the lobe (3 dw, dlambda,
//                    3 d axis) are accumulated per lane, then butterfly-reduced across the wave; the chain rule through
//                    exp / tanh / the axis runs once per lobe.  No [N, K, ..., H, W] intermediate exists anywhere.
//   k_sg_render      the same render alone: rec [N][3][H][W].
//   k_sh_project     coeffs [T][(n, c)] = sum_q Y_t(q) dOmega(q) img[n][q][c]: a GEMM whose basis operand is built in
//                    registers from the separable tables (row table [H][T] with the solid angle folded in, column table
//                    [W][T]), so no [H W, T] matrix ever exists.  fp32 MFMA v_mfma_f32_32x32x2_f32, one wave per 32 (n, c)
//                    columns and all T rows.
//   k_sh_reconstruct out[(n, q)][c] = sum_t Y_t(q) coeffs[n][t][c]: the same GEMM the other way round, 128 pixels x 32 (n, c)
//                    columns per wave.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#include "reni_sphere.inc"  // the MFMA result-row map and the drain pad

namespace reni {

constexpr int SG_WAVES = 4;            // maps per workgroup (one wave each)
constexpr int SG_MAX_K = 64;           // lobes per map
constexpr int SG_LDS_MAX_PIX = 768;    // pixels per map up to which the directions and g live in LDS
constexpr int SG_MAX_BLOCKS_WS = 512;  // workgroups of the workspace path (each loops over map groups)
constexpr int SH_MAX_LMAX = 15;

// ---- spherical Gaussians -----------------------------------------------------------------------------------------------
struct SgArgs {
  const float* raw;      // [N][K][6] = (w0, w1, w2, theta~, phi~, lambda~)
  const float* theta_c;  // [K]
  const float* phi_c;    // [K]
  float theta_r, phi_r;
  int N, K, H, W;
  const float* logt;  // [N][3][H][W] log(env + 1)
  const float* sw;    // weight, element strides below (0 = broadcast)
  int64_t s0, s1, s2, s3;
  float* rec;      // [N][3][H][W] (render)
  float* loss;     // [N] per-map loss
  float* grad;     // [N][K][6]
  float* ws;       // per-workgroup directions + g when they do not fit in LDS
};

// SGEnvOptim's hemisphere grid (:41-52), computed in double and rounded to float as the reference does
DEV void sg_dir(int p, int H, int W, float& x, float& y, float& z) {
  const int i = p / W, j = p - i * W;
  const double az = (((double)j + 0.5) / W - 0.5) * 2.0 * M_PI;
  const double el = (((double)i + 0.5) / H) * M_PI / 2.0;
  const double se = sin(el);
  x = (float)(se * cos(az));
  y = (float)(se * sin(az));
  z = (float)cos(el);
}

// lane k < K of the wave: lobe k of map n -> lobe[k] = {ax, ay, az, lambda}, {w0, w1, w2, 0}
DEV void sg_lobes(const SgArgs& a, int n, int lane, float4* lobe) {
  if (lane < a.K) {
    const float* r = a.raw + ((size_t)n * a.K + lane) * 6;
    const float th = a.theta_r * tanhf(r[3]) + a.theta_c[lane];
    const float ph = a.phi_r * tanhf(r[4]) + a.phi_c[lane];
    const float st = sinf(th), ct = cosf(th), sp = sinf(ph), cp = cosf(ph);
    lobe[2 * lane] = float4{st * cp, st * sp, ct, expf(r[5])};
    lobe[2 * lane + 1] = float4{expf(r[0]), expf(r[1]), expf(r[2]), 0.f};
  }
}

DEV float wave_sum(float v) {  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) k_sg_render(const SgArgs a) {
  __shared__ float4 s_lobe[SG_WAVES][2 * SG_MAX_K];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * SG_WAVES + wave;
  if (n >= a.N) return;
  float4* lobe = s_lobe[wave];
  sg_lobes(a, n, lane, lobe);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int P = a.H * a.W;
  float* out = a.rec + (size_t)n * 3 * P;
  for (int p = lane; p < P; p += 64) {
    float lx, ly, lz;
    sg_dir(p, a.H, a.W, lx, ly, lz);
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const float4 g = lobe[2 * k], w = lobe[2 * k + 1];
      const float e = expf(g.w * (g.x * lx + g.y * ly + g.z * lz - 1.f));
      r0 += w.x * e; r1 += w.y * e; r2 += w.z * e;
    }
    out[p] = r0; out[P + p] = r1; out[2 * P + p] = r2;
  }
}

// dynamic LDS (LDS path): dirs x, y, z [3][P] shared by the four waves, then g [4 waves][3][P]
template <bool kLds>
__global__ void __launch_bounds__(256) k_sg_loss_grad(const SgArgs a) {
  __shared__ float4 s_lobe[SG_WAVES][2 * SG_MAX_K];
  extern __shared__ float s_dyn[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = a.H * a.W;
  float* base = kLds ? s_dyn : a.ws + (size_t)blockIdx.x * 15 * P;
  float* dir = base;                          // [3][P]
  float* gbuf = base + 3 * P + wave * 3 * P;  // [3][P] of this wave's map
  for (int p = tid; p < P; p += 256) sg_dir(p, a.H, a.W, dir[p], dir[P + p], dir[2 * P + p]);
  const int groups = (a.N + SG_WAVES - 1) / SG_WAVES;
  const float inv = 1.f / (float)(3 * P);
  float4* lobe = s_lobe[wave];
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int n = grp * SG_WAVES + wave;
    const bool live = n < a.N;
    __syncthreads();  // directions written; the previous group's lobes and g no longer read
    if (live) sg_lobes(a, n, lane, lobe);
    __syncthreads();
    // pass 1: render, loss partial, g = dL/drec
    float lpart = 0.f;
    if (live) {
      const float* lt = a.logt + (size_t)n * 3 * P;
      const float* swn = a.sw + n * a.s0;
      for (int p = lane; p < P; p += 64) {
        const float lx = dir[p], ly = dir[P + p], lz = dir[2 * P + p];
        float r[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < a.K; ++k) {
          const float4 g = lobe[2 * k], w = lobe[2 * k + 1];
          const float e = expf(g.w * (g.x * lx + g.y * ly + g.z * lz - 1.f));
          r[0] += w.x * e; r[1] += w.y * e; r[2] += w.z * e;
        }
        const int i = p / a.W, j = p - i * a.W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float s = swn[c * a.s1 + i * a.s2 + j * a.s3];
          const float r1 = r[c] + 1.f;
          const float d = logf(r1) - lt[c * P + p];
          lpart += s * (d * d);
          gbuf[c * P + p] = (2.f * inv) * s * d / r1;
        }
      }
    }
    const float lsum = wave_sum(lpart);
    if (live && lane == 0) a.loss[n] = lsum * inv;
    __syncthreads();  // g of every pixel written
    if (!live) continue;
    // pass 2: per lobe, the 7 sums over the pixels, then the chain rule to the raw parameters
    for (int k = 0; k < a.K; ++k) {
      const float4 g = lobe[2 * k], w = lobe[2 * k + 1];
      float sw0 = 0.f, sw1 = 0.f, sw2 = 0.f, sl = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
      for (int p = lane; p < P; p += 64) {
        const float lx = dir[p], ly = dir[P + p], lz = dir[2 * P + p];
        const float g0 = gbuf[p], g1 = gbuf[P + p], g2 = gbuf[2 * P + p];
        const float dm1 = g.x * lx + g.y * ly + g.z * lz - 1.f;
        const float e = expf(g.w * dm1);
        const float ge = (g0 * w.x + g1 * w.y + g2 * w.z) * e;
        sw0 += g0 * e; sw1 += g1 * e; sw2 += g2 * e;
        sl += ge * dm1;
        sx += ge * lx; sy += ge * ly; sz += ge * lz;
      }
      sw0 = wave_sum(sw0); sw1 = wave_sum(sw1); sw2 = wave_sum(sw2);
      sl = wave_sum(sl);
      sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
      if (lane == 0) {
        const float* r = a.raw + ((size_t)n * a.K + k) * 6;
        const float tt = tanhf(r[3]), tp = tanhf(r[4]);
        const float th = a.theta_r * tt + a.theta_c[k];
        const float ph = a.phi_r * tp + a.phi_c[k];
        const float st = sinf(th), ct = cosf(th), sp = sinf(ph), cp = cosf(ph);
        const float dax = g.w * sx, day = g.w * sy, daz = g.w * sz;  // dL/d axis
        const float dth = dax * (ct * cp) + day * (ct * sp) - daz * st;
        const float dph = -dax * (st * sp) + day * (st * cp);
        float* o = a.grad + ((size_t)n * a.K + k) * 6;
        o[0] = w.x * sw0;
        o[1] = w.y * sw1;
        o[2] = w.z * sw2;
        o[3] = dth * (a.theta_r * (1.f - tt * tt));
        o[4] = dph * (a.phi_r * (1.f - tp * tp));
        o[5] = g.w * sl;
      }
    }
  }
}

// total = sum of the per-map losses, in a fixed order (strided per thread, then a fixed tree)
__global__ void __launch_bounds__(256) k_sg_total(const float* __restrict__ loss, int N, float* __restrict__ total) {
  __shared__ float s[256];
  float v = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) v += loss[i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s[0];
}

// ---- spherical harmonics -----------------------------------------------------------------------------------------------
struct ShArgs {
  int N, H, W, T;
  const float* row;  // [H][T]  K P (sqrt 2 for m != 0), times dOmega(y) for the projection
  const float* col;  // [W][T]  cos(m phi) / 1 / sin(|m| phi)
  const float* in;
  float* out;
};

// coeffs [N][T][3] from img [N][H][W][3]; MT 32-row tiles of t cover T
template <int MT>
__global__ void __launch_bounds__(64) k_sh_project(const ShArgs a) {
  const int lane = threadIdx.x, j = lane & 31, hi = lane >> 5;
  const int64_t ncol = 3 * (int64_t)a.N;
  const int64_t col = (int64_t)blockIdx.x * 32 + j;
  const bool cok = col < ncol;
  const int64_t n = cok ? col / 3 : 0;
  const int c = cok ? (int)(col - 3 * n) : 0;
  const int Q = a.H * a.W, T = a.T;
  const float* xp = a.in + n * 3 * (int64_t)Q + c;
  mfma_f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  // one flat loop over pixel pairs: a nested row loop lets the compiler shuttle the accumulators between register files
  // (and pad the MFMA hazard too short across the branch)
  for (int q0 = 0; q0 < Q; q0 += 2) {
    const int q = q0 + hi;  // W is even: q and q0 share the row
    const int y = q0 / a.W, x = q - y * a.W;
    const float b = cok ? xp[3 * (int64_t)q] : 0.f;
    const float* rw = a.row + y * T;
    const float* cl = a.col + x * T;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int t = m * 32 + j;
      const float av = t < T ? rw[t] * cl[t] : 0.f;
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[m], 0, 0, 0);
    }
  }
  mfma_drain();
  if (!cok) return;
  float* o = a.out + n * 3 * (int64_t)T + c;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = m * 32 + mfma_rowmap(r, hi);
      if (t < T) o[3 * t] = acc[m][r];
    }
}

constexpr int SH_QT = 4;  // 32-pixel tiles per reconstruction wave

// out [N][H][W][3] from coeffs [N][T][3]
__global__ void __launch_bounds__(64) k_sh_reconstruct(const ShArgs a) {
  const int lane = threadIdx.x, j = lane & 31, hi = lane >> 5;
  const int64_t ncol = 3 * (int64_t)a.N;
  const int64_t col = (int64_t)blockIdx.x * 32 + j;
  const bool cok = col < ncol;
  const int64_t n = cok ? col / 3 : 0;
  const int c = cok ? (int)(col - 3 * n) : 0;
  const int Q = a.H * a.W, T = a.T;
  const int q0 = blockIdx.y * (32 * SH_QT);
  const float* rowp[SH_QT];
  const float* colp[SH_QT];
  bool qok[SH_QT];
  mfma_f32x16 acc[SH_QT];
#pragma unroll
  for (int u = 0; u < SH_QT; ++u) {
    const int q = q0 + u * 32 + j;
    qok[u] = q < Q;
    const int y = qok[u] ? q / a.W : 0, x = qok[u] ? q - y * a.W : 0;
    rowp[u] = a.row + y * T;
    colp[u] = a.col + x * T;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
  }
  const float* cp = a.in + n * 3 * (int64_t)T + c;
  for (int t0 = 0; t0 < T; t0 += 2) {
    const int t = t0 + hi;
    const bool tok = t < T;
    const float b = cok && tok ? cp[3 * t] : 0.f;
#pragma unroll
    for (int u = 0; u < SH_QT; ++u) {
      const float av = qok[u] && tok ? rowp[u][t] * colp[u][t] : 0.f;
      acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[u], 0, 0, 0);
    }
  }
  mfma_drain();
  if (!cok) return;
  float* o = a.out + n * 3 * (int64_t)Q + c;
#pragma unroll
  for (int u = 0; u < SH_QT; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = q0 + u * 32 + mfma_rowmap(r, hi);
      if (q < Q) o[3 * (int64_t)q] = acc[u][r];
    }
}

}  // namespace reni

namespace {

using reni::reni_set_error;
constexpr int64_t BL_MAX_ELEMS = 0x3fffffff;
constexpr int64_t SH_MAX_W = 4096;  // keeps the reconstruction grid's y extent (H W / 128) under 65536

bool sg_shape_ok(int64_t N, int64_t K, int64_t H, int64_t W) {
  return N >= 1 && K >= 1 && K <= reni::SG_MAX_K && H >= 1 && W >= 1 && H <= BL_MAX_ELEMS / W &&
         N <= BL_MAX_ELEMS / (3 * H * W) && N * K <= BL_MAX_ELEMS / 6;
}

bool sg_uses_lds(int64_t H, int64_t W) { return H * W <= reni::SG_LDS_MAX_PIX; }

int64_t sg_ws_blocks(int64_t N) {
  const int64_t groups = (N + reni::SG_WAVES - 1) / reni::SG_WAVES;
  return groups < reni::SG_MAX_BLOCKS_WS ? groups : reni::SG_MAX_BLOCKS_WS;
}

reni::SgArgs sg_args(int64_t N, int64_t K, int64_t H, int64_t W, const float* params, const float* theta_c, const float* phi_c,
                     float theta_range, float phi_range) {
  reni::SgArgs a = {};
  a.raw = params; a.theta_c = theta_c; a.phi_c = phi_c;
  a.theta_r = theta_range; a.phi_r = phi_range;
  a.N = (int)N; a.K = (int)K; a.H = (int)H; a.W = (int)W;
  return a;
}

int sh_check(int64_t N, int64_t H, int64_t W, int64_t lmax) {
  if (lmax < 0 || lmax > reni::SH_MAX_LMAX) return reni_set_error(RENI_EINVAL, "sh: lmax must be in [0, 15]");
  if (N < 1 || W < 2 || (W & 1) || H != W / 2) return reni_set_error(RENI_EINVAL, "sh: need N >= 1, W even, H == W / 2");
  if (W > SH_MAX_W || N > BL_MAX_ELEMS / (3 * H * W)) return reni_set_error(RENI_EINVAL, "sh: W > 4096 or too many elements");
  return RENI_OK;
}

}  // namespace

extern "C" {

size_t reni_sg_workspace_bytes(int64_t N, int64_t K, int64_t H, int64_t W) {
  if (!sg_shape_ok(N, K, H, W)) return 0;
  if (sg_uses_lds(H, W)) return 0;
  return (size_t)sg_ws_blocks(N) * 15 * (size_t)(H * W) * sizeof(float) + 256;
}

int reni_sg_render(int64_t N, int64_t K, int64_t H, int64_t W, const float* params, const float* theta_c, const float* phi_c,
                   float theta_range, float phi_range, float* rec, void* stream) {
  if (!sg_shape_ok(N, K, H, W)) return reni_set_error(RENI_EINVAL, "sg render: need N >= 1, 1 <= K <= 64, H, W >= 1");
  if (!params || !theta_c || !phi_c || !rec) return reni_set_error(RENI_EINVAL, "sg render: NULL argument");
  reni::SgArgs a = sg_args(N, K, H, W, params, theta_c, phi_c, theta_range, phi_range);
  a.rec = rec;
  const unsigned blocks = (unsigned)((N + reni::SG_WAVES - 1) / reni::SG_WAVES);
  return tu_launch(TU_PLAIN, reni::k_sg_render, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
}

int reni_sg_loss_grad(int64_t N, int64_t K, int64_t H, int64_t W, const float* params, const float* theta_c, const float* phi_c,
                      float theta_range, float phi_range, const float* log_target, const float* weight, int64_t w_stride_n,
                      int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, float* loss_per_map, float* loss_total,
                      float* dparams, void* ws, size_t ws_bytes, void* stream) {
  if (!sg_shape_ok(N, K, H, W)) return reni_set_error(RENI_EINVAL, "sg loss: need N >= 1, 1 <= K <= 64, H, W >= 1");
  if (!params || !theta_c || !phi_c || !log_target || !weight || !loss_per_map || !loss_total || !dparams)
    return reni_set_error(RENI_EINVAL, "sg loss: NULL argument");
  if (w_stride_n < 0 || w_stride_c < 0 || w_stride_h < 0 || w_stride_w < 0)
    return reni_set_error(RENI_EINVAL, "sg loss: weight strides must be >= 0");
  reni::SgArgs a = sg_args(N, K, H, W, params, theta_c, phi_c, theta_range, phi_range);
  a.logt = log_target; a.sw = weight;
  a.s0 = w_stride_n; a.s1 = w_stride_c; a.s2 = w_stride_h; a.s3 = w_stride_w;
  a.loss = loss_per_map; a.grad = dparams;
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = H * W;
  if (sg_uses_lds(H, W)) {
    const unsigned blocks = (unsigned)((N + reni::SG_WAVES - 1) / reni::SG_WAVES);
    if (int rc = tu_launch(TU_PLAIN, reni::k_sg_loss_grad<true>, dim3(blocks), dim3(256), (size_t)15 * P * sizeof(float), s, a)) return rc;
  } else {
    if (int rc = tu_check_ws("sg loss", ws, ws_bytes, (size_t)sg_ws_blocks(N) * 15 * (size_t)P * sizeof(float))) return rc;
    a.ws = (float*)ws;
    if (int rc = tu_launch(TU_PLAIN, reni::k_sg_loss_grad<false>, dim3((unsigned)sg_ws_blocks(N)), dim3(256), 0, s, a)) return rc;
  }
  return tu_launch(TU_PLAIN, reni::k_sg_total, dim3(1), dim3(256), 0, s, loss_per_map, (int)N, loss_total);
}

int reni_sh_project(int64_t N, int64_t H, int64_t W, int64_t lmax, const float* img, const float* row_table,
                    const float* col_table, float* coeffs, void* stream) {
  if (int rc = sh_check(N, H, W, lmax)) return rc;
  if (!img || !row_table || !col_table || !coeffs) return reni_set_error(RENI_EINVAL, "sh project: NULL argument");
  reni::ShArgs a;
  a.N = (int)N; a.H = (int)H; a.W = (int)W; a.T = (int)((lmax + 1) * (lmax + 1));
  a.row = row_table; a.col = col_table; a.in = img; a.out = coeffs;
  const dim3 grid((unsigned)((3 * N + 31) / 32));
  hipStream_t s = (hipStream_t)stream;
  if (a.T <= 32) return tu_launch(TU_PLAIN, reni::k_sh_project<1>, grid, dim3(64), 0, s, a);
  if (a.T <= 64) return tu_launch(TU_PLAIN, reni::k_sh_project<2>, grid, dim3(64), 0, s, a);
  if (a.T <= 128) return tu_launch(TU_PLAIN, reni::k_sh_project<4>, grid, dim3(64), 0, s, a);
  return tu_launch(TU_PLAIN, reni::k_sh_project<8>, grid, dim3(64), 0, s, a);
}

int reni_sh_reconstruct(int64_t N, int64_t H, int64_t W, int64_t lmax, const float* coeffs, const float* row_table,
                        const float* col_table, float* out, void* stream) {
  if (int rc = sh_check(N, H, W, lmax)) return rc;
  if (!coeffs || !row_table || !col_table || !out) return reni_set_error(RENI_EINVAL, "sh reconstruct: NULL argument");
  reni::ShArgs a;
  a.N = (int)N; a.H = (int)H; a.W = (int)W; a.T = (int)((lmax + 1) * (lmax + 1));
  a.row = row_table; a.col = col_table; a.in = coeffs; a.out = out;
  const int64_t Q = H * W;
  const dim3 grid((unsigned)((3 * N + 31) / 32), (unsigned)((Q + 32 * reni::SH_QT - 1) / (32 * reni::SH_QT)));
  return tu_launch(TU_PLAIN, reni::k_sh_reconstruct, grid, dim3(64), 0, (hipStream_t)stream, a);
}

}  // extern "C"
