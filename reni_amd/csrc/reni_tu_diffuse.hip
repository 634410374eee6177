// translation unit of libreni_hip.so: diffuse irradiance of environment maps -- the brute-force clamped-cosine convolution
// and the Ramamoorthi-Hanrahan L2 SH irradiance.
//
// Reference: src/models/spherical_harmonics.py (getDiffuseMap :383-437, shRenderL2 :485-505).  fp32 throughout, no float
// atomics: every sum runs in a fixed order that depends on (P, Q) only, so two calls give identical bits and a map's results
// do not depend on the batch around it.
//
//   k_diffuse_convolve  out[(o)][(n, c)] = sum_i A[o][i] src[n][i][c], A[o][i] = max(0, n_o . d_i) (w_i scale): a GEMM whose A operand
//                       is generated on the VALU (one fixed fmaf order) and never stored.  fp32 MFMA v_mfma_f32_32x32x2_f32,
//                       whose result is bitwise a k-ordered fmaf chain.  A wave owns DG_OT x 32 output rows and CT x 32
//                       (n, c) columns; the four waves of a workgroup share the columns (their src reads hit the same lines).
//                       blockIdx.z splits the i range into S chunks, S a function of (P, Q) only (dg_split); with S > 1 the
//                       partial sums go to the workspace and k_diffuse_reduce adds them in split order.
//                       Tile constants, result-row map, drain, split rule and the k-step are reni_sphere.inc's, shared with
//                       the lobe convolution and its transpose; the rest of the body is written out here as it is there.
//   k_diffuse_reduce    out = ((part_0 + part_1) + part_2) + ...
//   k_sh_irradiance_l2  shRenderL2 per (map, pixel), the reference's term order and constants, then / pi.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#include "reni_sphere.inc"  // tile constants, result-row map, drain, split rule, k-step

namespace reni {

struct DfArgs {
  int N, P, Q;  // N P, Q < 2^28
  const float* out_dirs;  // [P][3]
  const float* in_dirs;   // [Q][3]
  const float* in_w;      // [Q]
  const float* src;       // element (n, i, c) at n sn + i si + c sc
  int64_t sn, si, sc;
  float scale;
  int chunk;       // i per split (even)
  float* out;     // [N][P][3]
  float* ws;      // [S][N][P][3] partial sums when S > 1
};

template <int CT>
__global__ void __launch_bounds__(256) k_diffuse_convolve(const DfArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, hi = lane >> 5;
  const int64_t ncol = 3 * a.N;
  const int64_t o0 = (int64_t)blockIdx.x * DG_ROWS + wave * (32 * DG_OT);
  float ox[DG_OT], oy[DG_OT], oz[DG_OT];
#pragma unroll
  for (int u = 0; u < DG_OT; ++u) {
    const int64_t o = o0 + u * 32 + j;
    const bool ok = o < a.P;
    ox[u] = ok ? a.out_dirs[3 * o] : 0.f;
    oy[u] = ok ? a.out_dirs[3 * o + 1] : 0.f;
    oz[u] = ok ? a.out_dirs[3 * o + 2] : 0.f;
  }
  const float* colp[CT];
  bool cok[CT];
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    cok[v] = col < ncol;
    const int64_t n = cok[v] ? col / 3 : 0;
    const int64_t c = cok[v] ? col - 3 * n : 0;
    colp[v] = a.src + n * a.sn + c * a.sc;
  }
  mfma_f32x16 acc[DG_OT][CT];
#pragma unroll
  for (int u = 0; u < DG_OT; ++u)
#pragma unroll
    for (int v = 0; v < CT; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;
  // i = i0 + hi: lanes 0..31 feed k = 0 of the MFMA, lanes 32..63 k = 1.  The scale is folded into the weight, so the
  // accumulators are stored as they are (an epilogue multiply would copy them out of the AGPRs ahead of the drain).
  const int ilo = (int)blockIdx.z * a.chunk;
  const int ihi = ilo + a.chunk < a.Q ? ilo + a.chunk : a.Q;
  const float* dp = a.in_dirs + 3 * (int64_t)(ilo + hi);
  const float* wp = a.in_w + ilo + hi;
  const int64_t bstep = 2 * a.si;
#pragma unroll
  for (int v = 0; v < CT; ++v) colp[v] += (int64_t)(ilo + hi) * a.si;
  // one k-step; iok false zeroes both operands of the lanes of i == ihi (the tail of an odd range)
  auto step = [&](const bool iok) __attribute__((always_inline)) {
    const float dx = dp[0], dy = dp[1], dz = dp[2];
    const float w = iok ? wp[0] * a.scale : 0.f;
    float b[CT];
#pragma unroll
    for (int v = 0; v < CT; ++v) {
      const float x = *colp[v];
      b[v] = cok[v] && iok ? x : 0.f;
    }
    dg_kstep(ox, oy, oz, dx, dy, dz, w, b, DgCosine(), acc);
  };
  int i0 = ilo;
  for (; i0 + 1 < ihi; i0 += 2) {
    step(true);
    dp += 6;
    wp += 2;
#pragma unroll
    for (int v = 0; v < CT; ++v) colp[v] += bstep;
  }
  if (i0 < ihi) {  // odd range: the lanes of i0 + 1 re-read i0 and contribute zero
    dp -= 3 * hi;
    wp -= hi;
#pragma unroll
    for (int v = 0; v < CT; ++v) colp[v] -= hi * a.si;
    step(hi == 0);
  }
  mfma_drain();
  const bool split = gridDim.z > 1;
  float* dst = split ? a.ws + (int64_t)blockIdx.z * ncol * a.P : a.out;
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    if (!cok[v]) continue;
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    const int64_t n = col / 3, c = col - 3 * n;
    float* op = dst + n * 3 * a.P + c;
#pragma unroll
    for (int u = 0; u < DG_OT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t o = o0 + u * 32 + mfma_rowmap(r, hi);
        if (o < a.P) op[3 * o] = acc[u][v][r];
      }
  }
}

__global__ void __launch_bounds__(256) k_diffuse_reduce(const float* __restrict__ ws, int64_t total, int S,
                                                        float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float v = ws[e];
  for (int s = 1; s < S; ++s) v += ws[(int64_t)s * total + e];
  out[e] = v;
}

// shRenderL2 (Ramamoorthi & Hanrahan 2001) with the reference's constants and term order, including its - C5 L6 term
__global__ void __launch_bounds__(256) k_sh_irradiance_l2(int64_t N, int64_t P, const float* __restrict__ coeffs,
                                                          const float* __restrict__ normals, int64_t nstride,
                                                          float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * P) return;
  const int64_t n = e / P, p = e - n * P;
  const float* nv = normals + n * nstride + 3 * p;
  const float x = nv[0], y = nv[1], z = nv[2];
  const float C1 = 0.429043f, C2 = 0.511664f, C3 = 0.743125f, C4 = 0.886227f, C5 = 0.247708f;
  const float inv_pi = (float)(1.0 / M_PI);
  const float* L = coeffs + n * 27;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float r = C4 * L[c];
    r += 2.f * C2 * L[9 + c] * x;
    r += 2.f * C2 * L[3 + c] * y;
    r += 2.f * C2 * L[6 + c] * z;
    r += C1 * L[24 + c] * (x * x - y * y);
    r += C3 * L[18 + c] * z * z;
    r -= C5 * L[18 + c];
    r += 2.f * C1 * L[12 + c] * x * y;
    r += 2.f * C1 * L[21 + c] * x * z;
    r += 2.f * C1 * L[15 + c] * y * z;
    out[3 * e + c] = r * inv_pi;
  }
}

}  // namespace reni

namespace {

using reni::reni_set_error;

bool df_shape_ok(int64_t N, int64_t P, int64_t Q) {
  return N >= 1 && P >= 1 && Q >= 1 && P <= DG_MAX_ELEMS / 3 && Q <= DG_MAX_ELEMS / 3 && N <= DG_MAX_ELEMS / (3 * P) &&
         (3 * N + 31) / 32 <= 65535;
}

int64_t df_ws_bytes(int64_t N, int64_t P, int64_t Q) {
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  return S > 1 ? S * 3 * N * P * (int64_t)sizeof(float) : 0;
}

}  // namespace

extern "C" {

size_t reni_diffuse_workspace_bytes(int64_t N, int64_t P, int64_t Q) {
  if (!df_shape_ok(N, P, Q)) return 0;
  const int64_t b = df_ws_bytes(N, P, Q);
  return b ? (size_t)b + 256 : 0;
}

int reni_diffuse_convolve(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                          const float* src, int64_t src_stride_n, int64_t src_stride_i, int64_t src_stride_c, float scale,
                          float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!df_shape_ok(N, P, Q)) return reni_set_error(RENI_EINVAL, "diffuse convolve: need N, P, Q >= 1 and N P, Q < 2^28");
  if (!out_dirs || !in_dirs || !in_w || !src || !out) return reni_set_error(RENI_EINVAL, "diffuse convolve: NULL argument");
  if (src_stride_n < 0 || src_stride_i < 0 || src_stride_c < 0)
    return reni_set_error(RENI_EINVAL, "diffuse convolve: src strides must be >= 0");
  reni::DfArgs a = {};
  a.N = (int)N; a.P = (int)P; a.Q = (int)Q;
  a.out_dirs = out_dirs; a.in_dirs = in_dirs; a.in_w = in_w;
  a.src = src; a.sn = src_stride_n; a.si = src_stride_i; a.sc = src_stride_c;
  a.scale = scale; a.out = out;
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  a.chunk = (int)chunk;
  if (S > 1) {
    if (int rc = tu_check_ws("diffuse convolve", ws, ws_bytes, (size_t)df_ws_bytes(N, P, Q))) return rc;
    a.ws = (float*)ws;
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)((P + reni::DG_ROWS - 1) / reni::DG_ROWS);
  const bool one = 3 * N <= 32;  // one 32-column group per workgroup, else two
  const dim3 grid(gx, (unsigned)(one ? (3 * N + 31) / 32 : (3 * N + 63) / 64), (unsigned)S);
  if (int rc = tu_launch(TU_PLAIN, one ? reni::k_diffuse_convolve<1> : reni::k_diffuse_convolve<2>, grid, dim3(256), 0, s, a)) return rc;
  if (S == 1) return RENI_OK;
  const int64_t total = 3 * N * P;
  return tu_launch(TU_PLAIN, reni::k_diffuse_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.ws, total, (int)S, out);
}

int reni_sh_irradiance_l2(int64_t N, int64_t P, const float* coeffs, const float* normals, int64_t normals_stride_n, float* out,
                          void* stream) {
  if (N < 1 || P < 1 || P > DG_MAX_ELEMS / 3 || N > DG_MAX_ELEMS / (3 * P))
    return reni_set_error(RENI_EINVAL, "sh irradiance: need N, P >= 1 and N P < 2^28");
  if (normals_stride_n != 0 && normals_stride_n != 3 * P)
    return reni_set_error(RENI_EINVAL, "sh irradiance: the normals' map stride must be 0 (shared) or 3 P (per map)");
  if (!coeffs || !normals || !out) return reni_set_error(RENI_EINVAL, "sh irradiance: NULL argument");
  return tu_launch(TU_PLAIN, reni::k_sh_irradiance_l2, dim3((unsigned)((N * P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, P,
                   coeffs, normals, normals_stride_n, out);
}

}  // extern "C"
