// translation unit of libreni_hip.so: environment maps as glossy lighting -- the convolution of maps with a chain of zonal
// specular lobes, and the lookup of maps or of such a chain at arbitrary directions (reni_amd/glossy.py).  No reference
// counterpart: the reference lights glossy surfaces with its per-pixel Blinn-Phong shader only (reni_tu_shade.hip).
//
// fp32 throughout, no float atomics: every sum runs in a fixed order that depends on (P, Q) only, so two calls give identical
// bits, a map's results do not depend on the batch around it, and a lobe's results do not depend on the lobes that share the
// call.  Contraction is off for the whole unit: what is written is what runs.
//
//   k_lobe_convolve<KIND, CT>  part[s][l][col][o] = sum_(i in chunk s) f_l(o . d_i) (w_i scale) B[i][col], the GEMM of
//                       k_diffuse_convolve (reni_tu_diffuse.hip: same tiles, same i split, same v_mfma_f32_32x32x2_f32 chain;
//                       tiles, split, row map, drain and the k-step are reni_sphere.inc's)
//                       with another A generator: t = fma(oz, dz, fma(oy, dy, ox dx)), then the lobe, one straight-line
//                       generator per KIND with the lobe's parameter a uniform argument.  B's columns are the batch's 3 N
//                       colour columns and, when the call normalises, ONE column of ones behind them: the denominator
//                       sum_i f_l w_i comes out of the same chain once per (lobe, o), not once per map.  blockIdx.z is
//                       (lobe of this kind, split): a lobe never shares a workgroup with another.
//   k_lobe_finish       out[n][l][o][c] = ((part_0 + part_1) + ...) of column 3 n + c, divided by the same sum of the
//                       column of ones when normalising (0 where that sum is not positive).  The division sits here and
//                       not behind the MFMAs: arithmetic on the accumulators makes hipcc copy them ahead of the drain pad.
//   k_lobe_den_finish   den[l][o] = the same sum of the column of ones of a call WITHOUT maps (reni_lobe_denominators: the
//                       forward's own launch, so the bits the forward divided by), for the transpose in
//                       reni_tu_glossy_bwd.hip.
//   k_envmap_lookup     out[n][p][c] = the bilinear sample of src[n][level][.][.][c] at direction dirs[p] (or dirs[n][p]),
//                       mixed linearly between floor(level) and the next level.  Direction -> (row, col), the four taps and
//                       the level are reni_sphere.inc's (sph_rowcol, sph_taps, sph_level), the functions k_rotate_envmap,
//                       k_envmap_lookup_taps and k_envmap_lookup_dquery call.  One lane per direction computes the
//                       coordinate once and serves the channels and both levels with it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#include "reni_sphere.inc"  // GEMM pieces, lobes, split rule, (row, col), taps, level, query: shared with reni_tu_glossy_bwd.hip

namespace reni {

struct LbArgs {
  int N, P, Q;
  int ncol;               // 3 N, plus the column of ones when normalising
  const float* out_dirs;  // [P][3]
  const float* in_dirs;   // [Q][3]
  const float* in_w;      // [Q]
  const float* src;       // element (n, i, c) at n sn + i si + c sc
  int64_t sn, si, sc;
  float scale;
  int chunk;  // i per split (even)
  int S;      // splits
  int Lv;     // lobes of the call
  int nl;     // lobes of this launch (one kind)
  int lobe[LB_MAX_LOBES];   // their index in the call
  float par[LB_MAX_LOBES];  // PHONG: n; BLINN: s / 2; GGX: alpha^2
  float* ws;                // [S][Lv][ncol][P] partial sums
};

template <int KIND, int CT>
__global__ void __launch_bounds__(256) k_lobe_convolve(const LbArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, hi = lane >> 5;
  const int ll = (int)blockIdx.z / a.S, sp = (int)blockIdx.z - ll * a.S;  // lobe of this launch, split
  const DgLobe<KIND> lobe = {a.par[ll]};
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
  bool cok[CT], img[CT];
  float fill[CT];  // what a lane feeds in place of a map's value: 1 in the column of ones, 0 beyond the last column
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    cok[v] = col < a.ncol;
    img[v] = col < 3 * (int64_t)a.N;
    fill[v] = cok[v] && !img[v] ? 1.f : 0.f;  // (col == 3 N < ncol only when normalising)
    const int64_t n = img[v] ? col / 3 : 0;
    const int64_t c = img[v] ? col - 3 * n : 0;
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
  // accumulators are stored as they are.
  const int ilo = sp * a.chunk;
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
      b[v] = iok ? (img[v] ? x : fill[v]) : 0.f;  // (every lane loads: map 0 where there is no map, the value dropped)
    }
    dg_kstep(ox, oy, oz, dx, dy, dz, w, b, lobe, acc);
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
  float* dst = a.ws + ((int64_t)sp * a.Lv + a.lobe[ll]) * a.ncol * a.P;
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    if (!cok[v]) continue;
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    float* op = dst + col * a.P;
#pragma unroll
    for (int u = 0; u < DG_OT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t o = o0 + u * 32 + mfma_rowmap(r, hi);
        if (o < a.P) op[o] = acc[u][v][r];
      }
  }
}

// one lane per (lobe, map, o): the partial sums of a column in split order, then the division
__global__ void __launch_bounds__(256) k_lobe_finish(const float* __restrict__ ws, int N, int Lv, int P, int ncol, int S,
                                                     int normalise, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)Lv * N * P) return;
  const int64_t o = e % P, ln = e / P;
  const int64_t n = ln % N, l = ln / N;
  const int64_t slab = (int64_t)Lv * ncol * P;
  const float* base = ws + l * ncol * P + o;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = base + (3 * n + c) * P;
    float x = p[0];
    for (int s = 1; s < S; ++s) x += p[(int64_t)s * slab];
    v[c] = x;
  }
  if (normalise) {
    const float* p = base + 3 * (int64_t)N * P;
    float den = p[0];
    for (int s = 1; s < S; ++s) den += p[(int64_t)s * slab];
    const bool ok = den > 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ok ? v[c] / den : 0.f;
  }
  float* q = out + ((n * Lv + l) * P + o) * 3;
  q[0] = v[0];
  q[1] = v[1];
  q[2] = v[2];
}

// one lane per (lobe, o): the partial sums of the column of ones of a call without maps, in split order
__global__ void __launch_bounds__(256) k_lobe_den_finish(const float* __restrict__ ws, int Lv, int P, int S, float* __restrict__ den) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t slab = (int64_t)Lv * P;
  if (e >= slab) return;
  float x = ws[e];
  for (int s = 1; s < S; ++s) x += ws[(int64_t)s * slab + e];
  den[e] = x;
}

struct LkArgs : SphQuery {
  float* out;  // [N][P][3]
};

__global__ void __launch_bounds__(256) k_envmap_lookup(const LkArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;  // P < 2^30
  if (p >= a.P) return;
  const int64_t n = blockIdx.y;
  const float* d = a.dirs + n * a.dn + 3 * (int64_t)p;
  const float sx = d[0], sy = d[1], sz = d[2];
  float row, col;
  sph_rowcol(sx, sy, sz, a.H, a.W, a.row_scale, a.col_scale, a.col_bias, row, col);
  const SphTaps t = sph_taps(row, col, a.H, a.W);
  const float fr = t.fr, gr = t.gr, fc = t.fc, gc = t.gc;
  const int64_t r0 = (int64_t)t.i0 * (int64_t)a.sy, r1 = (int64_t)t.i1 * (int64_t)a.sy;
  const int64_t o00 = r0 + (int64_t)t.j00 * (int64_t)a.sx, o01 = r0 + (int64_t)t.j01 * (int64_t)a.sx;
  const int64_t o10 = r1 + (int64_t)t.j10 * (int64_t)a.sx, o11 = r1 + (int64_t)t.j11 * (int64_t)a.sx;
  // ---- the level: clamped to [0, Lv - 1] (fmaxf drops a NaN), one more lerp in the same fma order
  const SphLevel L = sph_level(a.level ? a.level[n * a.ln + p] : a.level_const, a.Lv);
  const int l0 = L.l0, l1 = L.l1;
  const float fl = L.fl, gl = L.gl;
  const float* b0 = a.src + n * a.sn + (int64_t)l0 * a.sl;
  const float* b1 = a.src + n * a.sn + (int64_t)l1 * a.sl;
  float* o = a.out + (n * a.P + p) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch, b0 += a.sc, b1 += a.sc) {
    const float top = fmaf(fc, b0[o01], gc * b0[o00]);
    const float bot = fmaf(fc, b0[o11], gc * b0[o10]);
    float v = fmaf(fr, bot, gr * top);
    if (fl > 0.f) {  // (fl == 0 would give the same bits for finite maps: fma(0, v1, 1 v))
      const float top1 = fmaf(fc, b1[o01], gc * b1[o00]);
      const float bot1 = fmaf(fc, b1[o11], gc * b1[o10]);
      v = fmaf(fl, fmaf(fr, bot1, gr * top1), gl * v);
    }
    o[ch] = v;
  }
}

}  // namespace reni

namespace {

using reni::reni_set_error;

int64_t lb_ws_bytes(int64_t N, int64_t P, int64_t Q, int64_t Lv) {
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  return S * Lv * (3 * N + 1) * P * (int64_t)sizeof(float);
}

template <int KIND>
int lb_launch(TuCount count, const reni::LbArgs& a, hipStream_t s) {
  const unsigned gx = (unsigned)((a.P + reni::DG_ROWS - 1) / reni::DG_ROWS), gz = (unsigned)(a.nl * a.S);
  if (a.ncol <= 32) return tu_launch(count, reni::k_lobe_convolve<KIND, 1>, dim3(gx, 1, gz), dim3(256), 0, s, a);
  return tu_launch(count, reni::k_lobe_convolve<KIND, 2>, dim3(gx, (unsigned)((a.ncol + 63) / 64), gz), dim3(256), 0, s, a);
}

// one launch per kind present, its lobes along z; counted or not as the caller's other launches are
int lb_launch_kinds(TuCount count, reni::LbArgs& a, int n_lobes, const int32_t* kinds, const float* params, hipStream_t s) {
  return lb_for_kinds(a, n_lobes, kinds, params, [&](int kind, const reni::LbArgs& a) {
    return kind == RENI_LOBE_PHONG   ? lb_launch<RENI_LOBE_PHONG>(count, a, s)
           : kind == RENI_LOBE_BLINN ? lb_launch<RENI_LOBE_BLINN>(count, a, s)
                                     : lb_launch<RENI_LOBE_GGX>(count, a, s);
  });
}

bool lb_den_shape_ok(int64_t P, int64_t Q, int64_t Lv) {
  return P >= 1 && Q >= 1 && Lv >= 1 && Lv <= reni::LB_MAX_LOBES && P <= DG_MAX_ELEMS / 3 && Q <= DG_MAX_ELEMS / 3 &&
         P <= DG_MAX_ELEMS / (3 * Lv);
}

}  // namespace

extern "C" {

size_t reni_lobe_workspace_bytes(int64_t N, int64_t P, int64_t Q, int64_t n_lobes) {
  if (!lb_shape_ok(N, P, Q, n_lobes)) return 0;
  return (size_t)lb_ws_bytes(N, P, Q, n_lobes) + 256;
}

int reni_lobe_convolve(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                       const float* src, int64_t src_stride_n, int64_t src_stride_i, int64_t src_stride_c, int n_lobes,
                       const int32_t* kinds, const float* params, int normalise, float scale, float* out, void* ws,
                       size_t ws_bytes, void* stream) {
  if (n_lobes < 1 || n_lobes > reni::LB_MAX_LOBES) return reni_set_error(RENI_EINVAL, "lobe convolve: need 1 <= n_lobes <= 16");
  if (!lb_shape_ok(N, P, Q, n_lobes))
    return reni_set_error(RENI_EINVAL, "lobe convolve: need N, P, Q >= 1 and n_lobes N P, Q < 2^28");
  if (!out_dirs || !in_dirs || !in_w || !src || !out || !kinds || !params)
    return reni_set_error(RENI_EINVAL, "lobe convolve: NULL argument");
  if (int rc = lb_check_lobes(n_lobes, kinds, params)) return rc;
  if (src_stride_n < 0 || src_stride_i < 0 || src_stride_c < 0)
    return reni_set_error(RENI_EINVAL, "lobe convolve: src strides must be >= 0");
  if (int rc = tu_check_ws("lobe convolve", ws, ws_bytes, (size_t)lb_ws_bytes(N, P, Q, n_lobes))) return rc;
  reni::LbArgs a = {};
  a.N = (int)N; a.P = (int)P; a.Q = (int)Q;
  a.ncol = (int)(3 * N + (normalise ? 1 : 0));
  a.out_dirs = out_dirs; a.in_dirs = in_dirs; a.in_w = in_w;
  a.src = src; a.sn = src_stride_n; a.si = src_stride_i; a.sc = src_stride_c;
  a.scale = normalise ? 1.f : scale;  // a normalised result does not depend on the scale
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  a.chunk = (int)chunk; a.S = (int)S; a.Lv = n_lobes;
  a.ws = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = lb_launch_kinds(TU_PLAIN, a, n_lobes, kinds, params, s)) return rc;
  const int64_t total = (int64_t)n_lobes * N * P;
  return tu_launch(TU_PLAIN, reni::k_lobe_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.ws, (int)N, n_lobes, (int)P,
                   a.ncol, (int)S, normalise ? 1 : 0, out);
}

size_t reni_lobe_denominators_workspace_bytes(int64_t P, int64_t Q, int64_t n_lobes) {
  if (!lb_den_shape_ok(P, Q, n_lobes)) return 0;
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  return (size_t)(S * n_lobes * P * (int64_t)sizeof(float)) + 256;
}

int reni_lobe_denominators(int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w, int n_lobes,
                           const int32_t* kinds, const float* params, float* den, void* ws, size_t ws_bytes, void* stream) {
  if (n_lobes < 1 || n_lobes > reni::LB_MAX_LOBES) return reni_set_error(RENI_EINVAL, "lobe convolve: need 1 <= n_lobes <= 16");
  if (!lb_den_shape_ok(P, Q, n_lobes))
    return reni_set_error(RENI_EINVAL, "lobe denominators: need P, Q >= 1 and n_lobes P, Q < 2^28");
  if (!out_dirs || !in_dirs || !in_w || !den || !kinds || !params)
    return reni_set_error(RENI_EINVAL, "lobe denominators: NULL argument");
  if (int rc = lb_check_lobes(n_lobes, kinds, params)) return rc;
  int64_t S, chunk;
  dg_split(P, Q, S, chunk);
  if (int rc = tu_check_ws("lobe denominators", ws, ws_bytes, (size_t)(S * n_lobes * P * (int64_t)sizeof(float)))) return rc;
  // the forward's own launch without maps: the column of ones is column 0 of one 32-column group, and a column's sums do not
  // depend on the columns beside it.  The kernel loads a map's value in every lane and drops it where there is no map: in_w
  // stands in for the maps it reads ([Q] floats, texel stride 1).
  reni::LbArgs a = {};
  a.N = 0; a.P = (int)P; a.Q = (int)Q;
  a.ncol = 1;
  a.out_dirs = out_dirs; a.in_dirs = in_dirs; a.in_w = in_w;
  a.src = in_w; a.sn = 0; a.si = 1; a.sc = 0;
  a.scale = 1.f;
  a.chunk = (int)chunk; a.S = (int)S; a.Lv = n_lobes;
  a.ws = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = lb_launch_kinds(TU_COUNTED, a, n_lobes, kinds, params, s)) return rc;
  return tu_launch(TU_COUNTED, reni::k_lobe_den_finish, dim3((unsigned)((n_lobes * P + 255) / 256)), dim3(256), 0, s, a.ws, n_lobes,
                   (int)P, (int)S, den);
}

int reni_envmap_lookup(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src, const int64_t src_strides[5],
                       const float* dirs, int64_t dirs_stride_n, const float* level, int64_t level_stride_n, float level_const,
                       float* out, void* stream) {
  if (int rc = sph_check_query(true, N, Lv, H, W, P, src, src_strides, dirs, dirs_stride_n, level, level_stride_n, out != nullptr))
    return rc;
  reni::LkArgs a = {};
  sph_fill_query(a, N, Lv, H, W, P, src, src_strides, dirs, dirs_stride_n, level, level_stride_n, level_const);
  a.out = out;
  return tu_launch(TU_PLAIN, reni::k_envmap_lookup, dim3((unsigned)((P + 255) / 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
}

}  // extern "C"
