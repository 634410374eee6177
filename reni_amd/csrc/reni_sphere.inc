// reni_sphere.inc -- the ONE definition of what the environment-map units share:
//   * the 32x32 MFMA result-row map and the drain pads (the SH kernels of reni_tu_baselines.hip and the direction GEMMs);
//   * of the direction GEMM (k_diffuse_convolve, k_lobe_convolve, k_lobe_convolve_t): tile constants, lobe generators, the
//     k-step (dot order, generator, per-k scalar, MFMA chain), and on the host the split rule, limits, the lobes' argument
//     checks and the loop over the kinds of a call.  The row-direction load, the accumulator clear, the k-pair loop with
//     its odd tail, the pointer advances, the drain and the store stay written out in each kernel: shared forms of them
//     cost registers or occupancy, or moved the listing and were not at or below the previous library's times (DESIGN 4.4h);
//   * of the equirectangular lookup (k_rotate_envmap, k_envmap_lookup, k_envmap_lookup_taps, k_envmap_lookup_dquery):
//     direction -> (row, col), the taps of the sphere (fractions, pole fold, seam wrap), the level interpolation, and on the
//     host the query record with its checks and its fill.  Each kernel keeps its own address form.
// Included at file scope, outside every namespace, behind reni_tu_host.inc.  Every function here that rounds switches
// contraction off for itself, so what is written is what runs whatever the including unit compiles with (the lobe generators
// hold no a * b + c outside fmaf).
#pragma once

#ifndef DEV
#define DEV __device__ __forceinline__
#endif

namespace reni {

// ---- MFMA result rows and drain --------------------------------------------------------------------------------------
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));

DEV constexpr int mfma_rowmap(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }  // 32x32 MFMA result row

#define MFMA_DRAIN_PAD "s_nop 15\n\ts_nop 3"  // 16-pass XDL write-back: 18 states (+2)

DEV void mfma_drain() {  // wait out the last MFMA's write-back (18 states) before its result is read
  __builtin_amdgcn_sched_barrier(0);
  asm volatile(MFMA_DRAIN_PAD);
  __builtin_amdgcn_sched_barrier(0);
}

// ---- direction GEMM ----------------------------------------------------------------------------------------------------
constexpr int DG_OT = 2;     // 32-row output tiles per wave
constexpr int DG_WAVES = 4;  // waves per workgroup, each its own output rows
constexpr int DG_ROWS = 32 * DG_OT * DG_WAVES;
constexpr int LB_MAX_LOBES = 16;

// mfma_drain with the accumulators tied to the pad: behind the transpose's loop over the lobes hipcc would otherwise copy them
// out of the AGPRs ahead of it, one wait state short of the write-back on the path that leaves the loop
template <int CT>
DEV void mfma_drain_tied(mfma_f32x16 (&acc)[DG_OT][CT]) {
  static_assert(DG_OT == 2 && (CT == 1 || CT == 2), "one operand per accumulator tile");
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (CT == 1) {
    asm volatile(MFMA_DRAIN_PAD : "+a"(acc[0][0]), "+a"(acc[1][0]));
  } else {
    asm volatile(MFMA_DRAIN_PAD : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));
  }
  __builtin_amdgcn_sched_barrier(0);
}

// ---- zonal lobes -------------------------------------------------------------------------------------------------------
DEV float lb_clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, 1.f); }
// b^p = exp2(p log2 b) on the hardware's v_log_f32 / v_exp_f32 (1 ulp each); b = 0: log2 = -inf, p > 0, exp2 = 0
DEV float lb_pow(float b, float p) { return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(b)); }

template <int KIND>
DEV float lb_lobe(float t, float p);
template <>
DEV float lb_lobe<RENI_LOBE_PHONG>(float t, float p) { return lb_pow(lb_clamp01(t), p); }
template <>
DEV float lb_lobe<RENI_LOBE_BLINN>(float t, float p) { return lb_pow(lb_clamp01(fmaf(t, 0.5f, 0.5f)), p); }
template <>
DEV float lb_lobe<RENI_LOBE_GGX>(float t, float p) {
  // m (a2 - 1) + 1 written as fma(m, a2, 1 - m): 1 - m is exact for m >= 1/2, where the sum cancels.  a2 / d^2 as
  // ((a2 r) r) with r = 1 / d <= 1 / a2, so that no intermediate leaves the normal range for a2 >= 2^-60
  const float m = lb_clamp01(fmaf(t, 0.5f, 0.5f));
  const float r = __builtin_amdgcn_rcpf(fmaf(m, p, 1.f - m));
  return ((p * r) * r) * lb_clamp01(t);
}

// the A generators of the direction GEMM: t = row direction . k-side direction -> the kernel matrix's entry
struct DgCosine {  // max(0, t): diffuse irradiance
  DEV float operator()(float t) const { return fmaxf(t, 0.f); }
};
template <int KIND>
struct DgLobe {
  float par;
  DEV float operator()(float t) const { return lb_lobe<KIND>(t, par); }
};

// one k-step of a wave: t = fma(z, kz, fma(y, ky, x kx)) per row tile, then gen(t) times the per-k scalar s as the A operand
// of the v_mfma_f32_32x32x2_f32 chain over the CT column tiles.  The two forwards (rows o, k-side d_i) call it; the transpose
// (rows d_i, k-side o: k_lobe_convolve_t) keeps a copy in the same order, so that both directions use one kernel matrix up to
// the generator's rounding (DESIGN 4.4h has why it is a copy)
template <int CT, class GEN>
DEV void dg_kstep(const float (&x)[DG_OT], const float (&y)[DG_OT], const float (&z)[DG_OT], float kx, float ky, float kz, float s,
                  const float (&b)[CT], const GEN gen, mfma_f32x16 (&acc)[DG_OT][CT]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int u = 0; u < DG_OT; ++u) {
    float t = x[u] * kx;
    t = fmaf(y[u], ky, t);
    t = fmaf(z[u], kz, t);
    const float av = gen(t) * s;
#pragma unroll
    for (int v = 0; v < CT; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[v], acc[u][v], 0, 0, 0);
  }
}

// ---- equirectangular maps ----------------------------------------------------------------------------------------------
// direction -> continuous (row, col) of the H x W grid: phi = atan2f(sqrtf(fma(s.z, s.z, s.x s.x)), s.y), theta =
// atan2f(s.x, -s.z), row = fma(phi, row_scale, -1/2), col = fma(theta, col_scale, col_bias).  atan2f needs no unit length; the
// zero vector gives phi = atan2f(0, 0) = 0, a finite theta and so the first row.  The clamps change nothing for finite
// directions (0 <= phi <= fp32(pi), |theta| <= fp32(pi)); they keep a NaN or an overflow from becoming an address.
DEV void sph_rowcol(float sx, float sy, float sz, int H, int W, float row_scale, float col_scale, float col_bias, float& row,
                    float& col) {
#pragma clang fp contract(off)
  const float phi = atan2f(sqrtf(fmaf(sz, sz, sx * sx)), sy);
  const float theta = atan2f(sx, -sz);
  row = fminf(fmaxf(fmaf(phi, row_scale, -0.5f), -1.f), (float)H);
  col = fminf(fmaxf(fmaf(theta, col_scale, col_bias), -1.f), (float)W);
}

// the taps of the sphere at a continuous (row, col) of sph_rowcol: i = floor(row), fr = row - i (exact), gr = 1 - fr, likewise
// j, fc, gc.  A row beyond a pole is the same row seen from the other side (column + W / 2, W even); columns modulo W.  i0, i1
// are the folded rows (the clamp acts for H == 1 with both poles crossed only), jRC the column of the tap in row R (0: i0,
// 1: i1), column C (0: j, 1: j + 1).  -1 <= i <= H and -1 <= j <= W by sph_rowcol's clamps.  The nearest tap of (row, col) is
// tap (i0, j00) of (row + 1/2, col + 1/2).
struct SphTaps {
  float fr, gr, fc, gc;
  int i0, i1;
  int j00, j01, j10, j11;
};

DEV SphTaps sph_taps(float row, float col, int H, int W) {
#pragma clang fp contract(off)
  SphTaps t;
  const float fi = floorf(row), fj = floorf(col);
  const int i = (int)fi, j = (int)fj;
  t.fr = row - fi, t.fc = col - fj;
  t.gr = 1.f - t.fr, t.gc = 1.f - t.fc;
  const int half = W >> 1;
  int i0 = i, i1 = i + 1;
  const bool x0 = i0 < 0 || i0 >= H, x1 = i1 >= H;  // beyond a pole: the far side
  if (i0 < 0) i0 = -1 - i0;
  if (i0 >= H) i0 = 2 * H - 1 - i0;
  if (i1 >= H) i1 = 2 * H - 1 - i1;
  t.i0 = min(max(i0, 0), H - 1);
  t.i1 = min(max(i1, 0), H - 1);
  int j0 = j < 0 ? j + W : (j >= W ? j - W : j);
  int j1 = j + 1 >= W ? j + 1 - W : j + 1;
  if (j1 >= W) j1 -= W;
  const int j0f = j0 + half >= W ? j0 - half : j0 + half, j1f = j1 + half >= W ? j1 - half : j1 + half;
  t.j00 = x0 ? j0f : j0, t.j01 = x0 ? j1f : j1;
  t.j10 = x1 ? j0f : j0, t.j11 = x1 ? j1f : j1;
  return t;
}

// the level of a lookup: clamped to [0, Lv - 1] (fmaxf drops a NaN), l0 = floor, fl the fraction, gl = 1 - fl.  The next
// level l1 is read, and so weighs, only when fl > 0 (the callers' test): fl == 0 gives the same bits for finite maps only.
struct SphLevel {
  int l0, l1;
  float fl, gl;
};

DEV SphLevel sph_level(float lv, int Lv) {
#pragma clang fp contract(off)
  lv = fminf(fmaxf(lv, 0.f), (float)(Lv - 1));
  const float fl0 = floorf(lv);
  SphLevel t;
  t.l0 = (int)fl0, t.l1 = min(t.l0 + 1, Lv - 1);
  t.fl = lv - fl0, t.gl = 1.f - t.fl;
  return t;
}

// the query of a lookup, as its kernels' argument records begin: which texels of which levels, at which directions
struct SphQuery {
  const float* src;  // element (n, level, y, x, c) at n sn + level sl + y sy + x sx + c sc; NULL where no source is part of it
  int64_t sn, sl, sc;
  int sy, sx;  // (< 2^31, checked: index x stride is then one 32 x 32 -> 64 bit multiply instead of a 64-bit product per tap)
  const float* dirs;  // direction p of map n at dirs + n dn + 3 p
  int64_t dn;
  const float* level;  // NULL: level_const for every direction; else level[n ln + p]
  int64_t ln;
  float level_const;
  int N, Lv, H, W, P;
  float row_scale, col_scale, col_bias;  // fp32(H / pi), fp32(W / 2 pi), W/2 - 1/2
};

}  // namespace reni

namespace {

constexpr int64_t DG_MAX_ELEMS = 0x3fffffff;
constexpr int64_t DG_MIN_CHUNK = 2048;  // fewest reduction indices per split
constexpr int64_t DG_TARGET_WGS = 256;  // workgroups per (column group, lobe) the split aims for (one per CU)

// the split of a direction GEMM's reduction over `red` indices for `rows` output rows: a function of the two sizes only -- not
// of N, and not of the lobes -- so a map's sums run in the same order in every batch.  The forwards call it with (P, Q), the
// transpose with (Q, P).
inline void dg_split(int64_t rows, int64_t red, int64_t& S, int64_t& chunk) {
  const int64_t wgs = (rows + reni::DG_ROWS - 1) / reni::DG_ROWS;
  int64_t s = (DG_TARGET_WGS + wgs - 1) / wgs;
  const int64_t smax = red / DG_MIN_CHUNK > 1 ? red / DG_MIN_CHUNK : 1;
  if (s > smax) s = smax;
  chunk = (red + s - 1) / s;
  chunk += chunk & 1;
  S = (red + chunk - 1) / chunk;
}

// the constants of sph_rowcol, rounded once from float64: fp32(H / pi), fp32(W / 2 pi), W/2 - 1/2
inline void sph_scales(int64_t H, int64_t W, float& row_scale, float& col_scale, float& col_bias) {
  const double pi = 3.14159265358979323846;
  row_scale = (float)((double)H / pi);
  col_scale = (float)((double)W / (2.0 * pi));
  col_bias = (float)(0.5 * (double)W - 0.5);
}

// the checks of a lookup's query, in the order and wording the entry points have had: RENI_OK, or the error set.  with_src: a
// source is part of the query (reni_envmap_lookup, reni_envmap_lookup_dquery), and sizes, limits and strides are checked here;
// without one (reni_envmap_lookup_taps) the caller has checked its sizes.  others_ok: the caller's own pointers are not NULL.
inline int sph_check_query(bool with_src, int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src,
                           const int64_t* src_strides, const float* dirs, int64_t dn, const float* level, int64_t ln, bool others_ok) {
  using reni::reni_set_error;
  const char* who = with_src ? "lookup" : "lookup taps";
  if (with_src) {
    if (N < 1 || Lv < 1 || H < 1 || W < 1 || P < 1) return reni_set_error(RENI_EINVAL, "lookup: sizes must be >= 1");
    if (W & 1) return reni_set_error(RENI_EINVAL, "lookup: W must be even (the far side of a pole is W / 2 columns away)");
    if (N > 65535 || Lv > 65535 || H > 0x3fffffff / W || P > 0x3fffffff / 3 || N > 0x3fffffff / (3 * P))
      return reni_set_error(RENI_EINVAL, "lookup: need N, Lv <= 65535, H W < 2^30 and N P < 2^28");
  }
  if ((with_src && (!src || !src_strides)) || !dirs || !others_ok) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (with_src) {
    if (int rc = tu_check_strides("lookup", "src strides", src_strides, 5)) return rc;
    if (src_strides[2] > 0x7fffffff || src_strides[3] > 0x7fffffff)
      return reni_set_error(RENI_EINVAL, "lookup: the row and column strides must be < 2^31 elements");
  }
  if (dn != 0 && dn != 3 * P) return tu_fail(RENI_EINVAL, who, "dirs_stride_n must be 0 (shared) or 3 P (per map)");
  if (level && ln != 0 && ln != P) return tu_fail(RENI_EINVAL, who, "level_stride_n must be 0 (shared) or P (per map)");
  return RENI_OK;
}

// a checked query into its record (src, src_strides NULL: no source)
inline void sph_fill_query(reni::SphQuery& q, int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src,
                           const int64_t* src_strides, const float* dirs, int64_t dn, const float* level, int64_t ln,
                           float level_const) {
  if (src) {
    q.src = src; q.sn = src_strides[0]; q.sl = src_strides[1]; q.sy = (int)src_strides[2]; q.sx = (int)src_strides[3];
    q.sc = src_strides[4];
  }
  q.dirs = dirs; q.dn = dn; q.level = level; q.ln = level ? ln : 0; q.level_const = level_const;
  q.N = (int)N; q.Lv = (int)Lv; q.H = (int)H; q.W = (int)W; q.P = (int)P;
  sph_scales(H, W, q.row_scale, q.col_scale, q.col_bias);
}

inline bool lb_shape_ok(int64_t N, int64_t P, int64_t Q, int64_t Lv) {
  return N >= 1 && P >= 1 && Q >= 1 && Lv >= 1 && Lv <= reni::LB_MAX_LOBES && P <= DG_MAX_ELEMS / 3 && Q <= DG_MAX_ELEMS / 3 &&
         N <= (DG_MAX_ELEMS / (3 * P) - 1) / Lv && (3 * N + 1 + 31) / 32 <= 65535;
}

// kinds and parameters of a call (HOST arrays): RENI_OK, or the error set
inline int lb_check_lobes(int n_lobes, const int32_t* kinds, const float* params) {
  for (int l = 0; l < n_lobes; ++l) {
    const float p = params[l];
    if (kinds[l] != RENI_LOBE_PHONG && kinds[l] != RENI_LOBE_BLINN && kinds[l] != RENI_LOBE_GGX)
      return reni::reni_set_error(RENI_EINVAL, "lobe convolve: unknown lobe kind");
    if (!(p > 0.f) || !(p <= 3.0e38f))
      return reni::reni_set_error(RENI_EINVAL, "lobe convolve: a lobe's parameter must be positive and finite");
    if (kinds[l] == RENI_LOBE_GGX && !(p <= 1.f && p >= 1e-9f))
      return reni::reni_set_error(RENI_EINVAL, "lobe convolve: GGX needs 1e-9 <= alpha <= 1");
  }
  return RENI_OK;
}

// the kernel's parameter of a lobe -- PHONG: n; BLINN: s / 2; GGX: alpha^2
inline float lb_kernel_param(int kind, float p) { return kind == RENI_LOBE_BLINN ? 0.5f * p : kind == RENI_LOBE_GGX ? p * p : p; }

// one launch(kind, a) per kind present, Phong, Blinn, GGX in that order, with a.nl, a.lobe[] and a.par[] the lobes of the kind
// (A: LbArgs or LbtArgs); the first error ends the loop
template <class A, class Launch>
inline int lb_for_kinds(A& a, int n_lobes, const int32_t* kinds, const float* params, Launch launch) {
  for (int kind = RENI_LOBE_PHONG; kind <= RENI_LOBE_GGX; ++kind) {
    a.nl = 0;
    for (int l = 0; l < n_lobes; ++l) {
      if (kinds[l] != kind) continue;
      a.lobe[a.nl] = l;
      a.par[a.nl] = lb_kernel_param(kind, params[l]);
      ++a.nl;
    }
    if (!a.nl) continue;
    if (int rc = launch(kind, a)) return rc;
  }
  return RENI_OK;
}

}  // namespace
