// reni_sphere.inc -- the ONE definition of what the environment-map units share without a change to their generated code:
//   * the 32x32 MFMA result-row map and the drain pads (the SH kernels of reni_tu_baselines.hip and the direction GEMMs);
//   * of the direction GEMM (k_diffuse_convolve, k_lobe_convolve, k_lobe_convolve_t): tile constants, lobe generators, split
//     rule, limits, the lobes' argument checks.  The body (row load, clear, k-step, k-pair loop, store) stays
//     written out in each kernel: every shared form of it changed the generated code (DESIGN 4.4h);
//   * of the equirectangular lookup (k_rotate_envmap, k_envmap_lookup, k_envmap_lookup_taps): direction -> (row, col), the
//     level interpolation, the host's three constants.  The four taps stay written out in each kernel, for the same reason.
// Included at file scope, outside every namespace.  Every function here that rounds switches contraction off for itself, so
// what is written is what runs whatever the including unit compiles with (the lobe generators hold no a * b + c outside fmaf).
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

}  // namespace
