// reni_lobe.inc -- what the lobe convolution (reni_tu_glossy.hip) and its transpose (reni_tu_glossy_bwd.hip) must share to
// stay each other's transpose: the tile geometry, the lobe generators, the MFMA drain, the split rule and the lobes' argument
// checks.  Included inside neither namespace; both units switch contraction off before they include it.
#pragma once

namespace reni {

typedef float lb_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LB_OT = 2;     // 32-row output tiles per wave
constexpr int LB_WAVES = 4;  // waves per workgroup, each its own output rows
constexpr int LB_ROWS = 32 * LB_OT * LB_WAVES;
constexpr int LB_MAX_LOBES = 16;

DEV constexpr int lb_rowmap(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }  // 32x32 MFMA result row

DEV void lb_mfma_drain() {  // wait out the last MFMA's write-back (18 states) before its result is read
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 15\n\ts_nop 3");
  __builtin_amdgcn_sched_barrier(0);
}

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

}  // namespace reni

namespace {

constexpr int64_t LB_MAX_ELEMS = 0x3fffffff;
constexpr int64_t LB_MIN_CHUNK = 2048;  // fewest reduction indices per split
constexpr int64_t LB_TARGET_WGS = 256;  // workgroups per (column group, lobe) the split aims for (one per CU)

inline bool lb_shape_ok(int64_t N, int64_t P, int64_t Q, int64_t Lv) {
  return N >= 1 && P >= 1 && Q >= 1 && Lv >= 1 && Lv <= reni::LB_MAX_LOBES && P <= LB_MAX_ELEMS / 3 && Q <= LB_MAX_ELEMS / 3 &&
         N <= (LB_MAX_ELEMS / (3 * P) - 1) / Lv && (3 * N + 1 + 31) / 32 <= 65535;
}

// the split of a reduction over `red` indices for `rows` output rows: reni_diffuse_convolve's rule, a function of the two
// sizes only -- not of N, and not of the lobes.  The forward calls it with (P, Q), the transpose with (Q, P).
inline void lb_split(int64_t rows, int64_t red, int64_t& S, int64_t& chunk) {
  const int64_t wgs = (rows + reni::LB_ROWS - 1) / reni::LB_ROWS;
  int64_t s = (LB_TARGET_WGS + wgs - 1) / wgs;
  const int64_t smax = red / LB_MIN_CHUNK > 1 ? red / LB_MIN_CHUNK : 1;
  if (s > smax) s = smax;
  chunk = (red + s - 1) / s;
  chunk += chunk & 1;
  S = (red + chunk - 1) / chunk;
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
