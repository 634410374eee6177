// reni_device.inc -- hand-written gfx950 (CDNA4) kernels for the RENI forward / training hot path.
//
// Included by the translation units reni_tu_*.hip (compiled in parallel by build.sh).  Each defines ONE of
//   RENI_TU_CORE       persistent training kernels, prologue / epilogue kernels, the C ABI (reni_capi.inc)
//   RENI_TU_MAIN_F32   k_reni_main<PolF32,  H, MODE, FILM=false> + its host launcher
//   RENI_TU_MAIN_BF16  k_reni_main<PolBF16, H, MODE, FILM=false>
//   RENI_TU_FILM_F32   k_reni_main<PolF32,  H, MODE, FILM=true>
//   RENI_TU_FILM_BF16  k_reni_main<PolBF16, H, MODE, FILM=true>
//   RENI_TU_TRAIN_FILM the FiLM instances of the persistent kernels (k_reni_train_bf16<.., FILM=true>, k_reni_dw1<.., true>)
//   RENI_TU_WIDE       k_reni_wide256: the persistent chain at H = 256 (frozen decoder / statistics / inference / training form) + k_wide_head_dw
// Kernels never cross a translation unit: the C ABI reaches the fused kernels through plain host
// launchers (launch_main_*), so no relocatable device code is needed.
//
// What is computed (reference: /root/reference/src/models/RENI.py:23-60 invariant encodings,
// :63-87 SineLayer, :132-178 decoder; src/utils/loss_functions.py:6-71 losses) and how it is
// re-factored for the GPU is described in DESIGN.md.  Short version:
//
//   * Every column of the reference's concatenated MLP input is either constant per image
//     (Gram entries, Z_y, vec(Z)) or linear in the direction d (inner products d.Z^T, |d_xz|,
//     d_y).  The first SineLayer therefore collapses to a per-image affine map
//         a0 = A_b . (dx, dy, dz, r, 1),   A_b in R^{H x 5}   (k_prep_image)
//     and its backward to a per-image H x 5 reduction dA_b (fused kernel) followed by tiny
//     per-image tails (k_tail_dz, k_tail_dw0).
//   * The dense part runs on MFMA with activations laid out [feature][sample]: the weights are
//     the A operand (read from LDS), the activations the B operand, so the accumulator of layer l
//     (lane = sample, registers = features) IS the B operand of layer l+1 after sin() -- the
//     chain never leaves registers.
//   * One 256-thread workgroup = 4 waves x 32 samples = a 128-sample tile.  Forward stashes the
//     sine arguments of every layer (u16 phase for bf16, fp32 pre-activation for fp32) to a
//     per-workgroup scratch ring that stays cache resident; backward replays them in reverse.
//   * Weight gradients are MFMA GEMMs with K = samples: gradients/activations are transposed
//     through LDS once per layer and tile; per-workgroup partial sums are reduced by
//     k_reduce_partials in a fixed order (deterministic, no float atomics).
//
// gfx950 only.  No portability layer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "reni_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define DEV __device__ __forceinline__

namespace reni {

#include "reni_dev_common.inc"
#include "reni_dev_main.inc"
#include "reni_dev_train.inc"

#ifdef RENI_TU_WIDE
#include "reni_dev_wide.inc"
#endif
#ifdef RENI_TU_CORE
#include "reni_dev_l0ring.inc"
#include "reni_dev_stream.inc"
#include "reni_dev_small.inc"
#endif  // RENI_TU_CORE

// ---- host launchers of the fused kernel (one precision / conditioning per translation unit) ----------
template <class Pol, int H, bool FILM>
hipError_t launch_main_one(int mode, const MainArgs& a, int nwg, hipStream_t s) {
  constexpr int lds = Geo<Pol, H>::LDS_BYTES + (FILM ? Geo<Pol, H>::FILM_LDS : 0);
  void (*fn)(const MainArgs) = nullptr;
  if (mode == MODE_FWD) fn = k_reni_main<Pol, H, MODE_FWD, FILM>;
  else if (mode == MODE_STATS) fn = k_reni_main<Pol, H, MODE_STATS, FILM>;
  else fn = k_reni_main<Pol, H, MODE_FWD_BWD, FILM>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(nwg), dim3(256), lds, s, a);
  return hipGetLastError();
}
template <class Pol, bool FILM>
hipError_t launch_main_h(int H, int mode, const MainArgs& a, int nwg, hipStream_t s) {
  if (H == 32) return launch_main_one<Pol, 32, FILM>(mode, a, nwg, s);
  if (H == 64) return launch_main_one<Pol, 64, FILM>(mode, a, nwg, s);
  if (H == 128) return launch_main_one<Pol, 128, FILM>(mode, a, nwg, s);
  if (H == 256) return launch_main_one<Pol, 256, FILM>(mode, a, nwg, s);
  return hipErrorInvalidValue;
}
#if defined(RENI_TU_TRAIN_FILM)
// FiLM instances of the persistent kernels: a translation unit of their own (reni_tu_train_film.hip)
int train_film_lds_bytes(int which) {
  // training instances (0; 2 = its SPEC form: + the per-lane accumulators): + the FiLM tables
  return GeoP<128>::LDS_BYTES + (which != 1 ? (5 + 1) * 2 * 128 * 4 : 0) + (which == 2 ? GeoP<128>::LACC_BYTES : 0);
}
hipError_t launch_train_film(int which, const MainArgs& a, int grid, hipStream_t s) {
  void (*fn)(const MainArgs) = which == 0 ? k_reni_train_bf16<128, true, false, true>
                               : which == 2 ? k_reni_train_bf16<128, true, false, true, true> : k_reni_train_bf16<128, false, true, true>;
  const int lds = train_film_lds_bytes(which);
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(which != 1 ? 256 : 512), lds, s, a);
  return hipGetLastError();
}
hipError_t launch_dw1_film(const MainArgs& a, int grid, hipStream_t s) {
  void (*f1)(const MainArgs) = k_reni_dw1<128, true>;
  hipError_t e = hipFuncSetAttribute((const void*)f1, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * TS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(f1, dim3(grid), dim3(256), 2 * TS_BYTES, s, a);
  return hipGetLastError();
}
#elif defined(RENI_TU_MAIN_F32)
hipError_t launch_main_f32(int H, int mode, const MainArgs& a, int nwg, hipStream_t s) { return launch_main_h<PolF32, false>(H, mode, a, nwg, s); }
#elif defined(RENI_TU_MAIN_BF16)
hipError_t launch_main_bf16(int H, int mode, const MainArgs& a, int nwg, hipStream_t s) { return launch_main_h<PolBF16, false>(H, mode, a, nwg, s); }
#elif defined(RENI_TU_FILM_F32)
hipError_t launch_film_f32(int H, int mode, const MainArgs& a, int nwg, hipStream_t s) { return launch_main_h<PolF32, true>(H, mode, a, nwg, s); }
#elif defined(RENI_TU_FILM_BF16)
hipError_t launch_film_bf16(int H, int mode, const MainArgs& a, int nwg, hipStream_t s) { return launch_main_h<PolBF16, true>(H, mode, a, nwg, s); }
#endif

}  // namespace reni

#ifdef RENI_TU_CORE
#include "reni_capi.inc"
#endif
