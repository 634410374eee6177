// reni_tu_host.inc -- the ONE host path of the utility units (shade, image, raster, baselines, diffuse, glossy, glossy_bwd,
// resample, rotate, metrics, lights, visibility): the prefixed error, the workspace and stride checks, and the launch.
// Host code only; the core's units, reni_internal.h and reni_capi.inc do not include it.  Included at file scope.
//   * a launch returns at once when it failed; it is counted (reni_launch_count) only where the caller says TU_COUNTED, and
//     only when it succeeded.  Which entry points count is history, not design: DESIGN 4.4i has the table.
//   * an instance is chosen by selecting the kernel pointer, then launched once:
//       const auto k = bilinear ? k_rotate_envmap<true> : k_rotate_envmap<false>;  tu_launch(TU_PLAIN, k, grid, ...)
//     The instances must stay named in the order they had: a unit's kernels are emitted in the order the host code first names
//     them, and a nested a ? x : b ? y : z names y and z before x (hence the assignments in reni_tu_metrics.hip).
#pragma once
#include <stdint.h>

#include <string>

#include "reni_internal.h"

namespace {

// "<who>: <text>" as reni_last_error()'s message; returns `code`
inline int tu_fail(int code, const char* who, const char* text) {
  return reni::reni_set_error(code, (std::string(who) + ": " + text).c_str());
}

// RENI_OK, or "<who>: workspace missing, too small or not 256-byte aligned" set
inline int tu_check_ws(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  if (ws && !((uintptr_t)ws & 255) && ws_bytes >= need) return RENI_OK;
  return tu_fail(RENI_EWORKSPACE, who, "workspace missing, too small or not 256-byte aligned");
}

// RENI_OK, or "<who>: <what> must be >= 0" set (what: "src strides", "image strides", ...)
inline int tu_check_strides(const char* who, const char* what, const int64_t* strides, int n) {
  for (int k = 0; k < n; ++k)
    if (strides[k] < 0) return tu_fail(RENI_EINVAL, who, (std::string(what) + " must be >= 0").c_str());
  return RENI_OK;
}

enum TuCount { TU_PLAIN, TU_COUNTED };

// one kernel launch: RENI_OK, or the launch's error set.  The arguments convert to the kernel's parameter types as at a
// written-out launch.
template <typename... Params, typename... Args>
inline int tu_launch(TuCount count, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                     const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
  const int rc = reni::hip_status();
  if (rc == RENI_OK && count == TU_COUNTED) reni::note_launches(1);
  return rc;
}

}  // namespace
