// translation unit of libreni_hip.so: the reducer behind the camera gradients of the mesh G-buffer and of the soft silhouette
// (reni_gbuffer_backward_camera, reni_soft_silhouette_backward_camera; include/reni_hip.h has the definitions).
//
// k_gb_face<true> / k_sil_face<true> store one record of CAM_REC = 13 floats per face (gR [9] row-major, gT [3], g_tan [1]);
// the camera gradient is the sum of the records over the faces.  It is a store-then-sum pass across launches, fp32, with
// no float atomic and no in-launch ticket: one kernel,
//
//   k_cam_reduce   one workgroup of four waves per CAM_CHUNK = 512 consecutive records.  Thread t adds records t and t + 256 of
//                  its chunk in this order (a record beyond n adds nothing), a butterfly of shuffles adds the 64 lanes of a wave
//                  in one fixed order, the four wave sums meet in LDS and thread c < 13 adds them in ascending wave order and
//                  writes component c of the chunk's sum.
//
// launched on [F][13], then on the [chunks][13] it wrote, until one chunk is left, which writes grad_camera itself (F <= 512:
// one launch; F <= 262144: two).  The number of launches, every chunk's extent and every order depend on F alone, so two calls
// give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

namespace reni {

__global__ void __launch_bounds__(256) k_cam_reduce(const float* __restrict__ rec, int n, float* __restrict__ out) {
  __shared__ float s_wave[4][CAM_REC];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t base = (int64_t)blockIdx.x * CAM_CHUNK;
  float s[CAM_REC];
#pragma unroll
  for (int c = 0; c < CAM_REC; ++c) s[c] = 0.f;
#pragma unroll
  for (int j = tid; j < CAM_CHUNK; j += 256) {
    const int64_t f = base + j;
    if (f >= n) continue;
    const float* r = rec + (size_t)f * CAM_REC;
#pragma unroll
    for (int c = 0; c < CAM_REC; ++c) s[c] += r[c];
  }
#pragma unroll
  for (int c = 0; c < CAM_REC; ++c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s[c] += __shfl_xor(s[c], m);
    if (lane == 0) s_wave[wave][c] = s[c];
  }
  __syncthreads();
  if (tid < CAM_REC) out[(size_t)blockIdx.x * CAM_REC + tid] = ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid];
}

size_t camera_part_floats(int64_t F) {
  size_t total = 0;
  for (int64_t n = (F + CAM_CHUNK - 1) / CAM_CHUNK; n > 1; n = (n + CAM_CHUNK - 1) / CAM_CHUNK) total += (size_t)n * CAM_REC;
  return total;
}

int launch_camera_reduce(const float* rec, int64_t F, float* part, float* grad_camera, hipStream_t s) {
  for (int64_t n = F;;) {
    const int64_t chunks = (n + CAM_CHUNK - 1) / CAM_CHUNK;
    float* dst = chunks == 1 ? grad_camera : part;
    if (int rc = tu_launch(TU_PLAIN, k_cam_reduce, dim3((unsigned)chunks), dim3(256), 0, s, rec, (int)n, dst)) return rc;
    if (chunks == 1) return RENI_OK;
    rec = dst; part += (size_t)chunks * CAM_REC; n = chunks;
  }
}

}  // namespace reni
