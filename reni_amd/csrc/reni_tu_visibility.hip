// translation unit of libreni_hip.so: cast shadows -- per-(pixel, direction) visibility masks of a mesh for the
// environment-map shader (FIT_INVERSE task).  include/reni_hip.h has the definition; DESIGN.md 4.4g the layouts and numbers.
//
// The lights are at infinity, so bit (p, j) asks one question: does the ray from the pixel's surface point o_p along the unit
// direction d_j meet any face but the pixel's own at t > t_min?  It is an any-hit query (no nearest hit, no ordering), so
// the answer does not depend on the order in which faces are visited and the pass is deterministic by construction.
//
//   reni_mesh_visibility_prepare   one workgroup of 64 threads per cluster of 64 consecutive faces (the caller's order:
//                                  Morton-sorted centroids keep a cluster compact): per-face v0, e1, e2 and id, and the
//                                  cluster's bounding box, inflated
//   reni_mesh_visibility           a workgroup = one pixel x 256 directions, a wave = 64 rays with ONE origin.  Per cluster:
//                                  each lane slab-tests its ray against the box; if no live lane touches it the wave skips
//                                  the cluster (one ballot).  Otherwise the wave stages the cluster's 64 faces in its own LDS
//                                  region -- lane k loads face k and finishes everything that depends on the origin alone
//                                  (s = o - v0, q = s x e1, e2 . q) -- and every lane reads the records by broadcast.
//                                  A ray that is occluded stops counting; the wave leaves when all of its rays are.
//
// Per (ray, face) the lanes spend 4 LDS broadcasts and ~30 fp32 operations; nothing here is matrix-shaped.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#define DEV __device__ __forceinline__

namespace reni {

constexpr int VIS_CLUSTER = 64;        // faces per cluster == lanes of a wave: one lane stages one face
constexpr int VIS_WAVES = 4;           // waves per workgroup: 256 directions of one pixel
constexpr int VIS_HEADER = 64;         // bytes in front of the boxes
constexpr uint32_t VIS_MAGIC = 0x52564953u;
constexpr float VIS_A_EPS = 1e-12f;    // |a| <= this: the ray is parallel to the face (or the face is degenerate), a miss
// The slab test's three quotients carry a relative error of a few 2^-24 each; the face test's u, v, t carry more on slivers
// and grazing rays.  A box grown by 2^-10 of its own size and position keeps the slab test on the safe side of both, and
// costs no culling worth measuring (the boxes of a Morton cluster overlap by far more than that anyway).
constexpr float VIS_BOX_MARGIN = 1.f / 1024.f;

struct VisHeader {
  uint32_t magic;
  int32_t F, NC;
};

// accel = [VIS_HEADER bytes][NC boxes: float4 lo, float4 hi][NC * 64 faces: float4 (v0, id), float4 (e1, 0), float4 (e2, 0)]
DEV const float4* vis_boxes(const void* accel) { return (const float4*)((const char*)accel + VIS_HEADER); }
DEV const float4* vis_faces(const void* accel, int NC) { return vis_boxes(accel) + (size_t)NC * 2; }

DEV float wave_min(float x) {
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
  return x;
}
DEV float wave_max(float x) {
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}

// slot k of the record holds face order[k] (order == NULL: face k); a face with an index outside [0, V), or an order entry
// outside [0, F), becomes an empty slot: zero edges (a == 0, never hit), id -1, no part in the box
__global__ void __launch_bounds__(VIS_CLUSTER) k_vis_prepare(int V, int F, const float* __restrict__ verts,
                                                             const int64_t* __restrict__ faces,
                                                             const int64_t* __restrict__ order, void* accel) {
  const int c = blockIdx.x, lane = threadIdx.x, NC = gridDim.x;
  const int k = c * VIS_CLUSTER + lane;
  float4 r0 = {0.f, 0.f, 0.f, __int_as_float(-1)}, r1 = {0.f, 0.f, 0.f, 0.f}, r2 = {0.f, 0.f, 0.f, 0.f};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (k < F) {
    const int64_t f = order ? order[k] : (int64_t)k;
    if (f >= 0 && f < F) {
      const int64_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
      if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        float p[3][3];
        const int64_t idx[3] = {i0, i1, i2};
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
          for (int x = 0; x < 3; ++x) p[v][x] = verts[idx[v] * 3 + x];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          lo[x] = fminf(p[0][x], fminf(p[1][x], p[2][x]));
          hi[x] = fmaxf(p[0][x], fmaxf(p[1][x], p[2][x]));
        }
        r0 = float4{p[0][0], p[0][1], p[0][2], __int_as_float((int)f)};
        r1 = float4{p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2], 0.f};
        r2 = float4{p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2], 0.f};
      }
    }
  }
  float4* rec = (float4*)vis_faces(accel, NC) + (size_t)k * 3;
  rec[0] = r0; rec[1] = r1; rec[2] = r2;
#pragma unroll
  for (int x = 0; x < 3; ++x) { lo[x] = wave_min(lo[x]); hi[x] = wave_max(hi[x]); }
  if (lane == 0) {
    float4 blo = {0.f, 0.f, 0.f, 1.f}, bhi = {0.f, 0.f, 0.f, 0.f};  // lo.w != 0: no valid face, never touched
    if (lo[0] <= hi[0]) {
      float m = 0.f;
#pragma unroll
      for (int x = 0; x < 3; ++x) m = fmaxf(m, fmaxf(hi[x] - lo[x], fmaxf(fabsf(lo[x]), fabsf(hi[x]))));
      m *= VIS_BOX_MARGIN;
      blo = float4{lo[0] - m, lo[1] - m, lo[2] - m, 0.f};
      bhi = float4{hi[0] + m, hi[1] + m, hi[2] + m, 0.f};
    }
    float4* box = (float4*)vis_boxes(accel) + (size_t)c * 2;
    box[0] = blo; box[1] = bhi;
    if (c == 0) {
      VisHeader* h = (VisHeader*)accel;
      h->magic = VIS_MAGIC; h->F = F; h->NC = NC;
    }
  }
}

struct VisArgs {
  const float* pos;         // [NP][3]
  const int64_t* p2f;       // [NP]
  const float* dirs;        // [NB][J][3] at dirs + nb * dirs_bstride
  const void* accel;
  uint32_t* vis;            // [NB][NP][JW]
  long long dirs_bstride;
  float t_min;
  int NP, J, JW, no_cull;
};

// one face of the staged cluster, as the lanes read it: everything that does not depend on the direction is already formed
struct VisStaged {
  float4 e1id;  // e1, id
  float4 e2t;   // e2, e2 . q  (t = this / a)
  float4 s;     // s = o - v0
  float4 q;     // q = s x e1
};

__global__ void __launch_bounds__(VIS_WAVES * 64) k_mesh_visibility(const VisArgs a) {
  __shared__ VisStaged stage[VIS_WAVES][VIS_CLUSTER];
  const int p = blockIdx.x, nb = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = (blockIdx.y * VIS_WAVES + wave) * 64 + lane;
  const int w0 = (blockIdx.y * VIS_WAVES + wave) * 2;  // the wave's two mask words
  uint32_t* out = a.vis + ((size_t)nb * a.NP + p) * a.JW;
  const int64_t own64 = a.p2f[p];
  if (own64 < 0) {  // background: all zeros (the whole workgroup takes this branch)
    if (lane == 0) {
      if (w0 < a.JW) out[w0] = 0u;
      if (w0 + 1 < a.JW) out[w0 + 1] = 0u;
    }
    return;
  }
  const int own = own64 > 0x7fffffff ? -2 : (int)own64;  // (an id the record cannot hold excludes nothing)
  const float o[3] = {a.pos[(size_t)p * 3], a.pos[(size_t)p * 3 + 1], a.pos[(size_t)p * 3 + 2]};
  const bool in_range = j < a.J;
  float d[3] = {0.f, 0.f, 1.f};
  if (in_range) {
    const float* dp = a.dirs + (size_t)nb * a.dirs_bstride + (size_t)j * 3;
    d[0] = dp[0]; d[1] = dp[1]; d[2] = dp[2];
  }
  const float inv[3] = {1.f / d[0], 1.f / d[1], 1.f / d[2]};  // +-inf for a zero component: the slab test's usual form
  bool occ = !in_range;  // a lane without a direction never holds the wave back
  const VisHeader* hd = (const VisHeader*)a.accel;
  const int NC = hd->magic == VIS_MAGIC ? hd->NC : 0;  // (a buffer that reni_mesh_visibility_prepare never filled is not walked)
  const float4* __restrict__ boxes = vis_boxes(a.accel);
  const float4* __restrict__ faces = vis_faces(a.accel, NC);
  VisStaged* st = stage[wave];
  for (int c = 0; c < NC; ++c) {
    if (!a.no_cull) {
      if (__ballot(!occ) == 0ull) break;  // every ray of the wave is occluded
      const float4 blo = boxes[(size_t)c * 2], bhi = boxes[(size_t)c * 2 + 1];
      // slabs: the ray is inside the box for t in [tn, tf].  NaN (0 * inf: the origin exactly on a slab plane of a
      // direction parallel to it) drops out of fminf / fmaxf, which return the pair's other quotient, +inf on a lo plane
      // (tn = +inf) and -inf on a hi plane (tf = -inf): the cluster is SKIPPED.  That is right, not merely safe: the
      // margin is > 0 on every axis, so every face lies strictly inside the box and a ray within one of its planes
      // meets none (tests/test_gpu_visibility_edges.py, the box-plane probes).  A zero, NaN or inf direction hits no
      // face (den is 0 or NaN, or u and v are), so whatever the slabs make of it moves no bit
      const float x0 = (blo.x - o[0]) * inv[0], x1 = (bhi.x - o[0]) * inv[0];
      const float y0 = (blo.y - o[1]) * inv[1], y1 = (bhi.y - o[1]) * inv[1];
      const float z0 = (blo.z - o[2]) * inv[2], z1 = (bhi.z - o[2]) * inv[2];
      const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
      const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
      // (tf >= 0, so the factor only ever widens the interval; lo.w != 0 marks a cluster without a valid face)
      const bool touch = blo.w == 0.f && tf >= 0.f && tf * 1.000002f >= tn;
      if (__ballot(touch && !occ) == 0ull) continue;
    }
    {  // stage: lane k owns face k of the cluster.  The previous cluster's reads are done: a wave runs in lockstep, and
       // the fences keep the compiler from moving LDS traffic across the two points
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const float4* rec = faces + ((size_t)c * VIS_CLUSTER + lane) * 3;
      const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
      const float s0 = o[0] - r0.x, s1 = o[1] - r0.y, s2 = o[2] - r0.z;
      const float q0 = s1 * r1.z - s2 * r1.y, q1 = s2 * r1.x - s0 * r1.z, q2 = s0 * r1.y - s1 * r1.x;  // s x e1
      VisStaged v;
      v.e1id = r1; v.e1id.w = r0.w;
      v.e2t = float4{r2.x, r2.y, r2.z, r2.x * q0 + r2.y * q1 + r2.z * q2};
      v.s = float4{s0, s1, s2, 0.f};
      v.q = float4{q0, q1, q2, 0.f};
      st[lane] = v;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (int k0 = 0; k0 < VIS_CLUSTER; k0 += 8) {
      if (!a.no_cull && __ballot(!occ) == 0ull) break;
#pragma unroll
      for (int k = k0; k < k0 + 8; ++k) {
        const float4 e1 = st[k].e1id, e2 = st[k].e2t, s = st[k].s, q = st[k].q;
        const float h0 = d[1] * e2.z - d[2] * e2.y, h1 = d[2] * e2.x - d[0] * e2.z, h2 = d[0] * e2.y - d[1] * e2.x;  // d x e2
        const float den = e1.x * h0 + e1.y * h1 + e1.z * h2;
        const float ia = __builtin_amdgcn_rcpf(den);  // 1 ulp; a zero den fails the |a| test below
        const float u = (s.x * h0 + s.y * h1 + s.z * h2) * ia;
        const float v = (d[0] * q.x + d[1] * q.y + d[2] * q.z) * ia;
        const float t = e2.w * ia;
        const bool hit = fabsf(den) > VIS_A_EPS && __float_as_int(e1.w) != own && u >= 0.f && v >= 0.f && u + v <= 1.f &&
                         t > a.t_min;
        occ = occ || hit;
      }
    }
  }
  const unsigned long long bits = __ballot(in_range && !occ);
  if (lane == 0) {
    if (w0 < a.JW) out[w0] = (uint32_t)bits;
    if (w0 + 1 < a.JW) out[w0 + 1] = (uint32_t)(bits >> 32);
  }
}

}  // namespace reni

namespace {
using reni::reni_set_error;
constexpr int64_t VIS_MAX_FACES = 0x3fffffff;

size_t accel_bytes(int64_t F) {
  const size_t NC = (size_t)((F + reni::VIS_CLUSTER - 1) / reni::VIS_CLUSTER);
  return reni::VIS_HEADER + NC * 32 + NC * reni::VIS_CLUSTER * 48;
}
}  // namespace

extern "C" {

size_t reni_mesh_visibility_accel_bytes(int64_t F) {
  if (F < 1 || F > VIS_MAX_FACES) return 0;
  return accel_bytes(F);
}

int reni_mesh_visibility_prepare(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* order,
                                 void* accel, size_t accel_bytes_given, void* stream) {
  if (V < 1 || F < 1 || V > VIS_MAX_FACES || F > VIS_MAX_FACES) return reni_set_error(RENI_EINVAL, "visibility prepare: bad V / F");
  if (!verts || !faces || !accel) return reni_set_error(RENI_EINVAL, "visibility prepare: NULL argument");
  if (((uintptr_t)accel & 15) != 0) return reni_set_error(RENI_EINVAL, "visibility prepare: accel must be 16-byte aligned");
  if (accel_bytes_given < accel_bytes(F)) return reni_set_error(RENI_EWORKSPACE, "visibility prepare: accel buffer too small");
  const unsigned NC = (unsigned)((F + reni::VIS_CLUSTER - 1) / reni::VIS_CLUSTER);
  return tu_launch(TU_COUNTED, reni::k_vis_prepare, dim3(NC), dim3(reni::VIS_CLUSTER), 0, (hipStream_t)stream, (int)V, (int)F, verts,
                   faces, order, accel);
}

int reni_mesh_visibility(int64_t B, int64_t NP, int64_t J, const float* positions, const int64_t* pix_to_face,
                         const float* dirs, int64_t dirs_batch_stride, const void* accel, float t_min, uint32_t flags,
                         uint32_t* vis, void* stream) {
  if (B < 1 || NP < 1 || J < 1) return reni_set_error(RENI_EINVAL, "visibility: B, NP and J must be >= 1");
  if (NP > 0x7fffffff || J > 65535ll * 256 || B > 65535) return reni_set_error(RENI_EINVAL, "visibility: problem too large");
  if (!positions || !pix_to_face || !dirs || !accel || !vis) return reni_set_error(RENI_EINVAL, "visibility: NULL argument");
  if (((uintptr_t)accel & 15) != 0) return reni_set_error(RENI_EINVAL, "visibility: accel must be 16-byte aligned");
  if (dirs_batch_stride != 0 && dirs_batch_stride < J * 3) return reni_set_error(RENI_EINVAL, "visibility: direction batch stride must be 0 or >= 3 J");
  if (!(t_min >= 0.f) || !isfinite(t_min)) return reni_set_error(RENI_EINVAL, "visibility: t_min must be finite and >= 0");
  if (flags & ~(uint32_t)RENI_VIS_NO_CULL) return reni_set_error(RENI_EINVAL, "visibility: unknown flag");
  reni::VisArgs a;
  a.pos = positions; a.p2f = pix_to_face; a.dirs = dirs; a.accel = accel; a.vis = vis;
  a.dirs_bstride = dirs_batch_stride; a.t_min = t_min;
  a.NP = (int)NP; a.J = (int)J; a.JW = (int)((J + 31) / 32); a.no_cull = (flags & RENI_VIS_NO_CULL) ? 1 : 0;
  const int NB = dirs_batch_stride == 0 ? 1 : (int)B;
  const dim3 grid((unsigned)NP, (unsigned)((J + 255) / 256), (unsigned)NB);
  return tu_launch(TU_COUNTED, reni::k_mesh_visibility, grid, dim3(reni::VIS_WAVES * 64), 0, (hipStream_t)stream, a);
}

}  // extern "C"
