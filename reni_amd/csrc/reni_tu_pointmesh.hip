// translation unit of libreni_hip.so: points against a mesh -- for every point the nearest triangle (reni_nearest_faces) and for
// every triangle the nearest point (reni_faces_nearest_points), each with the closest point as a tap row of the texture unit.
// include/reni_hip.h has the definitions in full ("points against a mesh"); DESIGN 4.4v the structure.
//
// fp32, no float atomic, no in-launch ticket, no host synchronisation, launches on `stream` only.
//
//   k_pm_search<FACEQ>   reni_tu_points.hip's k_np_search with a triangle on one side.  PM_Q queries per lane in registers,
//                        PM_BLOCK lanes; the targets of the workgroup's slice pass through LDS in tiles of PM_TILE records that
//                        every lane reads at the SAME address (a broadcast, ds_read_b128).  FACEQ = false: the queries are
//                        points, a record is a triangle prepared once per tile by the staging lanes -- (a, ab, ac) in three
//                        16-byte words, all NaN for a face that takes no part.  FACEQ = true: the queries are triangles, a
//                        record is one 16-byte point.  d = pm_pair(..), ascending j, strict <.  A tile's tail is padded with
//                        NaN records up to a multiple of PM_UNROLL: a NaN wins no comparison, so there is no remainder loop.
//                        grid.y = slices of the target range.  One slice: writes the results.  More: the partial (d, j).
//   k_pm_combine<FACEQ>  one lane per query: the lexicographic minimum of the slices' (d, j), then the results.
// The results of a query are written by pm_store from (d, j) alone: it evaluates pm_closest once more for the winning pair --
// the same function on the same operands, the same bits -- and writes the tap row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__

namespace reni {

constexpr int PM_BLOCK = 256;
constexpr int PM_Q = 2;                       // queries per lane (148 VGPRs with point queries, 111 with face queries: no scratch)
constexpr int PM_QUERIES = PM_BLOCK * PM_Q;   // per workgroup
constexpr int PM_TILE = 256;                  // targets staged at a time (12 KB of triangles, 4 KB of points)
constexpr int PM_UNROLL = 4;

struct PmArgs {
  const float* points;   // [N][3]
  const float* verts;    // [V][3]
  const int64_t* faces;  // [F][3]
  int N, V, F;
  int per;               // targets per slice
  float* pd;             // [slices][queries], slices > 1
  int32_t* pj;           // [slices][queries], -1: no comparison succeeded
  float* dist2;          // [queries]
  int64_t* idx;          // [queries]
  int32_t* tap_index;    // [queries][8]
  float* tap_weight;     // [queries][8]
};

struct PmTri {
  float a[3], ab[3], ac[3];
};

DEV float pm_dot(const float (&u)[3], const float (&v)[3]) { return fmaf(u[2], v[2], fmaf(u[1], v[1], u[0] * v[0])); }

// (v, w) of the closest point q = a + v ab + w ac of the triangle to p, ap = p - a: the region form (include/reni_hip.h has the
// order of the operations).  0 <= v <= 1, 0 <= w <= 1 - v for any operands, NaN included.
DEV void pm_closest(const PmTri& t, const float (&ap)[3], float& v, float& w) {
  float bp[3], cp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    bp[c] = ap[c] - t.ab[c];
    cp[c] = ap[c] - t.ac[c];
  }
  const float d1 = pm_dot(t.ab, ap), d2 = pm_dot(t.ac, ap);
  const float d3 = pm_dot(t.ab, bp), d4 = pm_dot(t.ac, bp);
  const float d5 = pm_dot(t.ab, cp), d6 = pm_dot(t.ac, cp);
  const float vc = fmaf(d1, d4, -(d3 * d2));
  const float vb = fmaf(d5, d2, -(d1 * d6));
  const float va = fmaf(d3, d6, -(d5 * d4));
  const float e43 = d4 - d3, e56 = d5 - d6;
  // the interior first, then the regions from the last tested to the first: the first that holds decides
  float nv = vb, nw = vc, den = (va + vb) + vc;
  if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { nv = e56; nw = e43; den = e43 + e56; }   // edge bc
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { nv = 0.f; nw = d2; den = d2 - d6; }         // edge ac
  if (d6 >= 0.f && d5 <= d6) { nv = 0.f; nw = 1.f; den = 1.f; }                          // vertex c
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { nv = d1; nw = 0.f; den = d1 - d3; }         // edge ab
  if (d3 >= 0.f && d4 <= d3) { nv = 1.f; nw = 0.f; den = 1.f; }                          // vertex b
  if (d1 <= 0.f && d2 <= 0.f) { nv = 0.f; nw = 0.f; den = 1.f; }                         // vertex a
  const float r = 1.f / den;
  v = fminf(fmaxf(nv * r, 0.f), 1.f);          // (a NaN -- 0 / 0 of a triangle without area -- becomes 0)
  w = fminf(fmaxf(nw * r, 0.f), 1.f - v);
}

// d(p, triangle) and the weights it was taken at
DEV float pm_pair(const PmTri& t, float p0, float p1, float p2, float& v, float& w) {
  const float ap[3] = {p0 - t.a[0], p1 - t.a[1], p2 - t.a[2]};
  pm_closest(t, ap, v, w);
  const float rx = p0 - fmaf(w, t.ac[0], fmaf(v, t.ab[0], t.a[0]));
  const float ry = p1 - fmaf(w, t.ac[1], fmaf(v, t.ab[1], t.a[1]));
  const float rz = p2 - fmaf(w, t.ac[2], fmaf(v, t.ab[2], t.a[2]));
  return fmaf(rz, rz, fmaf(ry, ry, rx * rx));
}

// face f as (a, ab, ac) and its vertex indices; all NaN (and false) for a face that takes no part: indices in [0, V), pairwise
// different.  f must be in [0, F).
DEV bool pm_load_tri(const PmArgs& a, int64_t f, PmTri& t, int32_t (&ii)[3]) {
  int64_t i[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) i[k] = a.faces[3 * f + k];
  bool ok = i[0] != i[1] && i[0] != i[2] && i[1] != i[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && i[k] >= 0 && i[k] < a.V;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t.a[c] = t.ab[c] = t.ac[c] = NAN;
    ii[c] = 0;
  }
  if (!ok) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float pa = a.verts[3 * i[0] + c];
    t.a[c] = pa;
    t.ab[c] = a.verts[3 * i[1] + c] - pa;
    t.ac[c] = a.verts[3 * i[2] + c] - pa;
    ii[c] = (int32_t)i[c];
  }
  return true;
}

// the results of query i from the best (d, j) found; j < 0: nothing compared below +inf -> -1, +inf, zero taps at index 0
template <bool FACEQ>
DEV void pm_store(const PmArgs& a, int i, float d, int j) {
  int32_t ii[3] = {0, 0, 0};
  float u = 0.f, v = 0.f, w = 0.f;
  const int targets = FACEQ ? a.N : a.F;
  bool ok = j >= 0 && j < targets;
  if (ok) {
    const int f = FACEQ ? i : j, p = FACEQ ? j : i;
    PmTri t;
    ok = pm_load_tri(a, f, t, ii);  // (true: the face won a comparison)
    if (ok) {
      const float* pp = a.points + 3 * (size_t)p;
      pm_pair(t, pp[0], pp[1], pp[2], v, w);
      u = (1.f - v) - w;
    }
  }
  if (!ok) {
    d = INFINITY;
    j = -1;
  }
  a.dist2[i] = d;
  a.idx[i] = (int64_t)j;
  int4* ip = (int4*)(a.tap_index + 8 * (size_t)i);
  float4* wp = (float4*)(a.tap_weight + 8 * (size_t)i);
  ip[0] = make_int4(ii[0], ii[1], ii[2], 0);
  ip[1] = make_int4(0, 0, 0, 0);
  wp[0] = make_float4(u, v, w, 0.f);
  wp[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <bool FACEQ>
__global__ void __launch_bounds__(PM_BLOCK) k_pm_search(const PmArgs a) {
  constexpr int REC = FACEQ ? 1 : 3;  // 16-byte words per staged target
  __shared__ float4 tile[PM_TILE * REC];
  const int tid = (int)threadIdx.x;
  const int queries = FACEQ ? a.F : a.N, targets = FACEQ ? a.N : a.F;
  PmTri qt[FACEQ ? PM_Q : 1];
  float qp[FACEQ ? 1 : PM_Q][3];
  float best[PM_Q];
  int bj[PM_Q];
#pragma unroll
  for (int q = 0; q < PM_Q; ++q) {
    const int64_t i = min((int64_t)blockIdx.x * PM_QUERIES + q * PM_BLOCK + tid, (int64_t)queries - 1);  // (a lane past the end repeats the last query)
    if (FACEQ) {
      int32_t ii[3];
      pm_load_tri(a, i, qt[q], ii);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) qp[q][c] = a.points[3 * i + c];
    }
    best[q] = INFINITY;
    bj[q] = -1;
  }
  const int64_t j0 = (int64_t)blockIdx.y * a.per;
  const int64_t j1 = min(j0 + (int64_t)a.per, (int64_t)targets);
  for (int64_t base = j0; base < j1; base += PM_TILE) {
    const int n = (int)min((int64_t)PM_TILE, j1 - base);
    const int n4 = (n + PM_UNROLL - 1) / PM_UNROLL * PM_UNROLL;  // <= PM_TILE: PM_TILE is a multiple of PM_UNROLL
    __syncthreads();
    for (int t = tid; t < n4; t += PM_BLOCK) {
      if (FACEQ) {
        float4 r = make_float4(NAN, NAN, NAN, 0.f);
        if (t < n) {
          const float* p = a.points + 3 * (base + t);
          r.x = p[0]; r.y = p[1]; r.z = p[2];
        }
        tile[t] = r;
      } else {
        PmTri tr;
        int32_t ii[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) tr.a[c] = tr.ab[c] = tr.ac[c] = NAN;
        if (t < n) pm_load_tri(a, base + t, tr, ii);
        tile[REC * t] = make_float4(tr.a[0], tr.a[1], tr.a[2], 0.f);
        tile[REC * t + 1] = make_float4(tr.ab[0], tr.ab[1], tr.ab[2], 0.f);
        tile[REC * t + 2] = make_float4(tr.ac[0], tr.ac[1], tr.ac[2], 0.f);
      }
    }
    __syncthreads();
    for (int t0 = 0; t0 < n4; t0 += PM_UNROLL) {
#pragma unroll
      for (int k = 0; k < PM_UNROLL; ++k) {
        const int j = (int)base + t0 + k;
        if (FACEQ) {
          const float4 r = tile[t0 + k];
#pragma unroll
          for (int q = 0; q < PM_Q; ++q) {
            float v, w;
            const float d = pm_pair(qt[q], r.x, r.y, r.z, v, w);
            const bool lt = d < best[q];
            best[q] = lt ? d : best[q];
            bj[q] = lt ? j : bj[q];
          }
        } else {
          const float4 r0 = tile[REC * (t0 + k)], r1 = tile[REC * (t0 + k) + 1], r2 = tile[REC * (t0 + k) + 2];
          const PmTri tr = {{r0.x, r0.y, r0.z}, {r1.x, r1.y, r1.z}, {r2.x, r2.y, r2.z}};
#pragma unroll
          for (int q = 0; q < PM_Q; ++q) {
            float v, w;
            const float d = pm_pair(tr, qp[q][0], qp[q][1], qp[q][2], v, w);
            const bool lt = d < best[q];
            best[q] = lt ? d : best[q];
            bj[q] = lt ? j : bj[q];
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < PM_Q; ++q) {
    const int64_t i = (int64_t)blockIdx.x * PM_QUERIES + q * PM_BLOCK + tid;
    if (i >= queries) continue;
    if (gridDim.y == 1) {
      pm_store<FACEQ>(a, (int)i, best[q], bj[q]);
    } else {
      const size_t o = (size_t)blockIdx.y * queries + i;
      a.pd[o] = best[q];
      a.pj[o] = bj[q];
    }
  }
}

template <bool FACEQ>
__global__ void __launch_bounds__(256) k_pm_combine(const PmArgs a, int slices) {
  const int queries = FACEQ ? a.F : a.N, targets = FACEQ ? a.N : a.F;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= queries) return;
  float bd = INFINITY;
  int bj = -1;
  for (int s = 0; s < slices; ++s) {
    const float d = a.pd[(size_t)s * queries + i];
    const int j = a.pj[(size_t)s * queries + i];
    if (j < 0 || j >= targets) continue;  // the slice found nothing (an entry is never taken for an index unchecked)
    if (bj < 0 || d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
  }
  pm_store<FACEQ>(a, (int)i, bd, bj);
}

}  // namespace reni

namespace {

constexpr int64_t PM_MAX_COUNT = 0x7fffffff - reni::PM_TILE;  // N, F: an index and base + tile offset fit an int32
constexpr int64_t PM_MAX_VERTS = 0x3fffffff;                  // V (the mesh units' limit)
constexpr int64_t PM_WORKGROUPS = 512;                        // what the library's slicing aims at (two per CU)

size_t pm_align(size_t n) { return (n + 255) & ~(size_t)255; }
bool pm_sizes_ok(int64_t N, int64_t V, int64_t F) {
  return N >= 1 && V >= 1 && F >= 1 && N <= PM_MAX_COUNT && F <= PM_MAX_COUNT && V <= PM_MAX_VERTS;
}
int64_t pm_blocks(int64_t Q) { return (Q + reni::PM_QUERIES - 1) / reni::PM_QUERIES; }
// the most slices a call of Q queries may use (reni_tu_points.hip's np_cap): Q cap(Q) <= PM_WORKGROUPS PM_QUERIES
int64_t pm_cap(int64_t Q) {
  const int64_t c = PM_WORKGROUPS / pm_blocks(Q);
  return c < 1 ? 1 : c;
}
int64_t pm_slices(int64_t Q, int64_t T, int64_t asked) {
  const int64_t cap = pm_cap(Q) < T ? pm_cap(Q) : T;
  if (asked > 0) return asked < cap ? asked : cap;
  const int64_t tiles = (T + reni::PM_TILE - 1) / reni::PM_TILE;  // a slice of the library's choice holds a full tile or more
  return tiles < cap ? tiles : cap;
}
size_t pm_rows(int64_t Q) { return pm_cap(Q) > 1 ? (size_t)Q * (size_t)pm_cap(Q) : 0; }  // (one slice writes no partials)
size_t pm_need(int64_t Q) { return pm_align(pm_rows(Q) * sizeof(float)) + pm_align(pm_rows(Q) * sizeof(int32_t)) + 256; }

// the checks and the launches of both entry points; Q queries against T targets
template <bool FACEQ>
int pm_run(const char* who, int64_t N, int64_t V, int64_t F, const float* points, const float* verts, const int64_t* faces,
           int32_t slices, float* dist2, int64_t* idx, int32_t* tap_index, float* tap_weight, void* ws, size_t ws_bytes,
           void* stream) {
  if (N < 1 || V < 1 || F < 1) return tu_fail(RENI_EINVAL, who, "N, V and F must be >= 1");
  if (!pm_sizes_ok(N, V, F)) return tu_fail(RENI_EINVAL, who, "too large: need N, F <= 2^31 - 257 and V < 2^30");
  if (slices < 0) return tu_fail(RENI_EINVAL, who, "slices must be >= 0");
  if (!points || !verts || !faces || !dist2 || !idx || !tap_index || !tap_weight) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (((uintptr_t)tap_index | (uintptr_t)tap_weight) & 15) return tu_fail(RENI_EINVAL, who, "the taps must be 16-byte aligned");
  const int64_t Q = FACEQ ? F : N, T = FACEQ ? N : F;
  if (int rc = tu_check_ws(who, ws, ws_bytes, pm_need(Q))) return rc;
  const int64_t sl = pm_slices(Q, T, slices);
  reni::PmArgs a;
  a.points = points; a.verts = verts; a.faces = faces;
  a.N = (int)N; a.V = (int)V; a.F = (int)F;
  a.per = (int)((T + sl - 1) / sl);
  const size_t rows = pm_rows(Q);
  a.pd = (float*)ws;
  a.pj = (int32_t*)((char*)ws + pm_align(rows * sizeof(float)));
  a.dist2 = dist2; a.idx = idx; a.tap_index = tap_index; a.tap_weight = tap_weight;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = tu_launch(TU_COUNTED, reni::k_pm_search<FACEQ>, dim3((unsigned)pm_blocks(Q), (unsigned)sl), dim3(reni::PM_BLOCK), 0, s, a))
    return rc;
  if (sl == 1) return RENI_OK;
  return tu_launch(TU_COUNTED, reni::k_pm_combine<FACEQ>, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, a, (int)sl);
}

}  // namespace

extern "C" {

size_t reni_nearest_faces_workspace_bytes(int64_t N, int64_t V, int64_t F) { return pm_sizes_ok(N, V, F) ? pm_need(N) : 0; }

int reni_nearest_faces(int64_t N, int64_t V, int64_t F, const float* points, const float* verts, const int64_t* faces, int32_t slices,
                       float* dist2, int64_t* face_idx, int32_t* tap_index, float* tap_weight, void* ws, size_t ws_bytes,
                       void* stream) {
  return pm_run<false>("nearest faces", N, V, F, points, verts, faces, slices, dist2, face_idx, tap_index, tap_weight, ws, ws_bytes,
                       stream);
}

size_t reni_faces_nearest_points_workspace_bytes(int64_t N, int64_t V, int64_t F) { return pm_sizes_ok(N, V, F) ? pm_need(F) : 0; }

int reni_faces_nearest_points(int64_t N, int64_t V, int64_t F, const float* points, const float* verts, const int64_t* faces,
                              int32_t slices, float* dist2, int64_t* point_idx, int32_t* tap_index, float* tap_weight, void* ws,
                              size_t ws_bytes, void* stream) {
  return pm_run<true>("faces nearest points", N, V, F, points, verts, faces, slices, dist2, point_idx, tap_index, tap_weight, ws,
                      ws_bytes, stream);
}

}  // extern "C"
