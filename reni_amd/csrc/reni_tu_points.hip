// translation unit of libreni_hip.so: point clouds against point clouds, and points on a mesh -- the brute-force nearest
// neighbour search (reni_nearest_points), the gradient of the chamfer distance through it (reni_chamfer_grad), the area table
// of a mesh and area-weighted surface samples as a tap table of the texture unit (reni_mesh_sample_table,
// reni_mesh_sample_points).  include/reni_hip.h has the definitions in full ("point clouds"); DESIGN 4.4u the structure.
//
// fp32, no float atomic, no in-launch ticket, no host synchronisation, launches on `stream` only.
//
//   k_np_search    NP_Q queries per lane in registers, NP_BLOCK lanes: the targets of the workgroup's slice pass through LDS in
//                  tiles of NP_TILE 16-byte records (x, y, z, pad), every lane reads the SAME record (a broadcast, ds_read_b128),
//                  d = fmaf(dz, dz, fmaf(dy, dy, dx dx)), ascending j, strict <.  A tile's tail is padded with NaN records up
//                  to a multiple of NP_UNROLL: a NaN wins no comparison, so the walk has no remainder loop.  grid.y = slices of
//                  the target range.  One slice: writes dist2 / idx.  More: writes the partial (d, j) of its slice.
//   k_np_combine   one lane per query: the lexicographic minimum of the slices' (d, j) -- the same bits for any slicing, since
//                  every slice kept the lowest j of its smallest d.
//   k_ch_grad      one lane per point x_i: its own match, then the y_j matched to it through the sorted table (order, offsets)
//                  by reni_texture_fetch_backward's rule: a range of at most CH_SHORT entries by its lane in order, a longer
//                  one by the wave in chunks of 64 with the butterfly 32 .. 1.
//   k_ps_area      one workgroup per PS_CHUNK faces: the areas, and the chunk's sum (a scan in double, its last value).
//   k_ps_chunks    one workgroup: the scan of the chunk sums, the total at the last chunk with mass, and per chunk the running
//                  maximum of (float)(prefix / total) -- the value the CDF must have at the chunk's end.
//   k_ps_cdf       one workgroup per chunk: the chunk's scan again (the same bits), divided by the total, clamped between the
//                  bounds of the chunk and made ascending by a running maximum, flat over faces without area.
//   k_ps_sample    one lane per sample: an upper-bound search of the CDF, pytorch3d's barycentrics, an 8-tap row.
// A scan is Hillis-Steele in a wave, the waves in order, the 256-entry tiles in order (reni_tu_lights.hip's): its additions
// depend on F alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__

namespace reni {

constexpr int NP_BLOCK = 256;
constexpr int NP_Q = 2;                       // queries per lane
constexpr int NP_QUERIES = NP_BLOCK * NP_Q;   // per workgroup
constexpr int NP_TILE = 1024;                 // targets staged at a time (16 KB)
constexpr int NP_UNROLL = 8;
constexpr int CH_SHORT = 128;                 // the longest range one lane walks alone (the texture unit's TX_SHORT)
constexpr int PS_TILES = 4;
constexpr int PS_CHUNK = 256 * PS_TILES;      // faces per workgroup of the table

// ---- nearest points ----------------------------------------------------------------------------------------------------
struct NpArgs {
  const float* x;   // [N][3]
  const float* y;   // [M][3]
  int N, M;
  int per;          // targets per slice
  float* pd;        // [slices][N], slices > 1
  int32_t* pj;      // [slices][N], -1: no comparison succeeded
  float* dist2;     // [N]
  int64_t* idx;     // [N]
};

DEV float np_d(float x0, float x1, float x2, float y0, float y1, float y2) {
  const float dx = x0 - y0, dy = x1 - y1, dz = x2 - y2;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// the result of query i from the best (d, j) found; j < 0: nothing compared below +inf -> index 0 and what d(i, 0) computes
DEV void np_store(const NpArgs& a, int i, float d, int j, float x0, float x1, float x2) {
  if (j < 0) {
    j = 0;
    d = np_d(x0, x1, x2, a.y[0], a.y[1], a.y[2]);
  }
  a.dist2[i] = d;
  a.idx[i] = (int64_t)j;
}

__global__ void __launch_bounds__(NP_BLOCK) k_np_search(const NpArgs a) {
  __shared__ float4 tile[NP_TILE];
  const int tid = (int)threadIdx.x;
  float qx[NP_Q], qy[NP_Q], qz[NP_Q], best[NP_Q];
  int bj[NP_Q];
#pragma unroll
  for (int q = 0; q < NP_Q; ++q) {
    const int64_t i = min((int64_t)blockIdx.x * NP_QUERIES + q * NP_BLOCK + tid, (int64_t)a.N - 1);  // (a lane past N repeats the last query)
    qx[q] = a.x[3 * i]; qy[q] = a.x[3 * i + 1]; qz[q] = a.x[3 * i + 2];
    best[q] = INFINITY;
    bj[q] = -1;
  }
  const int64_t j0 = (int64_t)blockIdx.y * a.per;
  const int64_t j1 = min(j0 + (int64_t)a.per, (int64_t)a.M);
  for (int64_t base = j0; base < j1; base += NP_TILE) {
    const int n = (int)min((int64_t)NP_TILE, j1 - base);
    const int n8 = (n + NP_UNROLL - 1) / NP_UNROLL * NP_UNROLL;  // <= NP_TILE: NP_TILE is a multiple of NP_UNROLL
    __syncthreads();
    for (int t = tid; t < n8; t += NP_BLOCK) {
      float4 r = make_float4(NAN, NAN, NAN, 0.f);
      if (t < n) {
        const float* p = a.y + 3 * (base + t);
        r.x = p[0]; r.y = p[1]; r.z = p[2];
      }
      tile[t] = r;
    }
    __syncthreads();
    for (int t0 = 0; t0 < n8; t0 += NP_UNROLL) {
#pragma unroll
      for (int k = 0; k < NP_UNROLL; ++k) {
        const float4 r = tile[t0 + k];
        const int j = (int)base + t0 + k;
#pragma unroll
        for (int q = 0; q < NP_Q; ++q) {
          const float d = np_d(qx[q], qy[q], qz[q], r.x, r.y, r.z);
          const bool lt = d < best[q];
          best[q] = lt ? d : best[q];
          bj[q] = lt ? j : bj[q];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NP_Q; ++q) {
    const int64_t i = (int64_t)blockIdx.x * NP_QUERIES + q * NP_BLOCK + tid;
    if (i >= a.N) continue;
    if (gridDim.y == 1) {
      np_store(a, (int)i, best[q], bj[q], qx[q], qy[q], qz[q]);
    } else {
      const size_t o = (size_t)blockIdx.y * a.N + i;
      a.pd[o] = best[q];
      a.pj[o] = bj[q];
    }
  }
}

__global__ void __launch_bounds__(256) k_np_combine(const NpArgs a, int slices) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  float bd = INFINITY;
  int bj = -1;
  for (int s = 0; s < slices; ++s) {
    const float d = a.pd[(size_t)s * a.N + i];
    const int j = a.pj[(size_t)s * a.N + i];
    if (j < 0 || j >= a.M) continue;  // the slice found nothing (an entry is never taken for an index unchecked)
    if (bj < 0 || d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
  }
  np_store(a, (int)i, bd, bj, a.x[3 * i], a.x[3 * i + 1], a.x[3 * i + 2]);
}

// ---- the chamfer gradient ----------------------------------------------------------------------------------------------
struct ChArgs {
  const float* x;         // [N][3]
  const float* y;         // [M][3]
  const int64_t* idx_xy;  // [N] or NULL (w_x = 0)
  const int64_t* order;   // [M] or NULL (w_y = 0)
  const int64_t* offsets; // [N + 1]
  const float* g;         // [1]
  float cx, cy;           // 2 w_x / N, 2 w_y / M
  int64_t N, M;
  float* grad;            // [N][3]
};

DEV void ch_add(const ChArgs& a, int64_t j, const float (&xi)[3], float (&acc)[3]) {
  if ((uint64_t)j >= (uint64_t)a.M) return;  // a malformed entry adds nothing
  const float* p = a.y + 3 * j;
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] += xi[c] - p[c];
}

__global__ void __launch_bounds__(256) k_ch_grad(const ChArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < a.N;
  float xi[3] = {0.f, 0.f, 0.f}, own[3] = {0.f, 0.f, 0.f}, acc[3] = {0.f, 0.f, 0.f};
  int64_t k0 = 0, k1 = 0;
  if (live) {
#pragma unroll
    for (int c = 0; c < 3; ++c) xi[c] = a.x[3 * i + c];
    if (a.idx_xy) ch_add(a, a.idx_xy[i], xi, own);
    if (a.order) {
      k0 = min(max(a.offsets[i], (int64_t)0), a.M);
      k1 = min(max(a.offsets[i + 1], k0), a.M);
    }
  }
  const bool lng = k1 - k0 > CH_SHORT;
  if (!lng)
    for (int64_t k = k0; k < k1; ++k) ch_add(a, a.order[k], xi, acc);
  unsigned long long todo = __ballot(lng);
  while (todo) {  // wave-uniform: the long ranges of this wave's 64 points, in lane order
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t b = __shfl(k0, owner), n = __shfl(k1, owner) - b;
    float xo[3], part[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) xo[c] = __shfl(xi[c], owner);
    for (int64_t k = lane; k < n; k += 64) ch_add(a, a.order[b + k], xo, part);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s = part[c];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
      if (lane == owner) acc[c] = s;
    }
  }
  if (!live) return;
  const float g = a.g[0];
  const float gx = g * a.cx, gy = g * a.cy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = 0.f;
    if (a.idx_xy) v = gx * own[c];
    if (a.order) v = v + gy * acc[c];
    a.grad[3 * i + c] = v;
  }
}

// ---- the area table ----------------------------------------------------------------------------------------------------
struct PsArgs {
  const float* verts;    // [V][3]
  const int64_t* faces;  // [F][3]
  int V, F;
  int chunks;
  float* area;           // [F]
  float* cdf;            // [F]
  double* csum;          // [chunks]      the chunk sums
  double* cincl;         // [chunks + 1]  their inclusive scan; [chunks]: the total (0: no mass)
  float* bound;          // [chunks]      the CDF at the chunk's end
};

// face f's area: 0 unless its indices lie in [0, V), are pairwise different and the area is finite
DEV float ps_area(const PsArgs& a, int64_t f) {
  int64_t i[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) i[k] = a.faces[3 * f + k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (i[k] < 0 || i[k] >= a.V) return 0.f;
  if (i[0] == i[1] || i[0] == i[2] || i[1] == i[2]) return 0.f;
  const float* p0 = a.verts + 3 * i[0];
  const float* p1 = a.verts + 3 * i[1];
  const float* p2 = a.verts + 3 * i[2];
  const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
  const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const float ar = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
  return ar > 0.f && ar <= 3.4028234663852886e38f ? ar : 0.f;  // (a NaN fails the comparisons)
}

// inclusive scan of one value per thread over the workgroup's 256 threads
DEV double ps_scan_d(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  if (lane == 63) red[wave] = v;
  __syncthreads();
  const double w0 = red[0], w1 = red[1], w2 = red[2];
  const double off = wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : (w0 + w1) + w2;
  __syncthreads();
  return wave == 0 ? v : off + v;
}

// inclusive running maximum of one value per thread (exact: any order gives it); *total = the maximum of all 256
DEV float ps_scan_max(float v, float* red, float* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(v, d, 64);
    if (lane >= d) v = fmaxf(v, t);
  }
  if (lane == 63) red[wave] = v;
  __syncthreads();
  const float w0 = red[0], w1 = red[1], w2 = red[2], w3 = red[3];
  const float off = wave == 0 ? -INFINITY : wave == 1 ? w0 : wave == 2 ? fmaxf(w0, w1) : fmaxf(fmaxf(w0, w1), w2);
  __syncthreads();
  *total = fmaxf(fmaxf(w0, w1), fmaxf(w2, w3));
  return fmaxf(v, off);
}

DEV int ps_block_max_i(int v, int* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = max(max(red[0], red[1]), max(red[2], red[3]));
  __syncthreads();
  return r;
}

// The inclusive scan of the chunk's PS_CHUNK values, entry k * 256 + thread in val[k] (in place): tile after tile, the carry
// added in front.  Returns the scan's last value in every thread.
DEV double ps_chunk_scan(double (&val)[PS_TILES], double* red, double* last) {
  double carry = 0.0;
#pragma unroll
  for (int k = 0; k < PS_TILES; ++k) {
    const double inc = ps_scan_d(val[k], red);
    val[k] = k == 0 ? inc : carry + inc;
    if (threadIdx.x == 255) *last = val[k];
    __syncthreads();
    carry = *last;
    __syncthreads();
  }
  return carry;
}

__global__ void __launch_bounds__(256) k_ps_area(const PsArgs a) {
  __shared__ double red[4];
  __shared__ double last;
  const int64_t base = (int64_t)blockIdx.x * PS_CHUNK;
  double val[PS_TILES];
#pragma unroll
  for (int k = 0; k < PS_TILES; ++k) {
    const int64_t f = base + k * 256 + (int)threadIdx.x;
    float ar = 0.f;
    if (f < a.F) {
      ar = ps_area(a, f);
      a.area[f] = ar;
    }
    val[k] = (double)ar;
  }
  const double total = ps_chunk_scan(val, red, &last);
  if (threadIdx.x == 0) a.csum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_ps_chunks(const PsArgs a) {
  __shared__ double red[4];
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ double last;
  const int tid = (int)threadIdx.x;
  double carry = 0.0;
  int top = -1;
  for (int b0 = 0; b0 < a.chunks; b0 += 256) {  // (uniform over the workgroup)
    const int b = b0 + tid;
    const double v = b < a.chunks ? a.csum[b] : 0.0;
    if (v > 0.0) top = b;
    const double inc = ps_scan_d(v, red);
    const double s = b0 == 0 ? inc : carry + inc;
    if (b < a.chunks) a.cincl[b] = s;
    if (tid == 255) last = s;
    __syncthreads();
    carry = last;
    __syncthreads();
  }
  const int at = ps_block_max_i(top, redi);  // the last chunk with mass
  const double total = at >= 0 ? a.cincl[at] : 0.0;  // (written above by this workgroup, behind its barriers)
  if (tid == 0) a.cincl[a.chunks] = total;
  float fcarry = 0.f;
  for (int b0 = 0; b0 < a.chunks; b0 += 256) {
    const int b = b0 + tid;
    float q = 0.f;
    if (b < a.chunks && at >= 0 && a.csum[b] > 0.0) q = (float)(a.cincl[b] / total);
    float tile_max;
    const float m = fmaxf(ps_scan_max(q, redf, &tile_max), fcarry);
    if (b < a.chunks) a.bound[b] = m;
    fcarry = fmaxf(fcarry, tile_max);
  }
}

__global__ void __launch_bounds__(256) k_ps_cdf(const PsArgs a) {
  __shared__ double red[4];
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ double last;
  const int tid = (int)threadIdx.x;
  const int b = (int)blockIdx.x;
  const int64_t base = (int64_t)b * PS_CHUNK;
  const double total = a.cincl[a.chunks];
  if (!(total > 0.0)) {  // no mass anywhere (uniform over the grid)
#pragma unroll
    for (int k = 0; k < PS_TILES; ++k) {
      const int64_t f = base + k * 256 + tid;
      if (f < a.F) a.cdf[f] = 0.f;
    }
    return;
  }
  const double excl = b > 0 ? a.cincl[b - 1] : 0.0;
  const float lo = b > 0 ? a.bound[b - 1] : 0.f, hi = a.bound[b];
  double val[PS_TILES];
  unsigned mass = 0;
  int top = -1;
#pragma unroll
  for (int k = 0; k < PS_TILES; ++k) {
    const int64_t f = base + k * 256 + tid;
    const float ar = f < a.F ? a.area[f] : 0.f;
    if (ar > 0.f) { mass |= 1u << k; top = k * 256 + tid; }
    val[k] = (double)ar;
  }
  ps_chunk_scan(val, red, &last);  // k_ps_area's scan: the same bits
  const int at = ps_block_max_i(top, redi);  // the chunk's last face with mass
  float carry = lo;
#pragma unroll
  for (int k = 0; k < PS_TILES; ++k) {
    float q = 0.f;
    if ((mass >> k) & 1u) q = fminf(fmaxf((float)((excl + val[k]) / total), lo), hi);
    float tile_max;
    float m = fmaxf(ps_scan_max(q, redf, &tile_max), carry);
    carry = fmaxf(carry, tile_max);
    if (at >= 0 && k * 256 + tid >= at) m = hi;  // the chunk ends on exactly what the next one starts from
    const int64_t f = base + k * 256 + tid;
    if (f < a.F) a.cdf[f] = m;
  }
}

// ---- sampling ----------------------------------------------------------------------------------------------------------
struct SmArgs {
  const int64_t* faces;  // [F][3]
  const float* area;     // [F]
  const float* cdf;      // [F]
  const float* u;        // [S][3]
  int V, F, S;
  int32_t* tap_index;    // [S][8]
  float* tap_weight;     // [S][8]
  int64_t* face_idx;     // [S]
};

DEV float sm_unit(float v, float top) { return fminf(fmaxf(v, 0.f), top); }  // (a NaN becomes 0)

__global__ void __launch_bounds__(256) k_ps_sample(const SmArgs a) {
  const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (s >= a.S) return;
  const float u0 = sm_unit(a.u[3 * (size_t)s], 0x1.fffffep-1f), u1 = sm_unit(a.u[3 * (size_t)s + 1], 1.f),
              u2 = sm_unit(a.u[3 * (size_t)s + 2], 1.f);
  int lo = 0, hi = a.F;
  while (lo < hi) {  // the number of entries <= u0
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (a.cdf[mid] <= u0) lo = mid + 1;
    else hi = mid;
  }
  const int f = min(lo, a.F - 1);
  int32_t ii[3] = {0, 0, 0};
  float w[3] = {0.f, 0.f, 0.f};
  bool ok = a.cdf[a.F - 1] == 1.f && a.area[f] > 0.f;  // a table without mass ends below 1
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t v = a.faces[3 * (size_t)f + k];
      ok = ok && v >= 0 && v < a.V;
      ii[k] = (int32_t)v;
    }
  }
  if (ok) {
    const float r = sqrtf(u1);
    w[0] = 1.f - r;
    w[1] = r * (1.f - u2);
    w[2] = r * u2;
  } else {
    ii[0] = ii[1] = ii[2] = 0;
  }
  int32_t* ip = a.tap_index + 8 * (size_t)s;
  float* wp = a.tap_weight + 8 * (size_t)s;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ip[k] = k < 3 ? ii[k] : 0;
    wp[k] = k < 3 ? w[k] : 0.f;
  }
  a.face_idx[s] = ok ? (int64_t)f : 0;
}

}  // namespace reni

namespace {

constexpr int64_t NP_MAX_POINTS = 0x7fffffff - reni::NP_TILE;  // N, M: an index and base + tile offset fit an int32
constexpr int64_t NP_WORKGROUPS = 512;                         // what the library's slicing aims at (two per CU)
constexpr int64_t PS_MAX_ELEMS = 0x3fffffff;                   // V, F (the mesh units' limit)
constexpr int64_t PS_MAX_SAMPLES = 0x0fffffff;                 // the texture unit's P

size_t np_align(size_t n) { return (n + 255) & ~(size_t)255; }
bool np_sizes_ok(int64_t N, int64_t M) { return N >= 1 && M >= 1 && N <= NP_MAX_POINTS && M <= NP_MAX_POINTS; }
int64_t np_blocks(int64_t N) { return (N + reni::NP_QUERIES - 1) / reni::NP_QUERIES; }
// the most slices a call of N queries may use: N cap(N) <= NP_WORKGROUPS NP_QUERIES, so the workspace is bounded
int64_t np_cap(int64_t N) {
  const int64_t c = NP_WORKGROUPS / np_blocks(N);
  return c < 1 ? 1 : c;
}
int64_t np_slices(int64_t N, int64_t M, int64_t asked) {
  const int64_t cap = np_cap(N) < M ? np_cap(N) : M;
  if (asked > 0) return asked < cap ? asked : cap;
  const int64_t tiles = (M + reni::NP_TILE - 1) / reni::NP_TILE;  // a slice of the library's choice holds a full tile or more
  return tiles < cap ? tiles : cap;
}
size_t np_rows(int64_t N) { return np_cap(N) > 1 ? (size_t)N * (size_t)np_cap(N) : 0; }  // (one slice writes no partials)
size_t np_need(int64_t N) { return np_align(np_rows(N) * sizeof(float)) + np_align(np_rows(N) * sizeof(int32_t)) + 256; }

int64_t ps_chunks(int64_t F) { return (F + reni::PS_CHUNK - 1) / reni::PS_CHUNK; }
size_t ps_need(int64_t F) {
  const size_t c = (size_t)ps_chunks(F);
  return np_align(c * sizeof(double)) + np_align((c + 1) * sizeof(double)) + np_align(c * sizeof(float));
}

}  // namespace

extern "C" {

size_t reni_nearest_points_workspace_bytes(int64_t N, int64_t M) { return np_sizes_ok(N, M) ? np_need(N) : 0; }

int reni_nearest_points(int64_t N, int64_t M, const float* x, const float* y, int32_t slices, float* dist2, int64_t* idx, void* ws,
                        size_t ws_bytes, void* stream) {
  const char* who = "nearest points";
  if (N < 1 || M < 1) return tu_fail(RENI_EINVAL, who, "N and M must be >= 1");
  if (!np_sizes_ok(N, M)) return tu_fail(RENI_EINVAL, who, "too large: need N, M <= 2^31 - 1025");
  if (slices < 0) return tu_fail(RENI_EINVAL, who, "slices must be >= 0");
  if (!x || !y || !dist2 || !idx) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = tu_check_ws(who, ws, ws_bytes, np_need(N))) return rc;
  const int64_t sl = np_slices(N, M, slices);
  reni::NpArgs a;
  a.x = x; a.y = y; a.N = (int)N; a.M = (int)M;
  a.per = (int)((M + sl - 1) / sl);
  const size_t rows = np_rows(N);
  a.pd = (float*)ws;
  a.pj = (int32_t*)((char*)ws + np_align(rows * sizeof(float)));
  a.dist2 = dist2; a.idx = idx;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = tu_launch(TU_COUNTED, reni::k_np_search, dim3((unsigned)np_blocks(N), (unsigned)sl), dim3(reni::NP_BLOCK), 0, s, a))
    return rc;
  if (sl == 1) return RENI_OK;
  return tu_launch(TU_COUNTED, reni::k_np_combine, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a, (int)sl);
}

int reni_chamfer_grad(int64_t N, int64_t M, const float* x, const float* y, const int64_t* idx_xy, const int64_t* order,
                      const int64_t* offsets, float w_x, float w_y, const float* g, float* grad_x, void* stream) {
  const char* who = "chamfer grad";
  if (N < 1 || M < 1) return tu_fail(RENI_EINVAL, who, "N and M must be >= 1");
  if (!np_sizes_ok(N, M)) return tu_fail(RENI_EINVAL, who, "too large: need N, M <= 2^31 - 1025");
  if (!(w_x >= 0.f) || !(w_y >= 0.f) || !isfinite(w_x) || !isfinite(w_y))
    return tu_fail(RENI_EINVAL, who, "the weights must be >= 0 and finite");
  if (!x || !y || !g || !grad_x) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (w_x > 0.f && !idx_xy) return tu_fail(RENI_EINVAL, who, "NULL idx_xy with w_x > 0");
  if (w_y > 0.f && (!order || !offsets)) return tu_fail(RENI_EINVAL, who, "NULL order or offsets with w_y > 0");
  reni::ChArgs a;
  a.x = x; a.y = y;
  a.idx_xy = w_x > 0.f ? idx_xy : nullptr;
  a.order = w_y > 0.f ? order : nullptr;
  a.offsets = offsets;
  a.g = g;
  a.cx = (2.f * w_x) / (float)N;
  a.cy = (2.f * w_y) / (float)M;
  a.N = N; a.M = M;
  a.grad = grad_x;
  return tu_launch(TU_COUNTED, reni::k_ch_grad, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

size_t reni_mesh_sample_table_workspace_bytes(int64_t F) { return F >= 1 && F <= PS_MAX_ELEMS ? ps_need(F) : 0; }

int reni_mesh_sample_table(int64_t V, int64_t F, const float* verts, const int64_t* faces, float* table, void* ws, size_t ws_bytes,
                           void* stream) {
  const char* who = "mesh sample table";
  if (V < 1 || F < 1 || V > PS_MAX_ELEMS || F > PS_MAX_ELEMS) return tu_fail(RENI_EINVAL, who, "bad V / F");
  if (!verts || !faces || !table) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = tu_check_ws(who, ws, ws_bytes, ps_need(F))) return rc;
  const size_t c = (size_t)ps_chunks(F);
  reni::PsArgs a;
  a.verts = verts; a.faces = faces; a.V = (int)V; a.F = (int)F; a.chunks = (int)c;
  a.area = table; a.cdf = table + F;
  char* p = (char*)ws;
  a.csum = (double*)p; p += np_align(c * sizeof(double));
  a.cincl = (double*)p; p += np_align((c + 1) * sizeof(double));
  a.bound = (float*)p;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = tu_launch(TU_COUNTED, reni::k_ps_area, dim3((unsigned)c), dim3(256), 0, s, a)) return rc;
  if (int rc = tu_launch(TU_COUNTED, reni::k_ps_chunks, dim3(1), dim3(256), 0, s, a)) return rc;
  return tu_launch(TU_COUNTED, reni::k_ps_cdf, dim3((unsigned)c), dim3(256), 0, s, a);
}

int reni_mesh_sample_points(int64_t V, int64_t F, int64_t S, const int64_t* faces, const float* table, const float* u,
                            int32_t* tap_index, float* tap_weight, int64_t* face_idx, void* stream) {
  const char* who = "mesh sample points";
  if (V < 1 || F < 1 || V > PS_MAX_ELEMS || F > PS_MAX_ELEMS) return tu_fail(RENI_EINVAL, who, "bad V / F");
  if (S < 1 || S > PS_MAX_SAMPLES) return tu_fail(RENI_EINVAL, who, "S must be in [1, 2^28)");
  if (!faces || !table || !u || !tap_index || !tap_weight || !face_idx) return tu_fail(RENI_EINVAL, who, "NULL argument");
  reni::SmArgs a;
  a.faces = faces; a.area = table; a.cdf = table + F; a.u = u;
  a.V = (int)V; a.F = (int)F; a.S = (int)S;
  a.tap_index = tap_index; a.tap_weight = tap_weight; a.face_idx = face_idx;
  return tu_launch(TU_COUNTED, reni::k_ps_sample, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

}  // extern "C"
