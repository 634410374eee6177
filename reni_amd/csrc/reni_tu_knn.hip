// translation unit of libreni_hip.so: cloud neighbourhoods -- the K nearest neighbours of every point by brute force
// (reni_knn_points) and normals from the principal axes of those neighbourhoods (reni_cloud_normals).  include/reni_hip.h has
// the definitions in full ("cloud neighbourhoods"); DESIGN 4.4w the structure.
//
// fp32, no float atomic, no in-launch ticket, no host synchronisation, launches on `stream` only.
//
//   k_knn_search<KB>  k_np_search's skeleton with ONE query per lane and a list of KB pairs (d, j) per lane in registers,
//                     ascending: the targets of the workgroup's slice pass through LDS in tiles of KN_TILE 16-byte records
//                     that every lane reads at the same address, padded with NaN records to a multiple of KN_UNROLL.  Per
//                     target: d against the lane's last slot (strict <); only where a wave ballot says some lane improved,
//                     the fully unrolled insertion -- slot s takes the new pair where d < D[s] and d >= D[s - 1], the old
//                     D[s - 1] where d < D[s - 1] (every index a constant: the lists never leave the registers).  Targets come
//                     in ascending j, so among equal d the lower j stays in front.  K < KB runs in the next bucket and stores
//                     its first K slots.  grid.y = slices of the target range.  One slice: writes dist2 / idx.  More: writes
//                     the slice's K pairs.
//   k_knn_combine<KB> one lane per query: the slices' lists, slice after slice and slot after slot, through the same insertion
//                     into one register list.  The slices hold ascending ranges of j and every list is in lexicographic
//                     order, so j ascends among equal d here too and the strict < IS the lexicographic merge of (d, j) --
//                     the same bits for any slicing.
//   k_cn_normals      one lane per point: the mean, the six centred second moments, cyclic Jacobi, the sign rule.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__

namespace reni {

constexpr int KN_BLOCK = 256;   // lanes, and queries, per workgroup
constexpr int KN_TILE = 1024;   // targets staged at a time (16 KB)
constexpr int KN_UNROLL = 4;
constexpr int KN_MAX_K = 32;
constexpr int CN_SWEEPS = 6;    // cyclic Jacobi sweeps of the 3 x 3 problem

// ---- k nearest points --------------------------------------------------------------------------------------------------
struct KnArgs {
  const float* x;   // [N][3]
  const float* y;   // [M][3]
  int N, M, K;
  int per;          // targets per slice
  float* pd;        // [slices][N][K], slices > 1
  int32_t* pj;      // [slices][N][K], -1: an empty slot
  float* dist2;     // [N][K]
  int64_t* idx;     // [N][K]
};

DEV float kn_d(float x0, float x1, float x2, float y0, float y1, float y2) {  // reni_nearest_points' expression
  const float dx = x0 - y0, dy = x1 - y1, dz = x2 - y2;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// the pair (d, j) into the ascending list where it is in front of slot s (lt(s)): a lane whose pair is in front of no slot
// keeps its list.  From the tail, so every slot reads its predecessor before that is overwritten.
template <int KB>
DEV void kn_insert(float (&D)[KB], int (&J)[KB], float d, int j) {
#pragma unroll
  for (int s = KB - 1; s >= 0; --s) {
    const bool here = d < D[s];
    bool prev = false;
    if (s > 0) prev = d < D[s - 1];
    const float nd = prev ? D[s > 0 ? s - 1 : 0] : d;
    const int nj = prev ? J[s > 0 ? s - 1 : 0] : j;
    D[s] = here ? nd : D[s];
    J[s] = here ? nj : J[s];
  }
}

template <int KB>
DEV void kn_store(const KnArgs& a, int64_t i, const float (&D)[KB], const int (&J)[KB]) {
  float* dp = a.dist2 + (size_t)i * a.K;
  int64_t* ip = a.idx + (size_t)i * a.K;
#pragma unroll
  for (int s = 0; s < KB; ++s)
    if (s < a.K) {
      const bool ok = J[s] >= 0 && J[s] < a.M;  // (nothing else is ever written)
      dp[s] = ok ? D[s] : INFINITY;
      ip[s] = ok ? (int64_t)J[s] : (int64_t)-1;
    }
}

template <int KB>
__global__ void __launch_bounds__(KN_BLOCK) k_knn_search(const KnArgs a) {
  __shared__ float4 tile[KN_TILE];
  const int tid = (int)threadIdx.x;
  const int64_t iq = (int64_t)blockIdx.x * KN_BLOCK + tid;
  const int64_t ic = min(iq, (int64_t)a.N - 1);  // (a lane past N repeats the last query)
  const float qx = a.x[3 * ic], qy = a.x[3 * ic + 1], qz = a.x[3 * ic + 2];
  float D[KB];
  int J[KB];
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    D[s] = INFINITY;
    J[s] = -1;
  }
  const int64_t j0 = (int64_t)blockIdx.y * a.per;
  const int64_t j1 = min(j0 + (int64_t)a.per, (int64_t)a.M);
  for (int64_t base = j0; base < j1; base += KN_TILE) {
    const int n = (int)min((int64_t)KN_TILE, j1 - base);
    const int n4 = (n + KN_UNROLL - 1) / KN_UNROLL * KN_UNROLL;  // <= KN_TILE: KN_TILE is a multiple of KN_UNROLL
    __syncthreads();
    for (int t = tid; t < n4; t += KN_BLOCK) {
      float4 r = make_float4(NAN, NAN, NAN, 0.f);
      if (t < n) {
        const float* p = a.y + 3 * (base + t);
        r.x = p[0]; r.y = p[1]; r.z = p[2];
      }
      tile[t] = r;
    }
    __syncthreads();
    for (int t0 = 0; t0 < n4; t0 += KN_UNROLL) {
#pragma unroll
      for (int k = 0; k < KN_UNROLL; ++k) {
        const float4 r = tile[t0 + k];
        const int j = (int)base + t0 + k;
        const float d = kn_d(qx, qy, qz, r.x, r.y, r.z);
        if (__ballot(d < D[KB - 1])) kn_insert<KB>(D, J, d, j);  // (wave-uniform; a NaN and +inf are in front of nothing)
      }
    }
  }
  if (iq >= a.N) return;
  if (gridDim.y == 1) {
    kn_store<KB>(a, iq, D, J);
  } else {
    const size_t o = ((size_t)blockIdx.y * a.N + iq) * a.K;
#pragma unroll
    for (int s = 0; s < KB; ++s)
      if (s < a.K) {
        a.pd[o + s] = D[s];
        a.pj[o + s] = J[s];
      }
  }
}

template <int KB>
__global__ void __launch_bounds__(256) k_knn_combine(const KnArgs a, int slices) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.N;
  float D[KB];
  int J[KB];
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    D[s] = INFINITY;
    J[s] = -1;
  }
  for (int sl = 0; sl < slices; ++sl) {  // ascending ranges of j
    const size_t o = ((size_t)sl * a.N + (live ? i : 0)) * a.K;
    for (int k = 0; k < a.K; ++k) {      // each in lexicographic order
      float d = INFINITY;
      int j = -1;
      if (live) {
        d = a.pd[o + k];
        j = a.pj[o + k];
      }
      d = j >= 0 && j < a.M ? d : INFINITY;  // (an entry is never taken for an index unchecked; +inf is in front of nothing)
      if (__ballot(d < D[KB - 1])) kn_insert<KB>(D, J, d, j);
    }
  }
  if (live) kn_store<KB>(a, i, D, J);
}

// ---- cloud normals -----------------------------------------------------------------------------------------------------
struct CnArgs {
  const float* y;       // [M][3]
  const int64_t* idx;   // [N][K]
  const float* view;    // [3] or NULL
  int N, M, K;
  float* normals;       // [N][3]
  float* eig;           // [N][3]
};

// one Jacobi rotation of the symmetric A (upper triangle in use) in the plane (P, Q), R the third axis; V's columns follow
template <int P, int Q, int R>
DEV void cn_rotate(float (&A)[3][3], float (&V)[3][3]) {
  const float apq = A[P][Q];
  if (apq == 0.f) return;
  const float theta = (A[Q][Q] - A[P][P]) / (2.f * apq);
  const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.f)));  // (theta = +-inf or NaN-free: t -> 0)
  const float c = 1.f / sqrtf(fmaf(t, t, 1.f));
  const float s = t * c;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = 0.f;
  A[Q][P] = 0.f;
  const float arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

// the columns of V and the values w ordered so that w[P] <= w[Q]
template <int P, int Q>
DEV void cn_order(float (&w)[3], float (&V)[3][3]) {
  const bool sw = w[Q] < w[P];
  const float a = w[P], b = w[Q];
  w[P] = sw ? b : a;
  w[Q] = sw ? a : b;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vp = V[k][P], vq = V[k][Q];
    V[k][P] = sw ? vq : vp;
    V[k][Q] = sw ? vp : vq;
  }
}

__global__ void __launch_bounds__(256) k_cn_normals(const CnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int64_t* row = a.idx + (size_t)i * a.K;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  int cnt = 0;
  for (int k = 0; k < a.K; ++k) {
    const int64_t j = row[k];
    if (j < 0 || j >= a.M) continue;
    const float* p = a.y + 3 * j;
    s0 += p[0]; s1 += p[1]; s2 += p[2];
    ++cnt;
  }
  float n[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f};
  if (cnt >= 3) {
    const float fc = (float)cnt;
    const float m0 = s0 / fc, m1 = s1 / fc, m2 = s2 / fc;
    float cxx = 0.f, cxy = 0.f, cxz = 0.f, cyy = 0.f, cyz = 0.f, czz = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const int64_t j = row[k];
      if (j < 0 || j >= a.M) continue;
      const float* p = a.y + 3 * j;
      const float dx = p[0] - m0, dy = p[1] - m1, dz = p[2] - m2;
      cxx = fmaf(dx, dx, cxx); cxy = fmaf(dx, dy, cxy); cxz = fmaf(dx, dz, cxz);
      cyy = fmaf(dy, dy, cyy); cyz = fmaf(dy, dz, cyz); czz = fmaf(dz, dz, czz);
    }
    float A[3][3] = {{cxx / fc, cxy / fc, cxz / fc}, {cxy / fc, cyy / fc, cyz / fc}, {cxz / fc, cyz / fc, czz / fc}};
    float V[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll 1
    for (int sweep = 0; sweep < CN_SWEEPS; ++sweep) {
      cn_rotate<0, 1, 2>(A, V);
      cn_rotate<0, 2, 1>(A, V);
      cn_rotate<1, 2, 0>(A, V);
    }
    w[0] = A[0][0]; w[1] = A[1][1]; w[2] = A[2][2];
    cn_order<0, 1>(w, V);
    cn_order<1, 2>(w, V);
    cn_order<0, 1>(w, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = fmaxf(w[k], 0.f);  // (a NaN becomes 0)
    const float v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];
    const float len = sqrtf(fmaf(v2, v2, fmaf(v1, v1, v0 * v0)));
    n[0] = v0 / len; n[1] = v1 / len; n[2] = v2 / len;
    const float chk = (n[0] + n[1]) + n[2];
    if (!(fabsf(chk) <= 2.f)) { n[0] = 0.f; n[1] = 0.f; n[2] = 1.f; }  // moments that are not finite: a unit vector all the same
    float sgn;
    if (a.view) {
      const float* p = a.y + 3 * i;  // (the host checked N <= M)
      const float e0 = a.view[0] - p[0], e1 = a.view[1] - p[1], e2 = a.view[2] - p[2];
      sgn = fmaf(n[2], e2, fmaf(n[1], e1, n[0] * e0));
    } else {
      sgn = n[0];
      float top = fabsf(n[0]);
      if (fabsf(n[1]) > top) { top = fabsf(n[1]); sgn = n[1]; }
      if (fabsf(n[2]) > top) sgn = n[2];
    }
    if (sgn < 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.normals[3 * i + k] = n[k];
    a.eig[3 * i + k] = w[k];
  }
}

}  // namespace reni

namespace {

constexpr int64_t KN_MAX_POINTS = 0x7fffffff - reni::KN_TILE;  // N, M: reni_nearest_points' limit
constexpr int64_t KN_WORKGROUPS = 512;                         // what the library's slicing aims at (two per CU)

size_t kn_align(size_t n) { return (n + 255) & ~(size_t)255; }
bool kn_sizes_ok(int64_t N, int64_t M, int64_t K) {
  return N >= 1 && M >= 1 && N <= KN_MAX_POINTS && M <= KN_MAX_POINTS && K >= 1 && K <= reni::KN_MAX_K;
}
int64_t kn_blocks(int64_t N) { return (N + reni::KN_BLOCK - 1) / reni::KN_BLOCK; }
// np_slices' cap rule: the most slices a call of N queries may use, N cap(N) <= KN_WORKGROUPS KN_BLOCK
int64_t kn_cap(int64_t N) {
  const int64_t c = KN_WORKGROUPS / kn_blocks(N);
  return c < 1 ? 1 : c;
}
int64_t kn_slices(int64_t N, int64_t M, int64_t asked) {
  const int64_t cap = kn_cap(N) < M ? kn_cap(N) : M;
  if (asked > 0) return asked < cap ? asked : cap;
  const int64_t tiles = (M + reni::KN_TILE - 1) / reni::KN_TILE;  // a slice of the library's choice holds a full tile or more
  return tiles < cap ? tiles : cap;
}
size_t kn_rows(int64_t N, int64_t K) { return kn_cap(N) > 1 ? (size_t)N * (size_t)kn_cap(N) * (size_t)K : 0; }
size_t kn_need(int64_t N, int64_t K) {
  return kn_align(kn_rows(N, K) * sizeof(float)) + kn_align(kn_rows(N, K) * sizeof(int32_t)) + 256;
}

template <int KB>
int kn_run(const reni::KnArgs& a, int64_t N, int64_t sl, hipStream_t s) {
  if (int rc = tu_launch(TU_COUNTED, reni::k_knn_search<KB>, dim3((unsigned)kn_blocks(N), (unsigned)sl), dim3(reni::KN_BLOCK), 0, s, a))
    return rc;
  if (sl == 1) return RENI_OK;
  return tu_launch(TU_COUNTED, reni::k_knn_combine<KB>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a, (int)sl);
}

}  // namespace

extern "C" {

size_t reni_knn_points_workspace_bytes(int64_t N, int64_t M, int64_t K) { return kn_sizes_ok(N, M, K) ? kn_need(N, K) : 0; }

int reni_knn_points(int64_t N, int64_t M, int64_t K, const float* x, const float* y, int32_t slices, float* dist2, int64_t* idx,
                    void* ws, size_t ws_bytes, void* stream) {
  const char* who = "knn points";
  if (N < 1 || M < 1) return tu_fail(RENI_EINVAL, who, "N and M must be >= 1");
  if (K < 1 || K > reni::KN_MAX_K) return tu_fail(RENI_EINVAL, who, "K must be in [1, 32]");
  if (!kn_sizes_ok(N, M, K)) return tu_fail(RENI_EINVAL, who, "too large: need N, M <= 2^31 - 1025");
  if (slices < 0) return tu_fail(RENI_EINVAL, who, "slices must be >= 0");
  if (!x || !y || !dist2 || !idx) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = tu_check_ws(who, ws, ws_bytes, kn_need(N, K))) return rc;
  const int64_t sl = kn_slices(N, M, slices);
  reni::KnArgs a;
  a.x = x; a.y = y; a.N = (int)N; a.M = (int)M; a.K = (int)K;
  a.per = (int)((M + sl - 1) / sl);
  a.pd = (float*)ws;
  a.pj = (int32_t*)((char*)ws + kn_align(kn_rows(N, K) * sizeof(float)));
  a.dist2 = dist2; a.idx = idx;
  hipStream_t s = (hipStream_t)stream;
  if (K <= 4) return kn_run<4>(a, N, sl, s);
  if (K <= 8) return kn_run<8>(a, N, sl, s);
  if (K <= 16) return kn_run<16>(a, N, sl, s);
  return kn_run<32>(a, N, sl, s);
}

int reni_cloud_normals(int64_t N, int64_t M, int64_t K, const float* y, const int64_t* idx, const float* viewpoint, float* normals,
                       float* eigenvalues, void* stream) {
  const char* who = "cloud normals";
  if (N < 1 || M < 1) return tu_fail(RENI_EINVAL, who, "N and M must be >= 1");
  if (K < 1 || K > reni::KN_MAX_K) return tu_fail(RENI_EINVAL, who, "K must be in [1, 32]");
  if (N > KN_MAX_POINTS || M > KN_MAX_POINTS) return tu_fail(RENI_EINVAL, who, "too large: need N, M <= 2^31 - 1025");
  if (!y || !idx || !normals || !eigenvalues) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (viewpoint && N > M) return tu_fail(RENI_EINVAL, who, "with a viewpoint row i is point y_i: need N <= M");
  reni::CnArgs a;
  a.y = y; a.idx = idx; a.view = viewpoint;
  a.N = (int)N; a.M = (int)M; a.K = (int)K;
  a.normals = normals; a.eig = eigenvalues;
  return tu_launch(TU_COUNTED, reni::k_cn_normals, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

}  // extern "C"
