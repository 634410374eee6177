// translation unit of libreni_hip.so: the transposes of glossy lighting's two linear operators (reni_tu_glossy.hip) -- what
// d loss / d map needs behind a prefiltered render (reni_amd/glossy.py's autograd functions).
//
// fp32 throughout, no float atomics: every sum runs in a fixed order, so two calls give identical bits and a map's gradient
// does not depend on the batch around it.  Contraction is off for the whole unit: what is written is what runs.
//
//   k_lobe_recip        r[l][o] = normalise ? (den[l][o] > 0 ? 1 / den[l][o] : 0) : scale -- what the forward multiplied
//                       num[.][l][o][.] by, once per (lobe, o).
//   k_lobe_convolve_t<KIND, CT>  part[s][col][i] = sum_(l of KIND) sum_(o in chunk s) f_l(o . d_i) r[l][o] g[o][col of lobe l]:
//                       k_lobe_convolve with the roles swapped.  Rows are the Q texels (the same 32-row tiles, DG_OT a
//                       wave, 4 waves), the reduction runs over o, two a step with lanes 32..63 feeding k = 1, and t is
//                       built in the order of the forwards' k-step (dg_kstep of reni_sphere.inc: ox dx, then two fma; here
//                       a copy with the roles exchanged), so both directions use one kernel matrix up to the lobe's rounding.  r sits where the forward has w_i, a per-k scalar.  The lobes of a
//                       kind are looped INSIDE the workgroup into the same accumulators; the o range is split by the
//                       forward's rule with P and Q exchanged.
//   k_lobe_finish_t     dsrc(n, i, c) = w_i ((slab_0 + slab_1) + ...) of column 3 n + c over the (kind, split) slabs in that
//                       order, written through element strides: every element is written.
//   k_envmap_lookup_taps  per direction the 8 texels k_envmap_lookup reads (4 on floor(level), 4 on the next level) as
//                       element indices level H W + y W + x, and their effective weights {gr gc, gr fc, fr gc, fr fc} x
//                       {gl, fl}; the second level weighs 0 unless fl > 0, as the forward reads it only then.  (row, col),
//                       the four taps and the level come from the functions k_envmap_lookup calls (sph_rowcol, sph_taps,
//                       sph_level).
//   k_envmap_lookup_bwd one lane per (map, element): the sum of weight x upstream over the element's taps, in the order a
//                       stable sort of the indices left them -- the scatter as a gather (as reni_mesh_vertex_normals does
//                       with the faces of a vertex).  A texel sampled by very many directions is summed by ONE lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#include "reni_sphere.inc"  // GEMM pieces, lobes, split rule, (row, col), taps, level, query: shared with reni_tu_glossy.hip

namespace reni {

struct LbtArgs {
  int P, Q;
  int ncol;               // 3 N
  const float* out_dirs;  // [P][3]
  const float* in_dirs;   // [Q][3]
  const float* g;         // upstream [N][Lv][P][3]: element (o, col = 3 n + c) of lobe l at ((n Lv + l) P + o) 3 + c
  const float* r;         // [Lv][P]
  int chunk;  // o per split (even)
  int S;      // splits
  int Lv;     // lobes of the call
  int nl;     // lobes of this launch (one kind)
  int lobe[LB_MAX_LOBES];   // their index in the call
  float par[LB_MAX_LOBES];  // PHONG: n; BLINN: s / 2; GGX: alpha^2
  float* ws;                // this kind's slabs [S][ncol][Q]
};

__global__ void __launch_bounds__(256) k_lobe_recip(const float* __restrict__ den, int64_t total, float scale,
                                                    float* __restrict__ r) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float v = scale;
  if (den) {  // (the largest finite number where 1 / den overflows: 0 f stays 0)
    const float d = den[e];
    v = d > 0.f ? fminf(1.f / d, 3.4028234664e38f) : 0.f;
  }
  r[e] = v;
}

template <int KIND, int CT>
__global__ void __launch_bounds__(256) k_lobe_convolve_t(const LbtArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, hi = lane >> 5;
  const int sp = (int)blockIdx.z;  // split
  const int64_t i0 = (int64_t)blockIdx.x * DG_ROWS + wave * (32 * DG_OT);
  float dx[DG_OT], dy[DG_OT], dz[DG_OT];
#pragma unroll
  for (int u = 0; u < DG_OT; ++u) {
    const int64_t i = i0 + u * 32 + j;
    const bool ok = i < a.Q;
    dx[u] = ok ? a.in_dirs[3 * i] : 0.f;
    dy[u] = ok ? a.in_dirs[3 * i + 1] : 0.f;
    dz[u] = ok ? a.in_dirs[3 * i + 2] : 0.f;
  }
  const float* colp[CT];  // column (n, c) of lobe 0 at o = olo + hi
  bool cok[CT];
  const int olo = sp * a.chunk;
  const int ohi = olo + a.chunk < a.P ? olo + a.chunk : a.P;
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    cok[v] = col < a.ncol;
    const int64_t n = cok[v] ? col / 3 : 0;  // (every lane loads: column 0 beyond the last column, the value dropped)
    const int64_t c = cok[v] ? col - 3 * n : 0;
    colp[v] = a.g + (n * a.Lv * a.P + olo + hi) * 3 + c;
  }
  mfma_f32x16 acc[DG_OT][CT];
#pragma unroll
  for (int u = 0; u < DG_OT; ++u)
#pragma unroll
    for (int v = 0; v < CT; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;
  int ll = 0;
  do {  // (nl >= 1: a loop that may run zero times makes hipcc merge the accumulators with their zeros ahead of the drain pad)
    const float par = a.par[ll];
    const int64_t lo = (int64_t)a.lobe[ll] * a.P;
    // o = o0 + hi: lanes 0..31 feed k = 0 of the MFMA, lanes 32..63 k = 1
    const float* dp = a.out_dirs + 3 * (int64_t)(olo + hi);
    const float* rp = a.r + lo + olo + hi;
    const float* bp[CT];
#pragma unroll
    for (int v = 0; v < CT; ++v) bp[v] = colp[v] + 3 * lo;
    // one k-step; ook false zeroes both operands of the lanes of o == ohi (the tail of an odd range)
    auto step = [&](const bool ook) __attribute__((always_inline)) {
      const float ox = dp[0], oy = dp[1], oz = dp[2];
      const float rv = ook ? rp[0] : 0.f;
      float b[CT];
#pragma unroll
      for (int v = 0; v < CT; ++v) {
        const float x = *bp[v];
        b[v] = ook && cok[v] ? x : 0.f;
      }
      // (dg_kstep of reni_sphere.inc with rows and k-side exchanged, as a copy: the shared call moved eight lines of the listing
      // and was not at or below the previous library's times in every row, profiles/sphere_body_refactor.md)
#pragma unroll
      for (int u = 0; u < DG_OT; ++u) {
        float t = ox * dx[u];
        t = fmaf(oy, dy[u], t);
        t = fmaf(oz, dz[u], t);
        const float av = lb_lobe<KIND>(t, par) * rv;
#pragma unroll
        for (int v = 0; v < CT; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[v], acc[u][v], 0, 0, 0);
      }
    };
    int o0 = olo;
    for (; o0 + 1 < ohi; o0 += 2) {
      step(true);
      dp += 6;
      rp += 2;
#pragma unroll
      for (int v = 0; v < CT; ++v) bp[v] += 6;
    }
    if (o0 < ohi) {  // odd range: the lanes of o0 + 1 re-read o0 and contribute zero
      dp -= 3 * hi;
      rp -= hi;
#pragma unroll
      for (int v = 0; v < CT; ++v) bp[v] -= 3 * hi;
      step(hi == 0);
    }
  } while (++ll < a.nl);
  mfma_drain_tied(acc);
  float* dst = a.ws + (int64_t)sp * a.ncol * a.Q;
#pragma unroll
  for (int v = 0; v < CT; ++v) {
    if (!cok[v]) continue;
    const int64_t col = (int64_t)blockIdx.y * (32 * CT) + v * 32 + j;
    float* op = dst + col * a.Q;
#pragma unroll
    for (int u = 0; u < DG_OT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t i = i0 + u * 32 + mfma_rowmap(r, hi);
        if (i < a.Q) op[i] = acc[u][v][r];
      }
  }
}

// one lane per (map, i): the slabs of its three columns in (kind, split) order, then the texel's weight
__global__ void __launch_bounds__(256) k_lobe_finish_t(const float* __restrict__ ws, const float* __restrict__ in_w, int N, int Q,
                                                       int slabs, float* __restrict__ dsrc, int64_t sn, int64_t si, int64_t sc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * Q) return;
  const int64_t i = e % Q, n = e / Q;
  const int64_t slab = 3 * (int64_t)N * Q;
  const float w = in_w[i];
  float* q = dsrc + n * sn + i * si;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = ws + (3 * n + c) * Q + i;
    float x = p[0];
    for (int s = 1; s < slabs; ++s) x += p[(int64_t)s * slab];
    q[c * sc] = w * x;
  }
}

struct LtArgs : SphQuery {  // (no source: the maps of the query are its T tables)
  int32_t* idx;  // [T][P][8]
  float* wgt;    // [T][P][8]
};

__global__ void __launch_bounds__(256) k_envmap_lookup_taps(const LtArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;  // P < 2^28
  if (p >= a.P) return;
  const int64_t n = blockIdx.y;
  const float* d = a.dirs + n * a.dn + 3 * (int64_t)p;
  const float sx = d[0], sy = d[1], sz = d[2];
  float row, col;
  sph_rowcol(sx, sy, sz, a.H, a.W, a.row_scale, a.col_scale, a.col_bias, row, col);
  const SphTaps t = sph_taps(row, col, a.H, a.W);
  const int r0 = t.i0 * a.W, r1 = t.i1 * a.W;
  const int e4[4] = {r0 + t.j00, r0 + t.j01, r1 + t.j10, r1 + t.j11};
  const float w4[4] = {t.gr * t.gc, t.gr * t.fc, t.fr * t.gc, t.fr * t.fc};
  // ---- the level, as the forward: the next level is read, and so weighs, only when fl > 0
  const SphLevel L = sph_level(a.level ? a.level[n * a.ln + p] : a.level_const, a.Lv);
  const int l0 = L.l0, l1 = L.l1;
  const float fl = L.fl, gl = L.gl;
  const bool two = fl > 0.f;
  const int hw = a.H * a.W;
  int32_t* ip = a.idx + (n * a.P + p) * 8;
  float* wp = a.wgt + (n * a.P + p) * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ip[k] = l0 * hw + e4[k];
    wp[k] = two ? w4[k] * gl : w4[k];
    ip[4 + k] = l1 * hw + e4[k];
    wp[4 + k] = two ? w4[k] * fl : 0.f;
  }
}

// T == 1: one table serves every map
__global__ void __launch_bounds__(256) k_envmap_lookup_bwd(const float* __restrict__ g, const float* __restrict__ wgt,
                                                           const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                           int64_t E, int64_t P, int T, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int64_t n = blockIdx.y, t = T == 1 ? 0 : n, taps = 8 * P;
  const int64_t* off = offsets + t * (E + 1) + e;
  int64_t k0 = off[0], k1 = off[1];
  k0 = k0 < 0 ? 0 : k0;  // (a table that is not what ops builds must not become an address)
  k1 = k1 > taps ? taps : k1;
  const int64_t* ord = order + t * taps;
  const float* w = wgt + t * taps;
  const float* gn = g + n * P * 3;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t tap = ord[k];
    if ((uint64_t)tap >= (uint64_t)taps) continue;
    const float wv = w[tap];
    if (wv == 0.f) continue;
    const float* gp = gn + (tap >> 3) * 3;
    s0 += wv * gp[0];
    s1 += wv * gp[1];
    s2 += wv * gp[2];
  }
  float* q = out + (n * E + e) * 3;
  q[0] = s0;
  q[1] = s1;
  q[2] = s2;
}

}  // namespace reni

namespace {

using reni::reni_set_error;

size_t lbt_align(size_t x) { return (x + 255) & ~(size_t)255; }

// r [Lv][P] (rounded up to 256 bytes), then 3 kinds x S slabs [3 N][Q]
size_t lbt_ws_bytes(int64_t N, int64_t P, int64_t Q, int64_t Lv) {
  int64_t S, chunk;
  dg_split(Q, P, S, chunk);
  return lbt_align((size_t)(Lv * P) * sizeof(float)) + (size_t)(3 * S * 3 * N * Q) * sizeof(float);
}

template <int KIND>
int lbt_launch(TuCount count, const reni::LbtArgs& a, hipStream_t s) {
  const unsigned gx = (unsigned)((a.Q + reni::DG_ROWS - 1) / reni::DG_ROWS);
  if (a.ncol <= 32) return tu_launch(count, reni::k_lobe_convolve_t<KIND, 1>, dim3(gx, 1, (unsigned)a.S), dim3(256), 0, s, a);
  return tu_launch(count, reni::k_lobe_convolve_t<KIND, 2>, dim3(gx, (unsigned)((a.ncol + 63) / 64), (unsigned)a.S), dim3(256), 0, s, a);
}

int lk_check_sizes(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, int64_t T) {
  if (N < 1 || Lv < 1 || H < 1 || W < 1 || P < 1) return reni_set_error(RENI_EINVAL, "lookup backward: sizes must be >= 1");
  if (W & 1) return reni_set_error(RENI_EINVAL, "lookup backward: W must be even");
  if (N > 65535 || Lv > 65535 || H > 0x3fffffff / W || Lv > 0x7ffffffe / (H * W) || P > 0x3fffffff / 3 || N > 0x3fffffff / (3 * P))
    return reni_set_error(RENI_EINVAL, "lookup backward: need N, Lv <= 65535, H W < 2^30, Lv H W < 2^31 and N P < 2^28");
  if (T != 1 && T != N) return reni_set_error(RENI_EINVAL, "lookup backward: n_tables must be 1 (shared) or N (per map)");
  return RENI_OK;
}

}  // namespace

extern "C" {

size_t reni_lobe_backward_workspace_bytes(int64_t N, int64_t P, int64_t Q, int64_t n_lobes) {
  if (!lb_shape_ok(N, P, Q, n_lobes)) return 0;
  return lbt_ws_bytes(N, P, Q, n_lobes) + 256;
}

int reni_lobe_convolve_backward(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                                const float* grad_out, int n_lobes, const int32_t* kinds, const float* params, int normalise,
                                float scale, const float* den, float* grad_src, int64_t grad_stride_n, int64_t grad_stride_i,
                                int64_t grad_stride_c, void* ws, size_t ws_bytes, void* stream) {
  if (n_lobes < 1 || n_lobes > reni::LB_MAX_LOBES) return reni_set_error(RENI_EINVAL, "lobe convolve: need 1 <= n_lobes <= 16");
  if (!lb_shape_ok(N, P, Q, n_lobes))
    return reni_set_error(RENI_EINVAL, "lobe convolve backward: need N, P, Q >= 1 and n_lobes N P, Q < 2^28");
  if (!out_dirs || !in_dirs || !in_w || !grad_out || !grad_src || !kinds || !params)
    return reni_set_error(RENI_EINVAL, "lobe convolve backward: NULL argument");
  if (normalise && !den)
    return reni_set_error(RENI_EINVAL, "lobe convolve backward: NULL den (the denominators are required when normalising)");
  if (int rc = lb_check_lobes(n_lobes, kinds, params)) return rc;
  if (grad_stride_n < 0 || grad_stride_i < 0 || grad_stride_c < 0)
    return reni_set_error(RENI_EINVAL, "lobe convolve backward: grad_src strides must be >= 0");
  if (int rc = tu_check_ws("lobe convolve backward", ws, ws_bytes, lbt_ws_bytes(N, P, Q, n_lobes))) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* r = (float*)ws;
  float* slabs = (float*)((char*)ws + lbt_align((size_t)(n_lobes * P) * sizeof(float)));
  const int64_t rtotal = (int64_t)n_lobes * P;
  if (int rc = tu_launch(TU_COUNTED, reni::k_lobe_recip, dim3((unsigned)((rtotal + 255) / 256)), dim3(256), 0, s,
                         normalise ? den : nullptr, rtotal, scale, r))
    return rc;
  reni::LbtArgs a = {};
  a.P = (int)P; a.Q = (int)Q;
  a.ncol = (int)(3 * N);
  a.out_dirs = out_dirs; a.in_dirs = in_dirs;
  a.g = grad_out; a.r = r;
  int64_t S, chunk;
  dg_split(Q, P, S, chunk);
  a.chunk = (int)chunk; a.S = (int)S; a.Lv = n_lobes;
  int nslab = 0;
  // one launch per kind present, its lobes inside, into the kind's own S slabs
  if (int rc = lb_for_kinds(a, n_lobes, kinds, params, [&](int kind, reni::LbtArgs& a) {
        a.ws = slabs + (int64_t)nslab * (3 * N) * Q;
        nslab += (int)S;
        return kind == RENI_LOBE_PHONG   ? lbt_launch<RENI_LOBE_PHONG>(TU_COUNTED, a, s)
               : kind == RENI_LOBE_BLINN ? lbt_launch<RENI_LOBE_BLINN>(TU_COUNTED, a, s)
                                         : lbt_launch<RENI_LOBE_GGX>(TU_COUNTED, a, s);
      }))
    return rc;
  const int64_t total = N * Q;
  return tu_launch(TU_COUNTED, reni::k_lobe_finish_t, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, slabs, in_w, (int)N, (int)Q,
                   nslab, grad_src, grad_stride_n, grad_stride_i, grad_stride_c);
}

int reni_envmap_lookup_taps(int64_t n_tables, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* dirs, int64_t dirs_stride_n,
                            const float* level, int64_t level_stride_n, float level_const, int32_t* tap_index, float* tap_weight,
                            void* stream) {
  if (int rc = lk_check_sizes(n_tables, Lv, H, W, P, n_tables)) return rc;
  if (int rc = sph_check_query(false, n_tables, Lv, H, W, P, nullptr, nullptr, dirs, dirs_stride_n, level, level_stride_n,
                               tap_index && tap_weight))
    return rc;
  reni::LtArgs a = {};
  sph_fill_query(a, n_tables, Lv, H, W, P, nullptr, nullptr, dirs, dirs_stride_n, level, level_stride_n, level_const);
  a.idx = tap_index; a.wgt = tap_weight;
  return tu_launch(TU_COUNTED, reni::k_envmap_lookup_taps, dim3((unsigned)((P + 255) / 256), (unsigned)n_tables), dim3(256), 0,
                   (hipStream_t)stream, a);
}

int reni_envmap_lookup_backward(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* grad_out, int64_t n_tables,
                                const float* tap_weight, const int64_t* tap_order, const int64_t* offsets, float* grad_src,
                                void* stream) {
  if (int rc = lk_check_sizes(N, Lv, H, W, P, n_tables)) return rc;
  if (!grad_out || !grad_src) return reni_set_error(RENI_EINVAL, "lookup backward: NULL argument");
  if (!tap_weight || !tap_order || !offsets) return reni_set_error(RENI_EINVAL, "lookup backward: NULL tap table, order or offsets");
  const int64_t E = Lv * H * W;
  return tu_launch(TU_COUNTED, reni::k_envmap_lookup_bwd, dim3((unsigned)((E + 255) / 256), (unsigned)N), dim3(256), 0,
                   (hipStream_t)stream, grad_out, tap_weight, tap_order, offsets, E, P, (int)n_tables, grad_src);
}

}  // extern "C"
