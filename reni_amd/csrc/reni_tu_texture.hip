// translation unit of libreni_hip.so: UV-space textures for the environment-map shader's materials -- the pixel's UV and
// footprint from the G-buffer, the mip pyramid, the trilinear fetch and the transposes of both (reni_amd/textures.py).
//
// No reference counterpart (the reference shades with scalar materials); the definitions are include/reni_hip.h's ("UV-space
// textures") and DESIGN 4.4k's.  fp32 throughout, no float atomics: every sum runs in an order that depends on the sizes and on
// the tap table only, so two calls give identical bits.
//
//   k_pixel_uv          one lane per pixel: uv = fmaf(b2, t2, fmaf(b1, t1, b0 t0)) from the rasteriser's own barycentrics, and the
//                       face's constant d(uv) / d(col, row) from its NDC vertices (reni_mesh.inc: mesh_project, mesh_bary_area).
//   k_texture_taps      one lane per pixel: lambda from the footprint, then the 8 (element index, weight) pairs of the fetch.
//   k_pyramid_down      one lane per texel of level l + 1: ((a00 + a01) + (a10 + a11)) / 4; where level l is one texel wide or high,
//                       (a0 + a1) / 2.  One launch per level, in place in the [E][C] buffer.
//   k_pyramid_up        the transpose, one lane per texel of level l: g_l[y][x] += r g_{l+1}[y >> 1][x >> 1], r = 1/4 or 1/2 as
//                       above; launched for l = L - 2 .. 0.  A gather: a fine texel has exactly one parent.
//   k_texture_fetch<C>  one lane per pixel, all C channels: out = fmaf chain over the taps k = 0 .. 7; the pixel's taps are read once.
//   k_texture_fetch_bwd<C>  one lane per texel e, all C channels, over its range of the sorted tap table.  A range of at most
//                       TX_SHORT entries is walked by its lane, ascending.  A longer one is cut into chunks of 64 consecutive
//                       entries, and the 64 lanes of the texel's wave sum them together: lane j adds entry j of chunk 0, 1, 2, ... in
//                       chunk order (so the wave reads a chunk's 64 order entries in one go), and the 64 lane sums are then combined by
//                       the xor butterfly 32, 16, 8, 4, 2, 1.  Which form a range takes and where it is cut depend on `offsets` only.
//                       The one texel of a 1 x 1 level costs 8 P / 64 steps, not 8 P.  plain != 0: every range is walked by its
//                       lane (the form the chunked one is measured against, profiles/tools/texture_time.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"
#include "reni_mesh.inc"

namespace reni {

constexpr int TX_SHORT = 128;    // the longest tap range one lane walks alone
constexpr int TX_MAX_LEVELS = 31;

struct PuvArgs {
  const float* verts;      // [V][3]
  const int64_t* faces;    // [F][3]
  const float* vuv;        // [Tn][2]
  const int64_t* fuv;      // [F][3]
  const int64_t* p2f;      // [P]
  const float* bary;       // [P][3]
  float* uv;               // [P][2]
  float* jac;              // [P][4]
  int64_t* valid;          // [P] or NULL: the pixel's face, -1 where the pixel is invalid
  Camera cam;
  int V, F, Tn, P;
  float step;  // d NDC / d pixel = -2 / S (NDC +x points left and +y up: both decrease with the column / row)
};

__global__ void __launch_bounds__(256) k_pixel_uv(const PuvArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= a.P) return;
  const int64_t f = a.p2f[p];
  float u = 0.f, v = 0.f, j0 = 0.f, j1 = 0.f, j2 = 0.f, j3 = 0.f;
  bool ok = f >= 0 && f < a.F;
  int64_t vi[3] = {0, 0, 0}, ti[3] = {0, 0, 0};
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      vi[k] = a.faces[3 * f + k];
      ti[k] = a.fuv[3 * f + k];
      ok = ok && vi[k] >= 0 && vi[k] < a.V && ti[k] >= 0 && ti[k] < a.Tn;
    }
  }
  if (ok) {
    float x[3], y[3], tu[3], tv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float z;
      mesh_project(a.cam, a.verts[3 * vi[k]], a.verts[3 * vi[k] + 1], a.verts[3 * vi[k] + 2], x[k], y[k], z);
      tu[k] = a.vuv[2 * ti[k]];
      tv[k] = a.vuv[2 * ti[k] + 1];
    }
    const float b0 = a.bary[3 * (size_t)p], b1 = a.bary[3 * (size_t)p + 1], b2 = a.bary[3 * (size_t)p + 2];
    u = fmaf(b2, tu[2], fmaf(b1, tu[1], b0 * tu[0]));
    v = fmaf(b2, tv[2], fmaf(b1, tv[1], b0 * tv[0]));
    // w0 = edge(p, v1, v2) / A, w1 = edge(p, v2, v0) / A, w2 = edge(p, v0, v1) / A with edge(p, a, b) = (px - ax)(by - ay) - (py - ay)(bx - ax):
    // d w / d px = (by - ay) / A, d w / d py = -(bx - ax) / A
    const float A = mesh_bary_area(x[0], y[0], x[1], y[1], x[2], y[2]);
    const float sx = a.step / A;
    const float wx0 = y[2] - y[1], wx1 = y[0] - y[2], wx2 = y[1] - y[0];
    const float wy0 = x[1] - x[2], wy1 = x[2] - x[0], wy2 = x[0] - x[1];
    j0 = fmaf(wx2, tu[2], fmaf(wx1, tu[1], wx0 * tu[0])) * sx;  // du / dcol
    j1 = fmaf(wx2, tv[2], fmaf(wx1, tv[1], wx0 * tv[0])) * sx;  // dv / dcol
    j2 = fmaf(wy2, tu[2], fmaf(wy1, tu[1], wy0 * tu[0])) * sx;  // du / drow
    j3 = fmaf(wy2, tv[2], fmaf(wy1, tv[1], wy0 * tv[0])) * sx;  // dv / drow
    if (!(isfinite(u) && isfinite(v))) {
      ok = false;
      u = v = j0 = j1 = j2 = j3 = 0.f;
    }
  }
  a.uv[2 * (size_t)p] = u;
  a.uv[2 * (size_t)p + 1] = v;
  float* q = a.jac + 4 * (size_t)p;
  q[0] = j0; q[1] = j1; q[2] = j2; q[3] = j3;
  if (a.valid) a.valid[p] = ok ? f : -1;
}

struct TapArgs {
  const float* uv;       // [P][2]
  const float* jac;      // [P][4] or NULL
  const int64_t* valid;  // [P] or NULL: < 0 marks an invalid pixel
  int32_t* idx;          // [P][8]
  float* wgt;            // [P][8]
  int P, L, H0, W0, repeat, align;
  float bias;
};

// one axis of the bilinear tap: texels i0, i1 and the fraction towards i1
DEV void tx_axis(float t, int n, int n0, int repeat, int align, bool flip, int& i0, int& i1, float& fr) {
  float x;
  if (align) {  // L = 1, clamp: x = clamp(t, 0, 1) (n0 - 1)
    const float c = fminf(fmaxf(t, 0.f), 1.f);
    x = (flip ? 1.f - c : c) * (float)(n0 - 1);
  } else if (repeat) {
    const float r = t - floorf(t);
    x = fmaf(flip ? 1.f - r : r, (float)n, -0.5f);
  } else {
    x = fminf(fmaxf(fmaf(flip ? 1.f - t : t, (float)n, -0.5f), 0.f), (float)(n - 1));
  }
  const float x0 = floorf(x);
  fr = x - x0;
  int k = (int)x0;
  if (repeat) {  // x0 in [-1, n - 1]
    i0 = k < 0 ? k + n : (k >= n ? k - n : k);
    i1 = k + 1 >= n ? k + 1 - n : k + 1;
  } else {
    k = min(max(k, 0), n - 1);
    i0 = k;
    i1 = min(k + 1, n - 1);
  }
}

__global__ void __launch_bounds__(256) k_texture_taps(const TapArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= a.P) return;
  int32_t* ip = a.idx + 8 * (size_t)p;
  float* wp = a.wgt + 8 * (size_t)p;
  const float u = a.uv[2 * (size_t)p], v = a.uv[2 * (size_t)p + 1];
  if ((a.valid && a.valid[p] < 0) || !(isfinite(u) && isfinite(v))) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { ip[k] = 0; wp[k] = 0.f; }
    return;
  }
  float lam = a.bias;
  if (a.jac) {
    const float* j = a.jac + 4 * (size_t)p;
    const float a0 = j[0] * (float)a.W0, a1 = j[1] * (float)a.H0, a2 = j[2] * (float)a.W0, a3 = j[3] * (float)a.H0;
    const float rho = fmaxf(hypotf(a0, a1), hypotf(a2, a3));  // (hypotf: no overflow or underflow of the squares)
    lam = (isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(a3) && isfinite(rho) && rho > 0.f) ? log2f(rho) + a.bias : 0.f;
  }
  lam = fminf(fmaxf(lam, 0.f), (float)(a.L - 1));
  int l0 = (int)floorf(lam);
  float fl = lam - (float)l0;
  if (l0 >= a.L - 1) { l0 = a.L - 1; fl = 0.f; }
  const int l1 = fl > 0.f ? l0 + 1 : l0;
  int off0 = 0;
  for (int l = 0; l < l0; ++l) off0 += max(1, a.H0 >> l) * max(1, a.W0 >> l);
  const int H_0 = max(1, a.H0 >> l0), W_0 = max(1, a.W0 >> l0);
  const int off1 = l1 > l0 ? off0 + H_0 * W_0 : off0;
  const int H_1 = max(1, a.H0 >> l1), W_1 = max(1, a.W0 >> l1);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int Hl = s ? H_1 : H_0, Wl = s ? W_1 : W_0, off = s ? off1 : off0;
    const float lw = s ? fl : 1.f - fl;
    int x0, x1, y0, y1;
    float fx, fy;
    tx_axis(u, Wl, a.W0, a.repeat, a.align, false, x0, x1, fx);
    tx_axis(v, Hl, a.H0, a.repeat, a.align, true, y0, y1, fy);
    const float gx = 1.f - fx, gy = 1.f - fy;
    ip[4 * s + 0] = off + y0 * Wl + x0; wp[4 * s + 0] = (gy * gx) * lw;
    ip[4 * s + 1] = off + y0 * Wl + x1; wp[4 * s + 1] = (gy * fx) * lw;
    ip[4 * s + 2] = off + y1 * Wl + x0; wp[4 * s + 2] = (fy * gx) * lw;
    ip[4 * s + 3] = off + y1 * Wl + x1; wp[4 * s + 3] = (fy * fx) * lw;
  }
}

// level l + 1 (Hn x Wn at element `dst`) from level l (H x W at element `src`) of tex [E][C]
__global__ void __launch_bounds__(256) k_pyramid_down(float* __restrict__ tex, int C, int64_t src, int H, int W, int64_t dst,
                                                      int Hn, int Wn) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= Hn * Wn) return;
  const int y = t / Wn, x = t - y * Wn;
  const int ya = H > 1 ? 2 * y : 0, yb = H > 1 ? 2 * y + 1 : 0, xa = W > 1 ? 2 * x : 0, xb = W > 1 ? 2 * x + 1 : 0;
  const float* r0 = tex + (src + (int64_t)ya * W) * C;
  const float* r1 = tex + (src + (int64_t)yb * W) * C;
  float* q = tex + (dst + t) * C;
  for (int c = 0; c < C; ++c) {
    const float a00 = r0[xa * C + c], a01 = r0[xb * C + c], a10 = r1[xa * C + c], a11 = r1[xb * C + c];
    if (H > 1 && W > 1) q[c] = ((a00 + a01) + (a10 + a11)) * 0.25f;
    else q[c] = (W > 1 ? a00 + a01 : a00 + a10) * 0.5f;
  }
}

// g of level l (H x W at `dst`) += r g of level l + 1 (Wn wide at `src`)
__global__ void __launch_bounds__(256) k_pyramid_up(float* __restrict__ g, int C, int64_t dst, int H, int W, int64_t src, int Wn) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= H * W) return;
  const int y = t / W, x = t - y * W;
  const int yp = H > 1 ? y >> 1 : 0, xp = W > 1 ? x >> 1 : 0;
  const float r = H > 1 && W > 1 ? 0.25f : 0.5f;
  const float* parent = g + (src + (int64_t)yp * Wn + xp) * C;
  float* q = g + (dst + t) * C;
  for (int c = 0; c < C; ++c) q[c] = fmaf(r, parent[c], q[c]);
}

template <int C>
__global__ void __launch_bounds__(256) k_texture_fetch(const float* __restrict__ tex, const int32_t* __restrict__ idx,
                                                       const float* __restrict__ wgt, int P, int E, float* __restrict__ out) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= P) return;
  const int4 i0 = *(const int4*)(idx + 8 * (size_t)p), i1 = *(const int4*)(idx + 8 * (size_t)p + 4);
  const float4 w0 = *(const float4*)(wgt + 8 * (size_t)p), w1 = *(const float4*)(wgt + 8 * (size_t)p + 4);
  const int ii[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
  const float ww[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (ww[k] == 0.f) continue;  // an unused tap reads nothing (a NaN texel behind a zero weight stays out)
    const float* t = tex + (size_t)min(max(ii[k], 0), E - 1) * C;  // (a table is trusted for weights, never for addresses)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(ww[k], t[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[(size_t)p * C + c] = acc[c];
}

template <int C>
DEV void tx_add_tap(const float* __restrict__ g, const float* __restrict__ wgt, int64_t tap, int64_t taps, float (&acc)[C]) {
  if ((uint64_t)tap >= (uint64_t)taps) return;  // a malformed order entry adds nothing
  const float wv = wgt[tap];
  if (wv == 0.f) return;
  const float* gp = g + (tap >> 3) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = fmaf(wv, gp[c], acc[c]);
}

template <int C>
__global__ void __launch_bounds__(256) k_texture_fetch_bwd(const float* __restrict__ g, const float* __restrict__ wgt,
                                                           const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                           int64_t E, int64_t P, int plain, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t taps = 8 * P;
  int64_t k0 = 0, k1 = 0;
  if (e < E) {
    k0 = min(max(offsets[e], (int64_t)0), taps);  // (a table that is not what ops builds must not become an address)
    k1 = min(max(offsets[e + 1], k0), taps);
  }
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  const bool lng = !plain && k1 - k0 > TX_SHORT;
  if (!lng)
    for (int64_t k = k0; k < k1; ++k) tx_add_tap<C>(g, wgt, order[k], taps, acc);
  unsigned long long todo = __ballot(lng);
  while (todo) {  // wave-uniform: the long ranges of this wave's 64 texels, in lane order
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t b = __shfl(k0, owner), n = __shfl(k1, owner) - b;
    float part[C];
#pragma unroll
    for (int c = 0; c < C; ++c) part[c] = 0.f;
    for (int64_t k = lane; k < n; k += 64) tx_add_tap<C>(g, wgt, order[b + k], taps, part);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float s = part[c];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
      if (lane == owner) acc[c] = s;
    }
  }
  if (e >= E) return;
#pragma unroll
  for (int c = 0; c < C; ++c) out[e * C + c] = acc[c];
}

}  // namespace reni

namespace {

using reni::reni_set_error;
constexpr int64_t TX_MAX_PIXELS = 0x0fffffff;  // 8 P fits an int32 with room to spare
constexpr int64_t TX_MAX_ELEMS = 0x7fffffff;   // E < 2^31

bool tx_pow2(int64_t x) { return x >= 1 && !(x & (x - 1)); }

// RENI_OK with E = sum of the level sizes, or the error set
int tx_check_pyramid(const char* who, int64_t L, int64_t H0, int64_t W0, int64_t* E) {
  if (L < 1 || H0 < 1 || W0 < 1) return tu_fail(RENI_EINVAL, who, "L, H0 and W0 must be >= 1");
  if (H0 > TX_MAX_ELEMS || W0 > TX_MAX_ELEMS || H0 > TX_MAX_ELEMS / W0) return tu_fail(RENI_EINVAL, who, "too large: need E < 2^31");
  if (L > 1 && !(tx_pow2(H0) && tx_pow2(W0))) return tu_fail(RENI_EINVAL, who, "L > 1 needs H0 and W0 to be powers of two");
  int64_t full = 1;
  for (int64_t m = H0 > W0 ? H0 : W0; m > 1; m >>= 1) ++full;
  if (L > full) return tu_fail(RENI_EINVAL, who, "L must be <= 1 + log2(max(H0, W0))");
  int64_t total = 0;
  for (int64_t l = 0; l < L; ++l) total += ((H0 >> l) > 1 ? (H0 >> l) : 1) * ((W0 >> l) > 1 ? (W0 >> l) : 1);
  if (total > TX_MAX_ELEMS) return tu_fail(RENI_EINVAL, who, "too large: need E < 2^31");
  *E = total;
  return RENI_OK;
}

int tx_check_fetch(const char* who, int64_t P, int64_t E, int64_t C) {
  if (P < 1 || E < 1 || C < 1) return tu_fail(RENI_EINVAL, who, "P, E and C must be >= 1");
  if (C > 8) return tu_fail(RENI_EINVAL, who, "C must be <= 8");
  if (P > TX_MAX_PIXELS || E > TX_MAX_ELEMS) return tu_fail(RENI_EINVAL, who, "too large: need P < 2^28 and E < 2^31");
  return RENI_OK;
}

template <int C>
int tx_fetch_launch(bool forward, int64_t P, int64_t E, const float* src, const int32_t* idx, const float* wgt, const int64_t* order,
                    const int64_t* offsets, int plain, float* out, hipStream_t s) {
  if (forward)
    return tu_launch(TU_PLAIN, reni::k_texture_fetch<C>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, src, idx, wgt, (int)P, (int)E,
                     out);
  return tu_launch(TU_PLAIN, reni::k_texture_fetch_bwd<C>, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, src, wgt, order, offsets, E,
                   P, plain, out);
}

int tx_fetch_dispatch(bool forward, int64_t P, int64_t E, int64_t C, const float* src, const int32_t* idx, const float* wgt,
                      const int64_t* order, const int64_t* offsets, int plain, float* out, hipStream_t s) {
  switch (C) {
    case 1: return tx_fetch_launch<1>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 2: return tx_fetch_launch<2>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 3: return tx_fetch_launch<3>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 4: return tx_fetch_launch<4>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 5: return tx_fetch_launch<5>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 6: return tx_fetch_launch<6>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    case 7: return tx_fetch_launch<7>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
    default: return tx_fetch_launch<8>(forward, P, E, src, idx, wgt, order, offsets, plain, out, s);
  }
}

int tx_pyramid(bool down, int64_t L, int64_t H0, int64_t W0, int64_t C, float* tex, void* stream) {
  const char* who = down ? "texture pyramid" : "texture pyramid backward";
  int64_t E = 0;
  if (int rc = tx_check_pyramid(who, L, H0, W0, &E)) return rc;
  if (C < 1 || C > 8) return tu_fail(RENI_EINVAL, who, "C must be 1..8");
  if (!tex) return tu_fail(RENI_EINVAL, who, "NULL argument");
  int64_t off[reni::TX_MAX_LEVELS + 1];
  int h[reni::TX_MAX_LEVELS + 1], w[reni::TX_MAX_LEVELS + 1];
  off[0] = 0;
  for (int64_t l = 0; l < L; ++l) {
    h[l] = (int)((H0 >> l) > 1 ? (H0 >> l) : 1);
    w[l] = (int)((W0 >> l) > 1 ? (W0 >> l) : 1);
    off[l + 1] = off[l] + (int64_t)h[l] * w[l];
  }
  hipStream_t s = (hipStream_t)stream;
  if (down) {
    for (int64_t l = 0; l + 1 < L; ++l)
      if (int rc = tu_launch(TU_PLAIN, reni::k_pyramid_down, dim3((unsigned)(((int64_t)h[l + 1] * w[l + 1] + 255) / 256)), dim3(256), 0, s,
                             tex, (int)C, off[l], h[l], w[l], off[l + 1], h[l + 1], w[l + 1]))
        return rc;
  } else {
    for (int64_t l = L - 2; l >= 0; --l)
      if (int rc = tu_launch(TU_PLAIN, reni::k_pyramid_up, dim3((unsigned)(((int64_t)h[l] * w[l] + 255) / 256)), dim3(256), 0, s, tex,
                             (int)C, off[l], h[l], w[l], off[l + 1], w[l + 1]))
        return rc;
  }
  return RENI_OK;
}

}  // namespace

extern "C" {

int reni_mesh_pixel_uv(int64_t V, int64_t F, int64_t Tn, const float* verts, const int64_t* faces, const float* verts_uvs,
                       const int64_t* faces_uvs, const float* R, const float* T, float tan_half_fov, int64_t S,
                       const int64_t* pix_to_face, const float* bary, float* uv, float* jac, int64_t* pix_valid, void* stream) {
  if (V < 1 || F < 1 || Tn < 1 || S < 1) return reni_set_error(RENI_EINVAL, "pixel uv: V, F, Tn and S must be >= 1");
  if (V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS || Tn > MESH_MAX_ELEMS || S * S > TX_MAX_PIXELS)
    return reni_set_error(RENI_EINVAL, "pixel uv: too large: need V, F, Tn < 2^30 and S S < 2^28");
  if (!verts || !faces || !verts_uvs || !faces_uvs || !R || !T || !pix_to_face || !bary || !uv || !jac)
    return reni_set_error(RENI_EINVAL, "pixel uv: NULL argument");
  if (int rc = mesh_check_fov("pixel uv", tan_half_fov)) return rc;
  reni::PuvArgs a = {};
  a.verts = verts; a.faces = faces; a.vuv = verts_uvs; a.fuv = faces_uvs; a.p2f = pix_to_face; a.bary = bary;
  a.uv = uv; a.jac = jac; a.valid = pix_valid;
  a.cam = mesh_camera(R, T, tan_half_fov);
  a.V = (int)V; a.F = (int)F; a.Tn = (int)Tn; a.P = (int)(S * S);
  a.step = -2.f / (float)S;
  return tu_launch(TU_PLAIN, reni::k_pixel_uv, dim3((unsigned)((S * S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

int reni_texture_taps(int64_t P, const float* uv, const float* jac, const int64_t* pix_valid, int64_t L, int64_t H0, int64_t W0,
                      float lod_bias, int32_t wrap, int32_t align_corners, int32_t* tap_index, float* tap_weight, void* stream) {
  if (P < 1) return reni_set_error(RENI_EINVAL, "texture taps: P must be >= 1");
  if (P > TX_MAX_PIXELS) return reni_set_error(RENI_EINVAL, "texture taps: too large: need P < 2^28");
  int64_t E = 0;
  if (int rc = tx_check_pyramid("texture taps", L, H0, W0, &E)) return rc;
  if (wrap != RENI_TEX_CLAMP && wrap != RENI_TEX_REPEAT) return reni_set_error(RENI_EINVAL, "texture taps: wrap must be RENI_TEX_CLAMP or RENI_TEX_REPEAT");
  if (align_corners != 0 && align_corners != 1) return reni_set_error(RENI_EINVAL, "texture taps: align_corners must be 0 or 1");
  if (align_corners && (L > 1 || wrap != RENI_TEX_CLAMP))
    return reni_set_error(RENI_EINVAL, "texture taps: align_corners needs L = 1 and RENI_TEX_CLAMP");
  if (!isfinite(lod_bias)) return reni_set_error(RENI_EINVAL, "texture taps: lod_bias must be finite");
  if (!uv || !tap_index || !tap_weight) return reni_set_error(RENI_EINVAL, "texture taps: NULL argument");
  if (((uintptr_t)tap_index | (uintptr_t)tap_weight) & 15)
    return reni_set_error(RENI_EINVAL, "texture taps: tap_index and tap_weight must be 16-byte aligned");
  reni::TapArgs a = {};
  a.uv = uv; a.jac = jac; a.valid = pix_valid; a.idx = tap_index; a.wgt = tap_weight;
  a.P = (int)P; a.L = (int)L; a.H0 = (int)H0; a.W0 = (int)W0; a.repeat = wrap == RENI_TEX_REPEAT; a.align = align_corners;
  a.bias = lod_bias;
  return tu_launch(TU_PLAIN, reni::k_texture_taps, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

int reni_texture_pyramid(int64_t L, int64_t H0, int64_t W0, int64_t C, float* tex, void* stream) {
  return tx_pyramid(true, L, H0, W0, C, tex, stream);
}

int reni_texture_pyramid_backward(int64_t L, int64_t H0, int64_t W0, int64_t C, float* grad_tex, void* stream) {
  return tx_pyramid(false, L, H0, W0, C, grad_tex, stream);
}

int reni_texture_fetch(int64_t P, int64_t E, int64_t C, const float* tex, const int32_t* tap_index, const float* tap_weight,
                       float* out, void* stream) {
  if (int rc = tx_check_fetch("texture fetch", P, E, C)) return rc;
  if (!tex || !tap_index || !tap_weight || !out) return reni_set_error(RENI_EINVAL, "texture fetch: NULL argument");
  if (((uintptr_t)tap_index | (uintptr_t)tap_weight) & 15)
    return reni_set_error(RENI_EINVAL, "texture fetch: tap_index and tap_weight must be 16-byte aligned");
  return tx_fetch_dispatch(true, P, E, C, tex, tap_index, tap_weight, nullptr, nullptr, 0, out, (hipStream_t)stream);
}

int reni_texture_fetch_backward(int64_t P, int64_t E, int64_t C, const float* grad_out, const float* tap_weight,
                                const int64_t* tap_order, const int64_t* offsets, int32_t plain, float* grad_tex, void* stream) {
  if (int rc = tx_check_fetch("texture fetch backward", P, E, C)) return rc;
  if (!grad_out || !grad_tex) return reni_set_error(RENI_EINVAL, "texture fetch backward: NULL argument");
  if (!tap_weight || !tap_order || !offsets) return reni_set_error(RENI_EINVAL, "texture fetch backward: NULL tap weights, order or offsets");
  if (plain != 0 && plain != 1) return reni_set_error(RENI_EINVAL, "texture fetch backward: plain must be 0 or 1");
  return tx_fetch_dispatch(false, P, E, C, grad_out, nullptr, tap_weight, tap_order, offsets, plain, grad_tex, (hipStream_t)stream);
}

}  // extern "C"
