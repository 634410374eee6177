// translation unit of libreni_hip.so: environment-map Blinn-Phong shading of a G-buffer (FIT_INVERSE task).
//
// Reference: blinn_phong_shading_env_map, src/utils/pytorch3d_envmap_shader.py:46-116 (the part after the two
// interpolate_face_attributes calls; the rasteriser itself is pytorch3d's and out of scope).  With N_p the pixel
// normal, V_p the unit view vector, L_j the direction and C_bj the (sine-weighted) colour of environment-map texel j:
//
//   M(p, j)       = kd * clamp(N_p . L_j, 0, 1) + ks * norm(s) * clamp(N_p . normalize(V_p + L_j), 0, 1) ^ s
//   colors[b,p,:] = sum_j M(p, j) C[b,j,:]                                    (:89-114)
//   dC[b,j,:]     = sum_p M(p, j) dcolors[b,p,:]                              (autograd of the two einsums, :99,:111)
//
// The reference materialises diffuse / half-way / specular tensors of B x H x W x J (x 3) elements; here M is a
// function evaluated in registers.  Forward and backward are the same kernel with the roles of the two axes swapped:
// a thread OWNS one element of one axis (its geometry and 3 * BC accumulators in registers) and walks the other axis,
// whose geometry and source rows are staged through LDS and read by broadcast.  M does not depend on the image when
// the texel directions are shared (the reference repeats one grid, RENI_module.py:376,112), so one evaluation of M
// serves BC images.  The other axis is split over blockIdx.y to fill the chip; partial sums are combined by a second
// kernel in a fixed order (deterministic, no atomics).  VALU-bound: ~25 fp32 operations and three transcendentals per
// (p, j) pair against 6 * BC flops of accumulation -- this is not GEMM-shaped work for the matrix cores.
//
// The unit holds five kernel families.  Three of them -- the terms, the microfacet terms and the microfacet pixel
// gradients -- stand on ONE skeleton: it owns the pixel load, the split bounds, the LDS stages, the mask
// words, the walk and the partial-sum store; a family is its argument struct, what a thread holds for its own element, and
// what one (pixel, texel) pair adds.  The scalar shader and the terms' normal gradient keep a body of their own, because
// their bits moved on the skeleton (see there).  The host half is one plan, one chunk loop and one set of checks for all five.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#define DEV __device__ __forceinline__

namespace reni {

// ---- the skeleton -----------------------------------------------------------------------------------------------------
struct WalkArgs {          // the head of every family's arguments
  const float* nrm;        // [NP][3] interpolated vertex normals (not normalised; 0 where no face covers the pixel)
  const float* pos;        // [NP][3] interpolated surface positions
  const float* ldir;       // [J][3] texel directions of the image chunk's first image
  float cam[3];
  int B, NP, J, b0, nb;    // images b0 .. b0 + nb - 1 are handled by this launch (nb <= BC)
  int per_split;           // elements of the other axis per blockIdx.y
  const uint32_t* vis;     // MASKED: [NP][JW] visibility bits of the chunk's first image (bit j & 31 of word j >> 5)
  int JW;                  // words per pixel, ceil(J / 32)
};

struct Normalize3 {  // F.normalize(p=2, eps=1e-6): v / max(|v|, eps)      (:82,:93,:107)
  DEV static void apply(float (&v)[3]) {
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float inv = 1.f / fmaxf(n, 1e-6f);
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
  }
};

// Normalize3 with its sum of squares written out: which products the compiler fuses there depends on the instance, and the
// WANT_DN instances of k_envmap_ggx_dpixel must agree about N and V to the bit.  The two are NOT interchangeable: each
// family keeps the one its bits were pinned with.
struct Normalize3Fma {
  DEV static void apply(float (&v)[3]) {
    const float n = sqrtf(fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])));
    const float inv = 1.f / fmaxf(n, 1e-6f);
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
  }
};

constexpr int SH_TILE = 128;  // elements of the other axis per LDS stage

// N = normalize(nrm[p]), V = normalize(cam - pos[p])      (:91)
template <class NORM>
DEV void load_pixel(const WalkArgs& a, int p, float (&n)[3], float (&v)[3]) {
  n[0] = a.nrm[(size_t)p * 3]; n[1] = a.nrm[(size_t)p * 3 + 1]; n[2] = a.nrm[(size_t)p * 3 + 2];
  NORM::apply(n);
  v[0] = a.cam[0] - a.pos[(size_t)p * 3]; v[1] = a.cam[1] - a.pos[(size_t)p * 3 + 1]; v[2] = a.cam[2] - a.pos[(size_t)p * 3 + 2];
  NORM::apply(v);
}

// Geometry of the stage's elements t0 .. t0 + SH_TILE - 1: texel (Lx, Ly, Lz, -) in g0, or pixel (Nx, Ny, Nz, Vx) in g0,
// (Vy, Vz, x0, x1) in g1 and x2 in g2, x the family's extras of the pixel (F::NX of them; beyond the range a neutral
// material, never walked).
template <bool OWN_PIXEL, class F>
DEV void stage_geometry(const typename F::Args& a, int t0, int t_end, float4* g0, float4* g1, float* g2) {
  const int tid = threadIdx.x;
  if (tid >= SH_TILE) return;
  const int t = t0 + tid;
  float4 q0 = {0.f, 0.f, 0.f, 0.f};
  if (OWN_PIXEL) {
    if (t < t_end) { q0.x = a.ldir[(size_t)t * 3]; q0.y = a.ldir[(size_t)t * 3 + 1]; q0.z = a.ldir[(size_t)t * 3 + 2]; }
    g0[tid] = q0;
  } else {
    float4 q1 = {0.f, 0.f, 1.f, 0.f};
    float q2 = 1.f;
    if (t < t_end) {
      float n[3], v[3], x[3] = {1.f, 0.f, 1.f};
      load_pixel<typename F::Norm>(a, t, n, v);
      F::extras(a, t, n, v, x);
      q0 = float4{n[0], n[1], n[2], v[0]};
      q1 = float4{v[1], v[2], x[0], x[1]};
      q2 = x[2];
    }
    g0[tid] = q0;
    g1[tid] = q1;
    if (F::NX > 2) g2[tid] = q2;
  }
}

// Source rows of the stage: NSRC = 3 BC floats from each of NSRC / (3 BC) source arrays [B][n_oth][3], zero beyond the range
// and beyond the chunk's images (they then add nothing).
template <int BC, int NSRC>
DEV void stage_rows(const WalkArgs& a, const float* s0, const float* s1, const float* s2, int n_oth, int t0, int t_end, float* svf) {
  constexpr int ROW = 4 * ((NSRC + 3) / 4), NH = NSRC / (3 * BC);
  for (int i = threadIdx.x; i < SH_TILE * NSRC; i += 256) {
    const int e = i / NSRC, r = i - e * NSRC, h = NH == 1 ? 0 : r / (3 * BC), rr = r - h * (3 * BC), b = rr / 3, c = rr - b * 3;
    const int t = t0 + e;
    const float* s = NH == 1 || h == 0 ? s0 : NH == 2 || h == 1 ? s1 : s2;
    float x = 0.f;
    if (t < t_end && b < a.nb) x = s[((size_t)(a.b0 + b) * n_oth + t) * 3 + c];
    svf[e * ROW + r] = x;
  }
}

// Backward, MASKED: the stage's 128 pixels x the workgroup's 8 mask words (its 256 texels)
DEV void stage_mask_words(const WalkArgs& a, int t0, int t_end, uint32_t (*mw)[8]) {
  for (int i = threadIdx.x; i < SH_TILE * 8; i += 256) {
    const int e = i >> 3, w = blockIdx.x * 8 + (i & 7), t = t0 + e;
    mw[e][i & 7] = (t < t_end && w < a.JW) ? a.vis[(size_t)t * a.JW + w] : 0u;
  }
}

// The MASKED walk: pair(e, on) for the stage's cnt elements in ascending e, `on` the pair's visibility bit.  A pair counts only
// where bit (p, j) of a.vis is set (cast shadows, reni_tu_visibility.hip) -- the families make it a select on the pair's
// terms, so the sums keep their order and an all-ones mask gives the unmasked instance's bits.  Forward: the pixel's four
// words of a 128-texel stage are one 16-byte load (four guarded loads when JW is no multiple of 4: the rows are then not
// 16-byte aligned).  Backward: the bit comes from stage_mask_words' block.
template <bool OWN_PIXEL, class PAIR>
DEV void walk_masked(const WalkArgs& a, int o, bool live, int t0, int cnt, const uint32_t (*mw)[8], PAIR pair) {
  const int tid = threadIdx.x;
  uint32_t wv[4] = {0u, 0u, 0u, 0u};
  if (OWN_PIXEL && live) {  // (t0 is a multiple of SH_TILE: per_split is)
    const uint32_t* row = a.vis + (size_t)o * a.JW;
    const int w0 = t0 >> 5;
    if ((a.JW & 3) == 0) {
      const uint4 q = *(const uint4*)(row + w0);
      wv[0] = q.x; wv[1] = q.y; wv[2] = q.z; wv[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) wv[k] = w0 + k < a.JW ? row[w0 + k] : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // the ascending walk of the unmasked instance, 32 elements per mask word
    const int e_end = min(cnt, 32 * k + 32);
    for (int e = 32 * k; e < e_end; ++e)
      pair(e, OWN_PIXEL ? (wv[k] >> (e & 31)) & 1u : (mw[e][tid >> 5] >> (tid & 31)) & 1u);
  }
}

// One output's partial sums of the chunk's images: out[(b0 + b) n_own + o][:] = acc[b][:]
template <int BC>
DEV void store_partial(const WalkArgs& a, const float (&acc)[BC][3], float* out, int n_own, int o) {
#pragma unroll
  for (int b = 0; b < BC; ++b) {
    if (b < a.nb) {
      float* dst = out + ((size_t)(a.b0 + b) * n_own + o) * 3;
      dst[0] = acc[b][0]; dst[1] = acc[b][1]; dst[2] = acc[b][2];
    }
  }
}

// The kernel body of every family.  OWN_PIXEL: a thread owns pixel p and sums over texels j (forward, and the pixel
// gradients); else it owns texel j and sums over pixels (backward).  The family F supplies
//   Args, Norm           its arguments (WalkArgs first) and the normaliser of load_pixel
//   NSRC, NX             source floats per staged element; extras a pixel carries (x[0 .. NX - 1], at most 3)
//   extras(a, p, N, V, x)   the pixel's extras (its shininess, its hoisted roughness terms)
//   sources(a, s0, s1, s2)  the NSRC / (3 BC) source arrays
//   begin(a, o, live, N, V, X)   what the thread holds beside its geometry: rows, constants, zeroed accumulators
//   pair(a, N, V, X, L, r, on)   one pair: the pixel's N, V, X against the texel's L, r the staged element's source row
//   store(a, o, n_own, N, V)     the live thread's sums, for split blockIdx.y
template <bool OWN_PIXEL, int BC, bool MASKED, class F>
DEV void shade_walk(const typename F::Args& a, F& f) {
  constexpr int ROW = 4 * ((F::NSRC + 3) / 4);
  __shared__ float4 g0[SH_TILE];
  __shared__ float4 g1[OWN_PIXEL ? 1 : SH_TILE];
  __shared__ float g2[!OWN_PIXEL && F::NX > 2 ? SH_TILE : 1];
  __shared__ float4 sv[SH_TILE][ROW / 4];                         // source rows of the BC images
  __shared__ uint32_t mw[MASKED && !OWN_PIXEL ? SH_TILE : 1][8];  // backward: mask words of the stage's pixels
  const int tid = threadIdx.x;
  const int n_own = OWN_PIXEL ? a.NP : a.J, n_oth = OWN_PIXEL ? a.J : a.NP;
  const int o = blockIdx.x * 256 + tid;
  const bool live = o < n_own;
  float N[3] = {0.f, 0.f, 0.f}, V[3] = {0.f, 0.f, 0.f}, L[3] = {0.f, 0.f, 0.f}, X[3] = {1.f, 0.f, 1.f};
  if (live) {
    if (OWN_PIXEL) { load_pixel<typename F::Norm>(a, o, N, V); F::extras(a, o, N, V, X); }
    else { L[0] = a.ldir[(size_t)o * 3]; L[1] = a.ldir[(size_t)o * 3 + 1]; L[2] = a.ldir[(size_t)o * 3 + 2]; }
  }
  f.begin(a, o, live, N, V, X);
  const float *s0 = nullptr, *s1 = nullptr, *s2 = nullptr;
  F::sources(a, s0, s1, s2);

  // element e of the stage against the thread's own element
  auto pair = [&](int e, bool on) {
    const float4 q0 = g0[e];
    const float* r = (const float*)sv[e];
    if (OWN_PIXEL) {
      const float Lo[3] = {q0.x, q0.y, q0.z};
      f.pair(a, N, V, X, Lo, r, on);
    } else {
      const float4 q1 = g1[e];
      const float No[3] = {q0.x, q0.y, q0.z}, Vo[3] = {q0.w, q1.x, q1.y}, Xo[3] = {q1.z, q1.w, F::NX > 2 ? g2[e] : 0.f};
      f.pair(a, No, Vo, Xo, L, r, on);
    }
  };

  const int t_begin = blockIdx.y * a.per_split, t_end = min(n_oth, t_begin + a.per_split);
  for (int t0 = t_begin; t0 < t_end; t0 += SH_TILE) {
    __syncthreads();
    stage_geometry<OWN_PIXEL, F>(a, t0, t_end, g0, g1, g2);
    stage_rows<BC, F::NSRC>(a, s0, s1, s2, n_oth, t0, t_end, (float*)sv);
    if constexpr (MASKED && !OWN_PIXEL) stage_mask_words(a, t0, t_end, mw);
    __syncthreads();
    // (the unmasked walk is written here, not behind walk_masked's call: behind it k_envmap_terms<false, 4, false, false>
    // needs 72 registers per wave for 48 -- DESIGN 4.4o has the table)
    const int cnt = min(SH_TILE, t_end - t0);
    if constexpr (MASKED) walk_masked<OWN_PIXEL>(a, o, live, t0, cnt, mw, pair);
    else for (int e = 0; e < cnt; ++e) pair(e, true);
  }
  if (live) f.store(a, o, n_own, N, V);
}

// sum over the image chunks (ascending) of the chunk's sum over its splits (ascending) of part[chunk][split][p][0 .. C - 1]
template <int C>
DEV void sum_slots(const float* part, int NCH, int S, int NP, int p, float (&g)[C]) {
#pragma unroll
  for (int k = 0; k < C; ++k) g[k] = 0.f;
  for (int ch = 0; ch < NCH; ++ch) {
    float cs[C];
#pragma unroll
    for (int k = 0; k < C; ++k) cs[k] = 0.f;
    for (int q = 0; q < S; ++q) {
      const float* src = part + (((size_t)ch * S + q) * NP + p) * C;
#pragma unroll
      for (int k = 0; k < C; ++k) cs[k] += src[k];
    }
#pragma unroll
    for (int k = 0; k < C; ++k) g[k] += cs[k];
  }
}

// F.normalize's Jacobian: out = (g - N (N.g)) / |n|, or g / 1e-6 under its eps
DEV void normalize_jacobian(const float* nrm, int p, const float (&g)[3], float* out) {
  const float n[3] = {nrm[(size_t)p * 3], nrm[(size_t)p * 3 + 1], nrm[(size_t)p * 3 + 2]};
  const float len = sqrtf(fmaf(n[2], n[2], fmaf(n[1], n[1], n[0] * n[0])));
  const float inv = 1.f / fmaxf(len, 1e-6f);
  if (len >= 1e-6f) {
    const float N[3] = {n[0] * inv, n[1] * inv, n[2] * inv};
    const float d = fmaf(N[2], g[2], fmaf(N[1], g[1], N[0] * g[0]));
    out[0] = fmaf(-N[0], d, g[0]) * inv; out[1] = fmaf(-N[1], d, g[1]) * inv; out[2] = fmaf(-N[2], d, g[2]) * inv;
  } else {
    out[0] = g[0] * inv; out[1] = g[1] * inv; out[2] = g[2] * inv;
  }
}

// ---- the scalar shader: one coefficient M(p, j) ----------------------------------------------------------------------------
struct ShadeArgs {
  const float* nrm;        // [NP][3] interpolated vertex normals (not normalised; 0 where no face covers the pixel)
  const float* pos;        // [NP][3] interpolated surface positions
  const float* ldir;       // [J][3] texel directions of the image chunk's first image
  const float* src;        // forward: C [B][J][3]; backward: dcolors [B][NP][3]
  float* part;             // [S][B][NOWN][3] partial sums (S == 1: the output itself)
  float cam[3];
  float shin, kd, ksn;     // ksn = ks * (s + 2) / (4 (2 - exp(-s / 2)))     (:112-114)
  int B, NP, J, b0, nb;    // images b0 .. b0 + nb - 1 are handled by this launch (nb <= BC)
  int per_split;           // elements of the other axis per blockIdx.y
  const uint32_t* vis;     // MASKED: [NP][JW] visibility bits of the chunk's first image (bit j & 31 of word j >> 5)
  int JW;                  // words per pixel, ceil(J / 32)
};

// (the sum of squares is Normalize3's: one definition)
DEV void normalize3(float (&v)[3]) { Normalize3::apply(v); }

DEV float shade_coeff(const float (&N)[3], const float (&V)[3], const float (&L)[3], float shin, float kd, float ksn) {
  const float nl = fminf(fmaxf(N[0] * L[0] + N[1] * L[1] + N[2] * L[2], 0.f), 1.f);        // :87-88
  const float hx = V[0] + L[0], hy = V[1] + L[1], hz = V[2] + L[2];                          // :105
  const float inv = __builtin_amdgcn_rsqf(fmaxf(hx * hx + hy * hy + hz * hz, 1e-12f));       // 1 / max(|h|, 1e-6)  :107
  // normalise first, then dot, as the reference does
  const float nh = fminf(fmaxf(N[0] * (hx * inv) + N[1] * (hy * inv) + N[2] * (hz * inv), 0.f), 1.f);  // :108-109
  const float spec = __builtin_amdgcn_exp2f(shin * __builtin_amdgcn_logf(nh));               // pow(x, s), x in [0, 1]; 0 -> 0
  return kd * nl + ksn * spec;
}

// NOT on the skeleton: with the shared body the forward instances' view vectors moved by an ulp -- which two
// products of Normalize3's sum of squares the compiler packs depends on where the arguments' cam[] lies -- so this family
// keeps the body and the argument layout its bits were pinned with.  Written without fmaf, unlike the families below.
// OWN_PIXEL: a thread owns pixel p and sums over texels j (forward); else it owns texel j and sums over pixels.
// MASKED: M(p, j) counts only where bit (p, j) of a.vis is set (cast shadows, reni_tu_visibility.hip) -- a select on the
// coefficient, so the sums keep their order and an all-ones mask gives the unmasked instance's bits.  Forward: the pixel's
// four words of a 128-texel stage are one 16-byte load (four guarded loads when JW is no multiple of 4: the rows are then
// not 16-byte aligned).  Backward: the stage's 128 pixels x the workgroup's 8 words (its 256 texels) go through LDS.
template <bool OWN_PIXEL, int BC, bool MASKED = false>
__global__ void __launch_bounds__(256) k_envmap_shade(const ShadeArgs a) {
  __shared__ float4 g0[SH_TILE];       // other axis geometry: texel (Lx, Ly, Lz, -) | pixel (Nx, Ny, Nz, Vx)
  __shared__ float4 g1[SH_TILE];       //                                            | pixel (Vy, Vz, -, -)
  __shared__ float4 sv[SH_TILE][(3 * BC + 3) / 4];  // source rows of the BC images
  __shared__ uint32_t mw[MASKED && !OWN_PIXEL ? SH_TILE : 1][8];  // backward: mask words of the stage's pixels
  const int tid = threadIdx.x;
  const int n_own = OWN_PIXEL ? a.NP : a.J, n_oth = OWN_PIXEL ? a.J : a.NP;
  const int o = blockIdx.x * 256 + tid;
  const bool live = o < n_own;
  float N[3] = {0.f, 0.f, 0.f}, V[3] = {0.f, 0.f, 0.f}, L[3] = {0.f, 0.f, 0.f};
  auto load_pixel = [&](int p, float (&n)[3], float (&v)[3]) {
    n[0] = a.nrm[(size_t)p * 3]; n[1] = a.nrm[(size_t)p * 3 + 1]; n[2] = a.nrm[(size_t)p * 3 + 2];
    normalize3(n);
    v[0] = a.cam[0] - a.pos[(size_t)p * 3]; v[1] = a.cam[1] - a.pos[(size_t)p * 3 + 1]; v[2] = a.cam[2] - a.pos[(size_t)p * 3 + 2];  // :91
    normalize3(v);
  };
  if (live) {
    if (OWN_PIXEL) load_pixel(o, N, V);
    else { L[0] = a.ldir[(size_t)o * 3]; L[1] = a.ldir[(size_t)o * 3 + 1]; L[2] = a.ldir[(size_t)o * 3 + 2]; }
  }
  float acc[BC][3];
#pragma unroll
  for (int b = 0; b < BC; ++b) { acc[b][0] = 0.f; acc[b][1] = 0.f; acc[b][2] = 0.f; }

  const int t_begin = blockIdx.y * a.per_split, t_end = min(n_oth, t_begin + a.per_split);
  for (int t0 = t_begin; t0 < t_end; t0 += SH_TILE) {
    __syncthreads();
    if (tid < SH_TILE) {
      const int t = t0 + tid;
      float4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
      if (t < t_end) {
        if (OWN_PIXEL) {
          q0.x = a.ldir[(size_t)t * 3]; q0.y = a.ldir[(size_t)t * 3 + 1]; q0.z = a.ldir[(size_t)t * 3 + 2];
        } else {
          float n[3], v[3];
          load_pixel(t, n, v);
          q0 = float4{n[0], n[1], n[2], v[0]};
          q1 = float4{v[1], v[2], 0.f, 0.f};
        }
      }
      g0[tid] = q0;
      if (!OWN_PIXEL) g1[tid] = q1;
    }
    {  // source rows: 3 * BC floats per element, zero beyond the range / the chunk's images (they then add nothing)
      float* svf = (float*)sv;
      constexpr int ROW = 4 * ((3 * BC + 3) / 4);
      for (int i = tid; i < SH_TILE * 3 * BC; i += 256) {
        const int e = i / (3 * BC), r = i - e * (3 * BC), b = r / 3, c = r - b * 3;
        const int t = t0 + e;
        float x = 0.f;
        if (t < t_end && b < a.nb) x = a.src[((size_t)(a.b0 + b) * n_oth + t) * 3 + c];
        svf[e * ROW + r] = x;
      }
    }
    if constexpr (MASKED && !OWN_PIXEL) {
      for (int i = tid; i < SH_TILE * 8; i += 256) {
        const int e = i >> 3, w = blockIdx.x * 8 + (i & 7), t = t0 + e;
        mw[e][i & 7] = (t < t_end && w < a.JW) ? a.vis[(size_t)t * a.JW + w] : 0u;
      }
    }
    __syncthreads();
    const int cnt = min(SH_TILE, t_end - t0);
    if constexpr (MASKED) {
      uint32_t wv[4] = {0u, 0u, 0u, 0u};
      if (OWN_PIXEL && live) {  // (t0 is a multiple of SH_TILE: per_split is)
        const uint32_t* row = a.vis + (size_t)o * a.JW;
        const int w0 = t0 >> 5;
        if ((a.JW & 3) == 0) {
          const uint4 q = *(const uint4*)(row + w0);
          wv[0] = q.x; wv[1] = q.y; wv[2] = q.z; wv[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) wv[k] = w0 + k < a.JW ? row[w0 + k] : 0u;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // the same ascending walk as below, 32 elements per mask word
        const int e_end = min(cnt, 32 * k + 32);
        for (int e = 32 * k; e < e_end; ++e) {
          const float4 q0 = g0[e];
          float m;
          bool on;
          if (OWN_PIXEL) {
            const float Lo[3] = {q0.x, q0.y, q0.z};
            m = shade_coeff(N, V, Lo, a.shin, a.kd, a.ksn);
            on = (wv[k] >> (e & 31)) & 1u;
          } else {
            const float4 q1 = g1[e];
            const float No[3] = {q0.x, q0.y, q0.z}, Vo[3] = {q0.w, q1.x, q1.y};
            m = shade_coeff(No, Vo, L, a.shin, a.kd, a.ksn);
            on = (mw[e][tid >> 5] >> (tid & 31)) & 1u;
          }
          m = on ? m : 0.f;
          const float* s = (const float*)sv[e];
#pragma unroll
          for (int b = 0; b < BC; ++b) {
            acc[b][0] += m * s[3 * b]; acc[b][1] += m * s[3 * b + 1]; acc[b][2] += m * s[3 * b + 2];
          }
        }
      }
    } else
    for (int e = 0; e < cnt; ++e) {
      const float4 q0 = g0[e];
      float m;
      if (OWN_PIXEL) {
        const float Lo[3] = {q0.x, q0.y, q0.z};
        m = shade_coeff(N, V, Lo, a.shin, a.kd, a.ksn);
      } else {
        const float4 q1 = g1[e];
        const float No[3] = {q0.x, q0.y, q0.z}, Vo[3] = {q0.w, q1.x, q1.y};
        m = shade_coeff(No, Vo, L, a.shin, a.kd, a.ksn);
      }
      const float* s = (const float*)sv[e];
#pragma unroll
      for (int b = 0; b < BC; ++b) {
        acc[b][0] += m * s[3 * b]; acc[b][1] += m * s[3 * b + 1]; acc[b][2] += m * s[3 * b + 2];
      }
    }
  }
  if (live) {
#pragma unroll
    for (int b = 0; b < BC; ++b) {
      if (b < a.nb) {
        float* dst = a.part + (((size_t)blockIdx.y * a.B + (a.b0 + b)) * n_own + o) * 3;
        dst[0] = acc[b][0]; dst[1] = acc[b][1]; dst[2] = acc[b][2];
      }
    }
  }
}

// out[i] = sum_s part[s][i], s ascending
__global__ void __launch_bounds__(256) k_shade_reduce(const float* part, size_t n, int S, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += part[(size_t)k * n + i];
  out[i] = s;
}

// ---- per-pixel materials: the shader's TERMS ------------------------------------------------------------
// With an albedo per pixel and channel, and gradients with respect to the material, one coefficient M(p, j) no longer
// serves: the diffuse and the specular sums are kept apart, without kd, ks and norm(s) (those are applied behind the
// kernel, O(B NP) work), and the shininess s_p is the pixel's own.  v(p, j) is the visibility bit (1 without a mask):
//
//   D[b,p,:]  = sum_j v nl(p,j)                 C[b,j,:]
//   S[b,p,:]  = sum_j v nh(p,j)^s_p             C[b,j,:]
//   T[b,p,:]  = sum_j v nh(p,j)^s_p ln nh(p,j)  C[b,j,:]      = dS / ds_p; a pair with nh = 0 adds exactly 0   (WANT_T)
//   dC[b,j,:] = sum_p v ( nl(p,j) gD[b,p,:] + nh(p,j)^s_p gS[b,p,:] )
//
// The transcendentals per pair are the scalar shader's three (rsq, log, exp2): T reuses the log.  The microfacet terms
// below take the same arguments: up to three sources, one scalar per pixel, up to three sums.
struct TermsArgs : WalkArgs {
  const float* src0;       // forward: C [B][J][3]; backward: gD [B][NP][3]
  const float* src1;       // backward: gS (terms) | gS0 (GGX) [B][NP][3]
  const float* src2;       // backward: gS1 (GGX)
  const float* mat;        // the pixel's scalar mat[p * mat_stride]: shininess s_p (terms) | alpha a_p (GGX)
  int mat_stride;          // 0: one value for all pixels, 1: per pixel
  float* out[3];           // forward: D, S, T | D, S0, S1 (partial sums of split 0 when there are splits); backward: out[0] = dC
  size_t split_stride;     // floats from one split's partial sums to the next split's
};

// what the two families of TermsArgs share: NT sums over the BC images, each at its own output
template <bool OWN_PIXEL, int BC, int NT_FWD, int NSRC_BWD>
struct TermsSums {
  using Args = TermsArgs;
  using Norm = Normalize3;
  static constexpr int NSRC = OWN_PIXEL ? 3 * BC : NSRC_BWD * 3 * BC;  // source floats per staged element
  static constexpr int NT = OWN_PIXEL ? NT_FWD : 1;
  float acc[NT][BC][3];
  DEV static void sources(const Args& a, const float*& s0, const float*& s1, const float*& s2) { s0 = a.src0; s1 = a.src1; s2 = a.src2; }
  DEV void begin(const Args&, int, bool, const float (&)[3], const float (&)[3], const float (&)[3]) {
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
      for (int b = 0; b < BC; ++b) { acc[k][b][0] = 0.f; acc[k][b][1] = 0.f; acc[k][b][2] = 0.f; }
  }
  DEV void store(const Args& a, int o, int n_own, const float (&)[3], const float (&)[3]) {
#pragma unroll
    for (int k = 0; k < NT; ++k) store_partial<BC>(a, acc[k], a.out[k] + (size_t)blockIdx.y * a.split_stride, n_own, o);
  }
};

struct PairTerms { float nl, nh, lg; };  // clamp(N.L), clamp(N.H), log2 of the latter (-inf at 0)

// shade_coeff's geometry.  The multiply-adds are written out (here and at the accumulators): which products the compiler
// fuses then does not depend on the instance, so the MASKED and WANT_T instances give the plain instance's bits.
DEV PairTerms shade_pair(const float (&N)[3], const float (&V)[3], const float (&L)[3]) {
  PairTerms t;
  t.nl = fminf(fmaxf(fmaf(N[2], L[2], fmaf(N[1], L[1], N[0] * L[0])), 0.f), 1.f);
  const float hx = V[0] + L[0], hy = V[1] + L[1], hz = V[2] + L[2];
  const float inv = __builtin_amdgcn_rsqf(fmaxf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)), 1e-12f));  // 1 / max(|h|, 1e-6)
  // normalise first, then dot, as the reference does
  t.nh = fminf(fmaxf(fmaf(N[2], hz * inv, fmaf(N[1], hy * inv, N[0] * (hx * inv))), 0.f), 1.f);
  t.lg = __builtin_amdgcn_logf(t.nh);
  return t;
}

// OWN_PIXEL: forward (a thread owns pixel p: its N, V, s_p and 6 BC accumulators, 9 BC with WANT_T); else backward (a thread
// owns texel j; the stage holds per pixel N, V, s_p and the rows gD, gS: 6 BC floats).
template <bool OWN_PIXEL, int BC, bool MASKED, bool WANT_T>
struct TermsFamily : TermsSums<OWN_PIXEL, BC, WANT_T ? 3 : 2, 2> {
  static_assert(OWN_PIXEL || !WANT_T, "T is a forward output");
  using Base = TermsSums<OWN_PIXEL, BC, WANT_T ? 3 : 2, 2>;
  using Base::acc;
  static constexpr int NX = 1, NT = Base::NT;
  static constexpr float LN2 = 0.6931471805599453f;
  DEV static void extras(const TermsArgs& a, int p, const float (&)[3], const float (&)[3], float (&x)[3]) {
    x[0] = a.mat[(size_t)p * a.mat_stride];
  }
  DEV void pair(const TermsArgs&, const float (&N)[3], const float (&V)[3], const float (&X)[3], const float (&L)[3],
                const float* r, bool on) {
    const PairTerms t = shade_pair(N, V, L);
    const float s = X[0];
    float nl = t.nl;
    float sp = __builtin_amdgcn_exp2f(s * t.lg);             // nh^s; nh = 0: exp2(-inf) = 0
    float dsp = 0.f;
    if (WANT_T) dsp = t.nh > 0.f ? sp * (t.lg * LN2) : 0.f;  // nh^s ln nh, and 0 (not 0 * -inf) at nh = 0
    if (MASKED) { nl = on ? nl : 0.f; sp = on ? sp : 0.f; dsp = on ? dsp : 0.f; }
#pragma unroll
    for (int b = 0; b < BC; ++b) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (OWN_PIXEL) {
          acc[0][b][c] = fmaf(nl, r[3 * b + c], acc[0][b][c]);
          acc[1][b][c] = fmaf(sp, r[3 * b + c], acc[1][b][c]);
          if (WANT_T) acc[NT - 1][b][c] = fmaf(dsp, r[3 * b + c], acc[NT - 1][b][c]);
        } else {
          acc[0][b][c] = fmaf(sp, r[3 * BC + 3 * b + c], fmaf(nl, r[3 * b + c], acc[0][b][c]));
        }
      }
    }
  }
};

template <bool OWN_PIXEL, int BC, bool MASKED, bool WANT_T>
__global__ void __launch_bounds__(256) k_envmap_terms(const TermsArgs a) {
  TermsFamily<OWN_PIXEL, BC, MASKED, WANT_T> f;
  shade_walk<OWN_PIXEL, BC, MASKED>(a, f);
}

// out[k][i] = sum_s part[(s * NT + k) * n + i], s ascending; blockIdx.y = k
struct TermsReduceArgs { const float* part; float* out[3]; size_t n; int S, NT; };
__global__ void __launch_bounds__(256) k_terms_reduce(const TermsReduceArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int k = blockIdx.y;
  float s = 0.f;
  for (int q = 0; q < a.S; ++q) s += a.part[((size_t)q * a.NT + k) * a.n + i];
  float* out = k == 0 ? a.out[0] : k == 1 ? a.out[1] : a.out[2];
  out[i] = s;
}

// ---- normal-mapped materials: d loss / d normals of the terms --------------------------------------------
// With x_l = N.L, x_h = N.H before their clamps, a = sum_c gD[b,p,c] C[b,j,c] and b' = sum_c gS[b,p,c] C[b,j,c]:
//
//   gN[p]        = sum_b sum_j v ( [x_l > 0] a L + [x_h > 0] s_p nh^(s_p - 1) b' H )       (d loss / d N, N the unit normal)
//   d_normals[p] = (gN - N (N.gN)) / |n_p|,   gN / 1e-6 where |n_p| < 1e-6                  (F.normalize's Jacobian)
//
// The gates are strict and the clamps at 1 are ignored (x <= 1, and at x = 1 the projection removes the term), so a
// background pixel (n_p = 0: x_l = x_h = 0) gets exactly 0.  A relative of the OWN_PIXEL forward: a thread owns pixel p --
// N, V, s_p and the rows gD[b,p,:], gS[b,p,:] of the chunk's BC images in registers -- and walks the texels through the
// forward's stage (L and the C rows of the BC images).  Per pair shade_pair's three transcendentals (s nh^(s-1) = s exp2((s - 1) log2 nh),
// selected to 0 where nh = 0), 6 BC multiply-adds for a and b', 6 for the accumulators.  The texel axis is split over
// blockIdx.y; every (chunk, split) writes its own partial slot and k_terms_dn_reduce sums them in a fixed order and applies
// the Jacobian once.
// NOT on the skeleton, for the scalar shader's reason: the body and the argument layout its bits were pinned with.
struct TermsDnArgs {
  const float* nrm;        // [NP][3]
  const float* pos;        // [NP][3]
  const float* ldir;       // [J][3] texel directions of the image chunk's first image
  const float* col;        // C [B][J][3]
  const float* gD;         // [B][NP][3]
  const float* gS;         // [B][NP][3]
  const float* shin;       // s_p = shin[p * shin_stride]
  float* part;             // [S][NP][3] partial sums of this chunk
  float cam[3];
  int shin_stride;
  int B, NP, J, b0, nb;
  int per_split;
  const uint32_t* vis;     // MASKED: as ShadeArgs::vis
  int JW;
};

template <int BC, bool MASKED>
__global__ void __launch_bounds__(256) k_envmap_terms_dn(const TermsDnArgs a) {
  constexpr int NSRC = 3 * BC;
  constexpr int ROW = 4 * ((NSRC + 3) / 4);
  __shared__ float4 g0[SH_TILE];           // texel (Lx, Ly, Lz, -)
  __shared__ float4 sv[SH_TILE][ROW / 4];  // C rows of the BC images
  const int tid = threadIdx.x;
  const int o = blockIdx.x * 256 + tid;
  const bool live = o < a.NP;
  float N[3] = {0.f, 0.f, 0.f}, V[3] = {0.f, 0.f, 0.f}, shin = 1.f;
  float gd[BC][3], gs[BC][3];
#pragma unroll
  for (int b = 0; b < BC; ++b)
#pragma unroll
    for (int c = 0; c < 3; ++c) { gd[b][c] = 0.f; gs[b][c] = 0.f; }
  if (live) {
    N[0] = a.nrm[(size_t)o * 3]; N[1] = a.nrm[(size_t)o * 3 + 1]; N[2] = a.nrm[(size_t)o * 3 + 2];
    normalize3(N);
    V[0] = a.cam[0] - a.pos[(size_t)o * 3]; V[1] = a.cam[1] - a.pos[(size_t)o * 3 + 1]; V[2] = a.cam[2] - a.pos[(size_t)o * 3 + 2];
    normalize3(V);
    shin = a.shin[(size_t)o * a.shin_stride];
#pragma unroll
    for (int b = 0; b < BC; ++b) {
      if (b < a.nb) {  // (beyond the chunk's images the rows stay 0, as the stage's do: they add nothing)
        const size_t i = ((size_t)(a.b0 + b) * a.NP + o) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { gd[b][c] = a.gD[i + c]; gs[b][c] = a.gS[i + c]; }
      }
    }
  }
  const float sm1 = shin - 1.f;
  float acc[3] = {0.f, 0.f, 0.f};

  auto pair = [&](int e, bool on) {
    const float4 q0 = g0[e];
    const float Lo[3] = {q0.x, q0.y, q0.z};
    const PairTerms t = shade_pair(N, V, Lo);
    // H, in shade_pair's own expressions: inlined, they are the same values, computed once (one rsq per pair)
    const float hx = V[0] + Lo[0], hy = V[1] + Lo[1], hz = V[2] + Lo[2];
    const float inv = __builtin_amdgcn_rsqf(fmaxf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)), 1e-12f));
    const float Hv[3] = {hx * inv, hy * inv, hz * inv};
    const float* r = (const float*)sv[e];
    float ad = 0.f, as = 0.f;
#pragma unroll
    for (int b = 0; b < BC; ++b) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ad = fmaf(gd[b][c], r[3 * b + c], ad);
        as = fmaf(gs[b][c], r[3 * b + c], as);
      }
    }
    // the clamp maps x <= 0 to 0, so nl > 0 is x_l > 0 and nh > 0 is x_h > 0; at nh = 0 the power is 0, inf or NaN: selected away
    const float w = shin * __builtin_amdgcn_exp2f(sm1 * t.lg);
    float cl = t.nl > 0.f ? ad : 0.f;
    float ch = t.nh > 0.f ? w * as : 0.f;
    if (MASKED) { cl = on ? cl : 0.f; ch = on ? ch : 0.f; }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = fmaf(ch, Hv[k], fmaf(cl, Lo[k], acc[k]));
  };

  const int t_begin = blockIdx.y * a.per_split, t_end = min(a.J, t_begin + a.per_split);
  for (int t0 = t_begin; t0 < t_end; t0 += SH_TILE) {
    __syncthreads();
    if (tid < SH_TILE) {
      const int t = t0 + tid;
      float4 q0 = {0.f, 0.f, 0.f, 0.f};
      if (t < t_end) { q0.x = a.ldir[(size_t)t * 3]; q0.y = a.ldir[(size_t)t * 3 + 1]; q0.z = a.ldir[(size_t)t * 3 + 2]; }
      g0[tid] = q0;
    }
    {  // source rows, zero beyond the range / the chunk's images
      float* svf = (float*)sv;
      for (int i = tid; i < SH_TILE * NSRC; i += 256) {
        const int e = i / NSRC, r = i - e * NSRC, b = r / 3, c = r - b * 3;
        const int t = t0 + e;
        float x = 0.f;
        if (t < t_end && b < a.nb) x = a.col[((size_t)(a.b0 + b) * a.J + t) * 3 + c];
        svf[e * ROW + r] = x;
      }
    }
    __syncthreads();
    const int cnt = min(SH_TILE, t_end - t0);
    if constexpr (MASKED) {
      uint32_t wv[4] = {0u, 0u, 0u, 0u};
      if (live) {  // (t0 is a multiple of SH_TILE: per_split is)
        const uint32_t* row = a.vis + (size_t)o * a.JW;
        const int w0 = t0 >> 5;
        if ((a.JW & 3) == 0) {
          const uint4 q = *(const uint4*)(row + w0);
          wv[0] = q.x; wv[1] = q.y; wv[2] = q.z; wv[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) wv[k] = w0 + k < a.JW ? row[w0 + k] : 0u;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // the ascending walk of the unmasked instance, 32 elements per mask word
        const int e_end = min(cnt, 32 * k + 32);
        for (int e = 32 * k; e < e_end; ++e) pair(e, (wv[k] >> (e & 31)) & 1u);
      }
    } else {
      for (int e = 0; e < cnt; ++e) pair(e, true);
    }
  }
  if (live) {
    float* dst = a.part + ((size_t)blockIdx.y * a.NP + o) * 3;
    dst[0] = acc[0]; dst[1] = acc[1]; dst[2] = acc[2];
  }
}

// d_alpha[p] and gN[p] = sum_slots of the chunks' partial slots; d_normals[p] = gN through F.normalize's Jacobian
struct PixelGradReduceArgs { const float* part_a; const float* part_n; const float* nrm; float* d_alpha; float* d_normals; int NP, S, NCH; };
__global__ void __launch_bounds__(256) k_terms_dn_reduce(const PixelGradReduceArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.NP) return;
  float g[3];
  sum_slots<3>(a.part_n, a.NCH, a.S, a.NP, p, g);
  normalize_jacobian(a.nrm, p, g, a.d_normals + (size_t)p * 3);
}

// ---- microfacet (GGX) materials: the shader's terms for base colour / roughness / metallic ----------------
// Per pair, with H = (V + L) / max(|V + L|, 1e-6), x_l = N.L, x_h = N.H, x_v = N.V (nl, nh, nv their clamps to [0, 1]),
// u = clamp(V.H, 0, 1), f = (1 - u)^5, s2 = |N x H|^2, d = a^2 nh^2 + s2, lam(x) = sqrt(a^2 + (1 - a^2) x^2), a = alpha_p:
//
//   k(p,j)    = [x_h > 0] a^2 nl / ( d^2 (nl + lam(nl)) (nv + lam(nv)) )      (GGX D x separable Smith x nl, no 1 / pi)
//   D [b,p,:] = sum_j v nl  C[b,j,:]        S0[b,p,:] = sum_j v k C[b,j,:]        S1[b,p,:] = sum_j v k f C[b,j,:]
//   dC[b,j,:] = sum_p v ( nl gD[b,p,:] + k gS0[b,p,:] + k f gS1[b,p,:] )
//
// Schlick's Fresnel is affine in F0, so S0 and S1 do not depend on the material's colour: the composition behind the
// kernel (envmap_shader.compose_microfacet) is F0 S0 + (1 - F0) S1.  fmaf everywhere -- nl is shade_pair's expression, so D
// has the terms' bits.  What depends on the pixel alone is hoisted (a^2, 1 - a^2, pv = a^2 / (nv + lam(nv))): the pixel's
// three extras; per pair one rsq (H), one sqrt (lam(nl)) and one rcp (the whole denominator).  s2 comes from the cross
// product: 1 - x_h^2 cancels at the lobe's peak, where d is a^2-small.  Every denominator is at least a power of a > 0; the
// gate is a select, so a zero normal (d = 0) gives exactly 0.
struct GgxPixel { float a2, om, pv; };  // a^2, 1 - a^2, a^2 / (nv + lam(nv))

DEV GgxPixel ggx_pixel(const float (&N)[3], const float (&V)[3], float al) {
  GgxPixel g;
  g.a2 = al * al;
  g.om = fmaf(-al, al, 1.f);
  const float nv = fminf(fmaxf(fmaf(N[2], V[2], fmaf(N[1], V[1], N[0] * V[0])), 0.f), 1.f);
  g.pv = g.a2 / (nv + sqrtf(fmaf(g.om, nv * nv, g.a2)));
  return g;
}

struct GgxPair { float nl, k, kf; };

DEV GgxPair ggx_pair(const float (&N)[3], const float (&V)[3], const float (&L)[3], const GgxPixel& g) {
  GgxPair t;
  t.nl = fminf(fmaxf(fmaf(N[2], L[2], fmaf(N[1], L[1], N[0] * L[0])), 0.f), 1.f);  // shade_pair's
  const float hx = V[0] + L[0], hy = V[1] + L[1], hz = V[2] + L[2];
  const float inv = __builtin_amdgcn_rsqf(fmaxf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)), 1e-12f));  // 1 / max(|h|, 1e-6)
  const float Hx = hx * inv, Hy = hy * inv, Hz = hz * inv;
  const float xh = fmaf(N[2], Hz, fmaf(N[1], Hy, N[0] * Hx));
  const float nh = fminf(fmaxf(xh, 0.f), 1.f);
  const float u = fminf(fmaxf(fmaf(V[2], Hz, fmaf(V[1], Hy, V[0] * Hx)), 0.f), 1.f);
  const float cx = fmaf(N[1], Hz, -(N[2] * Hy)), cy = fmaf(N[2], Hx, -(N[0] * Hz)), cz = fmaf(N[0], Hy, -(N[1] * Hx));
  const float d = fmaf(g.a2, nh * nh, fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
  const float lam = __builtin_amdgcn_sqrtf(fmaf(g.om, t.nl * t.nl, g.a2));
  const float r = __builtin_amdgcn_rcpf((d * d) * (t.nl + lam));
  t.k = xh > 0.f ? (g.pv * t.nl) * r : 0.f;  // (a zero normal: d = 0, 0 * inf -- selected away)
  const float m = 1.f - u, m2 = m * m;
  t.kf = t.k * ((m2 * m2) * m);
  return t;
}

// OWN_PIXEL: forward (a thread owns pixel p: N, V, the hoisted three and 9 BC accumulators); else backward (a thread owns
// texel j; the stage holds per pixel N, V, the hoisted three and the rows gD, gS0, gS1: 9 BC floats).
template <bool OWN_PIXEL, int BC, bool MASKED>
struct GgxFamily : TermsSums<OWN_PIXEL, BC, 3, 3> {
  using Base = TermsSums<OWN_PIXEL, BC, 3, 3>;
  using Base::acc;
  static constexpr int NX = 3, NT = Base::NT;
  DEV static void extras(const TermsArgs& a, int p, const float (&n)[3], const float (&v)[3], float (&x)[3]) {
    const GgxPixel g = ggx_pixel(n, v, a.mat[(size_t)p * a.mat_stride]);
    x[0] = g.a2; x[1] = g.om; x[2] = g.pv;
  }
  DEV void pair(const TermsArgs&, const float (&N)[3], const float (&V)[3], const float (&X)[3], const float (&L)[3],
                const float* r, bool on) {
    const GgxPixel g = {X[0], X[1], X[2]};
    GgxPair t = ggx_pair(N, V, L, g);
    if (MASKED) { t.nl = on ? t.nl : 0.f; t.k = on ? t.k : 0.f; t.kf = on ? t.kf : 0.f; }
#pragma unroll
    for (int b = 0; b < BC; ++b) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (OWN_PIXEL) {
          acc[0][b][c] = fmaf(t.nl, r[3 * b + c], acc[0][b][c]);
          acc[1][b][c] = fmaf(t.k, r[3 * b + c], acc[1][b][c]);
          acc[NT - 1][b][c] = fmaf(t.kf, r[3 * b + c], acc[NT - 1][b][c]);
        } else {
          acc[0][b][c] = fmaf(t.kf, r[6 * BC + 3 * b + c], fmaf(t.k, r[3 * BC + 3 * b + c], fmaf(t.nl, r[3 * b + c], acc[0][b][c])));
        }
      }
    }
  }
};

template <bool OWN_PIXEL, int BC, bool MASKED>
__global__ void __launch_bounds__(256) k_envmap_ggx(const TermsArgs a) {
  GgxFamily<OWN_PIXEL, BC, MASKED> f;
  shade_walk<OWN_PIXEL, BC, MASKED>(a, f);
}

// d loss / d alpha and d loss / d normals of the three sums.  With ad = sum_c gD C, w = sum_c gS0 C + f sum_c gS1 C,
// kk = k / nl (computed without the division: nl = 0 is no special case), rd = 1 / d, sl = nl + lam(nl):
//
//   dk/da   = k ( 2 / a - 4 a nh^2 rd - a (1 - nl^2) / (lam(nl) sl) - a (1 - nv^2) / (lam(nv) (nv + lam(nv))) )
//   dk/dN  ~= [x_l > 0] ( kk - k (1 + (1 - a^2) nl / lam(nl)) / sl ) L + 4 k (1 - a^2) nh rd H
//             - [x_v > 0] k (1 + (1 - a^2) nv / lam(nv)) / (nv + lam(nv)) V
//
// (~=: up to a multiple of N, which F.normalize's Jacobian removes: d s2 / dN = 2 N |H|^2 - 2 x_h H, and with the a^2 nh^2
// term d d / dN ~= -2 (1 - a^2) nh H; u and f do not depend on N.)  What multiplies a per-pixel constant is summed as
// W = sum v k w and applied once per (chunk, split): the first and last terms of dk/da and the V term of dk/dN.  A thread
// owns a pixel -- N, V, the hoisted values and the rows gD, gS0, gS1 of the chunk's BC images in registers -- and walks the
// texels through the forward's stage.  The alpha sums do not depend on WANT_DN: asking for the normals' gradient does not
// move the roughness's.  Strict gates as in k_envmap_terms_dn; rd is 0 where x_h <= 0, so a zero normal gets exact zeros.
struct PixelGradArgs : WalkArgs {
  const float* col;        // C [B][J][3]
  const float* g0;         // upstream gradients [B][NP][3]: gD
  const float* g1;         // gS0
  const float* g2;         // gS1
  const float* mat;        // as TermsArgs::mat: alpha
  int mat_stride;
  float* part_a;           // [S][NP] partial sums of this chunk: d alpha
  float* part_n;           // [S][NP][3]: d N (WANT_DN)
};

// the rows g[b,o,:] of the chunk's images (beyond them the rows stay 0, as the stage's do: they add nothing)
template <int BC>
DEV void load_own_rows(const WalkArgs& a, const float* g, int o, bool live, float (&row)[BC][3]) {
#pragma unroll
  for (int b = 0; b < BC; ++b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) row[b][c] = 0.f;
    if (live && b < a.nb) {
      const size_t i = ((size_t)(a.b0 + b) * a.NP + o) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) row[b][c] = g[i + c];
    }
  }
}

template <int BC, bool MASKED, bool WANT_DN>
struct GgxDpFamily {
  using Args = PixelGradArgs;
  using Norm = Normalize3Fma;
  static constexpr int NSRC = 3 * BC, NX = 1;
  float gd[BC][3], g0s[BC][3], g1s[BC][3];
  float al, a2, om, pv, ca, gv, om4, accW, accA, acc[3];
  DEV static void extras(const Args& a, int p, const float (&)[3], const float (&)[3], float (&x)[3]) {
    x[0] = a.mat[(size_t)p * a.mat_stride];
  }
  DEV static void sources(const Args& a, const float*& s0, const float*&, const float*&) { s0 = a.col; }
  DEV void begin(const Args& a, int o, bool live, const float (&N)[3], const float (&V)[3], const float (&X)[3]) {
    load_own_rows<BC>(a, a.g0, o, live, gd);
    load_own_rows<BC>(a, a.g1, o, live, g0s);
    load_own_rows<BC>(a, a.g2, o, live, g1s);
    al = X[0];
    // per pixel: pv as in the forward, the alpha terms that do not depend on the texel (ca) and the V term's factor (gv)
    a2 = al * al, om = fmaf(-al, al, 1.f);
    const float xv = fmaf(N[2], V[2], fmaf(N[1], V[1], N[0] * V[0]));
    const float nv = fminf(fmaxf(xv, 0.f), 1.f);
    const float lamv = sqrtf(fmaf(om, nv * nv, a2));
    const float rv = 1.f / (nv + lamv);
    pv = a2 * rv;
    ca = 2.f / al - al * fmaf(-nv, nv, 1.f) * rv / lamv;
    gv = xv > 0.f ? fmaf(om, nv / lamv, 1.f) * rv : 0.f;
    om4 = 4.f * om;
    accW = 0.f, accA = 0.f, acc[0] = 0.f, acc[1] = 0.f, acc[2] = 0.f;
  }
  DEV void pair(const Args&, const float (&N)[3], const float (&V)[3], const float (&)[3], const float (&Lo)[3], const float* r,
                bool on) {
    const float nl = fminf(fmaxf(fmaf(N[2], Lo[2], fmaf(N[1], Lo[1], N[0] * Lo[0])), 0.f), 1.f);
    const float hx = V[0] + Lo[0], hy = V[1] + Lo[1], hz = V[2] + Lo[2];
    const float inv = __builtin_amdgcn_rsqf(fmaxf(fmaf(hz, hz, fmaf(hy, hy, hx * hx)), 1e-12f));
    const float Hv[3] = {hx * inv, hy * inv, hz * inv};
    const float xh = fmaf(N[2], Hv[2], fmaf(N[1], Hv[1], N[0] * Hv[0]));
    const float nh = fminf(fmaxf(xh, 0.f), 1.f);
    const float u = fminf(fmaxf(fmaf(V[2], Hv[2], fmaf(V[1], Hv[1], V[0] * Hv[0])), 0.f), 1.f);
    const float cx = fmaf(N[1], Hv[2], -(N[2] * Hv[1])), cy = fmaf(N[2], Hv[0], -(N[0] * Hv[2])), cz = fmaf(N[0], Hv[1], -(N[1] * Hv[0]));
    const float d = fmaf(a2, nh * nh, fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    const float lam = __builtin_amdgcn_sqrtf(fmaf(om, nl * nl, a2));
    const float rd = xh > 0.f ? __builtin_amdgcn_rcpf(d) : 0.f;  // the gate: everything below is finite
    const float rsl = __builtin_amdgcn_rcpf(nl + lam), rlam = __builtin_amdgcn_rcpf(lam);
    const float m = 1.f - u, m2 = m * m, f = (m2 * m2) * m;
    float ad = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int b = 0; b < BC; ++b) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ad = fmaf(gd[b][c], r[3 * b + c], ad);
        a0 = fmaf(g0s[b][c], r[3 * b + c], a0);
        a1 = fmaf(g1s[b][c], r[3 * b + c], a1);
      }
    }
    const float w = fmaf(f, a1, a0);
    const float kk = (pv * (rd * rd)) * rsl;  // k / nl
    const float k = kk * nl;
    float ks = k;
    if (MASKED) ks = on ? ks : 0.f;
    const float kw = ks * w;
    // alpha: the two terms that depend on the texel, 4 nh^2 / d + (1 - nl^2) / (lam sl)
    const float ta = fmaf(fmaf(-nl, nl, 1.f), rlam * rsl, (4.f * (nh * nh)) * rd);
    accA = fmaf(kw, ta, accA);
    accW = fmaf(ks, w, accW);
    if (WANT_DN) {
      // w (kk - k (1 + (1 - a^2) nl / lam) / sl) = w kk (1 - nl (1 + (1 - a^2) nl / lam) / sl)
      const float tl = fmaf(-(nl * rsl), fmaf(om * nl, rlam, 1.f), 1.f);
      float cl = nl > 0.f ? fmaf(w * kk, tl, ad) : 0.f;
      if (MASKED) cl = on ? cl : 0.f;
      const float ch = kw * ((om4 * nh) * rd);
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[q] = fmaf(ch, Hv[q], fmaf(cl, Lo[q], acc[q]));
    }
  }
  DEV void store(const Args& a, int o, int, const float (&)[3], const float (&V)[3]) {
    a.part_a[(size_t)blockIdx.y * a.NP + o] = fmaf(ca, accW, -(al * accA));
    if (WANT_DN) {
      float* dst = a.part_n + ((size_t)blockIdx.y * a.NP + o) * 3;
      const float cv = -(gv * accW);
      dst[0] = fmaf(cv, V[0], acc[0]); dst[1] = fmaf(cv, V[1], acc[1]); dst[2] = fmaf(cv, V[2], acc[2]);
    }
  }
};

template <int BC, bool MASKED, bool WANT_DN>
__global__ void __launch_bounds__(256) k_envmap_ggx_dpixel(const PixelGradArgs a) {
  GgxDpFamily<BC, MASKED, WANT_DN> f;
  shade_walk<true, BC, MASKED>(a, f);
}

// as k_terms_dn_reduce, with d alpha in front.  part_n NULL: alpha only.
__global__ void __launch_bounds__(256) k_ggx_dpixel_reduce(const PixelGradReduceArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.NP) return;
  float ga[1];
  sum_slots<1>(a.part_a, a.NCH, a.S, a.NP, p, ga);
  a.d_alpha[p] = ga[0];
  if (!a.part_n) return;
  float g[3];
  sum_slots<3>(a.part_n, a.NCH, a.S, a.NP, p, g);
  normalize_jacobian(a.nrm, p, g, a.d_normals + (size_t)p * 3);
}

}  // namespace reni

namespace {

constexpr int SHADE_BC = 4;

int n_splits(int64_t n_own, int64_t n_oth) {  // enough workgroups for 256 CUs, whole LDS tiles per split
  const int64_t wg_x = (n_own + 255) / 256;
  int64_t s = (2048 + wg_x - 1) / wg_x;
  const int64_t max_s = (n_oth + reni::SH_TILE - 1) / reni::SH_TILE;
  if (s > max_s) s = max_s;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return (int)s;
}

// what every entry point of the unit is given (what: its name in the messages)
struct ShadeCall {
  const char* what;
  int64_t B, NP, J;
  const float* normals;
  const float* positions;
  float cam[3];
  const float* light_dirs;
  int64_t dirs_bstride;
  const uint32_t* vis;
  int64_t vis_bstride;
  void* ws;
  size_t ws_bytes;
  void* stream;
};

// how a call is cut up: the owned and the walked axis, the splits of the walked one, the image chunks
struct ShadePlan {
  int64_t n_own, n_oth, n_chunks;
  int S, per_split, step, JW;
  dim3 grid;
  ShadePlan(bool forward, int64_t B, int64_t NP, int64_t J, int64_t dirs_bstride)
      : n_own(forward ? NP : J), n_oth(forward ? J : NP), S(n_splits(n_own, n_oth)),
        // images that share their texel directions share the pair's terms: chunks of SHADE_BC; otherwise one image per launch
        step(dirs_bstride == 0 ? SHADE_BC : 1), JW((int)((J + 31) / 32)), grid((unsigned)((n_own + 255) / 256), (unsigned)S) {
    n_chunks = (B + step - 1) / step;
    const int64_t tiles = (n_oth + reni::SH_TILE - 1) / reni::SH_TILE;
    per_split = (int)((tiles + S - 1) / S) * reni::SH_TILE;
  }
};

// the argument checks the calls share; 0 when all hold.  mat: "shininess" | "alpha", the per-pixel scalar whose stride is
// checked (NULL: the scalar shader has none).
int shade_checks(const ShadeCall& c, bool any_null, const char* mat = nullptr, int64_t mat_stride = 0) {
  const auto fail = [&](const char* text) { return tu_fail(RENI_EINVAL, c.what, text); };
  if (c.B < 1 || c.NP < 1 || c.J < 1) return fail("B, NP and J must be >= 1");
  if (c.NP > 0x3fffffff || c.J > 0x3fffffff || c.B > 0xffff) return fail("problem too large");
  if (any_null) return fail("NULL argument");
  if (c.dirs_bstride != 0 && c.dirs_bstride < c.J * 3) return fail("direction batch stride must be 0 or >= 3 J");
  if (mat && mat_stride != 0 && mat_stride != 1) return fail((std::string(mat) + " stride must be 0 (one value) or 1 (per pixel)").c_str());
  return RENI_OK;
}

// the mask's checks (null_text: what a NULL or misaligned mask is told)
int mask_checks(const ShadeCall& c, const char* null_text) {
  const auto fail = [&](const char* text) { return tu_fail(RENI_EINVAL, c.what, text); };
  if (!c.vis || ((uintptr_t)c.vis & 15) != 0) return fail(null_text);
  const int64_t JW = (c.J + 31) / 32;
  // (rows of JW % 4 == 0 words are read 16 bytes at a time: every image's mask must then start on such a boundary)
  if (c.vis_bstride != 0 && (c.dirs_bstride == 0 || c.vis_bstride < c.NP * JW || ((JW & 3) == 0 && (c.vis_bstride & 3) != 0)))
    return fail("mask batch stride must be 0 (required with shared directions) or >= NP ceil(J/32) words");
  return RENI_OK;
}

int workspace_check(const ShadeCall& c, size_t need) {
  if (need > 0 && (!c.ws || c.ws_bytes < need)) return tu_fail(RENI_EWORKSPACE, c.what, "workspace too small");
  return RENI_OK;
}

// the head of the arguments, then one launch of k per image chunk; slot(a, chunk) sets what else depends on the chunk
template <class Args, class Slot>
int launch_chunks(const ShadeCall& c, const ShadePlan& pl, void (*k)(const Args), Args& a, Slot slot) {
  a.nrm = c.normals; a.pos = c.positions;
  a.cam[0] = c.cam[0]; a.cam[1] = c.cam[1]; a.cam[2] = c.cam[2];
  a.B = (int)c.B; a.NP = (int)c.NP; a.J = (int)c.J;
  a.per_split = pl.per_split;
  a.vis = nullptr; a.JW = pl.JW;
  int64_t chunk = 0;
  for (int64_t b0 = 0; b0 < c.B; b0 += pl.step, ++chunk) {
    a.b0 = (int)b0; a.nb = (int)((c.B - b0) < pl.step ? (c.B - b0) : pl.step);
    a.ldir = c.light_dirs + (size_t)b0 * c.dirs_bstride;
    if (c.vis) a.vis = c.vis + (size_t)b0 * c.vis_bstride;
    slot(a, chunk);
    if (int rc = tu_launch(TU_PLAIN, k, pl.grid, dim3(256), 0, (hipStream_t)c.stream, a)) return rc;
  }
  return RENI_OK;
}

const auto no_slot = [](auto&, int64_t) {};

int shade_common(const ShadeCall& c, bool forward, bool masked, const float* src, float shininess, float kd, float ks, float* out) {
  if (int rc = shade_checks(c, !c.normals || !c.positions || !c.light_dirs || !src || !out)) return rc;
  if (!(shininess > 0.f)) return tu_fail(RENI_EINVAL, c.what, "shininess must be positive");
  if (masked)
    if (int rc = mask_checks(c, "the mask must be non-NULL and 16-byte aligned")) return rc;
  const ShadePlan pl(forward, c.B, c.NP, c.J, c.dirs_bstride);
  const size_t n = (size_t)c.B * pl.n_own * 3;
  if (int rc = workspace_check(c, pl.S > 1 ? pl.S * n * sizeof(float) : 0)) return rc;
  reni::ShadeArgs a;
  a.src = src;
  a.part = pl.S > 1 ? (float*)c.ws : out;
  a.shin = shininess; a.kd = kd;
  a.ksn = ks * (shininess + 2.f) / (4.f * (2.f - expf(-shininess * 0.5f)));
  using reni::k_envmap_shade;
  static constexpr void (*K[2][2][2])(const reni::ShadeArgs) = {  // [masked][one image per launch][forward]
      {{k_envmap_shade<false, SHADE_BC>, k_envmap_shade<true, SHADE_BC>}, {k_envmap_shade<false, 1>, k_envmap_shade<true, 1>}},
      {{k_envmap_shade<false, SHADE_BC, true>, k_envmap_shade<true, SHADE_BC, true>},
       {k_envmap_shade<false, 1, true>, k_envmap_shade<true, 1, true>}}};
  if (int rc = launch_chunks(c, pl, K[masked][pl.step == 1][forward], a, no_slot)) return rc;
  if (pl.S == 1) return RENI_OK;
  return tu_launch(TU_PLAIN, reni::k_shade_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)c.stream,
                   (const float*)c.ws, n, pl.S, out);
}

// floats of partial sums the terms pair needs: NT terms forward, one gradient backward (0 when there is one split)
size_t terms_partials(bool forward, int64_t B, int64_t NP, int64_t J, int NT) {
  const ShadePlan pl(forward, B, NP, J, 0);
  return pl.S > 1 ? (size_t)pl.S * (forward ? NT : 1) * B * pl.n_own * 3 : 0;
}

using TermsKernel = void (*)(const reni::TermsArgs);

// the terms and the microfacet terms.  forward: src[0] = C, outs = the NT sums; backward: src = the sums' gradients, outs[0] = dC
// (NT: the forward's sums).  mat_name, mat: the per-pixel scalar.  k[one image per launch][masked]: the instances.
int terms_common(const ShadeCall& c, bool forward, int NT, const float* const (&src)[3], const char* mat_name, const float* mat,
                 int64_t mat_stride, float* const (&outs)[3], bool any_null, const TermsKernel (&k)[2][2]) {
  if (int rc = shade_checks(c, any_null, mat_name, mat_stride)) return rc;
  if (c.vis)
    if (int rc = mask_checks(c, "the mask must be 16-byte aligned")) return rc;
  const ShadePlan pl(forward, c.B, c.NP, c.J, c.dirs_bstride);
  if (!forward) NT = 1;
  if (int rc = workspace_check(c, terms_partials(forward, c.B, c.NP, c.J, NT) * sizeof(float))) return rc;
  const size_t n = (size_t)c.B * pl.n_own * 3;
  reni::TermsArgs a;
  a.src0 = src[0]; a.src1 = src[1]; a.src2 = src[2];
  for (int i = 0; i < 3; ++i) a.out[i] = i >= NT ? nullptr : pl.S > 1 ? (float*)c.ws + (size_t)i * n : outs[i];
  a.mat = mat; a.mat_stride = (int)mat_stride;
  a.split_stride = (size_t)NT * n;
  if (int rc = launch_chunks(c, pl, k[pl.step == 1][c.vis != nullptr], a, no_slot)) return rc;
  if (pl.S == 1) return RENI_OK;
  reni::TermsReduceArgs r;
  r.part = (const float*)c.ws; r.n = n; r.S = pl.S; r.NT = NT;
  for (int i = 0; i < 3; ++i) r.out[i] = i < NT ? outs[i] : nullptr;
  return tu_launch(TU_PLAIN, reni::k_terms_reduce, dim3((unsigned)((n + 255) / 256), (unsigned)NT), dim3(256), 0,
                   (hipStream_t)c.stream, r);
}

// the pixel gradients (d normals of the terms; d alpha and, when wanted, d normals of the microfacet terms): one launch per
// image chunk into its own partial slots -- d alpha's [chunk][S][NP] first, then d N's [chunk][S][NP][3] -- then the
// fixed-order reduce.  a: the family's arguments with its sources and scalar set; parts(a, part_a, part_n) sets the chunk's
// slots; k[one image per launch][masked]: the instances.
template <class Args, class Parts>
int pixel_grad_common(const ShadeCall& c, Args& a, Parts parts, const char* mat_name, int64_t mat_stride, float* d_alpha,
                      float* d_normals, bool any_null, void (*const (&k)[2][2])(const Args),
                      void (*reduce)(const reni::PixelGradReduceArgs)) {
  if (int rc = shade_checks(c, any_null, mat_name, mat_stride)) return rc;
  if (c.vis)
    if (int rc = mask_checks(c, "the mask must be 16-byte aligned")) return rc;
  const ShadePlan pl(true, c.B, c.NP, c.J, c.dirs_bstride);
  const size_t slots = (size_t)pl.n_chunks * pl.S * c.NP;
  if (int rc = workspace_check(c, slots * ((d_alpha ? 1 : 0) + (d_normals ? 3 : 0)) * sizeof(float))) return rc;
  float* const part_a = d_alpha ? (float*)c.ws : nullptr;
  float* const part_n = d_normals ? (float*)c.ws + (d_alpha ? slots : 0) : nullptr;
  const auto slot = [&](Args& x, int64_t chunk) {
    parts(x, part_a ? part_a + (size_t)chunk * pl.S * c.NP : nullptr, part_n ? part_n + (size_t)chunk * pl.S * c.NP * 3 : nullptr);
  };
  if (int rc = launch_chunks(c, pl, k[pl.step == 1][c.vis != nullptr], a, slot)) return rc;
  reni::PixelGradReduceArgs r;
  r.part_a = part_a; r.part_n = part_n; r.nrm = c.normals; r.d_alpha = d_alpha; r.d_normals = d_normals;
  r.NP = (int)c.NP; r.S = pl.S; r.NCH = (int)pl.n_chunks;
  return tu_launch(TU_PLAIN, reduce, dim3((unsigned)((c.NP + 255) / 256)), dim3(256), 0, (hipStream_t)c.stream, r);
}

}  // namespace

extern "C" {

size_t reni_envmap_shade_workspace_bytes(int64_t B, int64_t NP, int64_t J) {
  if (B < 1 || NP < 1 || J < 1) return 0;
  const size_t f = (size_t)n_splits(NP, J) * B * NP * 3 * sizeof(float);
  const size_t g = (size_t)n_splits(J, NP) * B * J * 3 * sizeof(float);
  return (f > g ? f : g) + 256;
}

int reni_envmap_shade(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                      float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                      const float* light_colors, float shininess, float kd, float ks, float* colors, void* ws,
                      size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       nullptr, 0, ws, ws_bytes, stream};
  return shade_common(c, true, false, light_colors, shininess, kd, ks, colors);
}

int reni_envmap_shade_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                               float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                               const float* dcolors, float shininess, float kd, float ks, float* dlight_colors, void* ws,
                               size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       nullptr, 0, ws, ws_bytes, stream};
  return shade_common(c, false, false, dcolors, shininess, kd, ks, dlight_colors);
}

int reni_envmap_shade_masked(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                             float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                             const float* light_colors, float shininess, float kd, float ks, const uint32_t* vis,
                             int64_t vis_batch_stride, float* colors, void* ws, size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  return shade_common(c, true, true, light_colors, shininess, kd, ks, colors);
}

int reni_envmap_shade_masked_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                      float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                      int64_t dirs_batch_stride, const float* dcolors, float shininess, float kd, float ks,
                                      const uint32_t* vis, int64_t vis_batch_stride, float* dlight_colors, void* ws,
                                      size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  return shade_common(c, false, true, dcolors, shininess, kd, ks, dlight_colors);
}

size_t reni_envmap_shade_terms_workspace_bytes(int64_t B, int64_t NP, int64_t J, uint32_t flags) {
  if (B < 1 || NP < 1 || J < 1 || (flags & ~RENI_SHADE_TERMS_DS) != 0) return 0;
  const size_t f = terms_partials(true, B, NP, J, (flags & RENI_SHADE_TERMS_DS) ? 3 : 2) * sizeof(float);
  const size_t g = terms_partials(false, B, NP, J, 1) * sizeof(float);
  return (f > g ? f : g) + 256;
}

int reni_envmap_shade_terms(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                            float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                            const float* light_colors, const float* shininess, int64_t shininess_stride, const uint32_t* vis,
                            int64_t vis_batch_stride, float* diffuse, float* specular, float* dspecular_ds, void* ws,
                            size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade terms", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !light_colors || !shininess || !diffuse || !specular;
  using reni::k_envmap_terms;
  static constexpr TermsKernel K[2][2][2] = {  // [T wanted][one image per launch][masked]
      {{k_envmap_terms<true, SHADE_BC, false, false>, k_envmap_terms<true, SHADE_BC, true, false>},
       {k_envmap_terms<true, 1, false, false>, k_envmap_terms<true, 1, true, false>}},
      {{k_envmap_terms<true, SHADE_BC, false, true>, k_envmap_terms<true, SHADE_BC, true, true>},
       {k_envmap_terms<true, 1, false, true>, k_envmap_terms<true, 1, true, true>}}};
  return terms_common(c, true, dspecular_ds ? 3 : 2, {light_colors, nullptr, nullptr}, "shininess", shininess, shininess_stride,
                      {diffuse, specular, dspecular_ds}, any_null, K[dspecular_ds != nullptr]);
}

int reni_envmap_shade_terms_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                     float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                     int64_t dirs_batch_stride, const float* shininess, int64_t shininess_stride,
                                     const uint32_t* vis, int64_t vis_batch_stride, const float* d_diffuse,
                                     const float* d_specular, float* dlight_colors, void* ws, size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade terms", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !d_diffuse || !shininess || !dlight_colors || !d_specular;
  using reni::k_envmap_terms;
  static constexpr TermsKernel K[2][2] = {  // [one image per launch][masked]
      {k_envmap_terms<false, SHADE_BC, false, false>, k_envmap_terms<false, SHADE_BC, true, false>},
      {k_envmap_terms<false, 1, false, false>, k_envmap_terms<false, 1, true, false>}};
  return terms_common(c, false, 1, {d_diffuse, d_specular, nullptr}, "shininess", shininess, shininess_stride,
                      {dlight_colors, nullptr, nullptr}, any_null, K);
}

size_t reni_envmap_shade_terms_dnormals_workspace_bytes(int64_t B, int64_t NP, int64_t J) {
  if (B < 1 || NP < 1 || J < 1) return 0;
  // one slot per (image chunk, split): per-image directions make every image a chunk
  return (size_t)B * n_splits(NP, J) * NP * 3 * sizeof(float) + 256;
}

int reni_envmap_shade_terms_dnormals(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                     float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                     int64_t dirs_batch_stride, const float* light_colors, const float* shininess,
                                     int64_t shininess_stride, const uint32_t* vis, int64_t vis_batch_stride,
                                     const float* d_diffuse, const float* d_specular, float* d_normals, void* ws,
                                     size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade terms dnormals", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs,
                       dirs_batch_stride, vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !light_colors || !shininess || !d_diffuse || !d_specular || !d_normals;
  using reni::k_envmap_terms_dn;
  static constexpr void (*K[2][2])(const reni::TermsDnArgs) = {  // [one image per launch][masked]
      {k_envmap_terms_dn<SHADE_BC, false>, k_envmap_terms_dn<SHADE_BC, true>}, {k_envmap_terms_dn<1, false>, k_envmap_terms_dn<1, true>}};
  reni::TermsDnArgs a;
  a.col = light_colors; a.gD = d_diffuse; a.gS = d_specular;
  a.shin = shininess; a.shin_stride = (int)shininess_stride;
  const auto parts = [](reni::TermsDnArgs& x, float*, float* part_n) { x.part = part_n; };
  return pixel_grad_common(c, a, parts, "shininess", shininess_stride, nullptr, d_normals, any_null, K, reni::k_terms_dn_reduce);
}

size_t reni_envmap_shade_ggx_workspace_bytes(int64_t B, int64_t NP, int64_t J) {
  if (B < 1 || NP < 1 || J < 1) return 0;
  const size_t f = terms_partials(true, B, NP, J, 3) * sizeof(float);
  const size_t g = terms_partials(false, B, NP, J, 1) * sizeof(float);
  return (f > g ? f : g) + 256;
}

int reni_envmap_shade_ggx(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                          float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                          const float* light_colors, const float* alpha, int64_t alpha_stride, const uint32_t* vis,
                          int64_t vis_batch_stride, float* diffuse, float* spec0, float* spec1, void* ws, size_t ws_bytes,
                          void* stream) {
  const ShadeCall c = {"envmap shade ggx", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !light_colors || !alpha || !diffuse || !spec0 || !spec1;
  using reni::k_envmap_ggx;
  static constexpr TermsKernel K[2][2] = {  // [one image per launch][masked]
      {k_envmap_ggx<true, SHADE_BC, false>, k_envmap_ggx<true, SHADE_BC, true>}, {k_envmap_ggx<true, 1, false>, k_envmap_ggx<true, 1, true>}};
  return terms_common(c, true, 3, {light_colors, nullptr, nullptr}, "alpha", alpha, alpha_stride, {diffuse, spec0, spec1}, any_null, K);
}

int reni_envmap_shade_ggx_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                                   float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                                   const float* alpha, int64_t alpha_stride, const uint32_t* vis, int64_t vis_batch_stride,
                                   const float* d_diffuse, const float* d_spec0, const float* d_spec1, float* dlight_colors,
                                   void* ws, size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade ggx", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs, dirs_batch_stride,
                       vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !d_diffuse || !alpha || !dlight_colors || !d_spec0 || !d_spec1;
  using reni::k_envmap_ggx;
  static constexpr TermsKernel K[2][2] = {  // [one image per launch][masked]
      {k_envmap_ggx<false, SHADE_BC, false>, k_envmap_ggx<false, SHADE_BC, true>}, {k_envmap_ggx<false, 1, false>, k_envmap_ggx<false, 1, true>}};
  return terms_common(c, false, 1, {d_diffuse, d_spec0, d_spec1}, "alpha", alpha, alpha_stride, {dlight_colors, nullptr, nullptr},
                      any_null, K);
}

size_t reni_envmap_shade_ggx_dpixel_workspace_bytes(int64_t B, int64_t NP, int64_t J) {
  if (B < 1 || NP < 1 || J < 1) return 0;
  // one slot of 1 + 3 floats per (image chunk, split, pixel): per-image directions make every image a chunk
  return (size_t)B * n_splits(NP, J) * NP * 4 * sizeof(float) + 256;
}

int reni_envmap_shade_ggx_dpixel(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                                 float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                                 const float* light_colors, const float* alpha, int64_t alpha_stride, const uint32_t* vis,
                                 int64_t vis_batch_stride, const float* d_diffuse, const float* d_spec0, const float* d_spec1,
                                 float* d_alpha, float* d_normals, void* ws, size_t ws_bytes, void* stream) {
  const ShadeCall c = {"envmap shade ggx dpixel", B, NP, J, normals, positions, {cam_x, cam_y, cam_z}, light_dirs,
                       dirs_batch_stride, vis, vis_batch_stride, ws, ws_bytes, stream};
  const bool any_null = !normals || !positions || !light_dirs || !light_colors || !alpha || !d_diffuse || !d_spec0 || !d_spec1 || !d_alpha;
  using reni::k_envmap_ggx_dpixel;
  static constexpr void (*K[2][2][2])(const reni::PixelGradArgs) = {  // [d normals wanted][one image per launch][masked]
      {{k_envmap_ggx_dpixel<SHADE_BC, false, false>, k_envmap_ggx_dpixel<SHADE_BC, true, false>},
       {k_envmap_ggx_dpixel<1, false, false>, k_envmap_ggx_dpixel<1, true, false>}},
      {{k_envmap_ggx_dpixel<SHADE_BC, false, true>, k_envmap_ggx_dpixel<SHADE_BC, true, true>},
       {k_envmap_ggx_dpixel<1, false, true>, k_envmap_ggx_dpixel<1, true, true>}}};
  reni::PixelGradArgs a;
  a.col = light_colors; a.g0 = d_diffuse; a.g1 = d_spec0; a.g2 = d_spec1;
  a.mat = alpha; a.mat_stride = (int)alpha_stride;
  const auto parts = [](reni::PixelGradArgs& x, float* part_a, float* part_n) { x.part_a = part_a; x.part_n = part_n; };
  return pixel_grad_common(c, a, parts, "alpha", alpha_stride, d_alpha, d_normals, any_null, K[d_normals != nullptr],
                           reni::k_ggx_dpixel_reduce);
}

}  // extern "C"
