// translation unit of libreni_hip.so: what split-sum microfacet shading from a prefiltered chain needs besides the glossy
// units (reni_tu_glossy.hip, reni_tu_glossy_bwd.hip; reni_amd/glossy.py: sample, ggx_dfg, shade_split_sum).  No reference
// counterpart.
//
// fp32 throughout, no float atomics, every sum in a fixed order: two calls give identical bits.  Contraction is off for the
// whole unit: what is written is what runs.
//
//   k_envmap_lookup_dquery<WANT_DIRS, WANT_LEVEL>   the derivative of k_envmap_lookup's output with respect to its QUERY -- the
//                       direction and the level -- contracted with grad_out [N][P][3].  One lane per direction; the coordinate
//                       chain is the lookup's (sph_rowcol, sph_taps, sph_level of reni_sphere.inc).  With b00 .. b11 the folded
//                       taps of a level and (fr, gr, fc, gc) the lookup's fractions
//                           d out / d row = gc (b10 - b00) + fc (b11 - b01)        d out / d col = gr (b01 - b00) + fr (b11 - b10)
//                       mixed over the two levels as the forward mixes the values; Gr = <g, d out / d row>, Gc likewise, and
//                           d_dirs = row_scale Gr d phi / d q + col_scale Gc d theta / d q
//                           d phi / d q = (q_y q_x / rho, -rho, q_y q_z / rho) / |q|^2,  d theta / d q = (-q_z, 0, q_x) / rho^2
//                       with rho^2 = q_x^2 + q_z^2 (q need not be a unit vector).  Exactly 0 where the row clamp is active, at
//                       a pole direction (rho^2 = 0) and for the zero vector; never NaN or Inf for finite maps.
//                           d_level = [0 <= level <= Lv - 1] <g, v(la + 1) - v(la)>,  la = min(floor(level), Lv - 2)
//                       the slope of the piecewise-linear mix, right-sided at interior knots and left-sided at the top one;
//                       0 for Lv = 1, a level outside the closed range, or a NaN level.
//                       An output whose operand is shared by the N maps (stride 0) is the sum over n ascending, written once
//                       ([P][3] / [P]): the lane then loops over n, else the grid spans n.  For shared directions Gr and Gc
//                       are summed over n and the chain rule is applied once.
//   k_ggx_dfg           the directional-albedo table A[m][j][i] of the microfacet material (DESIGN 4.4m's k and f):
//                       A0 = int k d omega, A1 = int k f d omega for N = (0, 0, 1), V = (sqrt(1 - x^2), 0, x), x = i / (R_v - 1),
//                       roughness r_j = r_min + j (1 - r_min) / (R_r - 1), alpha = r^2.  DEFINED as the midpoint rule on M_u x
//                       M_phi nodes of GGX's inverse-CDF parametrisation of the half vector, cos^2 theta_h = (1 - u) /
//                       (1 + (alpha^2 - 1) u), L = 2 (V.H) H - V, under which
//                           A0 = int int 2 nl (V.H) / (nh (nl + lam(nl)) (nv + lam(nv))) [nl > 0][V.H > 0] du dphi
//                       One workgroup per entry; a lane sums its nodes (lane, lane + 256, ...) ascending, a fixed-order LDS
//                       tree adds the lanes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"

#pragma clang fp contract(off)

#include "reni_sphere.inc"  // (row, col), taps and level of a lookup, the query record with its checks

namespace reni {

struct DqArgs : SphQuery {
  const float* grad_out;  // [N][P][3]
  float* d_dirs;          // [P][3] when dn == 0, else [N][P][3]
  float* d_level;         // [P] when ln == 0, else [N][P]
  int loop;  // 1: one lane serves every map of its direction (a wanted output is shared); 0: blockIdx.y is the map
};

// what of a direction the chain rule needs, or ok = false where the derivative is defined as 0
struct DqGeom {
  bool ok;
  float px, py, pz;  // d phi / d q
  float tx, tz;      // d theta / d q (its y is 0)
};

DEV DqGeom dq_geom(float sx, float sy, float sz, float row, int H) {
  DqGeom g;
  const float rho2 = fmaf(sz, sz, sx * sx);
  const float q2 = fmaf(sy, sy, rho2);
  g.ok = rho2 > 0.f && q2 > 0.f && q2 < INFINITY && row > -1.f && row < (float)H;  // (a NaN fails the comparisons)
  const float rho = sqrtf(rho2);
  const float cx = sx / rho, cz = sz / rho, yq = sy / q2;
  g.px = yq * cx;
  g.py = -(rho / q2);
  g.pz = yq * cz;
  g.tx = -sz / rho2;
  g.tz = sx / rho2;
  return g;
}

template <bool WANT_DIRS, bool WANT_LEVEL>
__global__ void __launch_bounds__(256) k_envmap_lookup_dquery(const DqArgs a) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;  // P < 2^30
  if (p >= a.P) return;
  const int n_lo = a.loop ? 0 : (int)blockIdx.y, n_hi = a.loop ? a.N : n_lo + 1;
  const bool dirs_shared = a.dn == 0, level_shared = a.ln == 0;
  float fr = 0.f, gr = 1.f, fc = 0.f, gc = 1.f;
  int64_t o00 = 0, o01 = 0, o10 = 0, o11 = 0;
  DqGeom geo = {};
  float GrS = 0.f, GcS = 0.f, GlS = 0.f;
  bool inrS = false;
  for (int nn = n_lo; nn < n_hi; ++nn) {
    const int64_t n = nn;
    if (nn == n_lo || !dirs_shared) {
      const float* d = a.dirs + n * a.dn + 3 * (int64_t)p;
      const float sx = d[0], sy = d[1], sz = d[2];
      float row, col;
      sph_rowcol(sx, sy, sz, a.H, a.W, a.row_scale, a.col_scale, a.col_bias, row, col);
      const SphTaps t = sph_taps(row, col, a.H, a.W);
      fr = t.fr, gr = t.gr, fc = t.fc, gc = t.gc;
      const int64_t r0 = (int64_t)t.i0 * (int64_t)a.sy, r1 = (int64_t)t.i1 * (int64_t)a.sy;
      o00 = r0 + (int64_t)t.j00 * (int64_t)a.sx, o01 = r0 + (int64_t)t.j01 * (int64_t)a.sx;
      o10 = r1 + (int64_t)t.j10 * (int64_t)a.sx, o11 = r1 + (int64_t)t.j11 * (int64_t)a.sx;
      if (WANT_DIRS) geo = dq_geom(sx, sy, sz, row, a.H);
    }
    // ---- the level: the forward's (l0, fl, gl), read as weights (wa, wb) of the pair (la, la + 1) the slope is taken over
    const float lv = a.level ? a.level[n * a.ln + p] : a.level_const;
    const SphLevel L = sph_level(lv, a.Lv);
    const int la = max(min(L.l0, a.Lv - 2), 0), lb = min(la + 1, a.Lv - 1);
    const bool top = L.l0 != la;  // the forward sits on the top knot (fl = 0): all of its weight is on lb
    const float wa = top ? 0.f : L.gl, wb = top ? 1.f : L.fl;
    const bool inr = a.Lv > 1 && lv >= 0.f && lv <= (float)(a.Lv - 1);  // (a NaN fails the comparisons)
    const float* ba = a.src + n * a.sn + (int64_t)la * a.sl;
    const float* bb = a.src + n * a.sn + (int64_t)lb * a.sl;
    const float* g = a.grad_out + (n * a.P + p) * 3;
    float Gr = 0.f, Gc = 0.f, Gl = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch, ba += a.sc, bb += a.sc) {
      const float gch = g[ch];
      const float a00 = ba[o00], a01 = ba[o01], a10 = ba[o10], a11 = ba[o11];
      const float b00 = bb[o00], b01 = bb[o01], b10 = bb[o10], b11 = bb[o11];
      if (WANT_DIRS) {
        const float dra = fmaf(fc, a11 - a01, gc * (a10 - a00)), drb = fmaf(fc, b11 - b01, gc * (b10 - b00));
        const float dca = fmaf(fr, a11 - a10, gr * (a01 - a00)), dcb = fmaf(fr, b11 - b10, gr * (b01 - b00));
        Gr = fmaf(gch, fmaf(wb, drb, wa * dra), Gr);
        Gc = fmaf(gch, fmaf(wb, dcb, wa * dca), Gc);
      }
      if (WANT_LEVEL) {
        const float va = fmaf(fr, fmaf(fc, a11, gc * a10), gr * fmaf(fc, a01, gc * a00));
        const float vb = fmaf(fr, fmaf(fc, b11, gc * b10), gr * fmaf(fc, b01, gc * b00));
        Gl = fmaf(gch, vb - va, Gl);
      }
    }
    if (WANT_DIRS) {
      if (dirs_shared) {
        GrS += Gr, GcS += Gc;
      } else {
        const float tr = a.row_scale * Gr, tc = a.col_scale * Gc;
        float* o = a.d_dirs + (n * a.P + p) * 3;
        o[0] = geo.ok ? fmaf(tc, geo.tx, tr * geo.px) : 0.f;
        o[1] = geo.ok ? tr * geo.py : 0.f;
        o[2] = geo.ok ? fmaf(tc, geo.tz, tr * geo.pz) : 0.f;
      }
    }
    if (WANT_LEVEL) {
      if (level_shared) {
        GlS += Gl, inrS = inr;
      } else {
        a.d_level[n * a.P + p] = inr ? Gl : 0.f;
      }
    }
  }
  if (WANT_DIRS && dirs_shared) {
    const float tr = a.row_scale * GrS, tc = a.col_scale * GcS;
    float* o = a.d_dirs + 3 * (int64_t)p;
    o[0] = geo.ok ? fmaf(tc, geo.tx, tr * geo.px) : 0.f;
    o[1] = geo.ok ? tr * geo.py : 0.f;
    o[2] = geo.ok ? fmaf(tc, geo.tz, tr * geo.pz) : 0.f;
  }
  if (WANT_LEVEL && level_shared) a.d_level[p] = inrS ? GlS : 0.f;
}

constexpr int DFG_LANES = 256;

// lam(t) = sqrt(alpha^2 + (1 - alpha^2) t^2)
DEV float dfg_lam(float t, float al2, float om) { return sqrtf(fmaf(om, t * t, al2)); }

__global__ void __launch_bounds__(DFG_LANES) k_ggx_dfg(int R_v, int R_r, float r_min, int M_u, int M_phi, float* __restrict__ out) {
  __shared__ float s0[DFG_LANES], s1[DFG_LANES];
  const int i = (int)blockIdx.x, j = (int)blockIdx.y, lane = (int)threadIdx.x;
  const float x = (float)i / (float)(R_v - 1);
  const float r = fmaf((float)j, (1.f - r_min) / (float)(R_r - 1), r_min);
  const float al = r * r, al2 = al * al, om = 1.f - al2;
  const float Vx = sqrtf(fmaxf(1.f - x * x, 0.f)), Vz = x;
  const float gv = Vz + dfg_lam(Vz, al2, om);  // nv + lam(nv) > 0: lam >= alpha
  const float two_pi = 6.283185307179586f;
  float A0 = 0.f, A1 = 0.f;
  const int nodes = M_u * M_phi;  // <= 2^20 (checked)
  for (int k = lane; k < nodes; k += DFG_LANES) {
    const int ku = k / M_phi, kp = k - ku * M_phi;
    const float u = ((float)ku + 0.5f) / (float)M_u;
    const float phi = two_pi * (((float)kp + 0.5f) / (float)M_phi);
    // cos^2 theta_h in (0, 1]; 1 + (alpha^2 - 1) u written as (1 - u) + alpha^2 u, which does not cancel towards u = 1
    const float c2 = (1.f - u) / fmaf(al2, u, 1.f - u);
    const float nh = sqrtf(c2), sh = sqrtf(fmaxf(1.f - c2, 0.f));
    float sp, cp;
    sincosf(phi, &sp, &cp);
    const float vh = fmaf(Vz, nh, Vx * (sh * cp));
    const float nl = fmaf(2.f * vh, nh, -Vz);
    const bool open = nl > 0.f && vh > 0.f;
    const float nls = open ? nl : 0.f;
    const float den = (nh * (nls + dfg_lam(nls, al2, om))) * gv;
    const float val = open ? ((2.f * nls) * vh) / den : 0.f;
    const float w = 1.f - fminf(vh, 1.f), w2 = w * w;
    A0 += val;
    A1 += val * ((w2 * w2) * w);
  }
  s0[lane] = A0;
  s1[lane] = A1;
  __syncthreads();
  for (int s = DFG_LANES / 2; s >= 1; s >>= 1) {
    if (lane < s) {
      s0[lane] += s0[lane + s];
      s1[lane] += s1[lane + s];
    }
    __syncthreads();
  }
  if (lane == 0) {
    const float wq = two_pi / ((float)M_u * (float)M_phi);  // du dphi of a node
    const int64_t e = (int64_t)j * R_v + i, plane = (int64_t)R_r * R_v;
    out[e] = s0[0] * wq;
    out[plane + e] = s1[0] * wq;
  }
}

}  // namespace reni

namespace {
using reni::reni_set_error;
}  // namespace

extern "C" {

int reni_envmap_lookup_dquery(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src,
                              const int64_t src_strides[5], const float* dirs, int64_t dirs_stride_n, const float* level,
                              int64_t level_stride_n, float level_const, const float* grad_out, float* d_dirs, float* d_level,
                              void* stream) {
  if (int rc = sph_check_query(true, N, Lv, H, W, P, src, src_strides, dirs, dirs_stride_n, level, level_stride_n, grad_out != nullptr))
    return rc;
  if (!d_dirs && !d_level) return reni_set_error(RENI_EINVAL, "lookup dquery: d_dirs and d_level are both NULL");
  if (d_level && !level) return reni_set_error(RENI_EINVAL, "lookup dquery: d_level needs a level array");
  reni::DqArgs a = {};
  sph_fill_query(a, N, Lv, H, W, P, src, src_strides, dirs, dirs_stride_n, level, level_stride_n, level_const);
  a.grad_out = grad_out; a.d_dirs = d_dirs; a.d_level = d_level;
  a.loop = ((d_dirs && a.dn == 0) || (d_level && a.ln == 0)) ? 1 : 0;
  const auto k = d_dirs && d_level ? reni::k_envmap_lookup_dquery<true, true>
                 : d_dirs          ? reni::k_envmap_lookup_dquery<true, false>
                                   : reni::k_envmap_lookup_dquery<false, true>;
  return tu_launch(TU_PLAIN, k, dim3((unsigned)((P + 255) / 256), a.loop ? 1u : (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
}

int reni_ggx_dfg(int64_t R_v, int64_t R_r, float r_min, int64_t M_u, int64_t M_phi, float* out, void* stream) {
  if (R_v < 2 || R_r < 2 || R_v > 1024 || R_r > 1024) return reni_set_error(RENI_EINVAL, "ggx dfg: need 2 <= R_v, R_r <= 1024");
  if (M_u < 1 || M_phi < 1 || M_u > 1024 || M_phi > 1024) return reni_set_error(RENI_EINVAL, "ggx dfg: need 1 <= M_u, M_phi <= 1024");
  if (R_v * R_r * M_u * M_phi > ((int64_t)1 << 28))
    return reni_set_error(RENI_EINVAL, "ggx dfg: need R_v R_r M_u M_phi <= 2^28 (entries x nodes)");
  if (!(r_min >= 1e-3f) || !(r_min < 1.f)) return reni_set_error(RENI_EINVAL, "ggx dfg: need 1e-3 <= r_min < 1");
  if (!out) return reni_set_error(RENI_EINVAL, "ggx dfg: NULL argument");
  return tu_launch(TU_PLAIN, reni::k_ggx_dfg, dim3((unsigned)R_v, (unsigned)R_r), dim3(reni::DFG_LANES), 0, (hipStream_t)stream, (int)R_v,
                   (int)R_r, r_min, (int)M_u, (int)M_phi, out);
}

}  // extern "C"
