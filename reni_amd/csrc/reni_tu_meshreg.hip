// translation unit of libreni_hip.so: the three mesh regularisers of SoftRas / pytorch3d.loss -- edge length, Laplacian
// smoothing (uniform or cotangent weights) and normal consistency -- as one weighted objective, its three values and its
// gradient with respect to the vertex positions (reni_mesh_regularizers; include/reni_hip.h has the definitions in full).
//
// Topology (ops.mesh_edge_lists, built once per face tensor): a face TAKES PART iff its indices lie in [0, V) and are pairwise
// different; edges [E][2] = the unique undirected edges (a < b) of those faces in ascending (a, b); per edge the corners
// 3 f + k OPPOSITE it in ascending order (ef); per vertex its edges in ascending order (ve); per corner the edge opposite it
// (corner_edge); per vertex its corners (vf, ops.vertex_face_lists).  A pair is two entries i < j of one edge's ef list.
//
// fp32, no float atomic, no in-launch ticket: every sum has one fixed order that depends on the lists alone, so two calls give
// identical bits.  The gradient is produced with the forward (the objective is a scalar).  Five kernels:
//
//   k_mr_face     (cot only) one thread per face: Heron's area, the three cotangents -> cotw [3F], 0 for a face not taking part.
//   k_mr_edge     one thread per edge: the length term and its gradient, the edge's cot weight (its ef entries in list order),
//                 the edge's pairs in ascending (i, j): 1 - cos and the gradients of the two END POINTS summed over the pairs.
//                 Writes a record of MR_EREC floats and the edge's row of the partial sums (length term, sum of 1 - cos, pairs).
//   k_mr_lap      one thread per vertex: walks its ascending edge list, r_v, |r_v| into the partial sums, u_v = r_v / |r_v| and
//                 q_v = n_v u_v into a record.
//   k_mr_reduce   the store-then-sum reducer on k_cam_reduce's pattern: a workgroup of four waves per MR_CHUNK rows, a fixed lane
//                 stride, a butterfly of shuffles, the waves in ascending order; relaunched on the chunk sums until one chunk is
//                 left, which writes the three values, the weighted total and w_n / P for the gather.  The pair count is an
//                 integer column.
//   k_mr_gather   one thread per vertex: its edges' records in list order (length and end-point gradients, w_e q_j of the
//                 Laplacian), minus u_v; then its corners in list order: for the edge opposite the corner, the pairs of this
//                 face with every other entry of that edge, recomputed with k_mr_edge's own function (mr_pair) -- the gradient of
//                 the OPPOSITE vertex.  grad = (w_e / E) g_e + (w_l / V) g_l + (w_n / P) g_n.
//
// Nothing of a list is trusted: an offset is clamped into its list, an edge must be 0 <= a < b < V, an ef entry must be a
// corner of a face taking part whose opposite edge is that edge, a ve entry must name an edge holding the vertex, a corner must
// name the vertex and corner_edge must agree with the face.  What fails adds nothing and is never turned into an address.
// Cost and limits: an edge of multiplicity m costs its thread m (m - 1) / 2 pairs, and so does a malformed ef_offsets that hands
// one edge a long range (H <= 3F bounds it); the pair count is a 32-bit integer, so P must stay below 2^31.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"
#include "reni_mesh.inc"

namespace reni {

constexpr int MR_EREC = 10;      // floats per edge record: d L_e / d a [3] (b gets the negative), the pairs' d / d a [3], d / d b [3], w_e
constexpr int MR_LREC = 6;       // floats per vertex record of the Laplacian: u_v [3], q_v = n_v u_v [3]
constexpr int MR_COLS = 4;       // columns of the partial sums: length terms, |r_v|, 1 - cos, pairs (an int)
constexpr int MR_CHUNK = 4096;   // rows per workgroup of the reducer (16 per thread)
constexpr float MR_AREA_FLOOR = 1e-12f;  // of Heron's area
constexpr float MR_NRM_FLOOR = 1e-8f;    // of |n0|, |n1| in the normal consistency (this loss's own, not the rasteriser's epsilon)

struct MrArgs {
  const float* verts;
  const int64_t* faces;
  const int64_t* edges;        // [E][2]
  const int64_t* ef_off;       // [E + 1] into ef_corner
  const int64_t* ef_corner;    // [H] corners 3 f + k opposite the edge
  const int64_t* ve_off;       // [V + 1] into ve_edge
  const int64_t* ve_edge;      // [2 E]
  const int64_t* vf_off;       // [V + 1] into vf_corner
  const int64_t* vf_corner;    // [NC]
  const int64_t* corner_edge;  // [3 F]
  int64_t H, NC;
  int V, F, E;
  int cot, do_e, do_l, do_n;
  float target;
  float ce, cl;                // w_e / E (0 when E = 0), w_l / V
  float* cotw;                 // [3 F]
  float* erec;                 // [E][MR_EREC]
  float* lrec;                 // [V][MR_LREC]
  float* part;                 // [max(E, V)][MR_COLS]
  const float* scal;           // [1]: w_n / P (0 when P = 0), written by the last reducer launch
  float* grad;                 // [V][3]
};

DEV void mr_load(const MrArgs& a, int64_t i, float (&x)[3]) {
  x[0] = a.verts[3 * i]; x[1] = a.verts[3 * i + 1]; x[2] = a.verts[3 * i + 2];
}
DEV void mr_cross(const float (&u)[3], const float (&v)[3], float (&o)[3]) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
DEV float mr_dot(const float (&u)[3], const float (&v)[3]) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// face f takes part: its indices, all in [0, V) and pairwise different
DEV bool mr_face(const MrArgs& a, int64_t f, int64_t (&i)[3]) {
  if (f < 0 || f >= a.F) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) i[k] = a.faces[3 * f + k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (i[k] < 0 || i[k] >= a.V) return false;
  return i[0] != i[1] && i[0] != i[2] && i[1] != i[2];
}

// edge e: 0 <= e < E and 0 <= ea < eb < V
DEV bool mr_edge(const MrArgs& a, int64_t e, int64_t& ea, int64_t& eb) {
  if (e < 0 || e >= a.E) return false;
  ea = a.edges[2 * e]; eb = a.edges[2 * e + 1];
  return ea >= 0 && ea < eb && eb < a.V;
}

// list entry c is a corner of a face taking part whose opposite edge is (ea, eb); opp = the corner's vertex
DEV bool mr_entry(const MrArgs& a, int64_t c, int64_t ea, int64_t eb, int64_t& opp) {
  if (c < 0 || c >= 3 * (int64_t)a.F) return false;
  int64_t i[3];
  const int64_t f = c / 3;
  if (!mr_face(a, f, i)) return false;
  const int k = (int)(c - 3 * f);
  const int64_t p = k == 0 ? i[1] : i[0], q = k == 2 ? i[1] : i[2];
  opp = k == 0 ? i[0] : k == 1 ? i[1] : i[2];
  return (p < q ? p : q) == ea && (p < q ? q : p) == eb;
}

DEV void mr_range(const int64_t* off, int64_t i, int64_t n, int64_t& b, int64_t& e) {  // clamped into [0, n], e >= b
  b = min(max(off[i], (int64_t)0), n);
  e = min(max(off[i + 1], b), n);
}

// the pair on edge (a, b) with the opposite vertices c, d: val = 1 - cos and its gradient with respect to the four points;
// n0 = (b - a) x (c - a), n1 = -(b - a) x (d - a), cos = n0 . n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)), a floor taken is a constant
DEV void mr_pair(const float (&xa)[3], const float (&xb)[3], const float (&xc)[3], const float (&xd)[3], float& val, float (&ga)[3],
                 float (&gb)[3], float (&gc)[3], float (&gd)[3]) {
  float e[3], p[3], q[3], n0[3], n1[3], G0[3], G1[3], t0[3], t1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { e[k] = xb[k] - xa[k]; p[k] = xc[k] - xa[k]; q[k] = xd[k] - xa[k]; }
  mr_cross(e, p, n0);
  mr_cross(q, e, n1);
  const float len0 = sqrtf(mr_dot(n0, n0)), len1 = sqrtf(mr_dot(n1, n1));
  const float l0 = fmaxf(len0, MR_NRM_FLOOR), l1 = fmaxf(len1, MR_NRM_FLOOR);
  const float cs = mr_dot(n0, n1) / (l0 * l1);
  val = 1.f - cs;
  const float k0 = len0 > MR_NRM_FLOOR ? cs / l0 : 0.f, k1 = len1 > MR_NRM_FLOOR ? cs / l1 : 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // G = -d cos / d n
    G0[k] = -(n1[k] / l1 - k0 * n0[k]) / l0;
    G1[k] = -(n0[k] / l0 - k1 * n1[k]) / l1;
  }
  mr_cross(p, G0, t0);  // d / d e of G0 . (e x p)
  mr_cross(G1, q, t1);  // d / d e of G1 . (q x e)
  mr_cross(G0, e, gc);  // d / d p
  mr_cross(e, G1, gd);  // d / d q
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gb[k] = t0[k] + t1[k];
    ga[k] = -((gb[k] + gc[k]) + gd[k]);
  }
}

// ---- per face: the cotangents (cot only) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mr_face(const MrArgs a) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  float ct[3] = {0.f, 0.f, 0.f};
  int64_t i[3];
  if (mr_face(a, f, i)) {
    float x0[3], x1[3], x2[3], d[3];
    mr_load(a, i[0], x0); mr_load(a, i[1], x1); mr_load(a, i[2], x2);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = x1[k] - x2[k];
    const float A2 = mr_dot(d, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = x0[k] - x2[k];
    const float B2 = mr_dot(d, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = x0[k] - x1[k];
    const float C2 = mr_dot(d, d);
    const float A = sqrtf(A2), B = sqrtf(B2), C = sqrtf(C2);
    const float s = 0.5f * ((A + B) + C);
    const float area = fmaxf(sqrtf(fmaxf(s * (s - A) * (s - B) * (s - C), 0.f)), MR_AREA_FLOOR);
    const float den = 4.f * area;
    ct[0] = ((B2 + C2) - A2) / den;
    ct[1] = ((A2 + C2) - B2) / den;
    ct[2] = ((A2 + B2) - C2) / den;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) a.cotw[3 * f + k] = ct[k];
}

// ---- per edge ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mr_edge(const MrArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  float rec[MR_EREC];
#pragma unroll
  for (int k = 0; k < MR_EREC; ++k) rec[k] = 0.f;
  float lt = 0.f, nt = 0.f;
  int pairs = 0;
  int64_t ea, eb;
  if (mr_edge(a, e, ea, eb)) {
    float xa[3], xb[3];
    mr_load(a, ea, xa); mr_load(a, eb, xb);
    if (a.do_e) {
      float d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = xa[k] - xb[k];
      const float len = sqrtf(mr_dot(d, d));
      const float diff = len - a.target;
      lt = diff * diff;
      const float g = len > 0.f ? 2.f * diff / len : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[k] = g * d[k];
    }
    if (a.do_n || (a.cot && a.do_l)) {
      int64_t rb, re;
      mr_range(a.ef_off, e, a.H, rb, re);
      float w = 0.f;
      for (int64_t i = rb; i < re; ++i) {
        const int64_t ci = a.ef_corner[i];
        int64_t oi;
        if (!mr_entry(a, ci, ea, eb, oi)) continue;
        if (a.cot && a.do_l) w += a.cotw[ci];
        if (!a.do_n) continue;
        float xc[3];
        mr_load(a, oi, xc);
        for (int64_t j = i + 1; j < re; ++j) {
          const int64_t cj = a.ef_corner[j];
          int64_t oj;
          if (cj == ci || !mr_entry(a, cj, ea, eb, oj)) continue;  // (a corner a malformed list repeats pairs with nothing, as in the gather)
          float xd[3], val, ga[3], gb[3], gc[3], gd[3];
          mr_load(a, oj, xd);
          mr_pair(xa, xb, xc, xd, val, ga, gb, gc, gd);
          nt += val;
          pairs += 1;
#pragma unroll
          for (int k = 0; k < 3; ++k) { rec[3 + k] += ga[k]; rec[6 + k] += gb[k]; }
        }
      }
      rec[9] = w;
    }
  }
  float* out = a.erec + (size_t)e * MR_EREC;
#pragma unroll
  for (int k = 0; k < MR_EREC; ++k) out[k] = rec[k];
  float* p = a.part + (size_t)e * MR_COLS;
  p[0] = lt; p[2] = nt; p[3] = __int_as_float(pairs);
}

// vertex v's entry k of the ve list: the edge, its other end j and its weight; false when the entry adds nothing
DEV bool mr_neighbour(const MrArgs& a, int v, int64_t k, int64_t& e, int64_t& j, bool& is_a) {
  e = a.ve_edge[k];
  int64_t ea, eb;
  if (!mr_edge(a, e, ea, eb)) return false;
  is_a = ea == v;
  if (!is_a && eb != v) return false;
  j = is_a ? eb : ea;
  return true;
}

// ---- per vertex: the Laplacian -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mr_lap(const MrArgs a) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  int64_t rb, re;
  mr_range(a.ve_off, v, 2 * (int64_t)a.E, rb, re);
  float sx[3] = {0.f, 0.f, 0.f}, s = 0.f;
  int deg = 0;
  for (int64_t k = rb; k < re; ++k) {
    int64_t e, j;
    bool is_a;
    if (!mr_neighbour(a, v, k, e, j, is_a)) continue;
    const float w = a.cot ? a.erec[(size_t)e * MR_EREC + 9] : 1.f;
    float xj[3];
    mr_load(a, j, xj);
#pragma unroll
    for (int c = 0; c < 3; ++c) sx[c] += w * xj[c];
    s += w;
    deg += 1;
  }
  float r[3] = {0.f, 0.f, 0.f}, n = 0.f;
  if (deg > 0) {  // a vertex without neighbours: r = 0
    float xv[3];
    mr_load(a, v, xv);
    n = a.cot ? (s > 0.f ? 1.f / s : s) : 1.f / (float)deg;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = sx[c] * n - xv[c];
  }
  const float len = sqrtf(mr_dot(r, r));
  float* o = a.lrec + (size_t)v * MR_LREC;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = len > 0.f ? r[c] / len : 0.f;
    o[c] = u;
    o[3 + c] = n * u;
  }
  a.part[(size_t)v * MR_COLS + 1] = len;
}

// ---- the reducer -------------------------------------------------------------------------------------------------------
struct MrFinal {
  float* values;  // [4] total, L_e, L_l, L_n; NULL: this launch writes chunk sums
  float* scal;    // [1] w_n / P
  float we, wl, wn;
  int V, E;
};

// rows [n_e) hold columns 0, 2, 3 and rows [n_v) column 1 (the first launch: the edges' and the vertices' rows of one array;
// later launches: n_e = n_v = the number of chunk sums)
__global__ void __launch_bounds__(256) k_mr_reduce(const float* __restrict__ part, int n_e, int n_v, float* __restrict__ out,
                                                   const MrFinal fin) {
  __shared__ float s_wave[4][MR_COLS];
  __shared__ float s_sum[MR_COLS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t base = (int64_t)blockIdx.x * MR_CHUNK;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  int s3 = 0;
  for (int j = tid; j < MR_CHUNK; j += 256) {
    const int64_t i = base + j;
    const float* r = part + (size_t)i * MR_COLS;
    if (i < n_e) { s0 += r[0]; s2 += r[2]; s3 += __float_as_int(r[3]); }
    if (i < n_v) s1 += r[1];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s0 += __shfl_xor(s0, m); s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); s3 += __shfl_xor(s3, m);
  }
  if (lane == 0) { s_wave[wave][0] = s0; s_wave[wave][1] = s1; s_wave[wave][2] = s2; s_wave[wave][3] = __int_as_float(s3); }
  __syncthreads();
  if (tid < MR_COLS) {
    float v;
    if (tid == 3) v = __int_as_float(((__float_as_int(s_wave[0][3]) + __float_as_int(s_wave[1][3])) + __float_as_int(s_wave[2][3])) +
                                     __float_as_int(s_wave[3][3]));
    else v = ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid];
    if (fin.values) s_sum[tid] = v;
    else out[(size_t)blockIdx.x * MR_COLS + tid] = v;
  }
  if (!fin.values) return;  // (uniform over the workgroup)
  __syncthreads();
  if (tid != 0) return;
  const int P = __float_as_int(s_sum[3]);
  const float Le = fin.E > 0 ? s_sum[0] / (float)fin.E : 0.f;
  const float Ll = s_sum[1] / (float)fin.V;
  const float Ln = P > 0 ? s_sum[2] / (float)P : 0.f;
  fin.values[0] = (fin.we * Le + fin.wl * Ll) + fin.wn * Ln;
  fin.values[1] = Le; fin.values[2] = Ll; fin.values[3] = Ln;
  fin.scal[0] = P > 0 ? fin.wn / (float)P : 0.f;
}

// ---- per vertex: the gather --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mr_gather(const MrArgs a) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  float ge[3] = {0.f, 0.f, 0.f}, gl[3] = {0.f, 0.f, 0.f}, gn[3] = {0.f, 0.f, 0.f};
  int64_t rb, re;
  mr_range(a.ve_off, v, 2 * (int64_t)a.E, rb, re);
  for (int64_t k = rb; k < re; ++k) {
    int64_t e, j;
    bool is_a;
    if (!mr_neighbour(a, v, k, e, j, is_a)) continue;
    const float* rec = a.erec + (size_t)e * MR_EREC;
    if (a.do_e) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ge[c] += is_a ? rec[c] : -rec[c];
    }
    if (a.do_n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gn[c] += is_a ? rec[3 + c] : rec[6 + c];
    }
    if (a.do_l) {
      const float w = a.cot ? rec[9] : 1.f;
      const float* q = a.lrec + (size_t)j * MR_LREC + 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) gl[c] += w * q[c];
    }
  }
  if (a.do_l) {
    const float* u = a.lrec + (size_t)v * MR_LREC;
#pragma unroll
    for (int c = 0; c < 3; ++c) gl[c] -= u[c];
  }
  if (a.do_n) {  // the pairs in which v is the vertex opposite the shared edge
    float xv[3];
    mr_load(a, v, xv);
    mr_range(a.vf_off, v, a.NC, rb, re);
    for (int64_t k = rb; k < re; ++k) {
      const int64_t c = a.vf_corner[k];
      if (c < 0 || c >= 3 * (int64_t)a.F || a.faces[c] != v) continue;
      const int64_t e = a.corner_edge[c];
      int64_t ea, eb, opp;
      if (!mr_edge(a, e, ea, eb) || !mr_entry(a, c, ea, eb, opp)) continue;
      float xa[3], xb[3];
      mr_load(a, ea, xa); mr_load(a, eb, xb);
      int64_t pb, pe;
      mr_range(a.ef_off, e, a.H, pb, pe);
      for (int64_t i = pb; i < pe; ++i) {
        const int64_t ci = a.ef_corner[i];
        int64_t oi;
        if (ci == c || !mr_entry(a, ci, ea, eb, oi)) continue;
        float xd[3], val, ga[3], gb[3], gc[3], gd[3];
        mr_load(a, oi, xd);
        mr_pair(xa, xb, xv, xd, val, ga, gb, gc, gd);
#pragma unroll
        for (int d = 0; d < 3; ++d) gn[d] += gc[d];
      }
    }
  }
  const float cn = a.do_n ? a.scal[0] : 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.grad[3 * (size_t)v + c] = (a.ce * ge[c] + a.cl * gl[c]) + cn * gn[c];
}

}  // namespace reni

namespace {

size_t mr_align(size_t n) { return (n + 255) & ~(size_t)255; }
size_t mr_part_floats(int64_t N) {  // the first array [N][MR_COLS] and every later level's chunk sums
  size_t total = (size_t)N * reni::MR_COLS;
  for (int64_t n = (N + reni::MR_CHUNK - 1) / reni::MR_CHUNK; n > 1; n = (n + reni::MR_CHUNK - 1) / reni::MR_CHUNK)
    total += (size_t)n * reni::MR_COLS;
  return total;
}
size_t mr_cot_bytes(int64_t F) { return mr_align((size_t)F * 3 * sizeof(float)); }
size_t mr_erec_bytes(int64_t E) { return mr_align((size_t)E * reni::MR_EREC * sizeof(float)); }
size_t mr_lrec_bytes(int64_t V) { return mr_align((size_t)V * reni::MR_LREC * sizeof(float)); }
size_t mr_part_bytes(int64_t V, int64_t E) { return mr_align(mr_part_floats(V > E ? V : E) * sizeof(float)); }
size_t mr_need(int64_t V, int64_t F, int64_t E) {
  return mr_cot_bytes(F) + mr_erec_bytes(E) + mr_lrec_bytes(V) + mr_part_bytes(V, E) + 256;
}
bool mr_sizes_ok(int64_t V, int64_t F, int64_t E) {
  return !(V < 1 || F < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS || E < 0 || E > MESH_MAX_ELEMS);
}
bool mr_weight_ok(float w) { return w >= 0.f && isfinite(w); }

}  // namespace

extern "C" {

size_t reni_mesh_regularizers_workspace_bytes(int64_t V, int64_t F, int64_t E) {
  return mr_sizes_ok(V, F, E) ? mr_need(V, F, E) : 0;
}

int reni_mesh_regularizers(int64_t V, int64_t F, int64_t E, int64_t H, int64_t NC, const float* verts, const int64_t* faces,
                           const int64_t* edges, const int64_t* ef_offsets, const int64_t* ef_corners, const int64_t* ve_offsets,
                           const int64_t* ve_edges, const int64_t* vf_offsets, const int64_t* vf_corners,
                           const int64_t* corner_edges, float w_edge, float w_laplacian, float w_normal, float target_length,
                           int32_t method, float* values, float* grad_verts, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "mesh regularizers";
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (E < 0 || E > MESH_MAX_ELEMS || H < 0 || H > 3 * F || NC < 0 || NC > 3 * F) return tu_fail(RENI_EINVAL, who, "bad E / H / NC");
  if (!verts || !faces || !edges || !ef_offsets || !ef_corners || !ve_offsets || !ve_edges || !vf_offsets || !vf_corners ||
      !corner_edges || !values)
    return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (!mr_weight_ok(w_edge) || !mr_weight_ok(w_laplacian) || !mr_weight_ok(w_normal))
    return tu_fail(RENI_EINVAL, who, "the weights must be >= 0 and finite");
  if (!mr_weight_ok(target_length)) return tu_fail(RENI_EINVAL, who, "target_length must be >= 0 and finite");
  if (method != RENI_LAPLACIAN_UNIFORM && method != RENI_LAPLACIAN_COT)
    return tu_fail(RENI_EINVAL, who, "method must be RENI_LAPLACIAN_UNIFORM or RENI_LAPLACIAN_COT");
  if (int rc = tu_check_ws(who, ws, ws_bytes, mr_need(V, F, E))) return rc;
  hipStream_t s = (hipStream_t)stream;
  reni::MrArgs a;
  a.verts = verts; a.faces = faces; a.edges = edges; a.ef_off = ef_offsets; a.ef_corner = ef_corners; a.ve_off = ve_offsets;
  a.ve_edge = ve_edges; a.vf_off = vf_offsets; a.vf_corner = vf_corners; a.corner_edge = corner_edges;
  a.H = H; a.NC = NC; a.V = (int)V; a.F = (int)F; a.E = (int)E;
  a.cot = method == RENI_LAPLACIAN_COT; a.do_e = w_edge > 0.f; a.do_l = w_laplacian > 0.f; a.do_n = w_normal > 0.f;
  a.target = target_length;
  a.ce = E > 0 ? w_edge / (float)E : 0.f;
  a.cl = w_laplacian / (float)V;
  char* p = (char*)ws;
  a.cotw = (float*)p; p += mr_cot_bytes(F);
  a.erec = (float*)p; p += mr_erec_bytes(E);
  a.lrec = (float*)p; p += mr_lrec_bytes(V);
  a.part = (float*)p; p += mr_part_bytes(V, E);  // behind it, the block's last 256 bytes: scal
  float* scal = (float*)p;
  a.scal = scal;
  a.grad = grad_verts;
  const bool edge_pass = E > 0 && (a.do_e || a.do_n || (a.cot && a.do_l));
  if (a.cot && a.do_l && E > 0)
    if (int rc = tu_launch(TU_PLAIN, reni::k_mr_face, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, a)) return rc;
  if (edge_pass)
    if (int rc = tu_launch(TU_PLAIN, reni::k_mr_edge, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, a)) return rc;
  if (a.do_l)
    if (int rc = tu_launch(TU_PLAIN, reni::k_mr_lap, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, a)) return rc;
  // rows the passes above did not write are not read: n_e / n_v are 0 for a pass that did not run
  int64_t n_e = edge_pass ? E : 0, n_v = a.do_l ? V : 0;
  const float* src = a.part;
  float* dst = a.part + (size_t)(V > E ? V : E) * reni::MR_COLS;
  for (;;) {
    const int64_t n = n_e > n_v ? n_e : n_v;
    const int64_t chunks = n > 0 ? (n + reni::MR_CHUNK - 1) / reni::MR_CHUNK : 1;
    reni::MrFinal fin;
    fin.values = chunks == 1 ? values : nullptr; fin.scal = scal;
    fin.we = w_edge; fin.wl = w_laplacian; fin.wn = w_normal; fin.V = (int)V; fin.E = (int)E;
    if (int rc = tu_launch(TU_PLAIN, reni::k_mr_reduce, dim3((unsigned)chunks), dim3(256), 0, s, src, (int)n_e, (int)n_v, dst, fin))
      return rc;
    if (chunks == 1) break;
    src = dst; dst += (size_t)chunks * reni::MR_COLS; n_e = n_v = chunks;
  }
  if (!grad_verts) return RENI_OK;
  return tu_launch(TU_PLAIN, reni::k_mr_gather, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, a);
}

}  // extern "C"
