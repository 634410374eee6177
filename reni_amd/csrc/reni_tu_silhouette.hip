// translation unit of libreni_hip.so: the soft silhouette of a mesh (a differentiable coverage mask, as SoftRas and pytorch3d's
// SoftSilhouetteShader) and its gradient with respect to the vertex positions -- the gradient that moves the outline, which the
// G-buffer backward (reni_tu_raster_bwd.hip) holds fixed.
//
// Definitions (include/reni_hip.h has them in full).  Camera, projection, pixel grid: reni_rasterize_mesh's (reni_mesh.inc).  A
// face TAKES PART iff mesh_face keeps it, all three view z are > 0 and its projected corners are finite.  For such a face and
// pixel centre p: c = the nearest point of the triangle's boundary, over the edges (0,1), (0,2), (1,2) in this order,
// c_e = a + t (b - a), t = clamp((b-a).(p-a) / |b-a|^2, 0, 1) (|b-a|^2 <= 1e-8: c_e = b, t = 1), the first edge with the
// strictly smallest |c_e - p|^2 wins; inside <=> w0, w1, w2 > 0 (mesh_bary); d = |c - p|^2, sd = -d inside, +d outside; the
// face takes part AT p iff inside or d < blur_radius; prob = 1 / (1 + exp(sd / sigma)); trans_p = prod (1 - prob) over the faces
// taking part at p in ascending face order from 1.0f; alpha_p = 1 - trans_p.  Every face near the pixel enters (no K-nearest cut).
// Gradient of sum_p gA_p alpha_p with membership, inside, the winning edge and a clamped t held constant:
// d alpha_p / d sd_f = -trans_p prob_f / sigma (no division by 1 - prob_f), d sd / da = 2 s (1 - t)(c - p), d sd / db = 2 s t (c - p),
// s = -1 inside, +1 outside; NDC -> view -> world as k_gb_face.  fp32, no float atomic: every sum and product has one fixed
// order, two calls give identical bits.  Four kernels:
//
//   k_sil_setup    one thread per face: a 64-byte record (NDC corners, view z, the taking-part flag) and the NDC box grown by
//                  sqrt(blur_radius) (and a rounding slack, SIL_GROW_*: the box only has to hold every pixel with d < r); empty
//                  for a face that does not take part.
//   k_sil_tile     one workgroup per 16 x 16 tile, built like k_raster_tile: the grown boxes stream through in chunks of 256
//                  against the tile's pixel-centre extent, the overlapping faces are compacted in ascending order (ballot +
//                  popcount prefix, then the waves' counts) and staged in LDS; every lane walks the list (LDS broadcast reads),
//                  computes sd and prob for the faces whose box holds its pixel and multiplies.  Writes alpha and trans.
//   k_sil_face     one wave64 per face.  The lanes walk the pixels of the face's grown box, clipped to the image, in row-major
//                  order with stride 64; each recomputes membership, c, t and prob with the forward's own functions (sil_in_box,
//                  sil_pair, sil_prob), reads trans_p and gA_p and accumulates the six NDC corner gradients.  A butterfly of
//                  shuffles adds the lanes in one fixed order; lane 0 takes (x, y) -> q -> p and writes 9 floats per face.
//   k_sil_vertex   one thread per vertex gathers its corners' records in ascending order through the vertex -> (face, corner)
//                  list (ops.vertex_face_lists).
//
// The nearest-point walk is this unit's own (sil_nearest): the rasteriser's point_line_dist2 returns the distance alone, the
// silhouette needs c and t beside it, so nothing of reni_tu_raster.hip moves and its emitted code stays what it was.
// exp is expf, not the bare hardware exponential: the tests' error bound is derived with a correctly rounded exp.
// reni_soft_silhouette_backward_camera adds the gradient with respect to the camera (R, T, tan_half_fov): k_sil_face<true>
// stores a camera record per face, the reducer of reni_tu_camera.hip adds them; without grad_verts k_sil_vertex is not launched.
// Malformed input adds nothing and reads nothing out of range: a vertex index outside [0, V) (mesh_face), a list entry outside
// [0, 3F) or one that does not name the vertex, offsets outside their list (mesh_corner_range, mesh_corner_names).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"
#include "reni_mesh.inc"

namespace reni {

constexpr int SIL_TILE = 16;    // pixels per tile side
constexpr int SIL_CHUNK = 256;  // faces per LDS stage (= threads per workgroup)
constexpr int SIL_REC = 9;      // floats per face record of the backward: the gradient of its three corners' positions
// the grown box must hold every pixel whose fp32 d comes out < r: sqrt(r) and a slack far above the rounding of d and the grid
constexpr float SIL_GROW_REL = 1.00001f, SIL_GROW_ABS = 1e-6f;

struct SilRec {   // 64 bytes, read as four float4 (world order of the corners)
  float4 xy01;    // NDC x0 y0 x1 y1
  float4 xy2z01;  // NDC x2 y2, view z0 z1
  float4 z2p;     // view z2, 1 when the face takes part else 0, -, -
  float4 box;     // the grown NDC box xmin xmax ymin ymax; empty (+inf, -inf, +inf, -inf) for a face that does not take part
};

DEV bool sil_in_box(float px, float py, const float4& b) { return px >= b.x && px <= b.y && py >= b.z && py <= b.w; }

// the nearest point c = a + t (b - a) of edge (a, b) to p, and |c - p|^2 (PointLineDistanceForward's rule with c and t kept)
DEV void sil_nearest(float px, float py, float ax, float ay, float bx, float by, float& cx, float& cy, float& t, float& d) {
  const float bax = bx - ax, bay = by - ay;
  const float l2 = bax * bax + bay * bay;
  if (l2 <= MESH_EPS) {
    t = 1.f; cx = bx; cy = by;
  } else {
    t = fminf(fmaxf((bax * (px - ax) + bay * (py - ay)) / l2, 0.f), 1.f);
    cx = ax + t * bax; cy = ay + t * bay;
  }
  const float dx = cx - px, dy = cy - py;
  d = dx * dx + dy * dy;
}

struct SilPair {
  float dx, dy;  // c - p
  float t, d;
  int edge;      // 0: (0,1), 1: (0,2), 2: (1,2)
  bool inside;
};

// pixel p against a taking-part face: true when the face takes part at p (inside, or d < r)
DEV bool sil_pair(float px, float py, float x0, float y0, float x1, float y1, float x2, float y2, float r, SilPair& o) {
  float cx, cy, t, d, cx1, cy1, t1, d1;
  sil_nearest(px, py, x0, y0, x1, y1, cx, cy, t, d);
  int e = 0;
  sil_nearest(px, py, x0, y0, x2, y2, cx1, cy1, t1, d1);
  if (d1 < d) { d = d1; cx = cx1; cy = cy1; t = t1; e = 1; }
  sil_nearest(px, py, x1, y1, x2, y2, cx1, cy1, t1, d1);
  if (d1 < d) { d = d1; cx = cx1; cy = cy1; t = t1; e = 2; }
  const float A = mesh_bary_area(x0, y0, x1, y1, x2, y2);
  float w0, w1, w2;
  mesh_bary(px, py, x0, y0, x1, y1, x2, y2, A, w0, w1, w2);
  o.inside = w0 > 0.f && w1 > 0.f && w2 > 0.f;
  o.dx = cx - px; o.dy = cy - py; o.t = t; o.d = d; o.edge = e;
  return o.inside || d < r;
}

DEV float sil_prob(const SilPair& q, float sigma) { return 1.f / (1.f + expf((q.inside ? -q.d : q.d) / sigma)); }

// ---- face setup --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sil_setup(int V, int F, const float* __restrict__ verts,
                                                   const int64_t* __restrict__ faces, const Camera cam, float grow,
                                                   SilRec* __restrict__ rec) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  float x[3], y[3], z[3], area;
  bool ok = mesh_face(cam, V, verts, faces, (size_t)f, x, y, z, area);
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && z[k] > 0.f && isfinite(x[k]) && isfinite(y[k]);
  SilRec r;
  r.xy01 = float4{x[0], y[0], x[1], y[1]};
  r.xy2z01 = float4{x[2], y[2], z[0], z[1]};
  r.z2p = float4{z[2], ok ? 1.f : 0.f, 0.f, 0.f};
  if (ok) r.box = float4{fminf(x[0], fminf(x[1], x[2])) - grow, fmaxf(x[0], fmaxf(x[1], x[2])) + grow,
                         fminf(y[0], fminf(y[1], y[2])) - grow, fmaxf(y[0], fmaxf(y[1], y[2])) + grow};
  else r.box = float4{INFINITY, -INFINITY, INFINITY, -INFINITY};
  rec[f] = r;
}

// ---- forward: one tile per workgroup -----------------------------------------------------------------------------------
struct SilArgs {
  const SilRec* rec;
  float* alpha;
  float* trans;
  float sigma, r;
  int F, S;
};

__global__ void __launch_bounds__(256) k_sil_tile(const SilArgs a) {
  __shared__ float4 s_geo[SIL_CHUNK][3];  // the overlapping faces' xy01, xy2z01, box, compacted in ascending face order
  __shared__ int s_wcount[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S;
  const int r = blockIdx.y * SIL_TILE + (wave >> 1) * 8 + (lane >> 3);
  const int c = blockIdx.x * SIL_TILE + (wave & 1) * 8 + (lane & 7);
  const bool live = r < S && c < S;
  const float px = mesh_pix_ndc(S - 1 - c, S), py = mesh_pix_ndc(S - 1 - r, S);
  // the tile's pixel-centre extent (rows / columns beyond the image excluded); x decreases with c, y with r
  const int c_hi = min(S, (int)(blockIdx.x + 1) * SIL_TILE) - 1, r_hi = min(S, (int)(blockIdx.y + 1) * SIL_TILE) - 1;
  const float tx_max = mesh_pix_ndc(S - 1 - blockIdx.x * SIL_TILE, S), tx_min = mesh_pix_ndc(S - 1 - c_hi, S);
  const float ty_max = mesh_pix_ndc(S - 1 - blockIdx.y * SIL_TILE, S), ty_min = mesh_pix_ndc(S - 1 - r_hi, S);

  float trans = 1.f;
  for (int base = 0; base < a.F; base += SIL_CHUNK) {
    const int f = base + tid;
    bool hit = false;
    if (f < a.F) {
      const float4 b = a.rec[f].box;
      hit = b.x <= tx_max && b.y >= tx_min && b.z <= ty_max && b.w >= ty_min;
    }
    const unsigned long long m = __ballot(hit);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcount[wave] = __popcll(m);
    __syncthreads();  // (also: the previous chunk's list is no longer read)
    int slot = before, n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int k = s_wcount[w];
      slot += w < wave ? k : 0;
      n += k;
    }
    if (hit) {  // slot < 256: at most one entry per thread of the chunk
      const SilRec& q = a.rec[f];
      s_geo[slot][0] = q.xy01;
      s_geo[slot][1] = q.xy2z01;
      s_geo[slot][2] = q.box;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float4 box = s_geo[k][2];
      if (!sil_in_box(px, py, box)) continue;
      const float4 g0 = s_geo[k][0], g1 = s_geo[k][1];
      SilPair q;
      if (!sil_pair(px, py, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, a.r, q)) continue;
      trans *= 1.f - sil_prob(q, a.sigma);
    }
  }
  if (!live) return;
  const size_t p = (size_t)r * S + c;
  a.alpha[p] = 1.f - trans;
  a.trans[p] = trans;
}

// ---- backward: per-face reduction --------------------------------------------------------------------------------------
struct SilBwdArgs {
  const SilRec* rec;
  const float* trans;  // [S S] the forward's
  const float* gA;     // [S S]
  float* out;          // [F][SIL_REC]
  Camera cam;
  float sigma, r;
  int F, S;
  // k_sil_face<true> alone: the camera records [F][CAM_REC], and the mesh for the corners' world positions
  float* crec;
  const float* verts;
  const int64_t* faces;
  int V;
};

DEV float sil_wave_sum(float s) {  // all 64 lanes, one fixed order (as gb_wave_sum)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

// the grid index i (counted from +x / +y, mesh_pix_ndc) nearest below / above NDC coordinate v, clamped to [-1, S]
DEV int sil_grid_floor(float v, int S) { return (int)floorf(fminf(fmaxf(((v + 1.f) * (float)S - 1.f) * 0.5f, -1.f), (float)S)); }

// CAM: lane 0 also writes the face's camera record (CAM_REC floats: gR, gT, g_tan; reni_mesh.inc: mesh_camera_record) from
// the NDC gradients and the corners it holds -- no second pixel walk.  <false> is the kernel as it was.
template <bool CAM>
__global__ void __launch_bounds__(256) k_sil_face(const SilBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= a.F) return;  // wave-uniform
  float* out = a.out + (size_t)f * SIL_REC;
  const SilRec& q = a.rec[f];
  const float4 g0 = q.xy01, g1 = q.xy2z01, g2 = q.z2p, box = q.box;
  const int S = a.S;
  // grid indices i = S - 1 - col (x) and S - 1 - row (y) the box can hold, one to spare on both sides; sil_in_box decides
  const int ix_lo = max(sil_grid_floor(box.x, S) - 1, 0), ix_hi = min(sil_grid_floor(box.y, S) + 2, S - 1);
  const int iy_lo = max(sil_grid_floor(box.z, S) - 1, 0), iy_hi = min(sil_grid_floor(box.w, S) + 2, S - 1);
  if (!(g2.y > 0.f) || ix_lo > ix_hi || iy_lo > iy_hi) {  // the face does not take part, or its box holds no pixel
    if (lane < SIL_REC) out[lane] = 0.f;
    if (CAM && lane < CAM_REC) a.crec[(size_t)f * CAM_REC + lane] = 0.f;
    return;
  }
  const float x[3] = {g0.x, g0.z, g1.x}, y[3] = {g0.y, g0.w, g1.y}, z[3] = {g1.z, g1.w, g2.x};
  const int c_lo = S - 1 - ix_hi, r_lo = S - 1 - iy_hi;  // columns c_lo .. c_lo + w - 1, rows r_lo .. r_lo + h - 1, all in [0, S)
  const int w = ix_hi - ix_lo + 1, h = iy_hi - iy_lo + 1;
  const int n = w * h;  // <= S S <= MESH_MAX_ELEMS
  float gx0 = 0.f, gy0 = 0.f, gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f;
  for (int j = lane; j < n; j += 64) {
    const int jr = j / w;
    const int r = r_lo + jr, c = c_lo + (j - jr * w);
    const float px = mesh_pix_ndc(S - 1 - c, S), py = mesh_pix_ndc(S - 1 - r, S);
    if (!sil_in_box(px, py, box)) continue;
    SilPair pr;
    if (!sil_pair(px, py, x[0], y[0], x[1], y[1], x[2], y[2], a.r, pr)) continue;
    const size_t p = (size_t)r * S + c;
    const float prob = sil_prob(pr, a.sigma);
    // gA d alpha / d sd = -gA trans prob / sigma; d sd / d(a, b) = 2 s ((1 - t), t)(c - p)
    const float g = a.gA[p] * (-(a.trans[p] * prob) / a.sigma) * (pr.inside ? -2.f : 2.f);
    const float wa = g * (1.f - pr.t), wb = g * pr.t;
    // edge 0: a = 0, b = 1; edge 1: a = 0, b = 2; edge 2: a = 1, b = 2.  The third corner gets 0.
    const float k0 = pr.edge == 2 ? 0.f : wa;
    const float k1 = pr.edge == 0 ? wb : pr.edge == 2 ? wa : 0.f;
    const float k2 = pr.edge == 0 ? 0.f : wb;
    gx0 += k0 * pr.dx; gy0 += k0 * pr.dy;
    gx1 += k1 * pr.dx; gy1 += k1 * pr.dy;
    gx2 += k2 * pr.dx; gy2 += k2 * pr.dy;
  }
  gx0 = sil_wave_sum(gx0); gy0 = sil_wave_sum(gy0);
  gx1 = sil_wave_sum(gx1); gy1 = sil_wave_sum(gy1);
  gx2 = sil_wave_sum(gx2); gy2 = sil_wave_sum(gy2);
  if (lane != 0) return;
  const float gx[3] = {gx0, gx1, gx2}, gy[3] = {gy0, gy1, gy2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // x = q_x / (q_z t), y = q_y / (q_z t)
    const float wz = z[k] * a.cam.tan_half_fov;
    const float qx = gx[k] / wz, qy = gy[k] / wz, qz = -(gx[k] * x[k] + gy[k] * y[k]) / z[k];
#pragma unroll
    for (int d = 0; d < 3; ++d) out[3 * k + d] = a.cam.R[3 * d] * qx + a.cam.R[3 * d + 1] * qy + a.cam.R[3 * d + 2] * qz;
  }
  // a.crec is never NULL in a <true> launch.  The test is NOT redundant and must stay: it puts the record in a block of its
  // own, which with mesh_opaque keeps grad_verts' bits those of the <false> instance (mesh_camera_record, reni_mesh.inc;
  // only the device's bit-equality tests, tests/test_gpu_camera_grad.py, notice when that is lost).
  if (CAM && a.crec) {
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t i = a.faces[3 * (size_t)f + k];  // in [0, V) for a face that takes part (mesh_face); checked all the same
      const bool ok = i >= 0 && i < a.V;
#pragma unroll
      for (int d = 0; d < 3; ++d) p[k][d] = ok ? a.verts[3 * i + d] : 0.f;
    }
    Camera cam = a.cam;
    cam.tan_half_fov = mesh_opaque(cam.tan_half_fov);
    float tx[3], ty[3], xo[3], yo[3], zo[3];
    mesh_opaque3(gx, tx); mesh_opaque3(gy, ty); mesh_opaque3(x, xo); mesh_opaque3(y, yo); mesh_opaque3(z, zo);
    mesh_camera_record(cam, tx, ty, xo, yo, zo, p, a.crec + (size_t)f * CAM_REC);
  }
}

// ---- backward: per-vertex gather of the face records -------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sil_vertex(const GbMesh m, const float* __restrict__ rec, float* __restrict__ gverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.V) return;
  int64_t b, e;
  mesh_corner_range(m, v, b, e);
  float gd[3] = {0.f, 0.f, 0.f};
  for (int64_t k = b; k < e; ++k) {
    const int64_t c = m.corner[k];
    if (!mesh_corner_names(m, c, v)) continue;
    const float* r = rec + (size_t)c * 3;  // face c / 3, corner c % 3: SIL_REC = 9 floats per face
    gd[0] += r[0]; gd[1] += r[1]; gd[2] += r[2];
  }
  gverts[3 * (size_t)v] = gd[0]; gverts[3 * (size_t)v + 1] = gd[1]; gverts[3 * (size_t)v + 2] = gd[2];
}

}  // namespace reni

namespace {

size_t sil_rec_bytes(int64_t F) { return ((size_t)F * sizeof(reni::SilRec) + 255) & ~(size_t)255; }
size_t sil_grad_bytes(int64_t F) { return ((size_t)F * reni::SIL_REC * sizeof(float) + 255) & ~(size_t)255; }

int sil_check_blur(const char* who, float sigma, float blur_radius) {
  if (!(sigma > 0.f) || !isfinite(sigma)) return tu_fail(RENI_EINVAL, who, "sigma must be positive and finite");
  if (!(blur_radius >= 0.f) || !isfinite(blur_radius)) return tu_fail(RENI_EINVAL, who, "blur_radius must be >= 0 and finite");
  return RENI_OK;
}

int sil_setup(int64_t V, int64_t F, const float* verts, const int64_t* faces, const reni::Camera& cam, float blur_radius,
              reni::SilRec* rec, hipStream_t s) {
  const float grow = sqrtf(blur_radius) * reni::SIL_GROW_REL + reni::SIL_GROW_ABS;
  return tu_launch(TU_PLAIN, reni::k_sil_setup, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, (int)V, (int)F, verts, faces, cam,
                   grow, rec);
}

// the camera records [F][CAM_REC] and, behind them, the reducer's chunk sums
size_t sil_cam_rec_bytes(int64_t F) { return ((size_t)F * reni::CAM_REC * sizeof(float) + 255) & ~(size_t)255; }
size_t sil_cam_bytes(int64_t F) { return sil_cam_rec_bytes(F) + ((reni::camera_part_floats(F) * sizeof(float) + 255) & ~(size_t)255); }

// reni_soft_silhouette_backward (camera false: grad_camera is not looked at, today's checks and launches) and
// reni_soft_silhouette_backward_camera (camera true: grad_verts and the vertex lists are optional, together)
int sil_backward(const char* who, bool camera, int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R,
                 const float* T, float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius, const float* trans,
                 const float* grad_alpha, const int64_t* vf_offsets, const int64_t* vf_corners, float* grad_verts,
                 float* grad_camera, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (int rc = mesh_check_image(who, H, W)) return rc;
  if (camera && !grad_verts && !grad_camera) return tu_fail(RENI_EINVAL, who, "grad_verts and grad_camera are both NULL");
  if (camera && !grad_camera)
    return tu_fail(RENI_EINVAL, who, "NULL grad_camera (reni_soft_silhouette_backward computes grad_verts alone)");
  const bool need_verts = !camera || grad_verts;
  if (!verts || !faces || !R || !T || !trans || !grad_alpha || (need_verts && (!vf_offsets || !vf_corners || !grad_verts)))
    return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = mesh_check_fov(who, tan_half_fov)) return rc;
  if (int rc = sil_check_blur(who, sigma, blur_radius)) return rc;
  const size_t base = sil_rec_bytes(F) + sil_grad_bytes(F);
  if (int rc = tu_check_ws(who, ws, ws_bytes, base + (camera ? sil_cam_bytes(F) : 0))) return rc;
  hipStream_t s = (hipStream_t)stream;
  reni::SilBwdArgs a;
  a.cam = mesh_camera(R, T, tan_half_fov);
  reni::SilRec* rec = (reni::SilRec*)ws;
  if (int rc = sil_setup(V, F, verts, faces, a.cam, blur_radius, rec, s)) return rc;
  a.rec = rec; a.trans = trans; a.gA = grad_alpha; a.out = (float*)((char*)ws + sil_rec_bytes(F));
  a.sigma = sigma; a.r = blur_radius; a.F = (int)F; a.S = (int)H;
  a.crec = camera ? (float*)((char*)ws + base) : nullptr;
  a.verts = verts; a.faces = faces; a.V = (int)V;
  const auto k = camera ? reni::k_sil_face<true> : reni::k_sil_face<false>;
  if (int rc = tu_launch(TU_PLAIN, k, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, s, a)) return rc;
  if (camera)
    if (int rc = reni::launch_camera_reduce(a.crec, F, (float*)((char*)a.crec + sil_cam_rec_bytes(F)), grad_camera, s)) return rc;
  if (!need_verts) return RENI_OK;  // the mesh is known and only the pose is fitted: no vertex kernel, no list
  const reni::GbMesh m{verts, faces, vf_offsets, vf_corners, (int)V, (int)F};
  return tu_launch(TU_PLAIN, reni::k_sil_vertex, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, m, (const float*)a.out,
                   grad_verts);
}

}  // namespace

extern "C" {

size_t reni_soft_silhouette_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return sil_rec_bytes(F) + 256;
}

int reni_soft_silhouette(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R, const float* T,
                         float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius, float* alpha, float* trans,
                         void* ws, size_t ws_bytes, void* stream) {
  const char* who = "soft silhouette";
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (int rc = mesh_check_image(who, H, W)) return rc;
  if (!verts || !faces || !R || !T || !alpha || !trans) return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = mesh_check_fov(who, tan_half_fov)) return rc;
  if (int rc = sil_check_blur(who, sigma, blur_radius)) return rc;
  if (int rc = tu_check_ws(who, ws, ws_bytes, sil_rec_bytes(F))) return rc;
  hipStream_t s = (hipStream_t)stream;
  reni::SilRec* rec = (reni::SilRec*)ws;
  if (int rc = sil_setup(V, F, verts, faces, mesh_camera(R, T, tan_half_fov), blur_radius, rec, s)) return rc;
  reni::SilArgs a;
  a.rec = rec; a.alpha = alpha; a.trans = trans; a.sigma = sigma; a.r = blur_radius; a.F = (int)F; a.S = (int)H;
  const unsigned tiles = (unsigned)((H + reni::SIL_TILE - 1) / reni::SIL_TILE);
  return tu_launch(TU_PLAIN, reni::k_sil_tile, dim3(tiles, tiles), dim3(256), 0, s, a);
}

size_t reni_soft_silhouette_backward_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return sil_rec_bytes(F) + sil_grad_bytes(F) + 256;
}

int reni_soft_silhouette_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R, const float* T,
                                  float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius, const float* trans,
                                  const float* grad_alpha, const int64_t* vf_offsets, const int64_t* vf_corners,
                                  float* grad_verts, void* ws, size_t ws_bytes, void* stream) {
  return sil_backward("soft silhouette backward", false, V, F, verts, faces, R, T, tan_half_fov, H, W, sigma, blur_radius, trans,
                      grad_alpha, vf_offsets, vf_corners, grad_verts, nullptr, ws, ws_bytes, stream);
}

size_t reni_soft_silhouette_backward_camera_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return sil_rec_bytes(F) + sil_grad_bytes(F) + sil_cam_bytes(F) + 256;
}

int reni_soft_silhouette_backward_camera(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R,
                                         const float* T, float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius,
                                         const float* trans, const float* grad_alpha, const int64_t* vf_offsets,
                                         const int64_t* vf_corners, float* grad_verts, float* grad_camera, void* ws, size_t ws_bytes,
                                         void* stream) {
  return sil_backward("soft silhouette backward camera", true, V, F, verts, faces, R, T, tan_half_fov, H, W, sigma, blur_radius,
                      trans, grad_alpha, vf_offsets, vf_corners, grad_verts, grad_camera, ws, ws_bytes, stream);
}

}  // extern "C"
