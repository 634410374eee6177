// translation unit of libreni_hip.so: the backward of the mesh G-buffer (reni_tu_raster.hip), from the gradients of the pixel
// normals and pixel positions to the vertex positions, with the rasteriser's face assignment held fixed.
//
// Definitions (include/reni_hip.h has them in full): q = p R + T, x = q_x / (q_z t), y = q_y / (q_z t); for pixel (px, py) on
// face (i0, i1, i2): A = E(v2, v0, v1) + 1e-8, w0 = E(p, 1, 2) / A, w1 = E(p, 2, 0) / A, w2 = E(p, 0, 1) / A;
// N_p = sum_k w_k n_ik, X_p = sum_k w_k p_ik; n_v = u_v / max(|u_v|, 1e-6), u_v = sum over the corners (f, k) that name v of
// cross(p_f1 - p_f0, p_f2 - p_f0).  Computed: g_verts = d/dp sum_p (gN_p . N_p + gX_p . X_p).  fp32, no float atomic: every
// sum has one fixed order, two calls give identical bits.  Three kernels:
//
//   k_gb_face      one wave64 per face.  The face's pixels come from a sorted list (a stable sort of pix_to_face); the lanes
//                  walk it with stride 64, each recomputing its pixel's weights from the projected corners with the forward's
//                  own functions (reni_mesh.inc: mesh_face, mesh_bary), and sum 25 partials: w_k gN (9), w_k gX (9), the NDC gradients of the three corners through the
//                  edge functions (6) and d loss / dA (1).  A butterfly of shuffles adds the lanes in one fixed order; lane 0
//                  folds dA into the corners, takes (x, y) -> q -> p and writes the face's record: per corner the sum
//                  w_k gN (for the vertex normal) and the gradient of the corner's position (direct + projection).
//   k_gb_vertex    one thread per vertex gathers its corners' records in ascending order through the vertex -> (face, corner)
//                  list: the direct part of g_verts, and g n_v, turned into g u_v (normalisation's Jacobian; I 1e6 in the
//                  max branch).
//   k_vn_bwd       one thread per vertex, over its faces ascending: G_f = g u_f0 + g u_f1 + g u_f2, a = p_f1 - p_f0,
//                  b = p_f2 - p_f0; corner 1 gets b x G_f, corner 2 G_f x a, corner 0 minus both.  <true>: g u read from the
//                  workspace (the G-buffer backward); <false>: recomputed from g n on the fly (reni_mesh_vertex_normals_backward,
//                  which has no workspace; the thread's own vertex once), the same arithmetic; u_v is mesh_u, the sum
//                  k_vertex_normals normalises.
//
// reni_gbuffer_backward_camera adds the gradient with respect to the camera (R, T, tan_half_fov; the barycentric path alone):
// k_gb_face<true> stores a camera record per face, the reducer of reni_tu_camera.hip adds them; without grad_verts k_gb_vertex
// and k_vn_bwd are not launched.
// Malformed input adds nothing and reads nothing out of range: a vertex index outside [0, V), a list entry outside [0, 3F) or
// one that does not name the vertex, offsets outside their list, a pixel entry outside [0, S S) or one whose pix_to_face is
// not the face, a face that k_face_setup skips (it has no pixel in a real pix_to_face).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"
#include "reni_mesh.inc"

namespace reni {

constexpr int GB_REC = 18;  // floats per face record: per corner (sum w_k gN [3], g position [3])

struct GbArgs {
  const float* verts;
  const float* vnrm;
  const int64_t* faces;
  const int64_t* p2f;
  const int64_t* foff;   // [F + 1] offsets into flist
  const int64_t* flist;  // [S S] pixels sorted by face
  const float* gN;       // [S S][3] or NULL
  const float* gX;       // [S S][3] or NULL
  float* rec;            // [F][GB_REC]
  Camera cam;
  int V, F, S;
  float* crec;           // [F][CAM_REC], k_gb_face<true> alone
};

DEV float gb_wave_sum(float s) {  // all 64 lanes, one fixed order
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

// ---- per-face reduction ------------------------------------------------------------------------------------------------
// CAM: lane 0 also writes the face's camera record (CAM_REC floats: gR, gT, g_tan; reni_mesh.inc: mesh_camera_record) from
// the NDC gradients and the corners it holds -- no second pixel walk.  <false> is the kernel as it was.
template <bool CAM>
__global__ void __launch_bounds__(256) k_gb_face(const GbArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= a.F) return;  // wave-uniform
  float* out = a.rec + (size_t)f * GB_REC;
  const int64_t P = (int64_t)a.S * a.S;
  float x[3], y[3], z[3], area;
  const bool ok = mesh_face(a.cam, a.V, a.verts, a.faces, (size_t)f, x, y, z, area);  // k_face_setup's corners and its rule
  const int64_t b = min(max(a.foff[f], (int64_t)0), P), e = min(max(a.foff[f + 1], b), P);
  if (!ok || b == e) {  // a skipped face has no pixel
    if (lane < GB_REC) out[lane] = 0.f;
    if (CAM && lane < CAM_REC) a.crec[(size_t)f * CAM_REC + lane] = 0.f;
    return;
  }
  float n[3][3], p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = a.faces[3 * (size_t)f + k];  // in [0, V): ok
#pragma unroll
    for (int d = 0; d < 3; ++d) { p[k][d] = a.verts[3 * i + d]; n[k][d] = a.vnrm[3 * i + d]; }
  }
  const float A = mesh_bary_area(x[0], y[0], x[1], y[1], x[2], y[2]);
  float wn[3][3], wx[3][3], gx[3], gy[3], sA = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gx[k] = gy[k] = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) wn[k][d] = wx[k][d] = 0.f;
  }
  for (int64_t j = b + lane; j < e; j += 64) {
    const int64_t pix = a.flist[j];
    if ((uint64_t)pix >= (uint64_t)P || a.p2f[pix] != f) continue;  // a malformed list entry adds nothing
    const int r = (int)(pix / a.S), c = (int)(pix - (int64_t)r * a.S);
    const float px = mesh_pix_ndc(a.S - 1 - c, a.S), py = mesh_pix_ndc(a.S - 1 - r, a.S);
    float w[3];
    mesh_bary(px, py, x[0], y[0], x[1], y[1], x[2], y[2], A, w[0], w[1], w[2]);  // the rasteriser's weights
    float gn[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f};
    if (a.gN) { gn[0] = a.gN[3 * pix]; gn[1] = a.gN[3 * pix + 1]; gn[2] = a.gN[3 * pix + 2]; }
    if (a.gX) { gp[0] = a.gX[3 * pix]; gp[1] = a.gX[3 * pix + 1]; gp[2] = a.gX[3 * pix + 2]; }
    float d[3], cw = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ck = gn[0] * n[k][0] + gn[1] * n[k][1] + gn[2] * n[k][2] + gp[0] * p[k][0] + gp[1] * p[k][1] + gp[2] * p[k][2];
      d[k] = ck / A;  // d loss / d e_k
      cw += ck * w[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        wn[k][q] += w[k] * gn[q];
        wx[k][q] += w[k] * gp[q];
      }
    }
    sA -= cw / A;  // d loss / dA
    // e(p, a, b): d/dax = py - by, d/day = bx - px, d/dbx = ay - py, d/dby = px - ax
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // e_k = E(p, k + 1, k + 2)
      const int ia = (k + 1) % 3, ib = (k + 2) % 3;
      gx[ia] += d[k] * (py - y[ib]);
      gy[ia] += d[k] * (x[ib] - px);
      gx[ib] += d[k] * (y[ia] - py);
      gy[ib] += d[k] * (px - x[ia]);
    }
  }
  sA = gb_wave_sum(sA);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gx[k] = gb_wave_sum(gx[k]);
    gy[k] = gb_wave_sum(gy[k]);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      wn[k][d] = gb_wave_sum(wn[k][d]);
      wx[k][d] = gb_wave_sum(wx[k][d]);
    }
  }
  if (lane != 0) return;
  // A = E(v2, v0, v1) + eps: dA/dx_k = y_(k+2) - y_(k+1), dA/dy_k = x_(k+1) - x_(k+2)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
    const float tx = gx[k] + sA * (y[i2] - y[i1]), ty = gy[k] + sA * (x[i1] - x[i2]);
    // x = q_x / (q_z t), y = q_y / (q_z t)
    const float wz = z[k] * a.cam.tan_half_fov;
    const float qx = tx / wz, qy = ty / wz, qz = -(tx * x[k] + ty * y[k]) / z[k];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      out[6 * k + d] = wn[k][d];
      out[6 * k + 3 + d] = wx[k][d] + (a.cam.R[3 * d] * qx + a.cam.R[3 * d + 1] * qy + a.cam.R[3 * d + 2] * qz);
    }
  }
  // a.crec is never NULL in a <true> launch.  The test is NOT redundant and must stay: it puts the record in a block of its
  // own, which with mesh_opaque keeps grad_verts' bits those of the <false> instance (mesh_camera_record, reni_mesh.inc;
  // only the device's bit-equality tests, tests/test_gpu_camera_grad.py, notice when that is lost).
  if (CAM && a.crec) {  // the barycentric path alone: wx is world-space
    Camera cam = a.cam;
    cam.tan_half_fov = mesh_opaque(cam.tan_half_fov);
    float tx[3], ty[3], xo[3], yo[3], zo[3], po[3][3];
    mesh_opaque3(gx, tx); mesh_opaque3(gy, ty); mesh_opaque3(x, xo); mesh_opaque3(y, yo); mesh_opaque3(z, zo);
    const float sAo = mesh_opaque(sA);
#pragma unroll
    for (int k = 0; k < 3; ++k) mesh_opaque3(p[k], po[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // A = E(v2, v0, v1) + eps folded in, as above
      const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
      const float dx = sAo * (yo[i2] - yo[i1]), dy = sAo * (xo[i1] - xo[i2]);
      tx[k] += dx;
      ty[k] += dy;
    }
    mesh_camera_record(cam, tx, ty, xo, yo, zo, po, a.crec + (size_t)f * CAM_REC);
  }
}

// ---- vertex normals: u_v, and g u_v from g n_v -------------------------------------------------------------------------
// g u_v of vertex v for its g n_v: mesh_u (k_vertex_normals' sum), then the Jacobian of u / max(|u|, 1e-6)
DEV void gb_gu(const GbMesh& m, int v, const float gn[3], float gu[3]) {
  float ux, uy, uz;
  mesh_u(m, v, ux, uy, uz);
  const float len = sqrtf(ux * ux + uy * uy + uz * uz);
  if (len > MESH_NRM_EPS) {
    const float inv = 1.f / len;
    const float nx = ux * inv, ny = uy * inv, nz = uz * inv;
    const float d = nx * gn[0] + ny * gn[1] + nz * gn[2];
    gu[0] = (gn[0] - nx * d) * inv;
    gu[1] = (gn[1] - ny * d) * inv;
    gu[2] = (gn[2] - nz * d) * inv;
  } else {  // the max branch: n = u 1e6
    const float s = 1.f / MESH_NRM_EPS;
    gu[0] = gn[0] * s; gu[1] = gn[1] * s; gu[2] = gn[2] * s;
  }
}

// ---- per-vertex gather of the face records ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gb_vertex(const GbMesh m, const float* __restrict__ rec, float* __restrict__ gu,
                                                   float* __restrict__ gverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.V) return;
  int64_t b, e;
  mesh_corner_range(m, v, b, e);
  float gn[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
  for (int64_t k = b; k < e; ++k) {
    const int64_t c = m.corner[k];
    if (!mesh_corner_names(m, c, v)) continue;
    const int64_t f = c / 3;
    const float* r = rec + (size_t)f * GB_REC + 6 * (int)(c - 3 * f);
    gn[0] += r[0]; gn[1] += r[1]; gn[2] += r[2];
    gd[0] += r[3]; gd[1] += r[4]; gd[2] += r[5];
  }
  gverts[3 * (size_t)v] = gd[0]; gverts[3 * (size_t)v + 1] = gd[1]; gverts[3 * (size_t)v + 2] = gd[2];
  if (gu) {
    float g[3];
    gb_gu(m, v, gn, g);
    gu[3 * (size_t)v] = g[0]; gu[3 * (size_t)v + 1] = g[1]; gu[3 * (size_t)v + 2] = g[2];
  }
}

// ---- vertex-normal backward --------------------------------------------------------------------------------------------
// g: g u [V][3] (STORED) or g n [V][3]; gverts[v] = (accumulate ? gverts[v] : 0) + the sum over v's corners.  Not STORED: g u of a
// corner's vertex is recomputed from its g n; the thread's own vertex, which every one of its faces names, once in front.
template <bool STORED>
__global__ void __launch_bounds__(256) k_vn_bwd(const GbMesh m, const float* __restrict__ g, int accumulate,
                                                float* __restrict__ gverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.V) return;
  int64_t b, e;
  mesh_corner_range(m, v, b, e);
  float own[3] = {0.f, 0.f, 0.f};
  if (!STORED && b < e) {
    const float gn[3] = {g[3 * (size_t)v], g[3 * (size_t)v + 1], g[3 * (size_t)v + 2]};
    gb_gu(m, v, gn, own);
  }
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int64_t k = b; k < e; ++k) {
    const int64_t c = m.corner[k];
    int64_t idx[3];
    if (!mesh_corner_face(m, c, v, idx[0], idx[1], idx[2])) continue;
    float Gx = 0.f, Gy = 0.f, Gz = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float gu[3];
      const float* s = g + 3 * idx[j];
      if (STORED) { gu[0] = s[0]; gu[1] = s[1]; gu[2] = s[2]; }
      else if (idx[j] == v) { gu[0] = own[0]; gu[1] = own[1]; gu[2] = own[2]; }
      else { const float gn[3] = {s[0], s[1], s[2]}; gb_gu(m, (int)idx[j], gn, gu); }
      Gx += gu[0]; Gy += gu[1]; Gz += gu[2];
    }
    const float* p0 = m.verts + 3 * idx[0];
    const float* p1 = m.verts + 3 * idx[1];
    const float* p2 = m.verts + 3 * idx[2];
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const float dax = by * Gz - bz * Gy, day = bz * Gx - bx * Gz, daz = bx * Gy - by * Gx;  // b x G
    const float dbx = Gy * az - Gz * ay, dby = Gz * ax - Gx * az, dbz = Gx * ay - Gy * ax;  // G x a
    const int kk = (int)(c - 3 * (c / 3));
    if (kk == 1) { sx += dax; sy += day; sz += daz; }
    else if (kk == 2) { sx += dbx; sy += dby; sz += dbz; }
    else { sx -= dax + dbx; sy -= day + dby; sz -= daz + dbz; }
  }
  float* o = gverts + 3 * (size_t)v;
  if (accumulate) { sx += o[0]; sy += o[1]; sz += o[2]; }
  o[0] = sx; o[1] = sy; o[2] = sz;
}

}  // namespace reni

namespace {

size_t gb_rec_bytes(int64_t F) { return ((size_t)F * reni::GB_REC * sizeof(float) + 255) & ~(size_t)255; }
size_t gb_gu_bytes(int64_t V) { return ((size_t)V * 3 * sizeof(float) + 255) & ~(size_t)255; }
// the camera records [F][CAM_REC] and, behind them, the reducer's chunk sums
size_t gb_cam_rec_bytes(int64_t F) { return ((size_t)F * reni::CAM_REC * sizeof(float) + 255) & ~(size_t)255; }
size_t gb_cam_bytes(int64_t F) { return gb_cam_rec_bytes(F) + ((reni::camera_part_floats(F) * sizeof(float) + 255) & ~(size_t)255); }

// reni_gbuffer_backward (camera false: grad_camera is not looked at, today's checks and launches) and
// reni_gbuffer_backward_camera (camera true: grad_verts and the vertex lists are optional, together)
int gb_backward(const char* who, bool camera, int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W, const int64_t* pix_to_face,
                const int64_t* face_pixel_offsets, const int64_t* face_pixel_list, const int64_t* vf_offsets, const int64_t* vf_corners,
                const float* grad_pixel_normals, const float* grad_pixel_positions, float* grad_verts, float* grad_camera, void* ws,
                size_t ws_bytes, void* stream) {
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (int rc = mesh_check_image(who, H, W)) return rc;
  if (camera && !grad_verts && !grad_camera) return tu_fail(RENI_EINVAL, who, "grad_verts and grad_camera are both NULL");
  if (camera && !grad_camera) return tu_fail(RENI_EINVAL, who, "NULL grad_camera (reni_gbuffer_backward computes grad_verts alone)");
  const bool need_verts = !camera || grad_verts;
  if (!verts || !faces || !vert_normals || !R || !T || !pix_to_face || !face_pixel_offsets || !face_pixel_list ||
      (need_verts && (!vf_offsets || !vf_corners || !grad_verts)))
    return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (!grad_pixel_normals && !grad_pixel_positions) return tu_fail(RENI_EINVAL, who, "both upstream gradients are NULL");
  if (int rc = mesh_check_fov(who, tan_half_fov)) return rc;
  const size_t need = camera ? gb_rec_bytes(F) + gb_gu_bytes(V) + gb_cam_bytes(F) : gb_rec_bytes(F) + (size_t)V * 3 * sizeof(float);
  if (int rc = tu_check_ws(who, ws, ws_bytes, need)) return rc;
  hipStream_t s = (hipStream_t)stream;
  reni::GbArgs a;
  a.verts = verts; a.vnrm = vert_normals; a.faces = faces; a.p2f = pix_to_face; a.foff = face_pixel_offsets;
  a.flist = face_pixel_list; a.gN = grad_pixel_normals; a.gX = grad_pixel_positions;
  a.rec = (float*)ws;
  a.cam = mesh_camera(R, T, tan_half_fov);
  a.V = (int)V; a.F = (int)F; a.S = (int)H;
  a.crec = camera ? (float*)((char*)ws + gb_rec_bytes(F) + gb_gu_bytes(V)) : nullptr;
  const auto k = camera ? reni::k_gb_face<true> : reni::k_gb_face<false>;
  if (int rc = tu_launch(TU_PLAIN, k, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, s, a)) return rc;
  if (camera)
    if (int rc = reni::launch_camera_reduce(a.crec, F, (float*)((char*)a.crec + gb_cam_rec_bytes(F)), grad_camera, s)) return rc;
  if (!need_verts) return RENI_OK;  // the mesh is known and only the pose is fitted: no vertex kernel, no list
  const reni::GbMesh m{verts, faces, vf_offsets, vf_corners, (int)V, (int)F};
  // without an upstream for the normals g n_v is 0 everywhere: the vertex-normal chain adds nothing and is not run
  float* gu = grad_pixel_normals ? (float*)((char*)ws + gb_rec_bytes(F)) : nullptr;
  const dim3 vgrid((unsigned)((V + 255) / 256));
  if (int rc = tu_launch(TU_PLAIN, reni::k_gb_vertex, vgrid, dim3(256), 0, s, m, (const float*)a.rec, gu, grad_verts)) return rc;
  if (!gu) return RENI_OK;
  return tu_launch(TU_PLAIN, reni::k_vn_bwd<true>, vgrid, dim3(256), 0, s, m, (const float*)gu, 1, grad_verts);
}

}  // namespace

extern "C" {

int reni_mesh_vertex_normals_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* vf_offsets,
                                      const int64_t* vf_corners, const float* grad_normals, float* grad_verts, void* stream) {
  const char* who = "vertex normals backward";
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (!verts || !faces || !vf_offsets || !vf_corners || !grad_normals || !grad_verts) return tu_fail(RENI_EINVAL, who, "NULL argument");
  const reni::GbMesh m{verts, faces, vf_offsets, vf_corners, (int)V, (int)F};
  return tu_launch(TU_PLAIN, reni::k_vn_bwd<false>, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m,
                   grad_normals, 0, grad_verts);
}

size_t reni_gbuffer_backward_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return gb_rec_bytes(F) + (size_t)V * 3 * sizeof(float) + 256;
}

int reni_gbuffer_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals, const float* R,
                          const float* T, float tan_half_fov, int64_t H, int64_t W, const int64_t* pix_to_face,
                          const int64_t* face_pixel_offsets, const int64_t* face_pixel_list, const int64_t* vf_offsets,
                          const int64_t* vf_corners, const float* grad_pixel_normals, const float* grad_pixel_positions,
                          float* grad_verts, void* ws, size_t ws_bytes, void* stream) {
  return gb_backward("gbuffer backward", false, V, F, verts, faces, vert_normals, R, T, tan_half_fov, H, W, pix_to_face,
                     face_pixel_offsets, face_pixel_list, vf_offsets, vf_corners, grad_pixel_normals, grad_pixel_positions, grad_verts,
                     nullptr, ws, ws_bytes, stream);
}

size_t reni_gbuffer_backward_camera_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return gb_rec_bytes(F) + gb_gu_bytes(V) + gb_cam_bytes(F) + 256;
}

int reni_gbuffer_backward_camera(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                                 const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W,
                                 const int64_t* pix_to_face, const int64_t* face_pixel_offsets, const int64_t* face_pixel_list,
                                 const int64_t* vf_offsets, const int64_t* vf_corners, const float* grad_pixel_normals,
                                 const float* grad_pixel_positions, float* grad_verts, float* grad_camera, void* ws, size_t ws_bytes,
                                 void* stream) {
  return gb_backward("gbuffer backward camera", true, V, F, verts, faces, vert_normals, R, T, tan_half_fov, H, W, pix_to_face,
                     face_pixel_offsets, face_pixel_list, vf_offsets, vf_corners, grad_pixel_normals, grad_pixel_positions, grad_verts,
                     grad_camera, ws, ws_bytes, stream);
}

}  // extern "C"
