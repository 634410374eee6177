// reni_mesh.inc -- the ONE definition of what the mesh units share: reni_tu_raster.hip (rasteriser, vertex normals),
// reni_tu_raster_bwd.hip (their gradients with respect to the vertex positions), reni_tu_silhouette.hip and reni_tu_texture.hip
// (k_pixel_uv); the camera record of the two face kernels (mesh_camera_record).
// pytorch3d's conventions restated from its documented behaviour, fp32, no float atomic: the camera and its projection, the
// edge function, PixToNdc, kEpsilon, the barycentric weights, the rule by which a face is skipped, the walk of a vertex's
// (face, corner) list and the sum u_v of the vertex normals; on the host the camera fill, MESH_MAX_ELEMS and the checks whose
// messages the entry points share.  The backward differentiates the forward because both call these functions: a change
// here changes both sides.  Included at file scope after reni_tu_host.inc.  DESIGN 4.4q.
#pragma once
#define DEV __device__ __forceinline__

namespace reni {

constexpr float MESH_EPS = 1e-8f;      // pytorch3d kEpsilon (rasterize_meshes)
constexpr float MESH_NRM_EPS = 1e-6f;  // the floor of |u_v| (Meshes.verts_normals_packed)

struct Camera {  // (by value in k_face_setup's signature: the name is part of that symbol)
  float R[9];    // row-major, p_view[j] = sum_i p[i] R[i][j] + T[j]
  float T[3];
  float tan_half_fov;
};

DEV float mesh_edge(float px, float py, float ax, float ay, float bx, float by) {  // EdgeFunctionForward(p, a, b)
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

DEV float mesh_pix_ndc(int i, int S) { return -1.f + (2.f * (float)i + 1.f) / (float)S; }  // PixToNdc, i counted from +x / +y

// world -> view (p R + T, row vectors) -> NDC x, y (divided by z tan(fov / 2)); the kept z is view z, no epsilon, no clipping
DEV void mesh_project(const Camera& cam, float px, float py, float pz, float& x, float& y, float& z) {
  const float vx = px * cam.R[0] + py * cam.R[3] + pz * cam.R[6] + cam.T[0];
  const float vy = px * cam.R[1] + py * cam.R[4] + pz * cam.R[7] + cam.T[1];
  const float vz = px * cam.R[2] + py * cam.R[5] + pz * cam.R[8] + cam.T[2];
  const float w = vz * cam.tan_half_fov;
  x = vx / w;
  y = vy / w;
  z = vz;
}

// BarycentricCoordsForward of pixel (px, py) in the NDC triangle (x, y)[0..2]: A = E(v2, v0, v1) + eps, w_k = E(p, k+1, k+2) / A
DEV float mesh_bary_area(float x0, float y0, float x1, float y1, float x2, float y2) {
  return mesh_edge(x2, y2, x0, y0, x1, y1) + MESH_EPS;
}
DEV void mesh_bary(float px, float py, float x0, float y0, float x1, float y1, float x2, float y2, float A, float& w0, float& w1,
                   float& w2) {
  w0 = mesh_edge(px, py, x1, y1, x2, y2) / A;
  w1 = mesh_edge(px, py, x2, y2, x0, y0) / A;
  w2 = mesh_edge(px, py, x0, y0, x1, y1) / A;
}

// Face f's corners in world order: NDC x y and view z (0 at an index outside [0, V), which is not read), the signed area
// E(v0, v1, v2); false when the rasteriser skips the face (an index outside [0, V), max z < 0, |area| <= eps: it owns no pixel).
DEV bool mesh_face(const Camera& cam, int V, const float* verts, const int64_t* faces, size_t f, float (&x)[3], float (&y)[3],
                   float (&z)[3], float& area) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = y[k] = z[k] = 0.f;  // (a loop of its own: k_face_setup's listing depends on it)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = faces[3 * f + k];
    if (i < 0 || i >= V) { ok = false; continue; }
    mesh_project(cam, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], x[k], y[k], z[k]);
  }
  area = mesh_edge(x[0], y[0], x[1], y[1], x[2], y[2]);
  const float zmax = fmaxf(z[0], fmaxf(z[1], z[2]));
  return ok && !(zmax < 0.f) && !(fabsf(area) <= MESH_EPS);
}

// A face's camera record (reni_internal.h: gR [9] row-major, gT [3], g_tan [1]) from its corners' NDC gradients (tx, ty), NDC
// positions (x, y), view z and world positions p: per corner g_q = (tx / (z t), ty / (z t), -(tx x + ty y) / z), then
// gT += g_q, gR[i][j] += p[i] g_q[j] (q = p R + T: d q_j / d R[i][j] = p_i) and g_tan -= (tx x + ty y) / t, the corners in
// ascending order from 0.  grad_verts must keep the bits of the CAM = false instance, and which of two products hipcc fuses
// into an a b + c d of the vertex gradient depends on what else uses them.  So the face kernels call this behind a branch of
// its own and hand it copies the compiler cannot see through (mesh_opaque) of the NDC gradients and the corners, not the g_q
// they form for the vertices: nothing of the vertex gradient gets a second use.
DEV float mesh_opaque(float v) {
  asm volatile("" : "+v"(v));  // no instruction: v in a VGPR, its origin hidden
  return v;
}
DEV void mesh_opaque3(const float (&v)[3], float (&o)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = mesh_opaque(v[k]);
}
DEV void mesh_camera_record(const Camera& cam, const float (&tx)[3], const float (&ty)[3], const float (&x)[3], const float (&y)[3],
                            const float (&z)[3], const float (&p)[3][3], float* __restrict__ out) {
  float cr[CAM_REC];
#pragma unroll
  for (int c = 0; c < CAM_REC; ++c) cr[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float wz = z[k] * cam.tan_half_fov, s = tx[k] * x[k] + ty[k] * y[k];
    const float q[3] = {tx[k] / wz, ty[k] / wz, -s / z[k]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) cr[3 * i + j] += p[k][i] * q[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) cr[9 + j] += q[j];
    cr[12] -= s / cam.tan_half_fov;
  }
#pragma unroll
  for (int c = 0; c < CAM_REC; ++c) out[c] = cr[c];
}

// ---- the vertex -> (face, corner) list ---------------------------------------------------------------------------------
struct GbMesh {  // (by value in k_gb_vertex's and k_vn_bwd's signatures: the name is part of those symbols)
  const float* verts;
  const int64_t* faces;
  const int64_t* off;     // [V + 1] offsets into corner
  const int64_t* corner;  // corners 3 f + k, ascending per vertex
  int V, F;
};

DEV void mesh_corner_range(const GbMesh& m, int v, int64_t& b, int64_t& e) {  // vertex v's range of the list, clamped into it
  const int64_t n3 = 3 * (int64_t)m.F;
  b = min(max(m.off[v], (int64_t)0), n3);
  e = min(max(m.off[v + 1], b), n3);
}

DEV bool mesh_corner_names(const GbMesh& m, int64_t c, int v) {  // list entry c is a corner and names v; else it adds nothing
  return !(c < 0 || c >= 3 * (int64_t)m.F || m.faces[c] != v);
}

// ... and the three vertex indices of its face, all in [0, V)
DEV bool mesh_corner_face(const GbMesh& m, int64_t c, int v, int64_t& i0, int64_t& i1, int64_t& i2) {
  if (!mesh_corner_names(m, c, v)) return false;
  const int64_t f = c / 3;
  i0 = m.faces[3 * f]; i1 = m.faces[3 * f + 1]; i2 = m.faces[3 * f + 2];
  return !(i0 < 0 || i0 >= m.V || i1 < 0 || i1 >= m.V || i2 < 0 || i2 >= m.V);
}

// u_v = the sum over v's corners, in list order, of cross(p_f1 - p_f0, p_f2 - p_f0); n_v = u_v / max(|u_v|, MESH_NRM_EPS)
DEV void mesh_u(const GbMesh& m, int v, float& ux, float& uy, float& uz) {
  int64_t b, e;
  mesh_corner_range(m, v, b, e);
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int64_t k = b; k < e; ++k) {
    int64_t i0, i1, i2;
    if (!mesh_corner_face(m, m.corner[k], v, i0, i1, i2)) continue;
    const float* p0 = m.verts + 3 * i0;
    const float* p1 = m.verts + 3 * i1;
    const float* p2 = m.verts + 3 * i2;
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    sx += ay * bz - az * by;
    sy += az * bx - ax * bz;
    sz += ax * by - ay * bx;
  }
  ux = sx; uy = sy; uz = sz;
}

}  // namespace reni

namespace {

constexpr int64_t MESH_MAX_ELEMS = 0x3fffffff;  // V, F, Tn; S * S

inline reni::Camera mesh_camera(const float* R, const float* T, float tan_half_fov) {
  reni::Camera cam;
  for (int i = 0; i < 9; ++i) cam.R[i] = R[i];
  for (int i = 0; i < 3; ++i) cam.T[i] = T[i];
  cam.tan_half_fov = tan_half_fov;
  return cam;
}

// RENI_OK, or "<who>: <the text>" set
inline int mesh_check_sizes(const char* who, int64_t V, int64_t F) {
  return V < 1 || F < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS ? tu_fail(RENI_EINVAL, who, "bad V / F") : RENI_OK;
}
inline int mesh_check_image(const char* who, int64_t H, int64_t W) {
  return H < 1 || H != W || H * W > MESH_MAX_ELEMS ? tu_fail(RENI_EINVAL, who, "the image must be square, H == W >= 1") : RENI_OK;
}
inline int mesh_check_fov(const char* who, float tan_half_fov) {
  return !(tan_half_fov > 0.f) || !isfinite(tan_half_fov) ? tu_fail(RENI_EINVAL, who, "tan_half_fov must be positive") : RENI_OK;
}

}  // namespace
