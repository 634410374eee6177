// translation unit of libreni_hip.so: the mesh pipeline in front of the environment-map shader (FIT_INVERSE task).
//
// Reference: build_renderer, src/utils/pytorch3d_envmap_shader.py:177-217 -- pytorch3d's Meshes.verts_normals_packed,
// FoVPerspectiveCameras (defaults), MeshRasterizer(image_size = S, blur_radius = 0, faces_per_pixel = 1,
// perspective_correct = False) and the two interpolate_face_attributes calls of the shader (:68-73).  Restated from
// pytorch3d's documented behaviour; all arithmetic is fp32 as there.  Three kernels, none with a float atomic; the mesh_*
// pieces (projection, edge function, weights, face rule, list walk) are reni_mesh.inc's, shared with the backward:
//
//   k_vertex_normals  one thread per vertex gathers cross(v1 - v0, v2 - v0) of its faces in ascending face order
//                     through a vertex -> (face, corner) CSR list, then v / max(|v|, 1e-6)        (pytorch3d: index_add)
//   k_face_setup      one thread per face: world -> view (p R + T, row vectors) -> NDC (x / (z tan(fov/2)), the kept z is
//                     view z, no epsilon, no clipping); a 64-byte record (NDC xy, view z, signed area) and an NDC box, empty
//                     when the face is skipped (max z < 0, |area| <= 1e-8, a vertex index outside [0, V)).  No culling.
//   k_raster_tile     one workgroup per 16 x 16 pixel tile (four wave64 waves of 8 x 8).  Face boxes stream through in chunks
//                     of 256: thread t tests face chunk + t against the tile's pixel-centre extent, the overlapping faces are
//                     compacted in ASCENDING order (ballot + popcount prefix, then the waves' counts) and their records staged
//                     in LDS; every lane then tests its pixel against the list (LDS broadcast reads).  Nearest face by strict <
//                     in ascending face order (lowest index wins an exact tie, pytorch3d's naive kernel).  The winner's
//                     distance and the interpolated vertex normal / world position (not normalised: what
//                     interpolate_face_attributes hands the shader) are computed once per pixel at the end.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reni_hip.h"
#include "reni_internal.h"
#include "reni_tu_host.inc"
#include "reni_mesh.inc"

namespace reni {

constexpr int RS_TILE = 16;       // pixels per tile side
constexpr int RS_CHUNK = 256;     // faces per LDS stage (= threads per workgroup)

struct FaceRec {  // 64 bytes, read as four float4 (world order of the corners)
  float4 xy01;    // NDC x0 y0 x1 y1
  float4 xy2z01;  // NDC x2 y2, view z0 z1
  float4 z2a;     // view z2, signed area edge(v0, v1, v2), -, -
  float4 box;     // NDC xmin xmax ymin ymax; empty (+inf, -inf, +inf, -inf) for a skipped face
};

DEV float point_line_dist2(float px, float py, float ax, float ay, float bx, float by) {  // PointLineDistanceForward
  const float bax = bx - ax, bay = by - ay;
  const float l2 = bax * bax + bay * bay;
  if (l2 <= MESH_EPS) return (px - bx) * (px - bx) + (py - by) * (py - by);
  const float t = fminf(fmaxf((bax * (px - ax) + bay * (py - ay)) / l2, 0.f), 1.f);
  const float dx = ax + t * bax - px, dy = ay + t * bay - py;
  return dx * dx + dy * dy;
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vertex_normals(int V, int F, const float* __restrict__ verts,
                                                        const int64_t* __restrict__ faces, const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ corner, float* __restrict__ nrm) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const GbMesh m{verts, faces, off, corner, V, F};
  float nx, ny, nz;
  mesh_u(m, v, nx, ny, nz);
  const float inv = 1.f / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), MESH_NRM_EPS);
  nrm[3 * (size_t)v] = nx * inv;
  nrm[3 * (size_t)v + 1] = ny * inv;
  nrm[3 * (size_t)v + 2] = nz * inv;
}

// ---- face setup --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_face_setup(int V, int F, const float* __restrict__ verts,
                                                    const int64_t* __restrict__ faces, const Camera cam,
                                                    FaceRec* __restrict__ rec) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  float x[3], y[3], z[3], area;
  const bool ok = mesh_face(cam, V, verts, faces, (size_t)f, x, y, z, area);
  FaceRec r;
  r.xy01 = float4{x[0], y[0], x[1], y[1]};
  r.xy2z01 = float4{x[2], y[2], z[0], z[1]};
  r.z2a = float4{z[2], area, 0.f, 0.f};
  if (ok) r.box = float4{fminf(x[0], fminf(x[1], x[2])), fmaxf(x[0], fmaxf(x[1], x[2])),
                         fminf(y[0], fminf(y[1], y[2])), fmaxf(y[0], fmaxf(y[1], y[2]))};
  else r.box = float4{INFINITY, -INFINITY, INFINITY, -INFINITY};
  rec[f] = r;
}

// ---- tile rasteriser + interpolation -----------------------------------------------------------------------------------
struct RasterArgs {
  const FaceRec* rec;
  const float* verts;
  const float* vnrm;
  const int64_t* faces;
  int64_t* pix_to_face;
  float* zbuf;
  float* bary;
  float* dists;
  float* gnrm;
  float* gpos;
  int F, S;
};

__global__ void __launch_bounds__(256) k_raster_tile(const RasterArgs a) {
  __shared__ float4 s_geo[RS_CHUNK][3];  // the overlapping faces' xy01, xy2z01, z2a, compacted in ascending face order
  __shared__ int s_idx[RS_CHUNK];
  __shared__ int s_wcount[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S;
  const int r = blockIdx.y * RS_TILE + (wave >> 1) * 8 + (lane >> 3);
  const int c = blockIdx.x * RS_TILE + (wave & 1) * 8 + (lane & 7);
  const bool live = r < S && c < S;
  const float px = mesh_pix_ndc(S - 1 - c, S), py = mesh_pix_ndc(S - 1 - r, S);
  // the tile's pixel-centre extent (rows / columns beyond the image excluded); x decreases with c, y with r
  const int c_hi = min(S, (int)(blockIdx.x + 1) * RS_TILE) - 1, r_hi = min(S, (int)(blockIdx.y + 1) * RS_TILE) - 1;
  const float tx_max = mesh_pix_ndc(S - 1 - blockIdx.x * RS_TILE, S), tx_min = mesh_pix_ndc(S - 1 - c_hi, S);
  const float ty_max = mesh_pix_ndc(S - 1 - blockIdx.y * RS_TILE, S), ty_min = mesh_pix_ndc(S - 1 - r_hi, S);

  float best_z = INFINITY, w0b = -1.f, w1b = -1.f, w2b = -1.f;
  int best_f = -1;
  for (int base = 0; base < a.F; base += RS_CHUNK) {
    const int f = base + tid;
    bool hit = false;
    if (f < a.F) {
      const float4 b = a.rec[f].box;  // CheckPointOutsideBoundingBox against any pixel of the tile
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
    if (hit) {
      const FaceRec& q = a.rec[f];
      s_geo[slot][0] = q.xy01;
      s_geo[slot][1] = q.xy2z01;
      s_geo[slot][2] = q.z2a;
      s_idx[slot] = f;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float4 g0 = s_geo[k][0], g1 = s_geo[k][1], g2 = s_geo[k][2];
      const float x0 = g0.x, y0 = g0.y, x1 = g0.z, y1 = g0.w, x2 = g1.x, y2 = g1.y;
      if (px > fmaxf(x0, fmaxf(x1, x2)) || px < fminf(x0, fminf(x1, x2)) ||
          py > fmaxf(y0, fmaxf(y1, y2)) || py < fminf(y0, fminf(y1, y2))) continue;
      const float A = mesh_bary_area(x0, y0, x1, y1, x2, y2);
      float w0, w1, w2;
      mesh_bary(px, py, x0, y0, x1, y1, x2, y2, A, w0, w1, w2);
      if (!(w0 > 0.f && w1 > 0.f && w2 > 0.f)) continue;  // blur_radius 0: inside only
      const float pz = w0 * g1.z + w1 * g1.w + w2 * g2.x;
      if (pz < 0.f || !(pz < best_z)) continue;
      best_z = pz; best_f = s_idx[k]; w0b = w0; w1b = w1; w2b = w2;
    }
  }
  if (!live) return;
  const size_t p = (size_t)r * S + c;
  float nx = 0.f, ny = 0.f, nz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f, dist = -1.f;
  if (best_f >= 0) {
    const FaceRec& q = a.rec[best_f];
    const float x0 = q.xy01.x, y0 = q.xy01.y, x1 = q.xy01.z, y1 = q.xy01.w, x2 = q.xy2z01.x, y2 = q.xy2z01.y;
    const float d = fminf(point_line_dist2(px, py, x0, y0, x1, y1),
                          fminf(point_line_dist2(px, py, x0, y0, x2, y2), point_line_dist2(px, py, x1, y1, x2, y2)));
    dist = -d;  // inside: negative (PointTriangleDistanceForward, signed)
    const int64_t* fi = a.faces + 3 * (size_t)best_f;  // in range: the face passed k_face_setup's index check
    const float* n0 = a.vnrm + 3 * fi[0];
    const float* n1 = a.vnrm + 3 * fi[1];
    const float* n2 = a.vnrm + 3 * fi[2];
    const float* v0 = a.verts + 3 * fi[0];
    const float* v1 = a.verts + 3 * fi[1];
    const float* v2 = a.verts + 3 * fi[2];
    nx = w0b * n0[0] + w1b * n1[0] + w2b * n2[0];
    ny = w0b * n0[1] + w1b * n1[1] + w2b * n2[1];
    nz = w0b * n0[2] + w1b * n1[2] + w2b * n2[2];
    qx = w0b * v0[0] + w1b * v1[0] + w2b * v2[0];
    qy = w0b * v0[1] + w1b * v1[1] + w2b * v2[1];
    qz = w0b * v0[2] + w1b * v1[2] + w2b * v2[2];
  } else {
    best_z = -1.f;
  }
  a.pix_to_face[p] = best_f;
  a.zbuf[p] = best_z;
  a.bary[3 * p] = w0b; a.bary[3 * p + 1] = w1b; a.bary[3 * p + 2] = w2b;
  a.dists[p] = dist;
  a.gnrm[3 * p] = nx; a.gnrm[3 * p + 1] = ny; a.gnrm[3 * p + 2] = nz;
  a.gpos[3 * p] = qx; a.gpos[3 * p + 1] = qy; a.gpos[3 * p + 2] = qz;
}

}  // namespace reni

extern "C" {

size_t reni_raster_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 1 || F < 1 || H < 1 || W < 1 || V > MESH_MAX_ELEMS || F > MESH_MAX_ELEMS) return 0;
  return (size_t)F * sizeof(reni::FaceRec) + 256;
}

int reni_mesh_vertex_normals(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* vf_offsets,
                             const int64_t* vf_corners, float* normals, void* stream) {
  const char* who = "vertex normals";
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (!verts || !faces || !vf_offsets || !vf_corners || !normals) return tu_fail(RENI_EINVAL, who, "NULL argument");
  return tu_launch(TU_PLAIN, reni::k_vertex_normals, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)V,
                   (int)F, verts, faces, vf_offsets, vf_corners, normals);
}

int reni_rasterize_mesh(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                        const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W, int64_t* pix_to_face,
                        float* zbuf, float* bary, float* dists, float* pixel_normals, float* pixel_positions, void* ws,
                        size_t ws_bytes, void* stream) {
  const char* who = "rasterize";
  if (int rc = mesh_check_sizes(who, V, F)) return rc;
  if (int rc = mesh_check_image(who, H, W)) return rc;
  if (!verts || !faces || !vert_normals || !R || !T || !pix_to_face || !zbuf || !bary || !dists || !pixel_normals ||
      !pixel_positions)
    return tu_fail(RENI_EINVAL, who, "NULL argument");
  if (int rc = mesh_check_fov(who, tan_half_fov)) return rc;
  if (int rc = tu_check_ws(who, ws, ws_bytes, (size_t)F * sizeof(reni::FaceRec))) return rc;
  hipStream_t s = (hipStream_t)stream;
  reni::FaceRec* rec = (reni::FaceRec*)ws;
  if (int rc = tu_launch(TU_PLAIN, reni::k_face_setup, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, (int)V, (int)F, verts, faces,
                         mesh_camera(R, T, tan_half_fov), rec))
    return rc;
  reni::RasterArgs a;
  a.rec = rec; a.verts = verts; a.vnrm = vert_normals; a.faces = faces;
  a.pix_to_face = pix_to_face; a.zbuf = zbuf; a.bary = bary; a.dists = dists; a.gnrm = pixel_normals; a.gpos = pixel_positions;
  a.F = (int)F; a.S = (int)H;
  const unsigned tiles = (unsigned)((H + reni::RS_TILE - 1) / reni::RS_TILE);
  return tu_launch(TU_PLAIN, reni::k_raster_tile, dim3(tiles, tiles), dim3(256), 0, s, a);
}

}  // extern "C"
