/* Host-only AddressSanitizer run of the C ABI's argument-validation and layout paths.
 * Plain C against include/reni_hip.h -- the same boundary a reference-side binding sees.  Built by tests/test_capi_asan_cpu.py with
 * `hipcc --cuda-host-only -fsanitize=address` from the library's own translation units (no device code, no GPU): every entry point
 * is driven up to the point where it would touch the device -- NULL and out-of-range arguments, every supported width / depth /
 * conditioning through plan creation, workspace sizing, launch / path reports, the workspace-too-small returns behind the layout
 * computation.  ASan watches the plan's offset tables, the layout arrays and the info buffers (heap allocated at their exact size).
 * Prints "capi_args: N checks ok" and exits 0; any unexpected return code is a failure with the library's message.
 * With the argument `dump` it also prints one line per (plan, B, P, flags) of the sweep and of the FiLM plans -- workspace bytes, the four
 * launch-info and the eight path-info values: two builds of the library whose dumps are equal size and report every call alike.
 * With the argument `errors` it runs the utility entry points' bad-argument cases alone (utility_cases below) and prints one line
 * per case -- entry point | case | code | message.  tests/golden/capi_errors.txt is that output of the sources before the utility
 * units shared one host path; every later build must print it byte for byte. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "reni_hip.h"

static int n_checks = 0, n_bad = 0;
#define EXPECT(expr, want)                                                                              \
  do {                                                                                                  \
    long long got_ = (long long)(expr);                                                                 \
    ++n_checks;                                                                                         \
    if (got_ != (long long)(want)) {                                                                    \
      ++n_bad;                                                                                          \
      fprintf(stderr, "%s:%d: %s = %lld, expected %lld (%s)\n", __FILE__, __LINE__, #expr, got_, (long long)(want), reni_last_error()); \
    }                                                                                                   \
  } while (0)
#define EXPECT_TRUE(expr) EXPECT(!!(expr), 1)

static int g_dump = 0;
static void dump_line(const char* kind, const reni_desc* d, const reni_plan* p, int64_t B, int64_t P, uint32_t fl) {
  int32_t i4[4] = {0, 0, 0, 0}, i8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!g_dump) return;
  reni_launch_info(p, B, P, i4);
  reni_path_info(p, B, P, fl, i8);
  printf("%s eq=%d H=%d L=%d dt=%d ml=%d B=%lld P=%lld fl=%u ws=%zu launch=%d,%d,%d,%d path=%d,%d,%d,%d,%d,%d,%d,%d\n", kind, d->equivariance,
         d->hidden_features, d->hidden_layers, d->dtype, d->mapping_layers, (long long)B, (long long)P, fl, reni_workspace_bytes(p, B, P, fl),
         i4[0], i4[1], i4[2], i4[3], i8[0], i8[1], i8[2], i8[3], i8[4], i8[5], i8[6], i8[7]);
}

static int64_t g_st3[3] = {3 * 128, 3, 1};
static const int64_t* st3(uint32_t unused) { (void)unused; return g_st3; }

static reni_desc desc(int eq, int nd, int H, int L, int dtype, int cond, int ml, int mf) {
  reni_desc d;
  memset(&d, 0, sizeof(d));
  d.equivariance = eq; d.ndims = nd; d.hidden_features = H; d.hidden_layers = L; d.out_features = 3;
  d.last_layer_linear = 1; d.output_activation = RENI_ACT_TANH; d.first_omega_0 = 30.f; d.hidden_omega_0 = 30.f;
  d.dtype = dtype; d.conditioning = cond; d.mapping_layers = ml; d.mapping_features = mf;
  return d;
}

/* ---- the utility entry points (shade, image, raster, baselines, diffuse, glossy and its backward, resample, rotate, metrics,
 * lights, visibility): every argument check that needs no device, one bad argument at a time behind otherwise valid ones, so
 * that exactly that check fires.  A *_workspace_bytes function must answer 0, every other call must fail (before any launch:
 * this binary has no device code).  Device pointers are never read on the host: one fake address stands in for all of them. */
static int g_errors = 0;
static void case_line(const char* entry, const char* label, long long rc, int is_size) {
  ++n_checks;
  if (is_size ? rc != 0 : rc == RENI_OK) {
    ++n_bad;
    fprintf(stderr, "%s [%s]: accepted (%lld)\n", entry, label, rc);
  }
  if (g_errors) printf("%s | %s | %lld | %s\n", entry, label, rc, is_size ? "" : reni_last_error());
}
#define BAD(entry, label, ...) case_line(#entry, label, (long long)entry(__VA_ARGS__), 0)
#define SIZE0(entry, label, ...) case_line(#entry, label, (long long)entry(__VA_ARGS__), 1)

static void utility_cases(void) {
  float* f = (float*)(uintptr_t)0x10000;
  double* dbl = (double*)(uintptr_t)0x10000;
  int64_t* i64 = (int64_t*)(uintptr_t)0x10000;
  int32_t* i32 = (int32_t*)(uintptr_t)0x10000;
  uint32_t* u32 = (uint32_t*)(uintptr_t)0x10000;
  void* ws = (void*)(uintptr_t)0x20000;   /* 256-byte aligned */
  void* wsm = (char*)ws + 8;              /* ... and not */
  const size_t big = (size_t)1 << 40;
  const int64_t st3[3] = {128, 16, 1}, st4[4] = {384, 128, 16, 1}, st5[5] = {384, 384, 48, 3, 1};
  const int64_t neg3[3] = {128, 16, -1}, neg4[4] = {384, 128, 16, -1}, neg5[5] = {384, 384, 48, 3, -1};
  const int64_t wide5[5] = {384, 384, (int64_t)1 << 31, 3, 1}, wide4[4] = {384, 128, (int64_t)1 << 31, 1};
  const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 3};
  const int32_t kinds[3] = {RENI_LOBE_PHONG, RENI_LOBE_BLINN, RENI_LOBE_GGX}, kinds_bad[3] = {RENI_LOBE_PHONG, 3, RENI_LOBE_GGX};
  const float par[3] = {8.f, 16.f, .5f}, par_neg[3] = {8.f, -1.f, .5f}, par_ggx[3] = {8.f, 16.f, 2.f};
  const float inf = 1.0f / 0.0f;
  size_t need;

  /* ---- shade (the four entry points share their checks; a workspace is needed once the other axis is split: J = 512) */
  SIZE0(reni_envmap_shade_workspace_bytes, "B = 0", 0, 4, 4);
  BAD(reni_envmap_shade, "B = 0", 0, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "NP = 2^30", 1, (int64_t)1 << 30, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "B = 65536", 65536, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "normals NULL", 1, 4, 4, NULL, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "positions NULL", 1, 4, 4, f, NULL, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "light_dirs NULL", 1, 4, 4, f, f, 0.f, 0.f, 2.f, NULL, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "light_colors NULL", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, NULL, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "colors NULL", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, NULL, ws, big, NULL);
  BAD(reni_envmap_shade, "dirs stride 3 J - 1", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 11, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "shininess 0", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 0.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade, "workspace NULL", 1, 4, 512, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, NULL, big, NULL);
  BAD(reni_envmap_shade, "workspace one byte short", 1, 4, 512, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, 4 * 4 * 3 * 4 - 1, NULL);
  BAD(reni_envmap_shade_backward, "J = 0", 1, 4, 0, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, big, NULL);
  BAD(reni_envmap_shade_backward, "workspace one byte short", 1, 512, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, f, ws, 4 * 4 * 3 * 4 - 1, NULL);
  BAD(reni_envmap_shade_masked, "NP = 0", 1, 0, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, u32, 0, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked, "mask NULL", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, NULL, 0, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked, "mask misaligned", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, u32 + 1, 0, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked, "mask stride with shared directions", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, u32, 4, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked, "mask stride NP JW - 1", 2, 4, 4, f, f, 0.f, 0.f, 2.f, f, 12, f, 50.f, .5f, .5f, u32, 3, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked, "mask stride not a multiple of 4 words at JW = 4", 2, 4, 128, f, f, 0.f, 0.f, 2.f, f, 384, f, 50.f, .5f, .5f, u32, 18, f, ws, big, NULL);
  BAD(reni_envmap_shade_masked_backward, "mask NULL", 1, 4, 4, f, f, 0.f, 0.f, 2.f, f, 0, f, 50.f, .5f, .5f, NULL, 0, f, ws, big, NULL);

  /* ---- image */
  SIZE0(reni_image_workspace_bytes, "H = 0", 1, 0, 16);
  need = reni_image_workspace_bytes(1, 8, 16);
  BAD(reni_unnormalise_srgb, "B = 0", 0, 8, 16, f, st4, 1, 0., 1., 1, f, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "B H W = 2^30", 1, 32768, 32768, f, st4, 1, 0., 1., 1, f, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "img NULL", 1, 8, 16, NULL, st4, 1, 0., 1., 1, f, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "strides NULL", 1, 8, 16, f, NULL, 1, 0., 1., 1, f, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "srgb without out_srgb", 1, 8, 16, f, st4, 1, 0., 1., 1, NULL, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "nothing to compute", 1, 8, 16, f, st4, 1, 0., 1., 0, f, NULL, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "H = 4097 with srgb", 1, 4097, 2, f, st4, 1, 0., 1., 1, f, f, ws, big, NULL);
  BAD(reni_unnormalise_srgb, "workspace NULL", 1, 8, 16, f, st4, 1, 0., 1., 1, f, f, NULL, big, NULL);
  BAD(reni_unnormalise_srgb, "workspace misaligned", 1, 8, 16, f, st4, 1, 0., 1., 1, f, f, wsm, big, NULL);
  BAD(reni_unnormalise_srgb, "workspace one byte short", 1, 8, 16, f, st4, 1, 0., 1., 1, f, f, ws, need - 1, NULL);
  BAD(reni_minmax_normalise, "n = 0", 0, f, 0., 1., f, ws, big, NULL);
  BAD(reni_minmax_normalise, "n = 2^38", (int64_t)1 << 38, f, 0., 1., f, ws, big, NULL);
  BAD(reni_minmax_normalise, "img NULL", 128, NULL, 0., 1., f, ws, big, NULL);
  BAD(reni_minmax_normalise, "out NULL", 128, f, 0., 1., NULL, ws, big, NULL);
  BAD(reni_minmax_normalise, "workspace NULL", 128, f, 0., 1., f, NULL, big, NULL);
  BAD(reni_minmax_normalise, "workspace misaligned", 128, f, 0., 1., f, wsm, big, NULL);
  BAD(reni_minmax_normalise, "workspace one byte short", 128, f, 0., 1., f, ws, 255, NULL);
  BAD(reni_minmax_normalise, "minmax equal", 128, f, 1., 1., f, ws, big, NULL);
  SIZE0(reni_minmax_batch_workspace_bytes, "N = 0", 0);
  SIZE0(reni_minmax_batch_workspace_bytes, "N = 65536", 65536);
  BAD(reni_minmax_normalise_batch, "N = 0", 0, 128, f, 0., 1., 1, f, ws, big, NULL);
  BAD(reni_minmax_normalise_batch, "n = 2^30", 2, (int64_t)1 << 30, f, 0., 1., 1, f, ws, big, NULL);
  BAD(reni_minmax_normalise_batch, "imgs NULL", 2, 128, NULL, 0., 1., 1, f, ws, big, NULL);
  BAD(reni_minmax_normalise_batch, "out NULL", 2, 128, f, 0., 1., 1, NULL, ws, big, NULL);
  BAD(reni_minmax_normalise_batch, "minmax reversed", 2, 128, f, 1., 0., 1, f, ws, big, NULL);
  BAD(reni_minmax_normalise_batch, "workspace NULL", 2, 128, f, 0., 1., 1, f, NULL, big, NULL);
  BAD(reni_minmax_normalise_batch, "workspace misaligned", 2, 128, f, 0., 1., 1, f, wsm, big, NULL);
  BAD(reni_minmax_normalise_batch, "workspace one byte short", 2, 128, f, 0., 1., 1, f, ws, 2 * 8 - 1, NULL);

  /* ---- raster */
  SIZE0(reni_raster_workspace_bytes, "V = 0", 0, 4, 16, 16);
  SIZE0(reni_raster_workspace_bytes, "F = 2^30", 4, (int64_t)1 << 30, 16, 16);
  BAD(reni_mesh_vertex_normals, "V = 0", 0, 4, f, i64, i64, i64, f, NULL);
  BAD(reni_mesh_vertex_normals, "F = 2^30", 4, (int64_t)1 << 30, f, i64, i64, i64, f, NULL);
  BAD(reni_mesh_vertex_normals, "verts NULL", 4, 4, NULL, i64, i64, i64, f, NULL);
  BAD(reni_mesh_vertex_normals, "faces NULL", 4, 4, f, NULL, i64, i64, f, NULL);
  BAD(reni_mesh_vertex_normals, "vf_offsets NULL", 4, 4, f, i64, NULL, i64, f, NULL);
  BAD(reni_mesh_vertex_normals, "vf_corners NULL", 4, 4, f, i64, i64, NULL, f, NULL);
  BAD(reni_mesh_vertex_normals, "normals NULL", 4, 4, f, i64, i64, i64, NULL, NULL);
  need = reni_raster_workspace_bytes(4, 4, 16, 16) - 256;
  BAD(reni_rasterize_mesh, "F = 0", 4, 0, f, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "H != W", 4, 4, f, i64, f, R, T, .5f, 16, 8, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "H = 0", 4, 4, f, i64, f, R, T, .5f, 0, 0, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "H W = 2^30", 4, 4, f, i64, f, R, T, .5f, 32768, 32768, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "verts NULL", 4, 4, NULL, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "faces NULL", 4, 4, f, NULL, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "vert_normals NULL", 4, 4, f, i64, NULL, R, T, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "R NULL", 4, 4, f, i64, f, NULL, T, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "T NULL", 4, 4, f, i64, f, R, NULL, .5f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "pix_to_face NULL", 4, 4, f, i64, f, R, T, .5f, 16, 16, NULL, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "pixel_positions NULL", 4, 4, f, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, NULL, ws, big, NULL);
  BAD(reni_rasterize_mesh, "tan_half_fov 0", 4, 4, f, i64, f, R, T, 0.f, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "tan_half_fov inf", 4, 4, f, i64, f, R, T, inf, 16, 16, i64, f, f, f, f, f, ws, big, NULL);
  BAD(reni_rasterize_mesh, "workspace NULL", 4, 4, f, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, NULL, big, NULL);
  BAD(reni_rasterize_mesh, "workspace misaligned", 4, 4, f, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, wsm, big, NULL);
  BAD(reni_rasterize_mesh, "workspace one byte short", 4, 4, f, i64, f, R, T, .5f, 16, 16, i64, f, f, f, f, f, ws, need - 1, NULL);

  /* ---- baselines (the SG loss needs a workspace above 768 pixels per map: 32 x 64) */
  SIZE0(reni_sg_workspace_bytes, "K = 65", 2, 65, 8, 16);
  BAD(reni_sg_render, "N = 0", 0, 4, 8, 16, f, f, f, .5f, .5f, f, NULL);
  BAD(reni_sg_render, "K = 65", 2, 65, 8, 16, f, f, f, .5f, .5f, f, NULL);
  BAD(reni_sg_render, "params NULL", 2, 4, 8, 16, NULL, f, f, .5f, .5f, f, NULL);
  BAD(reni_sg_render, "theta_c NULL", 2, 4, 8, 16, f, NULL, f, .5f, .5f, f, NULL);
  BAD(reni_sg_render, "phi_c NULL", 2, 4, 8, 16, f, f, NULL, .5f, .5f, f, NULL);
  BAD(reni_sg_render, "rec NULL", 2, 4, 8, 16, f, f, f, .5f, .5f, NULL, NULL);
  need = reni_sg_workspace_bytes(2, 4, 32, 64) - 256;
  BAD(reni_sg_loss_grad, "H = 0", 2, 4, 0, 16, f, f, f, .5f, .5f, f, f, 0, 0, 16, 1, f, f, f, ws, big, NULL);
  BAD(reni_sg_loss_grad, "log_target NULL", 2, 4, 8, 16, f, f, f, .5f, .5f, NULL, f, 0, 0, 16, 1, f, f, f, ws, big, NULL);
  BAD(reni_sg_loss_grad, "weight NULL", 2, 4, 8, 16, f, f, f, .5f, .5f, f, NULL, 0, 0, 16, 1, f, f, f, ws, big, NULL);
  BAD(reni_sg_loss_grad, "loss_total NULL", 2, 4, 8, 16, f, f, f, .5f, .5f, f, f, 0, 0, 16, 1, f, NULL, f, ws, big, NULL);
  BAD(reni_sg_loss_grad, "dparams NULL", 2, 4, 8, 16, f, f, f, .5f, .5f, f, f, 0, 0, 16, 1, f, f, NULL, ws, big, NULL);
  BAD(reni_sg_loss_grad, "weight stride -1", 2, 4, 8, 16, f, f, f, .5f, .5f, f, f, 0, 0, 16, -1, f, f, f, ws, big, NULL);
  BAD(reni_sg_loss_grad, "workspace NULL", 2, 4, 32, 64, f, f, f, .5f, .5f, f, f, 0, 0, 64, 1, f, f, f, NULL, big, NULL);
  BAD(reni_sg_loss_grad, "workspace misaligned", 2, 4, 32, 64, f, f, f, .5f, .5f, f, f, 0, 0, 64, 1, f, f, f, wsm, big, NULL);
  BAD(reni_sg_loss_grad, "workspace one byte short", 2, 4, 32, 64, f, f, f, .5f, .5f, f, f, 0, 0, 64, 1, f, f, f, ws, need - 1, NULL);
  BAD(reni_sh_project, "lmax = 16", 2, 8, 16, 16, f, f, f, f, NULL);
  BAD(reni_sh_project, "lmax = -1", 2, 8, 16, -1, f, f, f, f, NULL);
  BAD(reni_sh_project, "N = 0", 0, 8, 16, 2, f, f, f, f, NULL);
  BAD(reni_sh_project, "W odd", 2, 8, 17, 2, f, f, f, f, NULL);
  BAD(reni_sh_project, "H != W / 2", 2, 9, 16, 2, f, f, f, f, NULL);
  BAD(reni_sh_project, "W = 4098", 2, 2049, 4098, 2, f, f, f, f, NULL);
  BAD(reni_sh_project, "img NULL", 2, 8, 16, 2, NULL, f, f, f, NULL);
  BAD(reni_sh_project, "row_table NULL", 2, 8, 16, 2, f, NULL, f, f, NULL);
  BAD(reni_sh_project, "col_table NULL", 2, 8, 16, 2, f, f, NULL, f, NULL);
  BAD(reni_sh_project, "coeffs NULL", 2, 8, 16, 2, f, f, f, NULL, NULL);
  BAD(reni_sh_reconstruct, "lmax = 16", 2, 8, 16, 16, f, f, f, f, NULL);
  BAD(reni_sh_reconstruct, "W odd", 2, 8, 17, 2, f, f, f, f, NULL);
  BAD(reni_sh_reconstruct, "N = 2^30", (int64_t)1 << 30, 8, 16, 2, f, f, f, f, NULL);
  BAD(reni_sh_reconstruct, "coeffs NULL", 2, 8, 16, 2, NULL, f, f, f, NULL);
  BAD(reni_sh_reconstruct, "out NULL", 2, 8, 16, 2, f, f, f, NULL, NULL);

  /* ---- diffuse (a workspace is needed once the reduction is split: Q = 8192) */
  SIZE0(reni_diffuse_workspace_bytes, "N = 0", 0, 64, 128);
  BAD(reni_diffuse_convolve, "Q = 0", 2, 64, 0, f, f, f, f, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "P = 2^29", 2, (int64_t)1 << 29, 128, f, f, f, f, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "out_dirs NULL", 2, 64, 128, NULL, f, f, f, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "in_dirs NULL", 2, 64, 128, f, NULL, f, f, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "in_w NULL", 2, 64, 128, f, f, NULL, f, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "src NULL", 2, 64, 128, f, f, f, NULL, 384, 3, 1, 1.f, f, ws, big, NULL);
  BAD(reni_diffuse_convolve, "out NULL", 2, 64, 128, f, f, f, f, 384, 3, 1, 1.f, NULL, ws, big, NULL);
  BAD(reni_diffuse_convolve, "src stride -1", 2, 64, 128, f, f, f, f, 384, -1, 1, 1.f, f, ws, big, NULL);
  need = reni_diffuse_workspace_bytes(2, 64, 8192) - 256;
  BAD(reni_diffuse_convolve, "workspace NULL", 2, 64, 8192, f, f, f, f, 24576, 3, 1, 1.f, f, NULL, big, NULL);
  BAD(reni_diffuse_convolve, "workspace misaligned", 2, 64, 8192, f, f, f, f, 24576, 3, 1, 1.f, f, wsm, big, NULL);
  BAD(reni_diffuse_convolve, "workspace one byte short", 2, 64, 8192, f, f, f, f, 24576, 3, 1, 1.f, f, ws, need - 1, NULL);
  BAD(reni_sh_irradiance_l2, "N = 0", 0, 64, f, f, 0, f, NULL);
  BAD(reni_sh_irradiance_l2, "P = 2^29", 2, (int64_t)1 << 29, f, f, 0, f, NULL);
  BAD(reni_sh_irradiance_l2, "normals stride 3 P - 1", 2, 64, f, f, 191, f, NULL);
  BAD(reni_sh_irradiance_l2, "coeffs NULL", 2, 64, NULL, f, 0, f, NULL);
  BAD(reni_sh_irradiance_l2, "normals NULL", 2, 64, f, NULL, 0, f, NULL);
  BAD(reni_sh_irradiance_l2, "out NULL", 2, 64, f, f, 0, NULL, NULL);

  /* ---- glossy */
  SIZE0(reni_lobe_workspace_bytes, "n_lobes = 17", 2, 64, 128, 17);
  SIZE0(reni_lobe_workspace_bytes, "P = 0", 2, 0, 128, 3);
  need = reni_lobe_workspace_bytes(2, 64, 128, 3) - 256;
  BAD(reni_lobe_convolve, "n_lobes = 0", 2, 64, 128, f, f, f, f, 384, 3, 1, 0, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "n_lobes = 17", 2, 64, 128, f, f, f, f, 384, 3, 1, 17, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "N = 0", 0, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "out_dirs NULL", 2, 64, 128, NULL, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "src NULL", 2, 64, 128, f, f, f, NULL, 384, 3, 1, 3, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "kinds NULL", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, NULL, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "params NULL", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, NULL, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "out NULL", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, NULL, ws, big, NULL);
  BAD(reni_lobe_convolve, "unknown kind", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds_bad, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "parameter -1", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par_neg, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "GGX alpha 2", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par_ggx, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "src stride -1", 2, 64, 128, f, f, f, f, -1, 3, 1, 3, kinds, par, 1, 1.f, f, ws, big, NULL);
  BAD(reni_lobe_convolve, "workspace NULL", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, f, NULL, big, NULL);
  BAD(reni_lobe_convolve, "workspace misaligned", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, f, wsm, big, NULL);
  BAD(reni_lobe_convolve, "workspace one byte short", 2, 64, 128, f, f, f, f, 384, 3, 1, 3, kinds, par, 1, 1.f, f, ws, need - 1, NULL);
  SIZE0(reni_lobe_denominators_workspace_bytes, "Q = 0", 64, 0, 3);
  need = reni_lobe_denominators_workspace_bytes(64, 128, 3) - 256;
  BAD(reni_lobe_denominators, "n_lobes = 17", 64, 128, f, f, f, 17, kinds, par, f, ws, big, NULL);
  BAD(reni_lobe_denominators, "P = 0", 0, 128, f, f, f, 3, kinds, par, f, ws, big, NULL);
  BAD(reni_lobe_denominators, "in_w NULL", 64, 128, f, f, NULL, 3, kinds, par, f, ws, big, NULL);
  BAD(reni_lobe_denominators, "den NULL", 64, 128, f, f, f, 3, kinds, par, NULL, ws, big, NULL);
  BAD(reni_lobe_denominators, "kinds NULL", 64, 128, f, f, f, 3, NULL, par, f, ws, big, NULL);
  BAD(reni_lobe_denominators, "unknown kind", 64, 128, f, f, f, 3, kinds_bad, par, f, ws, big, NULL);
  BAD(reni_lobe_denominators, "workspace NULL", 64, 128, f, f, f, 3, kinds, par, f, NULL, big, NULL);
  BAD(reni_lobe_denominators, "workspace misaligned", 64, 128, f, f, f, 3, kinds, par, f, wsm, big, NULL);
  BAD(reni_lobe_denominators, "workspace one byte short", 64, 128, f, f, f, 3, kinds, par, f, ws, need - 1, NULL);
  BAD(reni_envmap_lookup, "Lv = 0", 2, 0, 8, 16, 64, f, st5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "W odd", 2, 1, 8, 17, 64, f, st5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "N = 65536", 65536, 1, 8, 16, 64, f, st5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "src NULL", 2, 1, 8, 16, 64, NULL, st5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "src_strides NULL", 2, 1, 8, 16, 64, f, NULL, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "dirs NULL", 2, 1, 8, 16, 64, f, st5, NULL, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "out NULL", 2, 1, 8, 16, 64, f, st5, f, 0, NULL, 0, 0.f, NULL, NULL);
  BAD(reni_envmap_lookup, "src stride -1", 2, 1, 8, 16, 64, f, neg5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "row stride 2^31", 2, 1, 8, 16, 64, f, wide5, f, 0, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "dirs stride 3 P - 1", 2, 1, 8, 16, 64, f, st5, f, 191, NULL, 0, 0.f, f, NULL);
  BAD(reni_envmap_lookup, "level stride P - 1", 2, 1, 8, 16, 64, f, st5, f, 0, f, 63, 0.f, f, NULL);

  /* ---- glossy, backward */
  SIZE0(reni_lobe_backward_workspace_bytes, "N = 0", 0, 64, 128, 3);
  need = reni_lobe_backward_workspace_bytes(2, 64, 128, 3) - 256;
  BAD(reni_lobe_convolve_backward, "n_lobes = 0", 2, 64, 128, f, f, f, f, 0, kinds, par, 1, 1.f, f, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "Q = 0", 2, 64, 0, f, f, f, f, 3, kinds, par, 1, 1.f, f, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "grad_out NULL", 2, 64, 128, f, f, f, NULL, 3, kinds, par, 1, 1.f, f, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "grad_src NULL", 2, 64, 128, f, f, f, f, 3, kinds, par, 1, 1.f, f, NULL, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "params NULL", 2, 64, 128, f, f, f, f, 3, kinds, NULL, 1, 1.f, f, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "den NULL when normalising", 2, 64, 128, f, f, f, f, 3, kinds, par, 1, 1.f, NULL, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "GGX alpha 2", 2, 64, 128, f, f, f, f, 3, kinds, par_ggx, 1, 1.f, f, f, 384, 3, 1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "grad_src stride -1", 2, 64, 128, f, f, f, f, 3, kinds, par, 1, 1.f, f, f, 384, 3, -1, ws, big, NULL);
  BAD(reni_lobe_convolve_backward, "workspace NULL", 2, 64, 128, f, f, f, f, 3, kinds, par, 0, 1.f, NULL, f, 384, 3, 1, NULL, big, NULL);
  BAD(reni_lobe_convolve_backward, "workspace misaligned", 2, 64, 128, f, f, f, f, 3, kinds, par, 1, 1.f, f, f, 384, 3, 1, wsm, big, NULL);
  BAD(reni_lobe_convolve_backward, "workspace one byte short", 2, 64, 128, f, f, f, f, 3, kinds, par, 1, 1.f, f, f, 384, 3, 1, ws, need - 1, NULL);
  BAD(reni_envmap_lookup_taps, "P = 0", 1, 1, 8, 16, 0, f, 0, NULL, 0, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_taps, "W odd", 1, 1, 8, 17, 64, f, 0, NULL, 0, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_taps, "Lv H W = 2^31", 1, 16, 8192, 16384, 64, f, 0, NULL, 0, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_taps, "dirs NULL", 1, 1, 8, 16, 64, NULL, 0, NULL, 0, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_taps, "tap_index NULL", 1, 1, 8, 16, 64, f, 0, NULL, 0, 0.f, NULL, f, NULL);
  BAD(reni_envmap_lookup_taps, "tap_weight NULL", 1, 1, 8, 16, 64, f, 0, NULL, 0, 0.f, i32, NULL, NULL);
  BAD(reni_envmap_lookup_taps, "dirs stride 3 P - 1", 2, 1, 8, 16, 64, f, 191, NULL, 0, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_taps, "level stride P - 1", 2, 1, 8, 16, 64, f, 0, f, 63, 0.f, i32, f, NULL);
  BAD(reni_envmap_lookup_backward, "N = 0", 0, 1, 8, 16, 64, f, 1, f, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "W odd", 2, 1, 8, 17, 64, f, 1, f, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "N = 65536", 65536, 1, 8, 16, 64, f, 1, f, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "n_tables = 3 of N = 2", 2, 1, 8, 16, 64, f, 3, f, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "grad_out NULL", 2, 1, 8, 16, 64, NULL, 1, f, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "grad_src NULL", 2, 1, 8, 16, 64, f, 1, f, i64, i64, NULL, NULL);
  BAD(reni_envmap_lookup_backward, "tap_weight NULL", 2, 1, 8, 16, 64, f, 1, NULL, i64, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "tap_order NULL", 2, 1, 8, 16, 64, f, 1, f, NULL, i64, f, NULL);
  BAD(reni_envmap_lookup_backward, "offsets NULL", 2, 1, 8, 16, 64, f, 1, f, i64, NULL, f, NULL);

  /* ---- resample, blur */
  BAD(reni_resample, "Hd = 0", 2, 3, 8, 16, 0, 8, f, st4, i32, f, 2, i32, f, 2, f, NULL);
  BAD(reni_resample, "N = 65536", 65536, 3, 8, 16, 4, 8, f, st4, i32, f, 2, i32, f, 2, f, NULL);
  BAD(reni_resample, "row_taps = 0", 2, 3, 8, 16, 4, 8, f, st4, i32, f, 0, i32, f, 2, f, NULL);
  BAD(reni_resample, "col_taps = 9", 2, 3, 8, 16, 4, 8, f, st4, i32, f, 2, i32, f, 9, f, NULL);
  BAD(reni_resample, "src NULL", 2, 3, 8, 16, 4, 8, NULL, st4, i32, f, 2, i32, f, 2, f, NULL);
  BAD(reni_resample, "src_strides NULL", 2, 3, 8, 16, 4, 8, f, NULL, i32, f, 2, i32, f, 2, f, NULL);
  BAD(reni_resample, "row_idx NULL", 2, 3, 8, 16, 4, 8, f, st4, NULL, f, 2, i32, f, 2, f, NULL);
  BAD(reni_resample, "col_w NULL", 2, 3, 8, 16, 4, 8, f, st4, i32, f, 2, i32, NULL, 2, f, NULL);
  BAD(reni_resample, "out NULL", 2, 3, 8, 16, 4, 8, f, st4, i32, f, 2, i32, f, 2, NULL, NULL);
  BAD(reni_resample, "src stride -1", 2, 3, 8, 16, 4, 8, f, neg4, i32, f, 2, i32, f, 2, f, NULL);
  SIZE0(reni_blur_workspace_bytes, "C = 65536", 65536, 8, 16);
  need = reni_blur_workspace_bytes(3, 8, 16) - 256;
  BAD(reni_gaussian_blur, "C = 0", 0, 8, 16, f, st3, f, 4, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "radius -1", 3, 8, 16, f, st3, f, -1, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "radius 2^20 + 1", 3, 8, 16, f, st3, f, (1 << 20) + 1, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "src NULL", 3, 8, 16, NULL, st3, f, 4, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "strides NULL", 3, 8, 16, f, NULL, f, 4, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "weights NULL", 3, 8, 16, f, st3, NULL, 4, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "out NULL", 3, 8, 16, f, st3, f, 4, NULL, ws, big, NULL);
  BAD(reni_gaussian_blur, "stride -1", 3, 8, 16, f, neg3, f, 4, f, ws, big, NULL);
  BAD(reni_gaussian_blur, "workspace NULL", 3, 8, 16, f, st3, f, 4, f, NULL, big, NULL);
  BAD(reni_gaussian_blur, "workspace misaligned", 3, 8, 16, f, st3, f, 4, f, wsm, big, NULL);
  BAD(reni_gaussian_blur, "workspace one byte short", 3, 8, 16, f, st3, f, 4, f, ws, need - 1, NULL);

  /* ---- rotate */
  BAD(reni_rotate_envmap, "C = 0", 2, 0, 8, 16, f, st4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "W odd", 2, 3, 8, 17, f, st4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "B = 65536", 65536, 3, 8, 16, f, st4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "src NULL", 2, 3, 8, 16, NULL, st4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "src_strides NULL", 2, 3, 8, 16, f, NULL, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "rot NULL", 2, 3, 8, 16, f, st4, NULL, 2, NULL, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "row_trig NULL", 2, 3, 8, 16, f, st4, NULL, 2, f, 0, NULL, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "col_trig NULL", 2, 3, 8, 16, f, st4, NULL, 2, f, 0, f, NULL, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "out NULL", 2, 3, 8, 16, f, st4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, NULL, NULL);
  BAD(reni_rotate_envmap, "src stride -1", 2, 3, 8, 16, f, neg4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "row stride 2^31", 2, 3, 8, 16, f, wide4, NULL, 2, f, 0, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "rot_stride 3", 2, 3, 8, 16, f, st4, NULL, 2, f, 3, f, f, RENI_ROTATE_BILINEAR, f, NULL);
  BAD(reni_rotate_envmap, "unknown mode", 2, 3, 8, 16, f, st4, NULL, 2, f, 0, f, f, 2, f, NULL);
  BAD(reni_rotate_envmap, "src_index with n_src = 0", 2, 3, 8, 16, f, st4, i64, 0, f, 0, f, f, RENI_ROTATE_NEAREST, f, NULL);

  /* ---- metrics (8 x 16: one block of sums, 64 bytes for two images; SSIM: one tile, 16 bytes) */
  SIZE0(reni_pair_stats_workspace_bytes, "B = 0", 0, 8, 16);
  SIZE0(reni_pair_stats_workspace_bytes, "B = 65536", 65536, 8, 16);
  BAD(reni_pair_stats, "B = 0", 0, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "H W = 2^30", 2, 32768, 32768, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "pred NULL", 2, 8, 16, NULL, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "pred_strides NULL", 2, 8, 16, f, NULL, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "target NULL", 2, 8, 16, f, st4, NULL, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "target_strides NULL", 2, 8, 16, f, st4, f, NULL, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "out NULL", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, NULL, ws, big, NULL);
  BAD(reni_pair_stats, "weight without strides", 2, 8, 16, f, st4, f, st4, f, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "pred stride -1", 2, 8, 16, f, neg4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "target stride -1", 2, 8, 16, f, st4, f, neg4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "weight stride -1", 2, 8, 16, f, st4, f, st4, f, neg3, RENI_SPACE_STORED, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "unknown space", 2, 8, 16, f, st4, f, st4, NULL, NULL, 3, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "minmax equal in a mapped space", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_LINEAR, 1., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "sRGB without exposures", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_SRGB, 0., 1., NULL, f, ws, big, NULL);
  BAD(reni_pair_stats, "workspace NULL", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, NULL, big, NULL);
  BAD(reni_pair_stats, "workspace misaligned", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, wsm, big, NULL);
  BAD(reni_pair_stats, "workspace one byte short", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, f, ws, 2 * 8 * 4 - 1, NULL);
  BAD(reni_ssim, "B = 0", 0, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "weight stride -1", 2, 8, 16, f, st4, f, st4, f, neg3, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "unknown mode", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, 2, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "L = 0", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 0.f, RENI_SSIM_SPHERE, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "W odd on the sphere", 2, 8, 17, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "H = 4 on the sphere", 2, 4, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "planar with a weight", 2, 16, 16, f, st4, f, st4, f, st3, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_PLANAR, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "planar with H = 10", 2, 10, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_PLANAR, f, NULL, ws, big, NULL);
  BAD(reni_ssim, "workspace NULL", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, NULL, big, NULL);
  BAD(reni_ssim, "workspace misaligned", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, wsm, big, NULL);
  BAD(reni_ssim, "workspace one byte short", 2, 8, 16, f, st4, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 1.f, RENI_SSIM_SPHERE, f, NULL, ws, 2 * 2 * 4 - 1, NULL);

  /* ---- lights */
  SIZE0(reni_light_table_workspace_bytes, "H != W / 2", 2, 9, 16);
  need = reni_light_table_workspace_bytes(2, 8, 16) - 256;
  BAD(reni_light_table_build, "W odd", 2, 8, 17, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "img NULL", 2, 8, 16, NULL, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "img_strides NULL", 2, 8, 16, f, NULL, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "img stride -1", 2, 8, 16, f, neg4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "sRGB space", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_SRGB, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "unknown space", 2, 8, 16, f, st4, NULL, NULL, 3, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "minmax equal in the linear space", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_LINEAR, 1., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "solid_angle NULL", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., NULL, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "marg NULL", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, NULL, ws, big, NULL);
  BAD(reni_light_table_build, "mask without strides", 2, 8, 16, f, st4, f, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "mask stride -1", 2, 8, 16, f, st4, f, neg3, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "uniform_mix 1.5", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 1.5, f, f, f, ws, big, NULL);
  BAD(reni_light_table_build, "workspace NULL", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, NULL, big, NULL);
  BAD(reni_light_table_build, "workspace misaligned", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, wsm, big, NULL);
  BAD(reni_light_table_build, "workspace one byte short", 2, 8, 16, f, st4, NULL, NULL, RENI_SPACE_STORED, 0., 1., f, 0., f, f, f, ws, need - 1, NULL);
  BAD(reni_light_sample, "B = 0", 0, 8, 16, 16, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 0, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "S = 0", 2, 8, 16, 0, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 0, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "img NULL", 2, 8, 16, 16, f, f, f, NULL, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 0, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "pmf NULL", 2, 8, 16, 16, NULL, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 0, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "index NULL", 2, 8, 16, 16, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 0, NULL, f, f, f, f, NULL);
  BAD(reni_light_sample, "uniforms stride 2 S - 1", 2, 8, 16, 16, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 31, f, f, dbl, NULL, 0, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "jitter 2", 2, 8, 16, 16, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, dbl, NULL, 2, i32, f, f, f, f, NULL);
  BAD(reni_light_sample, "jitter without row_cos", 2, 8, 16, 16, f, f, f, f, st4, RENI_SPACE_STORED, 0., 1., f, 0, f, f, NULL, NULL, 1, i32, f, f, f, f, NULL);
  BAD(reni_lights_irradiance, "S = 0", 2, 64, 0, f, 0, f, f, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "B P = 2^28", 2, (int64_t)1 << 27, 16, f, 0, f, f, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "normals stride 3 P - 1", 2, 64, 16, f, 191, f, f, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "normals NULL", 2, 64, 16, NULL, 0, f, f, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "dirs NULL", 2, 64, 16, f, 0, NULL, f, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "colors NULL", 2, 64, 16, f, 0, f, NULL, 1.f, f, NULL);
  BAD(reni_lights_irradiance, "out NULL", 2, 64, 16, f, 0, f, f, 1.f, NULL, NULL);

  /* ---- visibility */
  SIZE0(reni_mesh_visibility_accel_bytes, "F = 0", 0);
  SIZE0(reni_mesh_visibility_accel_bytes, "F = 2^30", (int64_t)1 << 30);
  need = reni_mesh_visibility_accel_bytes(4);
  BAD(reni_mesh_visibility_prepare, "V = 0", 0, 4, f, i64, NULL, ws, big, NULL);
  BAD(reni_mesh_visibility_prepare, "verts NULL", 4, 4, NULL, i64, NULL, ws, big, NULL);
  BAD(reni_mesh_visibility_prepare, "faces NULL", 4, 4, f, NULL, NULL, ws, big, NULL);
  BAD(reni_mesh_visibility_prepare, "accel NULL", 4, 4, f, i64, NULL, NULL, big, NULL);
  BAD(reni_mesh_visibility_prepare, "accel misaligned", 4, 4, f, i64, NULL, wsm, big, NULL);
  BAD(reni_mesh_visibility_prepare, "accel one byte short", 4, 4, f, i64, NULL, ws, need - 1, NULL);
  BAD(reni_mesh_visibility, "J = 0", 1, 256, 0, f, i64, f, 0, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "B = 65536", 65536, 256, 64, f, i64, f, 0, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "positions NULL", 1, 256, 64, NULL, i64, f, 0, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "pix_to_face NULL", 1, 256, 64, f, NULL, f, 0, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "dirs NULL", 1, 256, 64, f, i64, NULL, 0, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "accel NULL", 1, 256, 64, f, i64, f, 0, NULL, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "vis NULL", 1, 256, 64, f, i64, f, 0, ws, 1e-3f, 0, NULL, NULL);
  BAD(reni_mesh_visibility, "accel misaligned", 1, 256, 64, f, i64, f, 0, wsm, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "dirs stride 3 J - 1", 2, 256, 64, f, i64, f, 191, ws, 1e-3f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "t_min -1", 1, 256, 64, f, i64, f, 0, ws, -1.f, 0, u32, NULL);
  BAD(reni_mesh_visibility, "t_min inf", 1, 256, 64, f, i64, f, 0, ws, inf, 0, u32, NULL);
  BAD(reni_mesh_visibility, "unknown flag", 1, 256, 64, f, i64, f, 0, ws, 1e-3f, 2u, u32, NULL);
}

int main(int argc, char** argv) {
  reni_plan* p = NULL;
  g_dump = argc > 1 && strcmp(argv[1], "dump") == 0;
  g_errors = argc > 1 && strcmp(argv[1], "errors") == 0;
  if (g_errors) {
    utility_cases();
    return n_bad ? 1 : 0;
  }
  reni_desc d = desc(RENI_EQ_SO2, 36, 128, 5, RENI_BF16, RENI_COND_CONCAT, 0, 0);
  /* ---- plan creation: argument errors */
  EXPECT(reni_plan_create(NULL, &p), RENI_EINVAL);
  EXPECT(reni_plan_create(&d, NULL), RENI_EINVAL);
  { reni_desc b = d; b.equivariance = 3; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); EXPECT_TRUE(p == NULL); }
  { reni_desc b = d; b.ndims = 0; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  { reni_desc b = d; b.ndims = 257; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  { reni_desc b = d; b.out_features = 4; EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = d; b.hidden_layers = 15; EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = d; b.hidden_layers = -1; EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = d; b.hidden_features = 96; EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = d; b.output_activation = 3; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  { reni_desc b = d; b.dtype = 2; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  { reni_desc b = d; b.conditioning = 2; EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  { reni_desc b = desc(RENI_EQ_NONE, 9, 64, 3, RENI_F32, RENI_COND_FILM, 2, 32); EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = desc(RENI_EQ_SO2, 9, 64, 3, RENI_F32, RENI_COND_FILM, 9, 32); EXPECT(reni_plan_create(&b, &p), RENI_EUNSUPPORTED); }
  { reni_desc b = desc(RENI_EQ_SO2, 9, 64, 3, RENI_F32, RENI_COND_FILM, 2, 0); EXPECT(reni_plan_create(&b, &p), RENI_EINVAL); }
  EXPECT_TRUE(strlen(reni_last_error()) > 0);
  /* NULL plans */
  EXPECT(reni_param_count(NULL), 0);
  EXPECT(reni_in_features(NULL), 0);
  EXPECT(reni_workspace_bytes(NULL, 1, 1, 0), 0);
  EXPECT(reni_film_map_param_count(NULL), 0);
  reni_plan_destroy(NULL);

  /* ---- every width x depth x dtype x invariance: offsets, layouts, reports (heap buffers of the exact size: ASan sees an overrun) */
  const int Hs[4] = {32, 64, 128, 256};
  const int Ls[5] = {0, 1, 5, 6, 14};
  for (int eq = 0; eq <= 2; ++eq)
    for (int hi = 0; hi < 4; ++hi)
      for (int li = 0; li < 5; ++li)
        for (int dt = 0; dt <= 1; ++dt) {
          reni_desc c = desc(eq, eq == 0 ? 4 : 36, Hs[hi], Ls[li], dt, RENI_COND_CONCAT, 0, 0);
          EXPECT(reni_plan_create(&c, &p), RENI_OK);
          if (!p) continue;
          const int nd = c.ndims, H = Hs[hi], L = Ls[li];
          const int F = eq == RENI_EQ_SO2 ? 2 * nd + nd * nd + 2 : eq == RENI_EQ_SO3 ? nd + nd * nd : 4 * nd;
          EXPECT(reni_in_features(p), F);
          EXPECT(reni_param_count(p), (long long)H * F + H + (long long)L * (H * H + H) + 3 * H + 3);
          const int64_t Bs[3] = {1, 7, 64}, Ps[3] = {1, 129, 32768};
          for (int bi = 0; bi < 3; ++bi)
            for (int pi = 0; pi < 3; ++pi)
              for (uint32_t fl = 0; fl <= 3; ++fl) {
                EXPECT_TRUE(reni_workspace_bytes(p, Bs[bi], Ps[pi], fl) > 0);
                int32_t* i4 = (int32_t*)malloc(4 * sizeof(int32_t));
                int32_t* i8 = (int32_t*)malloc(8 * sizeof(int32_t));
                EXPECT(reni_launch_info(p, Bs[bi], Ps[pi], i4), RENI_OK);
                EXPECT(reni_path_info(p, Bs[bi], Ps[pi], fl, i8), RENI_OK);
                EXPECT_TRUE(i4[0] >= 1 && i4[3] == Bs[bi] * ((Ps[pi] + 127) / 128) && i8[6] == 0 && i8[7] >= 1);
                EXPECT_TRUE(i8[3] >= 1 && i8[3] <= Bs[bi]);
                free(i4); free(i8);
                dump_line("concat", &c, p, Bs[bi], Ps[pi], fl);
              }
          EXPECT(reni_workspace_bytes(p, 0, 128, 0), 0);
          EXPECT(reni_workspace_bytes(p, 1, 0, 0), 0);
          EXPECT(reni_launch_info(p, 1, 128, NULL), RENI_EINVAL);
          EXPECT(reni_path_info(p, 1, 128, 3, NULL), RENI_EINVAL);
          EXPECT(reni_path_info(p, 0, 128, 3, (int32_t*)&d), RENI_EINVAL);
          reni_plan_destroy(p);
          p = NULL;
        }
  /* FiLM with a mapping network: the mapping offsets (MAX_MAP_LAYERS + 1 entries) and the glue layout */
  for (int ml = 1; ml <= 8; ++ml) {
    reni_desc c = desc(RENI_EQ_SO2, 36, 128, 5, RENI_BF16, RENI_COND_FILM, ml, 128);
    EXPECT(reni_plan_create(&c, &p), RENI_OK);
    if (!p) continue;
    const long long M_in = 36 * 36 + 36, N_out = 2 * 6 * 128;
    EXPECT(reni_film_map_param_count(p), (M_in * 128 + 128) + (long long)(ml - 1) * (128 * 128 + 128) + (128 * N_out + N_out));
    EXPECT_TRUE(reni_workspace_bytes(p, 64, 32768, 3) > 0);
    for (uint32_t fl = 0; fl <= 3; ++fl) { dump_line("film", &c, p, 64, 32768, fl); dump_line("film", &c, p, 7, 129, fl); }
    reni_plan_destroy(p);
    p = NULL;
  }

  /* ---- compute entry points: rejected before anything touches the device */
  EXPECT(reni_plan_create(&d, &p), RENI_OK);
  float* fake = (float*)(uintptr_t)0x10000;   /* never dereferenced on the host: device pointers as far as the ABI is concerned */
  void* ws = (void*)(uintptr_t)0x20000;       /* 256-byte aligned */
  int64_t st[3] = {3 * 128, 3, 1};
  float terms[4];
  EXPECT(reni_forward(NULL, 1, 128, fake, fake, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 0, 128, fake, fake, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 0, fake, fake, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, NULL, fake, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, fake, NULL, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, fake, fake, 0, NULL, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, fake, fake, 0, fake, NULL, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, fake, fake, 0, fake, fake, NULL, 0, NULL), RENI_EWORKSPACE);
  EXPECT(reni_forward(p, 1, 128, fake, fake, 0, fake, fake, (char*)ws + 8, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_forward(p, 1, 128, fake, fake, 0, fake, fake, ws, 16, NULL), RENI_EWORKSPACE);
  EXPECT(reni_forward(p, (int64_t)1 << 40, 128, fake, fake, 0, fake, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, NULL, st, fake, st, RENI_LOSS_MSE, 0.f, 0.f, 3, NULL, terms, fake, fake,
                                    ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, fake, st, fake, st, 7, 0.f, 0.f, 3, NULL, terms, fake, fake, ws, 16,
                                    NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f, 0.f, 3, NULL, NULL, fake, fake,
                                    ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f, 0.f, RENI_NEED_DW, NULL, terms,
                                    fake, NULL, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f, 0.f, RENI_NEED_DZ, NULL, terms,
                                    NULL, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward(p, 2, 256, fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f, 3, NULL, terms, fake,
                                    fake, ws, 16, NULL), RENI_EWORKSPACE);
  EXPECT(reni_forward_loss_backward_rows(p, 2, 256, fake, 10, NULL, fake, 0, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f, 0.f, 3, NULL,
                                         terms, fake, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_forward_loss_backward_rows(p, 2, 256, fake, 0, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f,
                                         0.f, 3, NULL, terms, fake, fake, ws, 16, NULL), RENI_EINVAL);
  { uint32_t st = 3;
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, NULL, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE, 0.f, 0.f, fake, fake,
                                fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, &st, terms, fake, fake, ws, 16, NULL), RENI_EINVAL);
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE,
                                0.f, 0.f, fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 0, 1.f, &st, terms, fake, fake, ws, 16, NULL),
           RENI_EINVAL);
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE,
                                0.f, 0.f, NULL, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, &st, terms, fake, fake, ws, 16, NULL),
           RENI_EINVAL);
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE,
                                0.f, 0.f, fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL, terms, fake, fake, ws, 16, NULL),
           RENI_EINVAL);
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), 2, 0.f, 0.f,
                                fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, &st, terms, fake, fake, ws, 16, NULL), RENI_EINVAL);
    st = 3;  /* a stale 'staged' state: the call still sizes its layout, finds the workspace too small, and clears the state */
    EXPECT(reni_train_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, (const int64_t*)fake, fake, 0, fake, fake, st3(st), fake, st3(st),
                                RENI_LOSS_MSE, 0.f, 0.f, fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, &st, terms, fake, fake,
                                ws, 16, NULL), RENI_EWORKSPACE); }
  { uint32_t st = 0;  /* reni_train_step_rows_dp: a NULL communicator, then the same argument checks as the one-process step */
    EXPECT(reni_train_step_rows_dp(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE,
                                   0.f, 0.f, fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, .5f, NULL, 0, &st, terms, fake, fake, ws, 16,
                                   NULL), RENI_EINVAL);
    EXPECT(reni_train_step_rows_dp(p, 2, 256, fake, 10, NULL, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE, 0.f, 0.f, fake,
                                   fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, .5f, fake, 0, &st, terms, fake, fake, ws, 16, NULL),
           RENI_EINVAL);
    EXPECT(reni_train_step_rows_dp(p, 2, 256, fake, 10, (const int64_t*)fake, NULL, fake, 0, fake, fake, st3(st), fake, st3(st), RENI_LOSS_MSE,
                                   0.f, 0.f, fake, fake, fake, fake, 1e-3f, .9f, .999f, 1e-8f, 1, .5f, fake, 1, &st, terms, fake, fake, ws, 16,
                                   NULL), RENI_EWORKSPACE); }
  /* reni_weight_lists_*: sizes, flags, alignment; reni_latent_step_rows_cached: NULL lists, flags without a RENI_WEIGHT_* mode */
  EXPECT(reni_weight_lists_bytes(0, 256) == 0 ? RENI_OK : RENI_EINVAL, RENI_OK);
  EXPECT(reni_weight_lists_bytes(2, 256) > 2 * 256 * 4 ? RENI_OK : RENI_EINVAL, RENI_OK);
  EXPECT(reni_weight_lists_build(2, 256, fake, st, 0, ws, 1 << 20, NULL, NULL), RENI_EINVAL);
  EXPECT(reni_weight_lists_build(2, 256, NULL, st, RENI_WEIGHT_SPARSE, ws, 1 << 20, NULL, NULL), RENI_EINVAL);
  EXPECT(reni_weight_lists_build(2, 256, fake, st, RENI_WEIGHT_SPARSE, ws, 16, NULL, NULL), RENI_EWORKSPACE);
  EXPECT(reni_latent_step_rows_cached(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f,
                                      RENI_WEIGHT_SPARSE, NULL, fake, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows_cached(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f,
                                      0, ws, fake, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows_cached(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f,
                                      RENI_WEIGHT_COMPACT, ws, fake, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  /* (^ a lists buffer no reni_weight_lists_build is on record for: refused before anything reads it -- round 6) */
  /* reni_latent_step_rows: NULL idx / optimiser state, step 0, flags other than the RENI_WEIGHT_* bits, then the workspace check */
  EXPECT(reni_latent_step_rows(p, 2, 256, fake, 10, NULL, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f, 0, fake, fake,
                               1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f, 0,
                               NULL, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f, 0,
                               fake, fake, 1e-1f, .9f, .999f, 1e-8f, 0, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f,
                               RENI_NEED_DW, fake, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_latent_step_rows(p, 2, 256, fake, 10, (const int64_t*)fake, fake, 0, fake, fake, st, fake, st, RENI_LOSS_TEST, 1e-7f, 1e-4f,
                               RENI_WEIGHT_COMPACT, fake, fake, 1e-1f, .9f, .999f, 1e-8f, 1, terms, fake, ws, 16, NULL), RENI_EWORKSPACE);
  EXPECT(reni_backward(p, 2, 256, fake, fake, 0, fake, NULL, 3, fake, fake, ws, 16, NULL), RENI_EINVAL);
  EXPECT(reni_backward(p, 2, 256, fake, fake, 0, fake, fake, 3, fake, fake, ws, 16, NULL), RENI_EWORKSPACE);
  /* a concat plan through the FiLM entry points, and the other way round */
  EXPECT(reni_film_forward(p, 1, 128, fake, 0, fake, fake, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  EXPECT(reni_film_model_forward(p, 1, 128, fake, fake, 0, fake, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
  reni_plan_destroy(p);
  { reni_desc c = desc(RENI_EQ_SO3, 9, 64, 3, RENI_F32, RENI_COND_FILM, 2, 32);
    EXPECT(reni_plan_create(&c, &p), RENI_OK);
    EXPECT(reni_forward(p, 1, 128, fake, fake, 0, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
    EXPECT(reni_film_forward(p, 1, 128, fake, 0, NULL, fake, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
    EXPECT(reni_film_forward(p, 1, 128, fake, 0, fake, NULL, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
    EXPECT(reni_film_forward(p, 1, 128, fake, 0, fake, fake, fake, fake, ws, 16, NULL), RENI_EWORKSPACE);
    EXPECT(reni_film_forward_loss_backward(p, 1, 128, fake, 0, fake, fake, fake, fake, st, fake, st, RENI_LOSS_MSE, 0.f, 3, NULL, terms,
                                           NULL, fake, fake, ws, 16, NULL), RENI_EINVAL);
    EXPECT(reni_film_model_forward(p, 1, 128, NULL, fake, 0, fake, fake, fake, ws, 1 << 20, NULL), RENI_EINVAL);
    EXPECT(reni_film_model_forward(p, 1, 128, fake, fake, 0, fake, fake, fake, NULL, 0, NULL), RENI_EWORKSPACE);
    EXPECT(reni_film_model_forward(p, 1, 128, fake, fake, 0, fake, fake, fake, ws, 16, NULL), RENI_EWORKSPACE);
    for (uint32_t fl = 0; fl <= 3; ++fl) { dump_line("film", &c, p, 64, 32768, fl); dump_line("film", &c, p, 7, 129, fl); }
    reni_plan_destroy(p); }
  /* H = 256 training in image chunks: sizing and the chunk count */
  { reni_desc c = desc(RENI_EQ_SO2, 36, 256, 5, RENI_BF16, RENI_COND_CONCAT, 0, 0);
    int32_t i8[8];
    EXPECT(reni_plan_create(&c, &p), RENI_OK);
    /* (round 5: the cap is 16 GB of a 288 GB device -- the BASELINE batch of 64 images, 11.5 GB of stream, is ONE pass; 256 images run in
       equal chunks under the cap) */
    EXPECT(reni_path_info(p, 64, 32768, 3, i8), RENI_OK);
    EXPECT_TRUE(i8[3] == 64 && i8[5] == 1);
    EXPECT_TRUE(reni_workspace_bytes(p, 64, 32768, 3) < ((size_t)14 << 30));
    EXPECT(reni_path_info(p, 256, 32768, 3, i8), RENI_OK);
    EXPECT_TRUE(i8[3] >= 64 && i8[3] <= 96);  /* (three chunks of 86, 86, 84 -- not 95 + 95 + 66) */
    EXPECT_TRUE(reni_workspace_bytes(p, 256, 32768, 3) < ((size_t)18 << 30));
    for (uint32_t fl = 0; fl <= 3; ++fl) { dump_line("chunked", &c, p, 256, 32768, fl); dump_line("chunked", &c, p, 64, 32768, fl); }
    reni_plan_destroy(p); }
  /* optimiser / exchange / diagnostics */
  EXPECT(reni_adam_step(NULL, fake, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_step(fake, fake, fake, fake, -1, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_step(fake, fake, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 0, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_step(fake, fake, fake, fake, 0, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_OK);
  EXPECT(reni_adam_rows_step(fake, fake, NULL, 2, 27, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_rows_step(fake, fake, (const int64_t*)fake, 2, 0, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_rows_step(fake, fake, (const int64_t*)fake, 2, 27, fake, fake, 0, 1e-3f, .9f, .999f, 1e-8f, 1, 1.f, NULL), RENI_OK);
  EXPECT(reni_adam_step2(fake, fake, fake, fake, 4, NULL, fake, (const int64_t*)fake, 2, 27, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 1,
                         1.f, NULL), RENI_EINVAL);
  EXPECT(reni_adam_step2(fake, fake, fake, fake, 0, fake, fake, (const int64_t*)fake, 2, 27, fake, fake, 4, 1e-3f, .9f, .999f, 1e-8f, 1,
                         1.f, NULL), RENI_EINVAL);
  EXPECT(reni_allreduce_grads(NULL, fake, 4, 1.f, NULL), RENI_EINVAL);
  EXPECT(reni_rccl_unique_id(NULL), RENI_EINVAL);
  EXPECT(reni_rccl_comm_create(NULL, 1, 0, NULL), RENI_EINVAL);
  EXPECT(reni_rccl_comm_destroy(NULL), RENI_OK);
  EXPECT(reni_set_grad_ready_event(NULL), RENI_OK);
  EXPECT(reni_profile_enable(0), RENI_OK);
  { double ms = -1; int64_t n = -1;
    EXPECT(reni_profile_read(&ms, &n, 1), RENI_OK);
    EXPECT_TRUE(ms == 0.0 && n == 0);
    EXPECT(reni_profile_read(NULL, &n, 1), RENI_EINVAL); }
  EXPECT(reni_selftest_layouts(NULL, 2), RENI_EINVAL);
  { int32_t mm[2]; EXPECT(reni_selftest_layouts(mm, 1), RENI_EINVAL); }
  EXPECT_TRUE(reni_launch_count(1) >= 0);
  EXPECT(reni_launch_count(0), 0);
  EXPECT(reni_envmap_shade_workspace_bytes(0, 1, 1) == 0 || 1, 1);
  EXPECT_TRUE(reni_image_workspace_bytes(2, 128, 256) > 0);
  utility_cases();

  if (n_bad) {
    fprintf(stderr, "capi_args: %d of %d checks FAILED\n", n_bad, n_checks);
    return 1;
  }
  printf("capi_args: %d checks ok\n", n_checks);
  return 0;
}
