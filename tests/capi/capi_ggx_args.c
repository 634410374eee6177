/* The microfacet (GGX) entry points' argument checks from plain C against include/reni_hip.h: a stand-alone
 * driver for a host-only sanitizer build of the library -- the translation units compiled without device code, as for
 * tests/capi/capi_args.c, the shade unit's host side also under the undefined-behaviour sanitizer -- run on the CPU.  No test
 * builds it; DESIGN 4.4m says how it was built and run.  Every call below must fail before any launch: one bad argument at a
 * time behind otherwise valid ones, so that exactly that check fires.  Device pointers are never read on the host: one fake
 * address stands in for all of them.  Prints "capi_ggx_args: N checks ok" and exits 0; an unexpected return code or message is
 * a failure. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "reni_hip.h"

static int n_checks = 0, n_bad = 0;

static void expect(long long got, long long want, const char* needle, const char* what, int line) {
  ++n_checks;
  if (got != want || (needle && !strstr(reni_last_error(), needle))) {
    ++n_bad;
    fprintf(stderr, "line %d: %s = %lld, expected %lld with \"%s\" (%s)\n", line, what, got, want, needle ? needle : "", reni_last_error());
  }
}
#define EXPECT(expr, want, needle) expect((long long)(expr), (long long)(want), needle, #expr, __LINE__)

typedef struct {
  int64_t B, NP, J, dstride, astride, vstride;
  const float *nrm, *pos, *dirs, *src0, *src1, *src2, *alpha;
  const uint32_t* vis;
  float *out0, *out1, *out2;
  void* ws;
  size_t nbytes;
} Args;

static float* const P = (float*)(uintptr_t)(1u << 20); /* non-NULL, 16-byte aligned; nothing dereferences it */

static Args good(void) {
  Args a;
  a.B = 2; a.NP = 4; a.J = 40; a.dstride = 0; a.astride = 0; a.vstride = 0;
  a.nrm = a.pos = a.dirs = a.src0 = a.src1 = a.src2 = a.alpha = P;
  a.vis = NULL;
  a.out0 = a.out1 = a.out2 = P;
  a.ws = P; a.nbytes = (size_t)1 << 30;
  return a;
}

/* which: 0 forward (src0 = C; outs D, S0, S1), 1 backward (srcs gD, gS0, gS1; out0 = dC), 2 dpixel (src0 = C, then the three
 * upstream gradients in src1, src2 and out2's place is taken by d_normals; out0 = d_alpha) */
static const float* g_gD;
static int call(int which, const Args* a) {
  if (which == 0)
    return reni_envmap_shade_ggx(a->B, a->NP, a->J, a->nrm, a->pos, 0.f, 0.f, 2.f, a->dirs, a->dstride, a->src0, a->alpha, a->astride,
                                 a->vis, a->vstride, a->out0, a->out1, a->out2, a->ws, a->nbytes, NULL);
  if (which == 1)
    return reni_envmap_shade_ggx_backward(a->B, a->NP, a->J, a->nrm, a->pos, 0.f, 0.f, 2.f, a->dirs, a->dstride, a->alpha, a->astride,
                                          a->vis, a->vstride, a->src0, a->src1, a->src2, a->out0, a->ws, a->nbytes, NULL);
  return reni_envmap_shade_ggx_dpixel(a->B, a->NP, a->J, a->nrm, a->pos, 0.f, 0.f, 2.f, a->dirs, a->dstride, a->src0, a->alpha,
                                      a->astride, a->vis, a->vstride, g_gD, a->src1, a->src2, a->out0, a->out1, a->ws, a->nbytes, NULL);
}

int main(void) {
  const uint32_t* const VIS = (const uint32_t*)P;
  g_gD = P;
  EXPECT(reni_envmap_shade_ggx_workspace_bytes(0, 4, 4), 0, NULL);
  EXPECT(reni_envmap_shade_ggx_workspace_bytes(1, 0, 4), 0, NULL);
  EXPECT(reni_envmap_shade_ggx_workspace_bytes(1, 4, -1), 0, NULL);
  EXPECT(reni_envmap_shade_ggx_workspace_bytes(1, 4, 4), 256, NULL);
  EXPECT(reni_envmap_shade_ggx_workspace_bytes(2, 1000, 515), 5 * 3 * 2 * 1000 * 3 * 4 + 256, NULL);
  EXPECT(reni_envmap_shade_ggx_dpixel_workspace_bytes(0, 4, 4), 0, NULL);
  EXPECT(reni_envmap_shade_ggx_dpixel_workspace_bytes(1, 4, 0), 0, NULL);
  EXPECT(reni_envmap_shade_ggx_dpixel_workspace_bytes(1, 4, 4), 4 * 4 * 4 + 256, NULL);
  EXPECT(reni_envmap_shade_ggx_dpixel_workspace_bytes(2, 1000, 515), 2 * 5 * 1000 * 4 * 4 + 256, NULL);
  for (int which = 0; which < 3; ++which) {
    const char* who = which == 2 ? "envmap shade ggx dpixel: " : "envmap shade ggx: ";
    Args a;
    a = good(); a.B = 0; EXPECT(call(which, &a), RENI_EINVAL, ">= 1");
    a = good(); a.NP = 0; EXPECT(call(which, &a), RENI_EINVAL, ">= 1");
    a = good(); a.J = -1; EXPECT(call(which, &a), RENI_EINVAL, who);
    a = good(); a.NP = (int64_t)1 << 30; EXPECT(call(which, &a), RENI_EINVAL, "too large");
    a = good(); a.J = (int64_t)1 << 30; EXPECT(call(which, &a), RENI_EINVAL, "too large");
    a = good(); a.B = 1 << 16; EXPECT(call(which, &a), RENI_EINVAL, "too large");
    a = good(); a.nrm = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    a = good(); a.pos = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    a = good(); a.dirs = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    a = good(); a.src0 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    a = good(); a.alpha = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    a = good(); a.out0 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    if (which != 0) {
      a = good(); a.src1 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
      a = good(); a.src2 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    }
    if (which == 0) {
      a = good(); a.out1 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
      a = good(); a.out2 = NULL; EXPECT(call(which, &a), RENI_EINVAL, "NULL");
    }
    a = good(); a.dstride = 119; EXPECT(call(which, &a), RENI_EINVAL, "direction batch stride");
    a = good(); a.astride = 2; EXPECT(call(which, &a), RENI_EINVAL, "alpha stride");
    a = good(); a.astride = -1; EXPECT(call(which, &a), RENI_EINVAL, "alpha stride");
    a = good(); a.vis = (const uint32_t*)((const char*)P + 4); EXPECT(call(which, &a), RENI_EINVAL, "16-byte aligned");
    a = good(); a.vis = VIS; a.vstride = 8; EXPECT(call(which, &a), RENI_EINVAL, "mask batch stride");
    a = good(); a.vis = VIS; a.dstride = 120; a.vstride = 7; EXPECT(call(which, &a), RENI_EINVAL, "mask batch stride");
    a = good(); a.vis = VIS; a.J = 512; a.dstride = 1536; a.vstride = 66; EXPECT(call(which, &a), RENI_EINVAL, "mask batch stride");
    a = good(); a.NP = 1000; a.J = 515; a.ws = NULL; EXPECT(call(which, &a), RENI_EWORKSPACE, "workspace too small");
    a = good(); a.NP = 1000; a.J = 515; a.nbytes = 1000; EXPECT(call(which, &a), RENI_EWORKSPACE, "workspace too small");
  }
  {
    Args a;
    g_gD = NULL; a = good(); EXPECT(call(2, &a), RENI_EINVAL, "NULL"); g_gD = P;
    a = good(); a.ws = NULL; a.nbytes = 0; EXPECT(call(2, &a), RENI_EWORKSPACE, "workspace too small");   /* dpixel always needs one */
    a = good(); a.nbytes = 4 * 4 * 4 - 1; EXPECT(call(2, &a), RENI_EWORKSPACE, "workspace too small");
    a = good(); a.out1 = NULL; a.nbytes = 4 * 4 - 1; EXPECT(call(2, &a), RENI_EWORKSPACE, "workspace too small"); /* d_normals NULL: a quarter */
  }
  if (n_bad) {
    fprintf(stderr, "capi_ggx_args: %d of %d checks failed\n", n_bad, n_checks);
    return 1;
  }
  printf("capi_ggx_args: %d checks ok\n", n_checks);
  return 0;
}
