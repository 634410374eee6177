// reni_capi.inc -- extern "C" entry points of libreni_hip.so (declared in include/reni_hip.h).
// Included at the end of reni_device.inc in the RENI_TU_CORE translation unit.
#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/reni_hip.h"

struct reni_plan {
  reni_desc d;
  int F_in;
  int64_t n_params;
  int64_t n_first;  // elements of the first layer (W0 + b0): handled by the per-image tails
  unsigned p_off_w[reni::MAX_LAYERS + 2];
  unsigned p_off_b[reni::MAX_LAYERS + 2];
  // FiLM mapping network (reni_film_model_*): layer i is [mN[i]][mK[i]] at mw_off[i], bias at mb_off[i]
  int M_in, N_out;
  int64_t n_map_params;
  unsigned mw_off[reni::MAX_MAP_LAYERS + 1], mb_off[reni::MAX_MAP_LAYERS + 1];
  // path selectors, read from the environment ONCE at plan creation (both alternatives are correct and tested):
  // RENI_NO_PERSIST = the generic kernels instead of the register-persistent ones, RENI_NO_SIDE_STREAM = the per-image epilogue
  // on the caller's stream instead of a forked one
  int no_persist, no_side_stream, dw1_old;  // (RENI_DW1_OLD: k_reni_dw1 instead of k_reni_dw1_ring -- the A/B switch of profiles/tools)
  int no_l0x;          // RENI_NO_L0X: layer 0's backward stays inside the training kernel (round 4's split) instead of k_reni_l0_ring
  int train_wg;        // RENI_TRAIN_WG=n: at most n workgroups for the persistent training instances (0: one per CU) -- longer tile ranges at small shapes
  int env_overrides;   // which of them the environment set: 1 RENI_NO_PERSIST, 2 RENI_NO_SIDE_STREAM, 4 RENI_FRAG_WS_CAP_MB, 8 RENI_DW1_OLD, 16 RENI_NO_L0X, 32 RENI_TRAIN_WG
                       // (reni_path_info reports it, bench.py prints it: a stray variable must not silently change what is measured)
  size_t frag_ws_cap;  // bytes of stash + fragment stream one chunk of the H = 256 training path may use (run_backward_chunked);
                       // RENI_FRAG_WS_CAP_MB overrides the 3 GB default (tests force the chunked path at small sizes with it)
};

namespace {

thread_local std::string g_err;

// Every kernel launch of the core (RENI_LAUNCH and timed_launch below) is counted (reni_launch_count): bench.py reports launches per step beside ms_per_step -- at small
// problems a step is its dependent launches, not its FLOPs (DESIGN.md section 5).  Of the utility units only some count theirs
// (note_launches, through tu_launch(TU_COUNTED, ...) of reni_tu_host.inc): DESIGN.md section 4.4i has the table.
std::atomic<long long> g_launches{0};
// reni_set_grad_ready_event: recorded on the call's stream once the gradient of everything behind layer 1 is final (see the header)
thread_local hipEvent_t g_ev_rest = nullptr;
// (... and its launch error is the enclosing function's return: HIP_TRY, below)
#define RENI_LAUNCH(...) do { g_launches.fetch_add(1, std::memory_order_relaxed); hipLaunchKernelGGL(__VA_ARGS__); HIP_TRY(hipGetLastError()); } while (0)

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(RENI_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t al1k(size_t x) { return (x + 1023) & ~(size_t)1023; }

// (dtype, H, L) combinations served by the register-persistent training kernel k_reni_train_bf16
bool has_persistent(int dtype, int H, int L) {
  return dtype == RENI_BF16 && H == 128 && L >= 1 && L <= 5;
}
// k_reni_wide256 (round 5): the persistent chain at H = 256 for the calls that carry no weight gradient
// (FiLM, round 6: the forward-only calls -- inference, reni_film_forward / reni_film_model_forward -- of decoders whose per-image tables
//  fit the instance's LDS region, i.e. up to five hidden FiLM layers: the reference's default model, configs/default.py:9-13)
bool has_wide(int dtype, int H, int L, uint32_t flags, bool film, bool backward) {
  if (film && (backward || L > 5)) return false;
  return dtype == RENI_BF16 && H == 256 && L >= 2 && L <= reni::MAX_LAYERS - 1 && !(flags & RENI_NEED_DW);
}
// ... and its training form (MODE 2): the chain of a call WITH weight gradients -- it feeds k_dw_frag's fragment stream as
// k_reni_main's FRAG form does, and k_wide_head_dw takes the head's gradient
// (FiLM, round 6: EVERY backward call -- d(freq) / d(phase) come from the weight-gradient consumers, frozen decoder or not -- of decoders
//  with up to four hidden FiLM layers: the reference's default model)
bool has_wide_train(int dtype, int H, int L, uint32_t flags, bool film) {
  if (film) return dtype == RENI_BF16 && H == 256 && L >= 2 && L <= 4;
  return dtype == RENI_BF16 && H == 256 && L >= 2 && L <= reni::MAX_LAYERS - 1 && (flags & RENI_NEED_DW);
}

int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  return n;
}

struct GeoRt {  // run-time copy of reni::Geo<Pol,H>
  int img_hid, img_hf, img_hb, bias_hid, bias_head, lds_bytes, stash_layer_bytes, nks, nrb, head_bwd_ks;
};

template <class Pol, int H>
GeoRt geo_of() {
  using G = reni::Geo<Pol, H>;
  return {G::IMG_HID, G::IMG_HF, G::IMG_HB, G::BIAS_HID, G::BIAS_HEAD, G::LDS_BYTES, G::STASH_LAYER_BYTES,
          G::NKS, G::NRB, Pol::HEAD_BWD_KS};
}

bool geo_for(const reni_plan* p, GeoRt* g) {
  const int H = p->d.hidden_features;
  if (p->d.dtype == RENI_F32) {
    if (H == 32) *g = geo_of<reni::PolF32, 32>();
    else if (H == 64) *g = geo_of<reni::PolF32, 64>();
    else if (H == 128) *g = geo_of<reni::PolF32, 128>();
    else if (H == 256) *g = geo_of<reni::PolF32, 256>();
    else return false;
  } else {
    if (H == 32) *g = geo_of<reni::PolBF16, 32>();
    else if (H == 64) *g = geo_of<reni::PolBF16, 64>();
    else if (H == 128) *g = geo_of<reni::PolBF16, 128>();
    else if (H == 256) *g = geo_of<reni::PolBF16, 256>();
    else return false;
  }
  return true;
}

struct Layout {
  int tpi, n_tiles, nwg, persist, stream, kmax, frag;
  int wide_train;  // k_reni_wide256<2> runs the chain of this (H = 256, bf16, training) call: `persist` operands, the generic path's consumers
  // The training instance of the persistent H = 128 kernel runs: image runs, g_1 stream, a dW_1 kernel behind it.  THE definition: run_backward
  // and reni_path_info read it here.  (A call sees the same thing as `need_dw || fio`: a FiLM call always carries its FilmIO -- check_film,
  // and run_backward refuses a FiLM plan without one -- and MainArgs::need_dw mirrors RENI_NEED_DW.)
  int pdw;
  // Frozen-decoder call of a concat decoder on the persistent kernels (k_reni_train_bf16<128,false>, k_reni_wide256<1>): the packed W^T
  // images are 8 x the forward images' rounded weights, the rest of the factor rides on d loss / d y (MainArgs::gy_scale).  Why: with
  // the two images rounded independently -- bf16(W omega / 2 pi) forward, bf16(omega W) backward: the ratio 2 pi is no power of two --
  // the backward pass was the gradient of ANOTHER network than the forward pass evaluates, and a 200-step latent optimisation ended
  // 5 dB further from the reference's image than with consistent images (profiles/r06_trajectory.md).
  int consistent_bwd;
  size_t o_tflag, o_tlist, o_tcount, o_imgcos;  // RENI_WEIGHT_SPARSE (frozen persistent path): tile flags, the two lists, counts, per-image flags
  size_t o_pcnt, o_pscan, o_plist, o_nlive;     // RENI_WEIGHT_COMPACT: live pixels per tile, their exclusive scan, position -> pixel, per-image totals
  size_t o_skip;  // reni_train_step_rows: "the staged batch was not this call's batch" (k_tail_b writes, k_adam2 reads)
  size_t o_idxc, o_Zc, o_A, o_afrag, o_xconst, o_wimg, o_stash, o_dwp, o_dA_part, o_loss_part, o_img_loss, o_stats, o_dA, o_g1, o_dw1p, o_part2, o_mcol, o_ucol, o_dfp, o_dws, o_dfr, o_runimg, o_pruns, o_prunimg, total;
  int pkmax;  // image runs per workgroup of the persistent training kernel
  int nch, rt_chunk;
  size_t stash_per_wg, dwp_per_wg;
  unsigned fwd_off[reni::MAX_LAYERS + 2], bwd_off[reni::MAX_LAYERS + 2];
  size_t wimg_bytes;
};

// stage: which of the two copies of the per-batch prologue results (gathered rows, A_b, layer-0 operands, constant columns) the
// offsets point at -- reni_train_step_rows stages the NEXT batch's into the other copy while this step's are still being read.
Layout make_layout(const reni_plan* p, const GeoRt& g, int64_t B, int64_t P, uint32_t flags, bool backward,
                   bool allow_persist = true, int stage = 0) {
  Layout l;
  memset(&l, 0, sizeof(l));
  const int H = p->d.hidden_features, L = p->d.hidden_layers;
  l.tpi = (int)((P + 127) / 128);
  l.n_tiles = (int)(B * l.tpi);
  const bool film = p->d.conditioning == RENI_COND_FILM;
// (also without RENI_NEED_DW: the frozen-decoder instance k_reni_train_bf16<128, false>; and forward only: the
  // <128, false, true> instance without its statistics)
  // FiLM plans too (k_reni_train_bf16<.., FILM = true>): there the training instance also serves a frozen decoder, since
  // d(freq) / d(phase) need the same per-image weight-gradient sums
  l.wide_train = (backward && allow_persist && !p->no_persist && has_wide_train(p->d.dtype, H, L, flags, film)) ? 1 : 0;
  l.persist = (allow_persist && !p->no_persist && (has_persistent(p->d.dtype, H, L) || has_wide(p->d.dtype, H, L, flags, film, backward) || l.wide_train)) ? 1 : 0;
  l.pdw = (l.persist && !l.wide_train && (film || (flags & RENI_NEED_DW))) ? 1 : 0;
  // (every concat call on the persistent kernels: frozen-decoder and training calls at both widths -- the per-layer constants the weight
  //  gradients of a training call then carry are multiplied back where the per-workgroup partials are summed: reni::LayerScale; at
  //  H = 256 those partials are k_dw_frag's and k_wide_head_dw's, formed from the fragment stream the chain wrote with the same constants)
  l.consistent_bwd = (l.persist && !film && backward) ? 1 : 0;
  const int per_cu = (p->d.dtype == RENI_BF16 && !l.persist && H <= 128) ? 2 : 1;
  const int cap = device_cus() * per_cu;
  l.nwg = l.n_tiles < cap ? l.n_tiles : cap;
  if (l.pdw && l.n_tiles > cap) {
    // contiguous ranges: the longest range sets the time, so no more workgroups than give every one of them that length -- each
    // workgroup less is 0.33 MB of weight-gradient partials less to flush and to reduce (400 tiles: 200 x 2 instead of 256 x 1..2)
    const int rounds = (l.n_tiles + cap - 1) / cap;
    l.nwg = (l.n_tiles + rounds - 1) / rounds;
  }
  // (RENI_TRAIN_WG: fewer workgroups for the persistent training instances -- every one a longer contiguous range; the tests reach
  //  ranges of one, two and more tiles at shapes of a few tiles with it)
  if (l.pdw && p->train_wg > 0 && p->train_wg < l.nwg) l.nwg = p->train_wg;
  if (l.nwg < 1) l.nwg = 1;
  size_t o = 0;
  for (int st = 0; st < 2; ++st) {  // (two copies: see `stage`; 0.7 MB each at config 2)
    const bool mine = st == stage;
    if (mine) l.o_idxc = o;
    o += al256((size_t)B * 8);                   // the batch's row indices as the prologue saw them (checked by a staged step)
    if (mine) l.o_Zc = o;
    o += al256((size_t)B * p->d.ndims * 3 * 4);  // gathered latent rows (the *_rows entry points)
    if (mine) l.o_A = o;
    o += al256((size_t)B * H * 8 * 4);
    if (mine) l.o_afrag = o;
    if (l.persist) o += al256((size_t)B * (H / 32) * 1024);
    if (mine) l.o_xconst = o;
    o += al256((size_t)B * p->F_in * 4);
  }
  // weight images
  size_t w = 0;
  for (int i = 1; i <= L; ++i) { l.fwd_off[i] = (unsigned)w; w += al1k((size_t)g.img_hid + g.bias_hid); }
  l.fwd_off[L + 1] = (unsigned)w; w += al1k((size_t)g.img_hf + g.bias_head);
  for (int i = 1; i <= L; ++i) { l.bwd_off[i] = (unsigned)w; w += al1k((size_t)g.img_hid); }
  l.bwd_off[L + 1] = (unsigned)w; w += al1k((size_t)g.img_hb);
  l.wimg_bytes = w;
  w += 8192;  // the training kernel's LDS-DMA copies whole 3 KB groups, a whole number per wave: up to 4 KB of over-read behind an image
  l.o_wimg = o; o += al256(w);
  l.o_skip = o; o += 256;
  l.o_img_loss = o; o += al256((size_t)B * 16 * 4);
  l.o_stats = o; o += al256((size_t)B * 16 * 4);
  if (backward) {
    // (the frozen-decoder instance of the persistent kernel works on two tiles per workgroup)
    l.stash_per_wg = (size_t)(L + 1) * g.stash_layer_bytes * ((l.persist && !l.pdw && !l.wide_train) ? 2 : 1);
    // (H = 256 bf16 training: the fragment stream -- every tile's phase stash stays for k_dw_frag)
    l.frag = (p->d.dtype == RENI_BF16 && H == 256 && L >= 1 && (film || (flags & RENI_NEED_DW))) ? 1 : 0;
    // (fp32, concat: k_dw_frag32 -- fp32 fragments; the per-tile += of a 256 x 256 partial it replaces ran at 8 M samples/s)
    if (p->d.dtype == RENI_F32 && H == 256 && L >= 1 && !film && (flags & RENI_NEED_DW)) l.frag = 2;
    l.o_stash = o; o += al256(l.stash_per_wg * (l.frag ? (size_t)l.n_tiles : (size_t)l.nwg));
    l.dwp_per_wg = (flags & RENI_NEED_DW) ? (size_t)(p->n_params - p->n_first) : 0;
    // (the persistent training instances: every workgroup's slot starts on a 256-byte line -- the L0X instance flushes, and the quad-row
    //  reducer loads, 16 bytes at a time; the stride is the only thing that changes for the others)
    if (l.pdw) l.dwp_per_wg = (l.dwp_per_wg + 63) & ~(size_t)63;
    // image runs of the persistent training kernel: a workgroup's contiguous tile range meets at most this many images
    l.pkmax = ((l.n_tiles + l.nwg - 1) / l.nwg + l.tpi - 1) / l.tpi + 1;
    // (FiLM on the persistent path: one partial slot per image RUN -- the accumulators leave the registers with the image)
    const size_t run_slots = (film && l.persist && !l.wide_train) ? (size_t)l.pkmax : 1;   // (wide_train: the stream path's bookkeeping, below)
    l.o_dwp = o; o += al256(l.dwp_per_wg * 4 * l.nwg * run_slots);
    // (the persistent training instance keeps layer-0 dA on chip: image runs below, no per-tile partials)
    l.o_dA_part = o; if (!l.pdw) o += al256((size_t)l.n_tiles * H * 8 * 4);
    l.o_tflag = l.o_tlist = l.o_tcount = l.o_imgcos = o;
    if (!film && !(flags & RENI_NEED_DW)) {  // frozen concat decoder (sized whether or not the call sets RENI_WEIGHT_SPARSE: the layout does not depend on it)
      l.o_tflag = o; o += al256((size_t)l.n_tiles * 4);
      l.o_tlist = o; o += al256((size_t)2 * l.n_tiles * 4);
      l.o_tcount = o; o += 256;
      l.o_imgcos = o; o += al256((size_t)B * 4);
      l.o_pcnt = o; o += al256((size_t)l.n_tiles * 4);
      l.o_pscan = o; o += al256((size_t)(l.n_tiles + 1) * 4);
      l.o_nlive = o; o += al256((size_t)B * 4);
      l.o_plist = o; o += al256((size_t)B * P * 4);
    }
    l.o_loss_part = o; o += al256((size_t)l.n_tiles * 4 * 16 * 4);
    l.o_dA = o; o += al256((size_t)B * H * 8 * 4);
    // k_reni_dw1 runs two workgroups per CU with partials of its own: [2 nwg][H * H + H]
    l.o_dw1p = o; if (l.pdw && (flags & RENI_NEED_DW)) o += al256((size_t)2 * l.nwg * run_slots * ((size_t)H * H + H) * 4);
    // (g_1 stream [position in a workgroup's tile range][workgroup][H / 16 x 4 KB]: ceil(n_tiles / nwg) positions)
    l.o_g1 = o; if (l.pdw) o += al256((size_t)((l.n_tiles + l.nwg - 1) / l.nwg) * l.nwg * (H / 16) * 4096);
    l.o_pruns = o; if (l.pdw) o += al256((size_t)l.nwg * l.pkmax * (H * 8 + 16) * 4);
    // (FiLM: + the run tags of k_reni_dw1's 2 nwg workgroups behind the training kernel's)
    l.o_prunimg = o; if (l.pdw) o += al256((size_t)l.nwg * l.pkmax * (film ? 3 : 1) * 4);
    // tiles per stage-A block of the per-image tile reduction.  Independent of the batch on purpose: an image's sums are then
    // formed in the same order whatever batch it is part of (its gradient does not depend on its neighbours, bit for bit).
    l.rt_chunk = reni::RT_CHUNK;
    l.nch = (l.tpi + l.rt_chunk - 1) / l.rt_chunk;
    l.o_part2 = o; o += al256((size_t)B * l.nch * (H * 8 + 16) * 4);
    l.o_mcol = o; o += al256((size_t)B * p->F_in * 4);
    l.o_ucol = o; o += al256((size_t)B * p->d.ndims * 3 * 4);
    l.o_dfp = o; if (film && !l.persist) o += al256((size_t)l.n_tiles * L * 2 * H * 4);
    // bf16 stream path (k_dw_stream): H = 256 training, and FiLM at H = 128 / 256 (also with a frozen decoder: it is
    // how d(freq), d(phase) are obtained).  One record per (layer, tile, round) = the g image and the h image.
    const bool can = p->d.dtype == RENI_BF16 && L >= 1;
    l.stream = can && (H == 128 || H == 256) && (!l.persist || l.wide_train) && (film || (flags & RENI_NEED_DW)) ? 1 : 0;
    l.o_dws = o;
    l.o_dfr = o;
    l.o_runimg = o;
    if (l.frag == 2) o += al256((size_t)L * l.n_tiles * g.stash_layer_bytes);
    if (l.stream) {
      const int nround = (H == 256) ? 2 : 1;
      const size_t rec = (size_t)2 * (H == 256 ? 36864 : 34816);
      o += al256(l.frag ? (size_t)L * l.n_tiles * g.stash_layer_bytes + (l.wide_train ? (size_t)l.n_tiles * 2048 : 0)  // (+ the g_y stream: k_wide_head_dw)
                        : (size_t)L * l.n_tiles * nround * rec);
      const long long nrec = (long long)l.n_tiles * nround;
      const long long range = (nrec + l.nwg - 1) / l.nwg;
      l.kmax = (int)(range / ((long long)l.tpi * nround)) + 2;
      if (film) {
        l.o_dfr = o; o += al256((size_t)l.nwg * l.kmax * L * 2 * H * 4);
        l.o_runimg = o; o += al256((size_t)l.nwg * l.kmax * 4);
      }
    }
    if (film && l.persist && !l.wide_train) {  // d(freq), d(phase) per image run: [3 nwg pkmax][L][2][H], tagged by the run tags above
      l.o_dfr = o; o += al256((size_t)3 * l.nwg * l.pkmax * L * 2 * H * 4);
      l.o_runimg = l.o_prunimg;
    }
  }
  l.total = o;
  return l;
}

// the layout every backward call of this shape uses and reni_workspace_bytes sizes: RENI_NEED_DZ set, so that one buffer serves every call
Layout backward_layout(const reni_plan* p, const GeoRt& g, int64_t B, int64_t P, uint32_t flags) {
  return make_layout(p, g, B, P, flags | RENI_NEED_DZ, true, true);
}

// ---- optional HIP-event timing of the fused main kernel (reni_profile_*) --------------------
// kind of the timed launch: the fused forward+loss+backward pass, RENITestLoss's statistics pass, or plain inference
// (3: k_reni_l0_ring / k_reni_dw1_ring / k_reni_dw1 behind the training kernel; 4: the weight-gradient consumers of the fragment / operand
//  streams -- k_dw_frag, k_dw_frag32, k_dw_stream, k_wide_head_dw: bench.py's roofline.frac divides by the run time of EVERY kernel that
//  performs the step's FLOPs)
//  5: the data-parallel exchange inside reni_train_step_rows_dp (RCCL all-reduce on the caller's stream)
enum { PROF_FWD_BWD = 0, PROF_STATS = 1, PROF_FWD = 2, PROF_DW1 = 3, PROF_DWS = 4, PROF_COMM = 5 };
struct EvPair { hipEvent_t a, b; int kind; };
bool g_prof_on = false;
std::vector<EvPair> g_prof_pool;   // every pair ever created (reused after a reset)
size_t g_prof_used = 0;

bool prof_begin(hipStream_t s, EvPair* out, int kind) {
  if (!g_prof_on) return false;
  if (g_prof_used == g_prof_pool.size()) {
    EvPair e;
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return false;
    g_prof_pool.push_back(e);
  }
  g_prof_pool[g_prof_used].kind = kind;
  *out = g_prof_pool[g_prof_used++];
  return hipEventRecord(out->a, s) == hipSuccess;
}

// One timed launch: the profile pair around whatever `go` enqueues on `s` (a kernel of this translation unit, or another unit's host
// launcher), the launch count, the error check, the end event.
template <class Go>
int timed_launch(hipStream_t s, int kind, const char* what, Go go) {
  EvPair ev;
  const bool timed = prof_begin(s, &ev, kind);
  g_launches.fetch_add(1, std::memory_order_relaxed);
  const hipError_t e = go();
  if (e != hipSuccess) return fail(RENI_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
  if (timed) HIP_TRY(hipEventRecord(ev.b, s));
  return RENI_OK;
}
// ... of a MainArgs kernel of this translation unit: the dynamic-LDS attribute first, when the kernel asks for any
int timed_launch(void (*fn)(const reni::MainArgs), int grid, int block, int lds, hipStream_t s, const reni::MainArgs& a, int kind) {
  if (lds) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  return timed_launch(s, kind, "kernel", [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(block), lds, s, a); return hipGetLastError(); });
}

// the head / loss configuration of every shipped FIT_DECODER run (the SPEC instances' compile-time constants): linear head, tanh,
// WeightedMSE, no output image.  spec_head: what the plan and the flags decide of it (reni_path_info reports from that part alone).
bool spec_head(bool need_dw, int last_linear, int act) { return need_dw && last_linear && act == RENI_ACT_TANH; }
bool train_spec(const reni::MainArgs& a, bool stats) {
  return !stats && spec_head(a.need_dw, a.last_linear, a.act) && a.loss_kind == 0 && a.out == nullptr;
}

int launch_train(const reni_plan* p, const reni::MainArgs& a, int nwg, hipStream_t s, bool stats = false, bool l0x = false) {
  using G = reni::GeoP<128>;
  const int kind = !stats ? PROF_FWD_BWD : a.target ? PROF_STATS : PROF_FWD;
  const bool film = p->d.conditioning == RENI_COND_FILM;
  if (p->d.hidden_features == 256) {  // k_reni_wide256: forward / statistics (stats), the frozen-decoder pass, or the training form
    if (film && p->d.hidden_layers > (stats ? reni::wide256_film_max_layers() : reni::wide256_film_train_max_layers()))
      return fail(RENI_EINVAL, "internal: k_reni_wide256's FiLM instances hold <= 5 (forward) / <= 4 (training form) hidden layers' tables");
    if ((a.need_dw || film) && !stats && a.gfs == nullptr) return fail(RENI_EINVAL, "internal: the training form of k_reni_wide256 needs the fragment stream");
    const int mode = film ? (stats ? 3 : 4) : stats ? 0 : a.need_dw ? 2 : 1;
    return timed_launch(s, kind, "k_reni_wide256", [&] { return reni::launch_wide256(mode, a, nwg, s); });
  }
  if (!has_persistent(p->d.dtype, p->d.hidden_features, p->d.hidden_layers))
    return fail(RENI_EUNSUPPORTED, "no persistent training kernel for this configuration");
  if (p->d.hidden_layers >= 2 && (a.fwd_off[2] - a.fwd_off[1] != G::FWD_STRIDE || a.bwd_off[2] - a.bwd_off[1] != G::BWD_STRIDE))
    return fail(RENI_EINVAL, "packed weight images are not at the stride the persistent kernels assume");
  const bool spec = train_spec(a, stats);
  const int pairs = (a.n_tiles + 1) / 2, nwg2 = nwg < pairs ? nwg : pairs;  // (the forward-only instances: eight waves on two tiles)
  if (film)  // (the training instance also with a frozen decoder: see make_layout; 2: its SPEC form, as for the concat decoder below)
    return timed_launch(s, kind, "FiLM persistent kernel", [&] { return reni::launch_train_film(stats ? 1 : spec ? 2 : 0, a, stats ? nwg2 : nwg, s); });
  if (l0x && !spec) return fail(RENI_EINVAL, "internal: the L0X form exists for the SPEC instance only");
  void (*fn)(const reni::MainArgs) = stats ? reni::k_reni_train_bf16<128, false, true>
                                     : l0x ? reni::k_reni_train_bf16<128, true, false, false, true, true>
                                     : spec ? reni::k_reni_train_bf16<128, true, false, false, true>
                                     : a.need_dw ? reni::k_reni_train_bf16<128, true> : reni::k_reni_train_bf16<128, false>;
  const int lacc = spec ? G::LACC_BYTES + (l0x ? G::L0X_TW_BYTES : 0) : 0;  // the SPEC instance's per-lane accumulators (L0X: + the weight rows)
#ifdef RENI_TRACE
  const int LDS = G::LDS_BYTES + lacc + 4096;  // + the cycle trace's LDS words
#else
  const int LDS = G::LDS_BYTES + lacc;
#endif
  if (a.need_dw && !stats) return timed_launch(fn, nwg, 256, LDS, s, a, kind);
  return timed_launch(fn, nwg2, 512, LDS, s, a, kind);
}

// k_reni_dw1_ring's preconditions (reni_dev_train.inc): concatenation decoder, whole tiles, a tile's directions one 16-byte
// aligned run.  Decided ONCE per call (bwd_path) and handed to both the launch and the layer-1 reduction, whose slot
// count depends on it (ring: one partial per range, k_reni_dw1: two).
// Every run-time predicate here is two functions: *_plan_ok -- what the plan, the shape and the flags decide, all reni_path_info has --
// and *_call_ok -- what the call's pointers and loss add.  run_backward takes plan && call.
bool dw1_ring_plan_ok(const reni_plan* p, int64_t P) { return !p->dw1_old && p->d.conditioning != RENI_COND_FILM && P % 128 == 0; }
bool dw1_ring_call_ok(const reni::MainArgs& a) { return (((uintptr_t)a.D | (uintptr_t)(a.d_bstride * 4)) & 15) == 0; }
int dw1_slots(bool ring, int nwg) { return ring ? nwg : 2 * nwg; }
// The L0X split (round 5): the training kernel ends a tile with layer 2's step and k_reni_l0_ring takes layer 1's dX GEMM, g_0, the
// layer-0 dA and dW_1 from the g_1 stream.  Needs the ring's preconditions, the SPEC head / loss configuration and an odd number
// (>= 3) of hidden layers (the L0X instance's step pairing); every other call keeps round 4's kernels.
// (and target / weight rows the instance can fetch by LDS-DMA: [P][3] interleaved or channel-planar, 16-byte aligned runs)
bool l0x_rows_ok(const float* base, long long s0, long long s1, long long s2) {
  if (((uintptr_t)base | (uintptr_t)(s0 * 4)) & 15) return false;
  if (s1 == 3 && s2 == 1) return true;                     // interleaved: one 1536-byte run per tile
  return s1 == 1 && ((uintptr_t)(s2 * 4) & 15) == 0;      // planar: three 512-byte runs
}
bool l0x_plan_ok(const reni_plan* p, const Layout& l, int64_t P, uint32_t flags) {
  const int L = p->d.hidden_layers;
  return l.pdw && !p->no_l0x && dw1_ring_plan_ok(p, P) && spec_head(flags & RENI_NEED_DW, p->d.last_layer_linear, p->d.output_activation) &&
         L >= 3 && (L & 1) == 1;
}
bool l0x_call_ok(const reni::MainArgs& a) {
  return dw1_ring_call_ok(a) && train_spec(a, false) && l0x_rows_ok(a.target, a.ts0, a.ts1, a.ts2) && l0x_rows_ok(a.weight, a.ws0, a.ws1, a.ws2);
}
// "a side stream is allowed for this plan" -- not "this call forks": BwdPath::fork also needs !l0x and enough tiles per workgroup
bool side_stream_plan_ok(const reni_plan* p, const Layout& l) { return l.pdw && !p->no_side_stream; }

// dW_1 / db_1 from the stored g_1 stream (same grid: it fills the layer-1 slot of the same partials)
int launch_dw1(const reni::MainArgs& a, int nwg, bool ring, hipStream_t s, bool l0x = false) {
#ifdef RENI_TRACE_DW1
  constexpr int TRACE = 8192;  // + the cycle trace's LDS words (k_reni_l0_ring: build with -DRENI_L0_NSLOT=3)
#else
  constexpr int TRACE = 0;
#endif
  if (l0x)  // layer 0's backward + dW_1 (k_reni_l0_ring): one workgroup per range of the L0X training instance
    return timed_launch(reni::k_reni_l0_ring<128>, nwg, reni::L0Ring::THREADS, reni::L0Ring::LDS_BYTES + TRACE, s, a, PROF_DW1);
  if (a.film != nullptr) return timed_launch(s, PROF_DW1, "k_reni_dw1 (FiLM)", [&] { return reni::launch_dw1_film(a, 2 * nwg, s); });
  if (ring)  // one workgroup per range, inputs through an LDS-DMA ring (k_reni_dw1_ring)
    return timed_launch(reni::k_reni_dw1_ring<128>, nwg, reni::Dw1Ring::THREADS, reni::Dw1Ring::LDS_BYTES + TRACE, s, a, PROF_DW1);
  // two workgroups per range of the training kernel = two per CU (it is latency-bound at one)
  return timed_launch(reni::k_reni_dw1<128>, 2 * nwg, 256, 2 * reni::TS_BYTES + TRACE, s, a, PROF_DW1);
}

// k_reduce_partials: elements [lo, hi) of `nslot` per-workgroup partials (`per_wg` floats apart; `valid`: a tag per slot, or NULL = every
// slot counts) summed in a fixed order into out[lo .. hi)
// (quad_H > 0: the hidden layers' H x H slices are in the quad-row layout -- BwdPath::part_quad -- and H = quad_H: k_reduce_partials_quad)
int reduce_partials(const float* part, size_t per_wg, int nslot, float* out, int lo, int hi, const int* valid, const reni::LayerScale& lsc,
                    hipStream_t s, int quad_H = 0) {
  if (quad_H > 0) {
    if (valid != nullptr || (per_wg & 3) || (lo & 3) || ((uintptr_t)part & 15)) return fail(RENI_EINVAL, "internal: quad-row partials need untagged, 16-byte aligned slots");
    RENI_LAUNCH(reni::k_reduce_partials_quad, dim3((unsigned)((hi - lo + reni::QUAD_BLK_WORDS - 1) / reni::QUAD_BLK_WORDS)), dim3(256), 0, s, part, per_wg, nslot, out, lo, hi, quad_H, lsc);
    return RENI_OK;
  }
  RENI_LAUNCH(reni::k_reduce_partials, dim3((unsigned)((hi - lo + 63) / 64)), dim3(256), 0, s, part, per_wg, nslot, out, lo, hi, valid, lsc);
  return RENI_OK;
}

// A side stream and three events per device: the per-image epilogue (tile reductions, latent tails, loss) of the
// persistent path runs beside k_reni_dw1, which leaves 40 % of every CU's registers and 60 % of its LDS free.
struct SideStream { hipStream_t s; hipEvent_t ev[3]; bool ok; };
std::mutex g_side_mu;
SideStream* side_stream() {
  static SideStream tab[16];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  SideStream& t = tab[dev];
  if (!t.ok) {
    if (hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    for (int i = 0; i < 3; ++i)
      if (hipEventCreateWithFlags(&t.ev[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    t.ok = true;
  }
  return &t;
}

int launch_main(const reni_plan* p, int mode, const reni::MainArgs& a, int nwg, hipStream_t s) {
  const int H = p->d.hidden_features;
  const bool film = p->d.conditioning == RENI_COND_FILM, f32 = p->d.dtype == RENI_F32;
  return timed_launch(s, mode == reni::MODE_FWD_BWD ? PROF_FWD_BWD : mode == reni::MODE_STATS ? PROF_STATS : PROF_FWD, "fused kernel", [&] {
    if (f32) return film ? reni::launch_film_f32(H, mode, a, nwg, s) : reni::launch_main_f32(H, mode, a, nwg, s);
    return film ? reni::launch_film_bf16(H, mode, a, nwg, s) : reni::launch_main_bf16(H, mode, a, nwg, s);
  });
}

// Every compute entry point runs on the device that owns its buffers and leaves the caller's current device as
// it found it (the library lives inside a PyTorch process, whose current device is process-wide state).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  int enter(const void* ptr) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess) {
      if (hipGetDevice(&prev) == hipSuccess && prev != at.device) {
        HIP_TRY(hipSetDevice(at.device));
        switched = true;
      }
    } else {
      (void)hipGetLastError();
    }
    return RENI_OK;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// prologue shared by all entry points: A_b / xconst and the packed weight images
int run_prologue(const reni_plan* p, const GeoRt& g, const Layout& l, int64_t B, const float* Z,
                 const float* params, char* ws, bool backward, hipStream_t s, const int64_t* idx = nullptr,
                 const float* film_A = nullptr, int64_t n_rows = 0, bool shared_img = false) {
  // shared_img (BwdPath::l0x): the L0X training instance reads ONE image per hidden layer in both passes -- the forward images of the
  // hidden layers are written in the shared cell order (PackDesc::swz) and the W^T images of layers >= 2 are not packed at all
  // (layer 1's stays: k_reni_l0_ring's resident operand; the head's: resident in the training kernel)
  const int H = p->d.hidden_features, L = p->d.hidden_layers;
  const bool film = p->d.conditioning == RENI_COND_FILM;
  reni::PrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  if (!film) {  // FiLM: the caller supplies the per-image affine map
    pa.idx = (const long long*)idx; pa.n_rows = (long long)n_rows; pa.Zc = (float*)(ws + l.o_Zc);
    pa.idx_copy = idx ? (long long*)(ws + l.o_idxc) : nullptr;
    pa.Z = Z; pa.W0 = params; pa.b0 = params + (size_t)H * p->F_in;
    pa.xconst = (float*)(ws + l.o_xconst); pa.A = (float*)(ws + l.o_A);
    pa.afrag = l.persist ? ws + l.o_afrag : nullptr;
    pa.afrag_scale = p->d.first_omega_0 * 0.15915494309189535f;
    pa.eq = p->d.equivariance; pa.nd = p->d.ndims; pa.F_in = p->F_in; pa.H = H;
  }

  reni::PackArgs ka;
  ka.params = params; ka.wimg = ws + l.o_wimg;
  int n = 0;
  for (int i = 1; i <= L + 1; ++i) {
    const bool head = (i == L + 1);
    reni::PackDesc d;
    d.src = p->p_off_w[i]; d.bias_src = p->p_off_b[i]; d.dst = l.fwd_off[i];
    d.M = head ? 3 : H; d.K = H; d.transposed = 0; d.swz = (shared_img && !head) ? 1 : 0;
    d.nrb = head ? 1 : g.nrb; d.nks = g.nks;
    d.bias_n = head ? 3 : H; d.bias_n_pad = head ? 32 : H;
    // persistent training kernel: omega / 2 pi rides on the hidden forward images (its sine argument is in
    // revolutions) and omega on the W^T images (the factor of d sin(omega a) / da of the layer below)
    // (FiLM: freq / 2 pi and phase / 2 pi are per image -- the kernel's tables -- so the forward images stay plain, and the
    // W^T images of the layers whose product meets a table entry carry the 2 pi back)
    d.scale = (l.persist && !head && !film) ? p->d.hidden_omega_0 * 0.15915494309189535f : 1.f;
    // (FiLM on k_reni_wide256: the hidden forward images and biases carry the 1 / 2 pi of the angle's frequency term, its tables the plain
    //  frequency -- reni_dev_wide.inc)
    if (film && l.persist && H == 256 && !head) d.scale = 0.15915494309189535f;
    ka.d[n++] = d;
    if (backward && !(shared_img && i >= 2 && !head)) {
      d.dst = l.bwd_off[i]; d.transposed = 1; d.swz = 0;
      d.nrb = g.nrb; d.nks = head ? g.head_bwd_ks : g.nks;
      d.bias_n = 0; d.bias_n_pad = 0;
      d.scale = !l.persist ? 1.f : film ? ((i == 1 || H == 256) ? 1.f : 6.283185307179586f) : (i == 1 ? p->d.first_omega_0 : p->d.hidden_omega_0);
      // frozen-decoder calls (Layout::consistent_bwd): 8 x the scale of the FORWARD image -- the same fp32 product times a power of two,
      // so the bf16 rounding gives the same mantissas and the W^T image is exactly 8 x the transpose of the forward image
      if (l.consistent_bwd) d.scale = (head ? 1.f : p->d.hidden_omega_0 * 0.15915494309189535f) * 8.f;
      ka.d[n++] = d;
    }
  }
  const bool f32 = p->d.dtype == RENI_F32;
  if (!film || l.persist) {
    // ONE launch: k_prep_image's blocks, then k_pack's (k_prologue)
    // (FiLM on the persistent kernels: the caller's map A_b as layer-0 MFMA operands, in revolutions, instead of k_prep_image)
    reni::PrologueArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.prep = pa;
    ga.prep_gy = (H + 7) / 8; ga.n_prep = (int)B * ga.prep_gy; ga.pack_gx = f32 ? 16 : 8;
    if (film) {
      ga.film_A = film_A; ga.film_afrag = ws + l.o_afrag; ga.film_scale = 0.15915494309189535f; ga.film_B = (int)B;
      ga.prep.H = H; ga.n_prep = (int)((B * H + 255) / 256);
    }
    const unsigned grid = (unsigned)(ga.n_prep + ga.pack_gx * n);
    if (f32) RENI_LAUNCH(reni::k_prologue<reni::PolF32>, dim3(grid), dim3(256), (size_t)p->F_in * 4, s, ga, ka);
    else RENI_LAUNCH(reni::k_prologue<reni::PolBF16>, dim3(grid), dim3(256), (size_t)p->F_in * 4, s, ga, ka);
    return RENI_OK;
  }
  if (f32) RENI_LAUNCH(reni::k_pack<reni::PolF32>, dim3(16, n), dim3(256), 0, s, ka);
  else RENI_LAUNCH(reni::k_pack<reni::PolBF16>, dim3(8, n), dim3(256), 0, s, ka);
  return RENI_OK;
}

void fill_main_args(reni::MainArgs& a, const reni_plan* p, const Layout& l, int64_t B, int64_t P,
                    const float* Z, const float* D, int64_t dbs, char* ws) {
  memset(&a, 0, sizeof(a));
  a.B = (int)B; a.P = (int)P; a.tiles_per_image = l.tpi; a.n_tiles = l.n_tiles;
  a.L = p->d.hidden_layers; a.last_linear = p->d.last_layer_linear; a.act = p->d.output_activation;
  a.w_first = p->d.first_omega_0; a.w_hidden = p->d.hidden_omega_0;
  a.gy_scale = 1.f;
  if (l.consistent_bwd) {  // (2 pi)^L omega_first / 8^(L+1): see Layout::consistent_bwd (L = 5, omega = 30: 1.1207)
    double sc = (double)p->d.first_omega_0 / 8.0;
    for (int i = 0; i < p->d.hidden_layers; ++i) sc *= 6.283185307179586 / 8.0;
    a.gy_scale = (float)sc;
  }
  a.Z = Z; a.D = D; a.d_bstride = dbs;
  a.Apre = (const float*)(ws + l.o_A);
  a.afrag = ws + l.o_afrag;
  a.wimg = ws + l.o_wimg;
  for (int i = 0; i < reni::MAX_LAYERS + 2; ++i) {
    a.fwd_off[i] = l.fwd_off[i]; a.bwd_off[i] = l.bwd_off[i];
    a.p_off_w[i] = p->p_off_w[i] >= (unsigned)p->n_first ? p->p_off_w[i] - (unsigned)p->n_first : 0;
    a.p_off_b[i] = p->p_off_b[i] >= (unsigned)p->n_first ? p->p_off_b[i] - (unsigned)p->n_first : 0;
  }
  a.stash = ws + l.o_stash; a.stash_per_wg = l.stash_per_wg;
  a.dwp = (float*)(ws + l.o_dwp); a.dwp_per_wg = l.dwp_per_wg;
  a.dA_part = (float*)(ws + l.o_dA_part);
  a.loss_part = (float*)(ws + l.o_loss_part);
  a.g1 = ws + l.o_g1;
  a.dw1p = (float*)(ws + l.o_dw1p);
  a.stats = (const float*)(ws + l.o_stats);
  a.n_first = (unsigned)p->n_first;
  a.dfp_part = (float*)(ws + l.o_dfp);
  a.dws = l.stream ? ws + l.o_dws : nullptr;
  a.gfs = l.frag ? ws + l.o_dws : nullptr;
  a.dfr = (float*)(ws + l.o_dfr);
  a.run_image = (int*)(ws + l.o_runimg);
  a.kmax = l.kmax;
  a.pruns = (float*)(ws + l.o_pruns);
  a.prun_image = (int*)(ws + l.o_prunimg);
  a.pkmax = l.pkmax;
  a.nwg_main = l.nwg;
}

int check_common(const reni_plan* p, int64_t B, int64_t P, const void* Z, const void* D, const void* params,
                 const void* ws) {
  if (!p) return fail(RENI_EINVAL, "plan is NULL");
  if (B < 1 || P < 1) return fail(RENI_EINVAL, "B=%lld P=%lld must be >= 1", (long long)B, (long long)P);
  if (B * ((P + 127) / 128) > 0x3fffffffLL || P > 0x3fffffffLL) return fail(RENI_EINVAL, "problem too large");
  if (!Z || !D || !params) return fail(RENI_EINVAL, "Z, D and params must be non-NULL");
  if (!ws) return fail(RENI_EWORKSPACE, "workspace is NULL");
  if (((uintptr_t)ws & 255) != 0) return fail(RENI_EINVAL, "workspace must be 256-byte aligned");
  return RENI_OK;
}

// FiLM entry points: the caller owns the per-image glue (layer-0 affine map, mapping network)
struct FilmIO {
  const float* A = nullptr;     // [B][H][8]
  const float* film = nullptr;  // [B][L][2][H]
  float* dA = nullptr;          // [B][H][8]
  float* dfilm = nullptr;       // [B][L][2][H]
  const float* Zp = nullptr;    // reni_film_model_*: latents for the prior term of RENITestLoss (else NULL)
  float alpha = 0.f;
  int64_t nz = 0;
  int keep_first = 0;           // reni_film_model_*: the caller fills the first layer's gradient slot itself
};

int check_film(const reni_plan* p, const FilmIO* f, bool backward) {
  if (!p) return fail(RENI_EINVAL, "plan is NULL");
  if (p->d.conditioning != RENI_COND_FILM) return fail(RENI_EINVAL, "plan was not created with RENI_COND_FILM");
  if (!f->A) return fail(RENI_EINVAL, "A is NULL");
  if (p->d.hidden_layers > 0 && !f->film) return fail(RENI_EINVAL, "film is NULL");
  if (backward && (!f->dA || (p->d.hidden_layers > 0 && !f->dfilm))) return fail(RENI_EINVAL, "dA / dfilm is NULL");
  return RENI_OK;
}

// reni_train_step_rows: the optimiser step and the next step's prologue fused into the call (see the entry point)
int rccl_allreduce_inplace(void* comm, float* buf, size_t n, hipStream_t s);  // (defined with the RCCL binding, below)
int rccl_allreduce_max_i32(void* comm, int* buf, size_t n, hipStream_t s);

// RENI_WEIGHT_SPARSE / _COMPACT: the tile and pixel lists of a masked weight, in a CALLER-owned buffer (reni_weight_lists_build):
// the mask of a FIT_LATENT run is constant over its 2 400 epochs (configs/experiment.yaml:47-48), the lists were rebuilt from an
// 8 MB weight read by two or three dependent launches in every call.  Layout = a function of (B, P) only.
struct ListLayout { size_t o_hdr, o_tflag, o_tlist, o_tcount, o_imgcos, o_pcnt, o_pscan, o_nlive, o_plist, o_zstats, total; };
ListLayout make_list_layout(int64_t B, int64_t P) {
  ListLayout l;
  const size_t n_tiles = (size_t)(B * ((P + 127) / 128));
  size_t o = 0;
  l.o_hdr = o; o += 256;                                  // [B, P, flags, magic] as built (for the caller's own checks and for debugging)
  l.o_tflag = o; o += al256(n_tiles * 4);
  l.o_tlist = o; o += al256(2 * n_tiles * 4);
  l.o_tcount = o; o += 256;
  l.o_imgcos = o; o += al256((size_t)B * 4);
  l.o_pcnt = o; o += al256(n_tiles * 4);
  l.o_pscan = o; o += al256((n_tiles + 1) * 4);
  l.o_nlive = o; o += al256((size_t)B * 4);
  l.o_plist = o; o += al256((size_t)B * P * 4);
  l.o_zstats = o; o += al256((size_t)B * 16 * 4);         // zero cosine coefficients [B][16] (RENI_WEIGHT_COS_CONSTANT)
  l.total = o;
  return l;
}
constexpr long long LIST_MAGIC = 0x52454e494c495354ll;  // "RENILIST"
// where the lists live: in the call's workspace (Layout) or in the caller's buffer (ListLayout) -- the same member names in both
struct ListDst { int *tflag, *imgcos, *tlist, *tcount, *pcnt, *pscan, *nlive, *plist; };
template <class L>
ListDst list_dst(char* base, const L& l) {
  return {(int*)(base + l.o_tflag), (int*)(base + l.o_imgcos), (int*)(base + l.o_tlist), (int*)(base + l.o_tcount),
          (int*)(base + l.o_pcnt), (int*)(base + l.o_pscan), (int*)(base + l.o_nlive), (int*)(base + l.o_plist)};
}
// ... and the ONE place that builds them (run_backward per call, reni_weight_lists_build once per mask: the cached latent step is
// bit-equal to the rebuilding one because both issue these launches): tile flags -> the two tile lists and their counts
// (-> RENI_WEIGHT_COMPACT: position -> pixel)
int build_weight_lists(const float* weight, const int64_t* wst, int64_t P, int tpi, int n_tiles, bool compact, const ListDst& d,
                       hipStream_t s) {
  RENI_LAUNCH(reni::k_tile_flags, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, weight, (long long)wst[0], (long long)wst[1],
              (long long)wst[2], (int)P, tpi, n_tiles, d.tflag, d.imgcos, compact ? d.pcnt : (int*)nullptr);
  RENI_LAUNCH(reni::k_tile_compact, dim3(1), dim3(1024), 0, s, d.tflag, (const int*)d.imgcos, tpi, n_tiles, d.tlist, d.tlist + n_tiles,
              d.tcount, compact ? (const int*)d.pcnt : (const int*)nullptr, (int)P, d.pscan, d.nlive);
  if (compact) {
    RENI_LAUNCH(reni::k_pix_scatter, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, weight, (long long)wst[0], (long long)wst[1],
                (long long)wst[2], (int)P, tpi, n_tiles, (const int*)d.imgcos, (const int*)d.pscan, d.plist);
  }
  return RENI_OK;
}
struct WeightLists { const char* buf; uint32_t flags; };   // handed to run_backward by reni_latent_step_rows_cached
// What reni_weight_lists_build built where, on the HOST (ADVICE r05: the header in the buffer is device memory, a cached step cannot read
// it without a synchronisation; lists built for another B, P or mode would be read out of bounds).  The last 64 builds, newest first.
struct ListRecord { const void* buf; int64_t B, P; uint32_t mode; };
std::mutex g_lists_mu;
std::vector<ListRecord> g_lists;
void lists_remember(const void* buf, int64_t B, int64_t P, uint32_t mode) {
  std::lock_guard<std::mutex> lk(g_lists_mu);
  for (size_t i = 0; i < g_lists.size(); ++i)
    if (g_lists[i].buf == buf) { g_lists.erase(g_lists.begin() + (long)i); break; }
  g_lists.insert(g_lists.begin(), ListRecord{buf, B, P, mode});
  if (g_lists.size() > 64) g_lists.pop_back();
}
// 0: built for exactly this; 1: unknown buffer; 2: built for another shape / mode
int lists_check(const void* buf, int64_t B, int64_t P, uint32_t mode, ListRecord* found) {
  std::lock_guard<std::mutex> lk(g_lists_mu);
  for (const ListRecord& r : g_lists)
    if (r.buf == buf) { *found = r; return (r.B == B && r.P == P && r.mode == mode) ? 0 : 2; }
  return 1;
}

struct StepFuse {
  void* comm = nullptr;   // reni_train_step_rows_dp: the decoder gradient is summed over this RCCL communicator's ranks inside the call
  int overlap = 0;        // ... layers >= 2 + head on the library's side stream as soon as they are final, the rest behind the call's work
  float* params; float* table;                  // (writable views of run_backward's params / Z)
  float *m_dec, *v_dec, *m_lat, *v_lat;
  float lr, b1, b2, eps, bc1, bc2_sqrt, gscale;
  const int64_t* idx_next;                      // batch to stage for the next call (NULL: none)
  uint32_t* state;                              // in / out: bit 0 = this call's prologue is staged, bit 1 = in which copy
};

// One backward call: what run_backward, run_backward_chunked and film_model_backward take.  Every member's initialiser is its
// "absent" value, so an entry point names only what it has.
constexpr int LOSS_DOUT = 2;  // internal loss_kind beside RENI_LOSS_MSE / RENI_LOSS_TEST: no loss, the caller passed d loss / d out (`dout`)
struct BwdCall {
  int64_t B = 0, P = 0;
  const float *Z = nullptr, *D = nullptr, *params = nullptr;  // (Z: the latent TABLE when idx is set)
  int64_t dbs = 0;
  const float *target = nullptr, *weight = nullptr, *dout = nullptr;
  const int64_t *ts = nullptr, *wst = nullptr;
  int loss_kind = RENI_LOSS_MSE;
  float alpha = 0.f, beta = 0.f;
  uint32_t flags = 0;
  float *out = nullptr, *loss_terms = nullptr, *dZ = nullptr, *dparams = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stream = nullptr;
  const FilmIO* fio = nullptr;   // FiLM conditioning
  const int64_t* idx = nullptr;  // the batch's rows of the table Z [n_rows][nd][3]
  int64_t n_rows = 0;
  const StepFuse* fuse = nullptr;
  const WeightLists* lists = nullptr;
};

// The decisions of one backward call, each taken in ONE place: bwd_path fills the record right after the layout and MainArgs exist, the
// stages of run_backward only read it.  (Layout::pdw -- "the persistent training instance runs" -- is the layout's, see there.)
struct BwdPath {
  bool staged;      // this call's prologue was run by the previous call: no run_prologue, and k_tail_b checks the batch it was staged for
  int stage;        // ... into this copy of the per-batch prologue results; the next batch goes into the other one
  bool use_cos;     // RENITestLoss with beta != 0: the statistics pass runs (unless cos_const) and the main pass takes loss_kind 1
  bool sparse;      // the statistics and main passes visit the listed tiles only (bwd_weight_lists binds or builds the lists)
  bool compact;     // ... and the main pass reads each image's live pixels packed into its first tiles
  bool cos_const;   // no statistics pass, no k_stats_image: the coefficients are the zeros the cached lists' build left
  bool dw1_ring;    // which dW_1 kernel runs, and how many partial slots its reduction sums (dw1_slots)
  bool l0x;         // the L0X training instance + k_reni_l0_ring: no fork, the per-image epilogue behind the ring on the one stream
  bool part_quad;   // the training kernel's weight-gradient partials (dwp: layers >= 2) are in the quad-row layout: their reduction takes the
                    // matching reducer (reduce_partials' quad_H, TailFusedArgs::rp_quad) -- decided here, nowhere else.  (dw1p stays flat.)
  bool fork;        // the per-image epilogue goes to the side stream, if one can be had (bwd_fork_dw1)
  bool early_rest;  // layers >= 2 and the head are reduced apart from layer 1: alone in front of dW_1, or in k_tail_a's launch (rp_in_tail)
  bool dp_early;    // the data-parallel step wants that early slice all-reduced on the communication stream, beside dW_1
  bool fused_tail;  // concat decoder behind the training instance: the per-image epilogue is k_tail_a + k_tail_b
  bool fuse_on;     // layer 1's partial reduction is not launched: it rides in k_adam2's launch (its layer-1 blocks)
  bool fpers;       // FiLM on the H = 128 persistent instances: one partial slot per image run
  bool red2;        // ... with weight gradients: the runs' d(freq) / d(phase) and layer 1's tagged partials in ONE launch (k_film_reduce2)
  int n_rest;       // decoder parameters behind the first layer: what the per-workgroup partials hold
  int n_l1;         // ... of which layer 1's (W_1 + b_1): the dW_1 kernel's own partials on the persistent path
  // Resolved where the resource is acquired -- side_stream() can return NULL, an event or a collective is only then on record -- by
  // bwd_fork_dw1; false until then:
  bool rp_in_tail;     // the partial reduction of layers >= 2 is part of k_tail_a's launch
  bool ev_rest_done;   // the caller's grad-ready event was recorded at the early point (else: at the call's end)
  bool dp_early_done;  // reni_train_step_rows_dp: the early slice's all-reduce is on the side stream (the final exchange leaves it out)
};

// What the stages of run_backward share.
struct Bwd {
  const reni_plan* p;
  const BwdCall& c;
  GeoRt g; Layout l; reni::MainArgs a;
  char* ws;                // the workspace base
  hipStream_t s, se;       // the caller's stream; the side stream once forked (else = s)
  const float* Z;          // the call's latents: the batch's rows, gathered by k_prep_image, when the call came with a table and indices
  int stage_in;            // the copy the previous call staged this call's prologue into, -1: it staged none
  bool staged_shared;      // ... with the hidden layers' images in the shared form (run_prologue's shared_img)
  float *img_loss, *stats, *dA, *part2;
  ListDst ld;
  reni::LayerScale lsc;
  BwdPath path;
};

bool call_uses_cos(const BwdCall& c) { return c.loss_kind == RENI_LOSS_TEST && c.beta != 0.f; }  // RENITestLoss's cosine term is live

BwdPath bwd_path(const reni_plan* p, const Layout& l, const BwdCall& c, const reni::MainArgs& a, int stage_in) {
  BwdPath t{};
  const int H = p->d.hidden_features, L = p->d.hidden_layers;
  const bool need_dw = (c.flags & RENI_NEED_DW) != 0;
  t.staged = stage_in >= 0;
  t.stage = t.staged ? stage_in : 0;
  t.n_rest = (int)(p->n_params - p->n_first);
  t.n_l1 = H * H + H;
  t.use_cos = call_uses_cos(c);
  // RENI_WEIGHT_SPARSE with a frozen concat decoder: the tiles that can change the result, listed on the device from the
  // weight (k_tile_flags, k_tile_compact: two small launches); the statistics pass visits the images whose cosine term is not a
  // constant, the main pass the tiles with a non-zero weight and those images.  Same results (skipped records would be exact zeros).
  // (not when the output image is wanted: the tiles left out would leave holes in it)
  t.sparse = (c.flags & (RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT)) && !c.fio && !need_dw && c.loss_kind != LOSS_DOUT &&
             c.weight != nullptr && c.out == nullptr;  // (every concat kernel with a frozen decoder: persistent and generic, fp32 and bf16)
  t.compact = t.sparse && (c.flags & RENI_WEIGHT_COMPACT);  // + the pixels with weight packed into each image's first tiles
  // RENI_WEIGHT_COS_CONSTANT (cached lists whose build reported NO image with a live cosine term -- every mask of data/Masks: pixel 0
  // is masked): the statistics instance would visit nothing and k_stats_image would write B rows of zero coefficients; both launches
  // are left out and the coefficients are the zeros the build left in the lists buffer.  Same bits.
  t.cos_const = t.sparse && c.lists && (c.lists->flags & RENI_WEIGHT_COS_CONSTANT);
  t.dw1_ring = dw1_ring_plan_ok(p, c.P) && dw1_ring_call_ok(a);
  t.l0x = l0x_plan_ok(p, l, c.P, c.flags) && l0x_call_ok(a);  // (decided once: the training kernel, the ring and the tail's order follow it)
  t.part_quad = t.l0x;  // (the L0X instance is the only writer of that layout; RENI_NO_L0X, RENI_NO_PERSIST and FiLM never get here)
  // persistent path: fork.  `s` continues with k_reni_dw1 -> weight-gradient reduction -> first-layer weight tail;
  // `se` (side stream) takes everything that only needs the per-tile partials; joined before returning.
  // (small problems -- fewer than eight tiles per workgroup: the multi-resolution curriculum's first stages -- stay on ONE stream:
  // k_reni_dw1 is then a few microseconds, and the fork's and the join's cross-stream edges (~12 us each) cost more than it hides)
  // (L0X: the per-image epilogue needs k_reni_l0_ring's dA runs, so it runs BEHIND it on the one stream -- that kernel leaves no
  // registers for a neighbour anyway -- and the partial reduction of layers >= 2 rides in k_tail_a's launch)
  t.fork = side_stream_plan_ok(p, l) && !t.l0x && (c.fio || l.n_tiles >= 8 * l.nwg);
  t.early_rest = l.pdw && !c.fio && need_dw && L >= 1 && t.n_rest > t.n_l1;
  t.dp_early = c.fuse && c.fuse->comm && c.fuse->overlap;  // (its early slice is what the early reduction produces)
  t.fused_tail = l.pdw && !c.fio;
  // reni_train_step_rows on that path: layer 1's partial reduction is not launched -- it rides in the Adam launch behind the call's
  // work (k_adam2's layer-1 blocks)
  // (not with a data-parallel exchange inside the call: the collective needs layer 1's sum in the gradient buffer first)
  t.fuse_on = c.fuse && !c.fuse->comm && t.fused_tail && need_dw && (c.flags & RENI_NEED_DZ) && L >= 1;
  // (fpers: the H = 128 persistent FiLM instances' bookkeeping -- one partial slot per image run; k_reni_wide256<2, FILM> feeds the
  //  stream path's consumers, whose bookkeeping is the generic chain's)
  t.fpers = l.persist && !l.wide_train;
  // persistent path with weight gradients: the runs' d(freq) / d(phase) sums and layer 1's tagged partials in one launch
  t.red2 = L > 0 && t.fpers && need_dw;
  return t;
}

// the argument checks, and the kernels' geometry
int bwd_validate(Bwd& x) {
  const reni_plan* p = x.p; const BwdCall& c = x.c;
  if (const int rc = c.fio ? check_film(p, c.fio, true) : RENI_OK) return rc;
  if (!c.fio && p && p->d.conditioning != RENI_COND_CONCAT) return fail(RENI_EINVAL, "FiLM plan: use the reni_film_* entry points");
  if (const int rc = check_common(p, c.B, c.P, c.fio ? c.fio->A : c.Z, c.D, c.params, c.ws)) return rc;
  if ((c.flags & RENI_NEED_DW) && !c.dparams) return fail(RENI_EINVAL, "RENI_NEED_DW set but dparams is NULL");
  if (!c.fio && (c.flags & RENI_NEED_DZ) && !c.dZ) return fail(RENI_EINVAL, "RENI_NEED_DZ set but dZ is NULL");
  if (c.loss_kind == LOSS_DOUT) {
    if (!c.dout) return fail(RENI_EINVAL, "dout is NULL");
  } else {
    if (c.loss_kind != RENI_LOSS_MSE && c.loss_kind != RENI_LOSS_TEST) return fail(RENI_EINVAL, "unknown loss_kind %d", c.loss_kind);
    if (!c.target || !c.weight || !c.ts || !c.wst) return fail(RENI_EINVAL, "target/weight (and their strides) must be non-NULL");
    if (!c.loss_terms) return fail(RENI_EINVAL, "loss_terms is NULL");
  }
  if (!geo_for(p, &x.g)) return fail(RENI_EUNSUPPORTED, "hidden_features=%d unsupported", p->d.hidden_features);
  return RENI_OK;
}

// the layout (in the stage copy a staged step's prologue went to), the workspace check, the per-image buffers
int bwd_layout(Bwd& x) {
  const BwdCall& c = x.c;
  const bool staged = c.fuse && (*c.fuse->state & 1u);          // this call's prologue was run by the previous call
  x.stage_in = staged ? (int)((*c.fuse->state >> 1) & 1u) : -1;
  x.staged_shared = staged && ((*c.fuse->state >> 2) & 1u);
  x.l = make_layout(x.p, x.g, c.B, c.P, c.flags, true, true, staged ? x.stage_in : 0);
  const Layout& l = x.l;
  if (c.ws_bytes < l.total) return fail(RENI_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", l.total, c.ws_bytes);
  if (c.fuse) *c.fuse->state = 0;  // (whatever happens below: nothing is staged until this call has staged it)
  x.ws = (char*)c.ws;
  x.s = x.se = (hipStream_t)c.stream;
  x.Z = c.idx ? (const float*)(x.ws + l.o_Zc) : c.Z;  // behind the prologue: the batch's rows, gathered by k_prep_image
  x.img_loss = (float*)(x.ws + l.o_img_loss); x.stats = (float*)(x.ws + l.o_stats);
  x.dA = c.fio ? c.fio->dA : (float*)(x.ws + l.o_dA); x.part2 = (float*)(x.ws + l.o_part2);
  return RENI_OK;
}

// the constants the weight-gradient partials carry when the W^T images are 8 x the forward images (Layout::consistent_bwd; derivation:
// DESIGN.md section 4.2f): hidden layer l: (omega_hidden / omega_first) (8 / 2 pi)^l, head: 1 / gy_scale.  Ones otherwise.
void bwd_layer_scales(Bwd& x) {
  const reni_plan* p = x.p; reni::LayerScale& lsc = x.lsc;
  lsc.n_hid = p->d.hidden_features * p->d.hidden_features + p->d.hidden_features; lsc.L = p->d.hidden_layers;
  for (int i = 0; i <= reni::MAX_LAYERS; ++i) lsc.c[i] = 1.f;
  if (x.l.consistent_bwd && (x.c.flags & RENI_NEED_DW)) {
    double gy = (double)p->d.first_omega_0 / 8.0, cl = (double)p->d.hidden_omega_0 / (double)p->d.first_omega_0;
    for (int i = 0; i < p->d.hidden_layers; ++i) {
      gy *= 6.283185307179586 / 8.0;
      cl *= 8.0 / 6.283185307179586;
      lsc.c[i] = (float)cl;
    }
    lsc.c[p->d.hidden_layers] = (float)(1.0 / gy);
  }
}

// what the main pass takes (host work only: the pointers are the layout's), then the call's decisions from it
void bwd_main_args(Bwd& x) {
  const BwdCall& c = x.c; reni::MainArgs& a = x.a;
  fill_main_args(a, x.p, x.l, c.B, c.P, x.Z, c.D, c.dbs, x.ws);
  if (c.fio) { a.Apre = c.fio->A; a.film = c.fio->film; a.params = c.params; a.Z = nullptr; }
  a.need_dw = (c.flags & RENI_NEED_DW) ? 1 : 0;
#ifdef RENI_DEBUG  // diagnostic builds only (build.sh -DRENI_DEBUG): the ablation mask skips work, i.e. yields WRONG results
  if (const char* e = getenv("RENI_DEBUG_MASK")) a.dbg = c.fio ? 0 : atoi(e);
#endif
#if defined(RENI_TRACE) || defined(RENI_TRACE_DW1)  // cycle-trace builds only (profiles/tools/gpu_trace.py, gpu_trace_dw1.py)
  if (const char* e = getenv("RENI_TRACE_PTR")) a.trace = (long long*)strtoull(e, nullptr, 0);
#endif
  a.out = c.out; a.dout = c.dout; a.beta = c.beta;
  if (c.loss_kind != LOSS_DOUT) {
    a.target = c.target; a.ts0 = c.ts[0]; a.ts1 = c.ts[1]; a.ts2 = c.ts[2];
    a.weight = c.weight; a.ws0 = c.wst[0]; a.ws1 = c.wst[1]; a.ws2 = c.wst[2];
  }
  a.loss_kind = (c.loss_kind == LOSS_DOUT) ? LOSS_DOUT : (call_uses_cos(c) ? 1 : 0);  // (the statistics pass takes a copy with its own)
  x.path = bwd_path(x.p, x.l, c, a, x.stage_in);
  if (x.path.l0x) {
    // Shared images: the dX operand of the steps of layers L..2 is Wf_l^T, not 8 Wf_l^T.  The L - 1 factors of 8 ride on d loss / d y
    // instead, so that g_1 -- the stream k_reni_l0_ring reads -- and everything behind it are what they were, bit for bit; g_l (l >= 2)
    // and with it the partials of dW_l / db_l are 8^(l-1) times what they were, the head's 8^(L-1) times, and their constants
    // (reni::LayerScale) give the powers of two back: every product exact (DESIGN.md section 4.2f).
    const int L = x.p->d.hidden_layers;
    float up = 1.f;
    for (int i = 1; i < L; ++i) { up *= 8.f; x.lsc.c[i] /= up; }
    a.gy_scale *= up;
    x.lsc.c[L] /= up;
  }
}

// BwdPath::sparse: bind the caller's cached lists or build them in the workspace; BwdPath::cos_const: the cached zero coefficients
int bwd_weight_lists(Bwd& x) {
  const BwdCall& c = x.c; const BwdPath& path = x.path; reni::MainArgs& a = x.a;
  if (!path.sparse) return RENI_OK;
  if (c.lists) {
    // the caller's lists (reni_weight_lists_build for this B, P and these flags): no launch, no read of the weight
    x.ld = list_dst(const_cast<char*>(c.lists->buf), make_list_layout(c.B, c.P));
  } else {
    x.ld = list_dst(x.ws, x.l);
    if (const int rc = build_weight_lists(c.weight, c.wst, c.P, x.l.tpi, x.l.n_tiles, path.compact, x.ld, x.s)) return rc;
  }
  a.tlist = x.ld.tlist; a.tcount = x.ld.tcount;
  if (path.compact) { a.plist = x.ld.plist; a.nlive = x.ld.nlive; }
  if (path.cos_const) a.stats = x.stats = (float*)(const_cast<char*>(c.lists->buf) + make_list_layout(c.B, c.P).o_zstats);
  return RENI_OK;
}

// RENITestLoss's cosine term: the statistics of every image, then their coefficients
int bwd_stats_pass(Bwd& x) {
  const BwdCall& c = x.c; const Layout& l = x.l;
  if (!x.path.use_cos || x.path.cos_const) return RENI_OK;
  reni::MainArgs st = x.a;
  st.out = nullptr; st.loss_kind = 0;
  if (x.path.sparse) { st.tlist = x.a.tlist + l.n_tiles; st.tcount = x.a.tcount + 1; }
  // persistent path: the forward-only statistics instance of the same kernel, on the same pre-scaled weight images
  if (const int rc = l.persist ? launch_train(x.p, st, l.nwg, x.s, true) : launch_main(x.p, reni::MODE_STATS, st, l.nwg, x.s)) return rc;
  // the statistics of every image and their cosine coefficients: one launch (k_stats_image; it was three)
  RENI_LAUNCH(reni::k_stats_image, dim3((unsigned)c.B), dim3(256), 0, x.s, (const float*)x.a.loss_part, l.tpi, c.weight, (long long)c.wst[0],
                     (long long)c.wst[2], c.beta, x.img_loss, x.stats, (const int*)x.ld.imgcos);
  return RENI_OK;
}

// Whatever path leaves run_backward after the fork -- the joins at its end or an early error return -- the caller's stream waits for
// the side stream: a forked stream left un-joined would let the caller's next launch overtake work that reads its buffers.
struct SideJoin {
  SideStream* side = nullptr;
  hipStream_t s = nullptr;
  ~SideJoin() { if (side && hipEventRecord(side->ev[2], side->s) == hipSuccess) (void)hipStreamWaitEvent(s, side->ev[2], 0); }
};

// Behind the persistent training instance: the fork (BwdPath::fork), the early reduction of layers >= 2 with what hangs on it, the dW_1
// kernel.  Resolves rp_in_tail, ev_rest_done and dp_early_done.
int bwd_fork_dw1(Bwd& x, std::unique_lock<std::mutex>& side_lock, SideJoin& side_join) {
  const reni_plan* p = x.p; const BwdCall& c = x.c; const Layout& l = x.l; BwdPath& path = x.path; hipStream_t s = x.s;
  if (!l.pdw) return RENI_OK;
  SideStream* side = path.fork ? side_stream() : nullptr;
  if (side) {
    side_lock.lock();  // (the events are per device: one fork/join is enqueued at a time)
    HIP_TRY(hipEventRecord(side->ev[0], s));
    HIP_TRY(hipStreamWaitEvent(side->s, side->ev[0], 0));
    x.se = side->s;
    side_join.side = side; side_join.s = s;
  }
  // The partials of layers >= 2 (85 MB at the BASELINE shape; final when the training kernel ends) are reduced HERE, alone on
  // the device for 18 us: beside k_reni_dw1 the reduction took 116 us and slowed it by 25, and behind the latent tails of the
  // side stream it was the end of the longer chain (profiles/r03_step_timeline_c2.txt).
  // (one stream: the reduction's blocks ride in k_tail_a's launch -- bwd_epilogue_concat)
  path.rp_in_tail = path.early_rest && !side && !g_ev_rest && !path.dp_early;
  if (path.early_rest && !path.rp_in_tail) {
    // (alone in front of k_reni_dw1, not beside it on a stream of its own: measured again in round 4 with the fused epilogue --
    // beside, everything crawls and the step is 30 us longer: profiles/r04_tail.md)
    int rc = reduce_partials(x.a.dwp, l.dwp_per_wg, l.nwg, c.dparams + p->n_first, path.n_l1, path.n_rest, nullptr, x.lsc, s, path.part_quad ? p->d.hidden_features : 0);
    if (rc) return rc;
    // the gradient of layers >= 2 and of the head is final HERE, a whole k_reni_dw1 before the call ends: a data-parallel caller
    // starts their all-reduce on another stream behind this event (TrainEngine(overlap_comm=True))
    if (g_ev_rest) { HIP_TRY(hipEventRecord(g_ev_rest, s)); path.ev_rest_done = true; }
    if (path.dp_early) {
      // reni_train_step_rows_dp(overlap): the slice [n_first + n_l1, n_params) -- layers >= 2 and the head, 28 % of the gradient at
      // config 2 -- is final HERE: its all-reduce starts on the library's communication stream, beside the ring kernel and the
      // per-image epilogue; the optimiser launch waits for it below.  (Same order of collectives on every rank: early slice, then rest.)
      SideStream* cs = side_stream();
      if (!cs) return fail(RENI_EHIP, "no communication stream");
      if (!side_lock.owns_lock()) side_lock.lock();
      HIP_TRY(hipEventRecord(cs->ev[1], s));
      HIP_TRY(hipStreamWaitEvent(cs->s, cs->ev[1], 0));
      rc = rccl_allreduce_inplace(c.fuse->comm, c.dparams + p->n_first + path.n_l1, (size_t)(path.n_rest - path.n_l1), cs->s);
      if (rc) return rc;
      if (!side_join.side) { side_join.side = cs; side_join.s = s; }  // (joined like the forked epilogue: whatever path leaves)
      path.dp_early_done = true;
    }
  }
  return launch_dw1(x.a, l.nwg, path.dw1_ring, s, path.l0x);
}

// the weight-gradient consumers of the fragment / operand streams (the paths that do not keep the sums in registers)
int bwd_dw_consumers(Bwd& x) {
  const Layout& l = x.l; const reni::MainArgs& a = x.a; hipStream_t s = x.s;
  const int H = x.p->d.hidden_features;
  if (l.frag == 2) {  // fp32, H = 256: hidden-layer weight gradients from the fp32 fragment stream
    const int lds = 4 * ((reni::Geo<reni::PolF32, 256>::T_BYTES + 1023) & ~1023);
    if (const int rc = timed_launch(reni::k_dw_frag32<256>, l.nwg, 256, lds, s, a, PROF_DWS)) return rc;
  }
  if (l.wide_train && (x.c.flags & RENI_NEED_DW)) {  // the head's weight gradient from k_reni_wide256<2>'s g_y stream and phase stash (a frozen FiLM decoder: no partials to write)
    if (const int rc = timed_launch(s, PROF_DWS, "k_wide_head_dw", [&] { return reni::launch_wide_head_dw(a, l.nwg, s); })) return rc;
  }
  if (l.stream) {  // hidden-layer weight gradients (and FiLM d(freq), d(phase)) from the operand stream
    static_assert(reni::Geo<reni::PolBF16, 256>::T_BYTES_AL == 36864 && reni::Geo<reni::PolBF16, 128>::T_BYTES_AL == 34816,
                  "stream record sizes (make_layout)");
    const bool film = x.c.fio != nullptr;
    void (*fn)(const reni::MainArgs) = nullptr;
    if (H == 256) fn = film ? reni::k_dw_frag<256, true> : reni::k_dw_frag<256, false>;
    else fn = film ? reni::k_dw_stream<128, true> : reni::k_dw_stream<128, false>;
    if (film) HIP_TRY(hipMemsetAsync(a.run_image, 0xff, (size_t)l.nwg * l.kmax * 4, s));
    return timed_launch(fn, l.nwg, 256, 4 * (H == 256 ? 36864 : 34816), s, a, PROF_DWS);
  }
  return RENI_OK;
}

// the per-image sums -- dA_b and the loss -- of every path but the fused tail's (whose k_tail_a forms them): on `se`
int bwd_image_sums(Bwd& x) {
  const BwdCall& c = x.c; const Layout& l = x.l; const reni::MainArgs& a = x.a;
  const int H = x.p->d.hidden_features;
  if (x.path.fused_tail) return RENI_OK;
  if (l.pdw) {  // the training instance keeps the per-image sums on chip: a few image runs per image
    RENI_LAUNCH(reni::k_reduce_runs, dim3((unsigned)c.B, c.B < 16 ? (unsigned)((H * 8 + 16 + 63) / 64) : 1u), dim3(256), 0, x.se, (const float*)a.pruns, (const int*)a.prun_image,
                       l.nwg, l.pkmax, H, l.tpi, l.n_tiles, x.dA, x.img_loss);
    return RENI_OK;
  }
  RENI_LAUNCH(reni::k_reduce_tiles_a, dim3((unsigned)c.B, (unsigned)l.nch), dim3(256), 0, x.se, (const float*)a.dA_part,
                     (const float*)a.loss_part, l.tpi, H, x.part2, 1, l.rt_chunk, (const int*)x.ld.tflag);
  RENI_LAUNCH(reni::k_reduce_tiles_b, dim3((unsigned)c.B, (unsigned)((H * 8 + 16 + 255) / 256)), dim3(256), 0, x.se, (const float*)x.part2, l.nch, H, x.dA, x.img_loss, 1);
  return RENI_OK;
}

// FiLM: d(freq) / d(phase), the decoder's weight gradient, the loss terms
// (persistent path: `s` carries k_reni_dw1 and what needs its runs -- d(freq) / d(phase), layer 1's weight gradient;
// `se` what needs the training kernel only -- dA, the loss, the other layers' weight gradients)
int bwd_epilogue_film(Bwd& x) {
  const reni_plan* p = x.p; const BwdCall& c = x.c; const Layout& l = x.l; const BwdPath& path = x.path; const reni::MainArgs& a = x.a;
  hipStream_t s = x.s, se = x.se;
  const int H = p->d.hidden_features, L = p->d.hidden_layers;
  if (path.red2) {  // (in k_film_reduce2's launch, below)
  } else if (L > 0 && (l.stream || path.fpers)) {
    RENI_LAUNCH(reni::k_reduce_film_runs, dim3((unsigned)c.B, (unsigned)((L * H + 255) / 256)), dim3(256), 0, s, a, H,
                       path.fpers ? 3 * l.nwg * l.pkmax : l.nwg * l.kmax, c.fio->dfilm);
  } else if (L > 0) {
    RENI_LAUNCH(reni::k_reduce_film, dim3((unsigned)c.B, (unsigned)((L * 2 * H + 255) / 256)), dim3(256), 0, s,
                       (const float*)a.dfp_part, l.tpi, L * 2 * H, c.fio->dfilm);
  }
  if (c.flags & RENI_NEED_DW) {
    // the first layer's gradient belongs to the glue (it is a function of dA): zero its slot unless the caller
    // (reni_film_model_*) fills it
    if (!c.fio->keep_first) HIP_TRY(hipMemsetAsync(c.dparams, 0, (size_t)p->n_first * 4, s));
    if (path.fpers) {  // one partial slot per image run: layer 1 from k_reni_dw1's runs, the rest from the training kernel's
      const int n_l1 = path.n_l1, nslot = l.nwg * l.pkmax;
      reni::FilmReduce2 r2;
      r2.H = H; r2.nruns = 3 * l.nwg * l.pkmax; r2.B = (int)c.B; r2.gy = (L * H + 255) / 256; r2.dfilm = c.fio->dfilm;
      r2.part = a.dw1p; r2.per_wg = (size_t)n_l1; r2.nslot = 2 * nslot; r2.dparams = c.dparams + p->n_first; r2.n = n_l1;
      r2.valid = (const int*)a.prun_image + nslot;
      RENI_LAUNCH(reni::k_film_reduce2, dim3((unsigned)(r2.B * r2.gy + (n_l1 + 63) / 64)), dim3(256), 0, s, a, r2);
      if (const int rc = reduce_partials(a.dwp, l.dwp_per_wg, nslot, c.dparams + p->n_first, n_l1, path.n_rest, a.prun_image, x.lsc, se)) return rc;
    } else if (const int rc = reduce_partials(a.dwp, l.dwp_per_wg, l.nwg, c.dparams + p->n_first, 0, path.n_rest, nullptr, x.lsc, s)) {
      return rc;
    }
  }
  if (c.loss_kind != LOSS_DOUT) {
    RENI_LAUNCH(reni::k_finalize_loss, dim3(1), dim3(256), 0, se, (const float*)x.img_loss, (const float*)x.stats,
                       c.fio->Zp, (int)c.B, (int)c.P, (int)c.fio->nz, path.use_cos ? 1 : 0,
                       (c.fio->Zp != nullptr && c.loss_kind == RENI_LOSS_TEST) ? 1 : 0, c.fio->alpha, c.beta, c.loss_terms);
  }
  return RENI_OK;
}

// concat decoder: layer 1's reduction, the latent tails, the loss terms, the first layer's weight gradient, the generic paths' reduction
int bwd_epilogue_concat(Bwd& x) {
  const reni_plan* p = x.p; const BwdCall& c = x.c; const Layout& l = x.l; const BwdPath& path = x.path; const reni::MainArgs& a = x.a;
  hipStream_t s = x.s, se = x.se;
  const int H = p->d.hidden_features;
  const bool need_dw = (c.flags & RENI_NEED_DW) != 0;
  reni::TailArgs t;
  t.dA = x.dA; t.W0 = c.params; t.Z = x.Z; t.xconst = (const float*)(x.ws + l.o_xconst);
  t.mcol = (float*)(x.ws + l.o_mcol); t.ucol = (float*)(x.ws + l.o_ucol);
  t.dZ = c.dZ; t.dW0 = c.dparams; t.db0 = c.dparams ? c.dparams + (size_t)H * p->F_in : nullptr;
  t.alpha2 = (c.loss_kind == RENI_LOSS_TEST) ? c.alpha : 0.f;
  t.eq = p->d.equivariance; t.nd = p->d.ndims; t.F_in = p->F_in; t.H = H; t.B = (int)c.B;
  // persistent path: layer 1's H * H + H values come from k_reni_dw1's own partials (the rest was reduced in front of it)
  if (!path.fuse_on && need_dw && l.pdw && p->d.hidden_layers >= 1) {
    if (const int rc = reduce_partials(a.dw1p, (size_t)path.n_l1, dw1_slots(path.dw1_ring, l.nwg), c.dparams + p->n_first, 0, path.n_l1, nullptr, x.lsc, s)) return rc;
  }
  // what k_tail_b takes on either path: the per-image sums, the loss configuration, which outputs are wanted ...
  reni::TailFusedArgs f;
  memset(&f, 0, sizeof(f));
  f.t = t;
  f.img_loss = x.img_loss; f.stats = x.stats; f.P = (int)c.P; f.nz = (int)(c.B * p->d.ndims * 3); f.has_cos = path.use_cos ? 1 : 0;
  f.has_prior = (c.loss_kind == RENI_LOSS_TEST) ? 1 : 0; f.alpha = c.alpha; f.beta = c.beta;
  f.loss_terms = (c.loss_kind != LOSS_DOUT) ? c.loss_terms : nullptr;
  f.need_dz = (c.flags & RENI_NEED_DZ) ? 1 : 0;
  f.need_dw0 = need_dw ? 1 : 0;
  f.dw0_gx = (p->F_in + 1 + 255) / 256;
  // ... and, for a staged step: the batch the previous call prepared must be the batch this call was given (else: NaN, loudly)
  // (the staged-batch check of reni_train_step_rows on the generic kernels too: fp32, H = 32 / 64 / 256, RENI_NO_PERSIST -- ADVICE r04)
  f.idx_now = path.staged ? (const long long*)c.idx : nullptr;
  f.idx_staged = path.staged ? (const long long*)(x.ws + l.o_idxc) : nullptr;
  f.skip_flag = c.fuse ? (int*)(x.ws + l.o_skip) : nullptr;
  const unsigned nb = (unsigned)((f.need_dz ? c.B : 0) + 1 + (f.need_dw0 ? f.dw0_gx * H : 0));
  if (path.fused_tail) {
    // image runs -> dA_b, loss sums, m / u columns (k_tail_a); then dZ_b, loss terms, dW0 / db0 (k_tail_b): two launches, it was five
    f.pruns = a.pruns; f.prun_image = a.prun_image; f.nwg = l.nwg; f.kmax = l.pkmax; f.tpi = l.tpi; f.n_tiles = l.n_tiles;
    f.dA_out = x.dA;
    const unsigned ny = f.need_dz ? (unsigned)((p->F_in + 63) / 64) : 1u;
    unsigned gx = (unsigned)c.B;
    if (path.rp_in_tail) {
      f.rp_part = a.dwp; f.rp_per_wg = l.dwp_per_wg; f.rp_nwg = l.nwg; f.rp_out = c.dparams + p->n_first; f.rp_lo = path.n_l1; f.rp_n = path.n_rest; f.rp_ls = x.lsc;
      f.rp_quad = path.part_quad ? 1 : 0;
      if (f.rp_quad && ((l.dwp_per_wg | (size_t)path.n_l1) & 3)) return fail(RENI_EINVAL, "internal: quad-row partials need 16-byte aligned slots");
      const int per_blk = f.rp_quad ? reni::QUAD_BLK_WORDS : 64;  // (buffer words per block: reduce_partials_quad_body / reduce_partials_body)
      gx += ((unsigned)((path.n_rest - path.n_l1 + per_blk - 1) / per_blk) + ny - 1) / ny;
    }
    RENI_LAUNCH(reni::k_tail_a, dim3(gx, ny), dim3(256), (size_t)reni::tail_a_lds_bytes(H), se, f);
  } else if (c.flags & RENI_NEED_DZ) {
    RENI_LAUNCH(reni::k_tail_m, dim3((unsigned)c.B, (unsigned)((p->F_in + 63) / 64)), dim3(256), 0, se, t);
  }
  // dZ_b (B blocks; from k_tail_a's or k_tail_m's columns), the loss terms (one block), dW0 / db0 (from the per-image dA): all functions
  // of those results alone -> one launch (k_tail_b; it was three)
  RENI_LAUNCH(reni::k_tail_b, dim3(nb), dim3(256), 0, se, f);
  if (need_dw && !path.fused_tail && path.n_rest > 0) {  // (persistent path: reduced in front of k_reni_dw1, or in k_tail_a's launch)
    if (const int rc = reduce_partials(a.dwp, l.dwp_per_wg, l.nwg, c.dparams + p->n_first, 0, path.n_rest, nullptr, x.lsc, s)) return rc;
  }
  if (g_ev_rest && !path.ev_rest_done) HIP_TRY(hipEventRecord(g_ev_rest, s));  // (paths without the early point: final at the end)
  return RENI_OK;
}

// reni_train_step_rows: behind the call's work -- the side stream (if any) is joined first -- ONE launch takes the whole optimiser
// step (decoder, latent table and, on the persistent path, layer 1's partial reduction with its Adam step), then the next
// batch's prologue goes into the other stage copy.
// (Round 4 also tried the optimiser and the next prologue SPLIT around k_reni_dw1 -- everything but layer 1 beside it on the side
// stream, layer 1 behind it: beside that kernel the 23 us of Adam + prologue crawl for 80 and slow it by 10, and the extra
// cross-stream edge costs what is left: +-0 at config 2, +11 us at 64 x 128.  profiles/r04_tail.md.)
int bwd_fused_step(Bwd& x, SideJoin& side_join) {
  const reni_plan* p = x.p; const BwdCall& c = x.c; const Layout& l = x.l; const BwdPath& path = x.path; hipStream_t s = x.s;
  const StepFuse& fu = *c.fuse;
  if (side_join.side) {
    HIP_TRY(hipEventRecord(side_join.side->ev[2], side_join.side->s));
    HIP_TRY(hipStreamWaitEvent(s, side_join.side->ev[2], 0));
    side_join.side = nullptr;
  }
  if (fu.comm) {
    // the data-parallel exchange (run.py:97-110: DDP's all-reduce of the shared decoder's gradients) INSIDE the step: an in-place
    // RCCL sum of the flat decoder gradient over the communicator's ranks on the caller's stream; the 1 / world of the mean rides on
    // Adam's grad_scale.  Latent rows need no exchange (every row has one owner: reni_amd/dist.py).
    const size_t n_early = path.dp_early_done ? (size_t)(path.n_rest - path.n_l1) : 0;
    // (a staged step that met another batch than the one staged for it is skipped -- k_tail_b's flag, k_adam2 -- and that decision
    //  must be the same on every rank, or the replicas part: the flags' MAX first (4 bytes; ADVICE r05))
    // (unconditionally -- not only when THIS rank's step is staged: a collective every rank must enter)
    EvPair ev;
    const bool timed = prof_begin(s, &ev, PROF_COMM);
    int rc = rccl_allreduce_max_i32(fu.comm, (int*)(x.ws + l.o_skip), 1, s);
    if (rc) return rc;
    rc = rccl_allreduce_inplace(fu.comm, c.dparams, (size_t)p->n_params - n_early, s);
    if (rc) return rc;
    if (timed) HIP_TRY(hipEventRecord(ev.b, s));
  }
  reni::Adam2Args ad;
  ad.p = fu.params; ad.g = c.dparams; ad.m = fu.m_dec; ad.v = fu.v_dec; ad.n = p->n_params;
  ad.nb_dec = (int)((p->n_params + 255) / 256);
  ad.tp = fu.table; ad.g_rows = c.dZ; ad.idx = (const long long*)c.idx; ad.B = (int)c.B; ad.row_len = p->d.ndims * 3;
  ad.tm = fu.m_lat; ad.tv = fu.v_lat; ad.tn = c.n_rows * ad.row_len;
  ad.lr = fu.lr; ad.b1 = fu.b1; ad.b2 = fu.b2; ad.eps = fu.eps; ad.gscale = fu.gscale;
  ad.bc1 = fu.bc1; ad.bc2_sqrt = fu.bc2_sqrt;
  ad.skip_lo = 0; ad.skip_hi = 0; ad.l1_part = nullptr; ad.l1_per_wg = 0; ad.l1_nwg = 0; ad.nb_l1 = 0; ad.l1_scale = x.lsc.c[0];
  ad.skip_step = (const int*)(x.ws + l.o_skip);  // (written by this call's k_tail_b, in front of this launch on every path)
  if (path.fuse_on) {
    ad.skip_lo = p->n_first; ad.skip_hi = p->n_first + path.n_l1;
    ad.l1_part = x.a.dw1p; ad.l1_per_wg = (size_t)path.n_l1; ad.l1_nwg = dw1_slots(path.dw1_ring, l.nwg); ad.nb_l1 = (path.n_l1 + 63) / 64;
  }
  RENI_LAUNCH(reni::k_adam2, dim3((unsigned)(ad.nb_dec + (ad.tn + 255) / 256 + ad.nb_l1)), dim3(256), 0, s, ad);
  if (fu.idx_next) {
    const Layout ln = make_layout(p, x.g, c.B, c.P, c.flags, true, true, 1 - path.stage);
    // (the images are packed for the kernels THIS call ran -- the next call of a training loop runs the same; bit 2 says which, and a
    //  call that decides otherwise runs its own prologue: run_backward)
    if (const int rc = run_prologue(p, x.g, ln, c.B, fu.table, fu.params, x.ws, true, s, fu.idx_next, nullptr, c.n_rows, path.l0x)) return rc;
    *fu.state = 1u | ((uint32_t)(1 - path.stage) << 1) | (path.l0x ? 4u : 0u);
  }
  return RENI_OK;
}

// Everything behind the entry points' own argument handling, for every backward call (fio != NULL: FiLM conditioning): a driver over
// the stages above, in launch order.  The side stream's lock and join guard live in THIS frame, so every return below them -- an
// error from any stage included -- joins the side stream and then lets go of the lock.
int run_backward(const reni_plan* p, const BwdCall& c) {
  Bwd x{p, c};
  int rc = bwd_validate(x);
  if (rc) return rc;
  DeviceGuard dev_guard;
  if ((rc = dev_guard.enter(c.params))) return rc;
  if ((rc = bwd_layout(x))) return rc;
  bwd_layer_scales(x);
  bwd_main_args(x);  // (+ BwdPath: from here on every decision is on record)
  // (a staged prologue whose images are not in the form this call's kernels read is not used: the call packs its own, into the same copy)
  if (x.path.staged && x.staged_shared != x.path.l0x) x.path.staged = false;
  if (!x.path.staged && (rc = run_prologue(p, x.g, x.l, c.B, c.Z, c.params, x.ws, true, x.s, c.idx, c.fio ? c.fio->A : nullptr, c.n_rows, x.path.l0x))) return rc;
  if ((rc = bwd_weight_lists(x))) return rc;
  if ((rc = bwd_stats_pass(x))) return rc;
  rc = x.l.persist ? launch_train(p, x.a, x.l.nwg, x.s, false, x.path.l0x) : launch_main(p, reni::MODE_FWD_BWD, x.a, x.l.nwg, x.s);
  if (rc) return rc;
  std::unique_lock<std::mutex> side_lock(g_side_mu, std::defer_lock);
  SideJoin side_join;
  if ((rc = bwd_fork_dw1(x, side_lock, side_join))) return rc;
  if ((rc = bwd_dw_consumers(x))) return rc;
  if ((rc = bwd_image_sums(x))) return rc;
  if (c.fio) return bwd_epilogue_film(x);
  if ((rc = bwd_epilogue_concat(x))) return rc;
  return c.fuse ? bwd_fused_step(x, side_join) : RENI_OK;
}

// ---- H = 256 training in image chunks ---------------------------------------------------------------------------------
// The fragment-stream path (H = 256 with weight gradients: k_reni_main writes every tile's phase stash and g fragments, k_dw_frag /
// k_dw_frag32 consume them) keeps (2 L + 1) x 64 KB (bf16) per 128-sample tile: 11 GB at the BASELINE batch of 64 images, 23 GB in
// fp32 -- a workspace that grows with B x P and caps the batch.  A call whose stream would exceed reni_plan::frag_ws_cap (16 GB; RENI_FRAG_WS_CAP_MB) is run in
// CHUNKS OF WHOLE IMAGES through the same code path, one after the other on the caller's stream: every per-image result (out, dZ)
// lands in place, the loss terms and the decoder gradient -- sums over images (loss_functions.py:6-13) -- are accumulated.
int64_t frag_chunk_images(const reni_plan* p, int64_t B, int64_t P, uint32_t flags) {
  GeoRt g;
  if (!p || p->d.conditioning != RENI_COND_CONCAT || p->d.hidden_features != 256 || !(flags & RENI_NEED_DW) || !geo_for(p, &g)) return B;
  const Layout l = backward_layout(p, g, 1, P, flags);
  if (!l.frag) return B;
  const size_t per_image = (size_t)l.tpi * (size_t)(2 * p->d.hidden_layers + 1) * g.stash_layer_bytes;
  int64_t bc = (int64_t)(p->frag_ws_cap / (per_image ? per_image : 1));
  if (bc < 1) bc = 1;
  if (bc >= B) return B;
  // (equal chunks: 100 images under a cap of 88 run as 50 + 50, not 88 + 12 -- every chunk pays the same fixed costs: the weight-gradient
  // partials' flush and reduction, ~0.15 ms at 5 x 256)
  const int64_t n_chunks = (B + bc - 1) / bc;
  return (B + n_chunks - 1) / n_chunks;
}

int run_backward_chunked(const reni_plan* p, const BwdCall& c) {
  const int64_t B = c.B, P = c.P;
  const int64_t bc = (p && B >= 1 && P >= 1) ? frag_chunk_images(p, B, P, c.flags) : B;
  if (bc >= B) return run_backward(p, c);
  // workspace: [chunk's own layout | dparams of the chunk | loss terms of the chunk]
  GeoRt g;
  geo_for(p, &g);
  // the chunk loop's own launches (k_add_into) run on the device that owns the buffers, like everything run_backward launches
  DeviceGuard dev_guard;
  if (const int rcg = dev_guard.enter(c.params)) return rcg;
  const size_t core = al256(backward_layout(p, g, bc, P, c.flags).total);
  if (B % bc != 0 && backward_layout(p, g, B % bc, P, c.flags).total > core)
    return fail(RENI_EWORKSPACE, "internal: the last chunk's layout exceeds a full chunk's");
  const size_t extra = al256((size_t)p->n_params * 4) + 256;
  if (!c.ws) return fail(RENI_EWORKSPACE, "workspace is NULL");
  if (c.ws_bytes < core + extra) return fail(RENI_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", core + extra, c.ws_bytes);
  float* dp_c = (float*)((char*)c.ws + core);
  float* lt_c = (float*)((char*)c.ws + core + al256((size_t)p->n_params * 4));
  hipStream_t s = (hipStream_t)c.stream;
  const int nd3 = p->d.ndims * 3;
  for (int64_t b0 = 0; b0 < B; b0 += bc) {
    const bool first = b0 == 0;
    BwdCall k = c;  // the chunk: images [b0, b0 + k.B) of the call, every per-image buffer moved there
    k.B = (B - b0 < bc) ? B - b0 : bc;
    if (c.idx) k.idx = c.idx + b0;  // (Z stays the table)
    else if (c.Z) k.Z = c.Z + b0 * nd3;
    if (c.D) k.D = c.D + b0 * c.dbs;
    if (c.target) k.target = c.target + b0 * c.ts[0];
    if (c.weight) k.weight = c.weight + b0 * c.wst[0];
    if (c.dout) k.dout = c.dout + b0 * P * 3;
    if (c.out) k.out = c.out + b0 * P * 3;
    if (c.dZ) k.dZ = c.dZ + b0 * nd3;
    if (c.loss_terms && !first) k.loss_terms = lt_c;
    if (c.dparams && !first) k.dparams = dp_c;
    k.ws_bytes = core;
    const int rc = run_backward(p, k);
    if (rc) return rc;
    if (!first) {
      if (c.dparams) {
        RENI_LAUNCH(reni::k_add_into, dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, c.dparams, (const float*)dp_c, (size_t)p->n_params);
      }
      if (c.loss_terms) {
        RENI_LAUNCH(reni::k_add_into, dim3(1), dim3(256), 0, s, c.loss_terms, (const float*)lt_c, (size_t)4);
      }
    }
  }
  return RENI_OK;
}

// ---- FiLM, whole model: glue kernels around the per-sample core -------------------------------------------------
struct GlueLayout {
  size_t o_A, o_film, o_dA, o_dfilm, o_mapm, o_mapx, o_fo, o_dAb, o_dm, o_dly, total;
  unsigned dly_off[reni::MAX_MAP_LAYERS + 1];
};

GlueLayout make_glue_layout(const reni_plan* p, int64_t B) {
  GlueLayout g;
  memset(&g, 0, sizeof(g));
  const int H = p->d.hidden_features, L = p->d.hidden_layers, ML = p->d.mapping_layers, Hm = p->d.mapping_features;
  size_t o = 0;
  g.o_A = o; o += al256((size_t)B * H * 8 * 4);
  g.o_film = o; o += al256((size_t)B * (L > 0 ? L : 1) * 2 * H * 4);
  g.o_dA = o; o += al256((size_t)B * H * 8 * 4);
  g.o_dfilm = o; o += al256((size_t)B * (L > 0 ? L : 1) * 2 * H * 4);
  g.o_mapm = o; o += al256((size_t)B * p->M_in * 4);
  g.o_mapx = o; o += al256((size_t)B * ML * Hm * 4);
  g.o_fo = o; o += al256((size_t)B * p->N_out * 4);
  g.o_dAb = o; o += al256((size_t)B * H * 8 * 4);
  g.o_dm = o; o += al256((size_t)B * p->M_in * 4);
  g.o_dly = o;
  size_t d = 0;
  for (int i = 0; i <= ML; ++i) { g.dly_off[i] = (unsigned)d; d += (size_t)B * ((i < ML) ? Hm : p->N_out); }
  o += al256(d * 4);
  g.total = o;
  return g;
}

int check_film_model(const reni_plan* p, const void* Z, const void* map_params) {
  if (!p) return fail(RENI_EINVAL, "plan is NULL");
  if (p->d.conditioning != RENI_COND_FILM || p->d.mapping_layers < 1)
    return fail(RENI_EINVAL, "plan was not created with RENI_COND_FILM and a mapping network");
  if (!Z || !map_params) return fail(RENI_EINVAL, "Z and map_params must be non-NULL");
  return RENI_OK;
}

void fill_glue(reni::FilmGlueArgs& g, const reni_plan* p, const GlueLayout& gl, int64_t B, const float* Z,
               const float* params, const float* mparams, char* gw) {
  memset(&g, 0, sizeof(g));
  g.Z = Z; g.params = params; g.mparams = mparams;
  g.A = (float*)(gw + gl.o_A); g.film = (float*)(gw + gl.o_film);
  g.mapm = (float*)(gw + gl.o_mapm); g.mapx = (float*)(gw + gl.o_mapx); g.fo = (float*)(gw + gl.o_fo);
  g.dA = (const float*)(gw + gl.o_dA); g.dfilm = (const float*)(gw + gl.o_dfilm);
  g.dAb = (float*)(gw + gl.o_dAb); g.dly = (float*)(gw + gl.o_dly);
  g.eq = p->d.equivariance; g.nd = p->d.ndims; g.H = p->d.hidden_features; g.L = p->d.hidden_layers;
  g.F0 = p->F_in; g.M_in = p->M_in; g.Hm = p->d.mapping_features; g.ML = p->d.mapping_layers; g.N_out = p->N_out;
  g.B = (int)B;
  for (int i = 0; i <= g.ML; ++i) { g.mw_off[i] = p->mw_off[i]; g.mb_off[i] = p->mb_off[i]; g.dly_off[i] = gl.dly_off[i]; }
}

// forward glue: mapping input -> mapping network -> film / A
int run_film_glue_fwd(const reni::FilmGlueArgs& g, hipStream_t s) {
  const int B = g.B;
  RENI_LAUNCH(reni::k_film_minput, dim3((unsigned)B), dim3(256), 0, s, g);
  for (int i = 0; i <= g.ML; ++i) {
    const int N = (i < g.ML) ? g.Hm : g.N_out, K = (i == 0) ? g.M_in : g.Hm;
    const float* x = (i == 0) ? g.mapm : g.mapx + (size_t)(i - 1) * g.Hm;
    const int ldx = (i == 0) ? g.M_in : g.ML * g.Hm;
    float* y = (i < g.ML) ? g.mapx + (size_t)i * g.Hm : g.fo;
    const int ldy = (i < g.ML) ? g.ML * g.Hm : g.N_out;
    if ((long long)N * B >= 65536)
      RENI_LAUNCH(reni::k_film_linear<4>, dim3((unsigned)((N + 15) / 16), (unsigned)B), dim3(256), 0, s, x, ldx,
                         g.mparams + g.mw_off[i], g.mparams + g.mb_off[i], y, ldy, N, K, i < g.ML ? 1 : 0);
    else
      RENI_LAUNCH(reni::k_film_linear<1>, dim3((unsigned)((N + 3) / 4), (unsigned)B), dim3(256), 0, s, x, ldx,
                         g.mparams + g.mw_off[i], g.mparams + g.mb_off[i], y, ldy, N, K, i < g.ML ? 1 : 0);
  }
  RENI_LAUNCH(reni::k_film_fold, dim3((unsigned)B), dim3(256), 0, s, g);
  return RENI_OK;
}

// core workspace first, glue buffers behind it
size_t core_ws_bytes(const reni_plan* p, int64_t B, int64_t P, uint32_t flags) {
  GeoRt g;
  if (!geo_for(p, &g)) return 0;
  return al256(backward_layout(p, g, B, P, flags).total);  // (as reni_workspace_bytes sizes it)
}

// (c.Z: the latents; c.dparams / dmparams: the decoder's and the mapping network's gradients)
int film_model_backward(const reni_plan* p, const BwdCall& c, const float* mparams, float* dmparams) {
  const int64_t B = c.B;
  const uint32_t flags = c.flags;
  float* const dparams = c.dparams;
  int rc = check_film_model(p, c.Z, mparams);
  if (rc) return rc;
  if ((flags & RENI_NEED_DW) && (!dparams || !dmparams)) return fail(RENI_EINVAL, "RENI_NEED_DW set but dparams / dmap_params is NULL");
  if (!c.dZ) return fail(RENI_EINVAL, "dZ is NULL");
  if (!c.ws) return fail(RENI_EWORKSPACE, "workspace is NULL");
  const size_t core = core_ws_bytes(p, B, c.P, flags);
  const GlueLayout gl = make_glue_layout(p, B);
  if (core == 0 || c.ws_bytes < core + gl.total)
    return fail(RENI_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", core + gl.total, c.ws_bytes);
  DeviceGuard dev_guard;
  rc = dev_guard.enter(c.params);
  if (rc) return rc;
  char* gw = (char*)c.ws + core;
  hipStream_t s = (hipStream_t)c.stream;
  reni::FilmGlueArgs g;
  fill_glue(g, p, gl, B, c.Z, c.params, mparams, gw);
  g.dZ = c.dZ;
  g.alpha2 = (c.loss_kind == RENI_LOSS_TEST) ? 2.f * c.alpha : 0.f;
  rc = run_film_glue_fwd(g, s);
  if (rc) return rc;
  FilmIO fio;
  fio.A = g.A; fio.film = g.film; fio.dA = (float*)(gw + gl.o_dA); fio.dfilm = (float*)(gw + gl.o_dfilm);
  fio.Zp = c.Z; fio.alpha = c.alpha; fio.nz = B * p->d.ndims * 3; fio.keep_first = 1;
  BwdCall k = c;  // the per-sample core: the glue owns the latents, their prior and their gradient
  k.Z = nullptr; k.dZ = nullptr; k.alpha = 0.f; k.flags = flags & RENI_NEED_DW;
  k.ws_bytes = core; k.fio = &fio;
  rc = run_backward(p, k);
  if (rc) return rc;
  RENI_LAUNCH(reni::k_film_dout, dim3((unsigned)B), dim3(256), 0, s, g);
  float* dm = (float*)(gw + gl.o_dm);
  for (int i = g.ML; i >= 0; --i) {  // delta of layer i-1's output (i = 0: of the mapping input) from layer i's
    const int N = (i < g.ML) ? g.Hm : g.N_out, K = (i == 0) ? g.M_in : g.Hm;
    const float* xact = (i == 0) ? nullptr : g.mapx + (size_t)(i - 1) * g.Hm;
    float* dx = (i == 0) ? dm : g.dly + gl.dly_off[i - 1];
    RENI_LAUNCH(reni::k_film_linear_t, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(64 * reni::FLT_NG), 0, s,
                       (const float*)(g.dly + gl.dly_off[i]), N, g.mparams + g.mw_off[i], N, K, xact, g.ML * g.Hm, dx, K);
  }
  // dZ (needs dm), the first FiLM layer's and every mapping-network layer's weight gradients (need the deltas): one launch
  reni::FilmWgradAll wa;
  memset(&wa, 0, sizeof(wa));
  reni::FilmGrads fg;
  memset(&fg, 0, sizeof(fg));
  fg.dm = dm; fg.need_dw = (flags & RENI_NEED_DW) ? 1 : 0;
  unsigned nblk = (unsigned)B;
  if (flags & RENI_NEED_DW) {
    const int H = g.H, ML = g.ML, Hm = g.Hm;
    int nw = 0;
    for (int i = 0; i <= ML; ++i) {
      const int N = (i < ML) ? Hm : g.N_out, K = (i == 0) ? g.M_in : Hm;
      wa.delta[i] = g.dly + gl.dly_off[i]; wa.ldd[i] = N; wa.N[i] = N; wa.K[i] = K;
      wa.x[i] = (i == 0) ? g.mapm : g.mapx + (size_t)(i - 1) * Hm;
      wa.ldx[i] = (i == 0) ? g.M_in : ML * Hm;
      wa.out_w[i] = dmparams + p->mw_off[i]; wa.out_b[i] = dmparams + p->mb_off[i];
      fg.gxw[i] = (K + 1 + 255) / 256;
      nw += fg.gxw[i] * N;
      fg.blk_end[i] = nw;
    }
    wa.B = (int)B;
    fg.dW0 = dparams; fg.db0 = dparams + (size_t)H * g.F0;
    fg.gx0 = (g.F0 + 1 + 255) / 256; fg.nlayers = ML + 1;
    nblk += (unsigned)(fg.gx0 * H + nw);
  }
  RENI_LAUNCH(reni::k_film_grads, dim3(nblk), dim3(256), 0, s, g, wa, fg);
  return RENI_OK;
}

}  // namespace

// error hook of the other translation units (reni_tu_shade.hip): same thread-local message as fail()
namespace reni {
int reni_set_error(int code, const char* msg) { return fail(code, "%s", msg); }
void note_launches(int n) { g_launches.fetch_add(n, std::memory_order_relaxed); }
}  // namespace reni

extern "C" {

const char* reni_last_error(void) { return g_err.c_str(); }

int reni_plan_create(const reni_desc* d, reni_plan** out) {
  if (!d || !out) return fail(RENI_EINVAL, "desc/out_plan is NULL");
  *out = nullptr;
  if (d->equivariance < 0 || d->equivariance > 2) return fail(RENI_EINVAL, "equivariance %d not in {NONE,SO2,SO3}", d->equivariance);
  if (d->ndims < 1 || d->ndims > 256) return fail(RENI_EINVAL, "ndims=%d out of range", d->ndims);
  if (d->out_features != 3) return fail(RENI_EUNSUPPORTED, "out_features=%d (only 3 supported)", d->out_features);
  if (d->hidden_layers < 0 || d->hidden_layers > reni::MAX_LAYERS - 1) return fail(RENI_EUNSUPPORTED, "hidden_layers=%d unsupported", d->hidden_layers);
  if (d->hidden_features != 32 && d->hidden_features != 64 && d->hidden_features != 128 && d->hidden_features != 256)
    return fail(RENI_EUNSUPPORTED, "hidden_features=%d unsupported (32, 64, 128, 256)", d->hidden_features);
  if (d->output_activation < 0 || d->output_activation > 2) return fail(RENI_EINVAL, "output_activation %d", d->output_activation);
  if (d->dtype != RENI_F32 && d->dtype != RENI_BF16) return fail(RENI_EINVAL, "dtype %d", d->dtype);
  if (d->conditioning != RENI_COND_CONCAT && d->conditioning != RENI_COND_FILM) return fail(RENI_EINVAL, "conditioning %d", d->conditioning);
  if (d->conditioning == RENI_COND_FILM) {
    // the reference's "None" FiLM encoding cannot run (in_features / mn_in_features are swapped,
    // src/models/RENI.py:552-555 vs :449-452), so there is nothing to be compatible with
    if (d->equivariance == RENI_EQ_NONE) return fail(RENI_EUNSUPPORTED, "FiLM with equivariance None is not runnable in the reference either");
    if (!d->last_layer_linear) return fail(RENI_EINVAL, "FiLM decoders end in a linear layer (RENI.py:570)");
  }
  reni_plan* p = new (std::nothrow) reni_plan;
  if (!p) return fail(RENI_EINVAL, "out of host memory");
  memset(p, 0, sizeof(*p));
  p->d = *d;
  // (a switch is ON when its variable is set to anything but "" or "0": `RENI_NO_PERSIST=0` used to mean ON -- set is set -- and cost
  //  round 6 an A/B whose two legs were the same kernels)
  auto env_on = [](const char* name) { const char* e = getenv(name); return e != nullptr && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0'); };
  p->no_persist = env_on("RENI_NO_PERSIST");
  p->no_side_stream = env_on("RENI_NO_SIDE_STREAM");
  p->dw1_old = env_on("RENI_DW1_OLD");
  p->no_l0x = env_on("RENI_NO_L0X");
  p->frag_ws_cap = (size_t)16 << 30;  // (round 5: 16 GB of a 288 GB device -- 3 GB before: config 2's 64 images at 5 x 256 took four passes)
  {  // ... and never more than a quarter of what the current device has free when the plan is made (ADVICE r05: a constant 16 GB is an
     // out-of-memory risk on a shared or smaller device); without a device (the CPU-side checks) the constant stands
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const size_t quarter = fr / 4 > ((size_t)1 << 30) ? fr / 4 : ((size_t)1 << 30);
      if (quarter < p->frag_ws_cap) p->frag_ws_cap = quarter;
    } else {
      (void)hipGetLastError();
    }
  }
  if (const char* e = getenv("RENI_FRAG_WS_CAP_MB")) { const long long mb = atoll(e); if (mb > 0) { p->frag_ws_cap = (size_t)mb << 20; p->env_overrides |= 4; } }
  if (const char* e = getenv("RENI_TRAIN_WG")) { const int n = atoi(e); if (n > 0) { p->train_wg = n; p->env_overrides |= 32; } }
  p->env_overrides |= (p->no_persist ? 1 : 0) | (p->no_side_stream ? 2 : 0) | (p->dw1_old ? 8 : 0) | (p->no_l0x ? 16 : 0);
  const int nd = d->ndims, H = d->hidden_features, L = d->hidden_layers;
  if (d->conditioning == RENI_COND_FILM) {
    p->F_in = d->equivariance == RENI_EQ_SO2 ? 2 + nd : nd;  // Siren_Input width, RENI.py:441,556-561
    p->d.first_omega_0 = 1.f;  // the first layer's frequency is folded into the caller's affine map
  } else {
    p->F_in = d->equivariance == RENI_EQ_SO2 ? 2 * nd + nd * nd + 2 : d->equivariance == RENI_EQ_SO3 ? nd + nd * nd : 4 * nd;
  }
  size_t o = 0;
  p->p_off_w[0] = 0; o += (size_t)H * p->F_in;
  p->p_off_b[0] = (unsigned)o; o += H;
  p->n_first = (int64_t)o;
  for (int i = 1; i <= L; ++i) {
    p->p_off_w[i] = (unsigned)o; o += (size_t)H * H;
    p->p_off_b[i] = (unsigned)o; o += H;
  }
  p->p_off_w[L + 1] = (unsigned)o; o += 3 * (size_t)H;
  p->p_off_b[L + 1] = (unsigned)o; o += 3;
  p->n_params = (int64_t)o;
  if (d->conditioning == RENI_COND_FILM && d->mapping_layers > 0) {
    if (d->mapping_layers > reni::MAX_MAP_LAYERS) { delete p; return fail(RENI_EUNSUPPORTED, "mapping_layers=%d unsupported", d->mapping_layers); }
    if (d->mapping_features < 1 || d->mapping_features > 4096) { delete p; return fail(RENI_EINVAL, "mapping_features=%d", d->mapping_features); }
    p->M_in = d->equivariance == RENI_EQ_SO2 ? nd * nd + nd : nd * nd;  // RENI.py:556-561
    p->N_out = 2 * (L + 1) * H;
    size_t m = 0;
    for (int i = 0; i <= d->mapping_layers; ++i) {
      const size_t N = (i < d->mapping_layers) ? d->mapping_features : p->N_out;
      const size_t K = (i == 0) ? p->M_in : d->mapping_features;
      p->mw_off[i] = (unsigned)m; m += N * K;
      p->mb_off[i] = (unsigned)m; m += N;
    }
    p->n_map_params = (int64_t)m;
  }
  *out = p;
  return RENI_OK;
}

void reni_plan_destroy(reni_plan* p) { delete p; }

int64_t reni_param_count(const reni_plan* p) { return p ? p->n_params : 0; }
int32_t reni_in_features(const reni_plan* p) { return p ? p->F_in : 0; }

size_t reni_workspace_bytes(const reni_plan* p, int64_t B, int64_t P, uint32_t flags) {
  GeoRt g;
  if (!p || B < 1 || P < 1 || !geo_for(p, &g)) return 0;
  // sized for the backward entry points so that one buffer serves every call.  The layout is the one the calls will use NOW:
  // RENI_NO_PERSIST is read here as it is there (sizing for both kernel choices made the headline path ask for 5.7 GB
  // instead of 0.7 GB); a caller that flips the variable between sizing and calling gets RENI_EWORKSPACE, not a wrong result.
  size_t n = backward_layout(p, g, B, P, flags).total;
  const int64_t bc = frag_chunk_images(p, B, P, flags);  // (H = 256 training: in image chunks, see run_backward_chunked)
  if (bc < B) n = al256(backward_layout(p, g, bc, P, flags).total) + al256((size_t)p->n_params * 4) + 256;
  if (p->d.conditioning == RENI_COND_FILM && p->d.mapping_layers > 0) n = al256(n) + make_glue_layout(p, B).total;
  return n;
}

int reni_launch_info(const reni_plan* p, int64_t B, int64_t P, int32_t* info4) {
  GeoRt g;
  if (!p || !info4 || !geo_for(p, &g)) return fail(RENI_EINVAL, "bad argument");
  const Layout l = make_layout(p, g, B, P, RENI_NEED_DW | RENI_NEED_DZ, true);
  info4[0] = l.nwg; info4[1] = 256; info4[2] = l.persist ? -1 : g.lds_bytes; info4[3] = l.n_tiles;
  return RENI_OK;
}

int reni_path_info(const reni_plan* p, int64_t B, int64_t P, uint32_t flags, int32_t* info8) {
  GeoRt g;
  if (!p || !info8 || B < 1 || P < 1 || !geo_for(p, &g)) return fail(RENI_EINVAL, "bad argument");
  const Layout l = make_layout(p, g, B, P, flags, true);
  info8[0] = l.persist;                                                    // register-persistent kernels (k_reni_train_bf16)
  // dW_1: none / k_reni_dw1_ring (given aligned directions) / k_reni_dw1 /
  // 3: k_reni_l0_ring behind the L0X training instance (layer 0's backward + dW_1; given, in addition, WeightedMSE and no output image)
  // (the *_plan_ok halves of the predicates run_backward decides with: what a call's pointers and loss add is not known here)
  info8[1] = !l.pdw ? 0 : l0x_plan_ok(p, l, P, flags) ? 3 : dw1_ring_plan_ok(p, P) ? 1 : 2;
  // "a side stream is ALLOWED for this plan", not "this call forks": a call forks (BwdPath::fork) when, in addition, it is not an L0X call
  // and -- concat decoder -- has at least eight tiles per workgroup.  bench.py records this value.
  info8[2] = side_stream_plan_ok(p, l) ? 1 : 0;
  info8[3] = (int32_t)frag_chunk_images(p, B, P, flags);                   // images per chunk of the H = 256 training path (B = one pass)
  info8[4] = l.stream;                                                     // operand stream (k_dw_stream / k_dw_frag)
  info8[5] = l.frag;                                                       // fragment stream: 1 bf16, 2 fp32
  info8[6] = p->env_overrides;                                             // selectors the environment set (0 in a clean run)
  info8[7] = l.nwg;
  return RENI_OK;
}

int reni_set_grad_ready_event(void* hip_event) {
  g_ev_rest = (hipEvent_t)hip_event;
  return RENI_OK;
}

int64_t reni_launch_count(int32_t reset) {
  return reset ? g_launches.exchange(0, std::memory_order_relaxed) : g_launches.load(std::memory_order_relaxed);
}

static int forward_impl(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D, int64_t dbs,
                        const float* params, float* out, void* ws_v, size_t ws_bytes, void* stream, const FilmIO* fio) {
  int rc = fio ? check_film(p, fio, false) : RENI_OK;
  if (rc) return rc;
  if (!fio && p && p->d.conditioning != RENI_COND_CONCAT) return fail(RENI_EINVAL, "FiLM plan: use the reni_film_* entry points");
  rc = check_common(p, B, P, fio ? fio->A : Z, D, params, ws_v);
  if (rc) return rc;
  if (!out) return fail(RENI_EINVAL, "out is NULL");
  GeoRt g;
  if (!geo_for(p, &g)) return fail(RENI_EUNSUPPORTED, "hidden_features=%d unsupported", p->d.hidden_features);
  DeviceGuard dev_guard;
  rc = dev_guard.enter(params);
  if (rc) return rc;
  const Layout l = make_layout(p, g, B, P, 0, false);
  if (ws_bytes < l.total) return fail(RENI_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", l.total, ws_bytes);
  char* ws = (char*)ws_v;
  hipStream_t s = (hipStream_t)stream;
  rc = run_prologue(p, g, l, B, Z, params, ws, false, s, nullptr, fio ? fio->A : nullptr);
  if (rc) return rc;
  reni::MainArgs a;
  fill_main_args(a, p, l, B, P, Z, D, dbs, ws);
  if (fio) { a.Apre = fio->A; a.film = fio->film; a.params = params; a.Z = nullptr; }
  a.out = out;
  if (l.persist) return launch_train(p, a, l.nwg, s, true);  // forward-only instance (a.target == NULL: no statistics)
  return launch_main(p, reni::MODE_FWD, a, l.nwg, s);
}

int reni_forward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D, int64_t dbs,
                 const float* params, float* out, void* ws, size_t ws_bytes, void* stream) {
  return forward_impl(p, B, P, Z, D, dbs, params, out, ws, ws_bytes, stream, nullptr);
}

int reni_film_forward(const reni_plan* p, int64_t B, int64_t P, const float* D, int64_t dbs, const float* A,
                      const float* film, const float* params, float* out, void* ws, size_t ws_bytes, void* stream) {
  FilmIO fio;
  fio.A = A; fio.film = film;
  return forward_impl(p, B, P, nullptr, D, dbs, params, out, ws, ws_bytes, stream, &fio);
}

int reni_film_forward_loss_backward(const reni_plan* p, int64_t B, int64_t P, const float* D, int64_t dbs,
                                    const float* A, const float* film, const float* params, const float* target,
                                    const int64_t ts[3], const float* weight, const int64_t wst[3],
                                    int32_t loss_kind, float beta, uint32_t flags, float* out, float* loss_terms,
                                    float* dA, float* dfilm, float* dparams, void* ws, size_t ws_bytes,
                                    void* stream) {
  FilmIO fio;
  fio.A = A; fio.film = film; fio.dA = dA; fio.dfilm = dfilm;
  BwdCall c;
  c.B = B; c.P = P; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.beta = beta;
  c.flags = flags; c.out = out; c.loss_terms = loss_terms; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream; c.fio = &fio;
  return run_backward(p, c);
}

int reni_film_backward(const reni_plan* p, int64_t B, int64_t P, const float* D, int64_t dbs, const float* A,
                       const float* film, const float* params, const float* dout, uint32_t flags, float* dA,
                       float* dfilm, float* dparams, void* ws, size_t ws_bytes, void* stream) {
  FilmIO fio;
  fio.A = A; fio.film = film; fio.dA = dA; fio.dfilm = dfilm;
  BwdCall c;
  c.B = B; c.P = P; c.D = D; c.dbs = dbs; c.params = params;
  c.dout = dout; c.loss_kind = LOSS_DOUT;
  c.flags = flags; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream; c.fio = &fio;
  return run_backward(p, c);
}

int reni_forward_loss_backward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D,
                               int64_t dbs, const float* params, const float* target, const int64_t ts[3],
                               const float* weight, const int64_t wst[3], int32_t loss_kind, float alpha,
                               float beta, uint32_t flags, float* out, float* loss_terms, float* dZ,
                               float* dparams, void* ws, size_t ws_bytes, void* stream) {
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.alpha = alpha; c.beta = beta;
  c.flags = flags; c.out = out; c.loss_terms = loss_terms; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  return run_backward_chunked(p, c);
}

int reni_forward_loss_backward_rows(const reni_plan* p, int64_t B, int64_t P, const float* Z_table, int64_t n_rows,
                                    const int64_t* idx, const float* D, int64_t dbs, const float* params, const float* target,
                                    const int64_t ts[3], const float* weight, const int64_t wst[3], int32_t loss_kind,
                                    float alpha, float beta, uint32_t flags, float* out, float* loss_terms, float* dZ,
                                    float* dparams, void* ws, size_t ws_bytes, void* stream) {
  if (!idx) return fail(RENI_EINVAL, "idx is NULL");
  if (n_rows < 1) return fail(RENI_EINVAL, "n_rows=%lld must be >= 1", (long long)n_rows);
  if (p && p->d.conditioning != RENI_COND_CONCAT) return fail(RENI_EINVAL, "FiLM plan: use the reni_film_* entry points");
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z_table; c.idx = idx; c.n_rows = n_rows; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.alpha = alpha; c.beta = beta;
  c.flags = flags; c.out = out; c.loss_terms = loss_terms; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  return run_backward_chunked(p, c);
}

// reni_latent_step_rows (weight_lists == NULL: the lists are rebuilt by the call) and reni_latent_step_rows_cached
static int latent_step_rows(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx, const float* D,
                            int64_t dbs, const float* params, const float* target, const int64_t ts[3], const float* weight,
                            const int64_t wst[3], int32_t loss_kind, float alpha, float beta, uint32_t flags, const void* weight_lists,
                            float* m_lat, float* v_lat, float lr, float b1, float b2, float eps, int64_t step, float* loss_terms,
                            float* dZ, void* ws, size_t ws_bytes, void* stream) {
  if (!idx) return fail(RENI_EINVAL, "idx is NULL");
  if (n_rows < 1 || step < 1) return fail(RENI_EINVAL, "n_rows=%lld step=%lld", (long long)n_rows, (long long)step);
  if (!m_lat || !v_lat || !dZ) return fail(RENI_EINVAL, "NULL optimiser state / output buffer");
  if (p && p->d.conditioning != RENI_COND_CONCAT) return fail(RENI_EINVAL, "FiLM plan: use reni_film_model_forward_loss_backward + reni_adam_rows_step");
  const uint32_t mode = flags & (RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT);
  if (!weight_lists) {
    if (flags & ~(uint32_t)(RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT)) return fail(RENI_EINVAL, "flags: RENI_WEIGHT_SPARSE / RENI_WEIGHT_COMPACT or 0");
  } else {
    if (!mode || (flags & ~(uint32_t)(RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT | RENI_WEIGHT_COS_CONSTANT)))
      return fail(RENI_EINVAL, "flags: RENI_WEIGHT_SPARSE or RENI_WEIGHT_COMPACT (the mode the lists were built for) [| RENI_WEIGHT_COS_CONSTANT]");
    if (((uintptr_t)weight_lists & 255) != 0) return fail(RENI_EINVAL, "weight_lists must be 256-byte aligned");
    if (p && B >= 1 && P >= 1 && frag_chunk_images(p, B, P, flags | RENI_NEED_DZ) < B) return fail(RENI_EUNSUPPORTED, "chunked problems take reni_latent_step_rows");
    // the lists must be the ones THIS library built for THIS shape and mode (their layout is a function of B and P)
    ListRecord r{};
    const int known = lists_check(weight_lists, B, P, mode, &r);
    if (known == 1) return fail(RENI_EINVAL, "weight_lists: no reni_weight_lists_build is on record for this buffer");
    if (known == 2) return fail(RENI_EINVAL, "weight_lists were built for B=%lld P=%lld mode=%u, this call has B=%lld P=%lld mode=%u",
                                (long long)r.B, (long long)r.P, r.mode, (long long)B, (long long)P, mode);
  }
  // the frozen-decoder gradient call (the batch's rows are gathered into the workspace by its prologue: the table is free to move
  // behind it), then the dense Adam step on the table -- the two calls this replaces, in their order, on the caller's stream
  const WeightLists wl = {(const char*)weight_lists, flags};
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z_table; c.idx = idx; c.n_rows = n_rows; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.alpha = alpha; c.beta = beta;
  c.flags = flags | RENI_NEED_DZ; c.loss_terms = loss_terms; c.dZ = dZ;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  if (weight_lists) c.lists = &wl;
  const int rc = weight_lists ? run_backward(p, c) : run_backward_chunked(p, c);
  if (rc) return rc;
  return reni_adam_rows_step(Z_table, dZ, idx, B, (int64_t)p->d.ndims * 3, m_lat, v_lat, n_rows, lr, b1, b2, eps, step, 1.f, stream);
}

int reni_latent_step_rows(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx, const float* D,
                          int64_t dbs, const float* params, const float* target, const int64_t ts[3], const float* weight,
                          const int64_t wst[3], int32_t loss_kind, float alpha, float beta, uint32_t flags, float* m_lat, float* v_lat,
                          float lr, float b1, float b2, float eps, int64_t step, float* loss_terms, float* dZ, void* ws, size_t ws_bytes,
                          void* stream) {
  return latent_step_rows(p, B, P, Z_table, n_rows, idx, D, dbs, params, target, ts, weight, wst, loss_kind, alpha, beta, flags, nullptr,
                          m_lat, v_lat, lr, b1, b2, eps, step, loss_terms, dZ, ws, ws_bytes, stream);
}

int reni_latent_step_rows_cached(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                                 const float* D, int64_t dbs, const float* params, const float* target, const int64_t ts[3],
                                 const float* weight, const int64_t wst[3], int32_t loss_kind, float alpha, float beta, uint32_t flags,
                                 const void* weight_lists, float* m_lat, float* v_lat, float lr, float b1, float b2, float eps,
                                 int64_t step, float* loss_terms, float* dZ, void* ws, size_t ws_bytes, void* stream) {
  if (!weight_lists) return fail(RENI_EINVAL, "weight_lists is NULL (reni_weight_lists_build; without lists: reni_latent_step_rows)");
  return latent_step_rows(p, B, P, Z_table, n_rows, idx, D, dbs, params, target, ts, weight, wst, loss_kind, alpha, beta, flags, weight_lists,
                          m_lat, v_lat, lr, b1, b2, eps, step, loss_terms, dZ, ws, ws_bytes, stream);
}

size_t reni_weight_lists_bytes(int64_t B, int64_t P) {
  if (B < 1 || P < 1) return 0;
  return make_list_layout(B, P).total;
}

int reni_weight_lists_build(int64_t B, int64_t P, const float* weight, const int64_t wst[3], uint32_t flags, void* lists,
                            size_t lists_bytes, int32_t* summary_host, void* stream) {
  if (B < 1 || P < 1 || !weight || !wst || !lists) return fail(RENI_EINVAL, "bad argument");
  if (!(flags & (RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT)) || (flags & ~(uint32_t)(RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT)))
    return fail(RENI_EINVAL, "flags: RENI_WEIGHT_SPARSE or RENI_WEIGHT_COMPACT");
  if (((uintptr_t)lists & 255) != 0) return fail(RENI_EINVAL, "lists must be 256-byte aligned");
  if (B * ((P + 127) / 128) > 0x3fffffffLL) return fail(RENI_EINVAL, "problem too large");
  const ListLayout ll = make_list_layout(B, P);
  if (lists_bytes < ll.total) return fail(RENI_EWORKSPACE, "lists buffer too small: need %zu bytes, got %zu", ll.total, lists_bytes);
  DeviceGuard dev_guard;
  int rc = dev_guard.enter(weight);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* lb = (char*)lists;
  const int tpi = (int)((P + 127) / 128);
  const ListDst ld = list_dst(lb, ll);
  rc = build_weight_lists(weight, wst, P, tpi, (int)(B * tpi), (flags & RENI_WEIGHT_COMPACT) != 0, ld, s);
  if (rc) return rc;
  const long long hdr[4] = {(long long)B, (long long)P, (long long)(flags & (RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT)), LIST_MAGIC};
  HIP_TRY(hipMemcpyAsync(lb + ll.o_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
  lists_remember(lists, B, P, flags & (RENI_WEIGHT_SPARSE | RENI_WEIGHT_COMPACT));
  HIP_TRY(hipMemsetAsync(lb + ll.o_zstats, 0, (size_t)B * 16 * 4, s));
  if (summary_host) {  // (one synchronisation, once per mask: what the lists hold -- the caller may then set RENI_WEIGHT_COS_CONSTANT)
    int cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, ld.tcount, sizeof(cnt), hipMemcpyDeviceToHost, s));
    std::vector<int> ic((size_t)B);
    HIP_TRY(hipMemcpyAsync(ic.data(), ld.imgcos, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int live = 0;
    for (int64_t b = 0; b < B; ++b) live += ic[(size_t)b] != 0;
    summary_host[0] = cnt[0]; summary_host[1] = cnt[1]; summary_host[2] = live;
  }
  return RENI_OK;
}

// reni_train_step_rows (comm == NULL: the single-process step) and reni_train_step_rows_dp
static int train_step_rows(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                           const int64_t* idx_next, const float* D, int64_t dbs, float* params, const float* target,
                           const int64_t ts[3], const float* weight, const int64_t wst[3], int32_t loss_kind, float alpha, float beta,
                           float* m_dec, float* v_dec, float* m_lat, float* v_lat, float lr, float b1, float b2, float eps,
                           int64_t step, float grad_scale, void* comm, int32_t overlap, uint32_t* stage_state, float* loss_terms,
                           float* dZ, float* dparams, void* ws, size_t ws_bytes, void* stream) {
  if (!idx) return fail(RENI_EINVAL, "idx is NULL");
  if (n_rows < 1 || step < 1) return fail(RENI_EINVAL, "n_rows=%lld step=%lld", (long long)n_rows, (long long)step);
  if (!m_dec || !v_dec || !m_lat || !v_lat || !stage_state || !dZ || !dparams) return fail(RENI_EINVAL, "NULL optimiser state / output buffer");
  if (p && p->d.conditioning != RENI_COND_CONCAT)
    return fail(RENI_EINVAL, "FiLM plan: use reni_film_model_forward_loss_backward + %sreni_adam_step", comm ? "reni_allreduce_grads + " : "");
  if (loss_kind != RENI_LOSS_MSE && loss_kind != RENI_LOSS_TEST) return fail(RENI_EINVAL, "unknown loss_kind %d", loss_kind);
  StepFuse f;
  f.comm = comm; f.overlap = overlap ? 1 : 0;
  f.params = params; f.table = Z_table; f.m_dec = m_dec; f.v_dec = v_dec; f.m_lat = m_lat; f.v_lat = v_lat;
  f.lr = lr; f.b1 = b1; f.b2 = b2; f.eps = eps; f.gscale = grad_scale;
  f.bc1 = (float)(1.0 - std::pow((double)b1, (double)step));
  f.bc2_sqrt = (float)std::sqrt(1.0 - std::pow((double)b2, (double)step));
  f.idx_next = idx_next; f.state = stage_state;
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z_table; c.idx = idx; c.n_rows = n_rows; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.alpha = alpha; c.beta = beta;
  c.flags = RENI_NEED_DW | RENI_NEED_DZ; c.loss_terms = loss_terms; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  if (p && B >= 1 && P >= 1 && frag_chunk_images(p, B, P, c.flags) < B) {
    // H = 256 in image chunks: the chunks' gradients are summed first, then ONE exchange (with a communicator) and ONE optimiser step;
    // nothing is staged
    *stage_state = 0;
    int rc = run_backward_chunked(p, c);
    if (rc) return rc;
    if (comm) rc = reni_allreduce_grads(comm, dparams, (size_t)p->n_params, 1.f, stream);
    if (rc) return rc;
    return reni_adam_step2(params, dparams, m_dec, v_dec, p->n_params, Z_table, dZ, idx, B, (int64_t)p->d.ndims * 3, m_lat, v_lat,
                           n_rows, lr, b1, b2, eps, step, grad_scale, stream);
  }
  c.fuse = &f;
  return run_backward(p, c);
}

int reni_train_step_rows(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                         const int64_t* idx_next, const float* D, int64_t dbs, float* params, const float* target,
                         const int64_t ts[3], const float* weight, const int64_t wst[3], int32_t loss_kind, float alpha, float beta,
                         float* m_dec, float* v_dec, float* m_lat, float* v_lat, float lr, float b1, float b2, float eps,
                         int64_t step, float grad_scale, uint32_t* stage_state, float* loss_terms, float* dZ, float* dparams,
                         void* ws, size_t ws_bytes, void* stream) {
  return train_step_rows(p, B, P, Z_table, n_rows, idx, idx_next, D, dbs, params, target, ts, weight, wst, loss_kind, alpha, beta, m_dec, v_dec,
                         m_lat, v_lat, lr, b1, b2, eps, step, grad_scale, nullptr, 0, stage_state, loss_terms, dZ, dparams, ws, ws_bytes, stream);
}

int reni_train_step_rows_dp(const reni_plan* p, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                            const int64_t* idx_next, const float* D, int64_t dbs, float* params, const float* target,
                            const int64_t ts[3], const float* weight, const int64_t wst[3], int32_t loss_kind, float alpha, float beta,
                            float* m_dec, float* v_dec, float* m_lat, float* v_lat, float lr, float b1, float b2, float eps,
                            int64_t step, float grad_scale, void* comm, int32_t overlap, uint32_t* stage_state, float* loss_terms,
                            float* dZ, float* dparams, void* ws, size_t ws_bytes, void* stream) {
  if (!comm) return fail(RENI_EINVAL, "comm is NULL (reni_rccl_comm_create; one process: reni_train_step_rows)");
  return train_step_rows(p, B, P, Z_table, n_rows, idx, idx_next, D, dbs, params, target, ts, weight, wst, loss_kind, alpha, beta, m_dec, v_dec,
                         m_lat, v_lat, lr, b1, b2, eps, step, grad_scale, comm, overlap, stage_state, loss_terms, dZ, dparams, ws, ws_bytes, stream);
}

int reni_backward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D, int64_t dbs,
                  const float* params, const float* dout, uint32_t flags, float* dZ, float* dparams, void* ws,
                  size_t ws_bytes, void* stream) {
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z; c.D = D; c.dbs = dbs; c.params = params;
  c.dout = dout; c.loss_kind = LOSS_DOUT;
  c.flags = flags; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  return run_backward_chunked(p, c);
}

int64_t reni_film_map_param_count(const reni_plan* p) { return p ? p->n_map_params : 0; }

int reni_film_model_forward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D, int64_t dbs,
                            const float* params, const float* mparams, float* out, void* ws_v, size_t ws_bytes,
                            void* stream) {
  int rc = check_film_model(p, Z, mparams);
  if (rc) return rc;
  if (!ws_v) return fail(RENI_EWORKSPACE, "workspace is NULL");
  const size_t core = core_ws_bytes(p, B, P, 0);
  const GlueLayout gl = make_glue_layout(p, B);
  if (core == 0 || ws_bytes < core + gl.total)
    return fail(RENI_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", core + gl.total, ws_bytes);
  DeviceGuard dev_guard;
  rc = dev_guard.enter(params);
  if (rc) return rc;
  char* gw = (char*)ws_v + core;
  reni::FilmGlueArgs g;
  fill_glue(g, p, gl, B, Z, params, mparams, gw);
  rc = run_film_glue_fwd(g, (hipStream_t)stream);
  if (rc) return rc;
  FilmIO fio;
  fio.A = g.A; fio.film = g.film;
  return forward_impl(p, B, P, nullptr, D, dbs, params, out, ws_v, core, stream, &fio);
}

int reni_film_model_forward_loss_backward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D,
                                          int64_t dbs, const float* params, const float* mparams, const float* target,
                                          const int64_t ts[3], const float* weight, const int64_t wst[3],
                                          int32_t loss_kind, float alpha, float beta, uint32_t flags, float* out,
                                          float* loss_terms, float* dZ, float* dparams, float* dmparams, void* ws,
                                          size_t ws_bytes, void* stream) {
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z; c.D = D; c.dbs = dbs; c.params = params;
  c.target = target; c.ts = ts; c.weight = weight; c.wst = wst; c.loss_kind = loss_kind; c.alpha = alpha; c.beta = beta;
  c.flags = flags; c.out = out; c.loss_terms = loss_terms; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  return film_model_backward(p, c, mparams, dmparams);
}

int reni_film_model_backward(const reni_plan* p, int64_t B, int64_t P, const float* Z, const float* D, int64_t dbs,
                             const float* params, const float* mparams, const float* dout, uint32_t flags, float* dZ,
                             float* dparams, float* dmparams, void* ws, size_t ws_bytes, void* stream) {
  BwdCall c;
  c.B = B; c.P = P; c.Z = Z; c.D = D; c.dbs = dbs; c.params = params;
  c.dout = dout; c.loss_kind = LOSS_DOUT;
  c.flags = flags; c.dZ = dZ; c.dparams = dparams;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
  return film_model_backward(p, c, mparams, dmparams);
}

int reni_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                   float eps, int64_t step, float grad_scale, void* stream) {
  if (!p || !g || !m || !v) return fail(RENI_EINVAL, "NULL buffer");
  if (n < 0 || step < 1) return fail(RENI_EINVAL, "n=%lld step=%lld", (long long)n, (long long)step);
  if (n == 0) return RENI_OK;
  DeviceGuard dev_guard;
  int rc = dev_guard.enter(p);
  if (rc) return rc;
  const double bc1 = 1.0 - std::pow((double)b1, (double)step);
  const double bc2 = 1.0 - std::pow((double)b2, (double)step);
  RENI_LAUNCH(reni::k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     (long long)n, lr, b1, b2, eps, (float)bc1, (float)std::sqrt(bc2), grad_scale);
  return RENI_OK;
}

int reni_adam_rows_step(float* p, const float* g_rows, const int64_t* idx, int64_t B, int64_t row_len, float* m, float* v,
                        int64_t n_rows, float lr, float b1, float b2, float eps, int64_t step, float grad_scale,
                        void* stream) {
  if (!p || !g_rows || !idx || !m || !v) return fail(RENI_EINVAL, "NULL buffer");
  if (B < 0 || row_len < 1 || n_rows < 0 || step < 1 || B > 0x7fffffff || row_len > 0x7fffffff)
    return fail(RENI_EINVAL, "B=%lld row_len=%lld n_rows=%lld step=%lld", (long long)B, (long long)row_len, (long long)n_rows, (long long)step);
  const int64_t n = n_rows * row_len;
  if (n == 0) return RENI_OK;
  DeviceGuard dev_guard;
  int rc = dev_guard.enter(p);
  if (rc) return rc;
  const double bc1 = 1.0 - std::pow((double)b1, (double)step);
  const double bc2 = 1.0 - std::pow((double)b2, (double)step);
  RENI_LAUNCH(reni::k_adam_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g_rows,
                     (const long long*)idx, (int)B, (int)row_len, m, v, (long long)n, lr, b1, b2, eps, (float)bc1,
                     (float)std::sqrt(bc2), grad_scale);
  return RENI_OK;
}

int reni_adam_step2(float* p, const float* g, float* m, float* v, int64_t n, float* table, const float* g_rows,
                    const int64_t* idx, int64_t B, int64_t row_len, float* tm, float* tv, int64_t n_rows, float lr, float b1,
                    float b2, float eps, int64_t step, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || !table || !g_rows || !idx || !tm || !tv) return fail(RENI_EINVAL, "NULL buffer");
  if (n < 1 || B < 0 || row_len < 1 || n_rows < 1 || step < 1 || B > 0x7fffffff || row_len > 0x7fffffff)
    return fail(RENI_EINVAL, "n=%lld B=%lld row_len=%lld n_rows=%lld step=%lld", (long long)n, (long long)B, (long long)row_len,
                (long long)n_rows, (long long)step);
  DeviceGuard dev_guard;
  int rc = dev_guard.enter(p);
  if (rc) return rc;
  reni::Adam2Args a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.nb_dec = (int)((n + 255) / 256);
  a.tp = table; a.g_rows = g_rows; a.idx = (const long long*)idx; a.B = (int)B; a.row_len = (int)row_len;
  a.tm = tm; a.tv = tv; a.tn = n_rows * row_len;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = grad_scale;
  a.bc1 = (float)(1.0 - std::pow((double)b1, (double)step));
  a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow((double)b2, (double)step));
  a.skip_lo = 0; a.skip_hi = 0; a.l1_part = nullptr; a.l1_per_wg = 0; a.l1_nwg = 0; a.nb_l1 = 0; a.l1_scale = 1.f; a.skip_step = nullptr;
  const long long nb = a.nb_dec + (a.tn + 255) / 256;
  RENI_LAUNCH(reni::k_adam2, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
  return RENI_OK;
}

// ---- RCCL (SURVEY.md section 8 (b) item 7, (e)): the one exchange step of the data-parallel path ------------------
// librccl is bound at first use (dlopen), so the library loads -- and every other entry point works -- on a box without it.
// Inside a PyTorch process the name resolves to the librccl PyTorch has already mapped: one RCCL per process.
namespace {
struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, reni_rccl_id, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
Rccl* rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (!r.h) return;
    r.GetUniqueId = (int (*)(void*))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(void**, int, reni_rccl_id, int))dlsym(r.h, "ncclCommInitRank");
    r.CommDestroy = (int (*)(void*))dlsym(r.h, "ncclCommDestroy");
    r.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclAllReduce");
    r.GetErrorString = (const char* (*)(int))dlsym(r.h, "ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce && r.GetErrorString;
  });
  return r.ok ? &r : nullptr;
}
int rccl_fail(Rccl* r, const char* what, int e) { return fail(RENI_EHIP, "%s failed: %s", what, r->GetErrorString(e)); }
int rccl_allreduce_inplace(void* comm, float* buf, size_t n, hipStream_t s) {
  if (n == 0) return RENI_OK;
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  const int e = r->AllReduce(buf, buf, n, /*ncclFloat32*/ 7, /*ncclSum*/ 0, comm, s);
  return e ? rccl_fail(r, "ncclAllReduce", e) : RENI_OK;
}
int rccl_allreduce_max_i32(void* comm, int* buf, size_t n, hipStream_t s) {
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  const int e = r->AllReduce(buf, buf, n, /*ncclInt32*/ 2, /*ncclMax*/ 2, comm, s);
  return e ? rccl_fail(r, "ncclAllReduce", e) : RENI_OK;
}
}  // namespace

int reni_rccl_unique_id(reni_rccl_id* id) {
  if (!id) return fail(RENI_EINVAL, "id is NULL");
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  const int e = r->GetUniqueId(id);
  return e ? rccl_fail(r, "ncclGetUniqueId", e) : RENI_OK;
}

int reni_rccl_comm_create(const reni_rccl_id* id, int32_t nranks, int32_t rank, void** comm) {
  if (!id || !comm) return fail(RENI_EINVAL, "id / comm is NULL");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(RENI_EINVAL, "rank %d of %d", rank, nranks);
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  const int e = r->CommInitRank(comm, nranks, *id, rank);  // (collective: every rank calls it with the same id; current device)
  return e ? rccl_fail(r, "ncclCommInitRank", e) : RENI_OK;
}

int reni_rccl_comm_destroy(void* comm) {
  if (!comm) return RENI_OK;
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  const int e = r->CommDestroy(comm);
  return e ? rccl_fail(r, "ncclCommDestroy", e) : RENI_OK;
}

int reni_allreduce_grads(void* comm, float* flat, size_t n, float scale, void* stream) {
  if (!comm || !flat) return fail(RENI_EINVAL, "comm / flat is NULL");
  if (n == 0) return RENI_OK;
  Rccl* r = rccl();
  if (!r) return fail(RENI_EUNSUPPORTED, "librccl could not be loaded");
  DeviceGuard dev_guard;
  int rc = dev_guard.enter(flat);
  if (rc) return rc;
  const int e = r->AllReduce(flat, flat, n, /*ncclFloat32*/ 7, /*ncclSum*/ 0, comm, (hipStream_t)stream);
  if (e) return rccl_fail(r, "ncclAllReduce", e);
  if (scale != 1.f) {
    RENI_LAUNCH(reni::k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flat, n, scale);
  }
  return RENI_OK;
}

int reni_profile_enable(int32_t on) {
  g_prof_on = on != 0;
  return RENI_OK;
}

int reni_profile_read_kind(int32_t kind, double* total_ms, int64_t* launches, int32_t reset) {
  if (!total_ms || !launches) return fail(RENI_EINVAL, "NULL output");
  double tot = 0.0;
  int64_t n = 0;
  for (size_t i = 0; i < g_prof_used; ++i) {
    if (kind >= 0 && g_prof_pool[i].kind != kind) continue;
    HIP_TRY(hipEventSynchronize(g_prof_pool[i].b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof_pool[i].a, g_prof_pool[i].b));
    tot += ms;
    ++n;
  }
  *total_ms = tot;
  *launches = n;
  if (reset) g_prof_used = 0;
  return RENI_OK;
}

int reni_profile_minmax(int32_t kind, double* min_ms, double* max_ms) {
  if (!min_ms || !max_ms) return fail(RENI_EINVAL, "NULL output");
  double lo = 0.0, hi = 0.0;
  bool any = false;
  for (size_t i = 0; i < g_prof_used; ++i) {
    if (kind >= 0 && g_prof_pool[i].kind != kind) continue;
    HIP_TRY(hipEventSynchronize(g_prof_pool[i].b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof_pool[i].a, g_prof_pool[i].b));
    if (!any || ms < lo) lo = ms;
    if (!any || ms > hi) hi = ms;
    any = true;
  }
  *min_ms = lo; *max_ms = hi;
  return RENI_OK;
}

int reni_profile_read(double* total_ms, int64_t* launches, int32_t reset) {
  return reni_profile_read_kind(PROF_FWD_BWD, total_ms, launches, reset);
}

int reni_probe_tr(const int32_t* lane_addr_host, int32_t mode, uint16_t* out_host) {
  unsigned short* d = nullptr; int* da = nullptr;
  HIP_TRY(hipMalloc(&d, 256 * sizeof(unsigned short)));
  HIP_TRY(hipMalloc(&da, 64 * sizeof(int)));
  if (lane_addr_host) HIP_TRY(hipMemcpy(da, lane_addr_host, 64 * sizeof(int), hipMemcpyHostToDevice));
  RENI_LAUNCH(reni::k_probe_tr, dim3(1), dim3(64), 0, 0, d, da, mode);
  HIP_TRY(hipMemcpy(out_host, d, 256 * sizeof(unsigned short), hipMemcpyDeviceToHost));
  (void)hipFree(d); (void)hipFree(da);
  return RENI_OK;
}

int reni_selftest_layouts(int32_t* out_mismatch, int32_t n_probes) {
  if (!out_mismatch || n_probes < 2) return fail(RENI_EINVAL, "need room for 2 probes");
  float* d = nullptr;
  HIP_TRY(hipMalloc(&d, 32 * 32 * sizeof(float)));
  std::vector<float> h(32 * 32);
  for (int which = 0; which < 2; ++which) {
    HIP_TRY(hipMemset(d, 0xff, 32 * 32 * sizeof(float)));
    RENI_LAUNCH(reni::k_probe, dim3(1), dim3(64), 0, 0, d, which);
    HIP_TRY(hipMemcpy(h.data(), d, 32 * 32 * sizeof(float), hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < 32; ++i)
      for (int n = 0; n < 32; ++n) {
        double ref = 0;
        if (which == 0) {
          for (int k = 0; k < 2; ++k) ref += (1.0 + i + 100.0 * k) * (3.0 + 2.0 * n + 7.0 * k);
        } else {
          for (int k = 0; k < 16; ++k) ref += (double)(((i + 3 * k) % 7) - 3) * (double)(((2 * n + k) % 5) - 2);
        }
        if (std::fabs((double)h[i * 32 + n] - ref) > 1e-3) ++bad;
      }
    out_mismatch[which] = bad;
  }
  (void)hipFree(d);
  return RENI_OK;
}

}  // extern "C"
