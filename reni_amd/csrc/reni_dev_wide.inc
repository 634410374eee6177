// reni_dev_wide.inc -- k_reni_wide256: the register-persistent bf16 chain at H = 256 (frozen decoder / statistics / inference / the training chain in front of k_dw_frag)
// Part of reni_device.inc (RENI_TU_WIDE only; inside namespace reni; never compiled on its own).
//
// Round 5 (VERDICT r04 item 4).  H = 256 is the width of every configuration the reference ships (/root/reference/configs/default.py:13,
// experiment.yaml); until now it ran on the generic k_reni_main: fp32 activations between layers, operands packed per chunk, one wave
// per SIMD issuing ~190 k cycles of instructions per tile in order -- 14 % of the bf16 MFMA peak (profiles/r04_h256.md).  This kernel is
// the H = 128 persistent kernel's structure at 256 features, for the calls that carry no weight gradient (src/models/RENI.py:86-87,
// 132-178 forward; the autograd backward through the layers for d loss / d Z -- BASELINE config 4's latent optimisation, config 5's
// inference, RENITestLoss's statistics pass):
//   * activations and gradients travel between layers as PACKED bf16 MFMA B operands (sixteen fragments = 64 registers per wave), the
//     sine argument in revolutions (omega / 2 pi rides on the packed images: PackDesc::scale), phases stashed as fp16 pairs;
//   * a layer's 128 KB weight image streams through two 64 KB LDS buffers in halves of four row blocks, fetched by LDS-DMA one half
//     ahead (the stream runs on across layers, passes and tiles); one barrier per half = per 64 MFMAs of a wave;
//   * the activation derivative is applied in the dX GEMM's epilogue (cos of the stashed phase x the fp32 accumulator, packed once);
//   * the LAST backward step is computed TRANSPOSED (k_reni_l0_ring's trick): g_0^T [sample][feature] = g_1^T W_1 with the packed g_1
//     fragments as A operands and the W_1^T image's fragments as B operands, theta_0^T = X . A_b^T the same way, so that
//     g_0^T (.) cos(theta_0^T), packed, IS the A operand of dA = g_0 X^T -- no transposition image of g_0 (64 KB this kernel's LDS
//     does not have), only the 9-component X^T operand goes through a private LDS region.
// One workgroup = eight waves on TWO 128-sample tiles (waves 0..3: tile 2 it, waves 4..7: tile 2 it + 1; 4 waves x 32
// samples each), one workgroup per CU, two waves per SIMD: the two tiles share the weight stream (half the L2 -> LDS traffic, barriers
// and DMA issue per sample) and one wave's MFMAs run under the other's activation epilogue.  256 registers per wave: the backward GEMMs
// run in QUARTERS of two row blocks (two accumulator chains).  Tile pairs walked with stride gridDim.x (or MainArgs::tlist:
// RENI_WEIGHT_SPARSE; MainArgs::plist: RENI_WEIGHT_COMPACT); an odd tile count leaves the last pair's second group idle (it keeps the
// barriers and its share of the DMA, and stores nothing).  MODE 0: forward (+ output image, + the nine statistics sums per tile and wave when a target is given);
// MODE 1: forward + loss + backward, per-tile dA / loss partials (the reductions and latent tails are the generic path's).
// MODE 2: MODE 1 for a TRAINING call (RENI_NEED_DW): the producer of k_dw_frag's fragment stream, as k_reni_main's FRAG form is
// (reni_dev_main.inc) -- every tile keeps its phase stash (layer 0's too: h_0 for dW_1), g_L .. g_1 leave as the packed fragments
// they are held in (MainArgs::gfs: the same [chunk][thread] layout), and the head's g_y goes to a small fp32 stream behind the
// fragments ([tile][128 samples][4]) from which k_wide_head_dw forms dW_out / db_out (the generic chain transposes for them in LDS
// this kernel does not have).
struct Wide256 {
  static constexpr int H = 256, NRB = 8, NKS = 16;
  static constexpr int NWAVE = 8, NT = NWAVE / 4;   // waves per workgroup, tiles per workgroup
  static constexpr int HALF = 4 * NKS * 1024;                    // four row blocks of a hidden image: 64 KB
  static constexpr int BIAS_B = 1024;                            // a layer's 256 biases
  static constexpr int XT_ROW = 72, XT_BYTES = 9 * XT_ROW + 8;   // per wave: (x_hi | 1 | x_lo) component-major, 32 samples
  static constexpr int DAS_BYTES = 2 * NWAVE * 256 * 4;         // every wave's dA partials of two feature blocks (a tile's 128 samples = 4 waves x 32)
  static constexpr int LDS_BYTES = 2 * HALF + 2 * BIAS_B + NWAVE * XT_BYTES + DAS_BYTES;
  // FiLM forward instance: per tile group FT_LMAX layers x (freq | phase) x 256 floats in the X^T / dA region (unused by a forward pass)
  static constexpr int FT_LMAX = (NWAVE * XT_BYTES + DAS_BYTES) / (NT * 2 * 256 * 4);
  // FiLM training form: the tables alias the dA exchange alone (the X^T operands are written at the top of the tile and live to its end)
  static constexpr int FT_LMAX2 = DAS_BYTES / (NT * 2 * 256 * 4);
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// FILM = true (round 6; MODE 0 only): the forward / statistics pass of the reference's DEFAULT model at its shipped width
// (configs/default.py:9,13: FiLM conditioning, 256 features; src/models/RENI.py:508-519, 565-586, 665-676) -- hidden layer l of image b
// applies sin(freq_bl . (W_l h + b_l) + phase_bl).  The forward images stay plain (as for the H = 128 FiLM instances), the per-image
// (freq / 2 pi | phase / 2 pi) tables of the workgroup's two tiles' images sit in LDS -- in the region the backward modes use for their
// X^T operands and dA partials, which a forward pass does not have -- and enter the activation as one FMA + v_fract (FiLM angles reach
// tens of revolutions).  The folded first layer arrives as the caller's per-image affine map (afrag, in revolutions).
// Scales: the hidden layers' FORWARD images (and biases) carry 1 / 2 pi (k_pack, reni_capi.inc), the tables are [freq | phase / 2 pi] --
// angle in revolutions = acc . freq + phase / 2 pi: one FMA -- and the W^T images are plain, so that the same frequency row serves the
// backward epilogue (g_a = freq . g_theta) and the stream's g_theta needs no rescaling.
// MODE 2 with FILM (round 6): the chain of every FiLM backward call -- trainable or frozen decoder: d(freq) / d(phase) are per-image sums
// of the weight-gradient GEMMs' operands, so k_dw_frag<256, true> runs either way -- as the producer of the same fragment stream the
// generic chain writes: g_theta = cos(theta) . g_h goes to the stream (k_dw_frag applies the frequency where its sums need it), the
// chain goes on with g_a = freq . g_theta.  Its tables (<= FT_LMAX2 = 4 hidden
// layers: the default model's) sit in the dA-exchange region, which only the tile's LAST step uses: staged at the top of every tile pair.
// The training form's fragment stream -- g_l (k_dw_frag's operand, 64 KB per layer and tile), the head's g_y --
// leaves through NON-TEMPORAL stores: written once, read by another kernel much later.  With plain stores the stream pushed the tile's own phase
// stash -- which this kernel reads back in its backward pass -- out of the L2 / Infinity Cache: chain 4.38 -> 3.84 ms, config 2 at 256 features
// 6.79 -> 6.26 ms same box.  (The H = 128 kernel's g_1 stream is read by k_reni_l0_ring straight away, out of the Infinity Cache: plain stores,
// non-temporal ones cost +1.3 % on the step.)
template <int MODE, bool FILM = false>
__global__ void __launch_bounds__(64 * Wide256::NWAVE, 1) k_reni_wide256(const MainArgs a) {
  static_assert(!FILM || MODE == 0 || MODE == 2, "FiLM: the forward / statistics instance and the training form (which also serves a frozen decoder)");
  using W = Wide256;
  using G = Geo<PolBF16, 256>;
  constexpr int NRB = W::NRB, NKS = W::NKS, H = W::H;
  static_assert(G::IMG_HID == 2 * W::HALF && G::STASH_CH == 16, "image / stash geometry");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* const BIAS = smem + 2 * W::HALF;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // of the workgroup: DMA share, private LDS regions
  const int grp = wave >> 2, wq = wave & 3, tl = tid & 255;    // tile of the pair, wave and thread within that tile's chain
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  const unsigned lane16 = (unsigned)lane * 16;
  char* const xt = BIAS + 2 * W::BIAS_B + wave * W::XT_BYTES;
  const int L = a.L;
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  auto pk = [](float x, float y) -> unsigned { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, y}, bf16x2)); };

  // ---- the chunk stream: chunk k of a tile (see the header) -> (source, 1 KB pieces, bias source)
  const int nch = MODE >= 1 ? 4 * L + 2 : 2 * L + 1;
  struct Chunk { const char* src; int pieces; const char* bias; };
  auto chunk_of = [&](int k) -> Chunk {
    if (k < 2 * L) {
      const int l = (k >> 1) + 1;
      const char* img = a.wimg + a.fwd_off[l];
      return Chunk{img + (k & 1) * W::HALF, W::HALF / 1024, (k & 1) ? nullptr : img + G::IMG_HID};
    }
    if (k == 2 * L) return Chunk{a.wimg + a.fwd_off[L + 1], (G::IMG_HF + G::BIAS_HEAD + 1023) / 1024, nullptr};  // (bias behind the image)
    if (k == 2 * L + 1) return Chunk{a.wimg + a.bwd_off[L + 1], G::IMG_HB / 1024, nullptr};
    const int m = k - (2 * L + 2), l = L - (m >> 1);
    return Chunk{a.wimg + a.bwd_off[l] + (m & 1) * W::HALF, W::HALF / 1024, nullptr};
  };
  int kpar = 0;  // buffer of the tile's chunk 0 (chunk k sits in buffer (k ^ kpar) & 1: the parity runs on across tiles when nch is odd)
  auto dma_chunk = [&](int k, int par) {
    const Chunk c = chunk_of(k);
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_u32(smem + ((k ^ par) & 1) * W::HALF));
    for (int piece = wave; piece < c.pieces; piece += W::NWAVE) glds16(c.src + piece * 1024, lane16, dst + (unsigned)piece * 1024);
    if (c.bias != nullptr && wave == 0) glds16(c.bias, lane16, lds_u32(BIAS + ((k >> 1) & 1) * W::BIAS_B));
  };

  const int* const tlist = a.tlist;
  const int n_walk = tlist != nullptr ? __builtin_amdgcn_readfirstlane(*a.tcount) : a.n_tiles;
  const int n_pairs = (n_walk + W::NT - 1) / W::NT;
  if ((int)blockIdx.x >= n_pairs) return;
  // FiLM tables [group][layer 1..L][2][H] floats behind the bias slots (W::FT_LMAX layers fit: launch side checks L)
  float* const ftab_base = (float*)(BIAS + 2 * W::BIAS_B + (MODE == 0 ? 0 : W::NWAVE * W::XT_BYTES));
  constexpr int FT_STRIDE = (MODE == 0 ? W::FT_LMAX : W::FT_LMAX2) * 2 * H;   // floats per tile group
  int ft_img0 = -1, ft_img1 = -1;  // images whose tables are staged for group 0 / group 1
  dma_chunk(0, kpar);
  const float inv3p = 1.0f / (3.0f * (float)a.P);

#pragma unroll 1
  for (int it = (int)blockIdx.x; it < n_pairs; it += (int)gridDim.x) {
    const bool last_tile = it + (int)gridDim.x >= n_pairs;
    const int it2 = it * W::NT + grp;
    const bool active = it2 < n_walk;                       // (the idle group of an odd count's last pair recomputes its neighbour's tile)
    const int itw = active ? it2 : it * W::NT;
    const int tile = tlist != nullptr ? __builtin_amdgcn_readfirstlane(tlist[itw]) : itw;
    const int b = tile / a.tiles_per_image;
    if constexpr (FILM) {
      // the tables of the images this pair works on (wave-uniform decision from both groups' tiles: every wave takes both barriers)
      const int w0 = it * W::NT, w1 = (it * W::NT + 1 < n_walk) ? it * W::NT + 1 : it * W::NT;
      const int i0 = (tlist != nullptr ? __builtin_amdgcn_readfirstlane(tlist[w0]) : w0) / a.tiles_per_image;
      const int i1 = (tlist != nullptr ? __builtin_amdgcn_readfirstlane(tlist[w1]) : w1) / a.tiles_per_image;
      if (MODE != 0 || i0 != ft_img0 || (W::NT == 2 && i1 != ft_img1)) {  // (training form: every pair -- the region was the last tile's dA exchange)
        __syncthreads();  // nobody reads the old tables (or the dA exchange) any more
        int t0 = tid;  // (opaque here: the copy loops' addresses are otherwise formed outside the tile loop and kept -- spilled -- for it)
        asm volatile("" : "+v"(t0));
#pragma unroll 1
        for (int g2 = 0; g2 < W::NT; ++g2) {
          const float* src = a.film + (size_t)(g2 == 0 ? i0 : i1) * L * 2 * H;
          float* dst = ftab_base + g2 * FT_STRIDE;
#pragma unroll 1
          for (int i = t0; i < L * 2 * H; i += 64 * W::NWAVE)   // [freq | phase / 2 pi] per layer (the forward images carry the 1 / 2 pi of freq)
            dst[i] = src[i] * (((i / H) & 1) ? 0.15915494309189535f : 1.f);
        }
        __syncthreads();
        ft_img0 = i0; ft_img1 = i1;
      }
    }
    const float* const ftab = FILM ? ftab_base + grp * FT_STRIDE : nullptr;
    // [layer][16 chunks][256 threads][16 B]; the training form leaves every tile's in place for k_dw_frag (the frozen / forward forms: a
    // slot per workgroup and group -- make_layout sizes stash_per_wg for two)
    char* const stash = MODE == 2 ? a.stash + (size_t)tile * a.stash_per_wg
                                  : a.stash + (size_t)blockIdx.x * a.stash_per_wg + (size_t)grp * (size_t)(L + 1) * G::STASH_LAYER_BYTES;
    int p = (tile - b * a.tiles_per_image) * 128 + wq * 32 + j;
    // (RENI_WEIGHT_COMPACT: `p` is a POSITION among the image's pixels with weight; the pixel comes from MainArgs::plist)
    if (a.plist != nullptr) p = p < __builtin_amdgcn_readfirstlane(a.nlive[b]) ? a.plist[(size_t)b * a.P + p] : a.P;
    // (`valid` / `owner` gate what is READ: the idle group of an odd count's last pair reads its neighbour's inputs and so forms its
    //  neighbour's values bit for bit -- the FiLM training form's stream stores are unconditional and land on the neighbour's slot.
    //  Round 6's first version cleared `valid` for the idle group: zeros raced with the neighbour's words -- tests/test_gpu_fuzz.py at 600
    //  cases, H = 256 FiLM B = 3 P = 127.  What is WRITTEN elsewhere is gated by `active`.)
    const bool valid = p < a.P, owner = valid && hi == 0;
    // (opaque per tile: hipcc otherwise forms the per-lane 64-bit stash / stream addresses once, outside the tile loop, and spills them)
    unsigned tl16 = (unsigned)tl * 16, l16 = lane16;
    asm volatile("" : "+v"(tl16), "+v"(l16));
    // ---- x = (dx, dy, dz, r, 1) as bf16 hi + lo parts: layer 0's B operand (and, transposed, the last step's A operand)
    bf16x8 bop0;
    {
      const float* dp = a.D + (size_t)b * a.d_bstride + (size_t)(valid ? p : 0) * 3;
      const float x0 = dp[0], x1 = dp[1], x2 = dp[2];
      const float x3 = sqrtf(x0 * x0 + x2 * x2);
      const unsigned h01 = pk(x0, x1), h23 = pk(x2, x3);
      const float l0 = x0 - __builtin_bit_cast(float, h01 << 16), l1 = x1 - __builtin_bit_cast(float, h01 & 0xffff0000u);
      const float l2 = x2 - __builtin_bit_cast(float, h23 << 16), l3 = x3 - __builtin_bit_cast(float, h23 & 0xffff0000u);
      const unsigned q01 = pk(l0, l1), q23 = pk(l2, l3);
      constexpr unsigned ONE = 0x3f80u;
      const u32x4 first = {h01, h23, ONE | (h01 << 16), (h01 >> 16) | (h23 << 16)};
      const u32x4 second = {(h23 >> 16) | (ONE << 16), q01, q23, 0u};
      bop0 = __builtin_bit_cast(bf16x8, hi == 0 ? first : second);
      if constexpr (MODE >= 1) {  // (x_hi | 1 | x_lo) component-major for dA's B operand (rows 0..4, 5..8), this wave's private region
        typedef __attribute__((address_space(3))) unsigned short* lh;
        const unsigned xw = lds_u32(xt) + (unsigned)(j * 2);
        if (hi == 0) {
          *(lh)(uintptr_t)(xw + 0 * W::XT_ROW) = (unsigned short)h01;
          *(lh)(uintptr_t)(xw + 1 * W::XT_ROW) = (unsigned short)(h01 >> 16);
          *(lh)(uintptr_t)(xw + 2 * W::XT_ROW) = (unsigned short)h23;
          *(lh)(uintptr_t)(xw + 3 * W::XT_ROW) = (unsigned short)(h23 >> 16);
          *(lh)(uintptr_t)(xw + 4 * W::XT_ROW) = (unsigned short)ONE;
        } else {
          *(lh)(uintptr_t)(xw + 5 * W::XT_ROW) = (unsigned short)q01;
          *(lh)(uintptr_t)(xw + 6 * W::XT_ROW) = (unsigned short)(q01 >> 16);
          *(lh)(uintptr_t)(xw + 7 * W::XT_ROW) = (unsigned short)q23;
          *(lh)(uintptr_t)(xw + 8 * W::XT_ROW) = (unsigned short)(q23 >> 16);
        }
      }
    }
    float tgt[3] = {0.f, 0.f, 0.f}, swt[3] = {0.f, 0.f, 0.f};
    if (owner && a.target != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        tgt[c] = a.target[(size_t)b * a.ts0 + (size_t)p * a.ts1 + (size_t)c * a.ts2];
        if (a.weight != nullptr) swt[c] = a.weight[(size_t)b * a.ws0 + (size_t)p * a.ws1 + (size_t)c * a.ws2];
      }
    }
    // ---- layer 0: theta_0 = A_b . x (split-bf16 operands, omega_0 / 2 pi folded into afrag), h_0 = sin
    u32x4 hb[NKS];  // the current activations / gradients as packed B operands
    {
      const char* af = a.afrag + (size_t)b * (NRB * 1024) + l16;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const bf16x8 aop = *(const bf16x8*)(af + rb * 1024);
        f32x16 th;
#pragma unroll
        for (int r = 0; r < 16; ++r) th[r] = 0.f;
        th = PolBF16::mfma(aop, bop0, th);
        PolBF16::drain();
        if constexpr (FILM) {  // (FiLM angles reach tens of revolutions: reduced before the sine and -- training form -- the fp16 stash)
#pragma unroll
          for (int r = 0; r < 16; ++r) th[r] = __builtin_amdgcn_fractf(th[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; r += 2)
          hb[2 * rb + (r >> 3)][(r & 7) >> 1] = pk(__builtin_amdgcn_sinf(th[r]), __builtin_amdgcn_sinf(th[r + 1]));
        if constexpr (MODE == 2) {  // layer 0's phases: h_0 of dW_1 = g_1 h_0^T (k_dw_frag)
          u32x4 ph[2];
#pragma unroll
          for (int r = 0; r < 16; r += 2) ph[r >> 3][(r & 7) >> 1] = phase_pack(th[r], th[r + 1]);
          if (active) {
            *(u32x4*)(stash + (size_t)tl16 + (size_t)(2 * rb) * 4096) = ph[0];
            *(u32x4*)(stash + (size_t)tl16 + (size_t)(2 * rb + 1) * 4096) = ph[1];
          }
        }
      }
    }
    // one half layer: out rows 32 (4 h + i) .. = image-half[i][ks] . bin[ks] (+ bias); A fragments requested ahead between fences
    auto gemm_half = [&](const char* buf, const u32x4 (&bin)[NKS], f32x16 (&acc)[4]) {
      constexpr int N = 4 * NKS, PF = FILM ? 3 : 6;  // (FiLM: the activation's table quads need the registers of three fragments)
      auto fa = [&](int i) { return *(const bf16x8*)(buf + (((i & 3) * NKS + (i >> 2)) * 64 + lane) * 16); };  // (k-step outer: four chains)
      bf16x8 q[PF];
#pragma unroll
      for (int d = 0; d < PF; ++d) q[d] = fa(d);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const bf16x8 av = q[i % PF];
        if (i + PF < N) q[i % PF] = fa(i + PF);
        __builtin_amdgcn_sched_barrier(0);
        acc[i & 3] = PolBF16::mfma(av, __builtin_bit_cast(bf16x8, bin[i >> 2]), acc[i & 3]);
        __builtin_amdgcn_sched_barrier(0);
      }
      // (every MFMA chain of this kernel ends with its own pad: the epilogues read the accumulators from asm statements hipcc's hazard
      // recogniser does not look into, and its padding behind a block-ending MFMA is one state short by tests/isa_audit.py's strict count)
      PolBF16::drain();
    };
    int k = 0;  // chunk of the tile
    auto chunk_begin = [&]() -> const char* {
      dma_wait();        // this chunk (requested a chunk ago) and everything else this wave has in flight
      __syncthreads();   // every wave's pieces are there; every wave is done with the other buffer
      if (k + 1 < nch) dma_chunk(k + 1, kpar);
      else if (!last_tile) dma_chunk(0, kpar ^ (nch & 1));  // the next tile's first chunk
      const char* buf = smem + ((k ^ kpar) & 1) * W::HALF;
      ++k;
      return buf;
    };

    // ---- hidden layers, forward
#pragma unroll 1
    for (int l = 1; l <= L; ++l) {
      u32x4 hn[NKS];
      char* const sl = stash + (size_t)l * G::STASH_LAYER_BYTES + (size_t)tl16;
      // (FiLM: this layer's table slot + the lane's 4 hi, through an opaque offset -- formed here, not hoisted out of the tile loop)
      unsigned ft_off = FILM ? (unsigned)((l - 1) * 2 * H + 4 * hi) : 0u;
      if constexpr (FILM) asm volatile("" : "+v"(ft_off));
      const float* const ftl = FILM ? ftab + ft_off : nullptr;
      f32x4 fq4 = {0.f, 0.f, 0.f, 0.f}, ph4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const char* buf = chunk_begin();
        const float* bl = (const float*)(BIAS + ((l - 1) & 1) * W::BIAS_B);  // (fetched with the layer's first half: dma_chunk)
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][r] = bl[32 * (4 * h + i) + rowmap(r, hi)];
        gemm_half(buf, hb, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rb = 4 * h + i;
          u32x4 ph[2];
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            float t0 = acc[i][r], t1 = acc[i][r + 1];
            if constexpr (FILM) {  // angle = freq . (W h + b) + phase, in revolutions, reduced (rowmap: registers 4 m .. 4 m + 3 = four consecutive features)
              if ((r & 3) == 0) {  // (one quad of each table per four registers: two ds_read_b128)
                const float* tp = ftl + 32 * rb + 8 * (r >> 2);
                fq4 = *(const f32x4*)tp;
                ph4 = *(const f32x4*)(tp + H);
              }
              t0 = __builtin_amdgcn_fractf(__builtin_fmaf(t0, fq4[r & 3], ph4[r & 3]));
              t1 = __builtin_amdgcn_fractf(__builtin_fmaf(t1, fq4[(r & 3) + 1], ph4[(r & 3) + 1]));
            }
            hn[2 * rb + (r >> 3)][(r & 7) >> 1] = pk(__builtin_amdgcn_sinf(t0), __builtin_amdgcn_sinf(t1));
            ph[r >> 3][(r & 7) >> 1] = phase_pack(t0, t1);
          }
          if constexpr (MODE >= 1) {
            if (MODE == 1 || active) {
              *(u32x4*)(sl + (size_t)(2 * rb) * 4096) = ph[0];
              *(u32x4*)(sl + (size_t)(2 * rb + 1) * 4096) = ph[1];
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NKS; ++c) hb[c] = hn[c];
    }
    // ---- head (one row block, its bias behind the image in the buffer)
    float ylin[3], outv[3];
    {
      const char* buf = chunk_begin();
      const float* bias = (const float*)(buf + G::IMG_HF);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bias[rowmap(r, hi)];
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        acc = PolBF16::mfma(*(const bf16x8*)(buf + (ks * 64 + lane) * 16), __builtin_bit_cast(bf16x8, hb[ks]), acc);
      PolBF16::drain();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ylin[c] = acc[c];
        const float yv = a.last_linear ? ylin[c] : sin_f32(a.w_hidden * ylin[c]);
        const float y2 = yv * 2.885390081777927f;
        const float e2 = __builtin_amdgcn_exp2f(y2 > 60.f ? 60.f : y2);  // (compare-and-select: a NaN stays a NaN)
        outv[c] = (a.act == 1) ? (1.f - 2.f * __builtin_amdgcn_rcpf(e2 + 1.f)) : (a.act == 2) ? expf(yv) : yv;
      }
    }
    if (a.out != nullptr && owner && active) {
      float* op = a.out + ((size_t)b * a.P + p) * 3;
      op[0] = outv[0]; op[1] = outv[1]; op[2] = outv[2];
    }
    if constexpr (MODE == 0) {
      if (a.target != nullptr) {  // the statistics pass of RENITestLoss's cosine term: nine sums per tile and wave
        float s9[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = owner ? tgt[c] : 0.f, o = owner ? outv[c] : 0.f;
          s9[c] = o * t; s9[3 + c] = o * o; s9[6 + c] = t * t;
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const float sq = wave_sum(s9[q]);
          if (lane == 0 && active) a.loss_part[((size_t)tile * 4 + wq) * 16 + 1 + q] = sq;
        }
      }
      kpar ^= (nch & 1);
      continue;
    } else {
      // ---- loss and d loss / d out
      float gy[3] = {0.f, 0.f, 0.f};
      {
        float e = 0.f;
        if (a.loss_kind == 2) {
#pragma unroll
          for (int c = 0; c < 3; ++c) gy[c] = owner ? a.dout[((size_t)b * a.P + p) * 3 + c] : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (owner) {
              const float t = tgt[c], sw = swt[c], d = outv[c] - t;
              e += sw * d * d;
              gy[c] = 2.f * sw * d * inv3p;
              if (a.loss_kind == 1) gy[c] += a.stats[(size_t)b * 16 + c] * t - a.stats[(size_t)b * 16 + 4 + c] * outv[c];
            }
          }
        }
        const float es = wave_sum(e);
        if (lane == 0 && active) a.loss_part[((size_t)tile * 4 + wq) * 16] = es;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (a.act == 1) gy[c] *= (1.f - outv[c] * outv[c]);
          else if (a.act == 2) gy[c] *= outv[c];
          if (!a.last_linear) gy[c] *= a.w_hidden * cos_f32(a.w_hidden * ylin[c]);
          if (!owner) gy[c] = 0.f;
          gy[c] *= a.gy_scale;  // (the W^T images are 8 x the forward images: MainArgs::gy_scale)
        }
      }
      // (training form) g_l as held: slot l - 1 of the fragment stream; g_y behind the stream
      auto store_g = [&](int l, const u32x4 (&g)[NKS]) {
        char* const gp = a.gfs + ((size_t)(l - 1) * a.n_tiles + tile) * (size_t)G::STASH_LAYER_BYTES + (size_t)tl16;
        if (active) {
#pragma unroll
          for (int c = 0; c < NKS; ++c) {
            __builtin_nontemporal_store(g[c], (u32x4*)(gp + (size_t)c * 4096));
          }
        }
      };
      if constexpr (MODE == 2) {
        if (hi == 0 && active)
          __builtin_nontemporal_store(f32x4{gy[0], gy[1], gy[2], 0.f}, (f32x4*)(a.gfs + (size_t)L * a.n_tiles * (size_t)G::STASH_LAYER_BYTES + ((size_t)tile * 128 + ((tl16 >> 10) * 32 + ((tl16 >> 4) & 31))) * 16));  // (sample = 32 wq + j, from the opaque offset)
      }
      // phases of layer `l`, row blocks 4 h .. 4 h + 3 (eight 16-byte words per lane), requested at the top of the half that uses them
      // (per QUARTER: row blocks 2 qt, 2 qt + 1 -- four words)
      auto load_ph = [&](int l, int qt, u32x4 (&w)[4]) {
        const char* sl = stash + (size_t)l * G::STASH_LAYER_BYTES + (size_t)tl16 + (size_t)(4 * qt) * 4096;
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = *(const u32x4*)(sl + (size_t)c * 4096);
      };
      // one quarter layer of the backward pass: out rows 32 (4 h + 2 q2 + i), i = 0, 1, of the half in `buf` -- two accumulator chains
      auto gemm_quarter = [&](const char* buf, int q2, const u32x4 (&bin)[NKS], f32x16 (&acc)[2]) {
        constexpr int N = 2 * NKS, PF = FILM ? 3 : 6;  // (FiLM: the epilogue's table quad and stream words need the registers of three fragments)
        auto fa = [&](int i) { return *(const bf16x8*)(buf + (((2 * q2 + (i & 1)) * NKS + (i >> 1)) * 64 + lane) * 16); };
        bf16x8 q[PF];
#pragma unroll
        for (int d = 0; d < PF; ++d) q[d] = fa(d);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const bf16x8 av = q[i % PF];
          if (i + PF < N) q[i % PF] = fa(i + PF);
          __builtin_amdgcn_sched_barrier(0);
          acc[i & 1] = PolBF16::mfma(av, __builtin_bit_cast(bf16x8, bin[i >> 1]), acc[i & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        PolBF16::drain();
      };
      // g_prev[rb] = acc (.) cos(phase), packed (omega of the layer below rides on the W^T image)
      // (FiLM: tq = the layer's frequency row + 32 rb + 4 hi; one table quad per four registers.  The chain goes on with
      //  g_a = freq . g_theta, g_theta = cos(theta) . g_h; the fragment stream takes g_THETA -- as the generic chain's does: k_dw_frag's
      //  per-image sums M = g_theta h^T give d(phase), d(freq) and, times freq, the weight gradient -- so the two words of the row
      //  block leave from here (gst = the row block's first chunk of the layer's stream slot), not from the packed g_a afterwards)
      auto epilogue = [&](const f32x16& acc, const u32x4& w0, const u32x4& w1, u32x4& o0, u32x4& o1, const float* tq = nullptr,
                          unsigned long long gst = 0ull, int gofs = 0) {
        f32x4 fq4 = {1.f, 1.f, 1.f, 1.f};
        unsigned sprev = 0u;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const unsigned w = (r < 8 ? w0 : w1)[(r & 7) >> 1];
          float r0, r1;
          cos_mul2(w, acc[r], acc[r + 1], r0, r1);
          if constexpr (FILM) {
            // (the W^T image carries 2 pi for the chain's g_a = (freq / 2 pi) . (2 pi W^T g): the stream's g_theta is the plain one)
            // (in 8-byte pieces as they are made: two live words, not eight -- the instance is at its register limit.  The W^T images
            //  of this instance are plain and the table's frequency row is the plain frequency: g_theta needs no rescaling)
            const unsigned sw = pk(r0, r1);
            if ((r & 3) == 0) sprev = sw;
            else {  // (unconditional: the idle group of an odd count's last pair recomputes its neighbour's tile from the same inputs --
                    //  `valid` above -- and writes the SAME words to the same slot; a branch per store here cost the instance 420 B of scratch)
              // (scalar base + 32-bit lane offset, the offset formed HERE from the per-tile opaque tl16: left to hipcc the eight 64-bit
              //  per-lane addresses of a layer's row blocks are formed ahead of the GEMMs and spilled)
              unsigned off = tl16;
              asm volatile("" : "+v"(off));
              off += (unsigned)(gofs + (r >> 3) * 4096 + ((r & 7) >> 2) * 8);
              typedef __attribute__((address_space(1))) u32x2 gu32x2;
              __builtin_nontemporal_store(u32x2{sprev, sw}, (gu32x2*)((__attribute__((address_space(1))) char*)gst + off));
            }
            if ((r & 3) == 0) fq4 = *(const f32x4*)(tq + 8 * (r >> 2));
            r0 *= fq4[r & 3]; r1 *= fq4[(r & 3) + 1];
          }
          (r < 8 ? o0 : o1)[(r & 7) >> 1] = pk(r0, r1);
        }
      };
      // (FiLM) the stream slot of g_l for this tile, as a wave-uniform base (row block rb's chunks 2 rb, 2 rb + 1: + 8192 rb)
      auto gslot = [&](int l) -> unsigned long long {
        if constexpr (!FILM) return 0ull;
        unsigned long long base = (unsigned long long)(a.gfs + ((size_t)(l - 1) * a.n_tiles + tile) * (size_t)G::STASH_LAYER_BYTES);
        base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);  // (wave-uniform by construction: `tile` is)
        asm volatile("" : "+s"(base));
        return base;
      };
      // frequency row of hidden layer `layer` (1..L) for row block rb, this lane's half (FiLM; nullptr otherwise)
      auto freq_row = [&](int layer, int rb) -> const float* {
        if constexpr (!FILM) return nullptr;
        unsigned off = (unsigned)((layer - 1) * 2 * H + 32 * rb + 4 * hi);
        asm volatile("" : "+v"(off));  // (formed here: see the forward pass's ft_off)
        return ftab + off;
      };
      // ---- head backward: g_L = (W_out^T g_y) (.) cos(phase_L)
      u32x4 gb[NKS];
      {
        u32x4 wph[4];
        const char* buf = chunk_begin();
        u32x4 gyw = {pk(gy[0], gy[1]), pk(gy[2], 0.f), 0u, 0u};
        if (hi != 0) gyw = u32x4{0u, 0u, 0u, 0u};  // (k-slots 8..15 of the one k-step: zero)
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
          load_ph(L, qt, wph);
          f32x16 acc[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
            acc[i] = PolBF16::mfma(*(const bf16x8*)(buf + ((2 * qt + i) * 64 + lane) * 16), __builtin_bit_cast(bf16x8, gyw), acc[i]);
          }
          PolBF16::drain();
#pragma unroll
          for (int i = 0; i < 2; ++i) epilogue(acc[i], wph[2 * i], wph[2 * i + 1], gb[2 * (2 * qt + i)], gb[2 * (2 * qt + i) + 1], freq_row(L, 2 * qt + i), gslot(L), 8192 * (2 * qt + i));
        }
      }
      if constexpr (MODE == 2 && !FILM) store_g(L, gb);
      // ---- hidden layers l = L .. 2: g_{l-1} = (W_l^T g_l) (.) cos(phase_{l-1})
#pragma unroll 1
      for (int l = L; l >= 2; --l) {
        u32x4 gn[NKS];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const char* buf = chunk_begin();
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            u32x4 wph[4];
            load_ph(l - 1, 2 * h + q2, wph);
            f32x16 acc[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
            gemm_quarter(buf, q2, gb, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int rb = 4 * h + 2 * q2 + i;
              epilogue(acc[i], wph[2 * i], wph[2 * i + 1], gn[2 * rb], gn[2 * rb + 1], freq_row(l - 1, rb), gslot(l - 1), 8192 * rb);
            }
          }
        }
#pragma unroll
        for (int c = 0; c < NKS; ++c) gb[c] = gn[c];
        if constexpr (MODE == 2 && !FILM) store_g(l - 1, gb);
      }
      // ---- layer 1's dX and layer 0's backward, TRANSPOSED: feature block fb of g_0^T = (g_1^T W_1)[., fb] (.) cos(theta_0^T[., fb]);
      // dA[32 fb + ., component] = g_0 X^T for this tile, to the per-tile partial (columns 0..4 = (x_hi | 1), 8..11 = x_lo: hi + lo kept)
      {
        typedef __attribute__((address_space(3))) unsigned long long* lq;
        const int xrow = (lane & 15) < 5 ? (lane & 15) : ((lane & 15) >= 8 && (lane & 15) < 12) ? (lane & 15) - 3 : 0;
        const unsigned xr = lds_u32(xt) + (unsigned)(xrow * W::XT_ROW + 8 * hi);
        float* const dA_t = a.dA_part + (size_t)tile * H * 8;
        float* const das = (float*)(BIAS + 2 * W::BIAS_B + W::NWAVE * W::XT_BYTES);
        // (FiLM: the tables alias this region; their last readers -- the epilogue that made g_1 -- lie behind the chunk_begin barrier
        //  of the first half below in every wave, and the first write to `das` comes behind that half's GEMMs)
        const char* af = a.afrag + (size_t)b * (NRB * 1024) + l16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const char* buf = chunk_begin();
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
          for (int i2 = 0; i2 < 2; ++i2) {
            const int i = 2 * q2 + i2;
            const int fb = 4 * h + i;
            const bf16x8 aop = *(const bf16x8*)(af + fb * 1024);
            f32x16 dx, th;
#pragma unroll
            for (int r = 0; r < 16; ++r) { dx[r] = 0.f; th[r] = 0.f; }
            th = PolBF16::mfma(bop0, aop, th);  // theta_0^T: the operands of layer 0, swapped
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
              dx = PolBF16::mfma(__builtin_bit_cast(bf16x8, gb[ks]), *(const bf16x8*)(buf + ((i * NKS + ks) * 64 + lane) * 16), dx);
            PolBF16::drain();
            u32x4 gA[2];
#pragma unroll
            for (int r = 0; r < 16; r += 2)
              gA[r >> 3][(r & 7) >> 1] = pk(dx[r] * __builtin_amdgcn_cosf(th[r]), dx[r + 1] * __builtin_amdgcn_cosf(th[r + 1]));
            f32x16 accA;
#pragma unroll
            for (int r = 0; r < 16; ++r) accA[r] = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const unsigned long long q0 = *(lq)(uintptr_t)(xr + (unsigned)(t * 32));
              const unsigned long long q1 = *(lq)(uintptr_t)(xr + (unsigned)(t * 32 + 16));
              typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
              const u64x2 qq = {q0, q1};
              accA = PolBF16::mfma(__builtin_bit_cast(bf16x8, gA[t]), __builtin_bit_cast(bf16x8, qq), accA);
            }
            PolBF16::drain();
            // this WAVE's 32 samples' share of the block: to LDS [block i2][wave][row-in-block][8] (hi + lo parts summed)
            float* const ds = das + ((i2 * W::NWAVE + wave) * 32) * 8;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float lo = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, accA[r]), 0x108, 0xf, 0xf, true));
              if (j < 8) ds[rowmap(r, hi) * 8 + j] = accA[r] + ((j < 4) ? lo : 0.f);
            }
          }
          // the tile's dA of these two feature blocks = its four waves' shares in a fixed order: thread tl of the tile's 256 sums two
          // floats of block tl >> 7.  (Two barriers per quarter: the scratch is rewritten by the next quarter)
          __syncthreads();
          {
            const int blk = (int)(tl16 >> 11), e = (int)((tl16 >> 4) & 127) * 2;   // (tl >> 7, (tl & 127) * 2 -- from the opaque offset)
            const float* const d0 = das + ((blk * W::NWAVE + grp * 4) * 256) + e;   // [block][wave][256 floats]
            const f32x2 s0 = *(const f32x2*)d0, s1 = *(const f32x2*)(d0 + 256), s2 = *(const f32x2*)(d0 + 512), s3 = *(const f32x2*)(d0 + 768);
            const f32x2 tot = (s0 + s1) + (s2 + s3);
            if (active) *(f32x2*)(dA_t + (size_t)(32 * (4 * h + 2 * q2 + blk)) * 8 + e) = tot;
          }
          __syncthreads();
          }
        }
      }
      kpar ^= (nch & 1);
    }
  }
}
template __global__ void k_reni_wide256<0>(const MainArgs);
template __global__ void k_reni_wide256<1>(const MainArgs);
template __global__ void k_reni_wide256<2>(const MainArgs);
template __global__ void k_reni_wide256<0, true>(const MainArgs);
template __global__ void k_reni_wide256<2, true>(const MainArgs);

// dW_out / db_out of the training form: per workgroup a contiguous range of tiles, [3][256] + [3] into the workgroup's slot of the
// weight-gradient partials (MainArgs::dwp: what k_reni_main's in-kernel head phase writes on the generic path; the reduction over
// workgroups is the same launch).  dW_out[c][f] = sum_s g_y[s][c] sin(2 pi phase_L[f][s]): 512 threads, quarter q = tid >> 7 takes
// chunks 4 q .. 4 q + 3 of a record (row blocks 2 q, 2 q + 1), each thread the 32 phases of ITS sample's fragment words -- 32 sines and
// 96 multiply-adds per record; the sums over the 32 samples of a half wave and over the two waves of a quarter happen once, at the end.
// (Two waves per SIMD at ~150 registers: with 256 threads holding 64 phases each the kernel sat on its load latency, 124 us per chunk.)
__global__ void __launch_bounds__(512, 1) k_wide_head_dw(const MainArgs a) {
  using G = Geo<PolBF16, 256>;
  constexpr int H = 256;
  __shared__ float sm[2][3][H];
  __shared__ float smb[2][4];
  const int tid = threadIdx.x;
  const int quarter = tid >> 7, pt = tid & 127, pw = pt >> 6, phi = (pt & 63) >> 5, pj = pt & 31;
  const int t0 = (int)((long long)blockIdx.x * a.n_tiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * a.n_tiles / gridDim.x);
  const char* const gys = a.gfs + (size_t)a.L * a.n_tiles * (size_t)G::STASH_LAYER_BYTES;
  float acc[4][8][3];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[q][e][0] = acc[q][e][1] = acc[q][e][2] = 0.f;
  float dbv[3] = {0.f, 0.f, 0.f};
  u32x4 raw[4];
  f32x4 gy;
  auto load = [&](int rec) __attribute__((always_inline)) {
    const int tile = rec >> 1, round = rec & 1;
    const char* src = a.stash + (size_t)tile * a.stash_per_wg + (size_t)a.L * G::STASH_LAYER_BYTES + (size_t)(4 * quarter) * 4096 + (size_t)(round * 128 + pt) * 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = *(const u32x4*)(src + (size_t)q * 4096);
    gy = *(const f32x4*)(gys + ((size_t)tile * 128 + (2 * round + pw) * 32 + pj) * 16);
  };
  if (t0 < t1) load(2 * t0);
#pragma unroll 1
  for (int rec = 2 * t0; rec < 2 * t1; ++rec) {
    u32x4 w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = raw[q];
    const f32x4 g = gy;
    if (rec + 1 < 2 * t1) load(rec + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float s0 = __builtin_amdgcn_sinf(phase_lo(w[q][d])), s1 = __builtin_amdgcn_sinf(phase_hi(w[q][d]));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc[q][2 * d][c] = __builtin_fmaf(g[c], s0, acc[q][2 * d][c]);
          acc[q][2 * d + 1][c] = __builtin_fmaf(g[c], s1, acc[q][2 * d + 1][c]);
        }
      }
    if (quarter == 0 && phi == 0) { dbv[0] += g[0]; dbv[1] += g[1]; dbv[2] += g[2]; }
  }
  // chunk Q = 4 quarter + q = (row block Q >> 1, register half Q & 1); word d, half-word e -> accumulator row 8 (Q & 1) + 2 d + e
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int Q = 4 * quarter + q;
      const int f = 32 * (Q >> 1) + rowmap(8 * (Q & 1) + e, phi);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t = half_sum(acc[q][e][c]);
        if (pj == 0) sm[pw][c][f] = t;
      }
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = half_sum(dbv[c]);
    if (quarter == 0 && phi == 0 && pj == 0) smb[pw][c] = t;
  }
  __syncthreads();
  float* const dwp = a.dwp + (size_t)blockIdx.x * a.dwp_per_wg;
  float* const dw = dwp + a.p_off_w[a.L + 1];
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dw[c * H + tid] = sm[0][c][tid] + sm[1][c][tid];
  }
  if (tid < 3) dwp[a.p_off_b[a.L + 1] + tid] = smb[0][tid] + smb[1][tid];
}

hipError_t launch_wide_head_dw(const MainArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_wide_head_dw, dim3(grid), dim3(512), 0, s, a);
  return hipGetLastError();
}


// which: 0 forward / statistics, 1 frozen-decoder forward + loss + backward, 2 the training form (fragment stream for k_dw_frag)
// (which == 3: the FiLM forward / statistics instance, 4: the FiLM training form)
int wide256_film_max_layers() { return Wide256::FT_LMAX; }
int wide256_film_train_max_layers() { return Wide256::FT_LMAX2; }
hipError_t launch_wide256(int which, const MainArgs& a, int grid, hipStream_t s) {
  void (*fn)(const MainArgs) = which == 0 ? k_reni_wide256<0> : which == 1 ? k_reni_wide256<1> : which == 2 ? k_reni_wide256<2>
                               : which == 3 ? k_reni_wide256<0, true> : k_reni_wide256<2, true>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, Wide256::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * Wide256::NWAVE), Wide256::LDS_BYTES, s, a);
  return hipGetLastError();
}
