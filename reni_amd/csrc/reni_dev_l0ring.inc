// reni_dev_l0ring.inc -- k_reni_l0_ring: layer 0's backward AND dW_1 from the g_1 stream (concat decoder, bf16, H = 128)
// Part of reni_device.inc (RENI_TU_CORE only; inside namespace reni; never compiled on its own).
//
// Round 5.  The L0X form of the training kernel (k_reni_train_bf16<.., SPEC, L0X>) ends a tile with the step of layer 2 and streams
// g_1 = d loss / d (pre-activation of layer 1) out (bf16, 256 B per sample).  This kernel walks the same contiguous tile ranges
// (backwards: the most recently written -- still cached -- tiles first) and does everything that is left of the backward pass:
//     dW_1 += g_1 h_0^T                                  (reference autograd of src/models/RENI.py:86-87 for net[1])
//     g_0   = (W_1^T g_1) (.) omega_0 cos(theta_0)       (the SineLayer derivative of the first layer, RENI.py:86-87)
//     dA_b += g_0 (x_hi | 1 | x_lo)^T                    (gradient of the per-image affine map A_b, DESIGN.md section 2)
// It replaces k_reni_dw1_ring (dW_1 only: producer / consumer / loader roles around a transposition image of h_0) on that path.
//
// The trick that makes one wave do all of it without any transposition image: compute layer 0 and layer 1's dX TRANSPOSED.
//   * theta_0^T [sample][feature] = X [sample][16] . A_b^T [16][feature]: the MFMA's A operand is the hi/lo-split direction operand
//     of the forward pass (lane = sample), its B operand the image's layer-0 operand (k_prep_image's afrag, lane = feature) -- the
//     two fragments have the same (row | column, k) layout, so swapping them transposes the result.  Accumulator: lane = FEATURE,
//     registers = 16 of the block's 32 samples.
//   * sin(theta_0^T), packed to bf16, IS the B operand (K = samples, columns = layer-0 features) of dW_1 += g_1 h_0^T -- no LDS image
//     of h_0 at all (k_reni_dw1_ring: 32 KB written and 64 KB read per tile).  The A operand (rows = layer-1 features, K = samples)
//     comes out of the raw g_1 slot with ds_read_b64_tr_b16, as before, in the accumulator's sample order.
//   * dX_1^T [sample][feature] = g_1^T W_1: A operand = the stored g_1 chunk (a B fragment of g_1 = an A fragment of g_1^T), B
//     operand = the fragment of the packed W_1^T image (k_pack's backward image of layer 1, omega_0 folded in) -- eight fragments
//     per feature block, resident in registers for the whole kernel.  Same accumulator layout as theta_0^T: the epilogue
//     g_0^T = dX_1^T (.) cos(theta_0^T) is register-to-register.
//   * g_0^T packed to bf16 is the A operand (rows = features, K = samples) of dA += g_0 X^T; only its B operand -- (x_hi | 1 | x_lo) with
//     lane = component, eight samples per lane -- needs a transposition: 9 two-byte LDS writes per sample into a private 1 KB
//     region per wave.
// Work split: 8 waves, two per SIMD; wave (v = feature block 0..3, sh = sample half 0..1) handles layer-0 features 32 v .. 32 v + 31 and
// the sample blocks 2 sh, 2 sh + 1 of every tile: 38 MFMAs per wave and tile (2 x [1 theta + 8 dW + 8 dX + 2 dA]).  The two halves'
// partial sums of dA (per image run) and of dW_1 / db_1 (once per launch) are combined through LDS in a fixed order.
// Inputs arrive by LDS-DMA in a ring of NSLOT slots [g_1 32 KB | afrag 4 KB | directions 1.5 KB], NSLOT - 1 tiles ahead; every wave
// issues five DMA instructions per tile (counted by hand: the loop has no compiler-visible vector-memory operation).  One barrier
// per tile.
// g_1 is stored by the training kernel with its 16-byte cells XOR-swizzled (cell ^ 4 hi ^ 8 (chunk & 1)): the b128 operand reads
// and the transposing reads of the raw slot are both free of bank conflicts (k_reni_dw1_ring's A reads were 2-way conflicted: 47 % of
// its LDS-active cycles, profiles/r04_pmc_counters.md).
// Preconditions (launch_dw1 / dw1_ring_ok): P % 128 == 0, 16-byte aligned direction rows, odd L >= 3 (the L0X instance).
#ifndef RENI_L0_NSLOT
#define RENI_L0_NSLOT 4
#endif
struct L0Ring {
  static constexpr int SLOT_G = 8 * 4096, SLOT_A = 4 * 1024, SLOT_D = 1536, SLOT = SLOT_G + SLOT_A + SLOT_D;  // 38400 = 150 x 256 B
  static constexpr int NSLOT = RENI_L0_NSLOT;
  static constexpr int XT_ROW = 136, XT_BYTES = 9 * XT_ROW + 8;  // per wave: (x_hi | 1 | x_lo) component-major, 9 rows of 64 samples x 2 B + 8 B pad
  static constexpr int LDS_BYTES = NSLOT * SLOT + 8 * XT_BYTES;
  static constexpr int VM_PER_TILE = 5;  // LDS-DMA instructions per wave and tile (issue_part)
  static constexpr int THREADS = 512;
};
static_assert(L0Ring::LDS_BYTES <= 160 * 1024, "ring + private regions must fit a CU's LDS");
static_assert(L0Ring::NSLOT * L0Ring::SLOT >= 4 * 64 * 256 + 4 * 256, "the final dW_1 / db_1 exchange uses the slots' area");

template <int H>
__global__ void __launch_bounds__(512, 1) k_reni_l0_ring(const MainArgs a) {
  using R = L0Ring;
  static_assert(H == 128, "ring slot layout");
  constexpr int NRB = 4, NKS = 8;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const unsigned ring = __builtin_amdgcn_readfirstlane(lds_u32(smem));
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int v = wave & 3, sh = wave >> 2;
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  const unsigned lane16 = (unsigned)lane * 16;
  char* const xt = smem + R::NSLOT * R::SLOT + wave * R::XT_BYTES;
#if defined(RENI_TRACE_DW1)
  unsigned long long* const trace_lds = (unsigned long long*)(smem + R::LDS_BYTES);
  int trace_n = 0;
#ifndef RENI_TRACE_WAVE
#define RENI_TRACE_WAVE 0
#endif
  const bool trace_on = a.trace != nullptr && blockIdx.x == 0 && wave == RENI_TRACE_WAVE;
#endif
  TRACE1(100);

  f32x16 accW[NRB];  // dW_1[32 rb + ., 32 v + .] over this wave's sample half
  acc_zero<NRB>(accW);
  f32x16 accA[1];    // dA[32 v + ., component] of the current image run, this wave's sample half
  acc_zero<1>(accA);
  f32x16 accD[1];    // db_1[32 v + .] over this wave's sample half, in every column: row block v of g_1 against a ones operand -- one
  acc_zero<1>(accD); // MFMA per sixteen samples (sixteen v_dot2c -- which share the matrix pipe's dot unit -- per tile before)
  u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  asm volatile("" : "+v"(ones));

  // W_1^T as B operands of dX_1^T: fragment (row block v, k-step c) of the packed backward image of layer 1, resident
  bf16x8 wt[NKS];
  {
    const char* const wimg = a.wimg + a.bwd_off[1];
#pragma unroll
    for (int c = 0; c < NKS; ++c) wt[c] = *(const bf16x8*)(wimg + ((size_t)((v * NKS + c) * 64) + lane) * 16);
    // (consumed here as far as hipcc can tell: its s_waitcnt vmcnt(0) for these loads stands in front of the loop, not inside it --
    // where it would also wait out the ring's LDS-DMA every tile)
#pragma unroll
    for (int c = 0; c < NKS; ++c) asm volatile("" : "+v"(wt[c]));
  }

  const int G_ = a.nwg_main, g_ = (int)blockIdx.x;
  const int t_lo = (int)((long long)g_ * a.n_tiles / G_);
  const int t_hi = (int)((long long)(g_ + 1) * a.n_tiles / G_) - 1;
  const int n = t_hi - t_lo + 1;
  const int b_lo = t_lo / a.tiles_per_image;

  // The walk's coordinates are carried from tile to tile (this kernel is bound by the number of instructions its two waves per SIMD
  // issue -- ~5 cycles apiece whatever their kind: two integer divisions and the 64-bit address products per tile were ~90 scalar
  // instructions of a 485-instruction tile).  Issue side: the tile NSLOT - 1 ahead of the one being computed.
  int is_b = t_hi / a.tiles_per_image, is_tin = t_hi - is_b * a.tiles_per_image;
  const char* is_g = a.g1 + ((size_t)(t_hi - t_lo) * G_ + g_) * (NKS * 4096) + (size_t)wave * 4096;  // (layout: k_reni_train_bf16, L0X)
  const char* is_a = a.afrag + ((size_t)(is_b * NRB + (wave & 3)) * 64) * 16;
  const char* is_d = (const char*)(a.D + (size_t)is_b * a.d_bstride + (size_t)is_tin * 128 * 3) + (wave & 3) * 384;
  const long long is_d_wrap = (long long)a.tiles_per_image * 1536 - (long long)a.d_bstride * 4;
  const size_t is_g_step = (size_t)G_ * (NKS * 4096);
  unsigned is_dst = ring;
  // (in three PARTS, placed between the phases of a tile's compute: all eight waves issuing their five instructions at once, right
  // behind the barrier, met a full vector-memory queue and stalled together -- ~50 us of the kernel's 184 with nothing issuing)
  auto glds16x2 = [](const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst_uniform) : "memory");
  };
  auto issue_part = [&](int part) {  // this wave's share of the next tile of the walk into the next slot: VM_PER_TILE instructions in all
    if (part == 0) { glds16x2(is_g, lane16, is_dst + (unsigned)wave * 4096); return; }
    if (part == 1) { glds16x2(is_g + 2048, lane16, is_dst + (unsigned)wave * 4096 + 2048); return; }
    if (wave < 4) {  // the image's layer-0 operands (k_prep_image's afrag), one row block
      glds16(is_a, lane16, is_dst + R::SLOT_G + (unsigned)wave * 1024);
    } else {         // a quarter of the tile's 128 directions (1536 bytes)
      if (lane < 24) glds16(is_d, lane16, is_dst + R::SLOT_G + R::SLOT_A + (unsigned)(wave - 4) * 384);
    }
    is_g -= is_g_step;
    is_d -= 1536;
    is_dst += R::SLOT;
    if (is_dst == ring + R::NSLOT * R::SLOT) is_dst = ring;
    if (--is_tin < 0) { is_tin = a.tiles_per_image - 1; --is_b; is_a -= NRB * 1024; is_d += is_d_wrap; }
  };
  auto issue = [&]() { issue_part(0); issue_part(1); issue_part(2); };
  // (Measured and REJECTED, round 5: an L2 prefetch of the tile eight positions down the walk -- one plain load per wave and tile into a
  // register nobody reads, counted in the waits: 192 us against 188 without.  The kernel's 175-185 us against 135 us for its compute
  // alone and 113 us for its LDS-DMA alone is not the memory system's latency: profiles/r05_l0ring.md.)
  // per-lane address parts (see the header for the swizzle)
  //   b128 operand of dX_1^T: chunk c, sample block w -> c * 4096 + w * 1024 + (ecell ^ ((c & 1) * 128))
  unsigned ecell = (unsigned)(lane ^ (4 * hi)) * 16;
  //   transposing reads (A operand of dW_1, rows = layer-1 features 32 rb + (lane & 31), K = samples in the accumulator's order:
  //   lane half khi holds samples 16 t + 4 khi + {0..3, 8..11}): lane (khi, gq, u) supplies the address of the 8-byte piece
  //   (sample 16 t + 4 khi + 8 q + (u >> 2), features 32 rb + 16 gq + 4 (u & 3) + 0..3) = chunk 2 rb + gq, thread half hi' = u & 1 ...
  const int khi = lane >> 5, gq = (lane >> 4) & 1, u = lane & 15, pp = u & 3;
  unsigned trl = (unsigned)(gq * 4096 + (32 * (pp & 1) + ((4 * khi + (u >> 2)) ^ (4 * (pp & 1)) ^ (8 * gq))) * 16 + (pp >> 1) * 8);
  unsigned ecell1 = ecell ^ 128u, trl1 = trl ^ 128u;  // (the odd chunks' cells; the second four samples of a transposing read)
  asm volatile("" : "+v"(ecell), "+v"(trl), "+v"(ecell1), "+v"(trl1));
  typedef __attribute__((address_space(3))) s16x4* lp;
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) unsigned long long* lq;
  typedef __attribute__((address_space(3))) bf16x8* l8;
  typedef __attribute__((address_space(3))) float* lf;
  typedef __attribute__((address_space(3))) unsigned short* lh;
  // two fp32 -> one dword of two bf16 (low half = a): ONE v_cvt_pk_bf16_f32.  (Built element by element, hipcc makes every bf16x8 from
  // single converts + v_perm / v_alignbit: ~2.5 instructions per value, and this kernel is bound by its VALU issue -- two waves per
  // SIMD, each 64 transcendentals per tile.)
  // (a vector conversion, not an asm statement: hipcc pads the transcendental -> VALU hazard for its own instructions only, and a
  // v_cvt_pk in an asm statement straight behind the v_sin that feeds it read a stale register now and then -- dW_1 differed from run to run)
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  auto pk = [](float x, float y) -> unsigned { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, y}, bf16x2)); };
  auto swap32 = [](unsigned& x, unsigned& y) {  // x.lanes[32..63] <-> y.lanes[0..31]
    const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    x = r[0]; y = r[1];
  };
  // XT row of component k: rows 0..4 = (x_hi | 1), 5..8 = x_lo; the junk columns of the dA MFMA (5..7, 12..15) read row 0
  const int xrow = (lane & 15) < 5 ? (lane & 15) : ((lane & 15) >= 8 && (lane & 15) < 12) ? (lane & 15) - 3 : 0;
  unsigned xr_base = lds_u32(xt) + (unsigned)(xrow * R::XT_ROW + 8 * hi);
  unsigned xw_base = lds_u32(xt) + (unsigned)(lane * 2);
  asm volatile("" : "+v"(xr_base), "+v"(xw_base));

  // one tile: this wave's two 32-sample blocks w = 2 sh (lanes 0..31 of the X build) and 2 sh + 1 (lanes 32..63)
  auto tile_compute = [&](unsigned sbase, bool do_issue) {
    // ---- X: lane = one of the wave's 64 samples.  The forward pass's hi / lo split of (dx, dy, dz, r, 1) (k_reni_train_bf16: split_x),
    // built ONCE per sample; the MFMA operand of a block wants (first half | second half) of ITS samples in the two lane halves,
    // which is what v_permlane32_swap makes of the two halves' packed words.
    unsigned xa[4], xb[4];  // -> A operands of theta^T for block 2 sh (xa) and 2 sh + 1 (xb)
    {
      const lf dl = (lf)(uintptr_t)(sbase + R::SLOT_G + R::SLOT_A + (unsigned)((64 * sh + lane) * 12));
      const float x0 = dl[0], x1 = dl[1], x2 = dl[2];
      const float x3 = __builtin_amdgcn_sqrtf(x0 * x0 + x2 * x2);  // (1 ulp: the forward's sqrtf may differ in the last bit of r -- far inside bf16)
      const unsigned h01 = pk(x0, x1), h23 = pk(x2, x3);
      const float l0 = x0 - __builtin_bit_cast(float, h01 << 16), l1 = x1 - __builtin_bit_cast(float, h01 & 0xffff0000u);
      const float l2 = x2 - __builtin_bit_cast(float, h23 << 16), l3 = x3 - __builtin_bit_cast(float, h23 & 0xffff0000u);
      const unsigned q01 = pk(l0, l1), q23 = pk(l2, l3);
      constexpr unsigned ONE = 0x3f80u;  // bf16 1.0
      // first half  {xh0, xh1, xh2, xh3, 1, xh0, xh1, xh2};  second half {xh3, 1, xl0, xl1, xl2, xl3, 0, 0}
      xa[0] = h01; xa[1] = h23; xa[2] = ONE | (h01 << 16); xa[3] = (h01 >> 16) | (h23 << 16);
      xb[0] = (h23 >> 16) | (ONE << 16); xb[1] = q01; xb[2] = q23; xb[3] = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) swap32(xa[k], xb[k]);
      // (x_hi | 1 | x_lo) component-major for dA's B operand
      *(lh)(uintptr_t)(xw_base + 0 * R::XT_ROW) = (unsigned short)h01;
      *(lh)(uintptr_t)(xw_base + 1 * R::XT_ROW) = (unsigned short)(h01 >> 16);
      *(lh)(uintptr_t)(xw_base + 2 * R::XT_ROW) = (unsigned short)h23;
      *(lh)(uintptr_t)(xw_base + 3 * R::XT_ROW) = (unsigned short)(h23 >> 16);
      *(lh)(uintptr_t)(xw_base + 4 * R::XT_ROW) = (unsigned short)ONE;
      *(lh)(uintptr_t)(xw_base + 5 * R::XT_ROW) = (unsigned short)q01;
      *(lh)(uintptr_t)(xw_base + 6 * R::XT_ROW) = (unsigned short)(q01 >> 16);
      *(lh)(uintptr_t)(xw_base + 7 * R::XT_ROW) = (unsigned short)q23;
      *(lh)(uintptr_t)(xw_base + 8 * R::XT_ROW) = (unsigned short)(q23 >> 16);
    }
    const bf16x8 aop = *(l8)(uintptr_t)(sbase + R::SLOT_G + (unsigned)((v * 64 + lane) * 16));
    if (do_issue) issue_part(0);
#pragma unroll
    for (int wi = 0; wi < 2; ++wi) {
      const int w = 2 * sh + wi;
      if (wi == 1 && do_issue) issue_part(1);
      const u32x4 xop = wi == 0 ? u32x4{xa[0], xa[1], xa[2], xa[3]} : u32x4{xb[0], xb[1], xb[2], xb[3]};
      // ---- theta_0^T (revolutions: omega_0 / 2 pi rides on afrag)
      f32x16 th;
#pragma unroll
      for (int r = 0; r < 16; ++r) th[r] = 0.f;
      th = PolBF16::mfma(__builtin_bit_cast(bf16x8, xop), aop, th);
      // h_0^T = sin, as B operands of dW_1 (k-slot e of MFMA t = accumulator register 8 t + e); cos for the epilogue
      u32x4 hB[2];
      float cs[16];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        hB[r >> 3][(r & 7) >> 1] = pk(__builtin_amdgcn_sinf(th[r]), __builtin_amdgcn_sinf(th[r + 1]));
        cs[r] = __builtin_amdgcn_cosf(th[r]);
        cs[r + 1] = __builtin_amdgcn_cosf(th[r + 1]);
      }
      // ---- dW_1 += g_1 h_0^T over this block's 32 samples (two MFMA steps), all four row blocks.  Every read below is one of four
      // bases (slot + block + the lane's swizzled cell) plus an immediate.
      const unsigned sw = sbase + (unsigned)(w * 1024);
      const unsigned tb0 = sw + trl, tb1 = sw + trl1, tv0 = tb0 + (unsigned)(v * 8192), tv1 = tb1 + (unsigned)(v * 8192);
      auto tr_frag = [&](unsigned a0, unsigned a1, int off) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(a0 + (unsigned)off));
        const s16x4 h2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(a1 + (unsigned)off));
        const s16x8 w8 = {lo[0], lo[1], lo[2], lo[3], h2[0], h2[1], h2[2], h2[3]};
        return __builtin_bit_cast(bf16x8, w8);
      };
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
          accW[rb] = PolBF16::mfma(tr_frag(tb0, tb1, rb * 8192 + t * 256), __builtin_bit_cast(bf16x8, hB[t]), accW[rb]);
        // db_1 of row block v: the fragment read again at a wave-uniform offset (selected among the four above, hipcc if-converts the
        // uniform condition into four sums and selects)
        accD[0] = PolBF16::mfma(tr_frag(tv0, tv1, t * 256), __builtin_bit_cast(bf16x8, ones), accD[0]);
      }
      if (wi == 1 && do_issue) issue_part(2);
      // ---- dX_1^T = g_1^T W_1 for feature block v
      f32x16 dx;
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[r] = 0.f;
      const unsigned eb0 = sw + ecell, eb1 = sw + ecell1;
#pragma unroll
      for (int c = 0; c < NKS; ++c) {
        const bf16x8 ga = *(l8)(uintptr_t)(((c & 1) ? eb1 : eb0) + (unsigned)(c * 4096));
        dx = PolBF16::mfma(ga, wt[c], dx);
      }
      // g_0^T = dX_1^T (.) cos(theta_0^T) (omega_0 rides on the W_1^T image), packed: A operands of dA
      u32x4 gA[2];
#pragma unroll
      for (int r = 0; r < 16; r += 2) gA[r >> 3][(r & 7) >> 1] = pk(dx[r] * cs[r], dx[r + 1] * cs[r + 1]);
      // ---- dA += g_0 X^T: B operand lane (component row, half khi) = samples 32 wi + 16 t + 4 khi + {0..3, 8..11} of that component
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const unsigned long long q0 = *(lq)(uintptr_t)(xr_base + (unsigned)((32 * wi + 16 * t) * 2));
        const unsigned long long q1 = *(lq)(uintptr_t)(xr_base + (unsigned)((32 * wi + 16 * t) * 2 + 16));
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        const u64x2 qq = {q0, q1};
        accA[0] = PolBF16::mfma(__builtin_bit_cast(bf16x8, gA[t]), __builtin_bit_cast(bf16x8, qq), accA[0]);
      }
    }
    // (Tried, round 5: the two waves of a SIMD -- sh = 0 / 1 of one feature block -- in DIFFERENT piece orders, so that one is on the
    // transcendental unit while the other is on the matrix pipe [sh 0: T0 | MdW0 MdX0 | V0 T1 | MdW1 MdX1 | V1; sh 1: MdX0 | T0 V0 |
    // MdW0 MdX1 | T1 V1 | MdW1; the walk duplicated per order, 209 registers, no spill]: 180-183 us against 178 in lockstep order on
    // the same box.  The two waves do not wait for each other's pipe; the SIMD issues ~1 instruction per 4.5 cycles whichever
    // wave it comes from -- 2 x ~560 instructions per tile = the compute-only ablation's 5.1 k cycles.  Fewer instructions is the lever.)
    // (tests/isa_audit.py counts a taken branch as NO wait state: the shortest path hipcc lays out from the tile's last MFMA to code
    // that touches its accumulator -- the run flush, the loop's next MFMA on it -- is eleven; two more make the strict count)
    __builtin_amdgcn_sched_barrier(0);  // (behind the last MFMA, not in front of it)
    asm volatile("s_nop 1");
    __builtin_amdgcn_sched_barrier(0);
  };

  // the two sample halves' dA sums of an image run -> the run's record (pruns: the training kernel writes its tag and loss slots).
  // `scr`: LDS nobody reads or DMA-writes at the moment (the slot of the tile just finished).  Called by ALL waves.
  auto flush_dA = [&](int b_run, char* scr) {
    __syncthreads();  // every wave is done with the slot
    float* const sc = (float*)scr + (v * 16) * 64 + lane;
    if (sh == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r * 64] = accA[0][r];
    }
    __syncthreads();
    if (sh == 0) {
      float* const rec = a.pruns + ((size_t)g_ * a.pkmax + (size_t)(b_run - b_lo)) * (H * 8 + 16);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float tot = accA[0][r] + sc[r * 64];
        // columns 0..4 = (x_hi | 1), 8..11 = x_lo: the record keeps hi + lo, 8 floats per row (row_shl:8: lane j <- lane j + 8)
        const float lo = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, tot), 0x108, 0xf, 0xf, true));
        if (j < 8) rec[(32 * v + rowmap(r, hi)) * 8 + j] = tot + ((j < 4) ? lo : 0.f);
      }
    }
    acc_zero<1>(accA);
  };

  // ---- the ring
#pragma unroll
  for (int i = 0; i < R::NSLOT - 1; ++i) { if (i < n) issue(); }
  int b_prev = t_hi / a.tiles_per_image, cs_tin = t_hi - b_prev * a.tiles_per_image;  // compute side: image / position of tile i
  unsigned cs_base = ring;                                                              // its slot
#pragma unroll 1
  for (int i = 0; i < n; ++i) {
    TRACE1(1);
    // tile i has landed when at most the tiles behind it are outstanding (they are NSLOT - 2 while the ring is full)
    if (i + R::NSLOT - 2 < n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((R::NSLOT - 2) * R::VM_PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TRACE1(2);
    __syncthreads();  // everybody's pieces of tile i are there, and everybody is done with tile i - 1: its slot is free
    TRACE1(3);
    const bool do_issue = i + R::NSLOT - 1 < n;
    TRACE1(4);
    tile_compute(cs_base, do_issue);
    TRACE1(6);
    // the next tile of the walk: one position down; behind position 0 the image run ends and its dA leaves (the slot just used is free)
    if (--cs_tin < 0 && i + 1 < n) {
      flush_dA(b_prev, smem + (cs_base - ring));
      cs_tin = a.tiles_per_image - 1;
      --b_prev;
    }
    cs_base += R::SLOT;
    if (cs_base == ring + R::NSLOT * R::SLOT) cs_base = ring;
  }
  if (n > 0) flush_dA(b_prev, smem + ((n - 1) % R::NSLOT) * R::SLOT);  // (the last run: the last tile's slot)
  TRACE1(101);
  // ---- dW_1 / db_1: the two sample halves meet in LDS (the ring is idle), one partial [W_1 | b_1] per workgroup
  __syncthreads();
  {
    float* const sc = (float*)smem + (size_t)(v * 64) * 64 + lane;  // [v][rb][r][lane]
    float* const sd = (float*)smem + 4 * 64 * 64 + (v * 2 + hi) * 16;  // [v][hi][r]: column 0's lanes
    if (sh == 1) {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[(rb * 16 + r) * 64] = accW[rb][r];
      if (j == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sd[r] = accD[0][r];
      }
    }
    __syncthreads();
    if (sh == 0) {
      float* const dwp = a.dw1p + (size_t)blockIdx.x * (H * H + H);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          dwp[(size_t)(32 * rb + rowmap(r, hi)) * H + 32 * v + j] = accW[rb][r] + sc[(rb * 16 + r) * 64];
      if (j == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dwp[H * H + 32 * v + rowmap(r, hi)] = accD[0][r] + sd[r];
      }
    }
  }
#if defined(RENI_TRACE_DW1)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TRACE1(102);
  if (trace_on) {
    for (int k = lane; k < trace_n; k += 64) a.trace[k] = (long long)trace_lds[k];
  }
#endif
}
template __global__ void k_reni_l0_ring<128>(const MainArgs);
