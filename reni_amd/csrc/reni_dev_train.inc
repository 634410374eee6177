// reni_dev_train.inc -- the register-persistent bf16 kernels (H = 128, L <= 5): k_reni_train_bf16 (training / frozen / statistics / FiLM instances) and k_reni_dw1
// Part of reni_device.inc (included there, inside namespace reni; never compiled on its own).

// ---- helpers of the bf16 training path ---------------------------------------------------------
// Design decisions of the bf16 persistent kernels that were settled by same-box A/B measurements (profiles/r02_variants.md,
// profiles/r03_variants.md; the rejected alternatives are described there, not kept here):
//  * vector-memory operations go out in bursts / three-piece LDS-DMA groups, not one per MFMA slot;
//  * a backward step's dX GEMM is four single accumulate chains with the cos epilogue of row block r behind row block r + 1, and
//    in the training instance it is interleaved MFMA by MFMA with the step's dW GEMM (dwdx_layer);
//  * layer 0's phases are not stashed but rebuilt in the last backward step from the image's A operands (four K = 16 MFMAs);
//    the last layer's phases never leave the registers; the frozen instance also keeps layer L - 1's in registers;
//  * the forward pass is software-pipelined across layers (row blocks 2 and 3 of a layer are activated behind the first MFMAs
//    of the next layer's GEMM);
//  * the concat instances keep a sine argument as the fp16 number of revolutions it IS, not reduced to [0, 1) first:
//    v_sin_f32 / v_cos_f16 take any argument up to +-256 revolutions, and an fp16 keeps an unreduced |x| < 1/2 finer than its
//    fractional part in [1/2, 1) (a small negative x becomes 1 - |x|), |x| in [1/2, 1) as fine, [1, 2) twice and [2, 4) four times
//    coarser -- SIREN pre-activations at omega = 30 stay within about one revolution (measured parity unchanged:
//    profiles/r03_parity_numbers.txt).  FiLM keeps the reduction: its angles freq (W h + b) + phase reach tens of revolutions.
// pads behind the LAST MFMA of a chain at the sites where independent instructions follow on every path (see mfma_bf16_pin_v's TAILN):
// the values are the smallest the audit (tests/isa_audit.py, every instance, every path) accepts
constexpr int TAIL_RB2 = 1, TAIL_DWDX = 1, TAIL_DWDX_A = 1;
#ifdef RENI_TU_TRAIN_FILM
// (the pads are proven per translation unit on the emitted instruction streams: the FiLM instances interleave other fillers behind the
// forward GEMMs' first accumulator -- tests/isa_audit.py finds 10 / 11 states there with the concat instances' pad of three, twelve
// with five -- and take the concat values at the other three sites)
constexpr int TAIL_RB1 = 5;
#else
constexpr int TAIL_RB1 = 3;
#endif
template <int N, class F>
DEV void static_for_down(F&& f) {
  if constexpr (N >= 1) {
    f(std::integral_constant<int, N>{});
    static_for_down<N - 1>(f);
  }
}

template <int I, int N, class F>
DEV void static_for_up(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_up<I + 1, N>(f);
  }
}

template <int H>
struct GeoP {
  using G = Geo<PolBF16, H>;
  static constexpr int WBSZ = ((G::IMG_HID + G::BIAS_HID + 3071) / 3072 * 3072 + 1023) & ~1023;  // DMA moves 3 KB groups
  // (copying a whole number of groups PER WAVE -- twelve for the 33 KB image, so that every wave issues the same three --
  // was measured slower: the extra 3 KB per image cost more than the waves' imbalance at the barrier)
  static constexpr int TSZ = 128 * 256;  // sample-major image, see ts_write / ts_read
  // the two head images (W_out for the forward, W_out^T for the backward) stay resident for the whole kernel
  static constexpr int HFSZ = (G::IMG_HF + G::BIAS_HEAD + 3071) / 3072 * 3072, HBSZ = (G::IMG_HB + 3071) / 3072 * 3072;
  static constexpr int DASZ = H * 8 * 4;  // layer-0 dA of the current image run (training instance)
  static constexpr int LDS_BYTES = 2 * WBSZ + 2 * TSZ + 2048 + HFSZ + HBSZ + DASZ;  // + head dW accumulators + head images + dA
  static constexpr int LACC_BYTES = 128 * 16;  // concat training instance: per-lane (loss, g_y) accumulators behind dA (see LACC)
  static constexpr int L0X_TW_BYTES = 1536;    // L0X instance: the tile's weight rows behind the accumulators (directions and target: in the dA region)
  // distance between the packed images of consecutive hidden layers (make_layout, reni_capi.inc: every image starts on a 1 KB
  // boundary): the kernel forms an image's address from layer 1's offset + a multiple of this -- a table look-up was a scalar load
  // from the kernel-argument block and a wait for it, ten times per tile
  static constexpr unsigned FWD_STRIDE = (G::IMG_HID + G::BIAS_HID + 1023) & ~1023, BWD_STRIDE = (G::IMG_HID + 1023) & ~1023;
};

// async global -> LDS copy of `bytes` (rounded up to 1 KB; the image regions are padded) split over 4 waves.
// The LDS-DMA instruction is issued from inline asm ON PURPOSE: hipcc cannot tell which part of the one
// dynamic LDS array a __builtin_amdgcn_global_load_lds writes, so it put `s_waitcnt vmcnt(0)` in front of
// the next ds_read of ANY buffer -- every backward step waited out the DMA it had just issued instead of
// overlapping it with its two GEMMs.  An asm statement is invisible to that bookkeeping; completion is
// awaited explicitly with dma_wait() before the barrier that publishes the image (one step later).

template <int BYTES>
DEV void dma_image(char* lds_dst, const char* gsrc, int wave, int lane16) {
  constexpr int NP = (BYTES + 1023) / 1024;
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_dst);
#pragma unroll
  for (int pi = 0; pi < (NP + 3) / 4; ++pi) {
    const int piece = pi * 4 + wave;
    if (piece < NP) glds16(gsrc + piece * 1024, (unsigned)lane16, dst + piece * 1024);
  }
}

// The training kernel hands a DmaJob to its GEMM loops, which issue one 3 KB group per k-step between MFMAs (a burst
// of 8-9 LDS-DMA instructions per wave stalls on the memory pipeline's queue for ~1.2k cycles per step; spread out,
// the issue slots hide behind the MFMAs).
struct DmaJob {
  const char* src;    // image in global memory (wave-uniform)
  unsigned lane_off;  // lane * 16
  unsigned dst;       // wave-uniform LDS byte address of the image
  int ng;             // 3 KB groups (the copy is rounded up to whole groups: the buffers and the image region are padded)
};
// Three 1 KB pieces per M0 / base setup: the instruction offset of an LDS-DMA load applies to the global AND the
// LDS address, so consecutive pieces need no new registers.  Piece by piece (s_cmp, branch, two address adds, M0
// save / set / restore per KB) the copies were ~1000 scalar instructions per tile, a tenth of everything issued.
DEV void glds16x3(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  unsigned keep;  // M0 is saved and restored: it is a reserved register as far as hipcc is concerned
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, %2\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst_uniform) : "memory");
}
// group g of this wave (the waves take the groups round-robin); the GEMM loops issue one group per k-step
DEV void dma_group(const DmaJob& jb, int g, int wave, int nwaves = 4) {
  const int gi = g * nwaves + wave;
  if (gi < jb.ng) glds16x3(jb.src + gi * 3072, jb.lane_off, jb.dst + gi * 3072);
}
constexpr int DMA_GROUPS = 3;  // per wave: 4 x 3 x 3 KB = 36 KB >= the largest image
struct NoFill { DEV void operator()(int) const {} DEV void operator()(int, int) const {} };
// SHARED weight image (the L0X training instance: one image per hidden layer serves the forward GEMM and the backward step's dX GEMM).
// Fragment (row block, k-step ks) of the forward layout is 1 KB = 64 cells of 16 bytes, cell = lane; in a shared image lane (hi, r)'s cell
// sits at lane ^ (4 hi + 8 (ks & 1)) -- written so by k_pack (PackDesc::swz), copied as it lies by the LDS-DMA.  The forward ds_read_b128
// stays free of bank conflicts (an XOR with a constant per 32-lane half), and so are the transposing 8-byte reads that assemble the
// fragments of W^T from it (wimg_tr_base): the two halves of a k pair (hi) and the two k-steps of a column group (ks & 1), which lie
// 512 B and 1 KB apart -- the same banks -- in the plain layout, land in different 64-byte quarters of the 256-byte bank row.
DEV int wimg_cell(int lane, int ks) { return lane ^ (((lane >> 5) << 2) | ((ks & 1) << 3)); }
// per-lane byte offset (row block 0 of W^T, k-step 0, first half) of the transposing reads of a shared image.  A bf16 fragment holds the
// k indices kfeat(ks, hi, e) = 16 ks + 4 hi + (e & 3) + 8 (e >> 2): its 8-byte half e >> 2 is four consecutive k.  Fragment (kb, s) of W^T
// needs, in lane (khi, j), W[16 s + 8 q + 4 khi + 0..3][32 kb + j] in half q, so source lane (khi, g, u) of read q supplies row
// o = 8 q + 4 khi + (u >> 2) of W, columns 16 g + 4 (u & 3) .. + 3: forward fragment k-step g (+ 2 per row block kb), its half hi = u & 1,
// 8-byte half (u >> 1) & 1 of cell o.  Second read (q = 1): ^ 128; row block kb of W^T: + 2048 kb; k-step s: + 8192 (s >> 1) + 256 (s & 1)
// -- immediates.
DEV unsigned wimg_tr_base(int lane) {
  const int khi = lane >> 5, g = (lane >> 4) & 1, u = lane & 15, h = u & 1;
  return (unsigned)(g * 1024 + h * 512 + (((4 * khi + (u >> 2)) ^ (4 * h + 8 * g)) << 4) + ((u >> 1) & 1) * 8);
}

// acc[rbo] (+)= W-image[rbo] . bop   (row-block-outer order so the caller's per-row-block epilogue
// overlaps the next row block's MFMAs)
// All MFMAs of the training kernel name their accumulator's register file explicitly: the 256 AGPRs belong
// to the sixteen persistent dW tiles, so the chain GEMMs accumulate in VGPRs ("+v").  The last MFMA of a
// chain carries the wait states the following VALU reads of the result need.
template <int NKS>
DEV f32x16 gemm_rb(const char* wb, int rbo, const bf16x8 (&bop)[NKS], f32x16 acc, int lane) {
  // every A fragment is requested before the first MFMA: fetched one at a time, each of the chain's MFMAs waited out
  // a whole LDS round trip (cycle trace: the head's 8 MFMAs took 1280 cycles)
  constexpr int D = NKS;
  bf16x8 a[D];
#pragma unroll
  for (int ks = 0; ks < D; ++ks) a[ks] = *(const bf16x8*)(wb + ((rbo * NKS + ks) * 64 + lane) * 16);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const bf16x8 ak = a[ks % D];
    if (ks + D < NKS) a[ks % D] = *(const bf16x8*)(wb + ((rbo * NKS + ks + D) * 64 + lane) * 16);
    if (ks == NKS - 1) mfma_bf16_pin_v<true, NKS == 1>(acc, ak, bop[ks]);
    else if (ks == 0) mfma_bf16_pin_v<false, true>(acc, ak, bop[ks]);
    else mfma_bf16_pin_v<false, false>(acc, ak, bop[ks]);
  }
  return acc;
}

// two row blocks at once: their MFMA chains are independent, so alternating them keeps the matrix pipe
// busy instead of waiting out each dependent-accumulator latency
// SWZ: the image is a SHARED one (wimg_cell): the lane's 16-byte cell of fragment (row block, k-step) is XOR-ed with 4 hi + 8 (ks & 1)
template <int NKS, class F = NoFill, bool ZERO = false, bool SWZ = false>
DEV void gemm_rb2(const char* wb, int rbo0, const bf16x8 (&bop)[NKS], f32x16& acc0, f32x16& acc1, int lane,
                  const F& fill = F()) {  // ZERO: the accumulators start at zero (inline-constant SrcC, nothing to initialise)
  // A fragments are fetched two k-steps ahead of the MFMAs that use them (three and four: no faster, measured): with four waves and the LDS-DMA
  // writes on the LDS at once a ds_read_b128 takes longer than two MFMA pairs
  // (SWZ: two per-lane bases, the cell XOR-ed with 4 hi and -- odd k-steps -- with 8: an XOR of the address with 128, the buffers being
  // 1 KB aligned.  Both made HERE, per GEMM, and opaque: kept across the tile they would be two registers the instance does not have;
  // made at every odd k-step's read they were sixteen more VALU instructions per layer in an issue-bound kernel)
  typedef __attribute__((address_space(3))) const bf16x8* lbp;
  unsigned sb = SWZ ? (unsigned)(size_t)wb + (unsigned)(wimg_cell(lane, 0) * 16) : 0u, sb1 = sb ^ 0x80u;
  if constexpr (SWZ) asm volatile("" : "+v"(sb), "+v"(sb1));
  auto fa = [&](int r, int ks) {
    if constexpr (SWZ) {
      const unsigned ad = (ks & 1) ? sb1 : sb;
      return *(lbp)(uintptr_t)(ad + (unsigned)(((rbo0 + r) * NKS + ks) * 1024));
    } else {
      return *(const bf16x8*)(wb + (((rbo0 + r) * NKS + ks) * 64 + lane) * 16);
    }
  };
  constexpr int D = NKS >= 2 ? 2 : 1;
  bf16x8 q0[D], q1[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { q0[d] = fa(0, d); q1[d] = fa(1, d); }
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const bf16x8 a0 = q0[ks % D], a1 = q1[ks % D];
    if (ks + D < NKS) { q0[ks % D] = fa(0, ks + D); q1[ks % D] = fa(1, ks + D); }
    if (ks == 0 && ZERO) mfma_bf16_zero_v<false>(acc0, a0, bop[ks]);
    else if (ks == 0) mfma_bf16_pin_v<false, true>(acc0, a0, bop[ks]);
    else mfma_bf16_pin_v<false, false>(acc0, a0, bop[ks]);
    // the filler comes in two parts, one behind each MFMA: the second MFMA of a pair cannot issue before the first has
    // left the matrix pipe (8 passes), and nothing behind it issues either -- a filler placed after both overlaps one
    fill(ks, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks == 0 && ZERO) mfma_bf16_zero_v<NKS == 1>(acc1, a1, bop[ks]);
    else if (ks == NKS - 1) mfma_bf16_pin_v<true, NKS == 1, NKS == 1 ? -1 : TAIL_RB2>(acc1, a1, bop[ks]);
    else if (ks == 0) mfma_bf16_pin_v<false, true>(acc1, a1, bop[ks]);
    else mfma_bf16_pin_v<false, false>(acc1, a1, bop[ks]);
    fill(ks, 1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// one row block, ONE accumulate chain (consecutive MFMAs on the same accumulator issue at the pipe's rate, 33.6 cycles each
// with or without fillers: profiles/r02_mfma_shadow.md); fill(ks) runs behind the MFMA of k-step ks
template <int NKS, class F = NoFill, bool ZERO = false>
DEV void gemm_rb1(const char* wb, int rbo, const bf16x8 (&bop)[NKS], f32x16& acc, int lane, const F& fill = F()) {
  auto fa = [&](int ks) { return *(const bf16x8*)(wb + ((rbo * NKS + ks) * 64 + lane) * 16); };
  constexpr int D = NKS >= 4 ? 3 : NKS >= 2 ? 2 : 1;  // fragments in flight (one per MFMA here, two in gemm_rb2)
  bf16x8 q[D];
#pragma unroll
  for (int d = 0; d < D; ++d) q[d] = fa(d);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const bf16x8 a = q[ks % D];
    if (ks + D < NKS) q[ks % D] = fa(ks + D);
    if (ks == 0 && ZERO) mfma_bf16_zero_v<NKS == 1>(acc, a, bop[ks]);
    else if (ks == NKS - 1) mfma_bf16_pin_v<true, NKS == 1, NKS == 1 ? -1 : TAIL_RB1>(acc, a, bop[ks]);
    else if (ks == 0) mfma_bf16_pin_v<false, true>(acc, a, bop[ks]);
    else mfma_bf16_pin_v<false, false>(acc, a, bop[ks]);
    fill(ks);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int H, int NB>
DEV void t_write_b(char* T, const bf16x8 (&xb)[2 * NB], int wave, int hi, int j) {
  using G = Geo<PolBF16, H>;
#pragma unroll
  for (int rb = 0; rb < NB; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      *(__bf16*)(T + (32 * rb + rowmap(r, hi)) * G::T_ROWB + (wave * 32 + j) * 2) = xb[2 * rb + (r >> 3)][r & 7];
}

// phase (revolutions, u16) pair in one dword -> two floats in [1,2): sin/cos of 2*pi*x are periodic in 1

// ---- sample-major transposition image of the bf16 training path (H = 128) --------------------------
// Row s (one of the tile's 128 samples) = 256 B = 32 pieces of 8 B; logical piece c holds features
// 4c..4c+3 of that sample.  Pieces are stored at c ^ tswz(s), which makes both the 8-byte writes (a lane
// owns a sample) and the ds_read_b64_tr_b16 transpose reads (a lane ends up owning a feature) free of LDS
// bank conflicts (DESIGN.md section 4).  A fragment read returns, to lane l, feature 32*blk + (l & 31) for
// samples 16*ks + 8*(l >> 5) + 0..7 -- the MFMA operand layout with K = samples.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr int TS_BYTES = 128 * 256;
DEV int tswz(int s) { return ((s & 1) << 4) | ((s & 2) << 2) | ((s & 1) << 2) | ((s & 8) >> 2) | ((s & 4) >> 2); }

// The images sit at 256-byte-aligned LDS addresses (the dynamic LDS array is declared aligned(1024) and every
// image offset is a multiple of 1 KB), so a row's address has a zero low byte and the swizzled piece index can be
// XOR-ed straight into the ADDRESS: one v_xor per access with the lane's base held in a register, instead of
// rebuilding (piece ^ swizzle) << 3 and adding the row every time.
DEV unsigned lds_u32(const char* p) { return (unsigned)(size_t)p; }  // LDS byte address of a pointer into the dynamic array
typedef __attribute__((address_space(3))) u32x2* lds_u32x2_p;

// write NB 32-feature blocks of packed bf16 (D layout) for sample s
template <int NB>
DEV void ts_write(char* T, const bf16x8 (&xb)[2 * NB], int s, int hi) {
  // piece (8 rb + 2 u + hi) ^ tswz(s)  ==  (8 rb + 2 u) ^ (hi ^ tswz(s)): the lane part goes into the base
  unsigned base = lds_u32(T) + s * 256 + ((tswz(s) ^ hi) << 3);
  // opaque: otherwise hipcc hoists the swizzled addresses out of the tile loop and holds them in registers for
  // the whole kernel (the training kernel has none to spare)
  asm volatile("" : "+v"(base));
#pragma unroll
  for (int rb = 0; rb < NB; ++rb)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u32x4 w = __builtin_bit_cast(u32x4, xb[2 * rb + (u >> 1)]);
      const u32x2 h = (u & 1) ? u32x2{w[2], w[3]} : u32x2{w[0], w[1]};
      *(lds_u32x2_p)(uintptr_t)(base ^ (unsigned)((8 * rb + 2 * u) << 3)) = h;
    }
}
// the two 8-byte halves of one bf16x8 (features 8*(c&1).. of block c>>1, i.e. chunk index c) for sample s;
// `base` from ts_write_base
DEV unsigned ts_write_base(char* T, int s, int hi) {
  unsigned base = lds_u32(T) + s * 256 + ((tswz(s) ^ hi) << 3);
  asm volatile("" : "+v"(base));  // see ts_write
  return base;
}
DEV void ts_write_chunk(unsigned base, bf16x8 v, int c) {
  const u32x4 w = __builtin_bit_cast(u32x4, v);
  const int rb = c >> 1, u0 = 2 * (c & 1);
  *(lds_u32x2_p)(uintptr_t)(base ^ (unsigned)((8 * rb + 2 * u0) << 3)) = u32x2{w[0], w[1]};
  *(lds_u32x2_p)(uintptr_t)(base ^ (unsigned)((8 * rb + 2 * (u0 + 1)) << 3)) = u32x2{w[2], w[3]};
}
// per-lane LDS addresses (block 0, k-step 0) of the two transpose reads that make one fragment of image T
struct TsBase { unsigned q[2]; };
DEV TsBase ts_base(const char* T, int lane) {
  const int khi = lane >> 5, g = (lane >> 4) & 1, u = lane & 15;
  const int s0 = (u >> 2) & 1, s1 = (u >> 3) & 1;
  TsBase b;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int x = (s0 << 4) | (s1 << 3) | (s0 << 2) | (khi << 1) | q;
    const int phys = ((4 * g + (u & 3)) ^ (x & 7)) | ((x >> 3) << 3);
    b.q[q] = lds_u32(T) + (8 * khi + 4 * q + (u >> 2)) * 256 + phys * 8;
  }
  asm volatile("" : "+v"(b.q[0]), "+v"(b.q[1]));  // keeps the per-block XOR-ed addresses out of LICM (see ts_write)
  return b;
}
// block blk (its 64-byte column group XORs into the low address byte), k-step ks (an immediate offset)
// (img_off: the same fragment of the image that lies img_off bytes behind b's -- one more immediate, no bases of its own)
DEV bf16x8 ts_read(const TsBase& b, int blk, int ks, unsigned img_off = 0) {
  typedef __attribute__((address_space(3))) s16x4* lp;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)((b.q[0] ^ (unsigned)(blk << 6)) + (unsigned)(ks * 4096) + img_off));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)((b.q[1] ^ (unsigned)(blk << 6)) + (unsigned)(ks * 4096) + img_off));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// K = samples GEMM from sample-major images: rows block(s) x cols block(s), 128 samples.
// Wave w owns row block w (NBR == 4) and all NBC column blocks.  PIN: 0 compiler-allocated accumulator,
// 2 accumulator pinned to VGPRs (asm MFMA), starting from zero.
template <int NBC, int KIND, int PIN, class F = NoFill>
DEV void dw_gemm_s(const char* TA, const char* TB, f32x16 (&acc)[NBC], float& dbacc, int wave, int lane,
                   const F& fill = F()) {
  const TsBase bA = ts_base(TA, lane), bB = ts_base(TB, lane);
  // fragments are requested PF k-steps ahead (a ring of register sets): one k-step at a time, every MFMA of these short
  // GEMMs (head dW, layer-0 dA: one column block) waited out the transposing reads' round trip
  constexpr int PF = NBC == 1 ? 4 : 1;
  bf16x8 ra[PF], rbf[PF][NBC];
#pragma unroll
  for (int d = 0; d < PF; ++d) {
    ra[d] = ts_read(bA, wave, d);
#pragma unroll
    for (int m = 0; m < NBC; ++m) rbf[d][m] = ts_read(bB, m, d);
  }
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const bf16x8 fa = ra[ks % PF];
    bf16x8 fbv[NBC];
#pragma unroll
    for (int m = 0; m < NBC; ++m) fbv[m] = rbf[ks % PF][m];
    if (ks + PF < 8) {
      ra[ks % PF] = ts_read(bA, wave, ks + PF);
#pragma unroll
      for (int m = 0; m < NBC; ++m) rbf[ks % PF][m] = ts_read(bB, m, ks + PF);
    }
#pragma unroll
    for (int m = 0; m < NBC; ++m) {
      const bf16x8 fb = fbv[m];
      if constexpr (PIN == 2) {  // (the accumulators start at zero: inline-constant SrcC in the first k-step)
        if (ks == 7 && m == NBC - 1) mfma_bf16_pin_v<true, false>(acc[m], fa, fb);
        else if (ks == 0) mfma_bf16_zero_v<false>(acc[m], fa, fb);
        else mfma_bf16_pin_v<false, false>(acc[m], fa, fb);
      } else {
        acc[m] = PolBF16::mfma(fa, fb, acc[m]);
      }
      if (KIND == DW_HEAD && m == 0 && wave == 0) dbacc = frag_sum<PolBF16>(fb, dbacc);
    }
    if (KIND == DW_HIDDEN) dbacc = frag_sum<PolBF16>(fa, dbacc);
    fill(ks);
    if constexpr (PIN != 0) __builtin_amdgcn_sched_barrier(0);
  }
}

// ==========================================================================================
// bf16 TRAINING kernel with register-persistent weight-gradient accumulators (H = 128, L <= 5)
// ==========================================================================================
// Same arithmetic as k_reni_main<PolBF16, 128, MODE_FWD_BWD>, different schedule:
//   * the dW_l accumulators of all hidden layers (5 x 128 x 128 fp32 = 320 KB per workgroup, 62 % of a
//     CU's register file) stay in registers across the workgroup's whole tile loop and are written
//     ONCE per launch.  hipcc allocates every MFMA accumulator of a kernel in AGPRs (256 = sixteen
//     32x32 tiles), so the tiles are pinned by hand: layers 2..5 in AGPRs, layer 1 in VGPRs
//     (mfma_bf16_agpr_tile).  The generic kernel's per-tile "+=" flush of those partials was 65 % of
//     its run time (profiles/r01_b_ablation.md);
//   * one workgroup (4 waves, one per SIMD, up to 512 registers each) per CU;
//   * activations / gradients travel between layers as packed bf16 MFMA operands;
//   * weight images are double-buffered in LDS and fetched one step ahead by LDS-DMA
//     (global_load_lds): one barrier per forward layer, two per backward layer, no staging stall.
// DW = false: the frozen-decoder instance (latent-only optimisation, BASELINE config 4): the same forward and dX chain,
// no weight-gradient work -- no operand transposition, no dW GEMMs, no g_1 stream, one barrier per backward layer.
// STATS = true (with DW = false): forward only, per-tile sums of out*t, out^2, t^2 per channel -- the statistics pass
// of RENITestLoss's cosine term (loss_functions.py:25-32), on the same pre-scaled weight images as the main pass.
// FILM = true: FiLM conditioning on the persistent kernels (reference src/models/RENI.py:508-519, 665-676).  Hidden layer l of
// image b applies sin(freq_bl . (W_l h + b_l) + phase_bl): the per-image (freq / 2 pi, phase / 2 pi) vectors of the workgroup's
// current image sit in LDS (six 1 KB slots, slot 0 = the identity for the folded first layer) and enter the activation as one FMA;
// the backward's operand is g_a = freq . cos(theta) . g_h for BOTH GEMMs, so the weight-gradient accumulators need no per-image
// state, and at the end of an IMAGE RUN (contiguous tile ranges) the run's accumulators R = sum g_a h^T give
//   d phase = (sum g_a) / freq,   d freq = rowsum(W (.) R) / freq + b (.) d phase   (k_reduce_film_runs adds the b term),
// are flushed into the run's partial slot and start again from zero.  Instances: <H, true, false, true> (training, and a frozen
// decoder: d freq needs the weight-gradient GEMMs) and <H, false, true, true> (inference / statistics pass).
// SPEC = true (training instance only): the head / loss configuration every shipped FIT_DECODER run uses -- linear head, tanh,
// WeightedMSE (RENITrainLoss), no output image wanted -- as COMPILE-TIME constants.  The generic instance decides all four per tile
// with scalar branches and spilled-SGPR reads around ~20 MFMAs (cycle trace: 2.6 k cycles for head forward + loss); here that code is
// straight-line.  launch_train picks it when the call's flags match.
// L0X = true (SPEC concat training instance only, round 5): layer 0's backward is NOT part of this kernel.  The tile ends with the
// step of layer 2 -- whose dX epilogue produces g_1 -- and the g_1 stream's stores; layer 1's dX GEMM, its cosine epilogue, the
// layer-0 phase rebuild and the dA GEMM (13 % of a tile: profiles/r04_cycle_trace.txt, tags 191-214 and 8-9) are done by
// k_reni_l0_ring (reni_dev_l0ring.inc), which reads the g_1 stream anyway, holds W_1^T in registers and is bound by HBM, not by
// issue.  ONE weight image per hidden layer serves both passes (SHARED images: wimg_cell): the backward step of layer l reads
// W_l^T out of the forward image with transposing reads, in the buffer the forward pass used for it -- layer l's image lives in buffer
// (l - 1) & 1, whatever the tile.  Copies per tile (L = 5: six, where two images per layer made nine): the forward pass loads layers
// 3 .. L (layer 1's came with the previous tile's last step, layer 2's is still in its buffer from that step; the FIRST tile of a range
// loads both), the backward pass finds layers L and L - 1 where the forward pass left them and loads L - 2 .. 2, and the last step
// (layer 2's, reading buffer 1) fetches the next tile's layer 1 into buffer 0 -- nothing after the range's last tile.  Every copy goes
// into the buffer whose last reader lies behind the barrier the copy is issued after.  The g_1 stream is stored with its
// 16-byte cells XOR-swizzled (cell ^ 4 hi ^ 8 (chunk & 1)): both of the ring kernel's reads of the raw slot -- plain b128 operands and
// the transposing reads -- are then free of LDS bank conflicts.
template <int H, bool DW, bool STATS = false, bool FILM = false, bool SPEC = false, bool L0X = false>
__global__ void __launch_bounds__(DW ? 256 : 512, 1) k_reni_train_bf16(const MainArgs a) {
  static_assert(!(DW && STATS), "the statistics instance has no backward pass");
  static_assert(!SPEC || DW, "SPEC is an instance of the training kernel");
  static_assert(!L0X || (SPEC && !FILM), "L0X is a form of the concat SPEC instance");
  static_assert(!FILM || DW || STATS, "FiLM: the training instance serves the frozen decoder too");
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  using GP = GeoP<H>;
  static_assert(H == 128, "sample-major transposition image is laid out for H = 128");
  constexpr int NRB = G::NRB, NKS = G::NKS;
  constexpr int MYB_H = (NRB * NRB + 3) / 4;
  constexpr int PMAX = 5;
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // ts_write / ts_read XOR into the low address byte
  char* const TA = smem + 2 * GP::WBSZ;
  char* const TB = TA + GP::TSZ;
  float* const hdw = (float*)(TB + GP::TSZ);  // [3][H] dW_out + [3] db_out accumulated over the tile loop
  char* const HF = TB + GP::TSZ + 2048;       // resident head images: no DMA, no 'image landed' barrier in the head steps
  char* const HB = HF + GP::HFSZ;
  float* const dAacc = (float*)(HB + GP::HBSZ);  // [H][8] layer-0 dA summed over the tiles of the current image run
  // FiLM tables [slot 0..PMAX][2][H] of the current image (freq / 2 pi | phase / 2 pi; slot 0 = (1, 0)).  Training instance:
  // behind dAacc; the eight-wave instances: one table per half in the transposition image TB, which they never use.
  constexpr int FT_FLOATS = (PMAX + 1) * 2 * H;
  float* const ftab_base = FILM ? (DW ? dAacc + H * 8 : (float*)TB) : nullptr;

#ifdef RENI_TRACE
  // cycle trace of workgroup 0, wave 0 (profiles/tools/gpu_trace.py): (tag << 48 | s_memtime) words collected in the LDS
  // behind the kernel's own buffers and copied out once at the end -- a trace point costs one s_memtime round trip and one
  // ds_write_b64, and issues no vector-memory operation (global stores from the tile loop made every point a vmcnt(0))
  unsigned long long* const trace_lds = (unsigned long long*)(smem + GP::LDS_BYTES + GP::LACC_BYTES);  // (4 KB: 512 words)
  int trace_n = 0;
#ifndef RENI_TRACE_WAVE
#define RENI_TRACE_WAVE 0
#endif
  const bool trace_on = a.trace != nullptr && blockIdx.x == 0 && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == RENI_TRACE_WAVE;
#define TRACE(tag) do { __builtin_amdgcn_sched_barrier(0); if (trace_on && trace_n < 500) { trace_lds[trace_n] = ((unsigned long long)__builtin_amdgcn_s_memtime() & 0xffffffffffffull) | ((unsigned long long)(tag) << 48); ++trace_n; } __builtin_amdgcn_sched_barrier(0); } while (0)
#define TRACE_FLUSH(slot, tag) do { __builtin_amdgcn_sched_barrier(0); if (trace_on) trace_lds[slot] = ((unsigned long long)__builtin_amdgcn_s_memtime() & 0xffffffffffffull) | ((unsigned long long)(tag) << 48); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TRACE(tag) do {} while (0)
#define TRACE_FLUSH(slot, tag) do {} while (0)
#endif
  const int tid = threadIdx.x;
  // The frozen instance runs EIGHT waves (two per SIMD: it has no accumulator tiles to hold and is latency-bound at one)
  // on two 128-sample tiles at a time: waves 0-3 = half 0, waves 4-7 = half 1.  Both halves share the weight buffers
  // (one LDS-DMA per 256 samples) and every barrier; everything per tile is indexed by the wave's position in its
  // half (wq).  The training instance: NW = 4, one half, wq == wave.
  constexpr int NW = DW ? 4 : 8, NHALF = NW / 4, DG = DW ? DMA_GROUPS : 2;  // DG * NW 3 KB groups >= the largest image
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, half = wave >> 2;
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  // stash layout [layer][workgroup][32 KB (x 2 halves)]: the workgroups run in step, so at any moment all of them store (or load) the
  // SAME layer -- layer-major, those accesses cover one contiguous 8 MB region, spread evenly over the memory channels; workgroup-major
  // (stride = 6 layers x 32 KB) the cost of a layer's eight stores varied between 150 and 650 cycles with the layer's slot (cycle trace)
  char* const stash = a.stash + (size_t)blockIdx.x * (G::STASH_LAYER_BYTES * (DW ? 1 : 2));
  const size_t stash_layer_stride = (size_t)gridDim.x * (G::STASH_LAYER_BYTES * (DW ? 1 : 2));
  float* const dwp = a.dwp + (size_t)blockIdx.x * a.dwp_per_wg;
  const int L = a.L;
  const int nstep = L0X ? 2 * L + 1 : 2 * L + 2;  // weight images consumed per tile (L0X: no step for layer 1)

  static_assert(MYB_H == 4, "sixteen AGPR tiles = 4 layers x 4 column blocks");
  if constexpr (DW) agpr_zero_seq(std::make_integer_sequence<int, 256>{});  // dW_2..dW_5 accumulators: a[0:255]
  float pdb[PMAX];
#pragma unroll
  for (int l = 0; l < PMAX; ++l) pdb[l] = 0.f;
  if constexpr (DW) {
    for (int i = tid; i < 3 * H + 32; i += 256) hdw[i] = 0.f;
    for (int i = tid; i < H * 8; i += 256) dAacc[i] = 0.f;
  }
  // LACC: the tile's weighted squared error and its three d loss / d y sums (db_out) are NOT reduced across the lanes per tile (four
  // wave sums = 56 DPP instructions with their wait states, two LDS read-modify-writes on lane 0): every owner lane adds its four
  // values to a slot of its own in LDS (one ds_read_b128, two packed adds, one ds_write_b128); the loss leaves with the image run, the
  // db_out sums once per launch.  SPEC instance only.
  constexpr bool LACC = SPEC;  // (in the generic instance, at 256 registers, the same change costs 1.2 %: profiles/r04_variants.md)
  f32x4* const lacc = (f32x4*)(dAacc + H * 8 + (FILM ? FT_FLOATS : 0));  // [4 waves][32 owner lanes] (FiLM: behind the tables)
  float* const hdb = hdw + 3 * H + 16;      // [4 waves][4] db_out, each wave's own samples
  float* const loss_run = hdw + 3 * H + 8;  // [4] each wave's weighted squared error over the current image run (LDS: the
                                            // kernel has no register to spare for it)
  if constexpr (DW) { if (tid < 4) loss_run[tid] = 0.f; }
  if constexpr (LACC) { if (tid < 128) lacc[tid] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // (SPEC: the head's configuration as constants)
  const int act = SPEC ? 1 : a.act;
  const bool last_linear = SPEC ? true : (a.last_linear != 0);
  const int loss_kind = SPEC ? 0 : a.loss_kind;
  float* const out_img = SPEC ? nullptr : a.out;
  const float inv3p = 1.0f / (3.0f * (float)a.P);
  int run_k = 0;         // image runs flushed so far

  int lane16 = lane * 16, tid16 = tid * 16;  // re-made opaque at the top of every tile iteration
  // image of step k of a tile: k < L hidden fwd (layer k+1), k == L head fwd, k == L+1 head bwd,
  // then hidden bwd for layer 2L+2-k.  Buffer = k & 1.
  const char* wimg_f1 = a.wimg + a.fwd_off[1];  // layer 1's forward / W^T image; layer l's = + (l - 1) strides (GeoP)
  const char* wimg_b1 = a.wimg + a.bwd_off[1];
  auto make_job = [&](int k) -> DmaJob {
    if (k == L || k == L + 1) k = STATS ? 0 : L + 2;  // the head steps use the resident images: next in line is layer L's W^T
                                                      // (statistics instance: the next tile's first image)
    if constexpr (L0X) {  // the shared image of the step's layer (bias included: the next forward pass may find it resident), buffer (layer - 1) & 1
      const int layer = k < L ? k + 1 : 2 * L + 2 - k;
      const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(smem + ((layer - 1) & 1) * GP::WBSZ));
      return DmaJob{wimg_f1 + (unsigned)(layer - 1) * GP::FWD_STRIDE, (unsigned)lane16, dst, (G::IMG_HID + G::BIAS_HID + 3071) / 3072};
    }
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(smem + (k & 1) * GP::WBSZ));
    const char* img;
    int bytes;
    if constexpr (FILM && DW && !SPEC) {  // (the generic FiLM training instance has not one register for the two bases: 254 of 256, see DESIGN.md)
      if (k < L) { img = a.wimg + a.fwd_off[k + 1]; bytes = G::IMG_HID + G::BIAS_HID; }
      else { img = a.wimg + a.bwd_off[2 * L + 2 - k]; bytes = G::IMG_HID; }
    } else {
      if (k < L) { img = wimg_f1 + (unsigned)k * GP::FWD_STRIDE; bytes = G::IMG_HID + G::BIAS_HID; }
      else { img = wimg_b1 + (unsigned)(2 * L + 1 - k) * GP::BWD_STRIDE; bytes = G::IMG_HID; }
    }
    return DmaJob{img, (unsigned)lane16, dst, (bytes + 3071) / 3072};
  };
  auto issue_dma = [&](int k) {  // the whole image at once (small images, first tile)
    const DmaJob jb = make_job(k);
#pragma unroll
    for (int g = 0; g < DG; ++g) dma_group(jb, g, wave, NW);
  };
  issue_dma(0);
  {  // the head images, once
    const DmaJob jf{a.wimg + a.fwd_off[L + 1], (unsigned)lane16, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(size_t)HF), GP::HFSZ / 3072};
    const DmaJob jb{a.wimg + a.bwd_off[L + 1], (unsigned)lane16, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(size_t)HB), GP::HBSZ / 3072};
#pragma unroll
    for (int g = 0; g < DG; ++g) { dma_group(jf, g, wave, NW); dma_group(jb, g, wave, NW); }
  }
  dma_wait();

  // Training instance: workgroup g owns the CONTIGUOUS tiles [g n / G, (g + 1) n / G) -- consecutive tiles belong to
  // one image, so the image's layer-0 dA and loss sums stay on chip and leave once per image run (two launches of
  // per-tile partial reductions, 67 MB at config 2, are gone).  The other instances walk the tiles with stride G.
  // (FiLM: every instance owns a contiguous range -- its tables follow the image)
  constexpr bool CONTIG = DW || FILM;
  // (RENI_WEIGHT_SPARSE, strided walk only: positions in MainArgs::tlist instead of tiles -- tile_at() -- and its length instead of n_tiles)
  const int* const tlist = CONTIG ? nullptr : a.tlist;
  const int n_walk = (!CONTIG && tlist != nullptr) ? __builtin_amdgcn_readfirstlane(*a.tcount) : a.n_tiles;
  auto tile_at = [&](int i) -> int { return tlist != nullptr ? __builtin_amdgcn_readfirstlane(tlist[i]) : i; };
  const int t_first = CONTIG ? (int)((long long)blockIdx.x * a.n_tiles / gridDim.x) : (int)blockIdx.x * NHALF;
  const int t_stop = CONTIG ? (int)((long long)(blockIdx.x + 1) * a.n_tiles / gridDim.x) : n_walk;
  const int t_step = CONTIG ? NHALF : (int)gridDim.x * NHALF;
  if (!CONTIG && t_first >= t_stop) return;  // (the whole workgroup: nothing to visit -- fewer listed tiles than workgroups)
  int ft_img0 = -1, ft_img1 = -1;  // images whose FiLM tables are staged (half 0 / half 1)
  // A tile's first inputs -- the four layer-0 A operands of its image and this lane's direction -- are requested during the
  // PREVIOUS tile's dA phase (before the loop for the first): at the top of the tile their L2 round trip was exposed, ~900 cycles
  bf16x8 aop0_n[NRB];
  float d3_n[3];
  // Concat training instance: the tile's image and its position in the image are carried from tile to tile (the range is
  // contiguous, one tile per step) -- three integer divisions by a run-time value per tile (~30 instructions each) otherwise.
  constexpr bool INCR = DW && (!FILM || SPEC);  // (FiLM: its SPEC form has the two registers)
  int cur_b = 0, cur_tin = 0;  // image of tile0, tile0's index within it (INCR)
  if constexpr (INCR) { cur_b = t_first / a.tiles_per_image; cur_tin = t_first - cur_b * a.tiles_per_image; }
  int tile_pref = 0;  // (strided walk) the tile prefetch_tile looked up for the next iteration: the list is read once per tile, a tile ahead
  int p_pref = 0;     // (strided walk) and this lane's pixel in it (>= P: none)
  const int* const plist = CONTIG ? nullptr : a.plist;
  auto prefetch_tile = [&](int t0, int inc_b = -1, int inc_tin = 0) {
    const int tl = CONTIG ? (t0 + half < t_stop ? t0 + half : t_stop - 1) : tile_at(t0 + half < t_stop ? t0 + half : t_stop - 1);
    if constexpr (!CONTIG) tile_pref = tl;
    const int bi = (INCR && inc_b >= 0) ? inc_b : tl / a.tiles_per_image;
    int pi = ((INCR && inc_b >= 0) ? inc_tin : (tl - bi * a.tiles_per_image)) * 128 + wq * 32 + j;
    if constexpr (!CONTIG) {
      // (RENI_WEIGHT_COMPACT: `pi` is a POSITION among the image's pixels with weight; the pixel comes from MainArgs::plist.  Looked
      // up here, a tile ahead, and carried to the tile in p_pref / v_pref -- as the tile itself is)
      if (plist != nullptr) {
        const bool pv = pi < __builtin_amdgcn_readfirstlane(a.nlive[bi]);
        pi = pv ? plist[(size_t)bi * a.P + pi] : a.P;
      }
      p_pref = pi;
    }
    const float* dp = a.D + (size_t)bi * a.d_bstride + (size_t)((t0 + half < t_stop && pi < a.P) ? pi : 0) * 3;
#pragma unroll
    for (int rbo = 0; rbo < NRB; ++rbo) aop0_n[rbo] = *(const bf16x8*)(a.afrag + ((size_t)(bi * NRB + rbo) * 64) * 16 + (unsigned)(lane * 16));
    d3_n[0] = dp[0]; d3_n[1] = dp[1]; d3_n[2] = dp[2];
  };
  // (the generic FiLM training instance has no registers to carry them across the dA phase; its SPEC form has: 239 VGPRs with them)
  constexpr bool PREF = !(FILM && DW) || SPEC;
  if constexpr (PREF) prefetch_tile(t_first);
  // L0X: a tile's directions come through LDS -- every wave fetches ITS 32 samples' 384 bytes with one LDS-DMA instruction during the
  // previous tile's last step (no cross-wave dependency: the wave's own counted wait at the end of that tile covers it) and reads them
  // back at the top of the tile.  Three registers per lane carried across the last step's dW / dX stream instead made this instance
  // spill; loaded behind the stream they would be waited for with the g_1 stores in front of them.  (The region is the layer-0 dA
  // accumulator of the other instances; the ring kernel's preconditions -- whole tiles, 16-byte aligned direction rows -- hold.)
  char* const dnext = (char*)dAacc;
  auto dma_dirs = [&](int bi, int tin) {
    const char* src = (const char*)(a.D + (size_t)bi * a.d_bstride + (size_t)(tin * 128 + wq * 32) * 3);
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(dnext + wq * 384));
    if (lane < 24) glds16(src, (unsigned)lane16, dst);
  };
  // The tile's TARGET and WEIGHT rows come the same way (round 5, profiles/r05_l0ring.md: with them off the kernel ran 9.5 % faster.  They
  // were six strided dword loads per owner lane at the top of the tile, the OLDEST vector-memory operations in flight, so the first
  // vmcnt(0) of the forward pass -- for a weight image issued long after them -- waited out their trip to HBM, every tile).  Each
  // wave fetches its own 32 samples' rows of the NEXT tile at the start of the first backward step, a whole step ahead of the next
  // vmcnt(0), into a single buffer the loss of THIS tile has already left.  Layouts (launch_train checks; else round 4's kernels):
  // [P][3] interleaved rows (one 384-byte run per wave) or channel-planar [3][..P..] (three 128-byte runs), 16-byte aligned.
  char* const tnext = dnext + 1536;                                            // target rows (1536 B, in the dA region)
  char* const wnext = (char*)lacc + GP::LACC_BYTES;                            // weight rows (behind the per-lane accumulators)
  const bool t_planar = a.ts1 == 1, w_planar = a.ws1 == 1;
  auto dma_rows = [&](const float* base, long long s0, long long s2, bool planar, char* buf, int bi, int tin) {
    if (planar) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const char* src = (const char*)(base + (size_t)bi * s0 + (size_t)c * s2 + (size_t)(tin * 128 + wq * 32));
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(buf + (c * 128 + wq * 32) * 4));
        if (lane < 8) glds16(src, (unsigned)lane16, dst);
      }
    } else {
      const char* src = (const char*)(base + (size_t)bi * s0 + (size_t)(tin * 128 + wq * 32) * 3);
      const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(buf + wq * 384));
      if (lane < 24) glds16(src, (unsigned)lane16, dst);
    }
  };
  auto dma_tw = [&](int bi, int tin) {
    dma_rows(a.target, a.ts0, a.ts2, t_planar, tnext, bi, tin);
    dma_rows(a.weight, a.ws0, a.ws2, w_planar, wnext, bi, tin);
  };
  if constexpr (L0X) { dma_dirs(cur_b, cur_tin); dma_tw(cur_b, cur_tin); dma_wait(); }
#pragma unroll 1
  for (int tile0 = t_first; tile0 < t_stop; tile0 += t_step) {
    const bool last_tile = tile0 + t_step >= t_stop;
    asm volatile("" : "+v"(lane16), "+v"(tid16));
    // (L0X: the lane coordinates the LDS image addresses are formed from are opaque per tile as well -- hipcc otherwise hoists the
    // swizzled bases of the head step's and the backward steps' ts_write out of the tile loop, and in this instance, whose peak is a
    // few registers higher, spills them: 72 B of scratch, reloaded through the vector-memory path every tile)
    // (from the loop-carried lane16, itself opaque per tile: the kernel-wide j / hi, kept alive for this line alone, were spilled and
    // reloaded at the end of every tile)
    const int jx = L0X ? (int)(((unsigned)lane16 >> 4) & 31u) : j, hix = L0X ? (int)((unsigned)lane16 >> 9) : hi;
    const int j = jx, hi = hix;  // (shadow the kernel-wide coordinates for the whole tile body; the other instances: the same values)
    // (L0X: the lane the shared images' read bases are formed from -- wimg_cell, wimg_tr_base -- for the same reason)
    const int lanex = L0X ? (int)((unsigned)lane16 >> 4) : lane;
    TRACE(1);
    // this wave's tile; a half without one (odd tile count) runs on the last tile's addresses with everything masked
    const bool tvalid = tile0 + half < t_stop;
    const int tile = CONTIG ? (tvalid ? tile0 + half : t_stop - 1) : tile_pref;
    const int b = INCR ? cur_b : tile / a.tiles_per_image;
    // (INCR) the next tile's image / position: the tile behind the range's last is never used
    const bool wrap = cur_tin + 1 == a.tiles_per_image;
    const int nxt_b = wrap ? cur_b + 1 : cur_b, nxt_tin = wrap ? 0 : cur_tin + 1;
    if constexpr (FILM) {
      // stage the tables of the images this iteration works on (wave-uniform decision: every wave takes both barriers)
      const int i0 = INCR ? cur_b : tile0 / a.tiles_per_image;
      const int i1 = (tile0 + 1 < t_stop ? tile0 + 1 : t_stop - 1) / a.tiles_per_image;
      if (i0 != ft_img0 || (NHALF == 2 && i1 != ft_img1)) {
        __syncthreads();  // nobody reads the old tables any more
        int t0 = tid;  // (opaque here: the copy loops' trip counts are otherwise computed outside the tile loop and kept -- spilled -- for it)
        asm volatile("" : "+v"(t0));
        for (int hsel = 0; hsel < NHALF; ++hsel) {
          const int im = hsel == 0 ? i0 : i1;
          float* ft = ftab_base + hsel * FT_FLOATS;
#pragma unroll 1
          for (int i = t0; i < 2 * H; i += NW * 64) ft[i] = (i < H) ? 1.f : 0.f;  // slot 0: the folded first layer
          const float* src = a.film + (size_t)im * L * 2 * H;
#pragma unroll 1
          for (int i = t0; i < L * 2 * H; i += NW * 64) ft[2 * H + i] = src[i] * 0.15915494309189535f;
        }
        __syncthreads();
        ft_img0 = i0; ft_img1 = i1;
      }
    }
    // (the table's offset is opaque per tile: every table address is then formed where it is used -- hipcc otherwise hoists the
    // per-lane addresses of the unrolled steps' table reads out of the tile loop and spills them: ten registers with the paired loop,
    // each reloaded behind an s_waitcnt vmcnt(0) in the middle of a dX epilogue)
    unsigned ft_off = FILM ? (unsigned)(half * FT_FLOATS) : 0u;
    if constexpr (FILM) asm volatile("" : "+s"(ft_off));
    const float* const ftab = FILM ? ftab_base + ft_off : nullptr;
    const int p = CONTIG ? (INCR ? cur_tin : (tile - b * a.tiles_per_image)) * 128 + wq * 32 + j : p_pref;
    const bool valid = tvalid && p < a.P;
    // x = (dx, dy, dz, r, 1) as bf16 hi + lo parts.  Evaluated twice per tile (layer 0 forward, dA at the
    // end) rather than kept: nine registers for the length of the tile cost more than an L2-resident reload
    auto load_d = [&](float (&d3)[3]) {
      const float* dp = a.D + (size_t)b * a.d_bstride + (size_t)(valid ? p : 0) * 3;
      d3[0] = dp[0]; d3[1] = dp[1]; d3[2] = dp[2];
    };
    auto split_x = [&](const float (&d3)[3], __bf16 (&xh)[5], __bf16 (&xl)[4]) {
      float x[5];
      x[0] = d3[0]; x[1] = d3[1]; x[2] = d3[2];
      x[3] = sqrtf(x[0] * x[0] + x[2] * x[2]);
      x[4] = 1.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) xh[k] = (__bf16)x[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) xl[k] = (__bf16)(x[k] - (float)xh[k]);
    };
    bf16x8 aop0[NRB];  // layer-0 A operands of this image (prefetch_tile)
#pragma unroll
    for (int rbo = 0; rbo < NRB; ++rbo) {
      if constexpr (PREF) aop0[rbo] = aop0_n[rbo];
      else aop0[rbo] = *(const bf16x8*)(a.afrag + ((size_t)(b * NRB + rbo) * 64) * 16 + (unsigned)lane16);
    }
    // the direction is loaded AND consumed before the target / weight loads are issued: loads return in order and
    // hipcc joins the wait counts of the loss_kind branches to vmcnt(0), so a later use of D would wait out the
    // targets' HBM latency every tile (D and the A operands are L2 hits)
    bf16x8 bop0;  // layer-0 B operand: x = (dx, dy, dz, r, 1) as bf16 hi + lo parts
    {
      float d3[3] = {d3_n[0], d3_n[1], d3_n[2]};
      if constexpr (!PREF) load_d(d3);
      if constexpr (L0X) {  // (fetched by this wave's LDS-DMA during the previous tile's last step)
        typedef __attribute__((address_space(3))) float* lfp;  // (an explicit LDS address: as a generic pointer its 64-bit base was hoisted and spilled)
        const lfp dl = (lfp)(uintptr_t)(lds_u32(dnext) + (unsigned)((wq * 32 + j) * 12));
        d3[0] = dl[0]; d3[1] = dl[1]; d3[2] = dl[2];
      }
      __bf16 xh[5], xl[4];
      split_x(d3, xh, xl);
      if (hi == 0) { bop0[0] = xh[0]; bop0[1] = xh[1]; bop0[2] = xh[2]; bop0[3] = xh[3]; bop0[4] = xh[4]; bop0[5] = xh[0]; bop0[6] = xh[1]; bop0[7] = xh[2]; }
      else { bop0[0] = xh[3]; bop0[1] = xh[4]; bop0[2] = xl[0]; bop0[3] = xl[1]; bop0[4] = xl[2]; bop0[5] = xl[3]; bop0[6] = (__bf16)0.f; bop0[7] = (__bf16)0.f; }
    }
    asm volatile("" : "+v"(bop0) :: "memory");  // D is consumed (and waited for) before the target loads are issued
    const bool owner = valid && (hi == 0);
    float tgt[3] = {0.f, 0.f, 0.f}, swt[3] = {0.f, 0.f, 0.f};
    if (!L0X && owner && (!STATS || a.target != nullptr)) {  // target / weight: issued behind the first barrier (whose vmcnt(0) would expose
                             // them), consumed after the forward pass
      if (loss_kind == 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) tgt[c] = a.dout[((size_t)b * a.P + p) * 3 + c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tgt[c] = a.target[(size_t)b * a.ts0 + (size_t)p * a.ts1 + (size_t)c * a.ts2];
          swt[c] = a.weight[(size_t)b * a.ws0 + (size_t)p * a.ws1 + (size_t)c * a.ws2];
        }
      }
    }

    bf16x8 hb[NKS];       // current activations as MFMA B operands
    u32x4 wA[NRB * 2], wB[NRB * 2];  // the backward steps' phase arrays (declared here: the frozen instance fills wB during the last forward layer)
    constexpr bool KEEP1 = !STATS && !FILM;  // layer L - 1's phases stay in registers as well (the FiLM training instance has none to spare)
    u32x4 qst[NRB * 2];   // phases of the layer just computed; stored at the START of the next step so
                          // that the barrier after it never waits for these stores (vmcnt counts stores)

    // activation of one finished row block: keep the phase (for the stash) and the bf16 sin
    // sc < 0: the pre-activation already is the angle in revolutions (hidden layers: omega / 2 pi is folded
    // into the packed weight image and bias by k_pack, PackDesc::scale)
    // (FiLM: tp = the layer's table slot [freq / 2 pi | phase / 2 pi], angle = acc . freq + phase; nullptr = plain)
    auto red = [](float x) { if constexpr (!FILM) return x; else return __builtin_amdgcn_fractf(x); };  // (see the list above)
    // the same for elements 2q, 2q+1 only (hidden layers): fine-grained filler between another row block's MFMAs
    // FiLM: tp = the layer's table slot; the four (freq, phase) values of pairs q (even) and q + 1 are fetched at the even pair
    // (two ds_read_b128) and kept in `fs` for the odd one
    struct FilmQ { f32x4 fq, ph; };
    auto act_pair = [&](const f32x16& acc, int rb, int q, bf16x8 (&dst)[NKS], const float* tp = nullptr, FilmQ* fs = nullptr) {
      float v0 = acc[2 * q], v1 = acc[2 * q + 1];
      if constexpr (FILM) {
        if ((q & 1) == 0) {
          const float* f4 = tp + 32 * rb + 4 * q + 4 * hi;  // features of registers 2q .. 2q + 3 (rowmap): four consecutive
          fs->fq = *(const f32x4*)f4;
          fs->ph = *(const f32x4*)(f4 + H);
        }
        v0 = __builtin_fmaf(v0, fs->fq[2 * (q & 1)], fs->ph[2 * (q & 1)]);
        v1 = __builtin_fmaf(v1, fs->fq[2 * (q & 1) + 1], fs->ph[2 * (q & 1) + 1]);
      }
      const float t0 = red(v0), t1 = red(v1);
      // One volatile statement per pair (it keeps its place among the asm MFMAs): left to hipcc the packing converts sink to
      // one wait state in front of the MFMA that reads the operand (a VALU write needs two).  The phase pack sits between
      // the second sine and the operand pack: a transcendental's result needs one wait state before a VALU reads it.
      unsigned pk, s1, ph;
      asm volatile("v_sin_f32 %0, %3\n\tv_sin_f32 %1, %4\n\tv_cvt_pk_f16_f32 %2, %3, %4\n\tv_cvt_pk_bf16_f32 %0, %0, %1"
                   : "=&v"(pk), "=&v"(s1), "=&v"(ph) : "v"(t0), "v"(t1));
      u32x4 d4 = __builtin_bit_cast(u32x4, dst[2 * rb + (q >> 2)]);
      d4[q & 3] = pk;
      dst[2 * rb + (q >> 2)] = __builtin_bit_cast(bf16x8, d4);
      qst[2 * rb + (q >> 2)][q & 3] = ph;
    };
    // a whole finished row block (layer 0; the last layer's pending row blocks)
    auto activate = [&](const f32x16& acc, int rb, auto sc, bf16x8 (&dst)[NKS], const float* tp = nullptr) {
      if constexpr (!FILM) {  // eight pinned pair statements (left to hipcc: a single-value convert per sine and a v_perm per pair)
#pragma unroll
        for (int q = 0; q < 8; ++q) act_pair(acc, rb, q, dst);
        return;
      }
      float th[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[r];
        if constexpr (FILM) { if (tp != nullptr) { const int f = 32 * rb + rowmap(r, hi); v = __builtin_fmaf(v, tp[f], tp[H + f]); } }
        if constexpr (std::is_same<decltype(sc), float>::value) th[r] = red(v * sc);
        else th[r] = red(v);
        dst[2 * rb + (r >> 3)][r & 7] = (__bf16)__builtin_amdgcn_sinf(th[r]);
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d) qst[2 * rb + c][d] = phase_pack(th[8 * c + 2 * d], th[8 * c + 2 * d + 1]);
    };
    // stash layout of a layer: [wave][half-wave][chunk c][32 lanes] 16 B.  A lane's eight chunks are 512 B apart, so
    // every access is one per-layer address + an immediate (0..3584): no per-access address arithmetic and no
    // address registers (hipcc folds only non-negative immediates into global accesses)
    // A layer's slice of the stash is addressed as WAVE-UNIFORM base + one 32-bit lane offset (the scalar-base form of the
    // global instructions): no per-lane 64-bit address lives in registers across a GEMM.
    typedef __attribute__((address_space(1))) char gchar;      // (explicitly GLOBAL: the opaque scalar below hides the pointer's
    typedef __attribute__((address_space(1))) u32x4 gu32x4;    //  origin from hipcc, which would fall back to flat_ instructions)
    struct StashAt { gchar* base; unsigned off; };
    auto stash_mid = [&](int layer) -> StashAt {
      // = wave * 8192 + hi * 4096 + j * 16, derived from the per-tile opaque tid16 so that hipcc re-derives it at the point
      // of use (three VALU) instead of parking it in a register for the whole tile loop
      const unsigned off = ((unsigned)tid16 & 0x1f0u) | (((unsigned)tid16 >> 9) << 12);
      // (the layer's base as an opaque SCALAR: hipcc otherwise derives one layer's address from another's in 64-bit VALU
      // arithmetic -- two adds and a wait state in front of every store of the forward loop's second layer)
      unsigned long long base = (unsigned long long)(stash + (size_t)layer * stash_layer_stride);
      base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);  // (wave-uniform by construction; says so to hipcc)
      asm volatile("" : "+s"(base));
      return StashAt{(gchar*)base, off};
    };
    auto stash_chunk = [&](const StashAt& sa, int c) -> gu32x4* { return (gu32x4*)(sa.base + (size_t)(sa.off + (unsigned)(c * 512))); };

    // ---- layer 0 (per-image affine map, split-bf16 operands: see k_reni_main).  The A operands come ready-made
    // from k_prep_image (PrepArgs::afrag): four independent 16-byte loads issued at the top of the tile.  Built here
    // from A_b they were four dependent load -> convert -> MFMA rounds, each exposing a full memory latency.
    // The pre-activations of row blocks 2 and 3 of a layer stay PENDING (pa, pb) and are activated as fillers
    // between the first MFMAs of the NEXT layer's GEMM, which only need row blocks 0 and 1 (k-steps 0..3) -- instead of
    // as a VALU-only tail behind the layer while the matrix pipe idles.
    f32x16 pa, pb;
    {
#pragma unroll
      for (int rbo = 0; rbo < NRB; ++rbo) {
        f32x16 acc;
        mfma_bf16_zero_v<true>(acc, aop0[rbo], bop0);
        if (rbo == 2) pa = acc;
        else if (rbo == 3) pb = acc;
        else activate(acc, rbo, std::true_type{}, hb);  // (omega_0 / 2 pi is folded into the A operands: PrepArgs::afrag_scale)
      }
    }

    TRACE(2);
    // ---- hidden layers (step k = l - 1).  One layer = fwd_layer(l, hin -> hout, pending in -> pending out); the loop runs
    // two layers per iteration with the arrays' roles exchanged, so that nothing loop-carried is copied (35 v_mov per layer
    // otherwise: hipcc cannot rename registers across a back edge).
    auto fwd_layer = [&](int l, bf16x8 (&hin)[NKS], bf16x8 (&hout)[NKS], f32x16& pia, f32x16& pib, f32x16& poa, f32x16& pob) {
      if (l == 1) {
        // image 0 was fetched during the previous tile's last step and every wave has since waited for it (dma_wait
        // in the dA phase; before the loop for the first tile).  No dma_wait here: its vmcnt(0) would also wait out
        // this tile's target / weight loads, issued a moment ago -- a full HBM latency per tile
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      } else {
        dma_wait();
        __syncthreads();  // image of this step landed; the other buffer is free
      }
      TRACE(10 + l);
      DmaJob jb = make_job(l);  // next step's image: one group per k-step of the first GEMM below
      // (L0X, shared images: layer L's is still in its buffer at the first backward step; layer 2's is there from the previous tile's
      // last step -- in every tile of the range but the first)
      if (L0X && (l == L || (l == 1 && tile0 != t_first))) jb.ng = 0;
      // statistics instance, last layer: the next image is the next tile's first, into buffer 0 -- which this very layer
      // reads when L is odd (then it is issued behind a barrier after the GEMMs, below)
      if (STATS && l == L && ((L & 1) || last_tile)) jb.ng = 0;
      const StashAt sl_prev = stash_mid(l - 1);
      const float* const tp_prev = FILM ? ftab + (l - 1) * 2 * H : nullptr;  // FiLM table slots of the layer below / this layer
      const float* const tp_cur = FILM ? ftab + l * 2 * H : nullptr;
      FilmQ fs0, fsA, fsB;
      // fillers of the first GEMM (rows 0..63): behind the MFMAs of k-steps 0..3 (they read only row blocks 0 and 1 of the
      // layer below) the PENDING row blocks 2 and 3 of the layer below are activated, two pairs per MFMA; the layer
      // below's eight phase chunks go to the stash one per k-step.
      const char* wb = smem + ((l - 1) & 1) * GP::WBSZ;
      const float* bias = (const float*)(wb + G::IMG_HID);
      auto fill = [&](int ks, int part) {
        if (part == 0 && ks < DG) dma_group(jb, ks, wave, NW);
        // the bias values the second GEMM's accumulators start from are requested here (two quads per k-step once the pending
        // row blocks are done): loaded between the GEMMs, their LDS round trip stood in front of the second GEMM's first MFMA
        constexpr bool SPREAD = !FILM || SPEC;  // (FiLM: the SPEC instance has the registers for the two live table quads)
        if constexpr (SPREAD) {
          // The sixteen pending pairs spread over twelve MFMA slots instead of packed into the first eight (four pairs = 16 VALU
          // behind every MFMA pair there, nothing behind the last eight: the first half of the GEMM was VALU-bound, the second idle).
          // Row block 2 (k-steps 4, 5 read it) must be complete before slot 8, row block 3 (k-steps 6, 7) before slot 12:
          //   slot s < 8: pair s of row block 2, and on even s pair s / 2 of row block 3;  slots 8..11: pairs 4..7 of row block 3.
          // The second GEMM's bias values follow in slots 12..15, when the pending registers are free.
          const int sl = 2 * ks + part;
          // (FiLM: an even pair fetches the table entries it shares with the odd pair behind it -- one live quad per row block)
          if (sl < 8) act_pair(pia, 2, sl, hin, tp_prev, &fsA);
          if (sl < 8 && (sl & 1) == 0) act_pair(pib, 3, sl >> 1, hin, tp_prev, &fsB);
          if (sl >= 8 && sl < 12) act_pair(pib, 3, sl - 4, hin, tp_prev, &fsB);
          if (sl >= 12) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              if (sl < 14) poa[8 * (sl - 12) + r] = bias[64 + rowmap(8 * (sl - 12) + r, hi)];
              else pob[8 * (sl - 14) + r] = bias[96 + rowmap(8 * (sl - 14) + r, hi)];
            }
          }
        } else {
        if (part == 1 && ks >= 4) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            if (ks < 6) poa[8 * (ks - 4) + r] = bias[64 + rowmap(8 * (ks - 4) + r, hi)];
            else pob[8 * (ks - 6) + r] = bias[96 + rowmap(8 * (ks - 6) + r, hi)];
          }
        }
        if (ks < 4) {
          FilmQ fs;
          if (part == 0) { act_pair(pia, 2, 2 * ks, hin, tp_prev, &fs); act_pair(pia, 2, 2 * ks + 1, hin, tp_prev, &fs); }
          else { act_pair(pib, 3, 2 * ks, hin, tp_prev, &fs); act_pair(pib, 3, 2 * ks + 1, hin, tp_prev, &fs); }
        }
        }
        if constexpr (!STATS) {
          if constexpr (KEEP1) {  // (frozen instance: layer L - 1's phases stay in registers; layer 0's are rebuilt in backward)
            if (part == 1) {
              if (l == L) wB[ks] = qst[ks];
              else if (!(l == 1 && L >= 2)) *stash_chunk(sl_prev, ks) = qst[ks];
            }
          } else if constexpr (!FILM) { if (part == 1 && !(l == 1 && L >= 2)) *stash_chunk(sl_prev, ks) = qst[ks]; }  // (layer 0: rebuilt in backward)
          else { if (part == 1) *stash_chunk(sl_prev, ks) = qst[ks]; }
        }
      };
      // rows 0..63, then rows 64..127 with the activation of rows 0..63 (sine, phase packing) issued between
      // its MFMAs: VALU work in the shadow of the matrix pipe instead of after it
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc0[r] = bias[rowmap(r, hi)];
        acc1[r] = bias[32 + rowmap(r, hi)];
      }
      TRACE(100 + l);
      gemm_rb2<NKS, std::decay_t<decltype(fill)>, false, L0X>(wb, 0, hin, acc0, acc1, lanex, fill);
      TRACE(110 + l);
      auto fill2 = [&](int ks, int part) {
        if constexpr (FILM) {  // the two pairs that share one table fetch sit in consecutive slots (one live FilmQ, not two)
          if ((ks & 1) == 0) act_pair(acc0, 0, ks + part, hout, tp_cur, &fs0);
          else act_pair(acc1, 1, ks - 1 + part, hout, tp_cur, &fs0);
        } else {
          if (part == 0) act_pair(acc0, 0, ks, hout); else act_pair(acc1, 1, ks, hout);
        }
      };
      gemm_rb2<NKS, decltype(fill2), false, L0X>(wb, 2, hin, poa, pob, lanex, fill2);
      TRACE(120 + l);
      if (STATS && l == L && (L & 1) && !last_tile) {
        __syncthreads();  // every wave is done reading buffer 0
        issue_dma(0);
      }
    };
    {
      bf16x8 hb2[NKS];
      f32x16 pa2, pb2;
      int l = 1;
#pragma unroll 1
      for (; l + 1 <= L; l += 2) {
        fwd_layer(l, hb, hb2, pa, pb, pa2, pb2);
        fwd_layer(l + 1, hb2, hb, pa2, pb2, pa, pb);
      }
      if (l == L) {  // odd layer count: the last layer ends in the second set
        fwd_layer(L, hb, hb2, pa, pb, pa2, pb2);
        pa = pa2; pb = pb2;
#pragma unroll
        for (int ks = 0; ks < NKS / 2; ++ks) hb[ks] = hb2[ks];
      }
    }
    {  // the last hidden layer's pending row blocks (the head needs all of h_L)
      activate(pa, 2, std::true_type{}, hb, FILM ? ftab + L * 2 * H : nullptr);
      activate(pb, 3, std::true_type{}, hb, FILM ? ftab + L * 2 * H : nullptr);
      // the packed operands exist HERE (hipcc otherwise sinks the packing converts to one wait state in front of the asm
      // MFMA that reads them -- a VALU write needs two) and the pad is part of the statement
      asm volatile("s_nop 1" : "+v"(hb[4]), "+v"(hb[5]), "+v"(hb[6]), "+v"(hb[7]));
    }

    TRACE(3);
    // ---- head (step L)
    float ylin[3], outv[3];
    {  // (no barrier: the operand is in registers and the head image is resident)
      TRACE(4);
      const char* wb = HF;
      const float* bias = (const float*)(wb + G::IMG_HF);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bias[rowmap(r, hi)];
      acc = gemm_rb<NKS>(wb, 0, hb, acc, lanex);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ylin[c] = acc[c];
        const float yv = last_linear ? ylin[c] : sin_f32(a.w_hidden * ylin[c]);
        // tanh(y) = 1 - 2 / (exp(2y) + 1) on the hardware exp2 / rcp (abs error ~1e-6, far inside bf16's)
        const float y2 = yv * 2.885390081777927f;
        const float e2 = __builtin_amdgcn_exp2f(y2 > 60.f ? 60.f : y2);  // (a compare-and-select, not fminf: a NaN must stay a NaN --
                                                                         //  reni_forward_loss_backward_rows poisons a bad index with it)
        outv[c] = (act == 1) ? (1.f - 2.f * __builtin_amdgcn_rcpf(e2 + 1.f)) : (act == 2) ? expf(yv) : yv;
      }
    }
    if (out_img != nullptr && owner) {
      float* op = out_img + ((size_t)b * a.P + p) * 3;
      op[0] = outv[0]; op[1] = outv[1]; op[2] = outv[2];
    }

    TRACE(5);
    if constexpr (STATS) {
      if (a.target != nullptr) {  // (NULL: plain inference, the outputs above are all there is)
        float s9[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = owner ? tgt[c] : 0.f, o = owner ? outv[c] : 0.f;
          s9[c] = o * t; s9[3 + c] = o * o; s9[6 + c] = t * t;
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const float sq = wave_sum(s9[q]);
          if (lane == 0 && tvalid) a.loss_part[((size_t)tile * 4 + wq) * 16 + 1 + q] = sq;
        }
      }
      dma_wait();  // the next tile's first image: its barrier has no vmcnt
      if constexpr (PREF) prefetch_tile(tile0 + t_step);
      continue;
    }
    if constexpr (L0X) {  // this tile's target / weight rows: fetched by this wave's LDS-DMA a tile ago (dma_tw)
      typedef __attribute__((address_space(3))) float* lfp;
      const int sl = wq * 32 + j;
      const unsigned to = lds_u32(tnext) + (unsigned)(t_planar ? sl * 4 : sl * 12), ts = t_planar ? 512u : 4u;
      const unsigned wo = lds_u32(wnext) + (unsigned)(w_planar ? sl * 4 : sl * 12), wsx = w_planar ? 512u : 4u;
      if (owner) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tgt[c] = *(lfp)(uintptr_t)(to + (unsigned)c * ts);
          swt[c] = *(lfp)(uintptr_t)(wo + (unsigned)c * wsx);
        }
      }
    }
    // ---- loss and d loss / d out
    float gy[3] = {0.f, 0.f, 0.f};
    {
      float e = 0.f;
      if (loss_kind == 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gy[c] = tgt[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (owner) {
            const float t = tgt[c], sw = swt[c];
            const float d = outv[c] - t;
            e += sw * d * d;
            gy[c] = 2.f * sw * d * inv3p;
            if (loss_kind == 1) {
              const float cA = a.stats[(size_t)b * 16 + c], cB = a.stats[(size_t)b * 16 + 4 + c];
              gy[c] += cA * t - cB * outv[c];
            }
          }
        }
      }
      if constexpr (!LACC) {
        const float es = wave_sum(e);
        if constexpr (DW) { if (lane == 0) loss_run[wave] += es; }
        else if (lane == 0 && tvalid) a.loss_part[((size_t)tile * 4 + wq) * 16] = es;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (act == 1) gy[c] *= (1.f - outv[c] * outv[c]);
        else if (act == 2) gy[c] *= outv[c];
        if (!last_linear) gy[c] *= a.w_hidden * cos_f32(a.w_hidden * ylin[c]);
        if (!owner) gy[c] = 0.f;
        if constexpr (!FILM) gy[c] *= a.gy_scale;  // (the W^T images are 8 x the forward images: MainArgs::gy_scale; 1 where they are not)
      }
      if constexpr (LACC) {  // (loss, g_y) into this lane's slot: reduced across lanes once per image run / once per launch
        if (hi == 0) {
          f32x4 v = lacc[wave * 32 + jx];
          v[0] += e; v[1] += gy[0]; v[2] += gy[1]; v[3] += gy[2];
          lacc[wave * 32 + jx] = v;
        }
      }
    }

    TRACE(6);
    // =============================== backward ===============================
    // gradient w.r.t. a layer's pre-activation (g_a), packed: a step reads one array (B operand of its GEMMs) and
    // writes the layer below's into the other; the roles alternate, so nothing is copied between steps
    bf16x8 gA[NKS], gB[NKS];
    // two row blocks of a dX GEMM with the activation derivative of the layer below applied to the fp32 result:
    // ghb = (W^T g) * cos(phase) = the gradient w.r.t. that layer's pre-activation, packed once (only two fp32
    // accumulator tiles are ever live; packing g_h to bf16 and unpacking it again for the product in a separate pass
    // cost 1.5 instructions per value)
    // (FiLM: tq = table slot of the layer whose phases w holds; the result is g_a = freq . cos(theta) . g_h -- the W^T images
    // carry the 2 pi that turns the table's freq / 2 pi into freq)
    auto dx_rowblock_g = [&](const char* wb, int rbi, auto& bop, auto nks_tag, const auto& fill, const u32x4 (&w)[NRB * 2], bf16x8 (&ghb)[NKS],
                             const float* tq = nullptr) {
      constexpr int NK = decltype(nks_tag)::value;
      f32x16 acc0, acc1;
      gemm_rb2<NK, std::decay_t<decltype(fill)>, true>(wb, rbi, bop, acc0, acc1, lanex, fill);
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float r0, r1;
        cos_mul2(w[2 * rbi + (r >> 3)][(r & 7) >> 1], acc0[r], acc0[r + 1], r0, r1);
        if constexpr (FILM) { const int f = 32 * rbi + rowmap(r, hi); r0 *= tq[f]; r1 *= tq[f + 1]; }
        ghb[2 * rbi + (r >> 3)][r & 7] = (__bf16)r0;
        ghb[2 * rbi + (r >> 3)][(r & 7) + 1] = (__bf16)r1;
        cos_mul2(w[2 * rbi + 2 + (r >> 3)][(r & 7) >> 1], acc1[r], acc1[r + 1], r0, r1);
        if constexpr (FILM) { const int f = 32 * (rbi + 1) + rowmap(r, hi); r0 *= tq[f]; r1 *= tq[f + 1]; }
        ghb[2 * rbi + 2 + (r >> 3)][r & 7] = (__bf16)r0;
        ghb[2 * rbi + 2 + (r >> 3)][(r & 7) + 1] = (__bf16)r1;
      }
    };
    // all four row blocks of a hidden layer's dX GEMM; fillv(rb, ks) = the step's vector-memory fillers
    auto epi_pair = [&](const f32x16& acc, int rb, int q, const u32x4 (&w)[NRB * 2], bf16x8 (&ghb)[NKS], const float* tq, f32x4& fq4) {
      const int r = 2 * q;
      if constexpr (!FILM) {
        u32x4 d4 = __builtin_bit_cast(u32x4, ghb[2 * rb + (r >> 3)]);
        d4[(r & 7) >> 1] = cos_mul2_pk(w[2 * rb + (r >> 3)][(r & 7) >> 1], acc[r], acc[r + 1]);
        ghb[2 * rb + (r >> 3)] = __builtin_bit_cast(bf16x8, d4);
        return;
      }
      float r0, r1;
      cos_mul2(w[2 * rb + (r >> 3)][(r & 7) >> 1], acc[r], acc[r + 1], r0, r1);
      if constexpr (FILM) {  // (the four frequencies of pairs q (even) and q + 1: one ds_read_b128 at the even pair)
        if ((q & 1) == 0) fq4 = *(const f32x4*)(tq + 32 * rb + 4 * q + 4 * hi);
        r0 *= fq4[2 * (q & 1)];
        r1 *= fq4[2 * (q & 1) + 1];
      }
      ghb[2 * rb + (r >> 3)][r & 7] = (__bf16)r0;
      ghb[2 * rb + (r >> 3)][(r & 7) + 1] = (__bf16)r1;
    };
    auto dx_layer = [&](const char* wb, const bf16x8 (&bop)[NKS], const auto& fillv, const u32x4 (&w)[NRB * 2], bf16x8 (&ghb)[NKS],
                        const float* tq = nullptr, int ltag = 0) {
      f32x16 a0, a1, a2, a3;
      f32x4 fq4;
      auto f0 = [&](int ks) { fillv(0, ks); };
      gemm_rb1<NKS, decltype(f0), true>(wb, 0, bop, a0, lane, f0);
      TRACE(200 + 10 * ltag);
      auto f1 = [&](int ks) { epi_pair(a0, 0, ks, w, ghb, tq, fq4); fillv(1, ks); };
      gemm_rb1<NKS, decltype(f1), true>(wb, 1, bop, a1, lane, f1);
      TRACE(201 + 10 * ltag);
      auto f2 = [&](int ks) { epi_pair(a1, 1, ks, w, ghb, tq, fq4); fillv(2, ks); };
      gemm_rb1<NKS, decltype(f2), true>(wb, 2, bop, a2, lane, f2);
      TRACE(202 + 10 * ltag);
      auto f3 = [&](int ks) { epi_pair(a2, 2, ks, w, ghb, tq, fq4); fillv(3, ks); };
      gemm_rb1<NKS, decltype(f3), true>(wb, 3, bop, a3, lane, f3);
      TRACE(203 + 10 * ltag);
#pragma unroll
      for (int q = 0; q < 8; ++q) epi_pair(a3, 3, q, w, ghb, tq, fq4);
      TRACE(204 + 10 * ltag);
    };
    // dwdx_layer: the dW GEMM of a step (K = samples, operands from the transposition images, this wave's strip of dW_l in AGPR tiles
    // BASE .. BASE + 3) and its dX GEMM (K = features, A from the W^T image, four single chains with the cos epilogue) depend on
    // nothing of each other -- both start from what the step's second barrier published -- but a lone wave runs them one after
    // the other: the dW GEMM LDS-bound with the VALU idle (ten transposing reads per four MFMAs), the dX GEMM VALU-bound with the
    // LDS idle (cycle trace: 2150 + 2700 cycles for 2 x 1075 cycles of MFMA).  Here they are ONE stream, MFMA by MFMA: slot i issues
    // dX's MFMA (row block i / 8, k-step i % 8) and dW's MFMA (k-step i / 4, column block i % 4); behind them the epilogue pair of
    // the previous row block, the transposing reads of the next dW k-step (B fragment m is re-requested right behind its only use,
    // the A fragment is double-buffered) and one W^T fragment three slots ahead.
    // (L0X, layer 2's stream -- BASE == 0, the tile's last: its epilogue's results are g_1, and the g_1 stream's stores leave from
    // HERE, one behind the slot that completes its chunk (chunk c is final after slot 11 + 4 c; the last three behind the last row
    // block's epilogue).  Eight stores in a row at the end of the tile filled the vector-memory queue, and the next tile's first loads --
    // target, weight -- stalled the wave's issue behind them: cycle trace, +1.2 k cycles at the top of every tile.)
    auto dwdx_layer = [&](auto base_tag, const char* wb, const bf16x8 (&bop)[NKS], const DmaJob& jb, const u32x4 (&w)[NRB * 2],
                          bf16x8 (&ghb)[NKS], const float* tq, float& dbacc) {
      constexpr int BASE = decltype(base_tag)::value;
      constexpr bool G1ST = L0X && BASE == 0;
      // layout: [tile within the workgroup's range][workgroup][8 chunks x 4 KB], cells swizzled (kernel header).  The base is an opaque
      // SCALAR and the lane's cell is re-derived from tid16 at every store (hi = bit 9 of tid16): nothing per-lane lives across the stream
      unsigned long long g1b = 0;
      if constexpr (G1ST) {
        g1b = (unsigned long long)(a.g1 + ((size_t)(tile - t_first) * gridDim.x + blockIdx.x) * (NKS * 4096));
        g1b = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(g1b >> 32)) << 32) |
              (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)g1b);
        asm volatile("" : "+s"(g1b));
      }
      auto g1_store = [&](int c) {
        // (an asm store in the scalar-base + 32-bit-offset form, its offset formed HERE from an opaque copy of tid16: left to hipcc the
        // eight 64-bit per-lane offsets were computed at the top of the tile and carried -- spilled -- across the stream)
        unsigned t = (unsigned)tid16;
        asm volatile("" : "+v"(t));
        const unsigned off = ((t ^ ((t >> 3) & 64u)) ^ (unsigned)((c & 1) << 7)) + (unsigned)(c * 4096);
        asm volatile("global_store_dwordx4 %0, %1, %2" :: "v"(off), "v"(ghb[c]), "s"(g1b) : "memory");
      };
      // (L0X: TB lies TSZ bytes behind TA, so its fragments are read from TA's bases with one more immediate -- the two registers of
      // bases of its own are the ones the shared image's second read base takes: rdB, xq1)
      const TsBase bA = ts_base(TA, lanex), bB = L0X ? bA : ts_base(TB, lanex);
      auto rdB = [&](int m, int ks) { return L0X ? ts_read(bA, m, ks, (unsigned)GP::TSZ) : ts_read(bB, m, ks); };
      // (L0X: the A operand of the dX GEMM is fragment (row block i >> 3, k-step i & 7) of W_l^T read out of the layer's SHARED image --
      // two transposing reads, every address one base made here plus immediates: wimg_tr_base)
      unsigned xq = 0, xq1 = 0;
      if constexpr (L0X) {
        xq = lds_u32(wb) + wimg_tr_base(lanex);
        xq1 = xq ^ 0x80u;  // (the second read's base: per fragment it was 32 more VALU instructions per step)
        asm volatile("" : "+v"(xq), "+v"(xq1));  // (keeps the bases out of the tile loop's invariants: see ts_write)
      }
      auto fx = [&](int i) {
        if constexpr (L0X) {
          typedef __attribute__((address_space(3))) s16x4* lp;
          typedef short s16x8 __attribute__((ext_vector_type(8)));
          const unsigned off = (unsigned)((i >> 3) * 2048 + ((i & 7) >> 1) * 8192 + (i & 1) * 256);
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(xq + off));
          const s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(xq1 + off));
          const s16x8 v = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
          return __builtin_bit_cast(bf16x8, v);
        } else {
          return *(const bf16x8*)(wb + (((i >> 3) * NKS + (i & 7)) * 64 + lane) * 16);
        }
      };
      constexpr int D = 2;  // (W^T fragments in flight: two slots = four MFMAs ahead; a third set is four registers the kernel does not have)
      bf16x8 q[D];
#pragma unroll
      for (int d = 0; d < D; ++d) q[d] = fx(d);
      bf16x8 fa = ts_read(bA, wave, 0), fan = fa, fb0 = rdB(0, 0), fb1 = rdB(1, 0), fb2 = rdB(2, 0), fb3 = rdB(3, 0);
      f32x16 a0, a1, a2, a3;
      f32x4 fq4;
      auto slot = [&](auto ic, f32x16& acc, const f32x16& accp) {
        constexpr int i = decltype(ic)::value, rb = i >> 3, ks = i & 7, kk = i >> 2, m = i & 3;
        const bf16x8 ax = q[i % D];
        if (i + D < 32) q[i % D] = fx(i + D);
        if (ks == 0) mfma_bf16_zero_v<false>(acc, ax, bop[ks]);
        else if (ks == 7) mfma_bf16_pin_v<true, false, TAIL_DWDX>(acc, ax, bop[ks]);
        else mfma_bf16_pin_v<false, false>(acc, ax, bop[ks]);
        if constexpr (rb >= 1) epi_pair(accp, rb - 1, ks, w, ghb, tq, fq4);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 bx = m == 0 ? fb0 : m == 1 ? fb1 : m == 2 ? fb2 : fb3;
        if (i == 31) mfma_bf16_agpr_tile<BASE + m, true, TAIL_DWDX_A>(fa, bx);
        else mfma_bf16_agpr_tile<BASE + m, false>(fa, bx);
        if constexpr (kk < 7) {  // the next k-step's fragments: B fragment m behind its use, the A fragment behind the k-step's first MFMA
          if (m == 0) { fb0 = rdB(0, kk + 1); fan = ts_read(bA, wave, kk + 1); }
          else if (m == 1) fb1 = rdB(1, kk + 1);
          else if (m == 2) fb2 = rdB(2, kk + 1);
          else fb3 = rdB(3, kk + 1);
        }
        if constexpr (m == 3) { dbacc = frag_sum<PolBF16>(fa, dbacc); fa = fan; }  // (bias-gradient sums of the k-step)
        if constexpr (i % 4 == 2 && i / 4 < DG) dma_group(jb, i / 4, wave, NW);  // next step's image, one group per dW k-step
        if constexpr (G1ST && i >= 12 && i % 4 == 0) g1_store((i - 12) / 4);     // (chunks 0..4 behind slots 12, 16, .. 28)
        __builtin_amdgcn_sched_barrier(0);
      };
      static_for_up<0, 8>([&](auto ic) { slot(ic, a0, a0); });
      static_for_up<8, 16>([&](auto ic) { slot(ic, a1, a0); });
      static_for_up<16, 24>([&](auto ic) { slot(ic, a2, a1); });
      static_for_up<24, 32>([&](auto ic) { slot(ic, a3, a2); });
      if constexpr (G1ST) g1_store(5);
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) epi_pair(a3, 3, qq, w, ghb, tq, fq4);
      if constexpr (G1ST) { g1_store(6); g1_store(7); }
    };
    // one layer of the phase stash
    auto load_phases = [&](const StashAt& sl, u32x4 (&w)[NRB * 2]) {  // all loads in flight together
#pragma unroll
      for (int c = 0; c < NRB * 2; ++c) {
        w[c] = *stash_chunk(sl, c);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // (the factor omega of d sin(omega a) / da is folded into the W^T image that produces g_h: PackDesc::scale)
    // phases: wA / wB alternate like gA / gB.  A step uses the phases of the layer below its own (the dX epilogue's
    // cosine, the dW operand's sine); they are fetched from the stash ONE STEP AHEAD into the other array (training
    // instance: after the dW GEMM, whose registers are free again; frozen instance: right behind the step's barrier),
    // so no step waits for the stash (-1.8 % / essential for the frozen instance, which has nothing to hide it behind).
    // The last layer's phases are taken straight from the forward pass's registers (qst).
#pragma unroll
    for (int c = 0; c < NRB * 2; ++c) wA[c] = qst[c];
    // ---- head (step L+1): dW_out += h_L g_y^T ; g_h = W_out^T g_y
    {
      bf16x8 gyb[2];
#pragma unroll
      for (int e = 0; e < 8; ++e) { gyb[0][e] = (__bf16)((e < 3) ? gy[e] : 0.f); gyb[1][e] = (__bf16)0.f; }
      // (TA / TB are free: the previous tile's dA GEMM, their last reader, lies behind the forward pass's barriers)
      if constexpr (DW) {
        // db_out = sum over samples of g_y: every wave sums its own 32 samples (fp32, straight from the registers) into its own
        // slot -- through the operand image it was thirty-two v_dot2c on wave 0, a cross-half shuffle and an LDS round trip
        if constexpr (!LACC) {
          const float s0 = wave_sum(gy[0]), s1 = wave_sum(gy[1]), s2 = wave_sum(gy[2]);
          if (lane == 0) {  // (one read and one write of the wave's own slot)
            f32x4 o = *(f32x4*)(hdb + 4 * wave);
            o[0] += s0; o[1] += s1; o[2] += s2;
            *(f32x4*)(hdb + 4 * wave) = o;
          }
        }
        ts_write<NRB>(TA, hb, wq * 32 + jx, hix);
        if constexpr (L0X) {  // (the three constant pieces from a zero made HERE: hipcc otherwise keeps -- in this instance: spills -- zero pairs for the whole kernel)
          const unsigned gbase = ts_write_base(TB, wq * 32 + jx, hix);
          u32x2 zz;
          asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0" : "=v"(zz[0]), "=v"(zz[1]));
          const u32x4 w0 = __builtin_bit_cast(u32x4, gyb[0]);
          *(lds_u32x2_p)(uintptr_t)(gbase) = u32x2{w0[0], w0[1]};
          *(lds_u32x2_p)(uintptr_t)(gbase ^ 16u) = zz;
          *(lds_u32x2_p)(uintptr_t)(gbase ^ 32u) = zz;
          *(lds_u32x2_p)(uintptr_t)(gbase ^ 48u) = zz;
        } else
        ts_write<1>(TB, gyb, wq * 32 + jx, hix);
      }
      dma_wait();  // the stash stores of the forward pass are complete before the first read-back below
      if constexpr (DW) __syncthreads();  // the operand images are complete (frozen instance: nothing is shared here)
      TRACE(7);
      if constexpr (!KEEP1) load_phases(stash_mid(L - 1), wB);  // for step L (KEEP1: wB already holds them)
      if constexpr (DW) {
        f32x16 ah[1];
        float dbh = 0.f;
        TRACE(91);
        // (L0X: from the per-tile opaque lane16 -- the pre-swizzle bases of this GEMM's transposing reads, or `lane` itself, were kept
        // across the tile loop in a scratch slot and reloaded every tile)
        const int lane_h = L0X ? (int)((unsigned)lane16 >> 4) : lane;
        dw_gemm_s<1, DW_L0, 2>(TA, TB, ah, dbh, wave, lane_h);  // (DW_L0: no bias sum from the operand image, see below)
        TRACE(92);
        if (j < 3) {  // element (c = j, feature) is owned by exactly one lane of one wave: plain LDS += (all reads, then all writes)
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) old[r] = hdw[j * H + 32 * wave + rowmap(r, hi)];
#pragma unroll
          for (int r = 0; r < 16; ++r) hdw[j * H + 32 * wave + rowmap(r, hi)] = old[r] + ah[0][r];
        }

        TRACE(93);
      }
      const char* wb = HB;
      const bf16x8 g1[1] = {gyb[0]};
#pragma unroll
      for (int rbi = 0; rbi < NRB; rbi += 2)
        dx_rowblock_g(wb, rbi, g1, std::integral_constant<int, 1>{}, NoFill{}, wA, gA, FILM ? ftab + L * 2 * H : nullptr);
    }
    // ---- hidden layers l = L..1 (step k = 2L+2-l)
    // gb = g_l, the gradient w.r.t. layer l's pre-activation, is ready at the top of step l: the dX GEMM of the step
    // above applied cos(phase_l) in its epilogue (dx_rowblock_g).  phase_{l-1} is read from the stash once per step and
    // serves h_{l-1} = sin (the dW column operand) and that epilogue's cosine.
    float dre[3] = {0.f, 0.f, 0.f};
    // gb = g_l in, ghb = g_{l-1} out; wph = phases(l-1) (fetched during the previous step), wnx <- phases(l-2)
    // (L0X: the tile's LAST step is layer 2's.  Instead of the layer below's phases it fetches the NEXT tile's first inputs -- its
    // image's layer-0 A operands through the same eight loads, its directions by LDS-DMA -- and the image it requests is the next
    // tile's first.  All of it selected at run time without a compiler-visible vector-memory operation behind a condition.)
    auto step = [&](int l, bf16x8 (&gb)[NKS], bf16x8 (&ghb)[NKS], u32x4 (&wph)[NRB * 2], u32x4 (&wnx)[NRB * 2]) {
      const bool LASTSTEP = L0X && l == 2;
      const int k = 2 * L + 2 - l;
      TRACE(20 + l);
      if constexpr (!FILM && !STATS && !L0X) {
        if (l == 1 && L >= 2) {  // wph[2r] = the image's layer-0 A operand r (fetched during step 2): rebuild layer 0's phase words
          const bf16x8 bop = bop0;  // (the tile's layer-0 B operand stays alive: four registers, against a reload + re-split of D)
#pragma unroll
          for (int rbo = 0; rbo < NRB; ++rbo) {  // row block r's words land in wph[2r], wph[2r + 1]
            f32x16 acc;
            mfma_bf16_zero_v<true>(acc, __builtin_bit_cast(bf16x8, wph[2 * rbo]), bop);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              u32x4 w;
#pragma unroll
              for (int d = 0; d < 4; ++d)
                w[d] = phase_pack(red(acc[8 * c + 2 * d]), red(acc[8 * c + 2 * d + 1]));
              wph[2 * rbo + c] = w;
            }
          }
        }
      }
      if (DW && FILM && l == 1) {  // the sixteen AGPR tiles hold dW_2..dW_5; dW_1 = sum g_1 h_0^T is finished by k_reni_dw1 (concat: fillv below)
        char* gp = a.g1 + ((size_t)(tile - t_first) * gridDim.x + blockIdx.x) * (NKS * 4096);  // (layout: see fillv below)
#pragma unroll
        for (int c = 0; c < NKS; ++c) {
          *(bf16x8*)(gp + c * 4096 + (unsigned)tid16) = gb[c];
        }
      }
      TRACE(30 + l);
      if (DW && l >= 2) {  // (layer 1 has no in-kernel dW GEMM: nothing to transpose, one barrier for the weight image)
        __syncthreads();  // B1: every wave finished the previous step's LDS reads
        TRACE(40 + l);
        ts_write<NRB>(TA, gb, wave * 32 + jx, hix);
        TRACE(80 + l);
        // h_{l-1} = sin(phase_{l-1}) straight into the transposed image (dW_l's column operand)
        const unsigned hbase = ts_write_base(TB, wave * 32 + jx, hix);
#pragma unroll
        for (int c = 0; c < NRB * 2; ++c) {
          bf16x8 hv;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            hv[2 * d] = (__bf16)__builtin_amdgcn_sinf(phase_lo(wph[c][d]));
            hv[2 * d + 1] = (__bf16)__builtin_amdgcn_sinf(phase_hi(wph[c][d]));
          }
          ts_write_chunk(hbase, hv, c);
        }
      }
      TRACE(50 + l);
      dma_wait();       // this step's W^T image (issued one step ago)
      __syncthreads();  // B2
      TRACE(60 + l);
      if (!DW && l >= 2) {  // behind the vmcnt(0) above: a whole step to land
        if constexpr (!FILM) {
          load_phases(l == 2 ? StashAt{(gchar*)(unsigned long long)(a.afrag + (size_t)b * (NRB * 1024)), (unsigned)lane16} : stash_mid(l - 2), wnx);
        } else {
          load_phases(stash_mid(l - 2), wnx);
        }
      }
      // next step's image (or the next tile's first): one LDS-DMA group per k-step of the GEMM below
      DmaJob jb = make_job(k + 1 < nstep ? k + 1 : 0);  // (L0X: k + 1 == nstep in the last step)
      if (k + 1 >= nstep && last_tile) jb.ng = 0;
      if (L0X && l == L) jb.ng = 0;  // (shared images: layer L - 1's is still in the other buffer)
      TRACE(70 + l);
      // (l == 2: instead of layer 0's phases, the image's layer-0 A operands, through the SAME eight loads -- no second
      // code path: with the 512-byte chunk stride and the lane offset, chunk 2r is operand r of this lane; the odd chunks are
      // not used.  Step 1 rebuilds the phase words from them.)
      const StashAt sl_nx = [&]() -> StashAt {
        // (L0X, last step: the NEXT tile's image -- chunk 2 r is its layer-0 A operand r, carried to the next iteration in aop0_n)
        if constexpr (L0X) { if (l == 2) return StashAt{(gchar*)(unsigned long long)(a.afrag + (size_t)(last_tile ? cur_b : nxt_b) * (NRB * 1024)), (unsigned)lane16}; }
        if constexpr (DW && !FILM && !L0X) { if (l == 2) return StashAt{(gchar*)(unsigned long long)(a.afrag + (size_t)b * (NRB * 1024)), (unsigned)lane16}; }
        return stash_mid(l >= 2 ? l - 2 : 0);  // (l == 1: a harmless re-read of layer 0's chunks, no branch)
      }();
      // a whole step ahead.  NOT conditional on l >= 2 (step 1 re-reads layer 0's chunks to no purpose): with the loads behind a
      // runtime condition hipcc's wait counts for the phase words this step uses assume the path WITHOUT them, i.e. vmcnt(7 - c) --
      // which in the path with them waits for the loads just issued (cycle trace: +500 cycles on every second step of the loop)
      if constexpr (DW) load_phases(sl_nx, wnx);
      if constexpr (!L0X) { if (l == 1) load_d(dre); }  // for the dA phase after the loop; in flight during the dX GEMM
      if constexpr (L0X) { if (l == 2) dma_dirs(last_tile ? cur_b : nxt_b, last_tile ? cur_tin : nxt_tin); }  // the next tile's directions
      if constexpr (L0X) { if (l == L) dma_tw(last_tile ? cur_b : nxt_b, last_tile ? cur_tin : nxt_tin); }  // ... target / weight rows
      const char* wb = smem + ((L0X ? l - 1 : k) & 1) * GP::WBSZ;  // (L0X: the buffer the forward pass used for this layer)
      const float* const tq_prev = FILM ? ftab + (l - 1) * 2 * H : nullptr;  // frequencies of layer l - 1 (slot 0: ones)
      {
        const bool had_dw = DW && l >= 2;  // (then the image's groups went behind the dW GEMM's k-steps)
        // vector-memory fillers of the dX GEMM's 32 MFMA slots
        auto fillv = [&](int rb, int ks) {
          if (!had_dw && rb == 0 && ks < DG) dma_group(jb, ks, wave, NW);
          if constexpr (DW && !FILM) {  // the g_1 stream (dW_1 is finished by k_reni_dw1)
            if (l == 1 && (ks & 3) == 2) {
              const int c = 2 * rb + (ks >> 2);
              // g_1 stream layout [tile within the workgroup's range][workgroup][32 KB]: the workgroups run in step, so at any moment they
              // write (and k_reni_dw1's read) the same position of their ranges -- range-major these are 256 blocks 2 MB apart,
              // interleaved like this one contiguous 8 MB region, spread evenly over the memory channels
              *(bf16x8*)(a.g1 + ((size_t)(tile - t_first) * gridDim.x + blockIdx.x) * (NKS * 4096) + (size_t)((unsigned)tid16 + (unsigned)(c * 4096))) = gb[c];
            }
          }
        };
        TRACE(190 + l);
        if constexpr (DW) {
          switch (l) {  // one static AGPR tile set per layer
            case 5: dwdx_layer(std::integral_constant<int, 12>{}, wb, gb, jb, wph, ghb, tq_prev, pdb[4]); break;
            case 4: dwdx_layer(std::integral_constant<int, 8>{}, wb, gb, jb, wph, ghb, tq_prev, pdb[3]); break;
            case 3: dwdx_layer(std::integral_constant<int, 4>{}, wb, gb, jb, wph, ghb, tq_prev, pdb[2]); break;
            case 2: dwdx_layer(std::integral_constant<int, 0>{}, wb, gb, jb, wph, ghb, tq_prev, pdb[1]); break;
            default: if constexpr (!L0X) dx_layer(wb, gb, fillv, wph, ghb, tq_prev, l); break;  // layer 1: no in-kernel dW (k_reni_dw1)
          }
        } else {
          dx_layer(wb, gb, fillv, wph, ghb, tq_prev, l);
        }
      }
    };
    {
      // Steps run in pairs with the arrays' roles exchanged (nothing loop-carried is copied) and BOTH steps of a pair have l >= 2 as
      // far as hipcc can tell: with `for (l >= 2) { step(l); step(l - 1); }` the second step may be step 1, so it carried step 1's
      // conditional g_1 stores, weight-image groups and branches around them -- +10 % on every second dX GEMM (cycle trace).  An even
      // layer count takes its first step ahead of the loop (and pays the 64 copies that put the arrays back in their roles).
      // (round 5: the FiLM training instances take the paired loop too -- with the table addresses formed per tile, above, they no longer
      // spill with one more copy of the step)
      if constexpr (L0X) {
        // odd L >= 3 (launch_train): pairs down to (3, 2) -- layer 2's is the LAST step: g_1 ends in gA, the next tile's layer-0 A
        // operands in wB[0, 2, 4, 6]
        // (do-while: the instance is only launched with L >= 3 -- l0x_ok -- and a loop that may run zero times gives the counted wait
        // below a predecessor path without the g_1 stores it counts: tests/test_build_audit.py walks every path)
        int l = L;
#pragma unroll 1
        do { step(l, gA, gB, wB, wA); step(l - 1, gB, gA, wA, wB); } while ((l -= 2) >= 3);
      } else {
      int l = L;
      if ((L & 1) == 0) {
        step(l, gA, gB, wB, wA);
        --l;
#pragma unroll
        for (int c = 0; c < NKS; ++c) gA[c] = gB[c];
#pragma unroll
        for (int c = 0; c < NRB * 2; ++c) wB[c] = wA[c];
      }
#pragma unroll 1
      for (; l >= 3; l -= 2) { step(l, gA, gB, wB, wA); step(l - 1, gB, gA, wA, wB); }
      step(1, gA, gB, wB, wA);  // (l == 1 here: g_0 ends in gB)
      }
    }
    bf16x8 (&gb)[NKS] = gB;  // g_0
    TRACE(8);
    if constexpr (L0X) {
      // ---- the tile ends here: g_1 (in gA) goes to the stream; k_reni_l0_ring does layer 1's dX GEMM, g_0, dA and dW_1 from it.
      // Stream layout [tile within the workgroup's range][workgroup][8 chunks x 4 KB]; within a chunk the 16-byte cell of thread t
      // sits at cell (t ^ 4 hi ^ 8 (chunk & 1)): see the kernel's header.
      // (the stores left from layer 2's stream: dwdx_layer, G1ST)
      // the next tile's first image (its groups went out behind the last step's first MFMAs): "all but the eight newest" = all but the
      // g_1 stores (the next tile's first barrier has no vmcnt; tests/test_build_audit.py checks the order on the emitted ISA)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
#pragma unroll
      for (int rbo = 0; rbo < NRB; ++rbo) aop0_n[rbo] = __builtin_bit_cast(bf16x8, wB[2 * rbo]);    } else
    // ---- layer 0: dA (per tile) = g_0 (x_hi | x_lo)^T
    {
      bf16x8 xcb[2];
#pragma unroll
      for (int e = 0; e < 8; ++e) { xcb[0][e] = (__bf16)0.f; xcb[1][e] = (__bf16)0.f; }
      {
        __bf16 xh[5], xl[4];
        split_x(dre, xh, xl);  // direction re-read issued before the last dX GEMM
        if (hi == 0) {
#pragma unroll
          for (int k2 = 0; k2 < 4; ++k2) { xcb[0][k2] = xh[k2]; xcb[0][4 + k2] = xl[k2]; }
        } else {
          xcb[0][0] = (__bf16)1.f;
        }
      }
#pragma unroll
      for (int hsel = 0; hsel < NHALF; ++hsel) {  // the halves take turns on the one pair of transposition images
        // (first turn: the images' last readers -- step 2's dW GEMM, or the previous tile's dA GEMM in the frozen
        // instance -- already lie behind a later barrier of every wave)
        if (hsel > 0) __syncthreads();
        if (half == hsel) {
          ts_write<NRB>(TA, gb, wq * 32 + j, hi);
          ts_write<1>(TB, xcb, wq * 32 + j, hi);
        }
        // the next tile's first image (issued during the last dX GEMM): its barrier has no vmcnt.  Training instance: the
        // eight g_1 stores were issued BEHIND the image's last piece (dx_layer's fillv) and nothing else since, so "all but the
        // eight newest" covers the image without waiting out the stores' trip to HBM (tests/test_build_audit.py checks the
        // order on the emitted ISA)
        if (hsel == 0) {
          if constexpr (DW && !FILM) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
          else dma_wait();
          if constexpr (INCR) {  // (the last tile "prefetches" itself: harmless, as before)
            prefetch_tile(tile0 + t_step, last_tile ? cur_b : nxt_b, last_tile ? cur_tin : nxt_tin);
          } else if constexpr (PREF) prefetch_tile(tile0 + t_step);  // the next tile's first inputs: a barrier, the dA GEMM and the loop's tail to land in
        }
        TRACE(94);
        __syncthreads();
        TRACE(95);
        if (half == hsel) {
          f32x16 accA[1];
          float dummy = 0.f;
          dw_gemm_s<1, DW_L0, 2>(TA, TB, accA, dummy, wq, lane);
          TRACE(96);
          int lane_o = lane;  // opaque: the lane's offset into the partial is loop-invariant, and hipcc would hoist it out of the
          asm volatile("" : "+v"(lane_o));  // tile loop into a scratch slot it reloads (and waits for) every tile
          if constexpr (DW) {
            // columns 0..4 = (x_hi | 1), 8..11 = x_lo: the sum keeps hi + lo, 8 floats per row (as dw_flush<DW_L0> does);
            // element (row, j) belongs to exactly one lane of one wave: plain LDS +=, no atomics, fixed order
            // (the lo parts come over with one DPP row shift each and the sixteen read-modify-writes are sixteen reads, then sixteen
            // writes: __shfl_down + += one element at a time were sixteen dependent LDS round trips, 2700 cycles per tile; sixteen
            // ds_add_f32 without return value were no better -- LDS float atomics take ~170 cycles apiece)
            float* const dl = dAacc + (32 * wq + 4 * (lane_o >> 5)) * 8 + (lane_o & 31);  // (all of it from the opaque lane_o: see above)
            float add[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float lo = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, accA[0][r]), 0x108, 0xf, 0xf, true));  // row_shl:8: lane j <- lane j + 8
              add[r] = accA[0][r] + (((lane_o & 31) < 4) ? lo : 0.f);
            }
            if ((lane_o & 31) < 8) {
              float old[16];
#pragma unroll
              for (int r = 0; r < 16; ++r) old[r] = dl[((r & 3) + 8 * (r >> 2)) * 8];
#pragma unroll
              for (int r = 0; r < 16; ++r) dl[((r & 3) + 8 * (r >> 2)) * 8] = old[r] + add[r];
            }
          } else {
            if (tvalid) dw_flush<Pol, H, NRB, 1, DW_L0, 1>(accA, 0.f, a.dA_part + (size_t)tile * H * 8, nullptr, 16, true, wq, lane_o);
          }
        }
      }
    }
    if constexpr (DW) {
      // end of an image run (the next tile belongs to another image, or there is none): the sums leave the chip.
      // Every accumulator element has one owner lane, which writes and clears it: no barrier.
      if (last_tile || (INCR ? nxt_b : (tile0 + 1) / a.tiles_per_image) != b) {
        // (wave-uniform base + a 32-bit lane offset re-derived here: a per-lane 64-bit address held across the tile loop
        // is a register pair the kernel does not have)
        char* const run = (char*)(a.pruns + ((size_t)blockIdx.x * a.pkmax + run_k) * (H * 8 + 16));
        unsigned eb = (unsigned)((32 * wave + 4 * hi) * 8 + j) * 4u;
        asm volatile("" : "+v"(eb));
        if (!L0X && j < 8) {  // (L0X: the run's dA is written by k_reni_l0_ring, which walks the same range)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned e = eb + (unsigned)(((r & 3) + 8 * (r >> 2)) * 32);
            float* const q = (float*)((char*)dAacc + e);
            *(float*)(run + e) = *q;
            *q = 0.f;
          }
        }
        if constexpr (LACC) {  // the run's weighted squared error: this wave's lane slots, summed here (once per image run)
          float ev = 0.f;
          if (hi == 0) { ev = lacc[wave * 32 + j][0]; lacc[wave * 32 + j][0] = 0.f; }
          const float es = wave_sum(ev);
          if (lane == 0) *(float*)(run + (H * 8 + wave) * 4) = es;
        } else {
          if (lane == 0) { *(float*)(run + (H * 8 + wave) * 4) = loss_run[wave]; loss_run[wave] = 0.f; }
        }
        if (tid == 0) a.prun_image[blockIdx.x * a.pkmax + run_k] = b;
        if constexpr (FILM) {
          // FiLM: the run's accumulators R_l = sum g_a h^T (layers 2..L; layer 1: k_reni_dw1's runs) leave the registers:
          //   dfr[slot][l-1][0][f] = rowsum_k(W_l[f][k] R_l[f][k]) / freq[f]   (= rowsum(W (.) M), M = sum g_theta h^T)
          //   dfr[slot][l-1][1][f] = (sum g_a)[f] / freq[f]                    (= d phase)
          // and, with a trainable decoder, into the run's partial slot; then they start again from zero.
          const size_t slot = (size_t)blockIdx.x * a.pkmax + run_k;
          float* const dwr = a.dwp + slot * a.dwp_per_wg;
          float* const fr = a.dfr + slot * (size_t)L * 2 * H;
          for (int i = tid; i < 2 * H; i += 256) fr[i] = 0.f;  // layer 1's entries come from k_reni_dw1's runs
          if (a.need_dw && run_k > 0) {  // (run 0's head slot is written once, at the end of the kernel; the others hold zeros)
            for (int i = tid; i < 3 * H; i += 256) dwr[a.p_off_w[L + 1] + i] = 0.f;
            if (tid < 3) dwr[a.p_off_b[L + 1] + tid] = 0.f;
          }
          asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
          // (opaque copies of the lane's coordinates: every address below is then formed HERE -- hipcc otherwise hoists the
          // 256 per-lane 64-bit addresses of this block out of the tile loop and spills them)
          int hio = hi, jo = j;
          asm volatile("" : "+v"(hio), "+v"(jo));
          auto film_flush = [&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if (l <= L) {
              f32x16 t[MYB_H] = {agpr_read_tile<4 * (l - 2) + 0>(), agpr_read_tile<4 * (l - 2) + 1>(),
                                 agpr_read_tile<4 * (l - 2) + 2>(), agpr_read_tile<4 * (l - 2) + 3>()};
              const float* const tq = ftab + l * 2 * H;                       // freq / 2 pi of this layer and image
              const float* const Wl = a.params + a.n_first + a.p_off_w[l];    // fp32 W_l [H][H]
              float dbs = pdb[l - 1];
              dbs += __shfl_xor(dbs, 32, 64);
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int row = 32 * wave + rowmap(r, hio);
                float pr = 0.f;
#pragma unroll
                for (int m = 0; m < MYB_H; ++m) pr = __builtin_fmaf(Wl[(unsigned)(row * H + 32 * m + jo)], t[m][r], pr);
                pr = half_sum(pr);
                const float fq = tq[row] * 6.283185307179586f;
                if (jo == r) fr[(unsigned)((l - 1) * 2 * H + row)] = (fq != 0.f) ? pr / fq : 0.f;
              }
              if (hio == 0) {
                const int row = 32 * wave + jo;
                const float fq = tq[row] * 6.283185307179586f;
                fr[(unsigned)((l - 1) * 2 * H + H + row)] = (fq != 0.f) ? dbs / fq : 0.f;
              }
              if (a.need_dw) dw_flush<Pol, H, NRB, NRB, DW_HIDDEN, MYB_H>(t, pdb[l - 1], dwr + a.p_off_w[l], dwr + a.p_off_b[l], H, true, wave, hio * 32 + jo);
              agpr_zero_range<64 * (l - 2)>(std::make_integer_sequence<int, 64>{});
              pdb[l - 1] = 0.f;
            }
          };
          film_flush(std::integral_constant<int, 2>{});
          film_flush(std::integral_constant<int, 3>{});
          film_flush(std::integral_constant<int, 4>{});
          film_flush(std::integral_constant<int, 5>{});
        }
        ++run_k;
      }
    }
    if constexpr (INCR) { cur_b = nxt_b; cur_tin = nxt_tin; }
    TRACE(9);
  }
  int tid_e = L0X ? (int)((unsigned)tid16 >> 4) : tid;  // opaque copy for the epilogue: addresses derived from tid before the tile loop are not kept alive across it
                                                       // (L0X: from the loop-carried tid16 -- tid itself, kept for this line alone, was spilled and reloaded every tile)
  asm volatile("" : "+v"(tid_e));
  if constexpr (DW) {  // the run slots this workgroup did not use
    for (int k = run_k + tid_e; k < a.pkmax; k += 256) a.prun_image[blockIdx.x * a.pkmax + k] = -1;
  }
  // ---- the only write of the hidden-layer weight-gradient partials: once per workgroup per launch
  if constexpr (DW && FILM) {  // FiLM: the hidden layers left with their image runs; the head's sums go to run 0's slot
    if (a.need_dw) {
      if constexpr (LACC) {  // db_out: every wave sums its lanes' (g_y) slots, once per launch (as below)
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((tid_e & 63) < 32) v = lacc[(tid_e >> 6) * 32 + (tid_e & 31)];
        const float s0 = wave_sum(v[1]), s1 = wave_sum(v[2]), s2 = wave_sum(v[3]);
        if ((tid_e & 63) == 0) { float* o = hdb + 4 * (tid_e >> 6); o[0] = s0; o[1] = s1; o[2] = s2; }
      }
      __syncthreads();
      float* const dw0 = a.dwp + (size_t)blockIdx.x * a.pkmax * a.dwp_per_wg;
      for (int i = tid_e; i < 3 * H; i += 256) dw0[a.p_off_w[L + 1] + i] = hdw[i];
      if (tid_e < 3) dw0[a.p_off_b[L + 1] + tid_e] = (hdb[tid_e] + hdb[4 + tid_e]) + (hdb[8 + tid_e] + hdb[12 + tid_e]);
    }
  } else if constexpr (DW) {
    if constexpr (LACC) {  // db_out: every wave sums its lanes' (g_y) slots, once per launch
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((tid_e & 63) < 32) v = lacc[(tid_e >> 6) * 32 + (tid_e & 31)];
      const float s0 = wave_sum(v[1]), s1 = wave_sum(v[2]), s2 = wave_sum(v[3]);
      if ((tid_e & 63) == 0) { float* o = hdb + 4 * (tid_e >> 6); o[0] = s0; o[1] = s1; o[2] = s2; }
    }
    __syncthreads();
    for (int i = tid_e; i < 3 * H; i += 256) dwp[a.p_off_w[L + 1] + i] = hdw[i];
    if (tid_e < 3) dwp[a.p_off_b[L + 1] + tid_e] = (hdb[tid_e] + hdb[4 + tid_e]) + (hdb[8 + tid_e] + hdb[12 + tid_e]);
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    TRACE_FLUSH(510, 10);
    auto flush_layer = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      if (l <= L) {
        f32x16 t[MYB_H] = {agpr_read_tile<4 * (l - 2) + 0>(), agpr_read_tile<4 * (l - 2) + 1>(),
                           agpr_read_tile<4 * (l - 2) + 2>(), agpr_read_tile<4 * (l - 2) + 3>()};
        // (L0X: the layer's H x H slice in the quad-row layout, 16-byte stores -- dw_flush_quad; the host sums it with the matching reducer)
        if constexpr (L0X) dw_flush_quad<H, NRB, MYB_H>(t, pdb[l - 1], dwp + a.p_off_w[l], dwp + a.p_off_b[l], wave, tid_e & 63);
        else dw_flush<Pol, H, NRB, NRB, DW_HIDDEN, MYB_H>(t, pdb[l - 1], dwp + a.p_off_w[l], dwp + a.p_off_b[l], H, true, wave, L0X ? (tid_e & 63) : lane);
      }
    };
    flush_layer(std::integral_constant<int, 2>{});
    flush_layer(std::integral_constant<int, 3>{});
    flush_layer(std::integral_constant<int, 4>{});
    flush_layer(std::integral_constant<int, 5>{});
  }
#ifdef RENI_TRACE
  if constexpr (DW && !FILM) {  // (the flush's own stamps, slots 510 / 511 behind the tile loop's: before it, and when its stores have left)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TRACE_FLUSH(511, 11);
  }
  if (trace_on) {
    for (int i = (int)(threadIdx.x & 63); i < 512; i += 64) a.trace[i] = (i < trace_n || (DW && !FILM && i >= 510)) ? (long long)trace_lds[i] : 0ll;
  }
#endif
}
#ifdef RENI_TU_CORE
template __global__ void k_reni_train_bf16<128, true>(const MainArgs);
template __global__ void k_reni_train_bf16<128, true, false, false, true>(const MainArgs);
template __global__ void k_reni_train_bf16<128, true, false, false, true, true>(const MainArgs);
template __global__ void k_reni_train_bf16<128, false>(const MainArgs);
template __global__ void k_reni_train_bf16<128, false, true>(const MainArgs);
#endif

// dW_1 / db_1 for the persistent training path: K = samples GEMM of the stored g_1 stream (bf16,
// D layout, written by k_reni_train_bf16) with h_0 = sin(2 pi (afrag_b x)) recomputed from the directions --
// the training kernel's own layer-0 arithmetic (same pre-scaled A operands, same hi/lo split of x), so h_0 is
// bit-identical to what its forward pass used.
// Persistent workgroups, two per CU (the kernel is latency-bound at one: -30 us); the 128 x 128 accumulator stays in
// registers over all of a workgroup's tiles.
// FILM = true (FiLM on the persistent path): g_1 is g_a = freq . g_theta, so dW_1 needs no per-image state, but
// d freq_1 = rowsum(W_1 (.) R) / freq + b (.) d phase and d phase_1 = (sum g_a) / freq are per image: the accumulator leaves the
// registers at the end of every IMAGE RUN of the walk (into the run's partial slot and MainArgs::dfr, slots behind the training
// kernel's) and starts again from zero.
#if defined(RENI_TRACE_DW1)
#define TRACE1(tag) do { __builtin_amdgcn_sched_barrier(0); if (trace_on && trace_n < 1000) { trace_lds[trace_n] = ((unsigned long long)__builtin_amdgcn_s_memtime() & 0xffffffffffffull) | ((unsigned long long)(tag) << 48); ++trace_n; } __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TRACE1(tag) do {} while (0)
#endif
template <int H, bool FILM = false>
__global__ void __launch_bounds__(256, 2) k_reni_dw1(const MainArgs a) {
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  constexpr int NRB = G::NRB, NKS = G::NKS;
  constexpr int MYB_H = (NRB * NRB + 3) / 4;
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // ts_write / ts_read XOR into the low address byte
  char* const TA = smem;
  char* const TB = smem + TS_BYTES;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
#if defined(RENI_TRACE_DW1)  // cycle trace of wave 0 of workgroup 0 (as k_reni_train_bf16's; profiles/tools/gpu_trace_dw1.py)
  unsigned long long* const trace_lds = (unsigned long long*)(smem + 2 * TS_BYTES);
  int trace_n = 0;
  const bool trace_on = a.trace != nullptr && blockIdx.x == 0 && wave == 0;
#endif
  TRACE1(100);
#if defined(RENI_TRACE_DW1) && RENI_TRACE_DW1 == 2  // every workgroup's start / end on the 100 MHz wall clock instead of the one-wave trace
  const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();
#endif
  f32x16 acc[MYB_H];
  acc_zero<MYB_H>(acc);
  float db = 0.f;

  // inputs of a tile: the g_1 fragments, this lane's direction and the image's layer-0 A operands (k_prep_image's
  // afrag).  They are fetched one tile ahead so their HBM latency hides behind the previous tile's work.
  bf16x8 gbN[NKS], aopN[NRB];
  float dN[3];
  int imgN = -1;  // image whose A operands aopN holds: a range walks an image's tiles one after another, so they are fetched once
                  // per image run instead of once per tile (four of a tile's fifteen vector-memory instructions)
  const int G_ = a.nwg_main, g_ = (int)blockIdx.x % G_, par_ = (int)blockIdx.x / G_;
  const int t_lo = (int)((long long)g_ * a.n_tiles / G_);
  auto fetch = [&](int tile) {
    const int b = tile / a.tiles_per_image;
    const int p = (tile - b * a.tiles_per_image) * 128 + wave * 32 + j;
    const float* dp = a.D + (size_t)b * a.d_bstride + (size_t)(p < a.P ? p : 0) * 3;
    dN[0] = dp[0]; dN[1] = dp[1]; dN[2] = dp[2];
    const char* gp = a.g1 + ((size_t)(tile - t_lo) * G_ + g_) * (NKS * 4096);  // ([position in the range][range]: k_reni_train_bf16)
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
      gbN[c] = *(const bf16x8*)(gp + c * 4096 + tid * 16);
    }
    if (b != imgN) {
      imgN = b;
#pragma unroll
      for (int rbo = 0; rbo < NRB; ++rbo) aopN[rbo] = *(const bf16x8*)(a.afrag + ((size_t)(b * NRB + rbo) * 64 + lane) * 16);
    }
  };
  // Two workgroups per range of the training kernel (its workgroup g wrote the g_1 fragments of tiles [g n / G, (g + 1) n / G)
  // in ascending order), each walking it BACKWARDS with stride 2: the most recently written fragments -- the part of the
  // 0.5 GB stream that is still in the 256 MB Infinity Cache -- are read first, before later reads push them out.
  const int t_hi = (int)((long long)(g_ + 1) * a.n_tiles / G_) - 1 - par_;
  if (t_hi >= t_lo) fetch(t_hi);
  int run_k = 0;
  const size_t slot0 = (size_t)a.nwg_main * a.pkmax + (size_t)blockIdx.x * a.pkmax;  // this workgroup's run slots (FiLM)
  auto film_flush = [&](int b_run) {
    const size_t slot = slot0 + run_k;
    const int L = a.L;
    float* const fr = a.dfr + slot * (size_t)L * 2 * H;
    for (int i = tid; i < (L - 1) * 2 * H; i += 256) fr[2 * H + i] = 0.f;  // layers >= 2: the training kernel's runs
    const float* const fq1 = a.film + (size_t)b_run * L * 2 * H;           // freq of layer 1, this image
    const float* const Wl = a.params + a.n_first + a.p_off_w[1];
    float dbs = db;
    dbs += __shfl_xor(dbs, 32, 64);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * wave + rowmap(r, hi);
      float pr = 0.f;
#pragma unroll
      for (int m = 0; m < MYB_H; ++m) pr = __builtin_fmaf(Wl[(size_t)row * H + 32 * m + j], acc[m][r], pr);
      pr = half_sum(pr);
      const float fq = fq1[row];
      if (j == r) fr[row] = (fq != 0.f) ? pr / fq : 0.f;
    }
    if (hi == 0) {
      const int row = 32 * wave + j;
      const float fq = fq1[row];
      fr[H + row] = (fq != 0.f) ? dbs / fq : 0.f;
    }
    if (a.need_dw) {
      float* const dwr = a.dw1p + slot0 / a.pkmax * 0 + ((size_t)blockIdx.x * a.pkmax + run_k) * (H * H + H);
      dw_flush<Pol, H, NRB, NRB, DW_HIDDEN, MYB_H>(acc, db, dwr, dwr + H * H, H, true, wave, lane);
    }
    if (tid == 0) a.prun_image[slot] = b_run;
    acc_zero<MYB_H>(acc);
    db = 0.f;
    ++run_k;
  };
#pragma unroll 1
  for (int tile = t_hi; tile >= t_lo; tile -= 2) {
    bf16x8 gb[NKS], aop[NRB];
    float x[5];
    TRACE1(1);
#pragma unroll
    for (int c = 0; c < NKS; ++c) gb[c] = gbN[c];
#pragma unroll
    for (int rbo = 0; rbo < NRB; ++rbo) aop[rbo] = aopN[rbo];
    x[0] = dN[0]; x[1] = dN[1]; x[2] = dN[2];
    TRACE1(2);
    if (tile - 2 >= t_lo) fetch(tile - 2);
    TRACE1(3);
    x[3] = sqrtf(x[0] * x[0] + x[2] * x[2]);
    x[4] = 1.f;
    __bf16 xh[5], xl[4];
#pragma unroll
    for (int k = 0; k < 5; ++k) xh[k] = (__bf16)x[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) xl[k] = (__bf16)(x[k] - (float)xh[k]);
    bf16x8 hb[NKS];
    {
      bf16x8 bop;
      if (hi == 0) { bop[0] = xh[0]; bop[1] = xh[1]; bop[2] = xh[2]; bop[3] = xh[3]; bop[4] = xh[4]; bop[5] = xh[0]; bop[6] = xh[1]; bop[7] = xh[2]; }
      else { bop[0] = xh[3]; bop[1] = xh[4]; bop[2] = xl[0]; bop[3] = xl[1]; bop[4] = xl[2]; bop[5] = xl[3]; bop[6] = (__bf16)0.f; bop[7] = (__bf16)0.f; }
#pragma unroll
      for (int rbo = 0; rbo < NRB; ++rbo) {
        f32x16 a0;
#pragma unroll
        for (int r = 0; r < 16; ++r) a0[r] = 0.f;
        a0 = PolBF16::mfma(aop[rbo], bop, a0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          hb[2 * rbo + (r >> 3)][r & 7] = (__bf16)__builtin_amdgcn_sinf(!FILM ? a0[r] : __builtin_amdgcn_fractf(a0[r]));  // (as the training kernel's forward)
      }
    }
    TRACE1(4);
    __syncthreads();
    TRACE1(5);
    ts_write<NRB>(TA, gb, wave * 32 + j, hi);
    ts_write<NRB>(TB, hb, wave * 32 + j, hi);
    TRACE1(6);
    __syncthreads();
    TRACE1(7);
    dw_gemm_s<NRB, DW_HIDDEN, 0>(TA, TB, acc, db, wave, lane);
    TRACE1(8);
    if constexpr (FILM) {  // end of an image run of the walk (the next tile, two below, belongs to another image or to nobody)
      const int b_now = tile / a.tiles_per_image;
      if (tile - 2 < t_lo || (tile - 2) / a.tiles_per_image != b_now) film_flush(b_now);
    }
  }
  if constexpr (FILM) {
    for (int k = run_k + tid; k < a.pkmax; k += 256) a.prun_image[slot0 + k] = -1;  // the run slots this workgroup did not use
  } else {
    float* const dwp = a.dw1p + (size_t)blockIdx.x * (H * H + H);  // its own partials: [W_1 | b_1] per workgroup
    TRACE1(101);
    dw_flush<Pol, H, NRB, NRB, DW_HIDDEN, MYB_H>(acc, db, dwp, dwp + H * H, H, true, wave, lane);
  }
#ifdef RENI_TRACE_DW1
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TRACE1(102);
#if RENI_TRACE_DW1 == 2
  if (a.trace != nullptr && tid == 0 && blockIdx.x < 512) {
    a.trace[2 * blockIdx.x] = (long long)wg_t0;
    a.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  }
#else
  if (trace_on) {
    for (int i = lane; i < trace_n; i += 64) a.trace[i] = (long long)trace_lds[i];
  }
#endif
#endif
}
#ifdef RENI_TU_CORE
template __global__ void k_reni_dw1<128>(const MainArgs);
#endif

// ---- k_reni_dw1_ring: the same sum for the concatenation decoder, fed by LDS-DMA -----------------------------------------------------
// k_reni_dw1 above takes a tile's g_1 fragments through registers (eight 16-byte loads per lane, one tile ahead) and re-writes them
// into a transposition image: its tile takes what the memory round trip takes (per-workgroup timeline, profiles/r03_dw1.md), two
// workgroups per CU are the most the registers and the two images allow, and the second of each pair ends 25 % after the first.
// Here a tile's inputs never touch a register before they are operands:
//   * one workgroup per CU walks a whole range of the training kernel (backwards, as above: the most recently written -- still
//     cached -- tiles first); a ring of three LDS slots holds [the tile's 32 KB of g_1 AS STORED | the image's four layer-0 A
//     operands | the tile's 128 directions], filled by global_load_lds two tiles ahead of the GEMM (76 KB in flight per CU);
//   * the A operand of dW_1 = sum g_1 h_0^T is read from the RAW slot with the transposing LDS read: in the stored (D) layout the
//     8-byte piece (sample s, features 32 blk + 8 q' + 4 hi' + 0..3) sits at chunk (2 blk + (q' >> 1)), thread (64 (s >> 5) + 32 hi' +
//     (s & 31)), half (q' & 1) -- ds_read_b64_tr_b16 takes any per-lane row address, so no second image and no ds_write of g_1;
//   * h_0 is rebuilt as above (bit-identical to the forward pass's) and written to the one transposition image TB.
// Per wave and tile: 10 LDS-DMA instructions (counted by hand: vmcnt(10) = "everything but the newest tile has landed"; the loop
// has no compiler-visible vector-memory operation, so hipcc inserts no wait of its own), two barriers.
// Needs P % 128 == 0 (a tile's directions are one 1536-byte run) and 16-byte aligned direction rows; otherwise, and for FiLM,
// launch_dw1 keeps k_reni_dw1.
DEV void glds16x4(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, %2\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst_uniform) : "memory");
}
struct Dw1Ring {
  static constexpr int SLOT_G = 8 * 4096, SLOT_A = 4 * 1024, SLOT_D = 2048, SLOT = SLOT_G + SLOT_A + SLOT_D, NSLOT = 3;
  static constexpr int TBH = TS_BYTES / 2;  // transposition image of HALF a tile's h_0 (64 samples), two of them
  static constexpr int LDS_BYTES = 2 * TBH + NSLOT * SLOT;
  static constexpr int VM_PER_TILE = 10;  // LDS-DMA instructions per loader wave and tile (issue())
  static constexpr int THREADS = 768;
};
// Eight waves in two ROLES, one wave of each per SIMD (measured first with every wave doing everything: a lone wave per SIMD took
// 5.5 k cycles per tile, two took 5.1 k -- the h_0 rebuild is bound by the transcendental unit (64 v_sin_f32 per SIMD and tile) and
// the GEMM by LDS bandwidth (every fragment an MFMA takes is 1 KB), and the phases alternated instead of overlapping):
//   * waves 0..3, PRODUCERS: rebuild h_0 half a tile (64 samples) at a time -- wave w: samples 32 (w & 1).., feature blocks
//     2 (w >> 1), 2 (w >> 1) + 1 -- into the half-tile image TBh[half];
//   * waves 4..7, CONSUMERS: the K = 64 slice of dW_1 += g_1 h_0^T for the half tile the producers wrote one step EARLIER, a
//     2 x 2 block of 32 x 32 accumulators per wave (eight LDS reads per four MFMAs; 1 x 4 blocks need ten).
// One barrier per half tile; the slot of tile i + 2 is requested when tile i - 1's g_1 has been consumed (step 2 i + 1).
template <int H>
__global__ void __launch_bounds__(768, 1) k_reni_dw1_ring(const MainArgs a) {
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  constexpr int NRB = G::NRB, NKS = G::NKS;
  static_assert(NRB == 4 && NKS == 8, "ring slot layout");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const unsigned ring = __builtin_amdgcn_readfirstlane(lds_u32(smem + 2 * Dw1Ring::TBH));
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2;  // 0 producer, 1 consumer, 2 loader
  const int v = wave & 3;
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  const unsigned lane16 = (unsigned)lane * 16;
#if defined(RENI_TRACE_DW1)
  unsigned long long* const trace_lds = (unsigned long long*)(smem + Dw1Ring::LDS_BYTES);
  int trace_n = 0;
#ifndef RENI_TRACE_WAVE
#define RENI_TRACE_WAVE 0
#endif
  const bool trace_on = a.trace != nullptr && blockIdx.x == 0 && wave == RENI_TRACE_WAVE;
#if RENI_TRACE_DW1 == 2
  const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();
#endif
#endif
  TRACE1(100);
  f32x16 acc[2][2];  // consumers: [row block 2 (v >> 1) + .][column block 2 (v & 1) + .]
  acc_zero<2>(acc[0]);
  acc_zero<2>(acc[1]);
  float db[2] = {0.f, 0.f};
  const int G_ = a.nwg_main, g_ = (int)blockIdx.x;
  const int t_lo = (int)((long long)g_ * a.n_tiles / G_);
  const int t_hi = (int)((long long)(g_ + 1) * a.n_tiles / G_) - 1;
  const int n = t_hi - t_lo + 1;
  auto issue = [&](int i) {  // loader wave v: its quarter of tile t_hi - i into slot i % NSLOT, VM_PER_TILE instructions
    const int tile = t_hi - i;
    const int b = tile / a.tiles_per_image;
    const int p0 = (tile - b * a.tiles_per_image) * 128;
    const unsigned dst = ring + (unsigned)(i % Dw1Ring::NSLOT) * Dw1Ring::SLOT;
    const char* gp = a.g1 + ((size_t)(tile - t_lo) * G_ + g_) * (NKS * 4096) + (size_t)v * 8192;  // (layout: k_reni_train_bf16's fillv)
    glds16x4(gp, lane16, dst + (unsigned)v * 8192);
    glds16x4(gp + 4096, lane16, dst + (unsigned)v * 8192 + 4096);
    // the image's layer-0 A operands (k_prep_image's afrag), one row block; a quarter of the tile's 128 directions (1536 bytes)
    glds16(a.afrag + ((size_t)(b * NRB + v) * 64) * 16, lane16, dst + Dw1Ring::SLOT_G + (unsigned)v * 1024);
    const char* dp = (const char*)(a.D + (size_t)b * a.d_bstride + (size_t)p0 * 3) + v * 384;
    if (lane < 24) glds16(dp, lane16, dst + Dw1Ring::SLOT_G + Dw1Ring::SLOT_A + (unsigned)v * 384);
  };
  // producer: half `hh` of tile step i
  auto produce = [&](int i, int hh) {
    const char* const sb = smem + 2 * Dw1Ring::TBH + (i % Dw1Ring::NSLOT) * Dw1Ring::SLOT;
    char* const T = smem + hh * Dw1Ring::TBH;
    const int sl = 32 * (v & 1) + j;  // sample within the half tile
    float x[5];
    {
      const float* dl = (const float*)(sb + Dw1Ring::SLOT_G + Dw1Ring::SLOT_A) + (64 * hh + sl) * 3;
      x[0] = dl[0]; x[1] = dl[1]; x[2] = dl[2];
    }
    bf16x8 aop[2];
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2) aop[r2] = *(const bf16x8*)(sb + Dw1Ring::SLOT_G + ((2 * (v >> 1) + r2) * 64 + lane) * 16);
    x[3] = sqrtf(x[0] * x[0] + x[2] * x[2]);
    x[4] = 1.f;
    __bf16 xh[5], xl[4];
#pragma unroll
    for (int k = 0; k < 5; ++k) xh[k] = (__bf16)x[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) xl[k] = (__bf16)(x[k] - (float)xh[k]);
    bf16x8 bop;
    if (hi == 0) { bop[0] = xh[0]; bop[1] = xh[1]; bop[2] = xh[2]; bop[3] = xh[3]; bop[4] = xh[4]; bop[5] = xh[0]; bop[6] = xh[1]; bop[7] = xh[2]; }
    else { bop[0] = xh[3]; bop[1] = xh[4]; bop[2] = xl[0]; bop[3] = xl[1]; bop[4] = xl[2]; bop[5] = xl[3]; bop[6] = (__bf16)0.f; bop[7] = (__bf16)0.f; }
    const unsigned hbase = ts_write_base(T, sl, hi);
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2) {
      f32x16 a0;
#pragma unroll
      for (int r = 0; r < 16; ++r) a0[r] = 0.f;
      a0 = PolBF16::mfma(aop[r2], bop, a0);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 hv;
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = (__bf16)__builtin_amdgcn_sinf(a0[8 * c + e]);  // (as the training kernel's forward)
        ts_write_chunk(hbase, hv, 2 * (2 * (v >> 1) + r2) + c);
      }
    }
  };
  // consumer: K = 64 samples (half `hh`) of tile step i
  const int khi = lane >> 5, gq = (lane >> 4) & 1, u = lane & 15, pp = u & 3;
  unsigned a_lane = (unsigned)(2 * (v >> 1) * 8192 + gq * 4096 + (pp & 1) * 512 + khi * 128 + (u >> 2) * 16 + (pp >> 1) * 8);
  asm volatile("" : "+v"(a_lane));
  auto consume = [&](int i, auto hh_c) {
    constexpr int hh = decltype(hh_c)::value;
    const char* const sb = smem + 2 * Dw1Ring::TBH + (i % Dw1Ring::NSLOT) * Dw1Ring::SLOT;
    const TsBase bB = ts_base(smem + hh * Dw1Ring::TBH, lane);
    const unsigned ab = lds_u32(sb) + a_lane;
    typedef __attribute__((address_space(3))) s16x4* lp;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    auto a_read = [&](int rbi, int ks) {  // (ks: k-step within the whole tile)
      const unsigned at = ab + (unsigned)(rbi * 8192 + (ks >> 1) * 1024 + (ks & 1) * 256);
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)at);
      const s16x4 hh2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(at + 64));
      const s16x8 w8 = {lo[0], lo[1], lo[2], lo[3], hh2[0], hh2[1], hh2[2], hh2[3]};
      return __builtin_bit_cast(bf16x8, w8);
    };
    // fragments two k-steps ahead (one: every k-step's four MFMAs, 128 cycles, waited out the eight reads' round trip)
    constexpr int PF = 2;
    bf16x8 ra0[PF], ra1[PF], rb0[PF], rb1[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) {
      ra0[d] = a_read(0, 4 * hh + d); ra1[d] = a_read(1, 4 * hh + d);
      rb0[d] = ts_read(bB, 2 * (v & 1), d); rb1[d] = ts_read(bB, 2 * (v & 1) + 1, d);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 fa0 = ra0[ks % PF], fa1 = ra1[ks % PF], f0 = rb0[ks % PF], f1 = rb1[ks % PF];
      if (ks + PF < 4) {
        ra0[ks % PF] = a_read(0, 4 * hh + ks + PF);
        ra1[ks % PF] = a_read(1, 4 * hh + ks + PF);
        rb0[ks % PF] = ts_read(bB, 2 * (v & 1), ks + PF);
        rb1[ks % PF] = ts_read(bB, 2 * (v & 1) + 1, ks + PF);
      }
      acc[0][0] = PolBF16::mfma(fa0, f0, acc[0][0]);
      acc[0][1] = PolBF16::mfma(fa0, f1, acc[0][1]);
      acc[1][0] = PolBF16::mfma(fa1, f0, acc[1][0]);
      acc[1][1] = PolBF16::mfma(fa1, f1, acc[1][1]);
      if ((v & 1) == 0) {  // (the other wave of the row-block pair reads the same g_1 rows)
        db[0] = frag_sum<PolBF16>(fa0, db[0]);
        db[1] = frag_sum<PolBF16>(fa1, db[1]);
      }
    }
    // (tests/isa_audit.py counts a barrier as ONE wait state: the shortest path hipcc lays out from the last MFMA to code that
    // rewrites an accumulator register -- the role dispatch behind the loop -- is ten; four more make the strict count)
    asm volatile("s_nop 3");
  };
  // The three roles run the SAME sequence of barriers from three copies of the loop (one loop with the role tested inside every
  // step kept the consumers' accumulators alive through the producers' code: 256 registers and scratch).
  //   step 2 i    : producers half 0 of tile i, consumers half 1 of tile i - 1
  //   step 2 i + 1: tile i - 1's slot is free -> the loaders request tile i + 2; producers half 1 of tile i, consumers half 0 of
  //                 tile i; the next step needs tile i + 1's slot: only tile i + 2's instructions may be outstanding
  // (LDS-DMA issued by the compute waves themselves, five instructions each, stalled them 500-700 cycles per tile.)
  if (role == 2) {
    if (n > 0) issue(0);
    if (n > 1) issue(1);
    if (n > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Dw1Ring::VM_PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (role == 0) {
#pragma unroll 1
    for (int i = 0; i <= n; ++i) {
      TRACE1(1);
      if (i < n) produce(i, 0);
      TRACE1(2);
      __syncthreads();
      TRACE1(3);
      if (i < n) produce(i, 1);
      TRACE1(5);
      __syncthreads();
      TRACE1(7);
    }
  } else if (role == 1) {
#pragma unroll 1
    for (int i = 0; i <= n; ++i) {
      TRACE1(1);
      if (i >= 1) consume(i - 1, std::integral_constant<int, 1>{});
      TRACE1(2);
      __syncthreads();
      TRACE1(3);
      if (i < n) consume(i, std::integral_constant<int, 0>{});
      TRACE1(5);
      __syncthreads();
      TRACE1(7);
    }
  } else {
#pragma unroll 1
    for (int i = 0; i <= n; ++i) {
      TRACE1(1);
      __syncthreads();
      TRACE1(3);
      if (i + 2 < n) issue(i + 2);
      TRACE1(4);
      if (i + 2 < n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Dw1Ring::VM_PER_TILE) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      TRACE1(6);
      __syncthreads();
      TRACE1(7);
    }
  }
  float* const dwp = a.dw1p + (size_t)blockIdx.x * (H * H + H);  // its own partials: [W_1 | b_1] per workgroup
  TRACE1(101);
  if (role == 1) {
#pragma unroll
    for (int rbi = 0; rbi < 2; ++rbi) {
      const int rb = 2 * (v >> 1) + rbi;
#pragma unroll
      for (int cbi = 0; cbi < 2; ++cbi) {
        const int cb = 2 * (v & 1) + cbi;
#pragma unroll
        for (int r = 0; r < 16; ++r) dwp[(size_t)(32 * rb + rowmap(r, hi)) * H + 32 * cb + j] = acc[rbi][cbi][r];
      }
      if ((v & 1) == 0) {
        const float t = db[rbi] + __shfl_xor(db[rbi], 32, 64);
        if (hi == 0) dwp[H * H + 32 * rb + j] = t;
      }
    }
  }
#if defined(RENI_TRACE_DW1)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TRACE1(102);
#if RENI_TRACE_DW1 == 2
  if (a.trace != nullptr && tid == 0 && blockIdx.x < 512) {
    a.trace[2 * blockIdx.x] = (long long)wg_t0;
    a.trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
  }
#else
  if (trace_on) {
    for (int k = lane; k < trace_n; k += 64) a.trace[k] = (long long)trace_lds[k];
  }
#endif
#endif
}
#ifdef RENI_TU_CORE
template __global__ void k_reni_dw1_ring<128>(const MainArgs);
#endif


