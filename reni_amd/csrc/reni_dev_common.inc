// reni_dev_common.inc -- precision policies, LDS geometry and the helpers every fused kernel shares
// Part of reni_device.inc (included there, inside namespace reni; never compiled on its own).


// Row (within a 32-row block) held by accumulator register r of a 32x32 MFMA result in a lane
// of the upper (hi=1) or lower (hi=0) half-wave.  (cdna_hip_programming.md section 3.)
DEV constexpr int rowmap(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ------------------------------------------------------------------------------------------
// precision policies
// ------------------------------------------------------------------------------------------
struct PolF32 {
  static constexpr bool BF = false;
  static constexpr int FRAGB = 4;        // bytes per lane of one A/B fragment
  static constexpr int KF = 2;           // features contracted per MFMA (k-step)
  static constexpr int TS = 2;           // samples contracted per MFMA in the dW GEMMs
  static constexpr int WPS = 1;          // waves per SIMD to compile for
  static constexpr int HEAD_BWD_KS = 3;  // k-steps that cover the 3 real head outputs
  static constexpr int STASH_CH_PER_RB = 4;  // 16-byte chunks per lane per 32-feature block
  using Frag = float;
  static DEV f32x16 mfma(Frag a, Frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
  // Wait out the write-back of the last MFMA of a chain before anything else may touch its result.
  // hipcc's own hazard padding cannot be relied on across branches (ROCm 7.2: it counts a taken
  // s_cbranch as a wait state and, with an MFMA at the end of a block, was seen to place the pad AFTER
  // the first read of the result: H = 256 bf16 head dW, nondeterministic rows).  The generic kernels
  // therefore end every chain with their own pad; tests/test_build_audit.py checks the emitted ISA.
  static DEV void drain() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 3");  // 16-pass XDL: 18 states (+2)
    __builtin_amdgcn_sched_barrier(0);
  }
};
struct PolBF16 {
  static constexpr bool BF = true;
  static constexpr int FRAGB = 16;
  static constexpr int KF = 16;
  static constexpr int TS = 16;
  static constexpr int WPS = 2;
  static constexpr int HEAD_BWD_KS = 1;
  static constexpr int STASH_CH_PER_RB = 2;
  using Frag = bf16x8;
  static DEV f32x16 mfma(Frag a, Frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static DEV void drain() {  // see PolF32::drain
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 11");  // 8-pass XDL: 12 states
    __builtin_amdgcn_sched_barrier(0);
  }
};

// feature index (within the layer input) that k-slot (ks, hi, e) of a fragment stands for.
// It is the order in which a D-layout register file enumerates features, so that accumulators
// can be fed back as B operands without any data movement.
template <class Pol>
__host__ __device__ constexpr int kfeat(int ks, int hi, int e) {
  if (Pol::BF) return 16 * ks + (e & 3) + 8 * (e >> 2) + 4 * hi;
  return 32 * (ks >> 4) + ((ks & 15) & 3) + 8 * ((ks & 15) >> 2) + 4 * hi;
}

// LDS geometry ------------------------------------------------------------------------------
template <class Pol, int H>
struct Geo {
  static constexpr int NRB = H / 32;
  static constexpr int NKS = H / Pol::KF;                       // k-steps of an H-wide contraction
  static constexpr int IMG_HID = NRB * NKS * 64 * Pol::FRAGB;   // hidden layer image (fwd or bwd)
  static constexpr int IMG_HF = 1 * NKS * 64 * Pol::FRAGB;      // head forward image
  static constexpr int IMG_HB = NRB * Pol::HEAD_BWD_KS * 64 * Pol::FRAGB;  // head backward image
  static constexpr int BIAS_HID = H * 4;
  static constexpr int BIAS_HEAD = 32 * 4;
  // a hidden image is staged into LDS CH_RB row blocks at a time (the whole layer up to H = 128)
  static constexpr int CH_RB = (H > 128) ? 2 : NRB;
  static constexpr int NCHUNK = NRB / CH_RB;
  static constexpr int CHUNK_BYTES = CH_RB * NKS * 64 * Pol::FRAGB;
  // waves whose samples share one dW transposition round
  static constexpr int ROUND_WAVES = Pol::BF ? (H > 128 ? 2 : 4) : 1;
  static constexpr int ROUND_SAMPLES = 32 * ROUND_WAVES;
  // transposition images: bf16 [feature][sample] rows padded by 16 B; fp32 [sample][feature+1]
  static constexpr int T_ROWB = ROUND_SAMPLES * 2 + 16;
  static constexpr int T_BYTES = Pol::BF ? (H * T_ROWB) : (ROUND_SAMPLES * (H + 1) * 4);
  static constexpr int T_BYTES_AL = (T_BYTES + 255) & ~255;
  static constexpr int WB_A = CHUNK_BYTES > T_BYTES_AL ? CHUNK_BYTES : T_BYTES_AL;
  static constexpr int WB_B = IMG_HF > IMG_HB ? IMG_HF : IMG_HB;
  static constexpr int WB_RAW = WB_A > WB_B ? WB_A : WB_B;
  static constexpr int WB_BYTES = (WB_RAW + 255) & ~255;
  static constexpr int BIAS_LDS = (BIAS_HID + 255) & ~255;      // the layer's bias lives after the images
  // chunked layers (H = 256): a second chunk buffer, filled by LDS-DMA while the first is multiplied
  static constexpr int WB1_BYTES = (NCHUNK > 1 && Pol::BF) ? CHUNK_BYTES : 0;  // (fp32 chunks are 64 KB: no room)
  static constexpr int LDS_BYTES = WB_BYTES + T_BYTES_AL + BIAS_LDS + WB1_BYTES;
  // FiLM kernels append: two (freq, phase) slots [2][2][H] and the d(freq) scratch [NRB + 1][H]
  static constexpr int FILM_FL = 2 * 2 * H * 4;
  static constexpr int FILM_LDS = FILM_FL + (NRB + 1) * H * 4;
  static constexpr int STASH_CH = NRB * Pol::STASH_CH_PER_RB;   // 16-B chunks per lane per layer
  static constexpr int STASH_LAYER_BYTES = STASH_CH * 256 * 16;
};

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
// sum over the 64 lanes, returned to all of them.  DPP adds within each row of 16, row broadcasts across the rows
// (gfx9 row_bcast15 / row_bcast31), one readlane: ~10 instructions; six __shfl_xor are six ds_bpermute round trips
DEV float wave_sum(float x) {
  auto step = [&](auto ctrl, auto rmask) {
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value,
                                                                decltype(rmask)::value, 0xf, true));
  };
  using std::integral_constant;
  step(integral_constant<int, 0xB1>{}, integral_constant<int, 0xf>{});   // quad_perm [1,0,3,2]
  step(integral_constant<int, 0x4E>{}, integral_constant<int, 0xf>{});   // quad_perm [2,3,0,1]
  step(integral_constant<int, 0x141>{}, integral_constant<int, 0xf>{});  // row_half_mirror
  step(integral_constant<int, 0x140>{}, integral_constant<int, 0xf>{});  // row_mirror: every lane has its row's sum
  step(integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{});  // row_bcast15 -> rows 1, 3
  step(integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{});  // row_bcast31 -> rows 2, 3: lane 63 has it all
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}


// sin and cos of an fp32 argument, ~1 ulp for |x| < 1e4: three-term Cody-Waite reduction by pi/2
// with FMAs, then degree-9 / degree-8 minimax polynomials on [-pi/4, pi/4].  Used by the fp32
// (parity-grade) kernels instead of the library sinf/cosf, whose huge-argument slow path costs
// scratch memory and a loop.
DEV void sincos_f32(float x, float& s, float& c) {
  const float kf = rintf(x * 0.63661977236758134f);
  float r = __builtin_fmaf(-kf, 1.57079637050628662109375f, x);
  r = __builtin_fmaf(-kf, -4.37113900018624283e-8f, r);
  r = __builtin_fmaf(-kf, -1.71512449e-15f, r);
  const float r2 = r * r;
  float ps = __builtin_fmaf(r2, 2.7557314297e-06f, -1.9841270114e-04f);
  ps = __builtin_fmaf(ps, r2, 8.3333337680e-03f);
  ps = __builtin_fmaf(ps, r2, -1.6666667163e-01f);
  const float sr = __builtin_fmaf(ps * r2, r, r);
  float pc = __builtin_fmaf(r2, -2.7557314297e-07f, 2.4801587642e-05f);
  pc = __builtin_fmaf(pc, r2, -1.3888889225e-03f);
  pc = __builtin_fmaf(pc, r2, 4.1666667908e-02f);
  const float cr = __builtin_fmaf(pc * r2, r2, __builtin_fmaf(-0.5f, r2, 1.0f));
  const int q = (int)kf;
  const float s0 = (q & 1) ? cr : sr;
  const float c0 = (q & 1) ? sr : cr;
  s = (q & 2) ? -s0 : s0;
  c = ((q + 1) & 2) ? -c0 : c0;
}
DEV float sin_f32(float x) { float s, c; sincos_f32(x, s, c); return s; }
DEV float cos_f32(float x) { float s, c; sincos_f32(x, s, c); return c; }

DEV void stage_to_lds(char* dst, const char* src, int bytes, int tid) {
  for (int o = tid * 16; o < bytes; o += 256 * 16) *(u32x4*)(dst + o) = *(const u32x4*)(src + o);
}

template <class Pol, int NRB_OUT>
DEV void acc_init_bias(f32x16 (&acc)[NRB_OUT], const float* bias_lds, int hi) {
#pragma unroll
  for (int rb = 0; rb < NRB_OUT; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rb][r] = bias_lds[32 * rb + rowmap(r, hi)];
}

template <int NRB_OUT>
DEV void acc_zero(f32x16 (&acc)[NRB_OUT]) {
#pragma unroll
  for (int rb = 0; rb < NRB_OUT; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
}

// D[32*rbo.., sample] += sum_k Wimg[rbo][k] * vin[k]  for the wave's 32 samples.
// vin is a D-layout register file (lane = sample, register = feature).
// bf16: the B operands of a layer, packed once (gemm_lds_bop below takes them; the chunked layers of H = 256 used to convert the whole
// fp32 register file again for every chunk, which kept 128 fp32 + 64 packed registers alive through the GEMM and left hipcc ONE
// fragment register: every MFMA waited out its own ds_read_b128 -- ~100 cycles per 33-cycle MFMA, profiles/r04_h256.md)
template <int NRB_IN, int NKS_USE>
DEV void pack_bop(const float (&vin)[NRB_IN][16], bf16x8 (&bop)[NKS_USE]) {
#pragma unroll
  for (int ks = 0; ks < NKS_USE; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) bop[ks][e] = (__bf16)vin[ks >> 1][(ks & 1) * 8 + e];
}
// acc[rbo] += image[rbo][ks] . bop[ks]: the A fragments are requested PF MFMAs ahead of their use
template <int NRB_OUT, int NKS_USE>
DEV void gemm_lds_bop(const char* wb, const bf16x8 (&bop)[NKS_USE], f32x16 (&acc)[NRB_OUT], int lane) {
  constexpr int N = NKS_USE * NRB_OUT;
  constexpr int PF = N >= 4 ? 4 : N;
  auto fa = [&](int i) { const int ks = i / NRB_OUT, rbo = i % NRB_OUT; return *(const bf16x8*)(wb + ((rbo * NKS_USE + ks) * 64 + lane) * 16); };
  bf16x8 q[PF];
#pragma unroll
  for (int d = 0; d < PF; ++d) q[d] = fa(d);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bf16x8 a = q[i % PF];
    if (i + PF < N) q[i % PF] = fa(i + PF);
    // (fences: left to itself hipcc's scheduler sinks every fragment read to just in front of its MFMA -- one fragment register,
    // one LDS round trip per MFMA -- to save registers it has)
    __builtin_amdgcn_sched_barrier(0);
    acc[i % NRB_OUT] = PolBF16::mfma(a, bop[i / NRB_OUT], acc[i % NRB_OUT]);
    __builtin_amdgcn_sched_barrier(0);
  }
  PolBF16::drain();
}
template <class Pol, int NRB_OUT, int NRB_IN, int NKS_USE>
DEV void gemm_lds(const char* wb, const float (&vin)[NRB_IN][16], f32x16 (&acc)[NRB_OUT], int lane) {
  if constexpr (Pol::BF) {
    bf16x8 bop[NKS_USE];
    pack_bop<NRB_IN, NKS_USE>(vin, bop);
    gemm_lds_bop<NRB_OUT, NKS_USE>(wb, bop, acc, lane);
    return;
  } else {
#pragma unroll
    for (int ks = 0; ks < NKS_USE; ++ks)
#pragma unroll
      for (int rbo = 0; rbo < NRB_OUT; ++rbo) {
        float a = *(const float*)(wb + ((rbo * NKS_USE + ks) * 64 + lane) * 4);
        acc[rbo] = PolF32::mfma(a, vin[ks >> 4][ks & 15], acc[rbo]);
      }
  }
  Pol::drain();
}

// The bf16 kernels stash a sine argument as an fp16 number of revolutions in [0, 1]: two per dword, packed
// by ONE v_cvt_pk_f16_f32 and unpacked by ONE v_cvt_f32_f16 (the high half through SDWA) -- a 16-bit integer
// phase cost three VALU per unpack, and the backward pass unpacks 128 per layer and lane.  Angle resolution
// 2 pi 2^-12 = 1.5e-3 rad, of the order of the bf16 rounding of the values it multiplies.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
DEV unsigned phase_pack(float t0, float t1) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{t0, t1}, f16x2)); }
DEV float phase_lo(unsigned w) { return (float)__builtin_bit_cast(f16x2, w)[0]; }
DEV float phase_hi(unsigned w) { return (float)__builtin_bit_cast(f16x2, w)[1]; }
// (r0, r1) = (g0, g1) * cos(2 pi * the two fp16 phases of w): v_cos_f16 reads either half of the word directly and
// v_fma_mix_f32 multiplies the fp16 cosine into the fp32 gradient -- no unpacking conversion (hipcc turns the plain
// C++ form into cos, cvt, pk_mul).  One instruction sits between each cosine and its use: a transcendental result
// needs one wait state before a VALU reads it, and hipcc does not look into asm statements.
DEV void cos_mul2(unsigned w, float g0, float g1, float& r0, float& r1) {
  unsigned c0, c1;
  asm("v_cos_f16_e32 %0, %4\n\t"
      "v_cos_f16_sdwa %1, %4 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t"
      "v_fma_mix_f32 %2, %0, %5, 0 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mix_f32 %3, %1, %6, 0 op_sel_hi:[1,0,0]"
      : "=&v"(c0), "=&v"(c1), "=&v"(r0), "=&v"(r1) : "v"(w), "v"(g0), "v"(g1));
}

// the same, packed: one VOLATILE statement (cosines, products, bf16 pack) that keeps its place among the asm MFMAs -- left to hipcc
// the packing converts sink to the MFMA that reads the operand, inside the two wait states a VALU write needs in front of it
// (tests/isa_audit.py::valu_to_mfma)
DEV unsigned cos_mul2_pk(unsigned w, float g0, float g1) {
  unsigned c0, c1, pk;
  asm volatile("v_cos_f16_e32 %0, %3\n\t"
               "v_cos_f16_sdwa %1, %3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t"
               "v_fma_mix_f32 %0, %0, %4, 0 op_sel_hi:[1,0,0]\n\t"
               "v_fma_mix_f32 %1, %1, %5, 0 op_sel_hi:[1,0,0]\n\t"
               "v_cvt_pk_bf16_f32 %2, %0, %1"
               : "=&v"(c0), "=&v"(c1), "=&v"(pk) : "v"(w), "v"(g0), "v"(g1));
  return pk;
}

// v: pre-activation a (in)  ->  h = sin(omega a) (out); the sine argument is stashed for backward.
// FiLM (fl != nullptr, LDS [2][H] = freq, phase of this layer and image): h = sin(freq . a + phase)
// (reference FiLMLayer.forward, src/models/RENI.py:515-519); the bf16 stash holds the full angle, the fp32
// stash the pre-activation a.
template <class Pol, int NRB, bool STASH, bool FILM = false>
DEV void act_forward(float (&v)[NRB][16], float omega, char* stash_layer, int tid, const float* fl = nullptr,
                     int H = 0) {
  const int hi = (tid & 63) >> 5;
  if constexpr (Pol::BF) {
    const float sc = omega * 0.15915494309189535f;  // argument in revolutions
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      float q[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float th;
        if constexpr (FILM) {
          const int f = 32 * rb + rowmap(r, hi);
          th = __builtin_amdgcn_fractf(__builtin_fmaf(v[rb][r], fl[f] * 0.15915494309189535f, fl[H + f] * 0.15915494309189535f));
        } else {
          th = __builtin_amdgcn_fractf(v[rb][r] * sc);
        }
        q[r] = th;
        v[rb][r] = __builtin_amdgcn_sinf(th);
      }
      if constexpr (STASH) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          u32x4 w;
#pragma unroll
          for (int d = 0; d < 4; ++d) w[d] = phase_pack(q[8 * c + 2 * d], q[8 * c + 2 * d + 1]);
          *(u32x4*)(stash_layer + ((rb * 2 + c) * 256 + tid) * 16) = w;
        }
      }
    }
  } else {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      if constexpr (STASH) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f32x4 w = {v[rb][4 * c], v[rb][4 * c + 1], v[rb][4 * c + 2], v[rb][4 * c + 3]};
          *(f32x4*)(stash_layer + ((rb * 4 + c) * 256 + tid) * 16) = w;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (FILM) {
          const int f = 32 * rb + rowmap(r, hi);
          v[rb][r] = sin_f32(__builtin_fmaf(fl[f], v[rb][r], fl[H + f]));
        } else {
          v[rb][r] = sin_f32(omega * v[rb][r]);
        }
      }
    }
  }
}

// Reload a layer's stash; WHAT = 0: cos(omega a) * scale * g (in place on g), WHAT = 1: sin(omega a) -> out.
// FiLM (fl != nullptr): the angle is freq . a + phase; WHAT = 0 then yields g . cos(angle) WITHOUT the
// frequency factor (the caller needs both g_theta and freq . g_theta).
template <class Pol, int NRB, int WHAT, bool FILM = false>
DEV void act_replay(float (&x)[NRB][16], const f32x16* g, float omega, float scale,
                    const char* stash_layer, int tid, const float* fl = nullptr, int H = 0) {
  const int hi = (tid & 63) >> 5;
  if constexpr (FILM) scale = (fl != nullptr) ? 1.f : scale;
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) {
    if constexpr (Pol::BF) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 w = *(const u32x4*)(stash_layer + ((rb * 2 + c) * 256 + tid) * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float t0 = phase_lo(w[d]), t1 = phase_hi(w[d]);
          const int r = 8 * c + 2 * d;
          if constexpr (WHAT == 0) {
            x[rb][r] = g[rb][r] * scale * __builtin_amdgcn_cosf(t0);
            x[rb][r + 1] = g[rb][r + 1] * scale * __builtin_amdgcn_cosf(t1);
          } else {
            x[rb][r] = __builtin_amdgcn_sinf(t0);
            x[rb][r + 1] = __builtin_amdgcn_sinf(t1);
          }
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f32x4 w = *(const f32x4*)(stash_layer + ((rb * 4 + c) * 256 + tid) * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int r = 4 * c + d;
          float arg = omega * w[d];
          if constexpr (FILM) {
            if (fl != nullptr) {
              const int f = 32 * rb + rowmap(r, hi);
              arg = __builtin_fmaf(fl[f], w[d], fl[H + f]);
            }
          }
          if constexpr (WHAT == 0) x[rb][r] = g[rb][r] * scale * cos_f32(arg);
          else x[rb][r] = sin_f32(arg);
        }
      }
    }
  }
}

// ---- transposition through LDS for the K = samples GEMMs ------------------------------------
template <class Pol, int H, int NB>
DEV void t_write(char* T, const float (&x)[NB][16], int wslot, int hi, int j) {
  using G = Geo<Pol, H>;
#pragma unroll
  for (int rb = 0; rb < NB; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * rb + rowmap(r, hi);
      if constexpr (Pol::BF) {
        *(__bf16*)(T + f * G::T_ROWB + (wslot * 32 + j) * 2) = (__bf16)x[rb][r];
      } else {
        *(float*)(T + (j * (32 * NB + 1) + f) * 4) = x[rb][r];
      }
    }
}

template <class Pol, int H, int NB>
DEV typename Pol::Frag t_read(const char* T, int blk, int ks, int i, int khi) {
  using G = Geo<Pol, H>;
  if constexpr (Pol::BF) {
    return *(const bf16x8*)(T + (32 * blk + i) * G::T_ROWB + (16 * ks + 8 * khi) * 2);
  } else {
    return *(const float*)(T + ((2 * ks + khi) * (32 * NB + 1) + 32 * blk + i) * 4);
  }
}

// sum of the k-elements of one fragment, added to c.  bf16: four v_dot2c_f32_bf16 against (1, 1) -- the
// unpack-and-add form cost ~24 VALU per fragment, the largest filler of the dW GEMMs
template <class Pol>
DEV float frag_sum(typename Pol::Frag a, float c = 0.f) {
  if constexpr (Pol::BF) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 one = {(__bf16)1.f, (__bf16)1.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[2 * e], a[2 * e + 1]}, one, c, false);
    return c;
  } else {
    return c + a;
  }
}

enum { DW_HIDDEN = 0, DW_HEAD = 1, DW_L0 = 2 };

// MFMA with the accumulator PINNED to the AGPR half ("a") or the VGPR half ("v") of the register
// file.  hipcc puts every MFMA accumulator of a kernel into AGPRs (256 = sixteen 32x32 tiles); the
// persistent training kernel needs twenty-odd live tiles, so it pins them by hand.  Operands come
// straight from ds_read (the compiler's s_waitcnt covers them) and the accumulator is only ever
// touched by these statements, so no MFMA hazard crosses the asm boundary (cdna guide, 5.7).
// ---- hand-owned AGPRs ------------------------------------------------------------------------------
// The persistent training kernel owns ALL 256 AGPRs as sixteen literal 32x32 fp32 tiles a[16t:16t+15]
// (t = 4*(layer-2) + column block): the dW accumulators of hidden layers 2..5.  The compiler never sees
// them as values -- every statement that touches them names the registers in its text and lists all AGPRs
// as clobbers (which also makes the kernel descriptor allocate them); the library is built with
// -amdgpu-spill-vgpr-to-agpr=0 and every MFMA of that kernel is an asm statement, so no compiler-generated
// instruction ever reads or writes an AGPR (checked on the emitted ISA by tests/test_build_audit.py).
//
// hipcc neither pads hazards inside an asm statement nor knows that the statement is an MFMA, so the wait
// states are part of the string: `s_nop 4` in front covers a VALU write of an operand just before; LAST =
// the final MFMA of a chain is followed by 20 wait states so that a read of the result never overtakes the
// 8-pass XDL write-back.
#define RENI_A10(n) "a" #n "0", "a" #n "1", "a" #n "2", "a" #n "3", "a" #n "4", "a" #n "5", "a" #n "6", "a" #n "7", "a" #n "8", "a" #n "9"
#define RENI_AGPR_ALL                                                                                       \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", RENI_A10(1), RENI_A10(2), RENI_A10(3),         \
      RENI_A10(4), RENI_A10(5), RENI_A10(6), RENI_A10(7), RENI_A10(8), RENI_A10(9), RENI_A10(10),            \
      RENI_A10(11), RENI_A10(12), RENI_A10(13), RENI_A10(14), RENI_A10(15), RENI_A10(16), RENI_A10(17),      \
      RENI_A10(18), RENI_A10(19), RENI_A10(20), RENI_A10(21), RENI_A10(22), RENI_A10(23), RENI_A10(24),      \
      "a250", "a251", "a252", "a253", "a254", "a255"

// Wait states in front of an asm MFMA: a VALU write of a VGPR needs 2 of them before an MFMA reads that VGPR
// as SrcA / SrcB / SrcC.  FIRST = the first MFMA of a chain (its accumulator was just initialised by VALU or
// loaded) carries `s_nop 1`; the others carry none -- a pad between MFMAs costs ~28 cycles each -- and
// tests/isa_audit.py::valu_to_mfma proves on the emitted ISA that no VALU write sits within 2 states of them.
// wait states behind the LAST MFMA of a chain before anything reads its result: an 8-pass XDL op on gfx950 needs 12
// (LLVM's GFX940_XDL_N_PassWriteVgprVALUReadWaitStates: passes + 3 + 1; the figure hipcc pads its own MFMAs with, and the
// one tests/isa_audit.py enforces).  Twenty, as first written, cost 8 dead states on each of ~60 chains per tile.
#define RENI_MFMA_TAIL "s_nop 11"
// TAILN >= 0: a SHORTER pad, `s_nop TAILN`, at a site where the instructions that follow on every path are independent of the
// result and make up the rest of the twelve states -- each such site is proven by tests/isa_audit.py on the emitted ISA (the pads
// cost 0.5 % of the kernel per four states over the ~45 chains of a tile: profiles/r04_variants.md)
template <int T, bool LAST, int TAILN = -1>
DEV void mfma_bf16_agpr_tile(bf16x8 a, bf16x8 b) {
  if constexpr (LAST && TAILN >= 0)
    asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]\n\ts_nop %c4"
                 :: "v"(a), "v"(b), "i"(16 * T), "i"(16 * T + 15), "i"(TAILN) : RENI_AGPR_ALL);
  else if constexpr (LAST)
    asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]\n\t" RENI_MFMA_TAIL
                 :: "v"(a), "v"(b), "i"(16 * T), "i"(16 * T + 15) : RENI_AGPR_ALL);
  else
    asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]"
                 :: "v"(a), "v"(b), "i"(16 * T), "i"(16 * T + 15) : RENI_AGPR_ALL);
}
template <int N>
DEV void agpr_zero_one() { asm volatile("v_accvgpr_write_b32 a[%c0], 0" :: "i"(N) : RENI_AGPR_ALL); }
template <int... I>
DEV void agpr_zero_seq(std::integer_sequence<int, I...>) { (agpr_zero_one<I>(), ...); }
template <int BASE, int... I>
DEV void agpr_zero_range(std::integer_sequence<int, I...>) { (agpr_zero_one<BASE + I>(), ...); }
template <int N>
DEV float agpr_read_one() { float x; asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "i"(N)); return x; }
template <int T, int... R>
DEV f32x16 agpr_read_tile_seq(std::integer_sequence<int, R...>) { f32x16 v = {agpr_read_one<16 * T + R>()...}; return v; }
template <int T>
DEV f32x16 agpr_read_tile() { return agpr_read_tile_seq<T>(std::make_integer_sequence<int, 16>{}); }

template <bool LAST, bool FIRST = true, int TAILN = -1>
DEV void mfma_bf16_pin_v(f32x16& acc, bf16x8 a, bf16x8 b) {
  if constexpr (LAST && !FIRST && TAILN >= 0)
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\ts_nop %c3" : "+v"(acc) : "v"(a), "v"(b), "i"(TAILN));
  else if constexpr (LAST && FIRST)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\t" RENI_MFMA_TAIL : "+v"(acc) : "v"(a), "v"(b));
  else if constexpr (LAST)
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\t" RENI_MFMA_TAIL : "+v"(acc) : "v"(a), "v"(b));
  else if constexpr (FIRST)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// first MFMA of a chain whose accumulator starts at zero: SrcC is the inline constant, no register initialisation
template <bool LAST>
DEV void mfma_bf16_zero_v(f32x16& acc, bf16x8 a, bf16x8 b) {
  if constexpr (LAST)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0\n\t" RENI_MFMA_TAIL : "=&v"(acc) : "v"(a), "v"(b));
  else
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}

// K = samples GEMM from the transposed LDS images: acc[m] += rows-block x cols-block over one round
// PIN: 0 = compiler-allocated accumulator, 1 = pinned to AGPRs, 2 = pinned to VGPRs (bf16 only)
template <class Pol, int H, int NBR, int NBC, int KIND, int MYB, int PIN = 0, int M0 = 0>
DEV void dw_gemm(const char* TA, const char* TB, f32x16 (&acc)[MYB], float& dbacc, int wave, int lane,
                 float* dbacc2 = nullptr) {  // dbacc2: bias sum of the wave's second row block (NBR == 8)
  using G = Geo<Pol, H>;
  using Frag = typename Pol::Frag;
  constexpr int NBLK = NBR * NBC;
  constexpr int NKS_T = G::ROUND_SAMPLES / Pol::TS;
  const int hi = lane >> 5, j = lane & 31;
  if constexpr (PIN == 0) {
#pragma unroll
    for (int ks = 0; ks < NKS_T; ++ks) {
#pragma unroll
      for (int m = 0; m < MYB; ++m) {
        const int blk = wave + 4 * (M0 + m);
        if (blk < NBLK) {
          const int rbo = blk % NBR, cb = blk / NBR;
          Frag fa = t_read<Pol, H, NBR>(TA, rbo, ks, j, hi);
          Frag fb = t_read<Pol, H, NBC>(TB, cb, ks, j, hi);
          acc[m] = Pol::mfma(fa, fb, acc[m]);
          // bias sums: the owner test is a 0/1 factor, never a branch -- hipcc counts a taken s_cbranch
          // as one of the 12 wait states between an 8-pass MFMA and the first read of its result, and a
          // wave that skipped the sum read stale accumulator rows (H = 256 head dW, waves 1..3)
          if (KIND == DW_HIDDEN && M0 + m == 0) {  // (m is an unrolled constant)
            if (NBR >= 4) dbacc += frag_sum<Pol>(fa);
            else dbacc += (cb == 0 ? 1.f : 0.f) * frag_sum<Pol>(fa);
          }
          if (KIND == DW_HIDDEN && NBR > 4 && M0 + m == 1 && dbacc2 != nullptr) *dbacc2 += frag_sum<Pol>(fa);
          if (KIND == DW_HEAD && M0 + m == 0) dbacc += (wave == 0 ? 1.f : 0.f) * frag_sum<Pol>(fb);
        }
      }
    }
    Pol::drain();
  } else {
    // pinned accumulators (persistent training kernel: NBR == 4, every wave owns row block `wave`
    // and all MYB column blocks).  Fragments are fetched one k-step ahead and the schedule is fenced
    // per k-step so that no more than two k-steps of fragments are ever live.
    static_assert(NBLK == 4 * MYB && M0 == 0, "pinned form: every wave owns exactly MYB blocks");
#pragma unroll
    for (int ks = 0; ks < NKS_T; ++ks) {
#pragma unroll
      for (int m = 0; m < MYB; ++m) {
        const int blk = wave + 4 * m;
        Frag fa = t_read<Pol, H, NBR>(TA, blk % NBR, ks, j, hi);
        Frag fb = t_read<Pol, H, NBC>(TB, blk / NBR, ks, j, hi);
        if (ks == NKS_T - 1 && m == MYB - 1) mfma_bf16_pin_v<true>(acc[m], fa, fb);
        else mfma_bf16_pin_v<false>(acc[m], fa, fb);
        if (KIND == DW_HIDDEN && m == 0 && (wave / NBR) == 0) dbacc += frag_sum<Pol>(fa);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// write the accumulated block(s) to the flat-layout destination (plain store when `first`, else +=)
// rscale (FiLM, LDS, indexed by output feature): every row of the block and the bias sum are multiplied by
// rscale[row] -- the accumulators hold g_theta h^T, the weight gradient is diag(freq) g_theta h^T
template <class Pol, int H, int NBR, int NBC, int KIND, int MYB, int M0 = 0, bool DO_W = true, bool DO_B = true>
DEV void dw_flush(const f32x16 (&acc_in)[MYB], float dbacc, float* dst_w, float* dst_b, int ldw, bool first,
                  int wave, int lane, int amode = 0, const float* rscale = nullptr) {
  constexpr int NBLK = NBR * NBC;
  const int hi = lane >> 5, j = lane & 31;
  f32x16 acc[MYB];
#pragma unroll
  for (int m = 0; m < MYB; ++m) {
    acc[m] = acc_in[m];
    if (rscale != nullptr) {
      const int rbo = (wave + 4 * (M0 + m)) % NBR;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][r] *= rscale[32 * rbo + rowmap(r, hi)];
    }
  }
#pragma unroll
  for (int m = 0; m < (DO_W ? MYB : 0); ++m) {
    const int blk = wave + 4 * (M0 + m);
    if (blk < NBLK) {
      const int rbo = blk % NBR, cb = blk / NBR;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * rbo + rowmap(r, hi);
        if constexpr (KIND == DW_HIDDEN) {
          float* p = dst_w + (size_t)row * ldw + 32 * cb + j;
          if (amode == 1) {
            __hip_atomic_fetch_add(p, acc[m][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else if (amode == 2) {
            const float t = acc[m][r] * 4096.f;  // 2^(44-32)
            const float h = floorf(t);
            const unsigned lo = (unsigned)((t - h) * 4294967296.f);
            const unsigned long long q = ((unsigned long long)(unsigned)(int)h << 32) | lo;
            __hip_atomic_fetch_add((unsigned long long*)dst_w + ((size_t)row * ldw + 32 * cb + j), q, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            *p = first ? acc[m][r] : (*p + acc[m][r]);
          }
        } else if constexpr (KIND == DW_HEAD) {
          if (j < 3) {
            float* p = dst_w + (size_t)j * ldw + row;
            *p = first ? acc[m][r] : (*p + acc[m][r]);
          }
        } else {
          // columns 0..4 = (x_hi | 1), 8..11 = x_lo: the per-tile partial keeps their sum, 8 floats per row
          const float lo = __shfl_down(acc[m][r], 8, 64);
          if (j < 8) dst_w[(size_t)row * 8 + j] = acc[m][r] + ((j < 4) ? lo : 0.f);
        }
      }
    }
  }
  if constexpr (!DO_B) {
    return;
  } else if constexpr (KIND == DW_HIDDEN) {
    dbacc += __shfl_xor(dbacc, 32, 64);
    if (wave < NBR && wave < NBLK && hi == 0) {
      if (rscale != nullptr) dbacc *= rscale[32 * (wave % NBR) + j];
      float* p = dst_b + 32 * (wave % NBR) + j;
      *p = first ? dbacc : (*p + dbacc);
    }
  } else if constexpr (KIND == DW_HEAD) {
    dbacc += __shfl_xor(dbacc, 32, 64);
    if (wave == 0 && hi == 0 && j < 3) {
      float* p = dst_b + j;
      *p = first ? dbacc : (*p + dbacc);
    }
  }
}

// The QUAD-ROW layout of a hidden layer's H x H partial (the L0X training instance only; the bias behind it, the head, k_reni_l0_ring's
// layer-1 partials and every other writer keep the flat layout): element (row, col) lives at word ((row / 4) * H + col) * 4 + row % 4 of the layer's
// slice.  Registers 4 i .. 4 i + 3 of a 32 x 32 accumulator block are four consecutive rows of one column (rowmap), so a lane's sixteen
// values leave in four 16-byte stores, and a wave instruction covers two 512-byte runs instead of two 128-byte row pieces.
// The reader is reduce_partials_quad_body (reni_dev_small.inc), which undoes the permutation where it writes the sum.
DEV constexpr unsigned quad_word(int row, int col, int H) { return (unsigned)((((row >> 2) * H + col) << 2) + (row & 3)); }
// dw_flush<.., DW_HIDDEN, MYB>'s plain store (`first`, no atomics, no row scale) of the pinned form -- wave w owns row block w and the
// MYB column blocks -- into a quad-row slice: the same values, the same bias sum, 16-byte stores
template <int H, int NBR, int MYB>
DEV void dw_flush_quad(const f32x16 (&acc)[MYB], float dbacc, float* dst_w, float* dst_b, int wave, int lane) {
  static_assert(NBR == 4 && MYB == H / 32, "pinned form: wave w owns row block w and every column block");
  static_assert(rowmap(4, 0) == 8 && rowmap(3, 1) == 7, "registers 4 i .. 4 i + 3: rows 8 i + 4 hi .. + 3 of the block");
  const int hi = lane >> 5, j = lane & 31;
  float* const base = dst_w + ((size_t)((8 * wave + hi) * H + j) << 2);  // row quad 8 wave + 2 i + hi, column 32 m + j
#pragma unroll
  for (int m = 0; m < MYB; ++m) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *(f32x4*)(base + ((2 * i * H + 32 * m) << 2)) = f32x4{acc[m][4 * i], acc[m][4 * i + 1], acc[m][4 * i + 2], acc[m][4 * i + 3]};
  }
  dbacc += __shfl_xor(dbacc, 32, 64);
  if (hi == 0) dst_b[32 * wave + j] = dbacc;
}

// FiLM extras of a hidden-layer dW phase.  The accumulators hold M = g_theta h^T (g_theta = cos(angle) g_h):
//   d(phase)[f] = sum_s g_theta[f][s]                 (the bias sum)
//   d(freq)[f]  = sum_s g_theta[f][s] a[f][s],  a = W h + b   =  sum_k W[f][k] M[f][k] + b[f] d(phase)[f]
//   dW = diag(freq) M,  db = freq . d(phase)          (row scaling at the flush)
struct FilmDw {
  const float* fl;   // LDS [2][H]: freq, phase of this layer and image
  float* fs;         // LDS scratch [NBC + 1][H]
  const float* W;    // global fp32 W_l [H][H] and b_l [H]
  const float* b;
  float* out;        // global [2][H]: this tile's d(freq), d(phase)
  int do_w;          // also flush dW / db (0 when the decoder is frozen)
};

// lane-group sum over the 32 lanes that share `hi`
DEV float half_sum(float t) {
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// dM[row-feature][col-feature] (+)= sum over the tile's 128 samples rows[.][s] * cols[.][s].
//   DW_HIDDEN: rows = g_a (layer outputs), cols = h_{l-1}; flushed to dW_l [out][in] and db_l
//   DW_HEAD  : rows = h_L, cols = g_y (3 real);            flushed to dW_out[c][feature], db_out
//   DW_L0    : rows = g_a0, cols = (x_hi[5], x_lo[4]);     stored to the per-tile dA partial
// dbg: ablation mask for profiling experiments (1 = no flush, 2 = no GEMM, 4 = no LDS transposition)
template <class Pol, int H, int NBR, int NBC, int KIND, bool FILM = false>
DEV void dw_phase(char* TA, char* TB, const float (&rows)[NBR][16], const float (&cols)[NBC][16],
                  float* dst_w, float* dst_b, int ldw, bool first, int wave, int lane, int dbg = 0,
                  const FilmDw* fd = nullptr) {
  constexpr int MYB = (NBR * NBC + 3) / 4;
  constexpr int NBLK = NBR * NBC;
  constexpr int NROUND = 4 / Geo<Pol, H>::ROUND_WAVES;
  const int hi = lane >> 5, j = lane & 31;
  const int tid = wave * 64 + lane;
  if constexpr (MYB <= 4) {
    f32x16 acc[MYB];
    acc_zero<MYB>(acc);
    float dbacc = 0.f;
#pragma unroll 1
    for (int round = 0; round < NROUND; ++round) {
      __syncthreads();
      if (wave / Geo<Pol, H>::ROUND_WAVES == round && !(dbg & 4)) {
        t_write<Pol, H, NBR>(TA, rows, wave % Geo<Pol, H>::ROUND_WAVES, hi, j);
        t_write<Pol, H, NBC>(TB, cols, wave % Geo<Pol, H>::ROUND_WAVES, hi, j);
      }
      __syncthreads();
      if (dbg & 2) continue;
      dw_gemm<Pol, H, NBR, NBC, KIND, MYB>(TA, TB, acc, dbacc, wave, lane);
    }
    if (dbg & 1) {
      float keep = dbacc;
#pragma unroll
      for (int m = 0; m < MYB; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) keep += acc[m][r];
      if (keep == 123.456f) dst_w[0] = keep;
      return;
    }
    if constexpr (FILM && KIND == DW_HIDDEN) {
#pragma unroll
      for (int m = 0; m < MYB; ++m) {
        const int blk = wave + 4 * m;
        if (blk < NBLK) {
          const int rbo = blk % NBR, cb = blk / NBR;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = 32 * rbo + rowmap(r, hi);
            const float t = half_sum(acc[m][r] * fd->W[(size_t)row * H + 32 * cb + j]);
            if (j == 0) fd->fs[cb * H + row] = t;
          }
        }
      }
      const float dph = dbacc + __shfl_xor(dbacc, 32, 64);
      if (wave < NBR && wave < NBLK && hi == 0) fd->fs[NBC * H + 32 * wave + j] = dph;
      __syncthreads();
      if (tid < H) {
        float dfr = fd->b[tid] * fd->fs[NBC * H + tid];
#pragma unroll
        for (int cb = 0; cb < NBC; ++cb) dfr += fd->fs[cb * H + tid];
        fd->out[tid] = dfr;
        fd->out[H + tid] = fd->fs[NBC * H + tid];
      }
      if (fd->do_w) dw_flush<Pol, H, NBR, NBC, KIND, MYB>(acc, dbacc, dst_w, dst_b, ldw, first, wave, lane, 0, fd->fl);
    } else {
      dw_flush<Pol, H, NBR, NBC, KIND, MYB>(acc, dbacc, dst_w, dst_b, ldw, first, wave, lane, (dbg >> 8) & 3);
    }
  } else {
    // wide layers (H = 256: 16 blocks per wave): four blocks at a time, every (round, group) result is added
    // to the partial right away -- more += traffic, bounded register use
    static_assert(MYB % 4 == 0, "block groups of four");
    static_assert(NBR == 8, "wide path: a wave owns row blocks w and w + 4");
    float dbacc = 0.f, dbacc2 = 0.f;
    float dfa[FILM ? 2 : 1][16];  // FiLM: sum_k W[row][k] M[row][k] of row blocks w, w + 4 (before the lane sum)
#pragma unroll
    for (int q = 0; q < (FILM ? 2 : 1); ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) dfa[q][r] = 0.f;
    const bool do_w = FILM ? (fd->do_w != 0) : true;
#pragma unroll 1
    for (int round = 0; round < NROUND; ++round) {
      __syncthreads();
      if (wave / Geo<Pol, H>::ROUND_WAVES == round) {
        t_write<Pol, H, NBR>(TA, rows, wave % Geo<Pol, H>::ROUND_WAVES, hi, j);
        t_write<Pol, H, NBC>(TB, cols, wave % Geo<Pol, H>::ROUND_WAVES, hi, j);
      }
      __syncthreads();
      const bool fw = first && round == 0;
      auto group = [&](auto gc) {
        constexpr int M0 = decltype(gc)::value * 4;
        f32x16 acc[4];
        acc_zero<4>(acc);
        dw_gemm<Pol, H, NBR, NBC, KIND, 4, 0, M0>(TA, TB, acc, dbacc, wave, lane, &dbacc2);
        if constexpr (FILM) {
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int rbo = wave + 4 * ((M0 + m) & 1), cb = (M0 + m) >> 1;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              dfa[(M0 + m) & 1][r] += acc[m][r] * fd->W[(size_t)(32 * rbo + rowmap(r, hi)) * H + 32 * cb + j];
          }
        }
        if (do_w) dw_flush<Pol, H, NBR, NBC, KIND, 4, M0, true, false>(acc, 0.f, dst_w, dst_b, ldw, fw, wave, lane, 0,
                                                                        FILM ? fd->fl : nullptr);
      };
      group(std::integral_constant<int, 0>{});
      if constexpr (MYB > 4) group(std::integral_constant<int, 1>{});
      if constexpr (MYB > 8) group(std::integral_constant<int, 2>{});
      if constexpr (MYB > 12) group(std::integral_constant<int, 3>{});
    }
    if constexpr (KIND == DW_HIDDEN) {  // bias gradients of row blocks w and w + 4
      dbacc += __shfl_xor(dbacc, 32, 64);
      dbacc2 += __shfl_xor(dbacc2, 32, 64);
      if constexpr (FILM) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float t = half_sum(dfa[q][r]);
            if (j == 0) fd->fs[32 * (wave + 4 * q) + rowmap(r, hi)] = t;
          }
        if (hi == 0) {
          fd->fs[H + 32 * wave + j] = dbacc;
          fd->fs[H + 32 * (wave + 4) + j] = dbacc2;
        }
        __syncthreads();
        if (tid < H) {
          fd->out[tid] = fd->fs[tid] + fd->b[tid] * fd->fs[H + tid];
          fd->out[H + tid] = fd->fs[H + tid];
        }
        dbacc *= fd->fl[32 * wave + j];
        dbacc2 *= fd->fl[32 * (wave + 4) + j];
      }
      if (hi == 0 && do_w) {
        float* p0 = dst_b + 32 * wave + j;
        float* p1 = dst_b + 32 * (wave + 4) + j;
        *p0 = first ? dbacc : (*p0 + dbacc);
        *p1 = first ? dbacc2 : (*p1 + dbacc2);
      }
    }
  }
}

// bf16 layers whose weight gradient is finished by k_dw_stream (H = 256; FiLM at H >= 128).  This phase only
// builds the two transposed operand images of every round of samples -- g_l from registers, h_{l-1} = sin(phase)
// straight from the stash, sixteen values at a time (never a second 128-register file) -- and copies the
// record (TA | TB, contiguous in LDS) to the stream.
// ONE_BUF (whole-layer weight images, H <= 128): both images pass through the single buffer T1 one after the other,
// so that the other weight buffer may hold the NEXT layer's prefetched image meanwhile (layer_gemm).
template <int H, bool ONE_BUF>
DEV void stream_phase(char* TA, char* TB, const float (&g)[H / 32][16], const char* stash_prev, char* rec_base,
                      int wave, int lane, int tid) {
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  constexpr int NRB = H / 32, NROUND = 4 / G::ROUND_WAVES, REC = 2 * G::T_BYTES_AL;
  static_assert(G::WB_BYTES == G::T_BYTES_AL, "TA | TB contiguous");
  static_assert(!ONE_BUF || NROUND == 1, "one round per tile");
  const int hi = lane >> 5, j = lane & 31;
  auto write_h = [&](char* T, int wslot) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const u32x4 w = *(const u32x4*)(stash_prev + ((rb * 2 + c) * 256 + tid) * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float t0 = phase_lo(w[d]), t1 = phase_hi(w[d]);
          const int r = 8 * c + 2 * d;
          *(__bf16*)(T + (32 * rb + rowmap(r, hi)) * G::T_ROWB + (wslot * 32 + j) * 2) = (__bf16)__builtin_amdgcn_sinf(t0);
          *(__bf16*)(T + (32 * rb + rowmap(r + 1, hi)) * G::T_ROWB + (wslot * 32 + j) * 2) = (__bf16)__builtin_amdgcn_sinf(t1);
        }
      }
  };
  if constexpr (ONE_BUF) {
    char* const T1 = TA;
    __syncthreads();
    t_write<Pol, H, NRB>(T1, g, wave, hi, j);
    __syncthreads();
    for (int o = tid * 16; o < G::T_BYTES_AL; o += 256 * 16) *(u32x4*)(rec_base + o) = *(const u32x4*)(T1 + o);
    __syncthreads();
    write_h(T1, wave);
    __syncthreads();
    for (int o = tid * 16; o < G::T_BYTES_AL; o += 256 * 16) *(u32x4*)(rec_base + G::T_BYTES_AL + o) = *(const u32x4*)(T1 + o);
  } else {
#pragma unroll 1
    for (int round = 0; round < NROUND; ++round) {
      __syncthreads();
      if (wave / G::ROUND_WAVES == round) {
        const int wslot = wave % G::ROUND_WAVES;
        t_write<Pol, H, NRB>(TA, g, wslot, hi, j);
        write_h(TB, wslot);
      }
      __syncthreads();
      char* rec = rec_base + (size_t)round * REC;
      for (int o = tid * 16; o < REC; o += 256 * 16) *(u32x4*)(rec + o) = *(const u32x4*)(TA + o);
    }
  }
}

// ---- LDS-DMA primitives (see dma_image below for why they are inline asm) ----------------------------
// source = wave-uniform base (SGPR pair) + per-lane byte offset (ONE VGPR shared by all pieces): no 64-bit
// per-piece address registers
DEV void glds16(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst_uniform) : "memory");
}
DEV void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ------------------------------------------------------------------------------------------
// the fused kernel
// ------------------------------------------------------------------------------------------
enum { MODE_FWD = 0, MODE_STATS = 1, MODE_FWD_BWD = 2 };

