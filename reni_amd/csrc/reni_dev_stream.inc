// reni_dev_stream.inc -- weight-gradient consumers of the operand streams: k_dw_stream, k_dw_frag, k_dw_frag32 (core translation unit only)
// Part of reni_device.inc (included there, inside namespace reni; never compiled on its own).

// ==========================================================================================
// dW_l = sum over samples of g_l h_{l-1}^T from the operand stream k_reni_main wrote (bf16; H = 128 FiLM, H = 256)
// ==========================================================================================
// One workgroup per CU, persistent over layers and records.  The workgroup's AGPRs hold one layer's accumulator
// (H = 256: all of them -- 4 waves x 16 tiles; wave w owns row blocks w and w + 4, every column block).  A record
// (one round of samples: the g image then the h image, already transposed and padded as the MFMA wants them) is
// copied into a two-slot LDS ring by LDS-DMA while the previous record is multiplied.
// Records are assigned in contiguous ranges.  FILM: the accumulator M = g_theta h^T is per image, so a range is cut
// into per-image runs; at the end of a run  d(phase) = row sums of g_theta,  sum_k W[f][k] M[f][k]  (FilmDw) and
// diag(freq) M (the weight gradient) leave the registers and the accumulator restarts.
template <int H, bool FILM>
__global__ void __launch_bounds__(256, 1) k_dw_stream(const MainArgs a) {
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  constexpr int NRB = H / 32, RPW = NRB / 4;  // row blocks per wave
  constexpr int NROUND = 4 / G::ROUND_WAVES;
  constexpr int REC = 2 * G::T_BYTES_AL;
  constexpr int NPIECE = REC / 1024;
  static_assert(REC % 4096 == 0, "records are whole DMA pieces, four waves");
  static_assert(RPW >= 1, "H >= 128");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  float* const dwp = a.dwp + (size_t)blockIdx.x * a.dwp_per_wg;
  const int nrec = a.n_tiles * NROUND;  // records of one layer
  const int r0 = (int)((long long)blockIdx.x * nrec / gridDim.x), r1 = (int)((long long)(blockIdx.x + 1) * nrec / gridDim.x);
  const int rec_per_image = a.tiles_per_image * NROUND;
  auto issue = [&](int l, int rec, int slot) {
    const char* src = a.dws + ((size_t)(l - 1) * nrec + rec) * REC;
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(smem + slot * REC));
#pragma unroll
    for (int pi = 0; pi < NPIECE / 4; ++pi) glds16(src + (pi * 4 + wave) * 1024, (unsigned)(lane * 16), dst + (pi * 4 + wave) * 1024);
  };
#pragma unroll 1
  for (int l = 1; l <= a.L; ++l) {
    f32x16 acc[RPW * NRB];
    acc_zero<RPW * NRB>(acc);
    float db[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) db[q] = 0.f;
    float* const dw = dwp + a.p_off_w[l];
    float* const dbp = dwp + a.p_off_b[l];
    bool first_flush = true;
    int run = 0;
    // leave the registers: weight-gradient partial (+= after the first run), FiLM row sums of the finished run
    auto flush = [&](int image) {
      Pol::drain();
      float sc[RPW][16];
#pragma unroll
      for (int q = 0; q < RPW; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[q][r] = 1.f;
      if constexpr (FILM) {
        const float* freq = a.film + ((size_t)image * a.L + (l - 1)) * 2 * H;
        const float* W = a.params + a.n_first + a.p_off_w[l];
        float* out = a.dfr + ((size_t)(blockIdx.x * a.kmax + run) * a.L + (l - 1)) * 2 * H;
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
          const int rb = wave + 4 * q;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = 32 * rb + rowmap(r, hi);
            float t = 0.f;
#pragma unroll
            for (int cb = 0; cb < NRB; ++cb) t += acc[q * NRB + cb][r] * W[(size_t)row * H + 32 * cb + j];
            t = half_sum(t);
            if (j == 0) out[row] = t;
            sc[q][r] = freq[row];
          }
          const float dph = db[q] + __shfl_xor(db[q], 32, 64);
          if (hi == 0) out[H + 32 * rb + j] = dph;
        }
        if (tid == 0) a.run_image[blockIdx.x * a.kmax + run] = image;
      }
      if (a.need_dw) {
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
          const int rb = wave + 4 * q;
#pragma unroll
          for (int cb = 0; cb < NRB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float* p = dw + (size_t)(32 * rb + rowmap(r, hi)) * H + 32 * cb + j;
              const float v = acc[q * NRB + cb][r] * sc[q][r];
              *p = first_flush ? v : (*p + v);
            }
          float dbv = db[q] + __shfl_xor(db[q], 32, 64);
          if constexpr (FILM) dbv *= a.film[((size_t)image * a.L + (l - 1)) * 2 * H + 32 * rb + j];
          if (hi == 0) dbp[32 * rb + j] = first_flush ? dbv : (dbp[32 * rb + j] + dbv);
        }
      }
      first_flush = false;
      ++run;
      acc_zero<RPW * NRB>(acc);
#pragma unroll
      for (int q = 0; q < RPW; ++q) db[q] = 0.f;
    };
    int slot = 0;
    if (r0 < r1) issue(l, r0, 0);
#pragma unroll 1
    for (int rec = r0; rec < r1; ++rec, slot ^= 1) {
      dma_wait();
      __syncthreads();  // this record landed (all waves' pieces); the other slot's readers are done
      if (rec + 1 < r1) issue(l, rec + 1, slot ^ 1);
      const char* TA = smem + slot * REC;
      const char* TB = TA + G::T_BYTES_AL;
#pragma unroll
      for (int ks = 0; ks < G::ROUND_SAMPLES / Pol::TS; ++ks) {
        bf16x8 fa[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) fa[q] = t_read<Pol, H, NRB>(TA, wave + 4 * q, ks, j, hi);
#pragma unroll
        for (int cb = 0; cb < NRB; ++cb) {
          const bf16x8 b = t_read<Pol, H, NRB>(TB, cb, ks, j, hi);
#pragma unroll
          for (int q = 0; q < RPW; ++q) acc[q * NRB + cb] = Pol::mfma(fa[q], b, acc[q * NRB + cb]);
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q) db[q] = frag_sum<Pol>(fa[q], db[q]);
      }
      if constexpr (FILM) {
        const int image = rec / rec_per_image;
        if (rec + 1 == r1 || (rec + 1) / rec_per_image != image) flush(image);
      }
    }
    if constexpr (!FILM) flush(0);
    else if (r0 >= r1 && a.need_dw) flush(0);  // (cannot happen: every workgroup owns at least one record)
    __syncthreads();
  }
}
template __global__ void k_dw_stream<128, false>(const MainArgs);
template __global__ void k_dw_stream<128, true>(const MainArgs);

// dW_l for H = 256 from the FRAGMENT stream (MainArgs::gfs): the chain stored g_l as it held it in
// registers and left every tile's phase stash in place; this kernel builds the two transposed operand images of a record
// (one round of 64 samples) in its own LDS -- threads 0..127 place the g values, threads 128..255 compute
// h_{l-1} = sin(2 pi phase) and place those -- while the MFMAs of the previous record run from the other slot, and the
// fragments of the next record are already on their way into registers.  Same ranges, accumulator ownership and partial
// layout (and, FiLM, per-image runs) as k_dw_stream.  (The image stream cost the chain 46 % of its run time: two of four waves transposing
// through 2-byte LDS stores behind barriers, 147 KB per layer and tile to HBM; this way it is 64 KB of plain stores.)
template <int V> struct DwFragMode { static constexpr int v = V; };
template <int H, bool FILM>
__global__ void __launch_bounds__(256, 1) k_dw_frag(const MainArgs a) {
  using Pol = PolBF16;
  using G = Geo<Pol, H>;
  constexpr int NRB = H / 32, RPW = NRB / 4;
  constexpr int NROUND = 4 / G::ROUND_WAVES;
  constexpr int REC = 2 * G::T_BYTES_AL;
  static_assert(G::ROUND_WAVES == 2 && G::STASH_LAYER_BYTES == NRB * 2 * 256 * 16, "two waves per round; fragment layout");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  // builder role: which image, and which thread of the chain's workgroup wrote the fragments this thread places
  const int half = tid >> 7, pt = tid & 127, pw = pt >> 6, phi = (pt & 63) >> 5, pj = pt & 31;
  float* const dwp = a.dwp + (size_t)blockIdx.x * a.dwp_per_wg;
  const int nrec = a.n_tiles * NROUND;
  const int r0 = (int)((long long)blockIdx.x * nrec / gridDim.x), r1 = (int)((long long)(blockIdx.x + 1) * nrec / gridDim.x);
  const int rec_per_image = a.tiles_per_image * NROUND;
  // The builder (round 6).  Work is split by ROW BLOCKS, not by operand: thread (half, pt) places the g values AND computes / places the
  // sines of row blocks 4 half .. 4 half + 3 of chain thread pt, in eight UNITS of two 16-byte words (unit u: chunk u of its row blocks'
  // g fragments -> raw[u], of their phases -> raw[NRB + u]).  (Round 2 gave threads 0..127 all of g and threads 128..255 all of the sines:
  // 128 v_sin_f32 + 128 converts per record on two of the four waves, and a barrier per record at which the other two waited.)
  // Pipelined: the units of record r + 1 are placed BETWEEN the MFMA groups of record r (into the other slot), and each unit's
  // registers are reloaded with record r + 2's words as soon as they have been placed: the ~460 VALU / LDS / transcendental instructions of
  // a record's build run under the 64 MFMAs of the record before instead of in front of them.  Same LDS images, same bits.
  u32x4 raw[NRB * 2];
  auto ptrs = [&](int l, int rec, const char*& sg, const char*& sp) __attribute__((always_inline)) {
    const int tile = rec / NROUND, round = rec - tile * NROUND;
    sg = a.gfs + ((size_t)(l - 1) * a.n_tiles + tile) * (size_t)G::STASH_LAYER_BYTES + (round * 128 + pt) * 16 + half * (NRB * 4096);
    sp = a.stash + (size_t)tile * a.stash_per_wg + (size_t)(l - 1) * G::STASH_LAYER_BYTES + (round * 128 + pt) * 16 + half * (NRB * 4096);
  };
  auto load_unit = [&](const char* sg, const char* sp, int u) __attribute__((always_inline)) {
    // (the fragments are read once: non-temporal loads, -1.0 % on the step)
    raw[u] = __builtin_nontemporal_load((const u32x4*)(sg + u * 4096));
    raw[NRB + u] = __builtin_nontemporal_load((const u32x4*)(sp + u * 4096));
  };
  // Dword stores: the kernel is bound by its LDS pipe (counters: an LDS instruction in flight 20 % of every wave's time x four waves
  // per CU; 128 two-byte stores per wave and record) -- neighbouring lanes (samples 2 k, 2 k + 1: adjacent columns of the images) swap
  // their words through DPP, the even lane stores BOTH samples' row-r values as one dword, the odd lane both row-(r + 1) values: 64
  // four-byte stores instead of 128 two-byte ones for two more VALU instructions per word.  Same LDS images, same bits.
  const unsigned w32_sel = (pj & 1) ? 0x03020706u : 0x05040100u;   // v_perm_b32(x = neighbour's word, w = own word, sel)
  auto build_unit = [&](int slot, int u) __attribute__((always_inline)) {
    const int rq = u >> 1, c = u & 1;
    const u32x4 wg = raw[u], wp = raw[NRB + u];
    char* const TAw = smem + slot * REC + (pw * 32 + (pj & ~1)) * 2 + (half * (NRB / 2) * 32 + (pj & 1)) * G::T_ROWB;   // (rowmap(r + 1) = rowmap(r) + 1 for even r)
    char* const TBw = TAw + G::T_BYTES_AL;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int r = 8 * c + 2 * d;
      static_assert(rowmap(1, 0) == rowmap(0, 0) + 1 && rowmap(7, 1) == rowmap(6, 1) + 1, "rows r, r + 1 of a word are adjacent");
      // (the two sines of a word converted by ONE v_cvt_pk_bf16_f32 -- converted one at a time hipcc issued a packed convert per value)
      typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
      const unsigned hp = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{__builtin_amdgcn_sinf(phase_lo(wp[d])), __builtin_amdgcn_sinf(phase_hi(wp[d]))}, bf16x2_t));
      const unsigned gx = (unsigned)__builtin_amdgcn_update_dpp(0, (int)wg[d], 0xB1, 0xf, 0xf, true);   // quad_perm [1, 0, 3, 2]
      const unsigned hx = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hp, 0xB1, 0xf, 0xf, true);
      *(unsigned*)(TAw + (32 * rq + rowmap(r, phi)) * G::T_ROWB) = __builtin_amdgcn_perm(gx, wg[d], w32_sel);
      *(unsigned*)(TBw + (32 * rq + rowmap(r, phi)) * G::T_ROWB) = __builtin_amdgcn_perm(hx, hp, w32_sel);
    }
  };
#pragma unroll 1
  for (int l = 1; l <= a.L; ++l) {
    f32x16 acc[RPW * NRB];
    acc_zero<RPW * NRB>(acc);
    float db[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) db[q] = 0.f;
    float* const dw = dwp + a.p_off_w[l];
    float* const dbp = dwp + a.p_off_b[l];
    bool first_flush = true;
    int run = 0;
    // The accumulator leaves the registers: once per layer (concat), or at the end of every image run of the range (FiLM:
    // M = g_theta h^T is per image -- d(phase) = row sums of g_theta, the W (.) M row sums and diag(freq) M; as k_dw_stream)
    auto flush = [&](int image) __attribute__((always_inline)) {
      Pol::drain();
      // (opaque copies of the lane's coordinates: every address below is formed HERE -- hipcc otherwise hoists the few hundred
      // per-lane 64-bit addresses of this block out of the record loop and spills them, 1.1 KB per lane measured.  One pass
      // over the accumulator, a row at a time: each element is read from its AGPR once, for the row sum and for the partial)
      int hio = hi, jo = j;
      asm volatile("" : "+v"(hio), "+v"(jo));
      const float* const freq = FILM ? a.film + ((size_t)image * a.L + (l - 1)) * 2 * H : nullptr;
      const float* const W = FILM ? a.params + a.n_first + a.p_off_w[l] : nullptr;
      float* const out = FILM ? a.dfr + ((size_t)(blockIdx.x * a.kmax + run) * a.L + (l - 1)) * 2 * H : nullptr;
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        const int rb = wave + 4 * q;
        float t[16], sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          t[r] = 0.f;
          sc[r] = 1.f;
          if constexpr (FILM) sc[r] = freq[32 * rb + rowmap(r, hio)];
        }
#pragma unroll
        for (int cb = 0; cb < NRB; ++cb) {  // one 32 x 32 block of the accumulator at a time
          asm volatile("" ::: "memory");
          const f32x16 blk = acc[q * NRB + cb];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned e = (unsigned)((32 * rb + rowmap(r, hio)) * H + 32 * cb + jo);
            if constexpr (FILM) t[r] += blk[r] * W[e];
            if (a.need_dw) dw[e] = first_flush ? blk[r] * sc[r] : (dw[e] + blk[r] * sc[r]);
          }
        }
        if constexpr (FILM) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float ts = half_sum(t[r]);
            if (jo == 0) out[32 * rb + rowmap(r, hio)] = ts;
          }
        }
        float dbv = db[q] + __shfl_xor(db[q], 32, 64);
        if constexpr (FILM) {
          if (hio == 0) out[H + 32 * rb + jo] = dbv;
          dbv *= freq[32 * rb + jo];
        }
        if (a.need_dw && hio == 0) dbp[32 * rb + jo] = first_flush ? dbv : (dbp[32 * rb + jo] + dbv);
      }
      if constexpr (FILM) {
        if (tid == 0) a.run_image[blockIdx.x * a.kmax + run] = image;
      }
      first_flush = false;
      ++run;
      acc_zero<RPW * NRB>(acc);
#pragma unroll
      for (int q = 0; q < RPW; ++q) db[q] = 0.f;
    };
    // Runs outside, records inside: the flush sits between two record loops, where no prefetched fragment is alive (inside
    // the record loop it cost 360 B of scratch per lane: the flush wants the registers `raw` occupies).
    int slot = 0;
#pragma unroll 1
    for (int rs = r0; rs < r1;) {
      const int image = rs / rec_per_image;
      int re = FILM ? (image + 1) * rec_per_image : r1;  // end of this image run (concat: the whole range is one run)
      re = re < r1 ? re : r1;
      // MODE 0: the record's MFMAs alone; 1: + the units of the next record placed into the other slot between them; 2: + each unit's
      // registers reloaded from (sgn, spn) -- the record after that -- behind its placement
      auto mma = [&](int slot, auto mode_c, const char* sgn, const char* spn) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_c)::v;
        const char* TA = smem + slot * REC;
        const char* TB = TA + G::T_BYTES_AL;
        // The B fragments are requested PF column blocks (PF x RPW MFMAs) ahead of their use and the A fragments of the next
        // k-step while the last column blocks of this one are multiplied; fenced, as gemm_lds_bop: left to itself hipcc sinks
        // every fragment read to just in front of its MFMAs -- one fragment register, one LDS round trip per MFMA pair.
        constexpr int NKS = G::ROUND_SAMPLES / Pol::TS, NSTEP = NKS * NRB, PF = 4;
        static_assert(NSTEP == 4 * NRB, "one builder unit per four MFMA steps");
        auto fb = [&](int i) __attribute__((always_inline)) { return t_read<Pol, H, NRB>(TB, i % NRB, i / NRB, j, hi); };
        bf16x8 fa[2][RPW], qb[PF];
#pragma unroll
        for (int q = 0; q < RPW; ++q) fa[0][q] = t_read<Pol, H, NRB>(TA, wave + 4 * q, 0, j, hi);
#pragma unroll
        for (int d = 0; d < PF; ++d) qb[d] = fb(d);
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
          const int ks = i / NRB, cb = i % NRB;
          const bf16x8 b = qb[i % PF];
          if (i + PF < NSTEP) qb[i % PF] = fb(i + PF);
          if (cb == NRB - PF && ks + 1 < NKS) {
#pragma unroll
            for (int q = 0; q < RPW; ++q) fa[(ks + 1) & 1][q] = t_read<Pol, H, NRB>(TA, wave + 4 * q, ks + 1, j, hi);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < RPW; ++q) acc[q * NRB + cb] = Pol::mfma(fa[ks & 1][q], b, acc[q * NRB + cb]);
          if (cb == NRB - 1) {
#pragma unroll
            for (int q = 0; q < RPW; ++q) db[q] = frag_sum<Pol>(fa[ks & 1][q], db[q]);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (MODE >= 1) {
            if ((i & 3) == 1) {   // (behind the step's MFMAs: they run while these ~60 instructions issue)
              build_unit(slot ^ 1, i >> 2);
              if constexpr (MODE == 2) load_unit(sgn, spn, i >> 2);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
        // (inside the loop body: whatever the register allocator places at the head of the exit block -- it was seen to put
        // accumulator spill code there, in front of the flush's own drain -- then sits behind a completed write-back)
        Pol::drain();
      };
      using M0 = DwFragMode<0>; using M1 = DwFragMode<1>; using M2 = DwFragMode<2>;
      const char *sg, *sp;
      ptrs(l, rs, sg, sp);
#pragma unroll
      for (int u = 0; u < NRB; ++u) load_unit(sg, sp, u);
#pragma unroll
      for (int u = 0; u < NRB; ++u) build_unit(slot, u);   // the run's first record: placed in front of its MFMAs
      if (rs + 1 < re) {
        ptrs(l, rs + 1, sg, sp);
#pragma unroll
        for (int u = 0; u < NRB; ++u) load_unit(sg, sp, u);
      }
      __syncthreads();
      int rec = rs;
#pragma unroll 1
      for (; rec + 2 < re; ++rec, slot ^= 1) {   // MFMAs of rec || placement of rec + 1 || requests of rec + 2
        ptrs(l, rec + 2, sg, sp);
        mma(slot, M2{}, sg, sp);
        __syncthreads();   // slot ^ 1 is complete; every wave is past its reads of `slot`
      }
      if (rec + 1 < re) {
        mma(slot, M1{}, sg, sp);
        __syncthreads();
        slot ^= 1;
      }
      mma(slot, M0{}, sg, sp);
      slot ^= 1;
      flush(image);
      rs = re;
    }
    if (r0 >= r1 && !FILM) flush(0);  // (cannot happen: every workgroup owns at least one record)
    __syncthreads();
  }
}
template __global__ void k_dw_frag<256, false>(const MainArgs);
template __global__ void k_dw_frag<256, true>(const MainArgs);

// fp32 counterpart of k_dw_frag (H = 256, concat): g_l and the pre-activations a_{l-1} arrive as fp32 fragments
// ([row block][quarter][256 threads][16 B], the fp32 stash layout); a record = the 32 samples of one wave of the chain.
// Threads 0..127 place g, threads 128..255 compute h = sin(omega a) with the chain's own sin_f32 (bit-identical h) and place
// it; [sample][feature + 1] images, v_mfma_f32_32x32x2_f32 with K = 2 samples, one layer's 256 x 256 accumulator in the AGPRs.
template <int H>
__global__ void __launch_bounds__(256, 1) k_dw_frag32(const MainArgs a) {
  using Pol = PolF32;
  using G = Geo<Pol, H>;
  constexpr int NRB = H / 32, RPW = NRB / 4, NROUND = 4;
  constexpr int TAL = (G::T_BYTES + 1023) & ~1023, REC = 2 * TAL;
  static_assert(G::ROUND_WAVES == 1 && G::STASH_LAYER_BYTES == NRB * 4 * 256 * 16, "one wave per round; fragment layout");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, hi = lane >> 5, j = lane & 31;
  const int half = tid >> 7, part = (tid >> 6) & 1, pl = tid & 63, phi = pl >> 5, pj = pl & 31;
  float* const dwp = a.dwp + (size_t)blockIdx.x * a.dwp_per_wg;
  const int nrec = a.n_tiles * NROUND;
  const int r0 = (int)((long long)blockIdx.x * nrec / gridDim.x), r1 = (int)((long long)(blockIdx.x + 1) * nrec / gridDim.x);
  f32x4 raw[NRB * 2];  // this thread's half of the producer lane's NRB * 4 chunks
  auto load = [&](int l, int rec) __attribute__((always_inline)) {
    const int tile = rec / NROUND, round = rec - tile * NROUND;
    const char* src = (half == 0) ? a.gfs + ((size_t)(l - 1) * a.n_tiles + tile) * (size_t)G::STASH_LAYER_BYTES
                                  : a.stash + (size_t)tile * a.stash_per_wg + (size_t)(l - 1) * G::STASH_LAYER_BYTES;
    src += (size_t)(part * NRB * 2) * 4096 + (round * 64 + pl) * 16;
#pragma unroll
    for (int q = 0; q < NRB * 2; ++q) raw[q] = *(const f32x4*)(src + q * 4096);
  };
  auto build = [&](int slot, float omega) __attribute__((always_inline)) {
    char* const T = smem + slot * REC + half * TAL + pj * (32 * NRB + 1) * 4;
#pragma unroll
    for (int q = 0; q < NRB * 2; ++q) {
      const int qq = part * NRB * 2 + q, rb = qq >> 2, c = qq & 3;  // (part is wave-uniform: two code paths, no divergence)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float v = (half == 0) ? raw[q][d] : sin_f32(omega * raw[q][d]);
        *(float*)(T + (32 * rb + rowmap(4 * c + d, phi)) * 4) = v;
      }
    }
  };
#pragma unroll 1
  for (int l = 1; l <= a.L; ++l) {
    const float omega = (l == 1) ? a.w_first : a.w_hidden;
    f32x16 acc[RPW * NRB];
    acc_zero<RPW * NRB>(acc);
    float db[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) db[q] = 0.f;
    int slot = 0;
    if (r0 < r1) load(l, r0);
#pragma unroll 1
    for (int rec = r0; rec < r1; ++rec, slot ^= 1) {
      if (part == 0) build(slot, omega); else build(slot, omega);
      if (rec + 1 < r1) load(l, rec + 1);
      __syncthreads();
      const char* TA = smem + slot * REC;
      const char* TB = TA + TAL;
#pragma unroll 4
      for (int ks = 0; ks < 32 / Pol::TS; ++ks) {
        float fa[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) fa[q] = t_read<Pol, H, NRB>(TA, wave + 4 * q, ks, j, hi);
#pragma unroll
        for (int cb = 0; cb < NRB; ++cb) {
          const float b = t_read<Pol, H, NRB>(TB, cb, ks, j, hi);
#pragma unroll
          for (int q = 0; q < RPW; ++q) acc[q * NRB + cb] = Pol::mfma(fa[q], b, acc[q * NRB + cb]);
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q) db[q] = frag_sum<Pol>(fa[q], db[q]);
      }
      Pol::drain();
    }
    Pol::drain();
    int hio = hi, jo = j;
    asm volatile("" : "+v"(hio), "+v"(jo));
    float* const dw = dwp + a.p_off_w[l];
    float* const dbp = dwp + a.p_off_b[l];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int rb = wave + 4 * q;
#pragma unroll
      for (int cb = 0; cb < NRB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[(unsigned)((32 * rb + rowmap(r, hio)) * H + 32 * cb + jo)] = acc[q * NRB + cb][r];
      const float dbv = db[q] + __shfl_xor(db[q], 32, 64);
      if (hio == 0) dbp[32 * rb + jo] = dbv;
    }
    __syncthreads();
  }
}
template __global__ void k_dw_frag32<256>(const MainArgs);

