// reni_dev_small.inc -- prologue / epilogue kernels: k_prep_image, k_pack, reductions, first-layer tails, FiLM glue, Adam, probes (core translation unit only)
// Part of reni_device.inc (included there, inside namespace reni; never compiled on its own).

// FiLM on the stream path: dfilm[b][l][0][f] = sum over the image's runs of the W (.) M row sums + b_l[f] d(phase),
// dfilm[b][l][1][f] = d(phase); runs are visited in a fixed order (deterministic)
DEV void reduce_film_runs_body(const MainArgs& a, int H, int nruns, float* dfilm, const int bx, const int by) {
  const float* dfr = a.dfr;
  const int* run_image = a.run_image;
  const int L = a.L;
  const float* params = a.params;
  const unsigned n_first = a.n_first;
  const unsigned* p_off_b = a.p_off_b;
  const int b = bx, i = by * 256 + threadIdx.x;
  const bool live = i < L * H;
  const int l = live ? i / H : 0, f = i - l * H;
  // the image's runs, compacted in run order by wave 0 (1024 runs at a time), then summed by everybody
  __shared__ int vl[1024];
  __shared__ int nv;
  float s0 = 0.f, s1 = 0.f;
  for (int base = 0; base < nruns; base += 1024) {
    const int cnt = nruns - base < 1024 ? nruns - base : 1024;
    __syncthreads();
    if (threadIdx.x < 64) {
      int c = 0;
      for (int w0 = 0; w0 < cnt; w0 += 64) {
        const int w = w0 + (int)threadIdx.x;
        const bool ok = w < cnt && run_image[base + w] == b;
        const unsigned long long m = __ballot(ok);
        if (ok) vl[c + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = base + w;
        c += __popcll(m);
      }
      if (threadIdx.x == 0) nv = c;
    }
    __syncthreads();
    if (live) {
      const int m = nv;
      for (int q = 0; q < m; ++q) {
        const float* p = dfr + ((size_t)vl[q] * L + l) * 2 * H;
        s0 += p[f];
        s1 += p[H + f];
      }
    }
  }
  if (!live) return;
  const float bias = params[n_first + p_off_b[l + 1] + f];
  dfilm[((size_t)b * L + l) * 2 * H + f] = s0 + bias * s1;
  dfilm[((size_t)b * L + l) * 2 * H + H + f] = s1;
}
__global__ void __launch_bounds__(256) k_reduce_film_runs(const MainArgs a, int H, int nruns, float* dfilm) {
  reduce_film_runs_body(a, H, nruns, dfilm, (int)blockIdx.x, (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------
// prologue: per-image constant input columns and the affine map A_b
// ------------------------------------------------------------------------------------------
// xconst[b][col] = value of input column col if it is constant over the image, else 0
// A[b][h][0..4] = coefficients of (dx, dy, dz, r, 1)
DEV void prep_image_body(const PrepArgs& a, const int bx, const int by, char* smem) {
  // block (bx = image, by = group of 8 rows): rebuilds the image's constant columns in LDS (cheap) and does 8 rows
  float* xc = (float*)smem;  // F_in
  const int b = bx, tid = threadIdx.x, nd = a.nd, F = a.F_in;
  // (with idx: the gather of the batch's latent rows happens here -- no separate gather kernel, no [B,nd,3] round trip)
  // An index outside the table [0, n_rows) reads row 0 instead and POISONS everything derived from it with NaN: the step's
  // loss and gradients come out NaN (loud, no host synchronisation) rather than computed from out-of-bounds memory -- a global /
  // local index mix-up is easy to make with sharded tables, and the Adam kernels would silently skip the unmatched row.
  const long long row = a.idx ? a.idx[b] : (long long)b;
  const bool bad = a.idx != nullptr && (row < 0 || row >= a.n_rows);
  const float poison = bad ? __builtin_nanf("") : 0.f;
  const float* z = a.Z + (size_t)(bad ? 0 : row) * nd * 3;
  if (a.idx != nullptr && by == 0) {
    for (int i = tid; i < nd * 3; i += 256) a.Zc[(size_t)b * nd * 3 + i] = z[i] + poison;
    if (a.idx_copy != nullptr && tid == 0) a.idx_copy[b] = row;
  }
  for (int col = tid; col < F; col += 256) {
    float val = 0.f;
    if (a.eq == 1) {  // SO2: [ip nd | G nd^2 | r | zy nd | dy]
      const int c1 = col - nd;
      if (c1 >= 0 && c1 < nd * nd) {
        const int i = c1 / nd, k = c1 - i * nd;
        val = z[i * 3] * z[k * 3] + z[i * 3 + 2] * z[k * 3 + 2];
      } else if (c1 > nd * nd && c1 <= nd * nd + nd) {
        val = z[(c1 - nd * nd - 1) * 3 + 1];
      }
    } else if (a.eq == 2) {  // SO3: [ip nd | G nd^2]
      const int c1 = col - nd;
      if (c1 >= 0) {
        const int i = c1 / nd, k = c1 - i * nd;
        val = z[i * 3] * z[k * 3] + z[i * 3 + 1] * z[k * 3 + 1] + z[i * 3 + 2] * z[k * 3 + 2];
      }
    } else {  // None: [ip nd | vec(Z) 3nd]
      const int c1 = col - nd;
      if (c1 >= 0) val = z[c1];
    }
    val += poison;
    xc[col] = val;
    if (by == 0) a.xconst[(size_t)b * F + col] = val;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int h = by * 8 + wave; h < min(a.H, (int)by * 8 + 8); h += 4) {
    const float* w = a.W0 + (size_t)h * F;
    // (eight loads of the weight row in flight per lane: as one dependent load per iteration the 1 370-column row of config 2 was
    // 22 exposed memory latencies per row, 20 us for the launch)
    float cs[8], ux = 0.f, uy = 0.f, uz = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) cs[u] = 0.f;
    int col = lane;
    for (; col + 7 * 64 < F; col += 8 * 64) {
      float wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) wv[u] = w[col + 64 * u];
#pragma unroll
      for (int u = 0; u < 8; ++u) cs[u] += wv[u] * xc[col + 64 * u];
    }
    for (; col < F; col += 64) cs[0] += w[col] * xc[col];
    float c = ((cs[0] + cs[1]) + (cs[2] + cs[3])) + ((cs[4] + cs[5]) + (cs[6] + cs[7]));
    for (int k = lane; k < nd; k += 64) {
      const float wv = w[k];
      ux += wv * z[k * 3];
      uy += wv * z[k * 3 + 1];
      uz += wv * z[k * 3 + 2];
    }
    c = wave_sum(c); ux = wave_sum(ux); uy = wave_sum(uy); uz = wave_sum(uz);
    if (lane == 0) {
      float* o = a.A + ((size_t)b * a.H + h) * 8;
      if (a.eq == 1) {
        o[0] = ux; o[1] = w[F - 1]; o[2] = uz; o[3] = w[nd + nd * nd];
      } else {
        o[0] = ux; o[1] = uy; o[2] = uz; o[3] = 0.f;
      }
      o[4] = c + a.b0[h] + poison;
      o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
      if (a.afrag != nullptr) {  // row h as the two lanes' operands of the layer-0 MFMA (hi + lo bf16 parts, see k_reni_train_bf16)
        __bf16 Ah[5], Al[5];
        for (int k = 0; k < 5; ++k) { const float v = o[k] * a.afrag_scale; Ah[k] = (__bf16)v; Al[k] = (__bf16)(v - (float)Ah[k]); }
        const bf16x8 f0 = {Ah[0], Ah[1], Ah[2], Ah[3], Ah[4], Al[0], Al[1], Al[2]};
        const bf16x8 f1 = {Al[3], Al[4], Ah[0], Ah[1], Ah[2], Ah[3], (__bf16)0.f, (__bf16)0.f};
        char* fr = a.afrag + (((size_t)b * (a.H / 32) + (h >> 5)) * 64 + (h & 31)) * 16;
        *(bf16x8*)fr = f0;
        *(bf16x8*)(fr + 32 * 16) = f1;
      }
    }
  }
}
// FiLM on the persistent kernels: the caller supplies A [B][H][8] (first FiLM layer folded in); this makes the layer-0 MFMA
// operands of it exactly as k_prep_image does for the concat models.  grid (B, H / 64), 64 rows per block.
// (k_prologue's FiLM role: block `blk` = 256 consecutive (image, row) pairs)
DEV void afrag_from_A_body(const float* A, char* afrag, float scale, int H, int B, int blk) {
  const int i = blk * 256 + (int)threadIdx.x;
  const int b = i / H, h = i - b * H;
  if (b >= B) return;
  const float* o = A + ((size_t)b * H + h) * 8;
  __bf16 Ah[5], Al[5];
  for (int k = 0; k < 5; ++k) { const float v = o[k] * scale; Ah[k] = (__bf16)v; Al[k] = (__bf16)(v - (float)Ah[k]); }
  const bf16x8 f0 = {Ah[0], Ah[1], Ah[2], Ah[3], Ah[4], Al[0], Al[1], Al[2]};
  const bf16x8 f1 = {Al[3], Al[4], Ah[0], Ah[1], Ah[2], Ah[3], (__bf16)0.f, (__bf16)0.f};
  char* fr = afrag + (((size_t)b * (H / 32) + (h >> 5)) * 64 + (h & 31)) * 16;
  *(bf16x8*)fr = f0;
  *(bf16x8*)(fr + 32 * 16) = f1;
}

// ------------------------------------------------------------------------------------------
// FiLM per-image glue (reference: CustomMappingNetwork src/models/RENI.py:482-505, forward_with_frequencies_
// phase_shifts :665-676, SO2/SO3InvariantRepresentationFiLM :407-447)
// ------------------------------------------------------------------------------------------
// first-layer row f of image b as coefficients of (dx, dy, dz, r) -- the Siren_Input is linear in them
DEV void film_row0(const FilmGlueArgs& a, const float* z, int f, float (&c)[4]) {
  const float* w = a.params + (size_t)f * a.F0;
  c[0] = c[1] = c[2] = c[3] = 0.f;
  // (unrolled: the loads of eight terms are in flight together -- as written it was a chain of nd dependent memory latencies)
  if (a.eq == 1) {  // [|d_xz|, d_y, D_xz Z_xz^T]
#pragma unroll 8
    for (int k = 0; k < a.nd; ++k) { c[0] += w[2 + k] * z[k * 3]; c[2] += w[2 + k] * z[k * 3 + 2]; }
    c[1] = w[1]; c[3] = w[0];
  } else {          // D Z^T
#pragma unroll 8
    for (int k = 0; k < a.nd; ++k) { c[0] += w[k] * z[k * 3]; c[1] += w[k] * z[k * 3 + 1]; c[2] += w[k] * z[k * 3 + 2]; }
  }
}

// The glue is a handful of batch-parallel kernels (one workgroup per image ran the mapping network's GEMVs
// serially: 1.3 ms per step for 0.1 GFLOP):
//   forward : k_film_minput -> k_film_linear x (ML + 1) -> k_film_fold
//   backward: k_film_dout -> k_film_linear_t x (ML + 1) -> k_film_grads (dZ, dW0 / db0, every mapping layer's weight gradient)

// grid B: mapping input m_b = [vec(G) | Z_y] (SO2) / vec(G) (SO3)
__global__ void __launch_bounds__(256) k_film_minput(const FilmGlueArgs a) {
  const int b = blockIdx.x, nd = a.nd;
  const float* z = a.Z + (size_t)b * nd * 3;
  for (int i = threadIdx.x; i < a.M_in; i += 256) {
    float v;
    if (i < nd * nd) {
      const int k = i / nd, q = i - k * nd;
      v = z[k * 3] * z[q * 3] + z[k * 3 + 2] * z[q * 3 + 2];
      if (a.eq == 2) v += z[k * 3 + 1] * z[q * 3 + 1];
    } else {
      v = z[(i - nd * nd) * 3 + 1];  // SO2: Z_y
    }
    a.mapm[(size_t)b * a.M_in + i] = v;
  }
}

// y[b][n] = act(sum_k W[n][k] x[b][k] + bias[n]); one wave per (image, RPW consecutive output rows), grid (ceil(N / (4 RPW)), B).
// RPW = 4 for the wide last layer (the rows share the lane's x values; one row per wave was 24 576 blocks = 13 us of block dispatch),
// RPW = 1 elsewhere (the first layer's 21-term lane sums with eight loads in flight; four rows per wave left the chip half empty there)
template <int RPW>
__global__ void __launch_bounds__(256) k_film_linear(const float* x, int ldx, const float* W, const float* bias, float* y,
                                                     int ldy, int N, int K, int leaky) {
  const int b = blockIdx.y, n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW, lane = threadIdx.x & 63;
  if (n0 >= N) return;
  const float* xr = x + (size_t)b * ldx;
  float s[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) s[r] = 0.f;
#pragma unroll RPW == 1 ? 8 : 2
  for (int k = lane; k < K; k += 64) {
    const float xv = xr[k];
#pragma unroll
    for (int r = 0; r < RPW; ++r) s[r] += (n0 + r < N) ? W[(size_t)(n0 + r) * K + k] * xv : 0.f;
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const float t = wave_sum(s[r]);
    if (lane == 0 && n0 + r < N) {
      float v = t + bias[n0 + r];
      if (leaky) v = (v > 0.f) ? v : 0.2f * v;  // LeakyReLU(0.2)
      y[(size_t)b * ldy + n0 + r] = v;
    }
  }
}
template __global__ void k_film_linear<1>(const float*, int, const float*, const float*, float*, int, int, int, int);
template __global__ void k_film_linear<4>(const float*, int, const float*, const float*, float*, int, int, int, int);

// grid B: mapping output -> film[b] (freq = 15 f + 30, phase) and the folded first layer A[b]
__global__ void __launch_bounds__(256) k_film_fold(const FilmGlueArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nd = a.nd, H = a.H, nF = a.L + 1;
  const float* z = a.Z + (size_t)b * nd * 3;
  const float* fo = a.fo + (size_t)b * a.N_out;  // [freq raw nF*H | phase nF*H]
  for (int i = tid; i < a.L * H; i += 256) {
    const int l = i / H + 1, f = i - (l - 1) * H;
    float* o = a.film + ((size_t)b * a.L + (l - 1)) * 2 * H;
    o[f] = 15.f * fo[l * H + f] + 30.f;
    o[H + f] = fo[nF * H + l * H + f];
  }
  for (int f = tid; f < H; f += 256) {
    float c[4];
    film_row0(a, z, f, c);
    const float fr = 15.f * fo[f] + 30.f, ph = fo[nF * H + f], b0 = a.params[(size_t)H * a.F0 + f];
    float* o = a.A + ((size_t)b * H + f) * 8;
    o[0] = fr * c[0]; o[1] = fr * c[1]; o[2] = fr * c[2]; o[3] = fr * c[3];
    o[4] = fr * b0 + ph;
    o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
  }
}

// grid B: (dA, dfilm) -> gradient of the mapping output (delta block ML) and dAb = freq_0 . dA
__global__ void __launch_bounds__(256) k_film_dout(const FilmGlueArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nd = a.nd, H = a.H, nF = a.L + 1;
  const float* z = a.Z + (size_t)b * nd * 3;
  const float* fo = a.fo + (size_t)b * a.N_out;
  float* d = a.dly + a.dly_off[a.ML] + (size_t)b * a.N_out;
  for (int i = tid; i < a.L * H; i += 256) {
    const int l = i / H + 1, f = i - (l - 1) * H;
    const float* g = a.dfilm + ((size_t)b * a.L + (l - 1)) * 2 * H;
    d[l * H + f] = 15.f * g[f];
    d[nF * H + l * H + f] = g[H + f];
  }
  for (int f = tid; f < H; f += 256) {
    float c[4];
    film_row0(a, z, f, c);
    const float* g = a.dA + ((size_t)b * H + f) * 8;
    const float b0 = a.params[(size_t)H * a.F0 + f], fr = 15.f * fo[f] + 30.f;
    d[f] = 15.f * (g[0] * c[0] + g[1] * c[1] + g[2] * c[2] + g[3] * c[3] + g[4] * b0);
    d[nF * H + f] = g[4];
    float* o = a.dAb + ((size_t)b * H + f) * 8;
#pragma unroll
    for (int q = 0; q < 5; ++q) o[q] = fr * g[q];
    o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
  }
}

// dx[b][k] = (sum_n W[n][k] dy[b][n]) * LeakyReLU'(xact[b][k])   (xact == NULL: no activation in front).
// grid (ceil(K / 64), B); a workgroup = 64 columns k x sixteen parts of the n range (one wave each; consecutive lanes read
// consecutive k of a weight row), partial sums combined in a fixed order through LDS
constexpr int FLT_NG = 16;  // groups of the n range per block (one wave each)
__global__ void __launch_bounds__(64 * FLT_NG) k_film_linear_t(const float* dy, int ldd, const float* W, int N, int K,
                                                              const float* xact, int ldxa, float* dx, int ldo) {
  __shared__ float red[FLT_NG][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const float* d = dy + (size_t)b * ldd;
  const int n0 = (int)((long long)q * N / FLT_NG), n1 = (int)((long long)(q + 1) * N / FLT_NG);
  // (eight loads in flight per lane: with N = 2 (L + 1) H rows per quarter-of-N and two in flight the last mapping layer's
  // transpose was a 62 us chain of memory latencies)
  float s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = 0.f;
  if (k < K) {
    int n = n0;
    for (; n + 7 < n1; n += 8) {
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = W[(size_t)(n + u) * K + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += w[u] * d[n + u];
    }
    for (; n < n1; ++n) s[0] += W[(size_t)n * K + k] * d[n];
  }
  red[q][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (q == 0 && k < K) {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < FLT_NG; u += 4) s += (red[u][lane] + red[u + 1][lane]) + (red[u + 2][lane] + red[u + 3][lane]);
    if (xact != nullptr) s *= (xact[(size_t)b * ldxa + k] > 0.f) ? 1.f : 0.2f;
    dx[(size_t)b * ldo + k] = s;
  }
}

// grid B: dZ from the gradient of the mapping input (dm [B][M_in]) and from dAb
DEV void film_dz_body(const FilmGlueArgs& a, const float* dm_all, const int bx) {
  const int b = bx, nd = a.nd, H = a.H;
  const float* z = a.Z + (size_t)b * nd * 3;
  const float* dm = dm_all + (size_t)b * a.M_in;
  const float* dab = a.dAb + (size_t)b * H * 8;
  for (int t = threadIdx.x; t < nd * 3; t += 256) {
    const int k = t / 3, c = t - 3 * k;
    float v = 0.f;
    if (a.eq == 2 || c != 1) {
#pragma unroll 6
      for (int q = 0; q < nd; ++q) v += (dm[k * nd + q] + dm[q * nd + k]) * z[q * 3 + c];
      const int wcol = (a.eq == 1) ? 2 + k : k;
#pragma unroll 16
      for (int f = 0; f < H; ++f) v += dab[f * 8 + c] * a.params[(size_t)f * a.F0 + wcol];
    } else {
      v = dm[nd * nd + k];  // SO2: Z_y enters the mapping input only
    }
    a.dZ[(size_t)b * nd * 3 + t] = v + a.alpha2 * z[t];
  }
}

// out[n][k] = sum_b delta[b][n] x[b][k],  out_b[n] = sum_b delta[b][n]:
// every mapping-network layer's weight gradient in ONE launch (grid (max ceil((K+1)/256), max N, layers)): the layers are
// independent given the deltas, and as ML + 1 dependent launches of 5-7 us they were launch latency, not work
struct FilmWgradAll {
  const float* delta[MAX_MAP_LAYERS + 1]; const float* x[MAX_MAP_LAYERS + 1];
  float* out_w[MAX_MAP_LAYERS + 1]; float* out_b[MAX_MAP_LAYERS + 1];
  int ldd[MAX_MAP_LAYERS + 1], ldx[MAX_MAP_LAYERS + 1], N[MAX_MAP_LAYERS + 1], K[MAX_MAP_LAYERS + 1];
  int B;
};
DEV void film_wgrad_all_body(const FilmWgradAll& a, const int bx, const int by, const int bz) {
  const int i = bz, k = bx * 256 + threadIdx.x, n = by, K = a.K[i];
  if (n >= a.N[i] || k > K) return;
  const float* delta = a.delta[i];
  const size_t ldd = (size_t)a.ldd[i];
  float s = 0.f;
  if (k == K) {
#pragma unroll 8
    for (int b = 0; b < a.B; ++b) s += delta[(size_t)b * ldd + n];
    a.out_b[i][n] = s;
    return;
  }
  const float* x = a.x[i];
  const size_t ldx = (size_t)a.ldx[i];
#pragma unroll 8
  for (int b = 0; b < a.B; ++b) s += delta[(size_t)b * ldd + n] * x[(size_t)b * ldx + k];
  a.out_w[i][(size_t)n * K + k] = s;
}

// first FiLM layer: dW0[f][col], db0[f] from dAb and the latents (grid (ceil((F0+1)/256), H))
DEV void film_w0grad_body(const FilmGlueArgs& a, float* dW0, float* db0, const int bx, const int by) {
  const int col = bx * 256 + threadIdx.x, f = by, nd = a.nd;
  if (col > a.F0) return;
  const float* g0 = a.dAb + (size_t)f * 8;
  const size_t gs = (size_t)a.H * 8;
  float s = 0.f;
  if (col == a.F0) {
#pragma unroll 8
    for (int b = 0; b < a.B; ++b) s += g0[b * gs + 4];
    db0[f] = s;
    return;
  }
  if (a.eq == 1 && col < 2) {
    const int q = (col == 0) ? 3 : 1;
#pragma unroll 8
    for (int b = 0; b < a.B; ++b) s += g0[b * gs + q];
  } else {
    const int k = (a.eq == 1) ? col - 2 : col;
    const float wy = (a.eq == 1) ? 0.f : 1.f;
#pragma unroll 8
    for (int b = 0; b < a.B; ++b) {
      const float* g = g0 + b * gs;
      const float* z = a.Z + ((size_t)b * nd + k) * 3;
      s += g[0] * z[0] + wy * g[1] * z[1] + g[2] * z[2];
    }
  }
  dW0[(size_t)f * a.F0 + col] = s;
}

// The gradients behind the mapping network's transposed chain in ONE launch: dZ (B blocks; needs dm), the first FiLM layer's dW0 / db0
// (gx0 x H blocks; needs dAb) and every mapping layer's weight gradient (per layer ceil((K + 1) / 256) x N blocks; needs the deltas) are
// independent of each other.  (They were three launches on two streams: the fork's and the join's cross-stream edges cost more than
// k_film_dz took once its loops had loads in flight.)
struct FilmGrads { const float* dm; float* dW0; float* db0; int need_dw, gx0, nlayers; int gxw[MAX_MAP_LAYERS + 1], blk_end[MAX_MAP_LAYERS + 1]; };
__global__ void __launch_bounds__(256) k_film_grads(const FilmGlueArgs a, const FilmWgradAll wa, const FilmGrads r) {
  int i = (int)blockIdx.x;
  if (i < a.B) { film_dz_body(a, r.dm, i); return; }
  i -= a.B;
  if (!r.need_dw) return;
  const int n0 = r.gx0 * a.H;
  if (i < n0) { film_w0grad_body(a, r.dW0, r.db0, i % r.gx0, i / r.gx0); return; }
  i -= n0;
  // (exactly ceil((K + 1) / 256) x N blocks per layer: a common grid of max x max x layers was 36 864 blocks, 31 000 of them empty --
  // 30 us of block dispatch)
  int ly = 0, first = 0;
  while (ly < r.nlayers - 1 && i >= r.blk_end[ly]) { first = r.blk_end[ly]; ++ly; }
  i -= first;
  film_wgrad_all_body(wa, i % r.gxw[ly], i / r.gxw[ly], ly);
}

// ------------------------------------------------------------------------------------------
// weight repacking into MFMA fragment order (once per call; the weights change every step)
// ------------------------------------------------------------------------------------------
template <class Pol>
DEV void pack_body(const PackArgs& a, const int bx, const int by, const int gx) {
  const PackDesc d = a.d[by];
  const int nfrag_lanes = d.nrb * d.nks * 64;
  for (int t = bx * 256 + threadIdx.x; t < nfrag_lanes; t += gx * 256) {
    const int lane = t & 63, fr = t >> 6;
    const int ks = fr % d.nks, rb = fr / d.nks;
    const int R = 32 * rb + (lane & 31), hi = lane >> 5;
    if constexpr (Pol::BF) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int Fk = kfeat<Pol>(ks, hi, e);
        float val = 0.f;
        if (!d.transposed) { if (R < d.M && Fk < d.K) val = a.params[d.src + (size_t)R * d.K + Fk]; }
        else { if (Fk < d.M && R < d.K) val = a.params[d.src + (size_t)Fk * d.K + R]; }
        o[e] = (__bf16)(val * d.scale);
      }
      const int cell = d.swz ? (t ^ ((hi << 2) | ((ks & 1) << 3))) : t;  // (a shared image: wimg_cell, reni_dev_train.inc)
      *(bf16x8*)(a.wimg + d.dst + (size_t)cell * 16) = o;
    } else {
      const int Fk = kfeat<Pol>(ks, hi, 0);
      float val = 0.f;
      if (!d.transposed) { if (R < d.M && Fk < d.K) val = a.params[d.src + (size_t)R * d.K + Fk]; }
      else { if (Fk < d.M && R < d.K) val = a.params[d.src + (size_t)Fk * d.K + R]; }
      *(float*)(a.wimg + d.dst + (size_t)t * 4) = val * d.scale;
    }
  }
  if (d.bias_n_pad > 0 && bx == 0) {
    float* bo = (float*)(a.wimg + d.dst + (size_t)nfrag_lanes * Pol::FRAGB);
    for (int i = threadIdx.x; i < d.bias_n_pad; i += 256) bo[i] = (i < d.bias_n) ? a.params[d.bias_src + i] * d.scale : 0.f;
  }
}
template <class Pol>
__global__ void __launch_bounds__(256) k_pack(const PackArgs a) { pack_body<Pol>(a, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x); }
template __global__ void k_pack<PolF32>(const PackArgs);
template __global__ void k_pack<PolBF16>(const PackArgs);

// The whole prologue of a concat-decoder call in ONE launch (it was k_prep_image, then k_pack: two launches and the gap between them
// in front of every step's main kernel): blocks [0, n_prep) are k_prep_image's (image = i / prep_gy, row group = i % prep_gy), the
// next pack_gx * n_pack are k_pack's.  Neither half reads what the other writes.
struct PrologueArgs {
  PrepArgs prep;
  int prep_gy, n_prep, pack_gx;
  const float* film_A; char* film_afrag; float film_scale; int film_B;  // FiLM (film_A != NULL): the first n_prep blocks are afrag_from_A_body's
};
template <class Pol>
__global__ void __launch_bounds__(256) k_prologue(const PrologueArgs a, const PackArgs ka) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int i = (int)blockIdx.x;
  if (i < a.n_prep && a.film_A != nullptr) afrag_from_A_body(a.film_A, a.film_afrag, a.film_scale, a.prep.H, a.film_B, i);
  else if (i < a.n_prep) prep_image_body(a.prep, i / a.prep_gy, i % a.prep_gy, smem);
  else pack_body<Pol>(ka, (i - a.n_prep) % a.pack_gx, (i - a.n_prep) / a.pack_gx, a.pack_gx);
}
template __global__ void k_prologue<PolF32>(const PrologueArgs, const PackArgs);
template __global__ void k_prologue<PolBF16>(const PrologueArgs, const PackArgs);

// ------------------------------------------------------------------------------------------
// epilogue kernels (all fixed-order sums: deterministic)
// ------------------------------------------------------------------------------------------
// dparams[i] = sum over workgroups of their partial, for i in [lo, n)
// (valid != nullptr: slot w counts only if valid[w] >= 0 -- the per-run slots of the FiLM persistent path; the tags are
// compacted in LDS 2048 slots at a time and the used slots summed in slot order: deterministic)
// (the plain path's block `blk`: also run by the extra blocks of k_tail_a when the step stays on one stream)
// Per-layer constants of the weight gradient (round 6).  With the W^T images of the persistent concat kernels written as 8 x the forward
// images (Layout::consistent_bwd, reni_capi.inc) the gradient w.r.t. layer l's pre-activation comes out of the chain times a constant
// that depends on l only, and so do the per-workgroup partials of dW_l / db_l; the one place every such partial passes through -- the
// fixed-order sum over workgroups -- multiplies it back: element e of the buffer behind the first layer belongs to hidden layer
// 1 + e / n_hid (n_hid = H H + H), the head behind the last.  All ones everywhere else (x 1.0f is exact).
struct LayerScale { int n_hid, L; float c[MAX_LAYERS + 1]; };
DEV float layer_scale(const LayerScale& ls, int e) {
  int k = ls.n_hid > 0 ? e / ls.n_hid : 0;
  k = k < ls.L ? k : ls.L;
  return ls.c[k];
}
DEV void reduce_partials_body(const float* part, size_t per_wg, int nwg, float* dparams, int lo, int n, int blk, float (*red2)[64],
                              const LayerScale& ls) {
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = lo + blk * 64 + lane;
  float s[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) s[q] = 0.f;
  if (e < n) {
    int q = grp;
    for (; q + 28 < nwg; q += 32) {
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += part[(size_t)(q + 4 * u) * per_wg + e];
    }
    for (; q < nwg; q += 4) s[0] += part[(size_t)q * per_wg + e];
  }
  red2[grp][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (grp == 0 && e < n) dparams[e] = ((red2[0][lane] + red2[1][lane]) + (red2[2][lane] + red2[3][lane])) * layer_scale(ls, e);
}
// The same sum over partials whose hidden layers' H x H slices are in the QUAD-ROW layout (quad_word, reni_dev_common.inc: the L0X training
// instance's): 16-byte loads.  A block is still 64 consecutive buffer words x the four slot groups (wave g: slots g, g + 4, ...), but sixteen
// lanes cover the 64 words, four words each, and the four quarters of a wave share out reduce_partials_body's eight accumulators: quarter uq
// owns s[2 uq] and s[2 uq + 1], so one wave instruction fetches 256 contiguous bytes of four slots.  Per word the arithmetic is
// reduce_partials_body's, operation for operation: s[u] takes slots grp + 4 u + 32 k in ascending k, the remainder goes into s[0], then
// ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) -- the inner pairs per quarter, the rest through LDS -- and (r0 + r1) + (r2 + r3) over the
// groups.  The permutation is undone where the sum leaves: buffer word w of the slot is handed to emit(e, sum) with e its element index in the
// flat layout (what layer_scale expects).
// Needs per_wg % 4 == 0 and lo % 4 == 0 (16-byte aligned loads, and the last thread's load stays inside its slot): make_layout pads the stride.
// red4: [4][64] of 16 bytes.  part: the slots' base; [lo, n): the words summed; hidden layers of n_hid = H H + H words from word 0.
DEV int quad_word_to_flat(int w, int H, int n_hid, int L) {
  const int k = w / n_hid, t = w - k * n_hid;
  if (k >= L || t >= H * H) return w;  // biases, the head: flat
  const int q = t >> 2, rq = q / H, col = q - rq * H;
  return k * n_hid + (4 * rq + (t & 3)) * H + col;
}
constexpr int QUAD_BLK_WORDS = 64;
template <class Emit>
DEV void reduce_partials_quad_body(const float* part, size_t per_wg, int nwg, int lo, int n, int blk, f32x4 (*red4)[64], int H, int n_hid, int L,
                                   Emit&& emit) {
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int l16 = lane & 15, uq = lane >> 4;  // sixteen lanes x 16 bytes = the block's 64 words; quarter uq of the wave owns s[2 uq], s[2 uq + 1]
  const int w = lo + blk * QUAD_BLK_WORDS + 4 * l16;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (w < n) {
    const float* const p = part + w + (size_t)(8 * uq) * per_wg;  // slot grp + 4 (2 uq) + 32 k, and the one four behind it
    int q = grp;
    // (four trips of the 32-slot loop at a time while they last: their eight loads are issued before the first add -- left to itself the
    //  compiler waits for every 16-byte load in turn -- and the adds follow in trip order.  Sixteen loads at a time cost k_tail_a a wave of
    //  occupancy, 116 VGPRs, and gave back most of the gain: profiles/partials_path.md)
    for (; q + 124 < nwg; q += 128) {
      f32x4 v[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = *(const f32x4*)(p + (size_t)(q + 32 * k) * per_wg);
        v[2 * k + 1] = *(const f32x4*)(p + (size_t)(q + 32 * k + 4) * per_wg);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 4; ++k) { s0 += v[2 * k]; s1 += v[2 * k + 1]; }
    }
    for (; q + 28 < nwg; q += 32) {
      const f32x4 a = *(const f32x4*)(p + (size_t)q * per_wg), b = *(const f32x4*)(p + (size_t)(q + 4) * per_wg);
      s0 += a; s1 += b;
    }
    if (uq == 0) {  // the remainder goes into s[0]
      for (; q < nwg; q += 4) s0 += *(const f32x4*)(p + (size_t)q * per_wg);
    }
  }
  red4[grp][lane] = s0 + s1;  // s[2 uq] + s[2 uq + 1]: the leaves of reduce_partials_body's first tree
  __syncthreads();
  if (threadIdx.x < QUAD_BLK_WORDS) {  // one word per thread: word i of the block is component i % 4 of lane i / 4's quad
    const int m = (int)threadIdx.x >> 2, c = (int)threadIdx.x & 3, ww = lo + blk * QUAD_BLK_WORDS + (int)threadIdx.x;
    float g[4];
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) g[gg] = (red4[gg][m][c] + red4[gg][16 + m][c]) + (red4[gg][32 + m][c] + red4[gg][48 + m][c]);
    if (ww < n) emit(quad_word_to_flat(ww, H, n_hid, L), (g[0] + g[1]) + (g[2] + g[3]));
  }
}
// (the tagged path's block `blk`: slot w counts only if valid[w] >= 0; also run by k_film_reduce2's second group of blocks)
DEV void reduce_partials_valid_body(const float* part, size_t per_wg, int nwg, float* dparams, int lo, int n, const int* valid, int blk) {
  // a block = 64 consecutive elements x 4 slot groups (wave g sums used slots g, g + 4, ...; eight loads in flight), the
  // groups are combined through LDS in group order: 4 x the blocks of the plain path (layer 1 alone would be 65 blocks)
  __shared__ int vl[2048];
  __shared__ int nv;
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = lo + blk * 64 + lane;
  float s[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) s[q] = 0.f;
  for (int base = 0; base < nwg; base += 2048) {
    const int cnt = nwg - base < 2048 ? nwg - base : 2048;
    __syncthreads();
    if (threadIdx.x < 64) {  // wave 0 compacts this chunk's used slots, in slot order
      int c = 0;
      for (int w0 = 0; w0 < cnt; w0 += 64) {
        const int w = w0 + (int)threadIdx.x;
        const bool ok = w < cnt && valid[base + w] >= 0;
        const unsigned long long m = __ballot(ok);
        if (ok) vl[c + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = base + w;
        c += __popcll(m);
      }
      if (threadIdx.x == 0) nv = c;
    }
    __syncthreads();
    if (e < n) {
      const int m = nv;
      int q = grp;
      for (; q + 28 < m; q += 32) {
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += part[(size_t)vl[q + 4 * u] * per_wg + e];
      }
      for (; q < m; q += 4) s[0] += part[(size_t)vl[q] * per_wg + e];
    }
  }
  red[grp][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (grp == 0 && e < n) dparams[e] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ void __launch_bounds__(256) k_reduce_partials(const float* part, size_t per_wg, int nwg,
                                                          float* dparams, int lo, int n, const int* valid, const LayerScale ls) {
  const int i = lo + blockIdx.x * 256 + threadIdx.x;
  if (valid != nullptr) {
    reduce_partials_valid_body(part, per_wg, nwg, dparams, lo, n, valid, (int)blockIdx.x);
    return;
  }
  // plain path: every slot counts.  A block = 64 consecutive elements x 4 slot groups as above (wave g sums slots g, g + 4, ... with
  // eight loads in flight; the groups are combined through LDS in group order: fixed order -> deterministic).  One thread per
  // element walking all 256-512 slots was a chain of dependent memory latencies on 260 blocks: 108 us for 85 MB beside k_reni_dw1.
  (void)i;
  __shared__ float red2[4][64];
  reduce_partials_body(part, per_wg, nwg, dparams, lo, n, (int)blockIdx.x, red2, ls);
}
// quad-row partials (every slot counts): grid = ceil((n - lo) / QUAD_BLK_WORDS) blocks of reduce_partials_quad_body
__global__ void __launch_bounds__(256) k_reduce_partials_quad(const float* part, size_t per_wg, int nwg, float* dparams, int lo, int n, int H,
                                                               const LayerScale ls) {
  __shared__ f32x4 red4[4][64];
  reduce_partials_quad_body(part, per_wg, nwg, lo, n, (int)blockIdx.x, red4, H, ls.n_hid, ls.L,
                            [&](int e, float v) { dparams[e] = v * layer_scale(ls, e); });
}

// FiLM, persistent path: k_reduce_film_runs' blocks and the tagged layer-1 partial reduction's, which both wait for k_reni_dw1 and for
// nothing else, in ONE launch (blocks [0, B gy): image runs; behind them: the partials)
struct FilmReduce2 { int H, nruns, B, gy; float* dfilm; const float* part; size_t per_wg; int nslot; float* dparams; int n; const int* valid; };
__global__ void __launch_bounds__(256) k_film_reduce2(const MainArgs a, const FilmReduce2 r) {
  const int i = (int)blockIdx.x, nb1 = r.B * r.gy;
  if (i < nb1) reduce_film_runs_body(a, r.H, r.nruns, r.dfilm, i / r.gy, i % r.gy);
  else reduce_partials_valid_body(r.part, r.per_wg, r.nslot, r.dparams, 0, r.n, r.valid, i - nb1);
}

// Per-image reduction of the per-tile partials, two fixed-order stages.
// stage A: grid (B, nchunk): sum RT_CHUNK consecutive tiles -> part2[b][chunk][H*8 + 16]
//          (dA_part[tile][h][k], k < 5 used; 16 loss/statistics slots summed over tiles and waves)
// stage B: grid B: sum the chunks -> dA[b][h][8], img_loss[b][16]
// (chunk = tiles per stage-A block: 4, so that one 256-tile image is 64 blocks -- with 16 a single image left the chip idle; the
// value does not depend on the batch: an image's sums are formed in the same order whatever batch it is part of)
constexpr int RT_CHUNK = 4;
// (tflag != NULL: only the tiles the kernel visited -- RENI_WEIGHT_SPARSE -- the others' records are stale, and would have been zero)
__global__ void __launch_bounds__(256) k_reduce_tiles_a(const float* dA_part, const float* loss_part,
                                                        int tiles_per_image, int H, float* part2, int have_dA, int chunk,
                                                        const int* tflag = nullptr) {
  const int b = blockIdx.x, ch = blockIdx.y, nch = gridDim.y;
  const int t0 = ch * chunk, t1 = min(t0 + chunk, tiles_per_image);
  float* out = part2 + ((size_t)b * nch + ch) * (H * 8 + 16);
  if (have_dA) {
    // H * 8 / 256 elements per thread (4 at H = 128), all of a tile's loads in flight together; the three padding
    // columns of a row (k >= 5) are never read
    const int k = threadIdx.x & 7;
    constexpr int MAXQ = 8;
    const int nq = (H * 8 + 255) / 256;
    float s[MAXQ];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) s[q] = 0.f;
    if (k < 5) {
#pragma unroll 4
      for (int t = t0; t < t1; ++t) {
        if (tflag != nullptr && tflag[b * tiles_per_image + t] == 0) continue;
        const float* row = dA_part + (size_t)(b * tiles_per_image + t) * H * 8 + threadIdx.x;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q)
          if (q < nq && q * 256 + (int)threadIdx.x < H * 8) s[q] += row[q * 256];
      }
    }
#pragma unroll
    for (int q = 0; q < MAXQ; ++q)
      if (q < nq && q * 256 + (int)threadIdx.x < H * 8) out[q * 256 + threadIdx.x] = s[q];
  }
  // the 16 loss / statistics slots of the chunk's (tile, wave) records: sixteen threads per slot, four loads each in flight, then a
  // fixed-order sum through LDS (one thread per slot walking 64 dependent loads was 11 us of the launch)
  {
    __shared__ float ls[16][17];
    const int slot = threadIdx.x & 15, part = threadIdx.x >> 4;  // 16 parts
    const int n = (t1 - t0) * 4;
    float v = 0.f;
    for (int t = part; t < n; t += 16) {
      if (tflag != nullptr && tflag[b * tiles_per_image + t0 + (t >> 2)] == 0) continue;
      v += loss_part[((size_t)b * tiles_per_image * 4 + t0 * 4 + t) * 16 + slot];
    }
    ls[part][slot] = v;
    __syncthreads();
    if (threadIdx.x < 16) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += ls[q][threadIdx.x];
      out[H * 8 + threadIdx.x] = s;
    }
  }
}

// stage B: grid (B, ceil((H * 8 + 16) / 256)): one element per thread, eight chunks' loads in flight, chunk order fixed
__global__ void __launch_bounds__(256) k_reduce_tiles_b(const float* part2, int nch, int H, float* dA,
                                                        float* img_loss, int have_dA) {
  const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
  const int n = H * 8 + 16;
  if (i >= n || (!have_dA && i < H * 8)) return;
  const float* in = part2 + (size_t)b * nch * n + i;
  float s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = 0.f;
  int c = 0;
  for (; c + 7 < nch; c += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += in[(size_t)(c + u) * n];
  }
  for (; c < nch; ++c) s[0] += in[(size_t)c * n];
  const float t = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  if (i < H * 8) dA[(size_t)b * H * 8 + i] = t;
  else img_loss[(size_t)b * 16 + (i - H * 8)] = t;
}

// Training instance of the persistent kernel: per-image sums arrive as image RUNS (MainArgs::pruns), one per (workgroup,
// image) pair -- a handful per image instead of one partial per tile.  grid B; fixed order (workgroup, then run).
__global__ void __launch_bounds__(256) k_reduce_runs(const float* pruns, const int* prun_image, int nwg, int kmax, int H,
                                                     int tiles_per_image, int n_tiles, float* dA, float* img_loss) {
  const int b = blockIdx.x;
  // workgroups whose tile range [g n / G, (g + 1) n / G) can meet the image's [b tpi, (b + 1) tpi): a safe superset,
  // the run's image tag decides
  int g0 = (int)((long long)b * tiles_per_image * nwg / n_tiles) - 1;
  int g1 = (int)((long long)(b + 1) * tiles_per_image * nwg / n_tiles) + 1;
  g0 = g0 < 0 ? 0 : g0;
  g1 = g1 > nwg - 1 ? nwg - 1 : g1;
  const int stride = H * 8 + 16;
  // the image's runs, in (workgroup, run) order: every candidate's tag is fetched in parallel (one dependent global load
  // per candidate and output element made this kernel 39 us), the ordered list is then built from LDS
  constexpr int MAXC = 1024;
  __shared__ int tag[MAXC];
  __shared__ int list[MAXC];
  __shared__ int nlist;
  const int ncand = (g1 - g0 + 1) * kmax;  // <= (256 + 2) * kmax; kmax is 2 unless a workgroup's range spans whole images
  for (int c = threadIdx.x; c < ncand && c < MAXC; c += 256) tag[c] = prun_image[g0 * kmax + c];
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int c = 0; c < ncand && c < MAXC; ++c)
      if (tag[c] == b) list[n++] = g0 * kmax + c;
    nlist = n;
  }
  __syncthreads();
  if (gridDim.y == 1) {
    // grid (B): one block per image, a handful of runs each (large batches: 18 us at B = 64, beside k_reni_dw1 and not on the
    // critical path; many small blocks instead were slower there, 37 us -- three dependent round trips per block)
    for (int i = threadIdx.x; i < H * 8 + 16; i += 256) {
      float s = 0.f;
      for (int q = 0; q < nlist; ++q) s += pruns[(size_t)list[q] * stride + i];
      for (int c = MAXC; c < ncand; ++c)  // (never at the shipped shapes: more than 1024 candidate runs for one image)
        if (prun_image[g0 * kmax + c] == b) s += pruns[(size_t)(g0 * kmax + c) * stride + i];
      if (i < H * 8) dA[(size_t)b * H * 8 + i] = s;
      else img_loss[(size_t)b * 16 + (i - H * 8)] = s;  // (slots 0..3: one per wave, summed below; the rest are zero)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float* q = img_loss + (size_t)b * 16;
      const float e = (q[0] + q[1]) + (q[2] + q[3]);
      q[0] = e; q[1] = 0.f; q[2] = 0.f; q[3] = 0.f;
    }
    return;
  }
  // grid (B, ceil((H * 8 + 16) / 64)), small batches (few images, each with dozens of runs: 64 at B = 4): a block = 64 output
  // elements x 4 run groups (wave g sums runs g, g + 4, ..., eight loads in flight), combined through LDS in group order:
  // 45 -> 13 us at B = 4.
  {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int n = H * 8 + 16, i = blockIdx.y * 64 + lane, nl = nlist;
    float s8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s8[u] = 0.f;
    if (i < n) {
      for (int q = grp; q < nl; q += 32) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool in = q + 4 * u < nl;  // (a short last group re-reads run q)
          const float v = pruns[(size_t)list[in ? q + 4 * u : q] * stride + i];
          s8[u] += in ? v : 0.f;
        }
      }
    }
    red[grp][lane] = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    __syncthreads();
    if (grp == 0) {  // (whole wave: the loss slots are combined with lane shuffles below)
      float t = 0.f;
      if (i < n) {
        t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        for (int c = MAXC; c < ncand; ++c)  // (never at the shipped shapes: more than 1024 candidate runs for one image)
          if (prun_image[g0 * kmax + c] == b) t += pruns[(size_t)(g0 * kmax + c) * stride + i];
      }
      if ((int)blockIdx.y * 64 >= H * 8) {
        // the block behind dA holds the 16 loss slots in lanes 0..15: slots 0..3 are one per wave of the training kernel and
        // become their sum in slot 0, as the consumers (k_finalize_loss) expect; the rest are zero
        const float e = (__shfl(t, 0, 64) + __shfl(t, 1, 64)) + (__shfl(t, 2, 64) + __shfl(t, 3, 64));
        if (lane < 16) img_loss[(size_t)b * 16 + lane] = (lane == 0) ? e : (lane < 4 ? 0.f : t);
      } else if (i < n) {
        dA[(size_t)b * H * 8 + i] = t;
      }
    }
  }
}

// FiLM: dfilm[b][i] = sum over the image's tiles of dfp_part[tile][i], i over [L][2][H] (fixed order)
__global__ void __launch_bounds__(256) k_reduce_film(const float* dfp_part, int tiles_per_image, int n, float* dfilm) {
  const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  const float* q = dfp_part + (size_t)b * tiles_per_image * n + i;
  float s0 = 0.f, s1 = 0.f;
  int t = 0;
  for (; t + 1 < tiles_per_image; t += 2) { s0 += q[(size_t)t * n]; s1 += q[(size_t)(t + 1) * n]; }
  if (t < tiles_per_image) s0 += q[(size_t)t * n];
  dfilm[(size_t)b * n + i] = s0 + s1;
}

// RENI_WEIGHT_SPARSE: which tiles can change the result.  A pixel whose loss weight is zero in all three channels contributes an
// exact zero to the weighted squared error and to every gradient; the cosine term (loss_functions.py:25-32: cosine similarity ALONG
// THE PIXEL AXIS, times the weight of pixel 0) sees every pixel of an image -- unless the image's pixel-0 weight is zero, which makes
// that term a constant.  (The notebook's inpainting masks, examples.ipynb cell 4: Mask-3 keeps rows 20-93 x columns 81-164 of
// 128 x 256 -- 148 of an image's 256 tiles, and pixel 0 is masked.)
//   k_tile_flags  : one wave per tile: tflag[tile] = any weight of its 128 pixels != 0; img_cos[b] = any channel of pixel 0 != 0
//   k_tile_compact: ONE block: list_main = tiles with tflag | img_cos[image] (ascending), list_stats = tiles of images with img_cos,
//                   counts[0 / 1] their lengths; tflag[tile] becomes "visited by the main pass" (the reductions' skip test)
// RENI_WEIGHT_COMPACT goes one step further: an image's pixels with weight are PACKED into its first tiles (k_pix_scatter writes the
// position -> pixel list, the kernels read a lane's pixel through it) -- Mask-3: 49 tiles per image instead of 148.  The sums are the
// same terms in another order: equal to rounding, not bit for bit.
// (a tile's pixels with weight, as two 64-bit masks: pixel p0 + lane in m0, p0 + 64 + lane in m1)
DEV void tile_live_masks(const float* w, long long ws1, long long ws2, int P, int p0, int lane, unsigned long long& m0, unsigned long long& m1) {
  bool nz[2] = {false, false};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int p = p0 + lane + 64 * u;
    if (p < P) {
#pragma unroll
      for (int c = 0; c < 3; ++c) nz[u] |= w[(size_t)p * ws1 + (size_t)c * ws2] != 0.f;
    }
  }
  m0 = __ballot(nz[0]);
  m1 = __ballot(nz[1]);
}
// (pcnt != NULL, RENI_WEIGHT_COMPACT: + the tile's number of pixels with weight)
__global__ void __launch_bounds__(256) k_tile_flags(const float* weight, long long ws0, long long ws1, long long ws2, int P,
                                                    int tiles_per_image, int n_tiles, int* tflag, int* img_cos, int* pcnt) {
  const int tile = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= n_tiles) return;
  const int b = tile / tiles_per_image, p0 = (tile - b * tiles_per_image) * 128;
  const float* w = weight + (size_t)b * ws0;
  unsigned long long m0, m1;
  tile_live_masks(w, ws1, ws2, P, p0, lane, m0, m1);
  if (lane == 0) {
    tflag[tile] = (m0 | m1) != 0ull;
    if (pcnt != nullptr) pcnt[tile] = __popcll(m0) + __popcll(m1);
    if (p0 == 0) img_cos[b] = (w[0] != 0.f) | (w[ws2] != 0.f) | (w[2 * ws2] != 0.f);
  }
}
// RENI_WEIGHT_COMPACT: plist[b * P + k] = the image's k-th pixel with weight (every pixel, in order, for an image whose cosine term is
// live); pscan = k_tile_compact's exclusive scan of the tiles' counts.  One wave per tile, as k_tile_flags.
__global__ void __launch_bounds__(256) k_pix_scatter(const float* weight, long long ws0, long long ws1, long long ws2, int P,
                                                     int tiles_per_image, int n_tiles, const int* img_cos, const int* pscan, int* plist) {
  const int tile = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= n_tiles) return;
  const int b = tile / tiles_per_image, p0 = (tile - b * tiles_per_image) * 128;
  unsigned long long m0, m1;
  if (img_cos[b] != 0) {
    m0 = __ballot(p0 + lane < P);
    m1 = __ballot(p0 + 64 + lane < P);
  } else {
    tile_live_masks(weight + (size_t)b * ws0, ws1, ws2, P, p0, lane, m0, m1);
  }
  int* const out = plist + (size_t)b * P + (pscan[tile] - pscan[b * tiles_per_image]);
  const unsigned long long below = (1ull << lane) - 1ull;
  if ((m0 >> lane) & 1ull) out[__popcll(m0 & below)] = p0 + lane;
  if ((m1 >> lane) & 1ull) out[__popcll(m0) + __popcll(m1 & below)] = p0 + 64 + lane;
}
// (every thread owns a run of ceil(n_tiles / 1024) consecutive tiles: a serial scan of its run, ONE block-wide scan of the 1024 run
// totals per pass -- as 1024-tile chunks with three barriers and a global round trip each, the launch took 17 us at 5 376 tiles)
DEV int block_excl_scan_1024(int v, int* wsum, int& total) {  // exclusive prefix of v over the block's 1024 threads (thread order)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  __syncthreads();  // (wsum's previous readers are done)
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { const int x = wsum[w]; off += (w < wave) ? x : 0; tot += x; }
  total = tot;
  return off + incl - v;
}
__global__ void __launch_bounds__(1024) k_tile_compact(int* tflag, const int* img_cos, int tiles_per_image, int n_tiles,
                                                       int* list_main, int* list_stats, int* counts,
                                                       const int* pcnt, int P, int* pscan, int* nlive) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  const int run = (n_tiles + 1023) / 1024;
  const int t_lo = tid * run < n_tiles ? tid * run : n_tiles, t_hi = t_lo + run < n_tiles ? t_lo + run : n_tiles;
  int total;
  if (pcnt != nullptr) {
    // RENI_WEIGHT_COMPACT, first: pscan = exclusive scan of the tiles' live-pixel counts (all of a tile's pixels for an image whose
    // cosine term is live), nlive[b] = the image's total; a tile is then visited iff its first POSITION lies below nlive[b]
    auto cnt = [&](int t) -> int {
      const int b = t / tiles_per_image, p0 = (t - b * tiles_per_image) * 128;
      return img_cos[b] != 0 ? (P - p0 < 128 ? P - p0 : 128) : pcnt[t];
    };
    int sum = 0;
#pragma unroll 8
    for (int t = t_lo; t < t_hi; ++t) sum += cnt(t);
    int off = block_excl_scan_1024(sum, wsum, total);
#pragma unroll 8
    for (int t = t_lo; t < t_hi; ++t) { pscan[t] = off; off += cnt(t); }  // (the counts again: L2 hits, no per-thread array)
    if (tid == 0) pscan[n_tiles] = total;
    __syncthreads();  // (the block's own global writes are visible to it behind the barrier)
    const int B = n_tiles / tiles_per_image;
    for (int b = tid; b < B; b += 1024) nlive[b] = pscan[(b + 1) * tiles_per_image] - pscan[b * tiles_per_image];
    __syncthreads();
  }
  // the two lists: flags of the thread's run, block-wide scans of the run totals, then the run's entries in order
  unsigned am = 0u, as = 0u;  // (bit i: tile t_lo + i; runs longer than 32 tiles are re-evaluated in the write loop)
  int nm = 0, ns = 0;
  auto flags_of = [&](int t, bool& m, bool& s_) {
    const int b = t / tiles_per_image;
    s_ = img_cos[b] != 0;
    m = s_ || (pcnt != nullptr ? (t - b * tiles_per_image) * 128 < nlive[b] : tflag[t] != 0);
  };
#pragma unroll 8
  for (int t = t_lo; t < t_hi; ++t) {
    bool m, s_;
    flags_of(t, m, s_);
    if (t - t_lo < 32) { am |= (m ? 1u : 0u) << (t - t_lo); as |= (s_ ? 1u : 0u) << (t - t_lo); }
    nm += m; ns += s_;
  }
  int tm, ts_;
  int om = block_excl_scan_1024(nm, wsum, tm);
  int os = block_excl_scan_1024(ns, wsum, ts_);
  for (int t = t_lo; t < t_hi; ++t) {
    bool m, s_;
    if (t - t_lo < 32) { m = (am >> (t - t_lo)) & 1u; s_ = (as >> (t - t_lo)) & 1u; }
    else flags_of(t, m, s_);
    tflag[t] = m ? 1 : 0;
    if (m) list_main[om++] = t;
    if (s_) list_stats[os++] = t;
  }
  if (tid == 0) { counts[0] = tm; counts[1] = ts_; }
}

// cosine-term coefficients per (image, channel) from the forward statistics:
// stats[b][c] = cA, stats[b][4+c] = cB, stats[b][8+c] = cosine similarity * pixel-0 weight
// RENITestLoss's statistics pass in ONE launch behind the forward-only kernel (it was k_reduce_tiles_a -> k_reduce_tiles_b ->
// k_cos_coeffs): block b sums image b's (tile, wave) records -- sixteen slots, sixteen parts of eight loads in flight each, the parts
// combined in a fixed order: an image's sums do not depend on its batch -- then forms the three channels' coefficients.
// (img_cos != NULL, RENI_WEIGHT_SPARSE: an image whose pixel-0 weight is zero in every channel was left out of the statistics pass --
// every coefficient of it carries that weight as a factor: zeros, and its records are not read)
__global__ void __launch_bounds__(256) k_stats_image(const float* loss_part, int tiles_per_image, const float* weight, long long ws0,
                                                     long long ws2, float beta, float* img_loss, float* stats,
                                                     const int* img_cos = nullptr) {
  __shared__ float ls[16][17];
  __shared__ float tot[16];
  const int b = blockIdx.x, slot = threadIdx.x & 15, part = threadIdx.x >> 4;
  if (img_cos != nullptr && img_cos[b] == 0) {  // (uniform per block)
    if (threadIdx.x < 16) { img_loss[(size_t)b * 16 + threadIdx.x] = 0.f; stats[(size_t)b * 16 + threadIdx.x] = 0.f; }
    return;
  }
  const int n = tiles_per_image * 4;
  const float* base = loss_part + (size_t)b * n * 16 + slot;
  float s8[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s8[u] = 0.f;
  int t = part;
  for (; t + 7 * 16 < n; t += 8 * 16) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s8[u] += base[(size_t)(t + 16 * u) * 16];
  }
  for (; t < n; t += 16) s8[0] += base[(size_t)t * 16];
  ls[part][slot] = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
  __syncthreads();
  if (threadIdx.x < 16) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += ls[q][threadIdx.x];
    tot[threadIdx.x] = v;
    img_loss[(size_t)b * 16 + threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {  // (k_cos_coeffs' arithmetic)
    const int c = threadIdx.x;
    const float sot = tot[1 + c], soo = tot[4 + c], stt = tot[7 + c];
    const float no = sqrtf(soo), nt = sqrtf(stt);
    const float den = fmaxf(no * nt, 1e-20f);
    const float cs = sot / den;
    const float s0 = weight[(size_t)b * ws0 + (size_t)c * ws2];  // weight of pixel 0 (loss_functions.py:29)
    stats[(size_t)b * 16 + c] = -beta * s0 / (3.f * den);
    stats[(size_t)b * 16 + 4 + c] = -beta * s0 * cs / (3.f * soo);
    stats[(size_t)b * 16 + 8 + c] = cs * s0;
  }
}

// loss_terms = (loss, mse, prior, cosine)
DEV void finalize_loss_body(const float* img_loss, const float* stats, const float* Z, int B, int P, int nz, int has_cos, int has_prior,
                            float alpha, float beta, float* loss_terms, float (*red)[256]) {
  // three fixed-shape tree reductions (deterministic): per-image MSE terms, per-image cosine terms, |Z|^2
  float mse = 0.f, cosv = 0.f, prior = 0.f;
  float m_ = 0.f, c_ = 0.f, zz = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    m_ += img_loss[(size_t)b * 16] / (3.f * (float)P);
    if (has_cos) c_ += 1.f - (stats[(size_t)b * 16 + 8] + stats[(size_t)b * 16 + 9] + stats[(size_t)b * 16 + 10]) / 3.f;
  }
  if (has_prior)
    for (int i = threadIdx.x; i < nz; i += 256) zz += Z[i] * Z[i];
  red[0][threadIdx.x] = zz; red[1][threadIdx.x] = m_; red[2][threadIdx.x] = c_;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  mse = red[1][0]; cosv = red[2][0];
  if (threadIdx.x == 0) {
    prior = alpha * red[0][0];
    cosv *= beta;
    loss_terms[0] = mse + prior + cosv;
    loss_terms[1] = mse;
    loss_terms[2] = prior;
    loss_terms[3] = cosv;
  }
}
__global__ void k_finalize_loss(const float* img_loss, const float* stats, const float* Z, int B, int P,
                                int nz, int has_cos, int has_prior, float alpha, float beta, float* loss_terms) {
  __shared__ float red[3][256];
  finalize_loss_body(img_loss, stats, Z, B, P, nz, has_cos, has_prior, alpha, beta, loss_terms, red);
}

// per image: m[col] = W0[:,col]^T g_c (g_c = constant-column gradient dA[:,4]) and, for the inner-product
// block, u[col][xyz] = W_ip[:,col]^T dA[:,xyz].   grid (B, ceil(F/64)); 4 row groups x 64 columns per block
__global__ void __launch_bounds__(256) k_tail_m(const TailArgs a) {
  // Two memory round trips, not 2 x H / 32: the kernel runs beside k_reni_dw1_ring, whose LDS-DMA ring keeps the memory system's
  // queues full -- every DEPENDENT load of a neighbour then waits microseconds (eight rounds of eight loads: 96 us beside it,
  // 16 us alone).  The image's dA goes to LDS in one go and a row group's H / 4 weight loads are issued together.
  __shared__ float red[4][64][4];
  __shared__ float dAs[256 * 8];
  const int F = a.F_in, nd = a.nd, H = a.H, b = blockIdx.x;
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.y * 64 + c;
  const float* dAb = a.dA + (size_t)b * H * 8;
  constexpr int RPT = 32;  // rows per batch of loads
  const int h0 = rg * (H / 4), h1 = h0 + H / 4;
  float w[RPT];
#pragma unroll
  for (int u = 0; u < RPT; ++u) w[u] = (col < F && h0 + u < h1) ? a.W0[(size_t)(h0 + u) * F + col] : 0.f;
  for (int i = threadIdx.x; i < H * 8; i += 256) dAs[i] = dAb[i];
  __syncthreads();
  float s = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  if (col < F) {
    for (int h = h0; h < h1; h += RPT) {
      if (h > h0) {  // (H = 256: the second batch)
#pragma unroll
        for (int u = 0; u < RPT; ++u) w[u] = (h + u < h1) ? a.W0[(size_t)(h + u) * F + col] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RPT; ++u) {
        if (h + u < h1) {
          const float* q = dAs + (h + u) * 8;
          s += w[u] * q[4];
          if (col < nd) { sx += w[u] * q[0]; sy += w[u] * q[1]; sz += w[u] * q[2]; }
        }
      }
    }
  }
  red[rg][c][0] = s; red[rg][c][1] = sx; red[rg][c][2] = sy; red[rg][c][3] = sz;
  __syncthreads();
  if (rg == 0 && col < F) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (red[0][c][k] + red[1][c][k]) + (red[2][c][k] + red[3][c][k]);
    a.mcol[(size_t)b * F + col] = t[0];
    if (col < nd) {
      float* u = a.ucol + ((size_t)b * nd + col) * 3;
      u[0] = t[1]; u[1] = t[2]; u[2] = t[3];
    }
  }
}

// assemble dZ from m / u (SURVEY.md Appendix A).  grid B
DEV void tail_dz_body(const TailArgs& a, const int b) {
  const int F = a.F_in, nd = a.nd, tid = threadIdx.x;
  const float* m = a.mcol + (size_t)b * F;
  const float* u = a.ucol + (size_t)b * nd * 3;
  const float* z = a.Z + (size_t)b * nd * 3;
  for (int t = tid; t < nd * 3; t += 256) {
    const int i = t / 3, k = t - 3 * i;
    float val = 0.f;
    if (a.eq == 1) {
      if (k == 1) {
        val = m[nd + nd * nd + 1 + i];
      } else {
        val = u[i * 3 + k];
        for (int q = 0; q < nd; ++q) val += (m[nd + i * nd + q] + m[nd + q * nd + i]) * z[q * 3 + k];
      }
    } else if (a.eq == 2) {
      val = u[i * 3 + k];
      for (int q = 0; q < nd; ++q) val += (m[nd + i * nd + q] + m[nd + q * nd + i]) * z[q * 3 + k];
    } else {
      val = u[i * 3 + k] + m[nd + i * 3 + k];
    }
    val += 2.f * a.alpha2 * z[t];  // prior term d(alpha |Z|^2) (0 unless RENITestLoss)
    a.dZ[(size_t)b * nd * 3 + t] = val;
  }
}

// ------------------------------------------------------------------------------------------
// The per-image epilogue of the persistent TRAINING path in TWO launches (it was k_reduce_runs -> k_tail_m -> k_tail_dz ->
// k_finalize_loss -> k_tail_dw0: five dependent launches on the side stream, each waiting out the launch latency of the one before).
//   k_tail_a, grid (B, ny): block (b, y) sums image b's runs into LDS (every block of the image does: a handful of 4 KB runs),
//     block y = 0 publishes dA_b and the image's loss sum; with need_dz every block then forms its 64 columns of m = W0^T g_c
//     (k_tail_m's arithmetic; the weight loads are issued before anything else).
//   k_tail_b, one grid of three kinds of blocks that all depend on k_tail_a alone: [0, B) assemble dZ_b (k_tail_dz), block B
//     finalises the loss terms (k_finalize_loss's fixed-shape tree), the rest form dW0 / db0 (k_tail_dw0).
// (A single launch with 'last block of the image' / 'last image' counters was tried first: on this multi-XCD part every
//  agent-scope fence writes back / invalidates a whole XCD's L2, and 1 400 blocks doing so beside k_reni_dw1_ring doubled ITS run
//  time -- 127 -> 243 us, profiles/r04_tail.md.  The kernel boundary is the cheap synchronisation here.)
// ------------------------------------------------------------------------------------------
struct TailFusedArgs {
  TailArgs t;            // (t.dA is written by k_tail_a: [B][H][8])
  const float* pruns; const int* prun_image; int nwg, kmax, tpi, n_tiles;
  float* dA_out; float* img_loss;
  const float* stats; int P, nz, has_cos, has_prior; float alpha, beta; float* loss_terms;  // loss_terms == nullptr: no loss to finalise
  int need_dz, need_dw0, dw0_gx;
  const long long* idx_now; const long long* idx_staged;  // both non-NULL in a staged step (reni_train_step_rows): must agree per image
  int* skip_flag;  // reni_train_step_rows: k_tail_b's loss block writes 1 here if the staged batch is not the call's batch (else 0), and
                   // k_adam2 then leaves parameters, table and moments untouched -- the step is SKIPPED, loudly (loss and gradients NaN)
  // k_tail_a on ONE stream (small problems: no side stream): the blocks with blockIdx.x >= t.B are k_reduce_partials' plain blocks
  // for the weight-gradient partials of layers >= 2 -- 85 MB of bandwidth-bound reads beside the per-image latency chains, one launch less
  const float* rp_part; size_t rp_per_wg; int rp_nwg, rp_lo, rp_n; float* rp_out; LayerScale rp_ls;
  int rp_quad;  // the partials are in the quad-row layout (the L0X training instance's): reduce_partials_quad_body's blocks
};
constexpr int TF_LMAX = 512;  // runs of one image kept in the LDS list (an image meets at most one run per workgroup: <= #CUs)
constexpr int tail_a_lds_bytes(int H) { return (H * 8 + 16) * 4 + 4 * 64 * 4 * 4 + TF_LMAX * 4; }
__global__ void __launch_bounds__(256) k_tail_a(const TailFusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((int)blockIdx.x >= a.t.B) {  // (uniform per block) the partial reduction's blocks, see TailFusedArgs
    const int blk = ((int)blockIdx.x - a.t.B) * (int)gridDim.y + (int)blockIdx.y;
    if (a.rp_quad) {
      static_assert(tail_a_lds_bytes(32) >= 4 * 64 * 16, "red4 fits the dynamic LDS at every width");
      reduce_partials_quad_body(a.rp_part, a.rp_per_wg, a.rp_nwg, a.rp_lo, a.rp_n, blk, (f32x4 (*)[64])smem, a.t.H, a.rp_ls.n_hid, a.rp_ls.L,
                                [&](int e, float v) { a.rp_out[e] = v * layer_scale(a.rp_ls, e); });
      return;
    }
    reduce_partials_body(a.rp_part, a.rp_per_wg, a.rp_nwg, a.rp_out, a.rp_lo, a.rp_n, blk, (float (*)[64])smem, a.rp_ls);
    return;
  }
  const int H = a.t.H, F = a.t.F_in, nd = a.t.nd, b = blockIdx.x, tid = threadIdx.x;
  float* const dAs = (float*)smem;                                   // [H * 8 + 16]
  float (*const red)[64][4] = (float (*)[64][4])(dAs + H * 8 + 16);  // [4][64][4]
  int* const list = (int*)(red + 4);                                 // [TF_LMAX]
  __shared__ int nlist;
  const int c = tid & 63, rg = tid >> 6;
  const int col = blockIdx.y * 64 + c;
  // (1) this thread's weights for the m slice: independent of everything below, so their latency hides behind the run sums
  constexpr int RPT = 32;
  const int h0 = rg * (H / 4), h1 = h0 + H / 4;
  float w[RPT];
  if (a.need_dz) {
#pragma unroll
    for (int u = 0; u < RPT; ++u) w[u] = (col < F && h0 + u < h1) ? a.t.W0[(size_t)(h0 + u) * F + col] : 0.f;
  }
  // (2) the image's runs in (workgroup, run) order: wave 0 compacts the candidates' tags with ballots
  int g0 = (int)((long long)b * a.tpi * a.nwg / a.n_tiles) - 1;
  int g1 = (int)((long long)(b + 1) * a.tpi * a.nwg / a.n_tiles) + 1;
  g0 = g0 < 0 ? 0 : g0;
  g1 = g1 > a.nwg - 1 ? a.nwg - 1 : g1;
  const int ncand = (g1 - g0 + 1) * a.kmax;
  if (tid < 64) {
    int n = 0;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
      const int cc = c0 + tid;
      const bool ok = cc < ncand && a.prun_image[g0 * a.kmax + cc] == b;
      const unsigned long long m = __ballot(ok);
      const int pos = n + __popcll(m & ((1ull << tid) - 1ull));
      if (ok && pos < TF_LMAX) list[pos] = g0 * a.kmax + cc;
      n += __popcll(m);
    }
    if (tid == 0) nlist = n;
  }
  __syncthreads();
  {
    const int stride = H * 8 + 16, nl = nlist < TF_LMAX ? nlist : TF_LMAX;
    for (int e = tid; e < stride; e += 256) {
      float s8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) s8[u] = 0.f;
      int q = 0;
      for (; q + 8 <= nl; q += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) s8[u] += a.pruns[(size_t)list[q + u] * stride + e];
      }
      for (int u = 0; q + u < nl; ++u) s8[u] += a.pruns[(size_t)list[q + u] * stride + e];
      float sv = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
      if (nlist > TF_LMAX) {  // (never at the shipped shapes: the runs behind the list, in candidate order)
        int seen = 0;
        for (int cc = 0; cc < ncand; ++cc)
          if (a.prun_image[g0 * a.kmax + cc] == b && seen++ >= TF_LMAX) sv += a.pruns[(size_t)(g0 * a.kmax + cc) * stride + e];
      }
      // (a staged step whose batch is not the batch that was staged for it: every result of the image becomes NaN)
      if (a.idx_now != nullptr && a.idx_now[b] != a.idx_staged[b]) sv = __builtin_nanf("");
      dAs[e] = sv;
    }
  }
  __syncthreads();
  if (blockIdx.y == 0) {
    for (int i = tid; i < H * 8; i += 256) a.dA_out[(size_t)b * H * 8 + i] = dAs[i];
    if (tid < 16) {  // slots 0..3: one per wave of the training kernel -> their sum in slot 0 (what the loss finaliser reads)
      const float* q = dAs + H * 8;
      a.img_loss[(size_t)b * 16 + tid] = tid == 0 ? (q[0] + q[1]) + (q[2] + q[3]) : tid < 4 ? 0.f : q[tid];
    }
  }
  if (!a.need_dz) return;
  // (3) m[col] = W0[:, col]^T g_c and, for the inner-product block, u[col][xyz] = W_ip[:, col]^T dA[:, xyz]  (k_tail_m)
  float sm = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  if (col < F) {
    for (int h = h0; h < h1; h += RPT) {
      if (h > h0) {  // (H = 256: the second batch)
#pragma unroll
        for (int u = 0; u < RPT; ++u) w[u] = (h + u < h1) ? a.t.W0[(size_t)(h + u) * F + col] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RPT; ++u) {
        if (h + u < h1) {
          const float* q = dAs + (h + u) * 8;
          sm += w[u] * q[4];
          if (col < nd) { sx += w[u] * q[0]; sy += w[u] * q[1]; sz += w[u] * q[2]; }
        }
      }
    }
  }
  red[rg][c][0] = sm; red[rg][c][1] = sx; red[rg][c][2] = sy; red[rg][c][3] = sz;
  __syncthreads();
  if (rg == 0 && col < F) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (red[0][c][k] + red[1][c][k]) + (red[2][c][k] + red[3][c][k]);
    a.t.mcol[(size_t)b * F + col] = t[0];
    if (col < nd) {
      float* u = a.t.ucol + ((size_t)b * nd + col) * 3;
      u[0] = t[1]; u[1] = t[2]; u[2] = t[3];
    }
  }
}

DEV void tail_dz_body(const TailArgs& a, const int b);
DEV void tail_dw0_body(const TailArgs& a, const int bx, const int h);
DEV void finalize_loss_body(const float* img_loss, const float* stats, const float* Z, int B, int P, int nz, int has_cos, int has_prior,
                            float alpha, float beta, float* loss_terms, float (*red)[256]);
__global__ void __launch_bounds__(256) k_tail_b(const TailFusedArgs a) {
  __shared__ float red[3][256];
  const int i = (int)blockIdx.x, B = a.t.B;
  const int n_dz = a.need_dz ? B : 0;
  if (i < n_dz) {
    tail_dz_body(a.t, i);
    // a staged step whose batch is not the batch that was staged for it: the image's latent gradient is NaN on EVERY path (the
    // persistent path's k_tail_a poisons dA as well; the generic kernels -- fp32, other widths -- come through here only)
    if (a.idx_now != nullptr && a.idx_now[i] != a.idx_staged[i]) {
      __syncthreads();
      for (int t = threadIdx.x; t < a.t.nd * 3; t += 256) a.t.dZ[(size_t)i * a.t.nd * 3 + t] = __builtin_nanf("");
    }
    return;
  }
  if (i == n_dz) {
    if (a.loss_terms != nullptr)
      finalize_loss_body(a.img_loss, a.stats, a.t.Z, B, a.P, a.nz, a.has_cos, a.has_prior, a.alpha, a.beta, a.loss_terms, red);
    if (a.skip_flag != nullptr) {  // (one block: every image's pair of indices)
      __shared__ int bad;
      if (threadIdx.x == 0) bad = 0;
      __syncthreads();
      if (a.idx_now != nullptr)
        for (int b = threadIdx.x; b < B; b += 256)
          if (a.idx_now[b] != a.idx_staged[b]) bad = 1;
      __syncthreads();
      if (threadIdx.x == 0) *a.skip_flag = bad;
      if (bad && a.loss_terms != nullptr && threadIdx.x < 4) a.loss_terms[threadIdx.x] = __builtin_nanf("");
    }
    return;
  }
  const int j = i - n_dz - 1;  // dW0 / db0 blocks: (j % dw0_gx, j / dw0_gx) = k_tail_dw0's (blockIdx.x, blockIdx.y)
  tail_dw0_body(a.t, j % a.dw0_gx, j / a.dw0_gx);
}

// dW0[h][col] and db0[h]: sums over the batch of per-image outer products
DEV void tail_dw0_body(const TailArgs& a, const int bx, const int h) {
  const int F = a.F_in, nd = a.nd, H = a.H, B = a.B;
  const int col = bx * 256 + threadIdx.x;
  if (col > F) return;
  if (col == F) {  // bias
    float s = 0.f;
#pragma unroll 8
    for (int b = 0; b < B; ++b) s += a.dA[((size_t)b * H + h) * 8 + 4];
    a.db0[h] = s;
    return;
  }
  // per-thread sum over the batch: the loads of different images are independent -- unrolled so that eight are
  // in flight (the rolled loop was a 64-deep chain of L2 latencies, 58 us for 11 MFLOP)
  float s = 0.f;
  int kind = 0;  // 0: constant column, 1: inner-product column, 2: r, 3: dy
  if (col < nd) kind = 1;
  else if (a.eq == 1 && col == nd + nd * nd) kind = 2;
  else if (a.eq == 1 && col == F - 1) kind = 3;
  const float* q0 = a.dA + (size_t)h * 8;
  const size_t qs = (size_t)H * 8;
  if (kind == 0) {
    const float* xc = a.xconst + col;
#pragma unroll 8
    for (int b = 0; b < B; ++b) s += q0[b * qs + 4] * xc[(size_t)b * F];
  } else if (kind == 1) {
    const float* z0 = a.Z + (size_t)col * 3;
    const size_t zs = (size_t)nd * 3;
    const float wy = (a.eq == 1) ? 0.f : 1.f;
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const float* q = q0 + b * qs;
      const float* z = z0 + b * zs;
      s += q[0] * z[0] + wy * q[1] * z[1] + q[2] * z[2];
    }
  } else {
    const int k = (kind == 2) ? 3 : 1;
#pragma unroll 8
    for (int b = 0; b < B; ++b) s += q0[b * qs + k];
  }
  a.dW0[(size_t)h * F + col] = s;
}

// One element of torch.optim.Adam (non-amsgrad): m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
// denom = sqrt(v) / sqrt(bias_correction2) + eps; p -= lr / bias_correction1 * m / denom.  Every rounding is pinned
// (no contraction left to the compiler), so the three kernels that use it agree bit for bit.
DEV void adam_apply(float* p, float* m, float* v, long long i, float g, float gscale, float lr, float b1, float b2, float eps,
                    float bc1, float bc2_sqrt) {
  const float gi = __fmul_rn(g, gscale);
  const float mi = __fmaf_rn(b1, m[i], __fmul_rn(1.f - b1, gi));
  const float vi = __fmaf_rn(b2, v[i], __fmul_rn(__fmul_rn(1.f - b2, gi), gi));
  m[i] = mi; v[i] = vi;
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vi), bc2_sqrt), eps);
  p[i] = __fsub_rn(p[i], __fmul_rn(__fdiv_rn(lr, bc1), __fdiv_rn(mi, denom)));
}

// The same step over a TABLE of n_rows x row_len parameters whose gradient is given for the B rows idx[0..B) only
// (g_rows [B][row_len]; repeated indices accumulate, like index_add_); every other row has gradient zero and still
// moves by its momentum -- the dense Adam over the whole latent table that the reference runs (RENI_module.py:178-192).
// Replaces zero_() + index_add_() + k_adam: no dense gradient buffer.
__global__ void __launch_bounds__(256) k_adam_rows(float* p, const float* g_rows, const long long* idx, int B, int row_len,
                                                   float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                                                   float bc1, float bc2_sqrt, float gscale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long r = i / row_len;
  const int c = (int)(i - r * row_len);
  float gi = 0.f;
  for (int b = 0; b < B; ++b)
    if (idx[b] == r) gi += g_rows[(size_t)b * row_len + c];
  adam_apply(p, m, v, i, gi, gscale, lr, b1, b2, eps, bc1, bc2_sqrt);
}

// flat[i] *= scale: the 1 / world_size of the data-parallel mean behind reni_allreduce_grads' RCCL sum
// x += y (the image chunks of run_backward_chunked: decoder gradient and loss terms are sums over images)
__global__ void __launch_bounds__(256) k_add_into(float* x, const float* y, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] += y[i];
}

__global__ void __launch_bounds__(256) k_scale(float* x, size_t n, float scale) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] *= scale;
}

// Both updates of a training step in ONE launch: blocks [0, nb_dec) run k_adam's body on the flat decoder buffer, the
// rest k_adam_rows' on the latent table (same hyper-parameters: the reference has one optimiser over all parameters,
// RENI_module.py:178-192).
struct Adam2Args {
  float* p; const float* g; float* m; float* v; long long n; int nb_dec;
  float* tp; const float* g_rows; const long long* idx; int B, row_len; float* tm; float* tv; long long tn;
  float lr, b1, b2, eps, bc1, bc2_sqrt, gscale;
  // reni_train_step_rows on the persistent path: decoder elements [skip_lo, skip_hi) -- layer 1 -- are not read from g: their
  // gradient is still k_reni_dw1's per-workgroup partials, and the nb_l1 blocks behind the table's first SUM them (k_reduce_partials'
  // plain order), store the sum in g and take the Adam step: layer 1's reduction costs no launch of its own
  long long skip_lo, skip_hi;
  const float* l1_part; size_t l1_per_wg; int l1_nwg, nb_l1;
  float l1_scale;  // LayerScale::c[0] (layer 1's constant: this launch is where its partials are summed on the fused path)
  const int* skip_step;  // optional: non-zero there = leave everything untouched (a staged step met another batch: k_tail_b's skip_flag)
};
__global__ void __launch_bounds__(256) k_adam2(const Adam2Args a) {
  const int nb_tab = (int)((a.tn + 255) / 256);
  if (a.skip_step != nullptr && *a.skip_step != 0) {  // (uniform over the grid)
    // a skipped step's gradients are NaN everywhere: layer 1's slice of g is written by THIS launch on the fused path (its blocks
    // below), so they fill it here instead of leaving the caller's uninitialised memory behind (ADVICE r05)
    if ((int)blockIdx.x >= a.nb_dec + nb_tab) {
      const int e = ((int)blockIdx.x - a.nb_dec - nb_tab) * 64 + (threadIdx.x & 63);
      if ((threadIdx.x >> 6) == 0 && e < (int)(a.skip_hi - a.skip_lo)) const_cast<float*>(a.g)[a.skip_lo + e] = __builtin_nanf("");
    }
    return;
  }
  if ((int)blockIdx.x >= a.nb_dec + nb_tab) {  // layer 1: 64 elements x 4 slot groups per block
    __shared__ float red2[4][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int n = (int)(a.skip_hi - a.skip_lo);
    const int e = ((int)blockIdx.x - a.nb_dec - nb_tab) * 64 + lane;
    float s[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = 0.f;
    if (e < n) {
      int q = grp;
      for (; q + 28 < a.l1_nwg; q += 32) {
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += a.l1_part[(size_t)(q + 4 * u) * a.l1_per_wg + e];
      }
      for (; q < a.l1_nwg; q += 4) s[0] += a.l1_part[(size_t)q * a.l1_per_wg + e];
    }
    red2[grp][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (grp == 0 && e < n) {
      const float gsum = ((red2[0][lane] + red2[1][lane]) + (red2[2][lane] + red2[3][lane])) * a.l1_scale;
      const_cast<float*>(a.g)[a.skip_lo + e] = gsum;
      adam_apply(a.p, a.m, a.v, a.skip_lo + e, gsum, a.gscale, a.lr, a.b1, a.b2, a.eps, a.bc1, a.bc2_sqrt);
    }
    return;
  }
  const bool dec = (int)blockIdx.x < a.nb_dec;
  const long long i = (long long)(dec ? blockIdx.x : blockIdx.x - a.nb_dec) * 256 + threadIdx.x;
  if (i >= (dec ? a.n : a.tn)) return;
  if (dec && i >= a.skip_lo && i < a.skip_hi) return;
  float gi = 0.f;
  if (dec) {
    gi = a.g[i];
  } else {
    const long long r = i / a.row_len;
    const int c = (int)(i - r * a.row_len);
    for (int b = 0; b < a.B; ++b)
      if (a.idx[b] == r) gi += a.g_rows[(size_t)b * a.row_len + c];
  }
  adam_apply(dec ? a.p : a.tp, dec ? a.m : a.tm, dec ? a.v : a.tv, i, gi, a.gscale, a.lr, a.b1, a.b2, a.eps, a.bc1, a.bc2_sqrt);
}

__global__ void __launch_bounds__(256) k_adam(float* p, const float* g, float* m, float* v, long long n,
                                              float lr, float b1, float b2, float eps, float bc1,
                                              float bc2_sqrt, float gscale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  adam_apply(p, m, v, i, g[i], gscale, lr, b1, b2, eps, bc1, bc2_sqrt);
}

// ------------------------------------------------------------------------------------------
// MFMA layout probes (reni_selftest_layouts)
// ------------------------------------------------------------------------------------------
// probe 0: fp32 32x32x2 : D = A(32x2) B(2x32) with the operand/result maps the kernels assume
// probe 1: bf16 32x32x16
__global__ void k_probe(float* outD, int which) {
  const int lane = threadIdx.x, hi = lane >> 5, j = lane & 31;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (which == 0) {
    // A[i][k] = 1 + i + 100 k ; B[k][n] = 3 + 2 n + 7 k
    const float av = 1.f + j + 100.f * hi;
    const float bv = 3.f + 2.f * j + 7.f * hi;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  } else {
    // A[i][k] = ((i + 3k) % 7) - 3 ; B[k][n] = ((2n + k) % 5) - 2 ; k = 8*hi + e  (exact in bf16)
    bf16x8 av, bv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * hi + e;
      av[e] = (__bf16)(float)(((j + 3 * k) % 7) - 3);
      bv[e] = (__bf16)(float)(((2 * j + k) % 5) - 2);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) outD[rowmap(r, hi) * 32 + j] = acc[r];
}

// probe of ds_read_b64_tr_b16: LDS holds u16 element i = i; lane l reads at byte address 8*l (mode 0) or
// at a caller-given per-lane byte address (mode 1); out[l*4 + e] = element e returned to lane l
__global__ void k_probe_tr(unsigned short* out, const int* lane_addr, int mode) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[4096];
  for (int i = threadIdx.x; i < 4096; i += 64) lds[i] = (unsigned short)i;
  __syncthreads();
  const unsigned addr = (unsigned)(size_t)lds + (mode == 0 ? threadIdx.x * 8 : lane_addr[threadIdx.x]);
  unsigned long long v;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  for (int e = 0; e < 4; ++e) out[threadIdx.x * 4 + e] = (unsigned short)(v >> (16 * e));
}

