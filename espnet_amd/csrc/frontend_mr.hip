// Log-mel frontend for a general STFT size: framed STFT(n_fft) -> power -> banded mel -> log with a mixed-radix FFT.
// n_fft even, 64 <= n_fft <= 1024, H = n_fft / 2 = 2^a 3^b 5^c.  The 512-point kernels of csrc/frontend.hip stay what
// they are; this file is a second kernel with the same semantics (the reference lines cited at the top of frontend.hip:
// center=True with reflect padding, at the utterance's own length when wlens is given; window zero padded to n_fft;
// one-sided spectrum; re^2 + im^2; banded mel; max(., 1e-10); log; frames >= flens[b] written as 0).
//
// Work split (that of frontend_logmel_kernel2): one wave per frame, four waves per workgroup, a wave walks FR frames.
//
// FFT.  The real frame is packed as z[n] = x[2n] + i x[2n+1] (an H-point complex FFT) and untangled into bins 0 .. H.
// Stockham autosort over the radix plan of em_stft_radix_plan (radix 4 first, then one 2, then the 3s, then the 5s: at
// most 5 stages for every size but 972, which has 6).  Stage s with radix r and p = the product of the radices before
// it does H / r butterflies, lane l takes i = l, l + 64, ...:
//     k = i mod p;  u[q] = in[i + (H / r) q] W_{rp}^{kq};  out[(i - k) r + k + q' p] = DFT_r(u)[q']
// One generic kernel loops over the plan at run time (the radix switch is wave-uniform); a stage's butterflies are
// compile-time code (stage<R>).  i mod p is taken with the plan's f32 reciprocal of p: i + 0.5 is never closer than
// 1 / 1024 (relative) to a multiple of p, five hundred times the rounding of the product.
//
// Where the state lives.  Frame-independent per lane, in registers: its window values (n_fft / 64 <= 16) and the mel
// weights (below).  Frame-independent per workgroup, in LDS, loaded once before the frame loop: the twiddle table the
// host built in float64 (2 H + 1 complex: stage s at offset p_s - 1 as [q - 1][k] = W_{rp}^{kq}, which are H - 1
// entries over all stages; then W_{n_fft}^k, k = 0 .. H, at offset H).  The stage twiddles cannot sit in registers
// under a run-time plan (up to 8 per stage, indexed by stage), so a butterfly reads r - 1 of them beside its r points.
// Per wave, in LDS: two ping-pong tiles of complex points (8-byte accesses) and H + 1 power bins followed by zeroed
// slack.  Between the steps only __builtin_amdgcn_wave_barrier(): a wave's LDS operations execute in order and no wave
// reads another's tiles.  The one __syncthreads() is in front of the frame loop (the twiddle table).
// LDS at H = 512, pad 6: 8.2 KiB + 4 x (2 x 608 x 8 + 564 x 4) = 55 KiB, dynamic, so the small sizes take less
// (n_fft 400: 20 - 22 KiB) and nothing above the 64 KiB default is asked for.
//
// Tile padding.  Point a sits at P(a) = a + c (a >> 5): c 8-byte slots of padding per 32.  frontend.hip's fpad (4 words
// per 32) is derived for the radix-4 strides 16 and 64 only.  A stage's q'-th store puts runs of p consecutive points
// r p apart, and with 3 or 5 in r p the runs' residues mod 32 wander instead of repeating (r = 3, p = 8: 24 g mod 32 =
// 0, 24, 16, 8 is conflict-free unpadded and 2-way at c = 4), while the consecutive reads, which start at multiples of
// H / r that are no multiples of 32 either, lose a little with every c > 0.  No single c serves all plans, so the
// launcher counts, per H and once, the bank passes of every stage's loads and stores for c = 0 .. 6 under the model
// "a 32-lane half of an 8-byte access takes as many passes as its fullest of 32 slots (address mod 32)" and takes the
// cheapest c, the smallest on a tie (mr_choose_pad; 512 -> what the count says, not fpad's value by decree).  The choice
// rests on that model alone: no per-pad timing and no LDS bank-conflict counter has been taken on the device, only the
// kernel's time with the chosen pad (profiles/frontend_nfft_bench.json).  The count is ~1e5 host operations, too many
// for every launch, so the entry keeps the result per H.
//
// Mel.  One lane per filter in rounds of 64.  Weights: registers behind a template on the band-length bucket, ML = 24
// or 48 taps for up to two rounds (n_mels <= 128); taps past the band carry zero weights and read the zeroed slack, so
// the frame loop has no per-tap predicate.  Wider bands or more filters (n_fft 1024 with 23 filters: 100+ taps) take
// ML = 0: mel_lo and the weights are read from global memory (L1 / L2 hits after the first frame) tap by tap for every
// frame, any band length, any n_mels.  LDS is no home for them: such a bank is 10 - 12 KiB and unbounded in general,
// and at n_fft 1024 the tiles and the twiddles already take 49 - 55 of the 64 KiB.  Timed as the 23-filter leg of
// tools/frontend_nfft_bench.py.
#include "em_common.h"

namespace {

constexpr int MR_MAX_STAGES = 6;  // n_fft 972: H = 486 = 2 3^5
constexpr int MR_MAX_PAD = 6;
constexpr int MR_SLACK = 48;  // zeroed words behind the H + 1 power bins: the largest register band

struct MrPlan {
  int H, ns, pad, tile, powlen;  // tile: complex slots per tile; powlen: floats of a wave's power row
  int r[MR_MAX_STAGES], p[MR_MAX_STAGES];
  float invp[MR_MAX_STAGES];
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cscale(float s, float2 a) { return make_float2(s * a.x, s * a.y); }
__device__ __forceinline__ float2 mul_neg_i(float2 a) { return make_float2(a.y, -a.x); }  // -i a

// forward DFTs of u[0 .. R), e^{-2 pi i m q / R}
template <int R>
__device__ __forceinline__ void bfly(float2* u);
template <>
__device__ __forceinline__ void bfly<2>(float2* u) {
  const float2 a = u[0], b = u[1];
  u[0] = cadd(a, b);
  u[1] = csub(a, b);
}
template <>
__device__ __forceinline__ void bfly<4>(float2* u) {
  const float2 a = cadd(u[0], u[2]), b = csub(u[0], u[2]), c = cadd(u[1], u[3]), d = mul_neg_i(csub(u[1], u[3]));
  u[0] = cadd(a, c);
  u[2] = csub(a, c);
  u[1] = cadd(b, d);
  u[3] = csub(b, d);
}
template <>
__device__ __forceinline__ void bfly<3>(float2* u) {
  // y0 = u0 + s, y1,2 = (u0 - s / 2) -+ i (sqrt(3) / 2) (u1 - u2): two real-by-complex multiplies
  const float2 s = cadd(u[1], u[2]);
  const float2 d = mul_neg_i(cscale(0.86602540378443865f, csub(u[1], u[2])));
  const float2 t = make_float2(fmaf(-0.5f, s.x, u[0].x), fmaf(-0.5f, s.y, u[0].y));
  u[0] = cadd(u[0], s);
  u[1] = cadd(t, d);
  u[2] = csub(t, d);
}
template <>
__device__ __forceinline__ void bfly<5>(float2* u) {
  // five real-by-complex multiplies: with a1 = u1 + u4, a2 = u2 + u3, b1 = u1 - u4, b2 = u2 - u3 and c1,2 = cos(2,4 pi / 5),
  // s1,2 = sin(2,4 pi / 5):  c1 a1 + c2 a2 = -(a1 + a2) / 4 + (c1 - c2) / 2 (a1 - a2)  (c1 + c2 = -1 / 2), and
  // s1 b1 + s2 b2 = (s1 - s2) b1 + s2 (b1 + b2),  s2 b1 - s1 b2 = s2 (b1 + b2) - (s1 + s2) b2
  const float2 a1 = cadd(u[1], u[4]), a2 = cadd(u[2], u[3]), b1 = csub(u[1], u[4]), b2 = csub(u[2], u[3]);
  const float2 s = cadd(a1, a2);
  const float2 m1 = make_float2(fmaf(-0.25f, s.x, u[0].x), fmaf(-0.25f, s.y, u[0].y));
  const float2 m2 = cscale(0.55901699437494742f, csub(a1, a2));
  const float2 t1 = cadd(m1, m2), t2 = csub(m1, m2);
  const float2 w = cscale(0.58778525229247313f, cadd(b1, b2));  // s2 (b1 + b2)
  const float2 v1 = mul_neg_i(make_float2(fmaf(0.36327126400268045f, b1.x, w.x), fmaf(0.36327126400268045f, b1.y, w.y)));
  const float2 v2 = mul_neg_i(make_float2(fmaf(-1.5388417685876267f, b2.x, w.x), fmaf(-1.5388417685876267f, b2.y, w.y)));
  u[0] = cadd(u[0], s);
  u[1] = cadd(t1, v1);
  u[4] = csub(t1, v1);
  u[2] = cadd(t2, v2);
  u[3] = csub(t2, v2);
}

__device__ __forceinline__ int mr_pad(int a, int c) { return a + c * (a >> 5); }

// one Stockham stage of radix R: src -> dst (padded tiles), twiddles tws = the stage's [R - 1][p] table in LDS
template <int R>
__device__ __forceinline__ void stage(const float2* src, float2* dst, const float2* tws, int H, int p, float invp, int c,
                                      int lane) {
  const int m = H / R;
  for (int i = lane; i < m; i += 64) {
    const int g = (int)(((float)i + 0.5f) * invp);
    const int k = i - g * p;
    float2 u[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float2 v = src[mr_pad(i + m * q, c)];
      u[q] = q == 0 ? v : cmul(v, tws[(q - 1) * p + k]);
    }
    bfly<R>(u);
    const int j = g * p * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) dst[mr_pad(j + q * p, c)] = u[q];
  }
}

__device__ __forceinline__ int reflect_idx(int p, int N) {
  if (p < 0) p = -p;
  if (p >= N) p = 2 * (N - 1) - p;
  return p;
}

template <int ML>
__global__ __launch_bounds__(256) void frontend_logmel_mr_kernel(
    const float* __restrict__ wav, int N, int hop, const float* __restrict__ window, const float2* __restrict__ twid,
    const MrPlan plan, int FR, const float* __restrict__ melw, const int* __restrict__ mel_lo, int mel_maxlen, int n_mels,
    const int* __restrict__ flens, const int* __restrict__ wlens, int T_f, float* __restrict__ feats) {
  extern __shared__ __attribute__((aligned(16))) float2 s_mr[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.y;
  const int H = plan.H, n_fft = 2 * H, c = plan.pad;
  const int ntw = 2 * H + 2;  // (2 H + 1 entries, rounded to 16 bytes)
  float2* const tws = s_mr;
  float2* const tile0 = s_mr + ntw + wave * 2 * plan.tile;
  float2* const tile1 = tile0 + plan.tile;
  float* const pw = (float*)(s_mr + ntw + 8 * plan.tile) + wave * plan.powlen;
  const float* x = wav + (size_t)b * N;
  const int Nb = wlens ? (wlens[b] < N ? wlens[b] : N) : N;
  const int flen = flens[b];

  for (int i = threadIdx.x; i < 2 * H + 1; i += 256) tws[i] = twid[i];
  // ---- frame-independent state of this lane
  float2 win[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int n = lane + 64 * m;
    win[m] = n < H ? *(const float2*)(window + 2 * n) : make_float2(0.f, 0.f);
  }
  constexpr int MLR = ML > 0 ? ML : 1;
  float wA[2][MLR];
  const float* pwA[2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int mm = lane + 64 * rd;
    const int mf = mm < n_mels ? mm : n_mels - 1;
    int lo = mel_lo[mf];
    lo = lo < 0 ? 0 : (lo > H ? H : lo);
    pwA[rd] = pw + lo;
#pragma unroll
    for (int s = 0; s < MLR; ++s) wA[rd][s] = (ML > 0 && s < mel_maxlen && lo + s <= H) ? melw[s * n_mels + mf] : 0.f;
  }
  for (int i = H + 1 + lane; i < plan.powlen; i += 64) pw[i] = 0.f;
  __syncthreads();  // the twiddle table; the only workgroup barrier

  for (int fi = 0; fi < FR; ++fi) {
    const int t = (blockIdx.x * FR + fi) * 4 + wave;
    if (t >= T_f) break;  // (wave-uniform)
    // ---- load + window: z[n] = x[2n] + i x[2n+1], n = lane + 64 m
    const int start = t * hop - H;
    const bool plain = start >= 0 && start + n_fft <= Nb && !(((size_t)b * N + start) & 1);  // (wave-uniform)
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int n = lane + 64 * m;
      if (n < H) {
        float2 v;
        if (plain) {
          v = *(const float2*)(x + start + 2 * n);
        } else {
          int i0 = reflect_idx(start + 2 * n, Nb), i1 = reflect_idx(start + 2 * n + 1, Nb);
          i0 = i0 < 0 ? 0 : (i0 < N ? i0 : N - 1);  // frames past flens[b] are zeroed below: keep them in range
          i1 = i1 < 0 ? 0 : (i1 < N ? i1 : N - 1);
          v = make_float2(x[i0], x[i1]);
        }
        tile0[mr_pad(n, c)] = make_float2(v.x * win[m].x, v.y * win[m].y);
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the plan's stages
    float2* src = tile0;
    float2* dst = tile1;
    for (int s = 0; s < plan.ns; ++s) {
      const int p = plan.p[s];
      const float2* tw = tws + (p - 1);
      switch (plan.r[s]) {
        case 4: stage<4>(src, dst, tw, H, p, plan.invp[s], c, lane); break;
        case 2: stage<2>(src, dst, tw, H, p, plan.invp[s], c, lane); break;
        case 3: stage<3>(src, dst, tw, H, p, plan.invp[s], c, lane); break;
        default: stage<5>(src, dst, tw, H, p, plan.invp[s], c, lane); break;
      }
      float2* const tmp = src;
      src = dst;
      dst = tmp;
      __builtin_amdgcn_wave_barrier();
    }
    // ---- real-FFT untangle + power, bins k = 0 .. H:  X[k] = E + W_{n_fft}^k O,  E = (Z[k] + conj Z[H - k]) / 2,
    // O = -i (Z[k] - conj Z[H - k]) / 2, indices mod H
    for (int k = lane; k <= H; k += 64) {
      const int ka = k == H ? 0 : k, kb = (k == 0 || k == H) ? 0 : H - k;
      const float2 zk = src[mr_pad(ka, c)];
      float2 zc = src[mr_pad(kb, c)];
      zc.y = -zc.y;
      const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
      const float2 dlt = csub(zk, zc);
      const float2 o = make_float2(0.5f * dlt.y, -0.5f * dlt.x);
      const float2 xo = cmul(tws[H + k], o);
      const float xr = e.x + xo.x, xi = e.y + xo.y;
      pw[k] = xr * xr + xi * xi;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- banded mel + log
    const bool valid_frame = t < flen;
    float* out = feats + ((size_t)b * T_f + t) * n_mels;
    if (ML > 0) {
#pragma unroll
      for (int rd = 0; rd < 2; ++rd) {
        if (rd == 1 && n_mels <= 64) break;  // (wave-uniform)
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < MLR; ++s) acc = fmaf(pwA[rd][s], wA[rd][s], acc);
        acc = fmaxf(acc, 1e-10f);
        if (lane + 64 * rd < n_mels) out[lane + 64 * rd] = valid_frame ? logf(acc) : 0.f;
      }
    } else {
      for (int mf = lane; mf < n_mels; mf += 64) {
        int lo = mel_lo[mf];
        lo = lo < 0 ? 0 : (lo > H ? H : lo);
        const int n = mel_maxlen < H + 1 - lo ? mel_maxlen : H + 1 - lo;
        float acc = 0.f;
        for (int s = 0; s < n; ++s) acc = fmaf(pw[lo + s], melw[s * n_mels + mf], acc);
        acc = fmaxf(acc, 1e-10f);
        out[mf] = valid_frame ? logf(acc) : 0.f;
      }
    }
    __builtin_amdgcn_wave_barrier();  // (the next frame's loads into the tile come after this frame's reads of it)
  }
}

// passes of one 8-byte access of up to 64 lanes under the model stated at the top: per 32-lane half, the fullest slot
int mr_passes(const int* addr, int n) {
  int total = 0;
  for (int h = 0; h < n; h += 32) {
    int cnt[32] = {0}, worst = 0;
    for (int l = h; l < n && l < h + 32; ++l) worst = ++cnt[addr[l] & 31] > worst ? cnt[addr[l] & 31] : worst;
    total += worst;
  }
  return total;
}

int mr_choose_pad(const MrPlan& pl) {
  int best = 0;
  long best_cost = -1;
  for (int c = 0; c <= MR_MAX_PAD; ++c) {
    long cost = 0;
    for (int s = 0; s < pl.ns; ++s) {
      const int r = pl.r[s], p = pl.p[s], m = pl.H / r;
      for (int i0 = 0; i0 < m; i0 += 64) {
        const int n = m - i0 < 64 ? m - i0 : 64;
        for (int q = 0; q < r; ++q) {
          int rd[64], wr[64];
          for (int l = 0; l < n; ++l) {
            const int i = i0 + l, k = i % p, a = i + m * q, j = (i - k) * r + k + q * p;
            rd[l] = a + c * (a >> 5);
            wr[l] = j + c * (j >> 5);
          }
          cost += mr_passes(rd, n) + mr_passes(wr, n);
        }
      }
    }
    if (best_cost < 0 || cost < best_cost) best_cost = cost, best = c;
  }
  return best;
}

}  // namespace

// The radix plan of H = n_fft / 2: radix 4 first, then one 2, then the 3s, then the 5s.  Returns the number of stages,
// 0 for an unsupported size; radix has room for 6.  espnet_amd/layers/stft_plan.py states the same rule for the
// twiddle table, and tests/test_cpu_frontend_nfft.py holds the two together for every size.
extern "C" int em_stft_radix_plan(int32_t n_fft, int32_t* radix) {
  if (n_fft < 64 || n_fft > 1024 || (n_fft & 1)) return 0;
  int h = n_fft / 2, e2 = 0, e3 = 0, e5 = 0;
  while (h % 2 == 0) h /= 2, ++e2;
  while (h % 3 == 0) h /= 3, ++e3;
  while (h % 5 == 0) h /= 5, ++e5;
  if (h != 1) return 0;
  int ns = 0;
  for (int i = 0; i < e2 / 2; ++i) radix[ns++] = 4;
  if (e2 & 1) radix[ns++] = 2;
  for (int i = 0; i < e3; ++i) radix[ns++] = 3;
  for (int i = 0; i < e5; ++i) radix[ns++] = 5;
  return ns;  // (<= 6: the powers of two take at most 5, H <= 512 = 4^4 2; of the sizes with a 3 or a 5 only 2 3^5 has 6)
}

extern "C" int em_frontend_logmel_nfft_f32(const float* wav, int32_t B, int32_t N, int32_t n_fft, int32_t hop,
                                           const float* window, const float* twiddles, const float* mel_packed,
                                           const int32_t* mel_lo, int32_t mel_maxlen, int32_t n_mels,
                                           const int32_t* flens, const int32_t* wlens, int32_t T_f, float* feats,
                                           void* stream) {
  int32_t radix[8];
  const int ns = em_stft_radix_plan(n_fft, radix);
  if (ns == 0 || ns > MR_MAX_STAGES) return EM_ERR_UNSUPPORTED;
  const int H = n_fft / 2;
  if (!wav || !window || !twiddles || !mel_packed || !mel_lo || !flens || !feats) return EM_ERR_BAD_ARG;
  if (B <= 0 || B > 65535 || T_f <= 0) return EM_ERR_BAD_ARG;
  if (N <= H || hop <= 0 || T_f != 1 + N / hop) return EM_ERR_BAD_ARG;
  if (mel_maxlen < 1 || mel_maxlen > H + 1 || n_mels < 1) return EM_ERR_BAD_ARG;
  MrPlan pl;
  pl.H = H;
  pl.ns = ns;
  int p = 1;
  for (int s = 0; s < MR_MAX_STAGES; ++s) {
    pl.r[s] = s < ns ? radix[s] : 1;
    pl.p[s] = p;
    pl.invp[s] = 1.0f / (float)p;
    if (s < ns) p *= radix[s];
  }
  static signed char pad_of[513];  // chosen pad + 1 per H; 0: not counted yet (idempotent, so a race only repeats the count)
  int pad = __atomic_load_n(&pad_of[H], __ATOMIC_RELAXED) - 1;
  if (pad < 0) {
    pad = mr_choose_pad(pl);
    __atomic_store_n(&pad_of[H], (signed char)(pad + 1), __ATOMIC_RELAXED);
  }
  pl.pad = pad;
  pl.tile = (H + pad * ((H + 31) >> 5) + 1) & ~1;
  pl.powlen = (H + 1 + MR_SLACK + 3) & ~3;
  const size_t lds = (size_t)(2 * H + 2 + 8 * pl.tile) * sizeof(float2) + (size_t)4 * pl.powlen * sizeof(float);
  if (lds > 64 * 1024) return EM_ERR_UNSUPPORTED;
  // frames per wave: the rule of em_frontend_logmel_f32 (8 for a batch, 2 where that would leave the chip mostly idle)
  const int FR = (long)em_cdiv(T_f, 32) * B < 256 ? 2 : 8;
  dim3 grid(em_cdiv(T_f, 4 * FR), B);
  const float2* tw = (const float2*)twiddles;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, wav, N, hop, window, tw, pl, FR, mel_packed, mel_lo,
                       mel_maxlen, n_mels, flens, wlens, T_f, feats);
  };
  if (n_mels > 128 || mel_maxlen > MR_SLACK) launch(frontend_logmel_mr_kernel<0>);
  else if (mel_maxlen <= 24) launch(frontend_logmel_mr_kernel<24>);
  else launch(frontend_logmel_mr_kernel<MR_SLACK>);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
