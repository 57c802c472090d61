// espnet_amd — Mask-CTC decoding on gfx950 (contract: include/espnet_amd.h, "Mask-CTC").  Reference:
// espnet2/asr/maskctc_model.py MaskCTCInference.forward, espnet2/asr/decoder/mlm_decoder.py MLMDecoder.forward.
//
// One greedy CTC pass that keeps the winning probability of every frame, a collapse that keeps the largest one of every
// run, and then K dense passes of the MLM decoder over the ragged batch, each followed by the easiest-first fill - all
// enqueued, nothing read back between the passes.  The decoder pass is csrc/dec_seq.hip's chain with the self-attention
// taken without the diagonal (em_dec_full_attention, csrc/lm_seq.hip).  What this file adds:
//   head_top_*        rows x vocabulary projection leaving (max, arg-max, sum-exp) per row: the [M][V] logits never exist.
//                     With the LayerNorm in front it is the MLM decoder's head (max logit, arg-max), without it the CTC
//                     head (arg-max, probability = 1 / sum-exp);
//   maskctc_collapse  runs of equal ids -> tokens with the run's largest probability, the threshold, the counts;
//   maskctc_fill      one pass of the mask-predict selection, ranked by counting in LDS.
#include <limits.h>
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

using em_host::Bump;
using em_host::gemm;
using em_host::LN_EPS;

// ---- a row's record over a set of columns: the maximum logit, the sum of exp(logit - maximum) and the lowest column that
// holds the maximum (csrc/transducer.hip Top with the sum-exp of csrc/lm_seq.hip Lse)
struct TopRec {
  float m, s;
  int i;
};
__device__ __forceinline__ TopRec top_merge(TopRec a, TopRec b) {
  TopRec r;
  r.m = fmaxf(a.m, b.m);
  r.i = (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b.i : a.i;
  r.s = (a.m == -INFINITY ? 0.f : a.s * __expf(a.m - r.m)) + (b.m == -INFINITY ? 0.f : b.s * __expf(b.m - r.m));
  return r;
}
__device__ __forceinline__ TopRec top_shfl_xor(TopRec v, int o) {
  return TopRec{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64), __shfl_xor(v.i, o, 64)};
}
// one more logit; a lane meets its columns in ascending order, so `>` keeps the lowest of equals
__device__ __forceinline__ void top_push(TopRec& a, float val, int col) {
  if (val > a.m) a.i = col;
  const float dlt = val - a.m;  // a.m = -inf at first: dlt = +inf, e = 0, s = 1
  const float e = __expf(-fabsf(dlt));
  a.s = dlt > 0.f ? a.s * e + 1.f : a.s + e;
  a.m = fmaxf(a.m, val);
}

constexpr int HEAD_ROWS = 64;    // rows of a workgroup: four 16-row MFMA tiles
constexpr int HEAD_SLICE = 512;  // vocabulary columns of a workgroup: 8 tiles of 16 for each of its 4 waves
constexpr int HEAD_DMAX = 1024;  // 64 rows of d + 8 bf16 stay inside the 160 KiB of LDS

// bf16: the shape of lm_head_nll_bf16_kernel (csrc/lm_seq.hip): workgroup (slice, row block) = 64 rows x 512 columns, the
// rows in LDS as bf16 (LN: normalised from the f32 residual rows; otherwise copied from the bf16 activations), wave w takes
// the column tiles w, w + 4, ... with the weight fragments straight from global memory; part[row][slice] receives the
// record.  Columns >= V count as -inf, rows >= M are zeros and never stored.
template <bool LN>
__global__ __launch_bounds__(256) void head_top_bf16_kernel(const void* __restrict__ xv, const float* __restrict__ g,
                                                            const float* __restrict__ be, const bf16* __restrict__ w,
                                                            const float* __restrict__ bias, int M, int V, int d,
                                                            float4* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_top_smem[];
  __shared__ float red[4][HEAD_ROWS][3];
  bf16* xs = (bf16*)head_top_smem;
  const int ldx = d + 8;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int r0 = blockIdx.y * HEAD_ROWS;
  for (int i = 0; i < 16; ++i) {
    const int rl = wave * 16 + i, r = r0 + rl;
    bf16* dst = xs + (size_t)rl * ldx;
    if (r >= M) {
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)0.f;
    } else if (LN) {
      const float* xr = (const float*)xv + (size_t)r * d;
      float s = 0.f;
      for (int c = lane; c < d; c += 64) s += xr[c];
      const float mean = wave_sum(s) / (float)d;
      float q = 0.f;
      for (int c = lane; c < d; c += 64) {
        const float t = xr[c] - mean;
        q += t * t;
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)((xr[c] - mean) * rstd * g[c] + be[c]);
    } else {
      const bf16* xr = (const bf16*)xv + (size_t)r * d;
      for (int c = lane; c < d; c += 64) dst[c] = xr[c];
    }
  }
  __syncthreads();
  TopRec rec[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) rec[rt][q] = TopRec{-INFINITY, 0.f, INT_MAX};
  const int vs0 = blockIdx.x * HEAD_SLICE;
  const int nk = d / 32;
  for (int t = wave; t < HEAD_SLICE / 16; t += 4) {
    const int v0 = vs0 + t * 16;
    if (v0 >= V) break;
    const int col = v0 + lr;
    const bf16* wrow = w + (size_t)min(col, V - 1) * d + lg * 8;
    const bf16* arow = xs + (size_t)lr * ldx + lg * 8;
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nk; ++s) {
      const bf16x8 bf = *(const bf16x8*)(wrow + s * 32);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt] = Mma<bf16>::mma(*(const bf16x8*)(arow + (size_t)rt * 16 * ldx + s * 32), bf, acc[rt]);
    }
    if (col < V) {
      const float bb = bias[col];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) top_push(rec[rt][q], acc[rt][q] + bb, col);
    }
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      TopRec a = rec[rt][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) a = top_merge(a, top_shfl_xor(a, o));
      if (lr == 0) {
        float* dst = red[wave][rt * 16 + lg * 4 + q];
        dst[0] = a.m;
        dst[1] = a.s;
        dst[2] = __int_as_float(a.i);
      }
    }
  __syncthreads();
  if (threadIdx.x < HEAD_ROWS && r0 + (int)threadIdx.x < M) {
    const int rl = threadIdx.x;
    TopRec a{red[0][rl][0], red[0][rl][1], __float_as_int(red[0][rl][2])};
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) a = top_merge(a, TopRec{red[wv][rl][0], red[wv][rl][1], __float_as_int(red[wv][rl][2])});
    part[(size_t)(r0 + rl) * gridDim.x + blockIdx.x] = make_float4(a.m, a.s, __int_as_float(a.i), 0.f);
  }
}

// a row's per-slice records -> its arg-max and either the maximum itself or the probability it has under the softmax
__global__ void head_top_merge_kernel(const float4* __restrict__ part, int M, int nsl, int as_prob, float* __restrict__ val,
                                      int32_t* __restrict__ idx) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  TopRec a{-INFINITY, 0.f, INT_MAX};
  for (int i = 0; i < nsl; ++i) {
    const float4 p = part[(size_t)r * nsl + i];
    a = top_merge(a, TopRec{p.x, p.y, __float_as_int(p.z)});
  }
  val[r] = as_prob ? 1.0f / a.s : a.m;
  idx[r] = a.i;
}

// f32 (parity path): a workgroup per row, the (normalised) row in LDS, thread t walks the columns t, t + 256, ...
template <bool LN>
__global__ __launch_bounds__(256) void head_top_f32_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ be, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int V, int d, int as_prob,
                                                           float* __restrict__ val, int32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_top_smem[];
  __shared__ float red[4][3];
  __shared__ float stat[2];
  float* xn = (float*)head_top_smem;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xr = x + (size_t)r * d;
  if (LN) {
    if (wave == 0) {
      float s = 0.f;
      for (int c = lane; c < d; c += 64) s += xr[c];
      const float mean = wave_sum(s) / (float)d;
      float q = 0.f;
      for (int c = lane; c < d; c += 64) {
        const float t = xr[c] - mean;
        q += t * t;
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
      if (lane == 0) {
        stat[0] = mean;
        stat[1] = rstd;
      }
    }
    __syncthreads();
    for (int c = tid; c < d; c += 256) xn[c] = (xr[c] - stat[0]) * stat[1] * g[c] + be[c];
  } else {
    for (int c = tid; c < d; c += 256) xn[c] = xr[c];
  }
  __syncthreads();
  TopRec a{-INFINITY, 0.f, INT_MAX};
  for (int v = tid; v < V; v += 256) {
    const float* wr = w + (size_t)v * d;
    float s = 0.f;
    for (int c = 0; c < d; ++c) s += xn[c] * wr[c];
    const float v1 = s + bias[v];
    if (v1 > a.m) a.i = v;
    const float mm = fmaxf(a.m, v1);
    a.s = a.s * expf(a.m - mm) + expf(v1 - mm);  // a.m = -inf: 0 * 0
    a.m = mm;
  }
  auto merge = [](TopRec p, TopRec q) {
    TopRec m;
    m.m = fmaxf(p.m, q.m);
    m.i = (q.m > p.m || (q.m == p.m && q.i < p.i)) ? q.i : p.i;
    m.s = (p.m == -INFINITY ? 0.f : p.s * expf(p.m - m.m)) + (q.m == -INFINITY ? 0.f : q.s * expf(q.m - m.m));
    return m;
  };
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) a = merge(a, top_shfl_xor(a, o));
  if (lane == 0) {
    red[wave][0] = a.m;
    red[wave][1] = a.s;
    red[wave][2] = __int_as_float(a.i);
  }
  __syncthreads();
  if (tid == 0) {
    TopRec t{red[0][0], red[0][1], __float_as_int(red[0][2])};
    for (int i = 1; i < 4; ++i) t = merge(t, TopRec{red[i][0], red[i][1], __float_as_int(red[i][2])});
    val[r] = as_prob ? 1.0f / t.s : t.m;
    idx[r] = t.i;
  }
}

EmLdsCap head_top_cap[2];

int head_slices(int V) { return em_cdiv(V, HEAD_SLICE); }

size_t head_top_ws_bytes(int dtype, int32_t M, int32_t V) {
  if (dtype != EM_BF16 || M <= 0 || V <= 0) return 0;
  return (size_t)M * head_slices(V) * sizeof(float4);
}

// val / idx [M] of the rows x [M][d] (LN: f32 residual rows through LayerNorm(g, be); otherwise rows in the compute dtype)
template <bool LN>
int head_top(int dtype, const void* x, const float* g, const float* be, const void* w, const float* bias, int M, int V, int d,
             int as_prob, float* val, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_F32) {
    if ((size_t)d * 4 > 64 * 1024) return EM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(head_top_f32_kernel<LN>, dim3(M), dim3(256), (size_t)d * 4, s, (const float*)x, g, be, (const float*)w,
                       bias, V, d, as_prob, val, idx);
    EM_CHECK_LAUNCH();
    return EM_OK;
  }
  if (dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (d % 32 || d > HEAD_DMAX) return EM_ERR_UNSUPPORTED;
  const int nsl = head_slices(V);
  if (em_cdiv(M, HEAD_ROWS) > 65535) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < head_top_ws_bytes(dtype, M, V)) return EM_ERR_WORKSPACE;
  const size_t lds = (size_t)HEAD_ROWS * (d + 8) * 2;
  EM_TRY(em_raise_lds_cap((const void*)head_top_bf16_kernel<LN>, lds, &head_top_cap[LN ? 1 : 0]));
  hipLaunchKernelGGL(head_top_bf16_kernel<LN>, dim3(nsl, em_cdiv(M, HEAD_ROWS)), dim3(256), lds, s, x, g, be, (const bf16*)w,
                     bias, M, V, d, (float4*)ws);
  hipLaunchKernelGGL(head_top_merge_kernel, dim3(em_cdiv(M, 256)), dim3(256), 0, s, (const float4*)ws, M, nsl, as_prob, val,
                     idx);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

// ---- collapse with confidence, one workgroup per utterance.  A frame opens a token when its id is not the blank and
// differs from the frame before it; a chunk of 256 frames counts its openings by ballot, so token j of the utterance is
// known to the thread of its first frame, which walks the run for its largest probability.  Everything behind the token
// count is written too: -1 / 0.
__global__ __launch_bounds__(256) void maskctc_collapse_kernel(const int32_t* __restrict__ ids, const float* __restrict__ prob,
                                                               const int32_t* __restrict__ olens, int T, int Lcap, int blank,
                                                               int mask_token, float p_thres, int32_t* __restrict__ tokens,
                                                               float* __restrict__ conf, int32_t* __restrict__ y_in,
                                                               int32_t* __restrict__ ylens, int32_t* __restrict__ nmask) {
  __shared__ int wcnt[4];
  __shared__ int nm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(olens[b], 0), T);
  const int32_t* id = ids + (size_t)b * T;
  const float* pr = prob + (size_t)b * T;
  int32_t* tk = tokens + (size_t)b * Lcap;
  float* cf = conf + (size_t)b * Lcap;
  int32_t* yi = y_in + (size_t)b * Lcap;
  if (tid == 0) nm = 0;
  int base = 0;  // tokens opened before this chunk (the same in every thread)
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int t = c0 + tid;
    const int me = t < n ? id[t] : blank;
    const bool opens = t < n && me != blank && (t == 0 || id[t - 1] != me);
    const unsigned long long bal = __ballot(opens);
    __syncthreads();  // the previous chunk's counts are read; nm = 0 is seen
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int j = base + __popcll(bal & ((1ull << lane) - 1ull));
    for (int wv = 0; wv < wave; ++wv) j += wcnt[wv];
    if (opens && j < Lcap) {
      float c = pr[t];
      for (int u = t + 1; u < n && id[u] == me; ++u) c = fmaxf(c, pr[u]);
      const bool masked = c < p_thres;
      tk[j] = me;
      cf[j] = c;
      yi[j] = masked ? mask_token : me;
      if (masked) atomicAdd(&nm, 1);
    }
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  }
  const int L = min(base, Lcap);
  for (int j = L + tid; j < Lcap; j += 256) {
    tk[j] = -1;
    cf[j] = 0.f;
    yi[j] = -1;
  }
  __syncthreads();
  if (tid == 0) {
    ylens[b] = L;
    nmask[b] = nm;
  }
}

// ---- one pass of the mask-predict fill, one workgroup per utterance.  With M0 = nmask0[b]: n_iter = min(K, M0) passes,
// n = M0 / n_iter positions per partial pass; pass p < n_iter - 1 takes the n masked positions with the largest score
// (equal scores: the lowest position first), pass n_iter - 1 every masked position, later passes nothing.  A masked
// position's rank is the count of masked positions ahead of it in that order, taken over the scores in LDS.
constexpr int FILL_LMAX = 2048;  // positions of a sentence: 16 KiB of LDS, Lp^2 / 256 comparisons per thread

__global__ __launch_bounds__(256) void maskctc_fill_kernel(int32_t* __restrict__ y_in, const float* __restrict__ s,
                                                           const int32_t* __restrict__ a, const int32_t* __restrict__ nmask0,
                                                           int Lp, int K, int pass, int mask_token,
                                                           int32_t* __restrict__ y_trace) {
  __shared__ float sc[FILL_LMAX];
  __shared__ int msk[FILL_LMAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t* y = y_in + (size_t)b * Lp;
  const float* sb = s + (size_t)b * Lp;
  const int32_t* ab = a + (size_t)b * Lp;
  const int M0 = nmask0[b];
  const int n_iter = M0 >= K ? K : M0;
  if (M0 > 0 && pass < n_iter) {  // (workgroup-uniform)
    const bool last = pass == n_iter - 1;
    const int n = M0 / n_iter;
    for (int j = tid; j < Lp; j += 256) {
      msk[j] = y[j] == mask_token;
      sc[j] = sb[j];
    }
    __syncthreads();
    for (int j = tid; j < Lp; j += 256) {
      if (!msk[j]) continue;
      bool take = last;
      if (!last) {
        const float mine = sc[j];
        int rank = 0;
        for (int i = 0; i < Lp; ++i) rank += (msk[i] && (sc[i] > mine || (sc[i] == mine && i < j))) ? 1 : 0;
        take = rank < n;
      }
      if (take) y[j] = ab[j];
    }
  }
  if (y_trace)  // (a thread reads back the positions it wrote itself)
    for (int j = tid; j < Lp; j += 256) y_trace[(size_t)b * Lp + j] = y[j];
}

struct RefineWs {
  size_t x, xn, qkv, ctx, h, head, s, a, total;
};
RefineWs refine_layout(int dtype, const EmDecoderWeights* dw, size_t M) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  Bump b;
  RefineWs w;
  w.x = b.take(M * dw->d * 4);
  w.xn = b.take(M * dw->d * es);
  w.qkv = b.take(M * 3 * dw->d * es);  // q | k | v of the self-attention, then the source attention's queries
  w.ctx = b.take(M * dw->d * es);
  w.h = b.take(M * dw->ff * es);
  w.head = b.take(head_top_ws_bytes(dtype, (int32_t)M, dw->vocab));
  w.s = b.take(M * 4);
  w.a = b.take(M * 4);
  w.total = b.o;
  return w;
}

bool refine_shape_ok(int dtype, const EmDecoderWeights* dw, int B, int Lp) {
  return dw && (dtype == EM_BF16 || dtype == EM_F32) && em_host::dec_seq_shape_ok(dw, B, Lp) && Lp <= FILL_LMAX;
}

}  // namespace

extern "C" size_t em_ctc_frame_top_workspace_bytes(int dtype, int32_t M, int32_t V) { return head_top_ws_bytes(dtype, M, V); }

extern "C" int em_ctc_frame_top(int dtype, const void* enc_act, const void* ctc_w, const float* ctc_b, int32_t M, int32_t V,
                                int32_t d, int32_t* ids, float* prob, void* ws, size_t ws_bytes, void* stream) {
  if (!enc_act || !ctc_w || !ctc_b || !ids || !prob || M <= 0 || V <= 0 || d <= 0) return EM_ERR_BAD_ARG;
  return head_top<false>(dtype, enc_act, nullptr, nullptr, ctc_w, ctc_b, M, V, d, 1, prob, ids, ws, ws_bytes, stream);
}

extern "C" size_t em_lm_head_top1_workspace_bytes(int dtype, int32_t M, int32_t V) { return head_top_ws_bytes(dtype, M, V); }

extern "C" int em_lm_head_top1(int dtype, const float* xrows, const float* norm_g, const float* norm_b, const void* out_w,
                               const float* out_b, int32_t M, int32_t V, int32_t d, float* smax, int32_t* amax, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!xrows || !norm_g || !norm_b || !out_w || !out_b || !smax || !amax || M <= 0 || V <= 0 || d <= 0) return EM_ERR_BAD_ARG;
  return head_top<true>(dtype, xrows, norm_g, norm_b, out_w, out_b, M, V, d, 0, smax, amax, ws, ws_bytes, stream);
}

extern "C" int em_maskctc_collapse(const int32_t* ids, const float* prob, const int32_t* olens, int32_t B, int32_t T,
                                   int32_t Lcap, int32_t blank, int32_t mask_token, float p_thres, int32_t* tokens,
                                   float* conf, int32_t* y_in, int32_t* ylens, int32_t* nmask, void* stream) {
  if (!ids || !prob || !olens || !tokens || !conf || !y_in || !ylens || !nmask || B <= 0 || T <= 0 || Lcap <= 0)
    return EM_ERR_BAD_ARG;
  hipLaunchKernelGGL(maskctc_collapse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, prob, olens, T, Lcap, blank,
                     mask_token, p_thres, tokens, conf, y_in, ylens, nmask);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" int em_maskctc_fill(int32_t* y_in, const float* s, const int32_t* a, const int32_t* nmask0, int32_t B, int32_t Lp,
                               int32_t K, int32_t pass, int32_t mask_token, int32_t* y_trace, void* stream) {
  if (!y_in || !s || !a || !nmask0 || B <= 0 || Lp <= 0 || K < 1 || pass < 0) return EM_ERR_BAD_ARG;
  if (Lp > FILL_LMAX) return EM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(maskctc_fill_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y_in, s, a, nmask0, Lp, K, pass,
                     mask_token, y_trace);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" size_t em_maskctc_refine_workspace_bytes(int dtype, const EmDecoderWeights* dw, int32_t B, int32_t Lp) {
  if (!refine_shape_ok(dtype, dw, B, Lp)) return 0;
  return refine_layout(dtype, dw, (size_t)B * Lp).total;
}

extern "C" int em_maskctc_refine(int dtype, const EmDecoderWeights* dw, const void* mem_kv, const void* mem_vT,
                                 const int32_t* klens, int32_t* y_in, const int32_t* ylens, const int32_t* nmask0, int32_t B,
                                 int32_t Lp, int32_t T, int32_t Tpad, int32_t K, int32_t mask_token, int32_t* y_trace,
                                 float* s_trace, int32_t* a_trace, void* ws, size_t ws_bytes, void* stream) {
  if (!dw || !dw->layers || !mem_kv || !mem_vT || !klens || !y_in || !ylens || !nmask0) return EM_ERR_BAD_ARG;
  if (dtype != EM_BF16 && dtype != EM_F32) return EM_ERR_BAD_ARG;
  if (B <= 0 || Lp <= 0 || T <= 0 || Tpad < T || Tpad % 32 != 0 || K < 1) return EM_ERR_BAD_ARG;
  if (dw->d <= 0 || dw->heads <= 0 || dw->d % dw->heads || Lp > dw->pe_len) return EM_ERR_BAD_ARG;
  if (mask_token < 0 || mask_token >= dw->vocab || (s_trace == nullptr) != (a_trace == nullptr)) return EM_ERR_BAD_ARG;
  if (!refine_shape_ok(dtype, dw, B, Lp)) return EM_ERR_UNSUPPORTED;
  const int M = B * Lp, V = dw->vocab, d = dw->d, ff = dw->ff, h = dw->heads;
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  const RefineWs o = refine_layout(dtype, dw, (size_t)M);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  unsigned char* base = (unsigned char*)ws;
  void *xn = base + o.xn, *qkv = base + o.qkv, *ctx = base + o.ctx, *hb = base + o.h;
  void* qs = qkv;  // q | k | v are consumed before the source attention's queries are projected
  float* xf = (float*)(base + o.x);
  for (int p = 0; p < K; ++p) {
    float* sp = s_trace ? s_trace + (size_t)p * M : (float*)(base + o.s);
    int32_t* ap = a_trace ? a_trace + (size_t)p * M : (int32_t*)(base + o.a);
    EM_TRY(em_dec_seq_embed_f32(dw->embed, dw->pe, y_in, M, V, d, Lp, dw->pe_len, xf, stream));
    for (int l = 0; l < dw->num_blocks; ++l) {
      const EmDecoderLayer& q = dw->layers[l];
      const unsigned char* kv = (const unsigned char*)mem_kv + (size_t)l * B * T * 2 * d * es;
      const unsigned char* vT = (const unsigned char*)mem_vT + (size_t)l * B * d * Tpad * es;
      EM_TRY(em_layernorm(dtype, xf, q.norm1_g, q.norm1_b, M, d, LN_EPS, xn, nullptr, stream));
      EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.self_wqkv, qkv, q.self_bqkv, M, 3 * d, d, d, 3 * d, 1.f, stream));
      EM_TRY(em_dec_full_attention(dtype, qkv, ylens, B, Lp, d, h, ctx, stream));
      EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.self_wout, xf, q.self_bout, M, d, d, d, d, 1.f, stream));
      EM_TRY(em_layernorm(dtype, xf, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
      EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.src_wq, qs, q.src_bq, M, d, d, d, d, 1.f, stream));
      EM_TRY(em_dec_seq_src_attention(dtype, qs, kv, 2 * d, vT, klens, nullptr, B, B, Lp, d, h, T, Tpad, ctx, stream));
      EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.src_wout, xf, q.src_bout, M, d, d, d, d, 1.f, stream));
      EM_TRY(em_layernorm(dtype, xf, q.norm3_g, q.norm3_b, M, d, LN_EPS, xn, nullptr, stream));
      EM_TRY(gemm(dtype, EM_EPI_RELU, xn, q.w1, hb, q.b1, M, ff, d, d, ff, 1.f, stream));
      EM_TRY(gemm(dtype, EM_EPI_RESID_F32, hb, q.w2, xf, q.b2, M, d, ff, ff, d, 1.f, stream));
    }
    EM_TRY(em_lm_head_top1(dtype, xf, dw->after_norm_g, dw->after_norm_b, dw->out_w, dw->out_b, M, V, d, sp, ap, base + o.head,
                           o.total - o.head, stream));
    EM_TRY(em_maskctc_fill(y_in, sp, ap, nmask0, B, Lp, K, p, mask_token, y_trace ? y_trace + (size_t)p * M : nullptr, stream));
  }
  return EM_OK;
}
