// espnet_amd — Mask-CTC decoding on gfx950 (contract: include/espnet_amd.h, "Mask-CTC").  Reference:
// espnet2/asr/maskctc_model.py MaskCTCInference.forward, espnet2/asr/decoder/mlm_decoder.py MLMDecoder.forward.
//
// One greedy CTC pass that keeps the winning probability of every frame, a collapse that keeps the largest one of every
// run, and then K dense passes of the MLM decoder over the ragged batch, each followed by the easiest-first fill - all
// enqueued, nothing read back between the passes.  The decoder pass is csrc/dec_seq.hip's chain (em_host::dec_seq_rows)
// with the self-attention taken without the diagonal (em_dec_full_attention, csrc/lm_seq.hip); both heads - the CTC
// frames' arg-max and probability, the decoder's max logit and arg-max - are csrc/vocab_head.hip's.  What this file adds:
//   maskctc_collapse  runs of equal ids -> tokens with the run's largest probability, the threshold, the counts;
//   maskctc_fill      one pass of the mask-predict selection, ranked by counting in LDS.
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

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

using em_host::DecSeqWs;

DecSeqWs refine_layout(int dtype, const EmDecoderWeights* dw, int M) {
  return em_host::dec_seq_layout(dtype, dw, (size_t)M, em_lm_head_top1_workspace_bytes(dtype, M, dw->vocab), true);
}

bool refine_shape_ok(int dtype, const EmDecoderWeights* dw, int B, int Lp) {
  return dw && (dtype == EM_BF16 || dtype == EM_F32) && em_host::dec_seq_shape_ok(dw, B, Lp) && Lp <= FILL_LMAX;
}

}  // namespace

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
  return refine_layout(dtype, dw, B * Lp).total;
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
  const int M = B * Lp;
  const DecSeqWs o = refine_layout(dtype, dw, M);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  unsigned char* base = (unsigned char*)ws;
  for (int p = 0; p < K; ++p) {
    float* sp = s_trace ? s_trace + (size_t)p * M : (float*)(base + o.s);
    int32_t* ap = a_trace ? a_trace + (size_t)p * M : (int32_t*)(base + o.a);
    EM_TRY(em_host::dec_seq_rows(dtype, dw, mem_kv, mem_vT, klens, nullptr, B, y_in, false, ylens, B, Lp, T, Tpad, ws, o,
                                 stream));
    EM_TRY(em_lm_head_top1(dtype, (const float*)(base + o.x), dw->after_norm_g, dw->after_norm_b, dw->out_w, dw->out_b, M,
                           dw->vocab, dw->d, sp, ap, base + o.head, o.total - o.head, stream));
    EM_TRY(em_maskctc_fill(y_in, sp, ap, nmask0, B, Lp, K, p, mask_token, y_trace ? y_trace + (size_t)p * M : nullptr, stream));
  }
  return EM_OK;
}
