// espnet_amd — the attention decoder over whole transcripts on gfx950: per-token negative log-likelihoods of a batch of
// transcripts given their encoder memories in one enqueue (contract: include/espnet_amd.h, "attention decoder over whole
// transcripts").  Reference: espnet2/asr/espnet_model.py ESPnetASRModel.nll / batchify_nll,
// espnet2/asr/decoder/transformer_decoder.py BaseTransformerDecoder.forward (tgt_mask = key padding & subsequent_mask,
// memory_mask from hlens), transformer/decoder_layer.py DecoderLayer.forward without a cache.
//
// The label-step path (csrc/search.hip decoder_step) feeds one position per call.  With the transcript known beforehand
// everything but the two attentions is row-local, so the M = B * Lp rows go through the library's GEMMs at once; the
// self-attention is csrc/lm_seq.hip's causal kernel (its token array is the key mask here) and the vocabulary head is
// em_lm_head_nll (csrc/vocab_head.hip).  The embedding and the layers are em_host::dec_seq_rows, which the Mask-CTC refinement
// (csrc/maskctc.hip) runs too, with the self-attention taken without the diagonal.  What this file adds:
//   dec_seq_embed       x[r] = embed[tok[r]] * sqrt(d) + pe[r % Lp] for all rows in one launch;
//   dec_seq_src_attn_*  source attention of Lp queries per sentence over a ragged memory of any length, a wave per 16
//                       queries of one (sentence, head) walking the memory in tiles of 32 frames.  The label step's
//                       dec_src_attn_kernel keeps a score row per frame in LDS and stops at ~1 690 frames; this one keeps
//                       nothing in LDS at all.
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

using em_host::gemm;
using em_host::LN_EPS;

// ---- x[r] = embed[tok[r]] * sqrt(d) + pe[r % Lp]  (embedding.py:93), f32 residual stream.  One workgroup per row.
__global__ __launch_bounds__(128) void dec_seq_embed_kernel(const float* __restrict__ embed, const float* __restrict__ pe,
                                                            const int32_t* __restrict__ tok, int V, int d, int Lp, float xscale,
                                                            float* __restrict__ x) {
  const int r = blockIdx.x;
  int t = tok[r];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);  // (the host refuses such ids; a stray one must not read outside the table)
  const float* e = embed + (size_t)t * d;
  const float* p = pe + (size_t)(r % Lp) * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) x[(size_t)r * d + c] = e[c] * xscale + p[c];
}

// ---- source attention, bf16 on the matrix cores.  One wave owns the 16 queries q0 .. q0 + 15 of one (sentence, head) and
// walks the frames 0 .. klen - 1 of the sentence's memory in tiles of 32.  Both products are taken transposed, as in
// lm_causal_attn_bf16_kernel, so that a lane's query never changes:
//   S^T[frame][query] = K . Q^T   A = K rows straight from mem_kv, B = Q (registers): lane (lr, lg) ends up with the scores
//                                 of query q0 + lr against the frames 16 kt + 4 lg + reg, kt = 0 | 1;
//   O^T[dv][query]    = V^T . P^T B = the lane's own eight probabilities, A = rows of mem_vT straight from global memory:
//                                 channel 16 t + lr, the frames 4 lg .. 4 lg + 3 of both half tiles (two 8-byte loads) -
//                                 the A operand uses the B operand's numbering of the 32 frames, so no value changes lanes
//                                 and no tile passes through LDS.
// The running maximum is shared by the four lane groups of a query, the running sum is per lane and meets at the end.  A
// frame at or behind klen takes p = 0.0 exactly and its V^T entries are replaced by zeros (whatever the caller left there,
// not-a-number included, contributes an exact zero); a sentence whose memory has no valid frame writes zeros.
template <int DK>
__global__ __launch_bounds__(64) void dec_seq_src_attn_bf16_kernel(const bf16* __restrict__ qs, const bf16* __restrict__ kmem,
                                                                   int ldk, const bf16* __restrict__ vT,
                                                                   const int32_t* __restrict__ klens,
                                                                   const int32_t* __restrict__ mem_of, int Bm, int Lp, int d,
                                                                   int T, int Tpad, bf16* __restrict__ ctx) {
  constexpr int NC = DK / 32, ND = DK / 16;
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  int mi = mem_of ? mem_of[b] : b;
  mi = min(max(mi, 0), Bm - 1);
  const int klen = min(max(klens[mi], 0), T);
  const size_t row0 = (size_t)b * Lp;
  const int qi = q0 + lr;
  const bf16* qrow = qs + (row0 + min(qi, Lp - 1)) * (size_t)d + h * DK + lg * 8;
  bf16x8 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) qf[c] = *(const bf16x8*)(qrow + c * 32);
  const bf16* kbase = kmem + (size_t)mi * T * ldk + h * DK + lg * 8;
  const bf16* vbase = vT + ((size_t)mi * d + h * DK + lr) * Tpad + lg * 4;
  const float scale = 1.0f / sqrtf((float)DK);
  float m = -INFINITY, l = 0.f;
  f32x4 acc[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < klen; k0 += 32) {
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const bf16* krow = kbase + (size_t)min(k0 + kt * 16 + lr, T - 1) * ldk;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[kt] = Mma<bf16>::mma(*(const bf16x8*)(krow + c * 32), qf[c], s[kt]);
    }
    const bool ragged = k0 + 32 > klen;  // (wave-uniform) the memory's last tile
    float sc[8];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + (j >> 2) * 16 + lg * 4 + (j & 3);
      sc[j] = key < klen ? s[j >> 2][j & 3] * scale : -INFINITY;
      tmax = fmaxf(tmax, sc[j]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);  // finite: frame k0 < klen is visible to every query
    const float alpha = __expf(m - m_new);  // m = -inf: 0
    m = m_new;
    bf16x8 pf;
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = sc[j] == -INFINITY ? 0.f : __expf(sc[j] - m_new);
      psum += p;
      pf[j] = (bf16)p;
    }
    l = l * alpha + psum;
#pragma unroll
    for (int t = 0; t < ND; ++t) {
      const bf16* vrow = vbase + (size_t)t * 16 * Tpad + k0;  // k0 + 31 < Tpad: Tpad is a multiple of 32 and >= T
      const bf16x4 lo = *(const bf16x4*)vrow, hi = *(const bf16x4*)(vrow + 16);
      bf16x8 vf;
#pragma unroll
      for (int j = 0; j < 4; ++j) vf[j] = lo[j], vf[4 + j] = hi[j];
      if (ragged) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k0 + (j >> 2) * 16 + lg * 4 + (j & 3) >= klen) vf[j] = (bf16)0.f;
      }
      acc[t] = Mma<bf16>::mma(vf, pf, acc[t] * alpha);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi >= Lp) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  bf16* out = ctx + (row0 + qi) * (size_t)d + h * DK + lg * 4;
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (bf16)(acc[t][r] * inv);
    *(bf16x4*)(out + t * 16) = o;
  }
}

// ---- the same attention in f32, plain (parity path): one wave per (query, head, sentence).  Pass 1 finds the row maximum,
// pass 2 recomputes the scores 64 frames at a time and lets lane c < dk accumulate channel c of the context from V^T.
__global__ __launch_bounds__(64) void dec_seq_src_attn_f32_kernel(const float* __restrict__ qs, const float* __restrict__ kmem,
                                                                  int ldk, const float* __restrict__ vT,
                                                                  const int32_t* __restrict__ klens,
                                                                  const int32_t* __restrict__ mem_of, int Bm, int Lp, int d,
                                                                  int dk, int T, int Tpad, float* __restrict__ ctx) {
  const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  int mi = mem_of ? mem_of[b] : b;
  mi = min(max(mi, 0), Bm - 1);
  const int klen = min(max(klens[mi], 0), T);
  const size_t row = (size_t)b * Lp + j;
  const float* q = qs + row * d + h * dk;
  const float* kb = kmem + (size_t)mi * T * ldk + h * dk;
  const float* vb = vT + ((size_t)mi * d + h * dk) * Tpad;
  const float scale = 1.0f / sqrtf((float)dk);
  float* out = ctx + row * d + h * dk;
  float m = -INFINITY;
  for (int k = lane; k < klen; k += 64) {
    const float* kr = kb + (size_t)k * ldk;
    float s = 0.f;
    for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
    m = fmaxf(m, s * scale);
  }
  m = wave_max(m);
  if (klen == 0) {  // (wave-uniform) no valid frame
    if (lane < dk) out[lane] = 0.f;
    return;
  }
  float lsum = 0.f, acc = 0.f;
  for (int k0 = 0; k0 < klen; k0 += 64) {
    const int k = k0 + lane;
    float p = 0.f;
    if (k < klen) {
      const float* kr = kb + (size_t)k * ldk;
      float s = 0.f;
      for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
      p = expf(s * scale - m);
    }
    lsum += p;
    const int n = min(64, klen - k0);
    for (int kk = 0; kk < n; ++kk) {
      const float pk = __shfl(p, kk, 64);
      if (lane < dk) acc += pk * vb[(size_t)lane * Tpad + k0 + kk];
    }
  }
  lsum = wave_sum(lsum);
  if (lane < dk) out[lane] = acc / lsum;
}

using em_host::dec_seq_shape_ok;
using em_host::DecSeqWs;

DecSeqWs nll_layout(int dtype, const EmDecoderWeights* dw, int M) {
  return em_host::dec_seq_layout(dtype, dw, (size_t)M, em_lm_head_nll_workspace_bytes(dtype, M, dw->vocab), false);
}

}  // namespace

extern "C" int em_dec_seq_embed_f32(const float* embed, const float* pe, const int32_t* tok, int32_t M, int32_t V, int32_t d,
                                    int32_t Lp, int32_t pe_len, float* x, void* stream) {
  if (!embed || !pe || !tok || !x || M <= 0 || V <= 0 || d <= 0 || Lp <= 0 || Lp > pe_len) return EM_ERR_BAD_ARG;
  hipLaunchKernelGGL(dec_seq_embed_kernel, dim3(M), dim3(128), 0, (hipStream_t)stream, embed, pe, tok, V, d, Lp,
                     sqrtf((float)d), x);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" int em_dec_seq_src_attention(int dtype, const void* qs, const void* kmem, int32_t ldk, const void* vT,
                                        const int32_t* klens, const int32_t* mem_of, int32_t B, int32_t Bm, int32_t Lp,
                                        int32_t d, int32_t heads, int32_t T, int32_t Tpad, void* ctx, void* stream) {
  if (!qs || !kmem || !vT || !klens || !ctx) return EM_ERR_BAD_ARG;
  if (B <= 0 || Bm <= 0 || Lp <= 0 || d <= 0 || heads <= 0 || d % heads || T <= 0 || Tpad < T || Tpad % 32 != 0 || ldk < d)
    return EM_ERR_BAD_ARG;
  if (!mem_of && Bm < B) return EM_ERR_BAD_ARG;
  const int dk = d / heads;
  if (dk != 32 && dk != 64) return EM_ERR_UNSUPPORTED;
  if (B > 65535 || heads > 65535) return EM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) {
    if (ldk % 8) return EM_ERR_UNSUPPORTED;  // 16-byte operand loads
    const dim3 grid(em_cdiv(Lp, 16), heads, B);
    if (dk == 64)
      hipLaunchKernelGGL(dec_seq_src_attn_bf16_kernel<64>, grid, dim3(64), 0, s, (const bf16*)qs, (const bf16*)kmem, ldk,
                         (const bf16*)vT, klens, mem_of, Bm, Lp, d, T, Tpad, (bf16*)ctx);
    else
      hipLaunchKernelGGL(dec_seq_src_attn_bf16_kernel<32>, grid, dim3(64), 0, s, (const bf16*)qs, (const bf16*)kmem, ldk,
                         (const bf16*)vT, klens, mem_of, Bm, Lp, d, T, Tpad, (bf16*)ctx);
  } else if (dtype == EM_F32) {
    hipLaunchKernelGGL(dec_seq_src_attn_f32_kernel, dim3(Lp, heads, B), dim3(64), 0, s, (const float*)qs, (const float*)kmem,
                       ldk, (const float*)vT, klens, mem_of, Bm, Lp, d, dk, T, Tpad, (float*)ctx);
  } else {
    return EM_ERR_BAD_ARG;
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

// (declared in csrc/enc_host.h)
int em_host::dec_seq_rows(int dtype, const EmDecoderWeights* dw, const void* mem_kv, const void* mem_vT, const int32_t* klens,
                          const int32_t* mem_of, int Bm, const int32_t* tok, bool causal, const int32_t* self_x, int B, int Lp,
                          int T, int Tpad, void* ws, const DecSeqWs& o, void* stream) {
  const int M = B * Lp, V = dw->vocab, d = dw->d, ff = dw->ff, h = dw->heads;
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  unsigned char* base = (unsigned char*)ws;
  void *xn = base + o.xn, *qkv = base + o.qkv, *ctx = base + o.ctx, *hb = base + o.h;
  void* qs = qkv;  // q | k | v are consumed before the source attention's queries are projected
  float* xf = (float*)(base + o.x);
  EM_TRY(em_dec_seq_embed_f32(dw->embed, dw->pe, tok, M, V, d, Lp, dw->pe_len, xf, stream));
  for (int l = 0; l < dw->num_blocks; ++l) {
    const EmDecoderLayer& q = dw->layers[l];
    const unsigned char* kv = (const unsigned char*)mem_kv + (size_t)l * Bm * T * 2 * d * es;
    const unsigned char* vT = (const unsigned char*)mem_vT + (size_t)l * Bm * d * Tpad * es;
    EM_TRY(em_layernorm(dtype, xf, q.norm1_g, q.norm1_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.self_wqkv, qkv, q.self_bqkv, M, 3 * d, d, d, 3 * d, 1.f, stream));
    EM_TRY((causal ? em_lm_causal_attention : em_dec_full_attention)(dtype, qkv, self_x, B, Lp, d, h, ctx, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.self_wout, xf, q.self_bout, M, d, d, d, d, 1.f, stream));
    EM_TRY(em_layernorm(dtype, xf, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.src_wq, qs, q.src_bq, M, d, d, d, d, 1.f, stream));
    EM_TRY(em_dec_seq_src_attention(dtype, qs, kv, 2 * d, vT, klens, mem_of, B, Bm, Lp, d, h, T, Tpad, ctx, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.src_wout, xf, q.src_bout, M, d, d, d, d, 1.f, stream));
    EM_TRY(em_layernorm(dtype, xf, q.norm3_g, q.norm3_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_RELU, xn, q.w1, hb, q.b1, M, ff, d, d, ff, 1.f, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, hb, q.w2, xf, q.b2, M, d, ff, ff, d, 1.f, stream));
  }
  return EM_OK;
}

extern "C" size_t em_dec_seq_nll_workspace_bytes(int dtype, const EmDecoderWeights* dw, int32_t B, int32_t Lp) {
  if (!dw || (dtype != EM_BF16 && dtype != EM_F32) || !dec_seq_shape_ok(dw, B, Lp)) return 0;
  return nll_layout(dtype, dw, B * Lp).total;
}

extern "C" int em_dec_seq_nll(int dtype, const EmDecoderWeights* dw, const void* mem_kv, const void* mem_vT,
                              const int32_t* klens, const int32_t* mem_of, const int32_t* x, const int32_t* keymask,
                              const int32_t* target, int32_t B, int32_t Bm, int32_t Lp, int32_t T, int32_t Tpad, float* nll,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!dw || !dw->layers || !mem_kv || !mem_vT || !klens || !x || !keymask || !target || !nll) return EM_ERR_BAD_ARG;
  if (dtype != EM_BF16 && dtype != EM_F32) return EM_ERR_BAD_ARG;
  if (B <= 0 || Bm <= 0 || Lp <= 0 || T <= 0 || Tpad < T || Tpad % 32 != 0 || (!mem_of && Bm < B)) return EM_ERR_BAD_ARG;
  if (dw->d <= 0 || dw->heads <= 0 || dw->d % dw->heads || Lp > dw->pe_len) return EM_ERR_BAD_ARG;
  if (!dec_seq_shape_ok(dw, B, Lp)) return EM_ERR_UNSUPPORTED;
  const int M = B * Lp;
  const DecSeqWs o = nll_layout(dtype, dw, M);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  unsigned char* base = (unsigned char*)ws;
  EM_TRY(em_host::dec_seq_rows(dtype, dw, mem_kv, mem_vT, klens, mem_of, Bm, x, true, keymask, B, Lp, T, Tpad, ws, o, stream));
  return em_lm_head_nll(dtype, (const float*)(base + o.x), dw->after_norm_g, dw->after_norm_b, dw->out_w, dw->out_b, target,
                        M, dw->vocab, dw->d, nll, base + o.head, o.total - o.head, stream);
}
