// espnet_amd — the TransformerLM over whole sentences on gfx950: per-token negative log-likelihoods of a batch in one
// enqueue (contract: include/espnet_amd.h, "language model over whole sentences").  Reference:
// espnet2/lm/espnet_model.py ESPnetLanguageModel.nll, espnet2/lm/transformer_lm.py TransformerLM.forward (Encoder with
// input_layer="linear", `_target_mask`: query j sees the keys k <= j whose token id is not 0).
//
// The search's step path (csrc/search.hip lm_step) feeds one position per call, ~6 launches per layer and position.  A
// sentence that is known beforehand needs none of that chain: everything but the attention is row-local, so the
// M = B * Lp rows go through the library's GEMMs at once and through the vocabulary head that never materialises the logits
// (em_lm_head_nll, csrc/vocab_head.hip).  What this file adds:
//   lm_seq_input_norm  the input layer's LayerNorm + ReLU + position on all rows;
//   lm_causal_attn_*   causal self-attention with the id-0 key mask, a wave per 16 queries of one (sentence, head); without
//                      the diagonal it is the MLM decoder's self-attention (em_dec_full_attention).
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

using em_host::Bump;
using em_host::gemm;
using em_host::LN_EPS;

// ---- input layer tail on all rows: torch LayerNorm(1e-5) -> ReLU -> optional x * sqrt(d) + pe[row % Lp], in place on
// x [M][d] f32 (csrc/decoder.hip lm_input_norm_kernel with the position taken from the row).  One wave per row.
__global__ __launch_bounds__(256) void lm_seq_input_norm_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                                const float* __restrict__ b, const float* __restrict__ pe,
                                                                int M, int d, int Lp) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int pos = row % Lp;
  float* xr = x + (size_t)row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float t = xr[c] - mean;
    q += t * t;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + 1e-5f);
  const float xs = sqrtf((float)d);
  for (int c = lane; c < d; c += 64) {
    float v = fmaxf((xr[c] - mean) * rstd * g[c] + b[c], 0.f);
    if (pe) v = v * xs + pe[(size_t)pos * d + c];
    xr[c] = v;
  }
}

// ---- causal self-attention, bf16 on the matrix cores.  One wave owns 16 queries q0 .. q0 + 15 of one (sentence, head) and
// walks the keys 0 .. q0 + 15 in tiles of 32, no further (the diagonal).  Both products are taken transposed so that a
// lane's query never changes:
//   S^T[key][query] = K . Q^T   A = K rows (straight from global memory), B = Q (registers): lane (lr, lg) ends up with the
//                               scores of query q0 + lr against the keys 16 kt + 4 lg + reg, kt = 0 | 1;
//   O^T[dv][query]  = V^T . P^T B = the lane's own eight probabilities (element 4 kt + reg of lane group lg is key
//                               16 kt + 4 lg + reg - the A operand uses the same numbering, so no value changes lanes),
//                               A = V^T read from the 32 x DK tile of V in LDS.
// The running maximum is shared by the four lane groups of a query (they all scale the same accumulators), the running sum is
// per lane and meets at the end.  A masked key (beyond the diagonal, id 0, or past Lp) takes p = 0.0 exactly; a query with no
// visible key writes zeros.  LDS: one V tile, 4.5 KiB at DK = 64, whatever Lp is.
// CAUSAL = false (em_dec_full_attention, the MLM decoder): no diagonal, x [B] holds the sentences' lengths and query (b, j)
// sees the keys below x[b]; the V rows of the keys behind it enter LDS as zeros (0.0 * whatever lies there would not be 0).
template <int DK, bool CAUSAL>
__global__ __launch_bounds__(64) void lm_causal_attn_bf16_kernel(const bf16* __restrict__ qkv, const int32_t* __restrict__ x,
                                                                 int Lp, int d, bf16* __restrict__ ctx) {
  constexpr int NC = DK / 32, ND = DK / 16, VLD = DK + 8;
  __shared__ __attribute__((aligned(16))) bf16 vs[32 * VLD];
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const size_t row0 = (size_t)b * Lp;
  const size_t ld = (size_t)3 * d;
  const int qi = q0 + lr;
  const bf16* qrow = qkv + (row0 + min(qi, Lp - 1)) * ld + h * DK + lg * 8;
  bf16x8 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) qf[c] = *(const bf16x8*)(qrow + c * 32);
  const float scale = 1.0f / sqrtf((float)DK);
  float m = -INFINITY, l = 0.f;
  f32x4 acc[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int kend = CAUSAL ? min(q0 + 16, Lp) : min(max(x[b], 0), Lp);
  for (int k0 = 0; k0 < kend; k0 += 32) {
    __syncthreads();  // the previous tile's V is read
    for (int i = lane; i < 32 * (DK / 8); i += 64) {
      const int kr = i / (DK / 8), cc = i % (DK / 8);
      const bf16* src = qkv + (row0 + min(k0 + kr, Lp - 1)) * ld + 2 * d + h * DK + cc * 8;
      bf16x8 v = *(const bf16x8*)src;
      if (!CAUSAL && k0 + kr >= kend) v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      *(bf16x8*)(vs + kr * VLD + cc * 8) = v;
    }
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const bf16* krow = qkv + (row0 + min(k0 + kt * 16 + lr, Lp - 1)) * ld + d + h * DK + lg * 8;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[kt] = Mma<bf16>::mma(*(const bf16x8*)(krow + c * 32), qf[c], s[kt]);
    }
    float sc[8];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + (j >> 2) * 16 + lg * 4 + (j & 3);
      const bool ok = CAUSAL ? key <= qi && key < Lp && x[row0 + min(key, Lp - 1)] != 0 : key < kend;
      sc[j] = ok ? s[j >> 2][j & 3] * scale : -INFINITY;
      tmax = fmaxf(tmax, sc[j]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __expf(m - m_use);  // m = -inf: 0
    m = m_new;
    bf16x8 pf;
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = sc[j] == -INFINITY ? 0.f : __expf(sc[j] - m_use);
      psum += p;
      pf[j] = (bf16)p;
    }
    l = l * alpha + psum;
    __syncthreads();  // the V tile is in LDS
#pragma unroll
    for (int t = 0; t < ND; ++t) {
      bf16x8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = vs[((j >> 2) * 16 + lg * 4 + (j & 3)) * VLD + t * 16 + lr];
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
// pass 2 recomputes the scores 64 keys at a time and lets lane c < dk accumulate channel c of the context.  CAUSAL = false:
// the keys below the sentence's length x[b], whatever the query.
template <bool CAUSAL>
__global__ __launch_bounds__(64) void lm_causal_attn_f32_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ x,
                                                                int Lp, int d, int dk, float* __restrict__ ctx) {
  const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const size_t row0 = (size_t)b * Lp;
  const size_t ld = (size_t)3 * d;
  const float* q = qkv + (row0 + j) * ld + h * dk;
  const float scale = 1.0f / sqrtf((float)dk);
  float* out = ctx + (row0 + j) * (size_t)d + h * dk;
  const int nkey = CAUSAL ? j + 1 : min(max(x[b], 0), Lp);  // the keys 0 .. nkey - 1 can be seen
  float m = -INFINITY;
  for (int k = lane; k < nkey; k += 64) {
    if (CAUSAL && x[row0 + k] == 0) continue;
    const float* kr = qkv + (row0 + k) * ld + d + h * dk;
    float s = 0.f;
    for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
    m = fmaxf(m, s * scale);
  }
  m = wave_max(m);
  if (m == -INFINITY) {  // no visible key
    if (lane < dk) out[lane] = 0.f;
    return;
  }
  float lsum = 0.f, acc = 0.f;
  for (int k0 = 0; k0 < nkey; k0 += 64) {
    const int k = k0 + lane;
    float p = 0.f;
    if (k < nkey && (!CAUSAL || x[row0 + k] != 0)) {
      const float* kr = qkv + (row0 + k) * ld + d + h * dk;
      float s = 0.f;
      for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
      p = expf(s * scale - m);
    }
    lsum += p;
    const int n = min(64, nkey - k0);
    for (int kk = 0; kk < n; ++kk) {
      const float pk = __shfl(p, kk, 64);
      if (lane < dk) acc += pk * qkv[(row0 + k0 + kk) * ld + 2 * d + h * dk + lane];
    }
  }
  lsum = wave_sum(lsum);
  if (lane < dk) out[lane] = acc / lsum;
}

struct SeqWs {
  size_t e, x, xn, qkv, ctx, h, head, total;
};
SeqWs seq_layout(int dtype, const EmLmWeights* lm, size_t M) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  Bump b;
  SeqWs s;
  s.e = b.take(M * lm->embed_unit * es);
  s.x = b.take(M * lm->d * 4);
  s.xn = b.take(M * lm->d * es);
  s.qkv = b.take(M * 3 * lm->d * es);
  s.ctx = b.take(M * lm->d * es);
  s.h = b.take(M * lm->ff * es);
  s.head = b.take(em_lm_head_nll_workspace_bytes(dtype, (int32_t)M, lm->vocab));
  s.total = b.o;
  return s;
}

// M rows and the widest activation row stay inside 31-bit element offsets (the GEMMs' buffer resources)
bool seq_shape_ok(const EmLmWeights* lm, int B, int Lp) {
  if (B <= 0 || Lp <= 0 || B > 65535) return false;
  const size_t wide = (size_t)(lm->ff > 3 * lm->d ? lm->ff : 3 * lm->d);
  return (size_t)B * Lp * wide * 4 < ((size_t)1 << 31);
}

// the launch of both attentions: x is the token array of the causal form, the lengths of the full one
template <bool CAUSAL>
int seq_attention(int dtype, const void* qkv, const int32_t* x, int32_t B, int32_t Lp, int32_t d, int32_t heads, void* ctx,
                  void* stream) {
  if (!qkv || !x || !ctx || B <= 0 || Lp <= 0 || d <= 0 || heads <= 0 || d % heads) return EM_ERR_BAD_ARG;
  const int dk = d / heads;
  if (dk != 32 && dk != 64) return EM_ERR_UNSUPPORTED;
  if (B > 65535 || heads > 65535) return EM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) {
    const dim3 grid(em_cdiv(Lp, 16), heads, B);
    if (dk == 64)
      hipLaunchKernelGGL((lm_causal_attn_bf16_kernel<64, CAUSAL>), grid, dim3(64), 0, s, (const bf16*)qkv, x, Lp, d,
                         (bf16*)ctx);
    else
      hipLaunchKernelGGL((lm_causal_attn_bf16_kernel<32, CAUSAL>), grid, dim3(64), 0, s, (const bf16*)qkv, x, Lp, d,
                         (bf16*)ctx);
  } else if (dtype == EM_F32) {
    hipLaunchKernelGGL(lm_causal_attn_f32_kernel<CAUSAL>, dim3(Lp, heads, B), dim3(64), 0, s, (const float*)qkv, x, Lp, d, dk,
                       (float*)ctx);
  } else {
    return EM_ERR_BAD_ARG;
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" int em_lm_causal_attention(int dtype, const void* qkv, const int32_t* x, int32_t B, int32_t Lp, int32_t d,
                                      int32_t heads, void* ctx, void* stream) {
  return seq_attention<true>(dtype, qkv, x, B, Lp, d, heads, ctx, stream);
}

// (contract: include/espnet_amd.h, "Mask-CTC")
extern "C" int em_dec_full_attention(int dtype, const void* qkv, const int32_t* lens, int32_t B, int32_t Lp, int32_t d,
                                     int32_t heads, void* ctx, void* stream) {
  return seq_attention<false>(dtype, qkv, lens, B, Lp, d, heads, ctx, stream);
}

extern "C" size_t em_lm_seq_nll_workspace_bytes(int dtype, const EmLmWeights* lm, int32_t B, int32_t Lp) {
  if (!lm || lm->kind != EM_LM_TRANSFORMER || !seq_shape_ok(lm, B, Lp)) return 0;
  return seq_layout(dtype, lm, (size_t)B * Lp).total;
}

extern "C" int em_lm_seq_nll(int dtype, const EmLmWeights* lm, const int32_t* x, const int32_t* target, int32_t B, int32_t Lp,
                             float* nll, void* ws, size_t ws_bytes, void* stream) {
  if (!lm || !x || !target || !nll || B <= 0 || Lp <= 0) return EM_ERR_BAD_ARG;
  if (dtype != EM_BF16 && dtype != EM_F32) return EM_ERR_BAD_ARG;
  if (lm->kind != EM_LM_TRANSFORMER || !lm->layers) return EM_ERR_BAD_ARG;
  if (!seq_shape_ok(lm, B, Lp)) return EM_ERR_UNSUPPORTED;
  const int M = B * Lp, V = lm->vocab, d = lm->d, ff = lm->ff, eu = lm->embed_unit;
  const SeqWs o = seq_layout(dtype, lm, (size_t)M);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  unsigned char* base = (unsigned char*)ws;
  void *e = base + o.e, *xn = base + o.xn, *qkv = base + o.qkv, *ctx = base + o.ctx, *hb = base + o.h;
  float* xf = (float*)(base + o.x);
  EM_TRY(em_lm_embed(dtype, lm->embed, x, M, V, eu, nullptr, 0, e, stream));
  EM_TRY(gemm(dtype, EM_EPI_SCALE_F32, e, lm->in_w, xf, lm->in_b, M, d, eu, eu, d, 1.f, stream));
  hipLaunchKernelGGL(lm_seq_input_norm_kernel, dim3(em_cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, xf, lm->in_ln_g,
                     lm->in_ln_b, lm->pe, M, d, Lp);
  EM_CHECK_LAUNCH();
  for (int l = 0; l < lm->num_blocks; ++l) {
    const EmLmLayer& q = lm->layers[l];
    EM_TRY(em_layernorm(dtype, xf, q.norm1_g, q.norm1_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.wqkv, qkv, q.bqkv, M, 3 * d, d, d, 3 * d, 1.f, stream));
    EM_TRY(em_lm_causal_attention(dtype, qkv, x, B, Lp, d, lm->heads, ctx, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.wout, xf, q.bout, M, d, d, d, d, 1.f, stream));
    EM_TRY(em_layernorm(dtype, xf, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_RELU, xn, q.w1, hb, q.b1, M, ff, d, d, ff, 1.f, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, hb, q.w2, xf, q.b2, M, d, ff, ff, d, 1.f, stream));
  }
  return em_lm_head_nll(dtype, xf, lm->after_norm_g, lm->after_norm_b, lm->out_w, lm->out_b, target, M, V, d, nll,
                        base + o.head, o.total - o.head, stream);
}
