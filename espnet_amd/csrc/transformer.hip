// Host-side launch sequence of the Transformer encoder: one C call enqueues every kernel of a forward pass on the
// caller's stream.  The only device code here is the positional-encoding add.
//
// Reference call graph being reproduced (eval mode, normalize_before=True, concat_after=False):
//   TransformerEncoder.forward   espnet2/asr/encoder/transformer_encoder.py
//   Conv2dSubsampling{,6,8} with PositionalEncoding as pos_enc: x = out(conv(feats)) * sqrt(d) + pe[:T]
//   EncoderLayer.forward         x = x + self_attn(norm1(x)) ; x = x + feed_forward(norm2(x))
//   MultiHeadedAttention         linear_q / k / v, softmax(q k^T / sqrt(d_k)) over unpadded keys, linear_out
//   PositionwiseFeedForward      w_2(relu(w_1(x)))
//   after_norm                   LayerNorm, eps 1e-12
//
// Per layer: LayerNorm -> q | k | V^T projections (bf16: per head, csrc/abs_attn.hip) -> attention -> linear_out + residual ->
// FFN + residual (d = 512, bf16: one row-block launch of csrc/ffn_rows.hip that also computes the next LayerNorm;
// otherwise LayerNorm, a GEMM with ReLU and the second GEMM with the residual) -> the next layer's norm1 / after_norm.
#include <math.h>
#include <stdlib.h>

#include "em_common.h"
#include "switches.h"
#include "subsample.h"
#include "enc_host.h"

using em_host::gemm;
using em_host::LN_EPS;

namespace {

struct Ws {
  size_t c1, c2, c3, x, xn, big, ctx, qh, kh, vt, total;
  int Tpad;
};
inline Ws layout(int dtype, const EmTransformerWeights* w, int B, int T_f) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  em_sub::Geo g;
  em_sub::geo(w->subsample, T_f, w->n_mels, &g);
  const size_t M = (size_t)B * g.T_out, d = w->d;
  size_t mb[3];
  em_sub::map_bytes(g, B, w->d, es, mb);
  const size_t wide = (size_t)w->ff > 3 * d ? (size_t)w->ff : 3 * d;
  Ws s;
  em_host::Bump b;
  s.c1 = b.take(mb[0]);
  s.c2 = b.take(mb[1]);
  s.c3 = b.take(mb[2]);
  s.x = b.take(M * d * 4);
  s.xn = b.take(M * d * es);
  s.big = b.take(M * wide * es);
  s.ctx = b.take(M * d * es);
  // per-head operands of the bf16 attention (q, k [B][H][Tpad][64], V^T [B][H][64][Tpad])
  s.Tpad = em_host::tpad256(g.T_out);
  const size_t per_head = dtype == EM_BF16 ? em_host::head_slab_bytes(B, w->d, s.Tpad, es) : 0;
  s.qh = b.take(per_head);
  s.kh = b.take(per_head);
  s.vt = b.take(per_head);
  s.total = b.o;
  return s;
}

// x[b*T + t][c] += pe[t][c]  (PositionalEncoding.forward after the * sqrt(d) of the embed GEMM's epilogue)
__global__ __launch_bounds__(256) void abs_pe_add_kernel(float* __restrict__ x, const float* __restrict__ pe, int T, int d4,
                                                         long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long row = i / d4;
  const int c = (int)(i - row * d4), t = (int)(row % T);
  float4 v = ((float4*)x)[i];
  const float4 p = ((const float4*)pe)[(long)t * d4 + c];
  v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
  ((float4*)x)[i] = v;
}

}  // namespace

extern "C" size_t em_transformer_workspace_bytes(int dtype, const EmTransformerWeights* w, int32_t B, int32_t T_f) {
  if (!w || B <= 0 || T_f < em_sub::min_frames(w->subsample)) return 0;
  return layout(dtype, w, B, T_f).total;
}

extern "C" int em_transformer_encode(int dtype, const EmTransformerWeights* w, const float* feats, const float* mvn_partial,
                                     const int32_t* flens, const int32_t* olens, int32_t B, int32_t T_f, const void* pos_emb,
                                     void* workspace, size_t workspace_bytes, float* enc_out, void* enc_act, int32_t flags,
                                     void* stream) {
  if (!w || (w->num_blocks > 0 && !w->layers) || !feats || !flens || !olens || !pos_emb || !workspace || !enc_out || !enc_act)
    return EM_ERR_BAD_ARG;
  if (dtype != EM_F32 && dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (B <= 0 || w->num_blocks < 0) return EM_ERR_BAD_ARG;
  if (T_f < em_sub::min_frames(w->subsample)) return EM_ERR_TOO_SHORT;
  const int d = w->d, h = w->heads, ff = w->ff, L = w->num_blocks;
  if (d % 64 != 0 || h <= 0 || d / h != 64 || d != 64 * h || ff % 64 != 0 || ff <= 0) return EM_ERR_UNSUPPORTED;
  const Ws s = layout(dtype, w, B, T_f);
  if (workspace_bytes < s.total) return EM_ERR_WORKSPACE;
  em_sub::Geo g;
  if (!em_sub::geo(w->subsample, T_f, w->n_mels, &g)) return EM_ERR_UNSUPPORTED;
  const int T = g.T_out, M = B * T;
  unsigned char* ws = (unsigned char*)workspace;
  float* x = (float*)(ws + s.x);
  void* xn = ws + s.xn;
  void* big = ws + s.big;
  void* ctx = ws + s.ctx;
  void* qh = ws + s.qh;
  void* kh = ws + s.kh;
  void* vt = ws + s.vt;
  hipStream_t hs = (hipStream_t)stream;

  // ---- Conv2dSubsampling{,6,8} (+ MVN) -> Linear, * sqrt(d) (subsample.h), + pe[:T]
  EM_TRY(em_sub::run(dtype, w, g, feats, mvn_partial, flens, B, ws + s.c1, ws + s.c2, ws + s.c3, x, stream, w->conv1_wf,
                     w->conv2_wf));
  {
    const long n4 = (long)M * d / 4;
    hipLaunchKernelGGL(abs_pe_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, hs, x, (const float*)pos_emb, T,
                       d / 4, n4);
    EM_CHECK_LAUNCH();
  }
  const EmTransformerLayer* ly = w->layers;
  if (L == 0)
    return em_layernorm(dtype, x, w->after_norm_g, w->after_norm_b, M, d, LN_EPS, enc_act, enc_out, stream);

  // bf16: q / k / V^T written per head by the projection GEMMs for the MFMA attention (as the Conformer's attention2 path;
  // ESPNET_AMD_NO_ATTN2_LARGE=1 - developer switch - and operands past 32-bit offsets keep the row-layout kernel).
  // EM_ENC_NO_FUSED does not switch this path off, unlike the Conformer's and the E-Branchformer's.
  const bool heads_path = em_host::head_operands_ok(dtype, d, h, B, s.Tpad);
  // 512-wide bf16 model: FFN + residual + the next LayerNorm as one row-block launch (csrc/ffn_rows.hip, ReLU) when a round of
  // 64-row workgroups fills its share of the chip - the rule and the developer switches of the Conformer / E-Branchformer
  // (ESPNET_AMD_NO_FFN_ROWS, ESPNET_AMD_FFN_ROWS_MIN_FILL; EM_ENC_IN_FLIGHT)
  bool ffn_rows = em_host::rows_ffn_ok(dtype, d, ff, flags, M);
  for (int l = 0; ffn_rows && l < L; ++l) ffn_rows = ly[l].ff_w1p && ly[l].ff_w2p;

  EM_TRY(em_layernorm(dtype, x, ly[0].norm1_g, ly[0].norm1_b, M, d, LN_EPS, xn, nullptr, stream));
  for (int l = 0; l < L; ++l) {
    const EmTransformerLayer& q = ly[l];
    const bool last = l + 1 == L;
    // ---- x += linear_out(MHA(norm1(x)))  (xn holds norm1(x))
    if (heads_path) {
      EM_TRY(em_host::project_heads(dtype, xn, q.wqkv, q.bqkv, qh, vt, M, d, h, T, s.Tpad, stream));
      EM_TRY(em_abs_attention_bf16(qh, kh, vt, olens, B, T, s.Tpad, h, ctx, stream));
    } else {
      EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.wqkv, big, q.bqkv, M, 3 * d, d, d, 3 * d, 1.f, stream));
      EM_TRY(em_abs_attention(dtype, big, olens, B, T, h, 64, ctx, stream));
    }
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.wout, x, q.bout, M, d, d, d, d, 1.f, stream));
    // ---- x += w_2(relu(w_1(norm2(x))))
    const float* ng = last ? w->after_norm_g : ly[l + 1].norm1_g;
    const float* nb = last ? w->after_norm_b : ly[l + 1].norm1_b;
    if (ffn_rows) {
      EM_TRY(em_layernorm(dtype, x, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
      EmFfnRowsArgs fa = {};
      fa.xn_in = xn; fa.x = x; fa.w1p = q.ff_w1p; fa.w2p = q.ff_w2p; fa.b1 = q.ff_b1; fa.b2 = q.ff_b2;
      fa.g1 = ng; fa.be1 = nb; fa.xn_out = xn;  // (xn_out may alias xn_in)
      fa.M = M; fa.d = d; fa.ff = ff; fa.ln_mode = 1; fa.scale = 1.f; fa.eps = LN_EPS;
      fa.main = EM_ROWS_FFN; fa.act = EM_ROWS_ACT_RELU;
      EM_TRY(em_ffn_rows_fused(&fa, stream));
      // (after the last layer the launch's LayerNorm is after_norm, written again with its f32 copy by one LayerNorm more)
      if (last) EM_TRY(em_layernorm(dtype, x, ng, nb, M, d, LN_EPS, enc_act, enc_out, stream));
      continue;
    }
    // (LayerNorm launch + tiled GEMM, not em_ln_gemm: that kernel is shaped for the decoder's few rows - 32 x 64 tiles, W
    // straight from global memory, every column strip re-normalising its rows - and at 32 x 10 s (M = 7 968, N = 2 048,
    // K = 256) measured 58 us per call against 5.4 + ~12.6 us here; profiles/transformer_enc256_b32_kernel_stats.md)
    EM_TRY(em_layernorm(dtype, x, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_RELU, xn, q.ff_w1, big, q.ff_b1, M, ff, d, d, ff, 1.f, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, big, q.ff_w2, x, q.ff_b2, M, d, ff, ff, d, 1.f, stream));
    if (last)
      EM_TRY(em_layernorm(dtype, x, ng, nb, M, d, LN_EPS, enc_act, enc_out, stream));
    else
      EM_TRY(em_layernorm(dtype, x, ng, nb, M, d, LN_EPS, xn, nullptr, stream));
  }
  return EM_OK;
}
