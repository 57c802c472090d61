// Streaming (contextual block) TRANSFORMER encoder step: the layer stack of ContextualBlockTransformerEncoder.forward_infer
// (espnet2/asr/encoder/contextual_block_transformer_encoder.py) on the blocks csrc/streaming.hip assembles.
//
// Reference layer: ContextualBlockEncoderLayer.forward_infer
// (espnet2/legacy/nets/pytorch_backend/transformer/contextual_block_encoder_layer.py), normalize_before, no concat_after,
// per block x [L][d]:
//     x = x + self_attn(norm1(x), mask)          MultiHeadedAttention (transformer/attention.py), contextual mask
//     x = x + w_2(relu(w_1(norm2(x))))           PositionwiseFeedForward (transformer/positionwise_feed_forward.py)
// then the context hand-over of the Conformer variant (slot 0 := the previous block's last slot, or the previous call's
// context vector of this layer; next_ctx[l] := the last slot of the last block).  Residual scale 1, no macaron module, no
// convolution module, no norm_final.  Block assembly, the per-operator attention (em_block_mha) and the hand-over kernel
// are csrc/streaming.hip's, reached through the C ABI; this file holds the two launch sequences and no kernel of its own:
// the fused layer's device code is csrc/block.hip (EM_BLOCK_Q / EM_BLOCK_T).
#include <math.h>
#include <stdlib.h>

#include "em_common.h"
#include "switches.h"
#include "enc_host.h"

using em_host::align_up;
using em_host::gemm;
using em_host::LN_EPS;

namespace {

struct Ws {
  size_t xn, big, ctx, qkv[2], part, ticket, total;  // qkv[i]: q | k | V^T per head, set i (fused path; two sets: see merge)
  size_t per_head;
  int Tpad;
};
inline Ws layout(int dtype, const EmTransformerWeights* w, int M) {
  Ws s = {};
  em_host::Bump b;
  const em_host::StreamWsHead h = em_host::stream_ws_head(b, dtype, w->d, w->ff, M);
  s.xn = h.xn;
  s.big = h.big;
  s.ctx = b.take(h.row);
  s.total = b.o;
  return s;
}
// The fused path keeps nothing of the per-operator scratch: per-head operands (bf16, two sets) + the split FFN's meeting place
// (em_host::stream_ffn_split: the rule measured for the Conformer layer's FFNs - the same FFN, the same launch shape)
inline Ws layout_fused(const EmTransformerWeights* w, int n_blk, int L) {
  Ws s = {};
  s.Tpad = (L + 63) / 64 * 64;
  s.per_head = align_up((size_t)n_blk * w->d * s.Tpad * 2);
  em_host::Bump b;
  for (int i = 0; i < 2; ++i) s.qkv[i] = b.take(3 * s.per_head);
  em_host::stream_ffn_slots(b, w->ff, n_blk * ((L + 31) / 32), &s.part, &s.ticket);
  s.total = b.o;
  return s;
}
// Which calls take the row-block launches: the gate of the Conformer variant (cb_fusable) - bf16, 256 wide, 4 heads,
// ff <= 4096 in whole chunk pairs, blocks of at most 64 slots, every layer packed for it by the host.
inline bool fusable(int dtype, const EmTransformerWeights* w, int L, int n_blk) {
  if (em_sw().stream_no_fused || n_blk < em_sw().stream_fused_min || dtype != EM_BF16 || w->d != 256 || w->heads != 4 ||
      w->ff > 4096 || w->ff % 128 != 0 || L > 64 || !w->layers)
    return false;
  for (int l = 0; l < w->num_blocks; ++l) {
    const EmTransformerLayer& q = w->layers[l];
    if (!q.cb_wqkvp || !q.cb_woutp || !q.cb_ff_w1p || !q.cb_ff_w2p || !q.fp_t || !q.ff_b1) return false;
  }
  return true;
}
// With the hand-over folded into the launches (em_host::stream_fold_ctx), layer l's block<ATT|T> may take layer l + 1's block<Q> into its launch (num_blocks + 1 launches per call).
// ESPNET_AMD_STREAM_TF_MERGE: developer A/B switch (1 on, 0 off); DESIGN.md 4k has what each form measured.
inline bool merge_default() { return true; }
inline bool merged(bool fold) {
  const int sw = em_sw().stream_tf_merge;
  return fold && (sw < 0 ? merge_default() : sw != 0);
}

int encode_impl(int dtype, const EmTransformerWeights* w, float* x, int32_t n_streams, int32_t n_blk_s, int32_t L,
                int32_t mask_mode, const float* past_ctx, float* next_ctx, void* workspace, size_t workspace_bytes,
                void* stream) {
  if (!w || !x || !workspace || n_streams <= 0 || n_blk_s <= 0 || L <= 0) return EM_ERR_BAD_ARG;
  if (dtype != EM_F32 && dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (w->num_blocks > 0 && !w->layers) return EM_ERR_BAD_ARG;
  if (mask_mode && L < 2) return EM_ERR_BAD_ARG;
  const int n_blk = n_streams * n_blk_s;
  const int d = w->d, h = w->heads, ff = w->ff, NL = w->num_blocks, M = n_blk * L;
  if (d % 64 != 0 || ff % 64 != 0 || h <= 0 || d % h != 0 || (d / h != 64 && d / h != 32) || L > 64) return EM_ERR_UNSUPPORTED;
  unsigned char* ws = (unsigned char*)workspace;
  auto propagate = [&](int l) { return em_host::stream_hand_over(x, past_ctx, next_ctx, l, n_streams, n_blk_s, L, d, NL, stream); };
  if (fusable(dtype, w, L, n_blk)) {
    const Ws s = layout_fused(w, n_blk, L);
    if (workspace_bytes < s.total) return EM_ERR_WORKSPACE;
    const bool fold = em_host::stream_fold_ctx(mask_mode, n_blk_s, past_ctx, next_ctx), merge = merged(fold);
    EmBlockArgs ba = {};
    ba.B = n_blk; ba.T = L; ba.Tpad = s.Tpad; ba.d = d; ba.ff = ff; ba.kernel = 0; ba.eps = LN_EPS;
    ba.x = x; ba.att_mask = mask_mode; ba.row_stride = NL * d;
    EM_TRY(em_host::stream_ffn_setup(ba, n_blk * ((L + 31) / 32), ws + s.part, ws + s.ticket, stream));
    auto set_qkv = [&](int set, bool out) {
      unsigned char* p = ws + s.qkv[set];
      if (out) { ba.qh_out = p; ba.kh_out = p + s.per_head; ba.vt_out = p + 2 * s.per_head; }
      else { ba.qh = p; ba.kh = p + s.per_head; ba.vt = p + 2 * s.per_head; }
    };
    for (int l = 0; l < NL; ++l) {
      const EmTransformerLayer& q = w->layers[l];
      const int set = merge ? (l & 1) : 0;
      set_qkv(set, false);
      if (l == 0 || !merge) {
        // block<Q>: norm1 + q / k / v per head; folded hand-over: slot 0 := the previous call's context vector of layer l - 1
        ba.wqkv = q.cb_wqkvp; ba.params = q.fp_t;
        ba.row0_src = (fold && l > 0) ? past_ctx + (size_t)(l - 1) * d : nullptr;
        ba.last_dst = nullptr;
        EM_TRY(em_conformer_block_fused(EM_BLOCK_Q | EM_BLOCK_RELU, &ba, stream));
      }
      // block<ATT|T>: attention + linear_out + residual + norm2 + FFN + residual; folded: last slot -> next_ctx[l]
      ba.wout = q.cb_woutp; ba.ff_w1 = q.cb_ff_w1p; ba.ff_w2 = q.cb_ff_w2p; ba.ff_b1g = q.ff_b1;
      ba.params = q.fp_t + EM_BLOCK_PARAM_GROUP;
      ba.last_dst = fold ? next_ctx + (size_t)l * d : nullptr;
      ba.row0_src = nullptr;
      if (merge && l + 1 < NL) {  // ... + the hand-over + layer l + 1's block<Q>, into the other set of per-head operands
        ba.wqkv = w->layers[l + 1].cb_wqkvp;
        ba.row0_src = past_ctx + (size_t)l * d;
        set_qkv(set ^ 1, true);
        EM_TRY(em_conformer_block_fused(EM_BLOCK_ATT | EM_BLOCK_T | EM_BLOCK_Q | EM_BLOCK_RELU, &ba, stream));
      } else {
        EM_TRY(em_conformer_block_fused(EM_BLOCK_ATT | EM_BLOCK_T | EM_BLOCK_RELU, &ba, stream));
      }
      if (mask_mode && !fold) EM_TRY(propagate(l));
    }
    return EM_OK;
  }
  // ---- per-operator sequence (f32 parity mode and every shape the row-block launches do not take): six launches per layer
  const Ws s = layout(dtype, w, M);
  if (workspace_bytes < s.total) return EM_ERR_WORKSPACE;
  void *xn = ws + s.xn, *big = ws + s.big, *ctx = ws + s.ctx;
  const em_host::StreamLnProj ln_proj{dtype, M, d, x, xn, stream};
  for (int l = 0; l < NL; ++l) {
    const EmTransformerLayer& q = w->layers[l];
    EM_TRY(ln_proj(EM_EPI_STORE, q.norm1_g, q.norm1_b, q.wqkv, q.bqkv, big, 3 * d));
    EM_TRY(em_block_mha(dtype, big, n_blk, L, d, h, mask_mode, ctx, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.wout, x, q.bout, M, d, d, d, d, 1.f, stream));
    EM_TRY(ln_proj(EM_EPI_RELU, q.norm2_g, q.norm2_b, q.ff_w1, q.ff_b1, big, ff));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, big, q.ff_w2, x, q.ff_b2, M, d, ff, ff, d, 1.f, stream));
    if (mask_mode) EM_TRY(propagate(l));
  }
  return EM_OK;
}

}  // namespace

extern "C" size_t em_cbt_workspace_bytes(int dtype, const EmTransformerWeights* w, int32_t n_blk, int32_t L) {
  if (!w || n_blk <= 0 || L <= 0) return 0;
  const size_t t = fusable(dtype, w, L, n_blk) ? layout_fused(w, n_blk, L).total : layout(dtype, w, n_blk * L).total;
  return t ? t : 256;
}

extern "C" int em_cbt_encode_plan(int dtype, const EmTransformerWeights* w, int32_t n_streams, int32_t n_blk, int32_t L,
                                  int32_t mask_mode, int32_t has_ctx) {
  if (!w || n_streams <= 0 || n_blk <= 0 || L <= 0) return EM_ERR_BAD_ARG;
  if (!fusable(dtype, w, L, n_streams * n_blk)) return 0;
  const bool fold = mask_mode && n_blk == 1 && has_ctx && !em_sw().stream_no_ctx_fold;
  return !fold ? 1 : merged(fold) ? 3 : 2;
}

extern "C" int em_cbt_encode_blocks(int dtype, const EmTransformerWeights* w, float* x, int32_t n_blk, int32_t L,
                                    int32_t mask_mode, const float* past_ctx, float* next_ctx, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return encode_impl(dtype, w, x, 1, n_blk, L, mask_mode, past_ctx, next_ctx, workspace, workspace_bytes, stream);
}

extern "C" int em_cbt_encode_blocks_batch(int dtype, const EmTransformerWeights* w, float* x, int32_t n_streams, int32_t n_blk,
                                          int32_t L, int32_t mask_mode, const float* past_ctx, float* next_ctx,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return encode_impl(dtype, w, x, n_streams, n_blk, L, mask_mode, past_ctx, next_ctx, workspace, workspace_bytes, stream);
}
