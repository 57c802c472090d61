// Host layer shared by the launch sequences (no device code): what encoder.hip, transformer.hip and ebranchformer.hip
// each used to define for themselves, and the pieces of it the streaming encoders, the search and the transducer use.
//   - EM_TRY, LN_EPS, align_up, gemm(): the conveniences of every launch sequence;
//   - Bump: workspace layouts as one call per slot;
//   - tpad256 / head_slab_bytes / project_heads / clear_head_slabs: the per-head operand format of the LDS-resident
//     attention kernels (csrc/attention2.hip, csrc/abs_attn.hip): q, k [B][H][Tpad][64], V^T [B][H][64][Tpad], bf16;
//   - dec_seq_shape_ok / DecSeqWs / dec_seq_rows: the attention decoder over whole sentences, for the transcript scorer
//     (dec_seq.hip) and the Mask-CTC refinement (maskctc.hip);
//   - rows_ffn_ok / head_operands_ok: the two rules that pick the 512-wide models' launch forms;
//   - stream_*: what the two streaming launch sequences (streaming.hip, streaming_tf.hip) share - the FFN share rule and
//     its set-up, the folded / launched context hand-over, the head of the per-operator scratch, LayerNorm + projection.
#pragma once
#include <stddef.h>

#include "em_common.h"
#include "switches.h"

#define EM_TRY(expr)                \
  do {                              \
    const int rc__ = (expr);        \
    if (rc__ != EM_OK) return rc__; \
  } while (0)

namespace em_host {

constexpr float LN_EPS = 1e-12f;  // transformer/layer_norm.py:23

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Workspace layout: every slot starts on a 256-byte boundary.  `s.x = b.take(bytes)` per slot, `b.o` is the total.
struct Bump {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += align_up(bytes);
    return at;
  }
};

// C = epi(A W^T + bias) * scale on plain row-major operands
inline int gemm(int dtype, int epi, const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda,
                int ldc, float scale, void* stream) {
  EmGemmArgs a = {};
  a.A = A; a.W = W; a.C = C; a.bias = bias;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.scale = scale;
  return em_gemm(dtype, epi, EM_A_PLAIN, &a, stream);
}

// ---- the attention decoder over whole sentences (csrc/dec_seq.hip, csrc/maskctc.hip): M = B * Lp rows and the widest
// activation row stay inside 31-bit element offsets (the GEMMs' buffer resources); B and the heads are grid dimensions
inline bool dec_seq_shape_ok(const EmDecoderWeights* dw, int B, int Lp) {
  if (B <= 0 || Lp <= 0 || B > 65535 || dw->heads <= 0 || dw->heads > 65535 || dw->d <= 0 || dw->d % dw->heads) return false;
  const int dk = dw->d / dw->heads;
  if ((dk != 32 && dk != 64) || dw->d > 1024) return false;  // (1024: the vocabulary head's rows in LDS)
  const size_t wide = (size_t)(dw->ff > 3 * dw->d ? dw->ff : 3 * dw->d);
  return (size_t)B * Lp * wide * 4 < ((size_t)1 << 31);
}
// ... its workspace: the f32 residual rows x, then xn, qkv (q | k | v of the self-attention, then the source attention's
// queries), ctx, h in the activation type, head_bytes for the caller's vocabulary head and, for the Mask-CTC refinement,
// the head's two outputs s and a [M]
struct DecSeqWs { size_t x, xn, qkv, ctx, h, head, s, a, total; };
inline DecSeqWs dec_seq_layout(int dtype, const EmDecoderWeights* dw, size_t M, size_t head_bytes, bool refine) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  Bump b;
  DecSeqWs w;
  w.x = b.take(M * dw->d * 4);
  w.xn = b.take(M * dw->d * es);
  w.qkv = b.take(M * 3 * dw->d * es);
  w.ctx = b.take(M * dw->d * es);
  w.h = b.take(M * dw->ff * es);
  w.head = b.take(head_bytes);
  w.s = w.a = b.o;
  if (refine) w.s = b.take(M * 4), w.a = b.take(M * 4);
  w.total = b.o;
  return w;
}
// ... and its rows (csrc/dec_seq.hip): the embedding of tok [B][Lp] and the num_blocks layers over the M = B * Lp rows,
// enqueue only; the f32 residual rows are left at ws + o.x for the caller's head.  The self-attention is causal with
// self_x [B][Lp] as the key mask (em_lm_causal_attention) or, without the diagonal, over the first self_x[b] keys
// (em_dec_full_attention); sentence b reads memory mem_of[b] (b itself without mem_of) of the Bm in mem_kv / mem_vT.
int dec_seq_rows(int dtype, const EmDecoderWeights* dw, const void* mem_kv, const void* mem_vT, const int32_t* klens,
                 const int32_t* mem_of, int Bm, const int32_t* tok, bool causal, const int32_t* self_x, int B, int Lp, int T,
                 int Tpad, void* ws, const DecSeqWs& o, void* stream);

// ---- per-head operands of the batch encoders' attention: Tpad frames per (utterance, head), a multiple of 256
inline int tpad256(int T) { return (T + 255) / 256 * 256; }
inline size_t head_slab_bytes(int B, int d, int Tpad, size_t es) { return (size_t)B * d * Tpad * es; }

// The shared part of "attention reads per-head operands": bf16, d_k = 64, offsets inside the slabs fit 32 bits
// (ESPNET_AMD_NO_ATTN2_LARGE=1: developer A/B switch).  What differs between the callers stays at their call sites.
inline bool head_operands_ok(int dtype, int d, int h, int B, int Tpad) {
  return dtype == EM_BF16 && !em_sw().no_attn2_large && d == 64 * h && (size_t)B * d * Tpad * 4 < ((size_t)1 << 32) - 64;
}

// The projection GEMMs write the operands themselves, no repacking pass: q | k of xn [M = B*T][d] through EM_EPI_QK_HEADS
// (k follows q at B * d * Tpad elements), V^T as the swapped product W_v . xn^T through EM_EPI_VT_HEADS.
// wqkv [3d][d]: the q, k, v rows; bqkv [3d].
inline int project_heads(int dtype, const void* xn, const void* wqkv, const float* bqkv, void* qh, void* vt, int M, int d, int h,
                         int T, int Tpad, void* stream) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  EmGemmArgs a = {};
  a.A = xn; a.W = wqkv; a.C = qh; a.bias = bqkv;
  a.M = M; a.N = 2 * d; a.K = d; a.lda = d; a.ldc = 64; a.scale = 1.f;
  a.T1 = T; a.T2 = Tpad; a.F1 = h; a.d = d;
  EM_TRY(em_gemm(dtype, EM_EPI_QK_HEADS, EM_A_PLAIN, &a, stream));
  a.A = (const unsigned char*)wqkv + (size_t)2 * d * d * es; a.W = xn; a.C = vt; a.bias = bqkv + 2 * d;
  a.M = d; a.N = M; a.ldc = Tpad;
  return em_gemm(dtype, EM_EPI_VT_HEADS, EM_A_PLAIN, &a, stream);
}

// Zero `bytes` of the slabs from `first` on: frames >= T of a (b, head) slab are masked, not skipped, so they must be finite.
inline int clear_head_slabs(void* first, size_t bytes, void* stream) {
  return hipMemsetAsync(first, 0, bytes, (hipStream_t)stream) == hipSuccess ? EM_OK : EM_ERR_LAUNCH;
}

// ---- a 512-wide bf16 model runs its feed-forward modules as row-block launches of 64-row workgroups (csrc/ffn_rows.hip)
// when the shape fits, nothing switches them off (EM_ENC_NO_FUSED; ESPNET_AMD_NO_FFN_ROWS=1: developer switch) and a round
// of workgroups fills its share of the chip (em_rows_fill_ok, csrc/encoder.hip).  The caller still checks that the host
// packed the operand streams.  espnet_amd/asr/encoder/_subsampled_base.py: rows_ffn_packable mirrors the shape part.
inline bool rows_ffn_ok(int dtype, int d, int ff, int flags, long M) {
  return dtype == EM_BF16 && d == 512 && ff % 128 == 0 && ff >= 256 && !(flags & EM_ENC_NO_FUSED) && !em_sw().no_ffn_rows &&
         em_rows_fill_ok(M, flags);
}

// ---- the two contextual-block streaming encoders (csrc/streaming.hip: Conformer layers, csrc/streaming_tf.hip: Transformer
// layers): the same blocks [n_streams * n_blk_s][L][d] f32, the same FFN launch shape, the same context hand-over.

// Shares of an FFN's hidden dimension per 32-row block in the fused streaming layers (EmBlockArgs.ffn_split, round 6).  A tick
// of a few streams runs every launch on a few of the chip's 256 CUs, each pushing the whole 2 MiB of an FFN through ONE CU's
// MFMA pipes (~8 us of a ~20 us launch); S workgroups per row block take 1 / S of it each and meet once (a store, a ticket,
// the last one sums: 3 - 5 us, growing with S).  Measured per call of 12 Conformer layers (profiles/r06t_stream_split_sweep.txt):
//   streams (row blocks)   1 (2)   8 (16)   16 (32)   32 (64)   64 (128)
//   S = 1                  926     941      941       945       946   us
//   S = 2                  788     807      846       874      1029
//   S = 4                  720     772      840       996      1430
//   S = 8                  742     826     1030      1429      2184
// so: 4 up to 32 row blocks, 2 up to 64, 1 beyond; whole pairs of 64-wide chunks per share.
// ESPNET_AMD_STREAM_FFN_SPLIT=n: developer switch (1 = off, n = forced).
inline int stream_ffn_split(int ff, int row_blocks) {
  const int forced = em_sw().stream_ffn_split;
  const int pairs = (((ff >> 6) + 1) & ~1) / 2;
  int S = forced > 0 ? forced : row_blocks <= 32 ? 4 : row_blocks <= 64 ? 2 : 1;
  if (S > 16) S = 16;
  while (S > 1 && pairs % S != 0) --S;
  return S;
}
// ... its meeting place behind a fused layout: partial sums [row blocks][S][8192] f32 + one ticket per row block
inline void stream_ffn_slots(Bump& b, int ff, int row_blocks, size_t* part, size_t* ticket) {
  const int S = stream_ffn_split(ff, row_blocks);
  *part = b.take(S > 1 ? (size_t)row_blocks * S * 8192 * 4 : 0);
  *ticket = b.take(S > 1 ? (size_t)row_blocks * 4 : 0);
}
// ... and a call's set-up.  The tickets start at zero and every launch leaves them there.
inline int stream_ffn_setup(EmBlockArgs& ba, int row_blocks, void* part, void* ticket, void* stream) {
  const int S = stream_ffn_split(ba.ff, row_blocks);
  if (S <= 1) return EM_OK;
  ba.ffn_split = S; ba.ffn_part = (float*)part; ba.ffn_ticket = (int32_t*)ticket;
  return hipMemsetAsync(ticket, 0, (size_t)row_blocks * 4, (hipStream_t)stream) == hipSuccess ? EM_OK : EM_ERR_LAUNCH;
}

// One block per stream (the steady-state tick) with both context buffers: the hand-over after layer l is "slot 0 := the
// previous call's context vector of layer l; this call's := the last slot", so it rides in the fused launches (EmBlockArgs
// row0_src / last_dst) - a launch less per layer (4.9 us each, 59 of a 32-stream tick's 1 170 us;
// profiles/r05x_stream_batch32_kernel_stats.csv).  past_ctx == next_ctx: the next layer would read THIS call's vector where it
// wants the previous call's - the hand-over launch reads before it writes and is safe in place, so an aliased call keeps it
// (ADVICE r05).  ESPNET_AMD_STREAM_NO_CTX_FOLD: developer A/B switch, read per call (tests/test_gpu_streaming.py compares
// the two bit for bit).
inline bool stream_fold_ctx(int mask_mode, int n_blk_s, const float* past_ctx, const float* next_ctx) {
  return mask_mode && n_blk_s == 1 && past_ctx && next_ctx && past_ctx != next_ctx && !em_sw().stream_no_ctx_fold;
}

// The hand-over after layer l as its own launch: x[b][0] := the block in front's last slot, or past_ctx[l] for a stream's first
// block; next_ctx[l] := the last slot of its last block.  past_ctx / next_ctx [n_streams][NL][d].
inline int stream_hand_over(float* x, const float* past_ctx, float* next_ctx, int l, int n_streams, int n_blk_s, int L, int d,
                            int NL, void* stream) {
  return em_cb_propagate_ctx_batch_f32(x, past_ctx ? past_ctx + (size_t)l * d : nullptr,
                                       next_ctx ? next_ctx + (size_t)l * d : nullptr, n_streams, n_blk_s, L, d, NL * d, stream);
}

// The per-operator sequences' scratch opens with xn [M][d] (a LayerNorm's output) and big [M][max(ff, 3d)] (an FFN's hidden
// rows, or q | k | v), in the activation type; `row` = the bytes of one more [M][d] slot (the attention's output, ...).
struct StreamWsHead { size_t xn, big, row; };
inline StreamWsHead stream_ws_head(Bump& b, int dtype, int d, int ff, int M) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  const size_t wide = ff > 3 * d ? ff : 3 * d;
  StreamWsHead s;
  s.row = (size_t)M * d * es;
  s.xn = b.take(s.row);
  s.big = b.take((size_t)M * wide * es);
  return s;
}

// C = epi(LayerNorm(x) W^T + bias) on the f32 blocks x [M][d] of a per-operator sequence.  The pre-norm rides in the prologue
// of the projection that consumes it (csrc/ln_gemm.hip) where that kernel has the shape: a launch less per projection.  A
// step is ~200 dependent launches of ~5.6 us for 42 rows - launch latency, nothing else - so the count is what matters
// (round 3: 1.30 -> see profiles/r03p).  ESPNET_AMD_STREAM_NO_LN_GEMM: developer A/B switch.
struct StreamLnProj {
  int dtype, M, d;
  const float* x;
  void* xn;  // [M][d] act: the LayerNorm's output where it is a launch of its own
  void* stream;
  bool lng = !em_sw().stream_no_ln_gemm && d % 64 == 0 && d <= 1024;
  int operator()(int epi, const float* g, const float* be, const void* W, const float* bias, void* C, int N) const {
    if (lng) return em_ln_gemm(dtype, epi, x, g, be, LN_EPS, W, bias, C, M, N, d, N, stream);
    EM_TRY(em_layernorm(dtype, x, g, be, M, d, LN_EPS, xn, nullptr, stream));
    return gemm(dtype, epi, xn, W, C, bias, M, N, d, d, N, 1.f, stream);
  }
};

}  // namespace em_host
