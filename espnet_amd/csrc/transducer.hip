// espnet_amd — transducer (RNN-T) decoding on gfx950: the prediction network step, the joint network and the fused
// greedy walk (contract: include/espnet_amd.h, "transducer").  Reference: espnet2/asr/decoder/transducer_decoder.py
// (TransducerDecoder.score / batch_score), espnet2/asr_transducer/joint_network.py (JointNetwork.forward),
// espnet2/asr/transducer/beam_search_transducer.py (BeamSearchTransducer.greedy_search).
//
// Every product here has few rows (the utterances of a batch, or the hypotheses of a beam: <= 64 per launch) against a
// weight matrix that is streamed once, so all three MFMA kernels share one shape: a workgroup of four waves owns 16 output
// columns (the cell kernel: 16 channels x 4 gates) for ALL rows, operands go from global memory straight into MFMA
// registers, the waves' results meet in 16 KiB of LDS and wave w finishes row tile w.  No workgroup ever waits for
// another one: the walk is a stream-ordered chain of launches per frame,
//     joint tiles -> decide -> cell (one launch per layer) -> lin_dec + next frame's tanh,
// with the same grid on every frame (so a vocabulary tile is read by the same XCD each time) and no host read-back.
#include <math.h>

#include "em_common.h"
#include "transducer_rows.h"
#include "enc_host.h"

namespace {

// ---- the greedy decision of frame t (BeamSearchTransducer.greedy_search: at most one label per frame): row b with
// t < olens[b] takes the arg-max of its joint log-softmax; a non-blank label is appended, its log-probability added to
// the score, and the row is marked to advance its prediction network.  One wave per utterance.
__global__ __launch_bounds__(64) void decide_kernel(const float4* __restrict__ part, int ntiles, int t, int T, int blank,
                                                    const int32_t* __restrict__ olens, int32_t* __restrict__ tokens,
                                                    int32_t* __restrict__ ylens, float* __restrict__ score,
                                                    int32_t* __restrict__ tok_cur, int32_t* __restrict__ emit,
                                                    int32_t* __restrict__ frame_tok, float* __restrict__ frame_top,
                                                    float* __restrict__ frame_margin) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (t >= olens[b]) {
    if (lane == 0) emit[b] = 0;
    return;
  }
  Top acc{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
  for (int i = lane; i < ntiles; i += 64) {
    const float4 p = part[(size_t)b * ntiles + i];
    acc = top_merge(acc, Top{p.x, __float_as_int(p.y), p.z, p.w});
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) acc = top_merge(acc, top_shfl_xor(acc, o));
  if (lane != 0) return;
  const float lp = -logf(acc.s);  // logit_max - logsumexp
  const int tok = acc.i1;
  const bool e = tok != blank;
  if (e) {
    const int y = ylens[b];
    tokens[(size_t)b * T + y] = tok;  // at most one label per frame: y <= t < T
    ylens[b] = y + 1;
    score[b] += lp;
    tok_cur[b] = tok;
  }
  emit[b] = e ? 1 : 0;
  if (frame_tok) {
    frame_tok[(size_t)b * T + t] = tok;
    frame_top[(size_t)b * T + t] = lp;
    frame_margin[(size_t)b * T + t] = acc.m1 - acc.m2;
  }
}

__global__ void walk_init_kernel(int B, int blank, int32_t* ylens, float* score, int32_t* tok_cur) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  ylens[b] = 0;
  score[b] = 0.f;
  tok_cur[b] = blank;
}

template <typename T>
int dec_step_t(const EmTransducerWeights* w, const int32_t* tok, const int32_t* mask, int n, const void* hs_in,
               const float* cs_in, void* hs_out, float* cs_out, float* dec_out, float* dec_proj, hipStream_t s) {
  const size_t ls = (size_t)n * w->d;
  for (int r0 = 0; r0 < n; r0 += MAXROWS) {
    const int m = n - r0 < MAXROWS ? n - r0 : MAXROWS;
    const size_t o = (size_t)r0 * w->d;
    EM_TRY(dec_rows<T>(w, tok + r0, mask ? mask + r0 : nullptr, m, ls, (const T*)hs_in + o, cs_in + o, (T*)hs_out + o,
                       cs_out + o, dec_out ? dec_out + (size_t)r0 * w->nhid : nullptr, dec_proj + (size_t)r0 * w->jp,
                       nullptr, 0, 0, (T*)nullptr, s));
  }
  return EM_OK;
}

template <typename T>
int joint_logp_t(const EmTransducerWeights* w, const float* enc_proj, const int32_t* enc_idx, const float* dec_proj,
                 const int32_t* dec_idx, int n, void* z_ws, float* logp, hipStream_t s) {
  const int V = w->vocab, jp = w->jp;
  hipLaunchKernelGGL(pair_tanh_kernel<T>, dim3(n), dim3(128), 0, s, enc_proj, enc_idx, dec_proj, dec_idx, n, jp, (T*)z_ws, (const int32_t*)nullptr);
  for (int r0 = 0; r0 < n; r0 += MAXROWS) {
    const int m = n - r0 < MAXROWS ? n - r0 : MAXROWS;
    hipLaunchKernelGGL((joint_kernel<T, true>), dim3(em_cdiv(V, 16)), dim3(256), 0, s, (const T*)z_ws + (size_t)r0 * jp,
                       (const T*)w->lin_out, w->out_b, m, V, jp, logp + (size_t)r0 * V, (float4*)nullptr, (const int32_t*)nullptr,
                       (const int32_t*)nullptr);
  }
  EM_CHECK_LAUNCH();
  return em_log_softmax_rows_f32(logp, n, V, s);
}

// em_log_softmax_rows_f32 (csrc/ctc.hip: one wave per row, wave_row_lse) for the rows with
// mask[r] != 0 only: the masked call of em_transducer_lm_step leaves the other rows as they are
__global__ __launch_bounds__(256) void masked_log_softmax_rows_kernel(float* __restrict__ x, const int32_t* __restrict__ mask,
                                                                      int M, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || mask[row] == 0) return;
  float* xr = x + (size_t)row * V;
  const float lse = wave_row_lse(xr, V, lane);
  for (int c = lane; c < V; c += 64) xr[c] = xr[c] - lse;
}

template <typename T>
int lm_step_t(const EmTransducerLmWeights* w, const int32_t* tok, const int32_t* mask, int n, const void* hs_in,
              const float* cs_in, void* hs_out, float* cs_out, float* logp, hipStream_t s) {
  const size_t ls = (size_t)n * w->d;
  for (int r0 = 0; r0 < n; r0 += MAXROWS) {
    const int m = n - r0 < MAXROWS ? n - r0 : MAXROWS;
    const size_t o = (size_t)r0 * w->d;
    const int32_t* mk = mask ? mask + r0 : nullptr;
    EM_TRY(lm_rows<T>(w, tok + r0, mk, mk, m, ls, (const T*)hs_in + o, cs_in + o, (T*)hs_out + o, cs_out + o,
                      logp + (size_t)r0 * w->vocab, s));
  }
  if (!mask) return em_log_softmax_rows_f32(logp, n, w->vocab, s);
  hipLaunchKernelGGL(masked_log_softmax_rows_kernel, dim3(em_cdiv(n, 4)), dim3(256), 0, s, logp, mask, n, w->vocab);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

// workspace of the walk: the carve-up below and em_transducer_greedy_workspace_bytes must agree
struct WalkWs {
  size_t part, z, dec_proj, hs, cs, tok_cur, emit, total;
};
WalkWs walk_layout(int dtype, const EmTransducerWeights* w, int B) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  WalkWs o;
  em_host::Bump b;
  o.part = b.take((size_t)B * em_cdiv(w->vocab, 16) * sizeof(float4));
  o.z = b.take((size_t)B * w->jp * es);
  o.dec_proj = b.take((size_t)B * w->jp * 4);
  o.hs = b.take((size_t)2 * w->num_layers * B * w->d * es);
  o.cs = b.take((size_t)2 * w->num_layers * B * w->d * 4);
  o.tok_cur = b.take((size_t)B * 4);
  o.emit = b.take((size_t)B * 4);
  o.total = b.o;
  return o;
}

template <typename T>
int greedy_t(int dtype, const EmTransducerWeights* w, const float* enc_proj, const int32_t* olens, int B, int T_frames,
             int32_t* tokens, int32_t* ylens, float* score, int32_t* frame_tok, float* frame_top, float* frame_margin,
             unsigned char* ws, hipStream_t s) {
  const WalkWs o = walk_layout(dtype, w, B);
  float4* part = (float4*)(ws + o.part);
  T* z = (T*)(ws + o.z);
  float* dec_proj = (float*)(ws + o.dec_proj);
  T* hs = (T*)(ws + o.hs);
  float* cs = (float*)(ws + o.cs);
  int32_t* tok_cur = (int32_t*)(ws + o.tok_cur);
  int32_t* emit = (int32_t*)(ws + o.emit);
  const size_t ls = (size_t)B * w->d, slot = ls * w->num_layers;
  const int V = w->vocab, ntiles = em_cdiv(V, 16);
  if (hipMemsetAsync(ws + o.hs, 0, o.tok_cur - o.hs, s) != hipSuccess) return EM_ERR_LAUNCH;  // zero states, both slots
  hipLaunchKernelGGL(walk_init_kernel, dim3(em_cdiv(B, 64)), dim3(64), 0, s, B, w->blank, ylens, score, tok_cur);
  // the blank label from the zero state (TransducerDecoder.init_state + the first score call), frame 0's hidden layer
  EM_TRY(dec_rows<T>(w, tok_cur, nullptr, B, ls, hs, cs, hs + slot, cs + slot, nullptr, dec_proj, enc_proj, T_frames, 0, z, s));
  int cur = 1;
  for (int t = 0; t < T_frames; ++t) {
    hipLaunchKernelGGL((joint_kernel<T, false>), dim3(ntiles), dim3(256), 0, s, (const T*)z, (const T*)w->lin_out, w->out_b,
                       B, V, w->jp, (float*)nullptr, part, (const int32_t*)nullptr, (const int32_t*)nullptr);
    hipLaunchKernelGGL(decide_kernel, dim3(B), dim3(64), 0, s, (const float4*)part, ntiles, t, T_frames, w->blank, olens,
                       tokens, ylens, score, tok_cur, emit, frame_tok, frame_top, frame_margin);
    if (t + 1 == T_frames) break;
    EM_TRY(dec_rows<T>(w, tok_cur, emit, B, ls, hs + cur * slot, cs + cur * slot, hs + (cur ^ 1) * slot,
                       cs + (cur ^ 1) * slot, nullptr, dec_proj, enc_proj, T_frames, t + 1, z, s));
    cur ^= 1;
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" int em_transducer_dec_step(int dtype, const EmTransducerWeights* w, const int32_t* tok, const int32_t* mask,
                                      int32_t n, const void* hs_in, const float* cs_in, void* hs_out, float* cs_out,
                                      float* dec_out, float* dec_proj, void* stream) {
  EM_TRY(check_weights(dtype, w));
  if (n <= 0 || !tok || !hs_in || !cs_in || !hs_out || !cs_out || !dec_proj || hs_in == hs_out || cs_in == cs_out)
    return EM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) return dec_step_t<bf16>(w, tok, mask, n, hs_in, cs_in, hs_out, cs_out, dec_out, dec_proj, s);
  return dec_step_t<float>(w, tok, mask, n, hs_in, cs_in, hs_out, cs_out, dec_out, dec_proj, s);
}

extern "C" int em_transducer_lm_step(int dtype, const EmTransducerLmWeights* w, const int32_t* tok, const int32_t* mask,
                                     int32_t n, const void* hs_in, const float* cs_in, void* hs_out, float* cs_out,
                                     float* logp, void* stream) {
  EM_TRY(check_lm_weights(dtype, w));
  if (n <= 0 || !tok || !hs_in || !cs_in || !hs_out || !cs_out || !logp || hs_in == hs_out || cs_in == cs_out)
    return EM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) return lm_step_t<bf16>(w, tok, mask, n, hs_in, cs_in, hs_out, cs_out, logp, s);
  return lm_step_t<float>(w, tok, mask, n, hs_in, cs_in, hs_out, cs_out, logp, s);
}

extern "C" int em_transducer_joint_logp(int dtype, const EmTransducerWeights* w, const float* enc_proj, const int32_t* enc_idx,
                                        const float* dec_proj, const int32_t* dec_idx, int32_t n, void* z_ws, float* logp,
                                        void* stream) {
  EM_TRY(check_weights(dtype, w));
  if (n <= 0 || !enc_proj || !dec_proj || !z_ws || !logp) return EM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) return joint_logp_t<bf16>(w, enc_proj, enc_idx, dec_proj, dec_idx, n, z_ws, logp, s);
  return joint_logp_t<float>(w, enc_proj, enc_idx, dec_proj, dec_idx, n, z_ws, logp, s);
}

extern "C" size_t em_transducer_greedy_workspace_bytes(int dtype, const EmTransducerWeights* w, int32_t B, int32_t T) {
  (void)T;
  if (check_weights(dtype, w) != EM_OK || B <= 0) return 0;
  return walk_layout(dtype, w, B).total;
}

extern "C" int em_transducer_greedy(int dtype, const EmTransducerWeights* w, const float* enc_proj, const int32_t* olens,
                                    int32_t B, int32_t T, int32_t* tokens, int32_t* ylens, float* score, int32_t* frame_tok,
                                    float* frame_top, float* frame_margin, void* ws, size_t ws_bytes, void* stream) {
  EM_TRY(check_weights(dtype, w));
  if (B <= 0 || T <= 0 || !enc_proj || !olens || !tokens || !ylens || !score) return EM_ERR_BAD_ARG;
  if (frame_tok && (!frame_top || !frame_margin)) return EM_ERR_BAD_ARG;
  if (B > MAXROWS) return EM_ERR_UNSUPPORTED;  // (the caller splits larger batches)
  if (!ws || ws_bytes < walk_layout(dtype, w, B).total) return EM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* p = (unsigned char*)ws;
  if (dtype == EM_BF16)
    return greedy_t<bf16>(dtype, w, enc_proj, olens, B, T, tokens, ylens, score, frame_tok, frame_top, frame_margin, p, s);
  return greedy_t<float>(dtype, w, enc_proj, olens, B, T, tokens, ylens, score, frame_tok, frame_top, frame_margin, p, s);
}
