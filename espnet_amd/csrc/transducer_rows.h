// espnet_amd — the row kernels of transducer decoding on gfx950, shared by the greedy walk and the primitives
// (csrc/transducer.hip) and the default beam search (csrc/transducer_beam.hip): one recurrent layer of the prediction
// network, lin_dec, the joint network's tanh and its output product.
//
// Every product here has few rows (the utterances of a batch, or the hypotheses of a beam: <= 64 per launch) against a
// weight matrix that is streamed once, so all three MFMA kernels share one shape: a workgroup of four waves owns 16 output
// columns (the cell kernel: 16 channels x 4 gates) for ALL rows, operands go from global memory straight into MFMA
// registers, the waves' results meet in 16 KiB of LDS and wave w finishes row tile w.  No workgroup ever waits for
// another one.  A row's result depends on that row's operands only (one MFMA row per row, the same k order whatever n
// is), so row r of an n-row launch carries the bits of the same row launched alone.
//
// `live` (NULL: none) is a device counter a chain of launches may hand over: a launch that reads zero there returns at
// once (the beam search's steps behind the end of its last utterance).
#pragma once
#include <math.h>

#include "em_common.h"
#include "rnn_cell.h"

namespace {

constexpr int MAXRT = 4;  // 16-row tiles per launch: n <= 64 rows
constexpr int MAXROWS = 16 * MAXRT;

// acc[rt] += A[row(rt)][k] * W[col][k] over the k-steps s0, s0 + stride, ... < nsteps of this wave.  arow / wrow carry
// the lane's k offset already (lg * EPL).  Only the nrt row tiles that hold rows are loaded and multiplied (nrt is
// uniform over the workgroup; the beam search calls with one row); rows past n inside the last tile are clamped by the
// caller and never stored.
template <typename T>
__device__ __forceinline__ void mma_span(const T* const (&arow)[MAXRT], const T* wrow, int s0, int stride, int nsteps,
                                         int nrt, f32x4 (&acc)[MAXRT]) {
  using MM = Mma<T>;
#pragma unroll 2
  for (int s = s0; s < nsteps; s += stride) {
    const typename MM::frag b = MM::load(wrow + (size_t)s * MM::K);
    typename MM::frag a[MAXRT];
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
      if (rt < nrt) a[rt] = MM::load(arow[rt] + (size_t)s * MM::K);
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
      if (rt < nrt) acc[rt] = MM::mma(a[rt], b, acc[rt]);
  }
}

__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MAXRT]) {
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// (max, arg-max, runner-up, sum of exp(x - max)) of a set of logits; merging two sets keeps the LOWEST id of equal maxima
// (torch.argmax / torch.topk on ties as the reference meets them) and, of two equal maxima, the other as runner-up.
struct Top {
  float m1;
  int i1;
  float m2, s;
};
__device__ __forceinline__ Top top_merge(Top a, Top b) {
  if (b.m1 == -INFINITY) return a;
  if (a.m1 == -INFINITY) return b;
  const bool take_b = b.m1 > a.m1 || (b.m1 == a.m1 && b.i1 < a.i1);
  Top r;
  r.m1 = take_b ? b.m1 : a.m1;
  r.i1 = take_b ? b.i1 : a.i1;
  r.m2 = take_b ? fmaxf(a.m1, b.m2) : fmaxf(a.m2, b.m1);
  r.s = a.s * expf(a.m1 - r.m1) + b.s * expf(b.m1 - r.m1);
  return r;
}
__device__ __forceinline__ Top top_shfl_xor(Top v, int o) {
  Top r;
  r.m1 = __shfl_xor(v.m1, o, 64);
  r.i1 = __shfl_xor(v.i1, o, 64);
  r.m2 = __shfl_xor(v.m2, o, 64);
  r.s = __shfl_xor(v.s, o, 64);
  return r;
}

// ---- joint network, output side: logits[r][v] = z[r] . lin_out[v] + out_b[v] for n <= 64 rows, z [n][jp] act =
// tanh(enc_proj + dec_proj).  One workgroup per 16 vocabulary columns; the waves split jp.
//   LOGITS: the f32 logits [n][V] are stored (em_transducer_joint_logp; the log-softmax follows in its own launch)
//   else  : one Top per (row, tile) goes to part [n][ntiles] (the greedy walk: the [B][V] logits never exist)
// rmask (NULL: none; LOGITS only): the logits of a row with rmask[r] == 0 are not stored.
// The same kernel is the language model's head in em_transducer_lm_step and the LM-fused beam search (z = the top
// layer's h, jp = the LM's padded hidden size).
template <typename T, bool LOGITS>
__global__ __launch_bounds__(256) void joint_kernel(const T* __restrict__ z, const T* __restrict__ w_out,
                                                    const float* __restrict__ out_b, int n, int V, int jp,
                                                    float* __restrict__ logits, float4* __restrict__ part,
                                                    const int32_t* __restrict__ live,
                                                    const int32_t* __restrict__ rmask) {
  using MM = Mma<T>;
  __shared__ f32x4 red[4][MAXRT][64];
  if (live && *live == 0) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int nrt = (n + 15) >> 4;
  const int v0 = blockIdx.x * 16;
  const int col = v0 + lr;
  const T* arow[MAXRT];
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt) {
    const int r = min(rt * 16 + lr, n - 1);
    arow[rt] = z + (size_t)r * jp + lg * MM::EPL;
  }
  const T* wrow = w_out + (size_t)min(col, V - 1) * jp + lg * MM::EPL;
  f32x4 acc[MAXRT];
  zero_acc(acc);
  mma_span<T>(arow, wrow, wave, 4, jp / MM::K, nrt, acc);
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt)
    if (rt < nrt) red[wave][rt][lane] = acc[rt];
  __syncthreads();
  if (wave >= nrt) return;
  const f32x4 v = (red[0][wave][lane] + red[1][wave][lane]) + (red[2][wave][lane] + red[3][wave][lane]);
  const float bias = out_b[min(col, V - 1)];
  const int ntiles = gridDim.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 16 + lg * 4 + q;
    const float x = v[q] + bias;
    if constexpr (LOGITS) {
      if (r < n && col < V && (!rmask || rmask[r] != 0)) logits[(size_t)r * V + col] = x;
    } else {
      Top t{col < V ? x : -INFINITY, col, -INFINITY, col < V ? 1.f : 0.f};
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) t = top_merge(t, top_shfl_xor(t, o));  // the 16 lanes of one row group
      if (lr == 0 && r < n) part[(size_t)r * ntiles + blockIdx.x] = make_float4(t.m1, __int_as_float(t.i1), t.m2, t.s);
    }
  }
}

// ---- one recurrent layer of the prediction network for n <= 64 rows (TransducerDecoder.rnn_forward, one step).
// Workgroup = 16 channels; wave g accumulates gate block g (EmRnnLayer: LSTM i | f | g | o, GRU r | z | n_x | n_h) of those
// channels over the layer input x and the previous hidden state, so that after the LDS exchange one lane holds the four
// gates of its (row, channel) and applies the cell (csrc/rnn_cell.h).  Layer 0 (tok != NULL) reads its input rows from
// the embedding table.  Rows with mask[r] == 0 copy their state; channels nhid .. d of every row are written zero.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void cell_kernel(const T* __restrict__ x, const int32_t* __restrict__ tok, int vocab,
                                                   int kin, const T* __restrict__ w_ih, const T* __restrict__ w_hh,
                                                   const float* __restrict__ bias, const int32_t* __restrict__ mask,
                                                   int n, int nhid, int d, const T* __restrict__ h_in,
                                                   const float* __restrict__ s_in, T* __restrict__ h_out,
                                                   float* __restrict__ s_out, float* __restrict__ dec_out) {
  using MM = Mma<T>;
  __shared__ f32x4 red[4][MAXRT][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int nrt = (n + 15) >> 4;
  const int ch = blockIdx.x * 16 + lr;
  const int live = (threadIdx.x < n) && (!mask || mask[threadIdx.x] != 0);
  const bool any = __syncthreads_or(live);
  if (any && blockIdx.x * 16 < nhid) {  // (workgroup-uniform)
    const T *xrow[MAXRT], *hrow[MAXRT];
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) {
      const int r = min(rt * 16 + lr, n - 1);
      int src = r;
      if (tok) src = min(max(tok[r], 0), vocab - 1);
      xrow[rt] = x + (size_t)src * kin + lg * MM::EPL;
      hrow[rt] = h_in + (size_t)r * d + lg * MM::EPL;
    }
    const size_t wr = (size_t)wave * nhid + min(ch, nhid - 1);
    f32x4 acc[MAXRT];
    zero_acc(acc);
    mma_span<T>(xrow, w_ih + wr * kin + lg * MM::EPL, 0, 1, kin / MM::K, nrt, acc);
    mma_span<T>(hrow, w_hh + wr * d + lg * MM::EPL, 0, 1, d / MM::K, nrt, acc);
    const float bg = bias[wr];
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
      if (rt < nrt) red[wave][rt][lane] = acc[rt] + bg;
  }
  __syncthreads();
  if (wave >= nrt || ch >= d) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 16 + lg * 4 + q;
    if (r >= n) continue;
    const size_t o = (size_t)r * d + ch;
    if (ch >= nhid) {
      h_out[o] = from_f32<T>(0.f);
      s_out[o] = 0.f;
      continue;
    }
    if (mask && mask[r] == 0) {
      h_out[o] = h_in[o];
      s_out[o] = s_in[o];
      continue;
    }
    float hh, ss;
    if constexpr (KIND == EM_LM_LSTM) {
      hh = em_lstm_cell(red[0][wave][lane][q], red[1][wave][lane][q], red[2][wave][lane][q], red[3][wave][lane][q],
                        s_in[o], &ss);
    } else {
      hh = ss = em_gru_cell(red[0][wave][lane][q], red[1][wave][lane][q], red[2][wave][lane][q], red[3][wave][lane][q],
                            s_in[o]);
    }
    h_out[o] = from_f32<T>(hh);
    s_out[o] = ss;
    if (dec_out) dec_out[(size_t)r * nhid + ch] = to_f32(from_f32<T>(hh));
  }
}

// ---- lin_dec of the joint network on the top layer's h (dec_proj [n][jp] f32, columns >= J zero, rows with mask[r] == 0
// not written) and, inside the walk (z != NULL), the joint network's hidden layer of the NEXT frame for every row:
// z[r][j] = tanh(enc_proj[r][t_next][j] + dec_proj[r][j]).  One workgroup per 16 columns; the waves split d.
template <typename T>
__global__ __launch_bounds__(256) void proj_kernel(const T* __restrict__ h, const T* __restrict__ w_dec,
                                                   const int32_t* __restrict__ mask, int n, int d, int J, int jp,
                                                   float* __restrict__ dec_proj, const float* __restrict__ enc_proj,
                                                   int T_frames, int t_next, T* __restrict__ z,
                                                   const int32_t* __restrict__ live) {
  using MM = Mma<T>;
  __shared__ f32x4 red[4][MAXRT][64];
  if (live && *live == 0) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int nrt = (n + 15) >> 4;
  const int j = blockIdx.x * 16 + lr;
  const T* arow[MAXRT];
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt) arow[rt] = h + (size_t)min(rt * 16 + lr, n - 1) * d + lg * MM::EPL;
  f32x4 acc[MAXRT];
  zero_acc(acc);
  mma_span<T>(arow, w_dec + (size_t)min(j, J - 1) * d + lg * MM::EPL, wave, 4, d / MM::K, nrt, acc);
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt)
    if (rt < nrt) red[wave][rt][lane] = acc[rt];
  __syncthreads();
  if (wave >= nrt || j >= jp) return;
  const f32x4 v = (red[0][wave][lane] + red[1][wave][lane]) + (red[2][wave][lane] + red[3][wave][lane]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 16 + lg * 4 + q;
    if (r >= n) continue;
    const size_t o = (size_t)r * jp + j;
    float dp;
    if (!mask || mask[r] != 0) {
      dp = j < J ? v[q] : 0.f;
      dec_proj[o] = dp;
    } else {
      dp = dec_proj[o];
    }
    if (z) z[o] = from_f32<T>(tanhf(enc_proj[((size_t)r * T_frames + t_next) * jp + j] + dp));
  }
}

// z[r][j] = tanh(enc_proj[enc_idx[r]][j] + dec_proj[dec_idx[r]][j]) for the pairs of em_transducer_joint_logp
template <typename T>
__global__ void pair_tanh_kernel(const float* __restrict__ enc_proj, const int32_t* __restrict__ enc_idx,
                                 const float* __restrict__ dec_proj, const int32_t* __restrict__ dec_idx, int n, int jp,
                                 T* __restrict__ z, const int32_t* __restrict__ live) {
  if (live && *live == 0) return;
  const int r = blockIdx.x;
  const float* e = enc_proj + (size_t)(enc_idx ? enc_idx[r] : r) * jp;
  const float* dd = dec_proj + (size_t)(dec_idx ? dec_idx[r] : r) * jp;
  for (int j = threadIdx.x; j < jp; j += blockDim.x) z[(size_t)r * jp + j] = from_f32<T>(tanhf(e[j] + dd[j]));
}

inline int check_weights(int dtype, const EmTransducerWeights* w) {
  if (!w || (dtype != EM_F32 && dtype != EM_BF16)) return EM_ERR_BAD_ARG;
  if (!w->embed || !w->rnn || !w->lin_dec || !w->lin_out || !w->out_b) return EM_ERR_BAD_ARG;
  if (w->vocab < 2 || w->nhid < 1 || w->num_layers < 1 || w->joint < 1 || w->blank < 0 || w->blank >= w->vocab) return EM_ERR_BAD_ARG;
  if (w->kind != EM_LM_LSTM && w->kind != EM_LM_GRU) return EM_ERR_UNSUPPORTED;
  if (w->d % 64 != 0 || w->jp % 64 != 0 || w->d < w->nhid || w->jp < w->joint) return EM_ERR_UNSUPPORTED;
  return EM_OK;
}

// the recurrent layers of a prediction network or a language model for n <= 64 rows (states: per-layer pointers at stride
// `lstride` elements): layer 0 reads its input rows, `kin0` wide, from the embedding table, the others the h below, d wide
template <typename T>
void rnn_layers(int kind, const EmRnnLayer* rnn, int num_layers, const void* embed, int vocab, int kin0, int nh, int d,
                const int32_t* tok, const int32_t* mask, int n, size_t lstride, const T* hs_in, const float* cs_in,
                T* hs_out, float* cs_out, float* dec_out, hipStream_t s) {
  for (int l = 0; l < num_layers; ++l) {
    const EmRnnLayer& q = rnn[l];
    const T* x = l == 0 ? (const T*)embed : hs_out + (size_t)(l - 1) * lstride;
    const int kin = l == 0 ? kin0 : d;
    float* dout = l == num_layers - 1 ? dec_out : nullptr;
    const dim3 grid(d / 16), block(256);
    if (kind == EM_LM_LSTM)
      hipLaunchKernelGGL((cell_kernel<T, EM_LM_LSTM>), grid, block, 0, s, x, l == 0 ? tok : nullptr, vocab, kin,
                         (const T*)q.w_ih, (const T*)q.w_hh, q.bias, mask, n, nh, d, hs_in + l * lstride,
                         cs_in + l * lstride, hs_out + l * lstride, cs_out + l * lstride, dout);
    else
      hipLaunchKernelGGL((cell_kernel<T, EM_LM_GRU>), grid, block, 0, s, x, l == 0 ? tok : nullptr, vocab, kin,
                         (const T*)q.w_ih, (const T*)q.w_hh, q.bias, mask, n, nh, d, hs_in + l * lstride,
                         cs_in + l * lstride, hs_out + l * lstride, cs_out + l * lstride, dout);
  }
}

// the prediction-network layers and lin_dec for n <= 64 rows
template <typename T>
int dec_rows(const EmTransducerWeights* w, const int32_t* tok, const int32_t* mask, int n, size_t lstride, const T* hs_in,
             const float* cs_in, T* hs_out, float* cs_out, float* dec_out, float* dec_proj, const float* enc_proj,
             int T_frames, int t_next, T* z, hipStream_t s, const int32_t* live = nullptr) {
  const int d = w->d;
  rnn_layers<T>(w->kind, w->rnn, w->num_layers, w->embed, w->vocab, d, w->nhid, d, tok, mask, n, lstride, hs_in, cs_in,
                hs_out, cs_out, dec_out, s);
  hipLaunchKernelGGL(proj_kernel<T>, dim3(w->jp / 16), dim3(256), 0, s, hs_out + (size_t)(w->num_layers - 1) * lstride,
                     (const T*)w->lin_dec, mask, n, d, w->joint, w->jp, dec_proj, enc_proj, T_frames, t_next, z, live);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

// ---- the language model fused into the beam search (EmTransducerLmWeights: a SequentialRNNLM, lstm or gru)
inline int check_lm_weights(int dtype, const EmTransducerLmWeights* w) {
  if (!w || (dtype != EM_F32 && dtype != EM_BF16)) return EM_ERR_BAD_ARG;
  if (!w->embed || !w->rnn || !w->out_w || !w->out_b) return EM_ERR_BAD_ARG;
  if (w->vocab < 2 || w->nhid < 1 || w->num_layers < 1 || w->embed_unit < 1) return EM_ERR_BAD_ARG;
  if (w->kind != EM_LM_LSTM && w->kind != EM_LM_GRU) return EM_ERR_UNSUPPORTED;
  if (w->d % 64 != 0 || w->embed_unit % 64 != 0 || w->d < w->nhid) return EM_ERR_UNSUPPORTED;
  return EM_OK;
}

// the LM's layers and its head (logits [n][vocab] f32, no log-softmax yet) for n <= 64 rows; states as dec_rows takes
// them.  Rows with mask[r] == 0 copy their state; head_mask (NULL: every row) keeps their logits rows unwritten.
template <typename T>
int lm_rows(const EmTransducerLmWeights* w, const int32_t* tok, const int32_t* mask, const int32_t* head_mask, int n,
            size_t lstride, const T* hs_in, const float* cs_in, T* hs_out, float* cs_out, float* logits, hipStream_t s,
            const int32_t* live = nullptr) {
  const int d = w->d;
  rnn_layers<T>(w->kind, w->rnn, w->num_layers, w->embed, w->vocab, w->embed_unit, w->nhid, d, tok, mask, n, lstride, hs_in,
                cs_in, hs_out, cs_out, (float*)nullptr, s);
  hipLaunchKernelGGL((joint_kernel<T, true>), dim3(em_cdiv(w->vocab, 16)), dim3(256), 0, s,
                     (const T*)(hs_out + (size_t)(w->num_layers - 1) * lstride), (const T*)w->out_w, w->out_b, n, w->vocab,
                     d, logits, (float4*)nullptr, live, head_mask);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace
