// espnet_amd — the SequentialRNNLM over whole sentences on gfx950: per-token negative log-likelihoods of a batch in one
// enqueue (contract: include/espnet_amd.h, "recurrent language model over whole sentences").  Reference:
// espnet2/lm/espnet_model.py ESPnetLanguageModel.nll over espnet2/lm/seq_rnn_lm.py SequentialRNNLM.forward.
//
// The search's step path (csrc/search.hip rnn_lm_step) serves unknown continuations: per position an embedding, a state
// gather, two GEMMs and a cell launch per layer, and a head that writes [n][V] logits.  A sentence that is known beforehand
// allows another split of the work:
//   (a) every input token is known, so layer 0's input product gx0[b][t] = embed[x[b][t]] W_ih0^T + bias0 of all M = B * Lp
//       rows is ONE full-size GEMM (em_lm_embed + em_gemm), outside the recurrence;
//   (b) what is left of the recurrence is rnn_seq_step_kernel, launched as a wavefront over the layers: launch s runs layer
//       l at time t = s - l, for every layer that has such a t - Lp + nlayers - 1 dependent launches, not Lp * nlayers.  The
//       stream's order of launches is the only ordering between workgroups;
//   (c) the top layer's h of all rows goes through the vocabulary head that never stores logits (csrc/vocab_head.hip).
#include <math.h>

#include "em_common.h"
#include "enc_host.h"
#include "transducer_rows.h"

namespace {

using em_host::Bump;
using em_host::gemm;

constexpr int SEQ_LAYERS = 8;  // layers of one step launch (grid.z); a deeper model takes more launches per step

// what one step launch needs: the layers' matrices (kernel arguments: EmLmWeights.rnn is a host array) and the call's buffers
template <typename T>
struct SeqStep {
  const T* w_ih[SEQ_LAYERS];  // of the layers l0 .. l0 + gridDim.z - 1
  const T* w_hh[SEQ_LAYERS];
  const float* bias[SEQ_LAYERS];
  const float* gx0;      // [B][Lp][G * nhid] f32: layer 0's input product with its bias
  const int32_t* xlens;  // [B] or NULL
  T* hslots;             // [nlayers - 1][2][B][d]: h of the layers below the top one, slot = t & 1
  T* h_top;              // [B][Lp][d]: the top layer's h at every time
  float* master;         // [nlayers][B][d] f32: LSTM c, GRU h; in place (one lane per element and launch)
  int B, Lp, nhid, d, nlayers, l0, s;
};

// ---- one time step of one layer for a tile of <= 64 sentences and a group of 16 hidden channels; grid (d / 16, row tiles,
// layers of this launch), four waves.
//   LSTM / GRU: wave g accumulates gate block g (EmRnnLayer: i | f | g | o, r | z | n_x | n_h) of the group's channels for all
//     rows, operands straight from global memory into MFMA registers (mma_span, csrc/transducer_rows.h); the four tiles meet
//     in 16 KiB of LDS and wave w finishes row tile w: one lane holds the four gates of its (sentence, channel) and applies
//     the cell (csrc/rnn_cell.h).  The GRU's zero blocks (W_hh of n_x, W_ih of n_h) are not multiplied;
//   tanh / relu RNN: one gate block; the four waves split K and their partial tiles are summed in LDS.
// Layer 0's accumulators start from gx0[b][t] and contract over h0[t - 1] (K = d); layer l >= 1 starts from its bias and
// contracts over h_{l-1}[t] and h_l[t - 1] (K = 2d).  At t = 0 the previous state is zero: nothing is read for it, so no
// buffer needs clearing.  h_l[t] goes to slot t & 1 of its layer (the launch reads slot (t - 1) & 1 of the same layer and
// slot t & 1 of the layer below, both written by the launch before), the top layer's to h_top[b][t], where its own
// h[t - 1] is read from too.  Channels nhid .. d of every h row are written zero.  A row's result depends on that row's
// operands only (one MFMA row per sentence).  A tile whose sentences all ended before t returns at once; what the rows
// behind a sentence's end hold is never scored.
template <typename T, int KIND>
__global__ __launch_bounds__(256, 2) void rnn_seq_step_kernel(const SeqStep<T> a) {
  using MM = Mma<T>;
  constexpr bool GATED = KIND == EM_LM_LSTM || KIND == EM_LM_GRU;
  constexpr int G = GATED ? 4 : 1;
  __shared__ f32x4 red[4][MAXRT][64];
  const int li = blockIdx.z, l = a.l0 + li, t = a.s - l;
  if (t < 0 || t >= a.Lp) return;  // (workgroup-uniform, as every return before the barrier)
  const int r0 = blockIdx.y * MAXROWS, n = min(MAXROWS, a.B - r0);
  if (a.xlens) {
    const int live = (int)threadIdx.x < n && a.xlens[r0 + threadIdx.x] > t;
    if (!__syncthreads_or(live)) return;
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int nrt = (n + 15) >> 4;
  const int ch = blockIdx.x * 16 + lr;
  const int d = a.d, nhid = a.nhid;
  // this layer's h: the row of sentence r0 at time t (h_new) and t - 1 (h_prev), rows `hstride` elements apart
  size_t hstride;
  T* h_new;
  const T* h_prev;
  if (l == a.nlayers - 1) {
    hstride = (size_t)a.Lp * d;
    h_new = a.h_top + (size_t)r0 * hstride + (size_t)t * d;
    h_prev = t > 0 ? h_new - d : h_new;
  } else {
    hstride = d;
    T* base = a.hslots + (size_t)l * 2 * a.B * d;
    h_new = base + ((size_t)(t & 1) * a.B + r0) * d;
    h_prev = base + ((size_t)((t & 1) ^ 1) * a.B + r0) * d;
  }
  if (blockIdx.x * 16 < nhid) {
    const T* x = l > 0 ? a.hslots + (((size_t)(l - 1) * 2 + (t & 1)) * a.B + r0) * d : h_prev;  // (l == 0: not read)
    const T *xrow[MAXRT], *hrow[MAXRT];
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) {
      const int r = min(rt * 16 + lr, n - 1);
      xrow[rt] = x + (size_t)r * d + lg * MM::EPL;
      hrow[rt] = h_prev + (size_t)r * hstride + lg * MM::EPL;
    }
    const size_t wr = (size_t)(GATED ? wave : 0) * nhid + min(ch, nhid - 1);
    f32x4 acc[MAXRT];
    zero_acc(acc);
    if (GATED || wave == 0) {  // where the sum starts
      const float bg = a.bias[li][wr];
#pragma unroll
      for (int rt = 0; rt < MAXRT; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = min(rt * 16 + lg * 4 + q, n - 1);
          if (rt < nrt) acc[rt][q] = l == 0 ? a.gx0[((size_t)(r0 + r) * a.Lp + t) * (G * nhid) + wr] : bg;
        }
    }
    const int s0 = GATED ? 0 : wave, stride = GATED ? 1 : 4;
    if (l > 0 && !(KIND == EM_LM_GRU && wave == 3))
      mma_span<T>(xrow, a.w_ih[li] + wr * d + lg * MM::EPL, s0, stride, d / MM::K, nrt, acc);
    if (t > 0 && !(KIND == EM_LM_GRU && wave == 2))
      mma_span<T>(hrow, a.w_hh[li] + wr * d + lg * MM::EPL, s0, stride, d / MM::K, nrt, acc);
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
      if (rt < nrt) red[wave][rt][lane] = acc[rt];
  }
  __syncthreads();
  if (wave >= nrt) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 16 + lg * 4 + q;
    if (r >= n) continue;
    T* ho = h_new + (size_t)r * hstride + ch;
    if (ch >= nhid) {
      *ho = from_f32<T>(0.f);
      continue;
    }
    float* m = a.master + ((size_t)l * a.B + r0 + r) * d + ch;
    float hh;
    if constexpr (GATED) {
      const float sp = t > 0 ? *m : 0.f;
      float ss;
      if constexpr (KIND == EM_LM_LSTM) {
        hh = em_lstm_cell(red[0][wave][lane][q], red[1][wave][lane][q], red[2][wave][lane][q], red[3][wave][lane][q], sp, &ss);
      } else {
        hh = ss = em_gru_cell(red[0][wave][lane][q], red[1][wave][lane][q], red[2][wave][lane][q], red[3][wave][lane][q], sp);
      }
      *m = ss;
    } else {
      const float g = (red[0][wave][lane][q] + red[1][wave][lane][q]) + (red[2][wave][lane][q] + red[3][wave][lane][q]);
      hh = KIND == EM_LM_RNN_TANH ? tanhf(g) : fmaxf(g, 0.f);
    }
    *ho = from_f32<T>(hh);
  }
}

int gate_blocks(int kind) { return kind == EM_LM_LSTM || kind == EM_LM_GRU ? 4 : 1; }

bool rnn_kind(int kind) {
  return kind == EM_LM_LSTM || kind == EM_LM_GRU || kind == EM_LM_RNN_TANH || kind == EM_LM_RNN_RELU;
}

// M rows and the widest row (gx0's, an h row, an embedding row) stay inside 31-bit element offsets (the GEMM's buffer
// resources); the row tiles are a grid dimension; the head holds 64 rows of d in LDS (bf16) or one (f32)
bool rnn_seq_shape_ok(int dtype, const EmLmWeights* lm, int B, int Lp) {
  if (B <= 0 || Lp <= 0 || em_cdiv(B, MAXROWS) > 65535) return false;
  if (lm->num_blocks < 1 || lm->vocab < 1 || lm->nhid < 1 || lm->nhid > lm->d || lm->d % 64 || lm->embed_unit < 64 ||
      lm->embed_unit % 64)
    return false;
  if (dtype == EM_BF16 ? lm->d > 1024 : lm->d > 16384) return false;
  size_t wide = (size_t)gate_blocks(lm->kind) * lm->nhid;
  if (wide < (size_t)lm->d) wide = lm->d;
  if (wide < (size_t)lm->embed_unit) wide = lm->embed_unit;
  return (size_t)B * Lp * wide * 4 < ((size_t)1 << 31);
}

struct RnnSeqWs {
  size_t e, gx0, hslots, master, h_top, head, total;
};
RnnSeqWs rnn_seq_layout(int dtype, const EmLmWeights* lm, size_t B, size_t Lp) {
  const size_t es = dtype == EM_BF16 ? 2 : 4, M = B * Lp, d = lm->d;
  Bump b;
  RnnSeqWs s;
  s.e = b.take(M * lm->embed_unit * es);
  s.gx0 = b.take(M * gate_blocks(lm->kind) * lm->nhid * 4);
  s.hslots = b.take((size_t)(lm->num_blocks - 1) * 2 * B * d * es);
  s.master = b.take((size_t)lm->num_blocks * B * d * 4);
  s.h_top = b.take(M * d * es);
  s.head = b.take(em_lm_head_nll_workspace_bytes(dtype, (int32_t)M, lm->vocab));
  s.total = b.o;
  return s;
}

// the wavefront: launch s runs the layers lo .. hi that have a time step t = s - l in [0, Lp)
template <typename T>
int rnn_seq_chain(const EmLmWeights* lm, const float* gx0, const int32_t* xlens, int B, int Lp, void* hslots, float* master,
                  void* h_top, hipStream_t stream) {
  const int nl = lm->num_blocks;
  SeqStep<T> a = {};
  a.gx0 = gx0; a.xlens = xlens; a.hslots = (T*)hslots; a.h_top = (T*)h_top; a.master = master;
  a.B = B; a.Lp = Lp; a.nhid = lm->nhid; a.d = lm->d; a.nlayers = nl;
  for (int s = 0; s < Lp + nl - 1; ++s) {
    const int lo = s - Lp + 1 > 0 ? s - Lp + 1 : 0, hi = s < nl - 1 ? s : nl - 1;
    for (int l0 = lo; l0 <= hi; l0 += SEQ_LAYERS) {
      const int nz = hi - l0 + 1 < SEQ_LAYERS ? hi - l0 + 1 : SEQ_LAYERS;
      for (int i = 0; i < nz; ++i) {
        const EmRnnLayer& q = lm->rnn[l0 + i];
        a.w_ih[i] = (const T*)q.w_ih; a.w_hh[i] = (const T*)q.w_hh; a.bias[i] = q.bias;
      }
      a.l0 = l0; a.s = s;
      const dim3 grid(lm->d / 16, em_cdiv(B, MAXROWS), nz), block(256);
      switch (lm->kind) {
        case EM_LM_LSTM: hipLaunchKernelGGL((rnn_seq_step_kernel<T, EM_LM_LSTM>), grid, block, 0, stream, a); break;
        case EM_LM_GRU: hipLaunchKernelGGL((rnn_seq_step_kernel<T, EM_LM_GRU>), grid, block, 0, stream, a); break;
        case EM_LM_RNN_TANH: hipLaunchKernelGGL((rnn_seq_step_kernel<T, EM_LM_RNN_TANH>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((rnn_seq_step_kernel<T, EM_LM_RNN_RELU>), grid, block, 0, stream, a); break;
      }
    }
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" size_t em_rnn_lm_seq_nll_workspace_bytes(int dtype, const EmLmWeights* lm, int32_t B, int32_t Lp) {
  if (!lm || !rnn_kind(lm->kind) || (dtype != EM_BF16 && dtype != EM_F32) || !rnn_seq_shape_ok(dtype, lm, B, Lp)) return 0;
  return rnn_seq_layout(dtype, lm, (size_t)B, (size_t)Lp).total;
}

extern "C" int em_rnn_lm_seq_nll_parts(int dtype, const EmLmWeights* lm, const int32_t* x, const int32_t* target,
                                       const int32_t* xlens, int32_t B, int32_t Lp, float* nll, void* ws, size_t ws_bytes,
                                       int32_t parts, void* stream) {
  if (!lm || !x || !target || !nll || B <= 0 || Lp <= 0) return EM_ERR_BAD_ARG;
  if (dtype != EM_BF16 && dtype != EM_F32) return EM_ERR_BAD_ARG;
  if (!rnn_kind(lm->kind) || !lm->rnn || !lm->embed || !lm->out_w || !lm->out_b) return EM_ERR_BAD_ARG;
  if (!rnn_seq_shape_ok(dtype, lm, B, Lp)) return EM_ERR_UNSUPPORTED;
  const RnnSeqWs o = rnn_seq_layout(dtype, lm, (size_t)B, (size_t)Lp);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  const int M = B * Lp, V = lm->vocab, d = lm->d, eu = lm->embed_unit, gw = gate_blocks(lm->kind) * lm->nhid;
  unsigned char* base = (unsigned char*)ws;
  void *e = base + o.e, *hslots = base + o.hslots, *h_top = base + o.h_top;
  float *gx0 = (float*)(base + o.gx0), *master = (float*)(base + o.master);
  if (parts & EM_RNN_SEQ_HOIST) {  // (a) layer 0's input product of every row
    EM_TRY(em_lm_embed(dtype, lm->embed, x, M, V, eu, nullptr, 0, e, stream));
    EM_TRY(gemm(dtype, EM_EPI_SCALE_F32, e, lm->rnn[0].w_ih, gx0, lm->rnn[0].bias, M, gw, eu, eu, gw, 1.f, stream));
  }
  if (parts & EM_RNN_SEQ_CHAIN) {  // (b) the recurrence
    if (dtype == EM_BF16)
      EM_TRY(rnn_seq_chain<bf16>(lm, gx0, xlens, B, Lp, hslots, master, h_top, (hipStream_t)stream));
    else
      EM_TRY(rnn_seq_chain<float>(lm, gx0, xlens, B, Lp, hslots, master, h_top, (hipStream_t)stream));
  }
  if (parts & EM_RNN_SEQ_HEAD)  // (c) the head on the top layer's rows
    return em_head_rows_nll(dtype, h_top, lm->out_w, lm->out_b, target, M, V, d, nll, base + o.head, o.total - o.head, stream);
  return EM_OK;
}

extern "C" int em_rnn_lm_seq_nll(int dtype, const EmLmWeights* lm, const int32_t* x, const int32_t* target,
                                 const int32_t* xlens, int32_t B, int32_t Lp, float* nll, void* ws, size_t ws_bytes,
                                 void* stream) {
  return em_rnn_lm_seq_nll_parts(dtype, lm, x, target, xlens, B, Lp, nll, ws, ws_bytes,
                                 EM_RNN_SEQ_HOIST | EM_RNN_SEQ_CHAIN | EM_RNN_SEQ_HEAD, stream);
}
