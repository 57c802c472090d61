// espnet_amd — the transducer's default beam search on gfx950, whole batches in lock-step (contract:
// include/espnet_amd.h, "transducer beam search").  Reference: espnet2/asr/transducer/beam_search_transducer.py
// (BeamSearchTransducer.default_beam_search).
//
// One STEP is one expansion - the pop of the best open hypothesis - for every utterance that is still live, enqueued as
// a stream-ordered chain with no read-back:
//     select -> cell (one launch per layer) -> lin_dec -> tanh -> joint logits -> expand
// select and expand are one workgroup per utterance and hold the search's bookkeeping; the four launches between them are
// the row kernels of csrc/transducer_rows.h with rows = utterances, so a row's log-probabilities carry the bits of
// em_transducer_dec_step + em_transducer_joint_logp called for that row alone, and with scores summed in double (the host
// route sums Python floats) both routes make the same decisions.
//
// Bookkeeping of one utterance (all in the workspace):
//   nodes   (parent, token, length, slot): one per EXPANDED hypothesis, never freed (T x EXP_CAP of them: every expansion
//           of every frame); label sequences are the back-pointer chains.
//   open    (score, node, token): the reference's `hyps`.  Appended in the reference's order and never moved inside a
//           frame - a popped entry is marked dead - so the lowest index of equal scores is the earliest inserted, which
//           is what max() over the list takes.  token >= 0: the child `node + [token]`, not expanded yet; TOK_CARRIED:
//           `node` itself, kept at the last frame's end - its state and lin_dec row are stored, the cell's result for its
//           row is ignored (the reference's cache by label sequence).
//   kept    (score, node): the reference's `kept`, one per expansion of the frame.
//   slots   h / c per layer and the lin_dec row of an expanded node, while something can still read them: a child reads
//           its parent's slot as its pre-state, a carried node its own lin_dec row.  At a frame's end every slot but the
//           carried nodes' is free again (a used flag per slot; nothing is copied).
// A frame ends when the kept entries strictly above the best open score number at least `beam`; exactly those are
// carried, in kept order (equal scores stay in insertion order, as the reference's stable sort leaves them).
//
// With a language model (em_transducer_beam_search_lm, shallow fusion) a step is
//     select -> cell.. -> lin_dec -> tanh -> joint logits -> LM cell (one launch per layer) -> LM head -> expand
// and every slot also holds the LM's h / c per layer: the state after the LM has read sos and the node's labels.  A
// child reads its parent's slot as the LM's pre-state; for a carried entry select lays the node's OWN slot into the LM's
// input state, the masked cells copy it through and the head recomputes the node's LM row from its stored top h (V-wide
// rows are not kept per slot).  expand adds lm_weight * lm_logp[k] to the beam_k children in double, product and sum
// rounded separately, as the host route's Python floats are.
#include <math.h>

#include "em_common.h"
#include "transducer_rows.h"
#include "enc_host.h"

namespace {

constexpr int MAX_BEAM = 16;
constexpr int EXP_CAP = 128;                             // expansions of one frame = its kept entries = carried entries
constexpr int NSLOT = 2 * EXP_CAP;                       // the carried nodes' and this frame's; = the workgroup size
constexpr int OPEN_CAP = EXP_CAP + EXP_CAP * MAX_BEAM;   // carried + beam_k children per expansion
constexpr int MAX_LABELS = 1024;                         // labels of one hypothesis, the leading blank included
constexpr int TOK_DEAD = -1, TOK_CARRIED = -2;
constexpr int WG = 256;
static_assert(NSLOT == WG, "one thread per slot in the free-slot search");

enum { ST_RUNNING = 0, ST_DONE = 1, ST_EXP_LIMIT = 2, ST_CAP_EXPANSIONS = 3, ST_CAP_LABELS = 4, ST_CAP_NBEST = 5 };
enum { C_LIVE, C_T, C_OLEN, C_NOPEN, C_NKEPT, C_NEXP, C_NNODES, C_CUR_NODE, C_CUR_TOK, C_TOTAL, C_MAXEXP, C_N = 16 };

struct BeamP {
  int B, T, V, L, d, jp, beam, beam_k, ocap, ncap, max_exp, Lmax, nbest_cap, blank;
  const int32_t* olens;
  int32_t *g_live, *ctl;
  double* cur_score;
  double* open_score;
  int32_t *open_node, *open_tok;
  double* kept_score;
  int32_t* kept_node;
  int4* node;
  int32_t* slot_used;
  void* slot_hs;
  float *slot_cs, *dec_proj_all;
  void *hs_in, *hs_out;
  float *cs_in, *cs_out;
  int32_t *tok, *mask, *enc_idx, *dec_idx;
  float* logits;
  int32_t *status, *out_tokens, *out_lens, *out_count;
  double* out_scores;
  float* step_logp;
  int32_t* step_trace;
  // the fused language model (lmL == 0: none)
  int lmL, lmd;
  double lm_weight;
  void *lm_slot_hs, *lm_hs_in, *lm_hs_out;
  float *lm_slot_cs, *lm_cs_in, *lm_cs_out;
  int32_t* lm_tok;
  float *lm_logits, *step_lm_logp;
};

// (base + w * x) with the product and the sum rounded one after the other: what the host route's Python floats give
__device__ __forceinline__ double add_lm_term(double base, double w, double x) {
#pragma clang fp contract(off)
  const double t = w * x;
  return base + t;
}

// the better of two (score, index) pairs: the higher score, the LOWER index of equal scores; index < 0: none
struct Best {
  double s;
  int i;
};
__device__ __forceinline__ Best best_merge(Best a, Best b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  return (b.s > a.s || (b.s == a.s && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ Best block_best(Best v, Best* sh) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = best_merge(v, Best{__shfl_xor(v.s, o, 64), __shfl_xor(v.i, o, 64)});
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const Best r = best_merge(best_merge(sh[0], sh[1]), best_merge(sh[2], sh[3]));
  __syncthreads();
  return r;
}

// (thread 0 of the utterance's workgroup) the utterance takes no further step
__device__ void beam_end(const BeamP& p, int b, int32_t* ctl, int state) {
  ctl[C_LIVE] = 0;
  p.mask[b] = 0;
  p.status[b * 4 + 0] = state;
  p.status[b * 4 + 1] = ctl[C_T];
  atomicSub(p.g_live, 1);
}

__global__ __launch_bounds__(64) void beam_init_kernel(BeamP p) {
  const int b = threadIdx.x;
  int live = 0;
  if (b < p.B) {
    const int olen = min(p.olens[b], p.T);
    live = olen > 0;
    int32_t* ctl = p.ctl + b * C_N;
    for (int i = 0; i < C_N; ++i) ctl[i] = 0;
    ctl[C_LIVE] = live;
    ctl[C_OLEN] = olen;
    ctl[C_NOPEN] = 1;
    p.open_score[(size_t)b * p.ocap] = 0.0;  // the reference's first hypothesis: [blank] from the zero state
    p.open_node[(size_t)b * p.ocap] = -1;
    p.open_tok[(size_t)b * p.ocap] = p.blank;
    p.tok[b] = p.blank;
    if (p.lmL) p.lm_tok[b] = p.V - 1;
    p.mask[b] = 0;
    p.enc_idx[b] = b * p.T;
    p.dec_idx[b] = p.B * NSLOT + b;
    p.status[b * 4 + 0] = live ? ST_RUNNING : ST_DONE;
    p.status[b * 4 + 1] = p.status[b * 4 + 2] = p.status[b * 4 + 3] = 0;
    p.out_count[b] = 0;
    for (int i = 0; i < NSLOT; ++i) p.slot_used[b * NSLOT + i] = 0;
    for (int j = 0; j < p.jp; ++j) p.dec_proj_all[((size_t)p.B * NSLOT + b) * p.jp + j] = 0.f;
  }
  const unsigned long long m = __ballot(live);
  if (threadIdx.x == 0) *p.g_live = __popcll(m);
}

// ---- select: pop the best open hypothesis of utterance b and lay out its row for the prediction network and the joint
template <typename T>
__global__ __launch_bounds__(WG) void beam_select_kernel(BeamP p) {
  __shared__ Best sh[4];
  __shared__ int s_pre, s_skip, s_lm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (*p.g_live == 0) return;
  int32_t* ctl = p.ctl + b * C_N;
  if (ctl[C_LIVE] == 0) return;
  const int n_open = ctl[C_NOPEN];
  const double* os = p.open_score + (size_t)b * p.ocap;
  int32_t* on = p.open_node + (size_t)b * p.ocap;
  int32_t* ot = p.open_tok + (size_t)b * p.ocap;
  Best v{0.0, -1};
  for (int i = tid; i < n_open; i += WG)
    if (ot[i] != TOK_DEAD) v = best_merge(v, Best{os[i], i});
  v = block_best(v, sh);
  if (tid == 0) {
    s_pre = -1;
    s_skip = 1;
    s_lm = -2;  // the slot the LM's input state comes from; -1: the zero state, -2: none (the utterance ended here)
    if (v.i < 0) {  // (an open set is never empty: every expansion appends beam_k >= 1 children)
      beam_end(p, b, ctl, ST_CAP_EXPANSIONS);
    } else {
      const int node = on[v.i], tk = ot[v.i];
      ot[v.i] = TOK_DEAD;
      if (tk == TOK_CARRIED) {
        p.mask[b] = 0;
        p.dec_idx[b] = b * NSLOT + p.node[(size_t)b * p.ncap + node].w;
        s_lm = p.node[(size_t)b * p.ncap + node].w;  // its own state: the masked cells copy it, the head reads its top h
      } else {
        if (node >= 0) s_pre = p.node[(size_t)b * p.ncap + node].w;
        s_lm = s_pre;
        if (p.lmL) p.lm_tok[b] = node < 0 ? p.V - 1 : tk;  // the first hypothesis feeds sos = V - 1
        p.tok[b] = tk;
        p.mask[b] = 1;
        p.dec_idx[b] = p.B * NSLOT + b;
        s_skip = 0;
      }
      p.enc_idx[b] = b * p.T + ctl[C_T];
      p.cur_score[b] = v.s;
      ctl[C_CUR_NODE] = node;
      ctl[C_CUR_TOK] = tk;
    }
  }
  __syncthreads();
  if (p.lmL && s_lm != -2) {
    const int src = s_lm, d = p.lmd, L = p.lmL;
    const T* shs = (const T*)p.lm_slot_hs + ((size_t)b * NSLOT + max(src, 0)) * L * d;
    const float* scs = p.lm_slot_cs + ((size_t)b * NSLOT + max(src, 0)) * L * d;
    for (int i = tid; i < L * d; i += WG) {
      const int l = i / d, c = i - l * d;
      const size_t o = ((size_t)l * p.B + b) * d + c;
      ((T*)p.lm_hs_in)[o] = src < 0 ? from_f32<T>(0.f) : shs[i];
      p.lm_cs_in[o] = src < 0 ? 0.f : scs[i];
    }
  }
  if (s_skip) return;
  const int pre = s_pre, d = p.d, L = p.L;
  const T* shs = (const T*)p.slot_hs + ((size_t)b * NSLOT + max(pre, 0)) * L * d;
  const float* scs = p.slot_cs + ((size_t)b * NSLOT + max(pre, 0)) * L * d;
  for (int i = tid; i < L * d; i += WG) {
    const int l = i / d, c = i - l * d;
    const size_t o = ((size_t)l * p.B + b) * d + c;
    ((T*)p.hs_in)[o] = pre < 0 ? from_f32<T>(0.f) : shs[i];
    p.cs_in[o] = pre < 0 ? 0.f : scs[i];
  }
}

// ---- expand: the log-softmax of the row, the blank extension to kept, the beam_k best labels to open, the frame's end
template <typename T>
__global__ __launch_bounds__(WG) void beam_expand_kernel(BeamP p) {
  __shared__ Best sh[4];
  __shared__ float s_lse, s_lm_lse;
  __shared__ int s_w[4], s_e, s_slot, s_ended;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (*p.g_live == 0) return;
  int32_t* ctl = p.ctl + b * C_N;
  if (ctl[C_LIVE] == 0) return;
  const int V = p.V, t = ctl[C_T], n_open0 = ctl[C_NOPEN], n_kept0 = ctl[C_NKEPT], n_exp = ctl[C_NEXP];
  const int cur_node = ctl[C_CUR_NODE], cur_tok = ctl[C_CUR_TOK], olen = ctl[C_OLEN];
  const bool marked = cur_tok == TOK_CARRIED;
  const double score = p.cur_score[b];
  float* row = p.logits + (size_t)b * V;
  const float* lm_row = p.lmL ? p.lm_logits + (size_t)b * V : nullptr;
  int4* nodes = p.node + (size_t)b * p.ncap;
  int32_t* su = p.slot_used + b * NSLOT;
  // the log-softmax exactly as em_log_softmax_rows_f32 takes it (wave_row_lse): one wave, its lanes stride the row
  if (wave == 0 || (wave == 1 && p.lmL)) {  // (wave 1: the LM row's, the same way, beside it)
    const float v = wave_row_lse(wave == 0 ? row : lm_row, V, lane);
    if (lane == 0) (wave == 0 ? s_lse : s_lm_lse) = v;
  }
  const unsigned long long fm = __ballot(su[tid] == 0);
  if (lane == 0) s_w[wave] = fm ? wave * 64 + __ffsll((long long)fm) - 1 : NSLOT;
  __syncthreads();
  const float lse = s_lse, lm_lse = p.lmL ? s_lm_lse : 0.f;
  for (int c = tid; c < V; c += WG) {
    const float x = row[c] - lse;
    row[c] = x;
    if (p.step_logp) p.step_logp[(size_t)b * V + c] = x;
    if (p.step_lm_logp) p.step_lm_logp[(size_t)b * V + c] = lm_row[c] - lm_lse;
  }
  if (tid == 0) {
    s_ended = 0;
    int e = cur_node, slot = -1;
    if (!marked) {
      const int len = (cur_node < 0 ? 0 : nodes[cur_node].z) + 1;
      slot = min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
      e = ctl[C_NNODES];
      if (len > p.Lmax) {
        beam_end(p, b, ctl, ST_CAP_LABELS);
        s_ended = 1;
      } else if (slot >= NSLOT || e >= p.ncap) {  // (neither can happen below EXP_CAP expansions per frame)
        beam_end(p, b, ctl, ST_CAP_EXPANSIONS);
        s_ended = 1;
      } else {
        nodes[e] = make_int4(cur_node, cur_tok, len, slot);
        su[slot] = 1;
        ctl[C_NNODES] = e + 1;
      }
    }
    s_e = e;
    s_slot = slot;
  }
  __syncthreads();
  if (s_ended) return;
  const int e = s_e;
  if (!marked) {  // the cell's and lin_dec's results of this row into the new node's slot
    const int d = p.d, L = p.L, slot = s_slot;
    T* shs = (T*)p.slot_hs + ((size_t)b * NSLOT + slot) * L * d;
    float* scs = p.slot_cs + ((size_t)b * NSLOT + slot) * L * d;
    for (int i = tid; i < L * d; i += WG) {
      const int l = i / d, c = i - l * d;
      const size_t o = ((size_t)l * p.B + b) * d + c;
      shs[i] = ((const T*)p.hs_out)[o];
      scs[i] = p.cs_out[o];
    }
    const float* src = p.dec_proj_all + ((size_t)p.B * NSLOT + b) * p.jp;
    float* dst = p.dec_proj_all + ((size_t)b * NSLOT + slot) * p.jp;
    for (int j = tid; j < p.jp; j += WG) dst[j] = src[j];
    if (p.lmL) {  // and the LM cells' results
      const int dl = p.lmd, Ll = p.lmL;
      T* lhs = (T*)p.lm_slot_hs + ((size_t)b * NSLOT + slot) * Ll * dl;
      float* lcs = p.lm_slot_cs + ((size_t)b * NSLOT + slot) * Ll * dl;
      for (int i = tid; i < Ll * dl; i += WG) {
        const int l = i / dl, c = i - l * dl;
        const size_t o = ((size_t)l * p.B + b) * dl + c;
        lhs[i] = ((const T*)p.lm_hs_out)[o];
        lcs[i] = p.lm_cs_out[o];
      }
    }
  }
  double* os = p.open_score + (size_t)b * p.ocap;
  int32_t* on = p.open_node + (size_t)b * p.ocap;
  int32_t* ot = p.open_tok + (size_t)b * p.ocap;
  double* ks = p.kept_score + (size_t)b * EXP_CAP;
  int32_t* kn = p.kept_node + (size_t)b * EXP_CAP;
  if (tid == 0) {
    ks[n_kept0] = score + (double)row[0];  // (index 0, as the reference's logp[0]; the labels are logp[1:])
    kn[n_kept0] = e;
    if (p.step_trace) {  // test hook: the expanded hypothesis of this step
      int32_t* tr = p.step_trace + (size_t)b * (4 + p.Lmax);
      const int len = nodes[e].z;
      tr[0] = 1, tr[1] = t, tr[2] = marked, tr[3] = len;
      for (int n = e, q = len - 1; q >= 0 && n >= 0; --q, n = nodes[n].x) tr[4 + q] = nodes[n].y;
    }
  }
  // the beam_k best labels on the log-probabilities, the lowest id first among equal ones, in rank order
  double pv = INFINITY;
  int pi = -1, found = 0;
  for (int j = 0; j < p.beam_k; ++j) {
    Best v{0.0, -1};
    for (int c = 1 + tid; c < V; c += WG) {
      const double x = (double)row[c];
      if (x < pv || (x == pv && c > pi)) v = best_merge(v, Best{x, c});
    }
    v = block_best(v, sh);
    if (v.i < 0) break;  // (fewer than beam_k comparable labels: a row of NaN)
    if (tid == 0) {
      const double child = score + v.s;
      os[n_open0 + j] = p.lmL ? add_lm_term(child, p.lm_weight, (double)(lm_row[v.i] - lm_lse)) : child;
      on[n_open0 + j] = e;
      ot[n_open0 + j] = v.i;
    }
    pv = v.s;
    pi = v.i;
    ++found;
  }
  const int n_open = n_open0 + found, n_kept = n_kept0 + 1;
  __syncthreads();
  // the end test: the kept entries strictly above the best open score
  Best bl{0.0, -1};
  for (int i = tid; i < n_open; i += WG)
    if (ot[i] != TOK_DEAD) bl = best_merge(bl, Best{os[i], i});
  bl = block_best(bl, sh);
  const bool above = tid < n_kept && bl.i >= 0 && ks[tid] > bl.s;
  const unsigned long long am = __ballot(above);
  if (lane == 0) s_w[wave] = __popcll(am);
  __syncthreads();
  const int cnt = s_w[0] + s_w[1];  // (n_kept <= EXP_CAP = 128: waves 0 and 1)
  const int pos = (wave == 1 ? s_w[0] : 0) + __popcll(am & ((1ull << lane) - 1ull));
  const int total = ctl[C_TOTAL] + 1, mexp = max(ctl[C_MAXEXP], n_exp + 1);
  __syncthreads();
  if (tid == 0) {
    ctl[C_TOTAL] = total;
    ctl[C_MAXEXP] = mexp;
    p.status[b * 4 + 2] = total;
    p.status[b * 4 + 3] = mexp;
  }
  if (cnt < p.beam) {  // the frame goes on
    if (tid == 0) {
      ctl[C_NOPEN] = n_open;
      ctl[C_NKEPT] = n_kept;
      ctl[C_NEXP] = n_exp + 1;
      if (n_exp + 1 >= min(p.max_exp, EXP_CAP)) beam_end(p, b, ctl, n_exp + 1 >= p.max_exp ? ST_EXP_LIMIT : ST_CAP_EXPANSIONS);
    }
    return;
  }
  if (t + 1 >= olen) {  // the last frame: the final kept list, in kept order
    if (cnt > p.nbest_cap) {
      if (tid == 0) beam_end(p, b, ctl, ST_CAP_NBEST);
      return;
    }
    if (above) {
      const size_t o = (size_t)b * p.nbest_cap + pos;
      const int len = nodes[kn[tid]].z;
      p.out_scores[o] = ks[tid];
      p.out_lens[o] = len;
      int32_t* yt = p.out_tokens + o * p.Lmax;
      for (int n = kn[tid], q = len - 1; q >= 0 && n >= 0; --q, n = nodes[n].x) yt[q] = nodes[n].y;
    }
    if (tid == 0) {
      p.out_count[b] = cnt;
      beam_end(p, b, ctl, ST_DONE);
    }
    return;
  }
  // the next frame: the qualifying kept entries are the open set, every slot but theirs is free
  if (above) {
    os[pos] = ks[tid];
    on[pos] = kn[tid];
    ot[pos] = TOK_CARRIED;
  }
  su[tid] = 0;
  __syncthreads();
  if (above) su[nodes[kn[tid]].w] = 1;
  if (tid == 0) {
    ctl[C_NOPEN] = cnt;
    ctl[C_NKEPT] = 0;
    ctl[C_NEXP] = 0;
    ctl[C_T] = t + 1;
  }
}

struct BeamWs {
  size_t g_live, ctl, cur_score, open_score, open_node, open_tok, kept_score, kept_node, node, slot_used, slot_hs, slot_cs,
      dec_proj_all, hs_in, hs_out, cs_in, cs_out, tok, mask, enc_idx, dec_idx, z, logits, lm_slot_hs, lm_slot_cs, lm_hs_in,
      lm_hs_out, lm_cs_in, lm_cs_out, lm_tok, lm_logits, total;
};
int beam_ocap(const EmTransducerWeights* w, int beam) {
  const int bm = beam < w->vocab ? beam : w->vocab;
  const int bk = bm < w->vocab - 1 ? bm : w->vocab - 1;
  return EXP_CAP + EXP_CAP * bk;
}
BeamWs beam_layout(int dtype, const EmTransducerWeights* w, const EmTransducerLmWeights* lm, int B, int T, int beam) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  const size_t ocap = beam_ocap(w, beam), st = (size_t)w->num_layers * w->d;
  BeamWs o;
  em_host::Bump b;
  o.g_live = b.take(4);
  o.ctl = b.take((size_t)B * C_N * 4);
  o.cur_score = b.take((size_t)B * 8);
  o.open_score = b.take((size_t)B * ocap * 8);
  o.open_node = b.take((size_t)B * ocap * 4);
  o.open_tok = b.take((size_t)B * ocap * 4);
  o.kept_score = b.take((size_t)B * EXP_CAP * 8);
  o.kept_node = b.take((size_t)B * EXP_CAP * 4);
  o.node = b.take((size_t)B * T * EXP_CAP * sizeof(int4));
  o.slot_used = b.take((size_t)B * NSLOT * 4);
  o.slot_hs = b.take((size_t)B * NSLOT * st * es);
  o.slot_cs = b.take((size_t)B * NSLOT * st * 4);
  o.dec_proj_all = b.take(((size_t)B * NSLOT + B) * w->jp * 4);
  o.hs_in = b.take((size_t)B * st * es);
  o.hs_out = b.take((size_t)B * st * es);
  o.cs_in = b.take((size_t)B * st * 4);
  o.cs_out = b.take((size_t)B * st * 4);
  o.tok = b.take((size_t)B * 4);
  o.mask = b.take((size_t)B * 4);
  o.enc_idx = b.take((size_t)B * 4);
  o.dec_idx = b.take((size_t)B * 4);
  o.z = b.take((size_t)B * w->jp * es);
  o.logits = b.take((size_t)B * w->vocab * 4);
  o.lm_slot_hs = o.lm_slot_cs = o.lm_hs_in = o.lm_hs_out = o.lm_cs_in = o.lm_cs_out = o.lm_tok = o.lm_logits = 0;
  if (lm) {
    const size_t lst = (size_t)lm->num_layers * lm->d;
    o.lm_slot_hs = b.take((size_t)B * NSLOT * lst * es);
    o.lm_slot_cs = b.take((size_t)B * NSLOT * lst * 4);
    o.lm_hs_in = b.take((size_t)B * lst * es);
    o.lm_hs_out = b.take((size_t)B * lst * es);
    o.lm_cs_in = b.take((size_t)B * lst * 4);
    o.lm_cs_out = b.take((size_t)B * lst * 4);
    o.lm_tok = b.take((size_t)B * 4);
    o.lm_logits = b.take((size_t)B * w->vocab * 4);
  }
  o.total = b.o;
  return o;
}

bool beam_shape_ok(int dtype, const EmTransducerWeights* w, const EmTransducerLmWeights* lm, int B, int T, int beam) {
  if (check_weights(dtype, w) != EM_OK || B <= 0 || T <= 0 || beam < 1) return false;
  if (lm && (check_lm_weights(dtype, lm) != EM_OK || lm->vocab != w->vocab)) return false;
  return B <= MAXROWS && beam <= MAX_BEAM && (long long)T * EXP_CAP < (1ll << 30) / B;
}

template <typename T>
int beam_t(int dtype, const EmTransducerWeights* w, const EmTransducerLmWeights* lm, BeamP p, const float* enc_proj,
           int T_frames, int first, int steps, unsigned char* ws, hipStream_t s) {
  const BeamWs o = beam_layout(dtype, w, lm, p.B, T_frames, p.beam);
  p.g_live = (int32_t*)(ws + o.g_live), p.ctl = (int32_t*)(ws + o.ctl), p.cur_score = (double*)(ws + o.cur_score);
  p.open_score = (double*)(ws + o.open_score), p.open_node = (int32_t*)(ws + o.open_node);
  p.open_tok = (int32_t*)(ws + o.open_tok), p.kept_score = (double*)(ws + o.kept_score);
  p.kept_node = (int32_t*)(ws + o.kept_node), p.node = (int4*)(ws + o.node), p.slot_used = (int32_t*)(ws + o.slot_used);
  p.slot_hs = ws + o.slot_hs, p.slot_cs = (float*)(ws + o.slot_cs), p.dec_proj_all = (float*)(ws + o.dec_proj_all);
  p.hs_in = ws + o.hs_in, p.hs_out = ws + o.hs_out, p.cs_in = (float*)(ws + o.cs_in), p.cs_out = (float*)(ws + o.cs_out);
  p.tok = (int32_t*)(ws + o.tok), p.mask = (int32_t*)(ws + o.mask), p.enc_idx = (int32_t*)(ws + o.enc_idx);
  p.dec_idx = (int32_t*)(ws + o.dec_idx), p.logits = (float*)(ws + o.logits);
  if (lm) {
    p.lm_slot_hs = ws + o.lm_slot_hs, p.lm_slot_cs = (float*)(ws + o.lm_slot_cs), p.lm_hs_in = ws + o.lm_hs_in;
    p.lm_hs_out = ws + o.lm_hs_out, p.lm_cs_in = (float*)(ws + o.lm_cs_in), p.lm_cs_out = (float*)(ws + o.lm_cs_out);
    p.lm_tok = (int32_t*)(ws + o.lm_tok), p.lm_logits = (float*)(ws + o.lm_logits);
  }
  T* z = (T*)(ws + o.z);
  const int B = p.B, V = p.V;
  if (first) hipLaunchKernelGGL(beam_init_kernel, dim3(1), dim3(64), 0, s, p);
  for (int i = 0; i < steps; ++i) {
    hipLaunchKernelGGL(beam_select_kernel<T>, dim3(B), dim3(WG), 0, s, p);
    EM_TRY(dec_rows<T>(w, p.tok, p.mask, B, (size_t)B * w->d, (const T*)p.hs_in, p.cs_in, (T*)p.hs_out, p.cs_out, nullptr,
                       p.dec_proj_all + (size_t)B * NSLOT * w->jp, nullptr, 0, 0, (T*)nullptr, s, p.g_live));
    hipLaunchKernelGGL(pair_tanh_kernel<T>, dim3(B), dim3(128), 0, s, enc_proj, (const int32_t*)p.enc_idx,
                       (const float*)p.dec_proj_all, (const int32_t*)p.dec_idx, B, w->jp, z, (const int32_t*)p.g_live);
    hipLaunchKernelGGL((joint_kernel<T, true>), dim3(em_cdiv(V, 16)), dim3(256), 0, s, (const T*)z, (const T*)w->lin_out,
                       w->out_b, B, V, w->jp, p.logits, (float4*)nullptr, (const int32_t*)p.g_live, (const int32_t*)nullptr);
    if (lm)  // (every row's head runs: a carried entry's LM row is recomputed from the state its masked cells copied)
      EM_TRY(lm_rows<T>(lm, p.lm_tok, p.mask, nullptr, B, (size_t)B * lm->d, (const T*)p.lm_hs_in, p.lm_cs_in,
                        (T*)p.lm_hs_out, p.lm_cs_out, p.lm_logits, s, p.g_live));
    hipLaunchKernelGGL(beam_expand_kernel<T>, dim3(B), dim3(WG), 0, s, p);
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" void em_transducer_beam_limits(int32_t* beam_max, int32_t* open_max, int32_t* kept_max, int32_t* expansions_max,
                                          int32_t* labels_max) {
  if (beam_max) *beam_max = MAX_BEAM;
  if (open_max) *open_max = OPEN_CAP;
  if (kept_max) *kept_max = EXP_CAP;
  if (expansions_max) *expansions_max = EXP_CAP;
  if (labels_max) *labels_max = MAX_LABELS;
}

extern "C" size_t em_transducer_beam_workspace_bytes_lm(int dtype, const EmTransducerWeights* w,
                                                        const EmTransducerLmWeights* lm, int32_t B, int32_t T, int32_t beam) {
  if (!beam_shape_ok(dtype, w, lm, B, T, beam)) return 0;
  return beam_layout(dtype, w, lm, B, T, beam).total;
}

extern "C" size_t em_transducer_beam_workspace_bytes(int dtype, const EmTransducerWeights* w, int32_t B, int32_t T,
                                                     int32_t beam) {
  return em_transducer_beam_workspace_bytes_lm(dtype, w, nullptr, B, T, beam);
}

extern "C" int em_transducer_beam_search_lm(int dtype, const EmTransducerWeights* w, const EmTransducerLmWeights* lm,
                                            double lm_weight, const float* enc_proj, const int32_t* olens, int32_t B,
                                            int32_t T, int32_t beam, int32_t max_expansions, int32_t Lmax, int32_t nbest_cap,
                                            int32_t first, int32_t steps, int32_t* status, int32_t* out_tokens,
                                            int32_t* out_lens, double* out_scores, int32_t* out_count, float* step_logp,
                                            int32_t* step_trace, float* step_lm_logp, void* ws, size_t ws_bytes,
                                            void* stream) {
  EM_TRY(check_weights(dtype, w));
  if (lm) EM_TRY(check_lm_weights(dtype, lm));
  if ((lm && lm->vocab != w->vocab) || (!lm && step_lm_logp)) return EM_ERR_BAD_ARG;
  if (B <= 0 || T <= 0 || beam < 1 || max_expansions < 1 || Lmax < 1 || nbest_cap < 1 || steps < 0) return EM_ERR_BAD_ARG;
  if (!enc_proj || !olens || !status || !out_tokens || !out_lens || !out_scores || !out_count) return EM_ERR_BAD_ARG;
  if (!beam_shape_ok(dtype, w, lm, B, T, beam) || Lmax > MAX_LABELS || nbest_cap > EXP_CAP) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < beam_layout(dtype, w, lm, B, T, beam).total) return EM_ERR_UNSUPPORTED;
  BeamP p{};
  p.B = B, p.T = T, p.V = w->vocab, p.L = w->num_layers, p.d = w->d, p.jp = w->jp;
  p.beam = beam < w->vocab ? beam : w->vocab;
  p.beam_k = p.beam < w->vocab - 1 ? p.beam : w->vocab - 1;
  p.ocap = beam_ocap(w, beam), p.ncap = T * EXP_CAP, p.max_exp = max_expansions, p.Lmax = Lmax, p.nbest_cap = nbest_cap;
  p.blank = w->blank, p.olens = olens;
  p.status = status, p.out_tokens = out_tokens, p.out_lens = out_lens, p.out_scores = out_scores, p.out_count = out_count;
  p.step_logp = step_logp, p.step_trace = step_trace;
  if (lm) p.lmL = lm->num_layers, p.lmd = lm->d, p.lm_weight = lm_weight, p.step_lm_logp = step_lm_logp;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* q = (unsigned char*)ws;
  if (dtype == EM_BF16) return beam_t<bf16>(dtype, w, lm, p, enc_proj, T, first, steps, q, s);
  return beam_t<float>(dtype, w, lm, p, enc_proj, T, first, steps, q, s);
}

extern "C" int em_transducer_beam_search(int dtype, const EmTransducerWeights* w, const float* enc_proj, const int32_t* olens,
                                         int32_t B, int32_t T, int32_t beam, int32_t max_expansions, int32_t Lmax,
                                         int32_t nbest_cap, int32_t first, int32_t steps, int32_t* status,
                                         int32_t* out_tokens, int32_t* out_lens, double* out_scores, int32_t* out_count,
                                         float* step_logp, int32_t* step_trace, void* ws, size_t ws_bytes, void* stream) {
  return em_transducer_beam_search_lm(dtype, w, nullptr, 0.0, enc_proj, olens, B, T, beam, max_expansions, Lmax, nbest_cap,
                                      first, steps, status, out_tokens, out_lens, out_scores, out_count, step_logp,
                                      step_trace, nullptr, ws, ws_bytes, stream);
}
