// Back-off n-gram LM (ARPA) as a beam-search scorer: espnet2/legacy/nets/scorers/ngram.py (Ngrambase, NgramFullScorer,
// NgramPartScorer) on kenlm's FullScore, restated on the sorted trie of EmNgramModel (the host reader: csrc/host_io.cpp).
//
// Score of token v after the history h (log10, as in the file; no renormalisation over the token vocabulary):
//   c_k = the last k words of h (k <= N-1), j* = the largest k such that the (k+1)-gram (c_k, v) is in the model (0: the
//   unigram), score = p(c_j*, v) + bow(c_{j*+1}) + ... + bow(c_{N-1}), absent contexts contributing nothing; summed in f32
//   in that order (kenlm's FullScore accumulation).
//
// State carried, not rebuilt: a hypothesis keeps the trie node of each context length 1 .. N-1 (-1: not in the model).
// Extending it by a word costs one successor lookup per order, all independent: c'_1 = the word's unigram, c'_k = the
// successor of the parent's c_{k-1} with that word (kenlm's BaseScore(state, y[-1], out_state)).  A successor range is
// searched by a whole wave: 64 probes per round cut the range 65-fold (two rounds for 5 000 successors, then one probe per
// lane), instead of a lane-serial binary search of ~13 dependent loads.
//
// Full pass (NgramFullScorer, all V tokens), one workgroup per row: every column gets uni(v) + bow_1 + ... + bow_m, then for
// k = 1 .. m in order (a barrier between orders) the columns of c_k's successors are overwritten with
// p + bow_{k+1} + ... + bow_m: V + the successor counts of reads and writes per row.  Successors are scattered to the word's
// primary token (word2tok); the other tokens of a word - every unmapped token shares <unk> - are looked up one by one
// afterwards (alias list, usually two or three tokens).
// Part pass (NgramPartScorer), one wave per (row, candidate): the longest match of that one token.
#include "em_common.h"
#include "ngram_trie.h"

namespace {

// The row's new context nodes (s_node, and `out` when non-NULL) from its parent's (`prev`) and its last token.
__device__ __forceinline__ void advance_row(const EmNgramModel& m, bool start, const int32_t* prev, int last_tok,
                                            int32_t* s_node, int32_t* out, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  const int w = start ? 0 : tok_word(m, last_tok);
  for (int k = wave; k < m.order - 1; k += blockDim.x >> 6) {  // one wave per order, independent lookups
    const int nd = advance_one(m, k, start, prev, w, lane);
    if (lane == 0) {
      s_node[k] = nd;
      if (out) out[k] = nd;
    }
  }
  __syncthreads();
}

// Full pass of one row into out[V] (see the file comment); s_node = the row's context nodes.  Block-wide.
__device__ void full_row(const EmNgramModel& m, const int32_t* s_node, float* s_bow, float* __restrict__ out, int tid) {
  const int N = m.order, V = m.vocab, nthr = blockDim.x;
  if (tid < N - 1) s_bow[tid] = s_node[tid] >= 0 ? m.bow[tid][s_node[tid]] : 0.f;
  __syncthreads();
  // 1. unigram + every back-off.  Eight columns per thread and round, their word ids and then their probabilities requested
  // together: the token -> word -> probability chain is two dependent loads per ROUND, not per column (the plain loop made
  // this step ~20 us of a 24 us launch at V = 5 000: two dependent round trips for each of a thread's 20 columns).
  constexpr int U = 8;
  for (int v0 = tid; v0 < V; v0 += U * nthr) {
    int w[U];
    float p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = v0 + u * nthr;
      w[u] = v < V ? m.tok2word[v] : m.unk;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = m.prob[0][w[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = v0 + u * nthr;
      float acc = p[u];
      for (int L = 1; L < N; ++L)
        if (s_node[L - 1] >= 0) acc += s_bow[L - 1];
      if (v < V) out[v] = acc;
    }
  }
  // 2. successors of c_1, c_2, ... overwrite, longer contexts last
  for (int L = 1; L < N; ++L) {
    const int nd = s_node[L - 1];
    if (nd < 0) continue;  // (block-uniform)
    __syncthreads();
    const int lo = m.next[L - 1][nd], hi = m.next[L - 1][nd + 1];
    for (int e = lo + tid; e < hi; e += nthr) {
      const int t = m.word2tok[m.wid[L][e]];
      if (t < 0) continue;
      float acc = m.prob[L][e];
      for (int L2 = L + 1; L2 < N; ++L2)
        if (s_node[L2 - 1] >= 0) acc += s_bow[L2 - 1];
      out[t] = acc;
    }
  }
  __syncthreads();
  // 3. the tokens whose word's successors went to another token (<unk> and its kin): one lookup each
  const int wave = tid >> 6, lane = tid & 63;
  for (int a = wave; a < m.n_alias; a += nthr >> 6) {
    const int t = m.alias[a];
    const float sc = wave_score(m, s_node, m.tok2word[t], lane);
    if (lane == 0) out[t] = sc;
  }
}

// ---- stand-alone scorer call (em_ngram_score): one workgroup per row
__global__ __launch_bounds__(256) void ngram_score_kernel(EmNgramModel m, const int32_t* __restrict__ prev_state,
                                                          const int32_t* __restrict__ last_tok, int32_t* __restrict__ out_state,
                                                          const int32_t* __restrict__ cand, int n_cand, float* __restrict__ out) {
  __shared__ int32_t s_node[NG_MAX];
  __shared__ float s_bow[NG_MAX];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int ld = ng_ld(m);
  const int lt = last_tok[r];
  const bool start = lt < 0;
  advance_row(m, start, (start || !prev_state) ? nullptr : prev_state + (size_t)r * ld, lt, s_node, out_state + (size_t)r * ld, tid);
  if (tid == 0 && m.order == 1) out_state[(size_t)r * ld] = -1;
  if (!cand) {
    full_row(m, s_node, s_bow, out + (size_t)r * m.vocab, tid);
    return;
  }
  const int wave = tid >> 6, lane = tid & 63;
  for (int c = wave; c < n_cand; c += blockDim.x >> 6) {
    const float sc = wave_score(m, s_node, tok_word(m, cand[(size_t)r * n_cand + c]), lane);
    if (lane == 0) out[(size_t)r * n_cand + c] = sc;
  }
}

// ---- inside the fused search (csrc/search.hip): the rows of step i advance from their parents (token tree) ---------
// State of the rows of step i in st_a (i even) / st_b (i odd); a row reads its parent's (row parent[i][r] of step i-1)
// from the other one.  Full mode goes on with the row's full pass into logp.
__global__ __launch_bounds__(256) void ngram_search_kernel(EmNgramModel m, NgSearchArgs a, int i_host) {
  __shared__ int32_t s_node[NG_MAX];
  __shared__ float s_bow[NG_MAX];
  const int i = a.step ? *a.step : i_host;
  if (i >= a.Lmax - 1) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!a.alive[r] || a.done[r / a.W]) return;
  const int ld = ng_ld(m);
  const int32_t* prv = (i & 1) ? a.st_a : a.st_b;
  int32_t* cur = (i & 1) ? a.st_b : a.st_a;
  const bool start = i == 0;
  const int prow = start ? r : a.parent[(size_t)i * a.n + r];
  advance_row(m, start, prv + (size_t)prow * ld, a.tok[(size_t)i * a.n + r], s_node, cur + (size_t)r * ld, tid);
  if (a.logp) full_row(m, s_node, s_bow, a.logp + (size_t)r * m.vocab, tid);
}

// Part mode: the n-gram score of every pre-beam candidate slot (0 for the <eos> slot S, which is outside the pre-beam), and
// the slot's total rebuilt in the reference's order: full + w_ctc * ctc + w_ngram * ngram + running score
// (beam_search.py:219-234, part scorers in dict order).  One wave per (row, slot).
__global__ __launch_bounds__(256) void ngram_part_kernel(EmNgramModel m, NgSearchArgs a, int i_host) {
  const int i = a.step ? *a.step : i_host;
  if (i >= a.Lmax - 1) return;
  const int lane = threadIdx.x & 63;
  const long idx = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (long)a.n * a.NC) return;
  const int r = (int)(idx / a.NC), s = (int)(idx - (long)r * a.NC);
  if (!a.alive[r] || a.done[r / a.W]) return;
  const size_t o = (size_t)r * a.NC + s;
  const int n_part = a.S < a.V ? a.S : a.V;
  if (s >= n_part) {
    if (lane == 0) a.cand_ngram[o] = 0.f;
    return;
  }
  const int32_t* node = ((i & 1) ? a.st_b : a.st_a) + (size_t)r * ng_ld(m);
  __shared__ int32_t s_node[4][NG_MAX];
  const int wv = threadIdx.x >> 6;
  if (lane < m.order - 1) s_node[wv][lane] = node[lane];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const float sc = wave_score(m, s_node[wv], tok_word(m, a.cand_tok[o]), lane);
  if (lane == 0) {
    a.cand_ngram[o] = sc;
    float total = a.cand_full[o];
    if (a.w_ctc != 0.f) total = total + a.w_ctc * (a.cand_psi[o] - a.s_prev[r]);
    total = total + a.w_ngram * sc;
    a.cand_total[o] = total + a.run_score[r];
  }
}

int check_model(const EmNgramModel* m) {
  if (!m || m->order < 1 || m->order > NG_MAX || m->vocab <= 0 || !m->tok2word || !m->word2tok) return EM_ERR_BAD_ARG;
  if (m->n_alias < 0 || (m->n_alias > 0 && !m->alias) || m->unk < 0 || m->unk >= m->count[0] || m->bos >= m->count[0])
    return EM_ERR_BAD_ARG;
  for (int k = 0; k < m->order; ++k) {
    if (m->count[k] < 0 || !m->wid[k] || !m->prob[k] || !m->bow[k]) return EM_ERR_BAD_ARG;
    if (k < m->order - 1 && !m->next[k]) return EM_ERR_BAD_ARG;
  }
  return EM_OK;
}

}  // namespace

int ngram_search_step(const EmNgramModel* m, const NgSearchArgs& a, int i, void* stream) {
  if (check_model(m) != EM_OK || !a.st_a || !a.st_b || !a.tok || !a.parent || !a.alive || !a.done) return EM_ERR_BAD_ARG;
  if (m->vocab != a.V) return EM_ERR_BAD_ARG;
  hipLaunchKernelGGL(ngram_search_kernel, dim3(a.n), dim3(256), 0, (hipStream_t)stream, *m, a, i);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

int ngram_search_part(const EmNgramModel* m, const NgSearchArgs& a, int i, void* stream) {
  if (!a.cand_tok || !a.cand_full || !a.cand_ngram || !a.cand_total || !a.run_score || (a.w_ctc != 0.f && (!a.cand_psi || !a.s_prev)))
    return EM_ERR_BAD_ARG;
  const long waves = (long)a.n * a.NC;
  hipLaunchKernelGGL(ngram_part_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *m, a, i);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" int em_ngram_score(const EmNgramModel* m, int32_t n, const int32_t* prev_state, const int32_t* last_tok,
                              int32_t* out_state, const int32_t* cand, int32_t n_cand, float* out, void* stream) {
  if (check_model(m) != EM_OK || n < 0 || !last_tok || !out_state || !out || (cand && n_cand <= 0)) return EM_ERR_BAD_ARG;
  if (n == 0) return EM_OK;
  hipLaunchKernelGGL(ngram_score_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, *m, prev_state, last_tok, out_state,
                     cand, cand ? n_cand : 0, out);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
