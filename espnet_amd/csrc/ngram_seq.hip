// Back-off n-gram LM (ARPA): the log-probability of every token of GIVEN sentences in one enqueue (em_ngram_seq_logp) - the
// whole-sequence form of the step scorer of csrc/ngram.hip, as csrc/lm_seq.hip is of the neural LM's.
//
// The step scorer hands a trie state from step to step because the search does not know the next token.  For a given
// sentence the context of position j is the N-1 words before it, all known beforehand: every (sentence, position) pair is
// an independent lookup, and a sentence costs one launch instead of len(y) dependent ones that write V floats each.
//
// Work split: one lane per scored position, 256 positions of ONE row per workgroup (workgroup = (row, tile); the tiles
// behind a row's end leave at once).  The workgroup stages the word ids of its 256 positions and of the 5 (NG_MAX - 1)
// positions before them into LDS - the token -> word gather happens once per token, and a lane reads its predecessors from
// LDS, not through `order` dependent global loads.  History index -1 is <s>; nothing lies before it.
//
// A lane, for word w at position i with avail = min(N-1, i+1) words of context, from the longest context down:
//   c_L = the trie node of the last L words: the first word's unigram (or <s>), then L-1 successor searches - the very chain
//         of advance_one calls through which the step scorer reached that node, so the same node or the same -1;
//   f   = the successor of c_L with w (lane_find, the one-lane form of the lookup wave_score makes).  Found: p = prob[L][f],
//         the walk ends (the step scorer keeps the LONGEST match: ngram_trie.h wave_score, full_row's overwrite order);
//         not found: bow[L-1][c_L] is kept for the sum.
//   value = p + bow_{j*+1} + ... + bow_{N-1}, the contexts that are in the model only, added in f32 in that order: term for
//         term wave_score's and full_row's sum.  order_tok = j* + 1.
// At most 1 + 2 + .. + (N-1) searches per lane (15 at N = 6, 3 for a 3-gram), N-1 when the longest context matches.
//
// Row sums (f64, in position order, by one lane: no atomics, no tree, so a row's sum cannot depend on its companions):
// in the same launch when every row is one tile (Lp + eos <= 256), from the LDS copy of the values; else a second launch,
// one workgroup per row, which streams the row's stored values through LDS in tiles of 256 and adds them in the same order.
#include "em_common.h"
#include "ngram_trie.h"

namespace {

constexpr int NS_TILE = 256;
constexpr int NS_HALO = NG_MAX - 1;

// successor of `node` (an entry of order L, L >= 1) with word w: its index among the entries of order L+1, or -1
__device__ __forceinline__ int lane_succ(const EmNgramModel& m, int L, int node, int w) {
  const int lo = m.next[L - 1][node], hi = m.next[L - 1][node + 1];
  return hi > lo ? lane_find(m.wid[L], lo, hi, w) : -1;
}

__device__ __forceinline__ int row_len(const int32_t* __restrict__ ylens, int r, int Lp) {
  const int yl = ylens[r];
  return yl < 0 ? 0 : yl > Lp ? Lp : yl;  // (the host entry has checked its copy; the device copy is clamped all the same)
}

// logp == NULL: a second launch sums (tiles > 1)
__global__ __launch_bounds__(NS_TILE) void ngram_seq_kernel(EmNgramModel m, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ ylens, int Lp, int tiles, int eos_id,
                                                            float* __restrict__ logp_tok, int32_t* __restrict__ order_tok,
                                                            double* __restrict__ logp) {
  __shared__ int32_t s_w[NS_HALO + NS_TILE];  // word of history index base - NS_HALO + slot
  __shared__ float s_lp[NS_TILE];
  const int r = blockIdx.x / tiles, base = (blockIdx.x - r * tiles) * NS_TILE, tid = threadIdx.x;
  const int yl = row_len(ylens, r, Lp);
  const int len = yl + (eos_id >= 0 ? 1 : 0);
  if (base >= len) {  // (block-uniform)
    if (logp && tid == 0) logp[r] = 0.0;  // an empty row of a one-tile launch
    return;
  }
  for (int s = tid; s < NS_HALO + NS_TILE; s += NS_TILE) {
    const int q = base - NS_HALO + s;
    int w = -1;
    if (q == -1) w = m.bos;
    else if (q >= 0 && q < yl) w = tok_word(m, ids[(size_t)r * Lp + q]);
    else if (q == yl) w = tok_word(m, eos_id);  // (q == yl < len only with eos_id >= 0; the slots behind are never read)
    s_w[s] = w;
  }
  __syncthreads();
  const int i = base + tid;
  if (i < len) {
    const int32_t* h = s_w + NS_HALO + tid;  // h[0] = the scored word, h[-d] = the word d positions before it
    const int w = h[0];
    const int avail = min(m.order - 1, i + 1);
    float p = m.prob[0][w];
    int js = 0;
    float bw[NG_MAX];
    bool has[NG_MAX];
    bool found = false;
#pragma unroll
    for (int L = NG_MAX - 1; L >= 1; --L) {
      bw[L] = 0.f;
      has[L] = false;
      if (L > avail || found) continue;
      int node = h[-L];
      for (int k = 1; k < L && node >= 0; ++k) node = lane_succ(m, k, node, h[k - L]);
      if (node < 0) continue;  // the context is not in the model: no match, no back-off weight
      has[L] = true;
      const int f = lane_succ(m, L, node, w);
      if (f >= 0) {
        p = m.prob[L][f];
        js = L;
        found = true;
      } else {
        bw[L] = m.bow[L - 1][node];
      }
    }
    float acc = p;
#pragma unroll
    for (int L = 1; L < NG_MAX; ++L)
      if (L > js && has[L]) acc += bw[L];
    const size_t o = (size_t)r * (Lp + 1) + i;
    logp_tok[o] = acc;
    order_tok[o] = js + 1;
    s_lp[tid] = acc;
  }
  if (!logp) return;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int j = 0; j < len; ++j) s += (double)s_lp[j];
    logp[r] = s;
  }
}

// rows longer than a tile: the stored values of row blockIdx.x, added in position order
__global__ __launch_bounds__(NS_TILE) void ngram_seq_sum_kernel(const int32_t* __restrict__ ylens, int Lp, int eos,
                                                                const float* __restrict__ logp_tok, double* __restrict__ logp) {
  __shared__ float s_lp[NS_TILE];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int len = row_len(ylens, r, Lp) + eos;
  const float* row = logp_tok + (size_t)r * (Lp + 1);
  double s = 0.0;
  for (int base = 0; base < len; base += NS_TILE) {
    const int n = min(NS_TILE, len - base);
    if (tid < n) s_lp[tid] = row[base + tid];
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < n; ++j) s += (double)s_lp[j];
    __syncthreads();
  }
  if (tid == 0) logp[r] = s;
}

// what the kernels above read of the pack
int seq_check_model(const EmNgramModel* m) {
  if (!m || m->order < 1 || m->vocab <= 0 || !m->tok2word) return EM_ERR_BAD_ARG;
  if (m->order > NG_MAX) return EM_ERR_UNSUPPORTED;
  if (m->unk < 0 || m->unk >= m->count[0] || m->bos >= m->count[0]) return EM_ERR_BAD_ARG;
  for (int k = 0; k < m->order; ++k) {
    if (m->count[k] < 0 || !m->wid[k] || !m->prob[k] || !m->bow[k]) return EM_ERR_BAD_ARG;
    if (k < m->order - 1 && !m->next[k]) return EM_ERR_BAD_ARG;
  }
  return EM_OK;
}

}  // namespace

extern "C" int em_ngram_seq_logp(const EmNgramModel* m, const int32_t* ids, const int32_t* ylens, const int32_t* ids_host,
                                 const int32_t* ylens_host, int32_t N, int32_t Lp, int32_t eos_id, float* logp_tok,
                                 int32_t* order_tok, double* logp, void* stream) {
  const int rc = seq_check_model(m);
  if (rc != EM_OK) return rc;
  if (N < 0 || Lp < 0 || eos_id >= m->vocab) return EM_ERR_BAD_ARG;
  if (N == 0) return EM_OK;
  if (!ylens || !ylens_host || !logp_tok || !order_tok || !logp || (Lp > 0 && (!ids || !ids_host))) return EM_ERR_BAD_ARG;
  for (int r = 0; r < N; ++r) {
    const int yl = ylens_host[r];
    if (yl < 0 || yl > Lp) return EM_ERR_BAD_ARG;
    for (int j = 0; j < yl; ++j)
      if ((unsigned)ids_host[(size_t)r * Lp + j] >= (unsigned)m->vocab) return EM_ERR_BAD_ARG;
  }
  const int eos = eos_id >= 0 ? 1 : 0;
  const long tiles = ((long)Lp + eos + NS_TILE - 1) / NS_TILE;
  if (tiles == 0) {  // nothing is scored anywhere: the sums alone
    hipLaunchKernelGGL(ngram_seq_sum_kernel, dim3(N), dim3(NS_TILE), 0, (hipStream_t)stream, ylens, Lp, eos, logp_tok, logp);
    EM_CHECK_LAUNCH();
    return EM_OK;
  }
  if ((long)N * tiles > 0x7fffffffL) return EM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ngram_seq_kernel, dim3((unsigned)(N * tiles)), dim3(NS_TILE), 0, (hipStream_t)stream, *m, ids, ylens, Lp,
                     (int)tiles, eos_id, logp_tok, order_tok, tiles == 1 ? logp : nullptr);
  EM_CHECK_LAUNCH();
  if (tiles > 1) {
    hipLaunchKernelGGL(ngram_seq_sum_kernel, dim3(N), dim3(NS_TILE), 0, (hipStream_t)stream, ylens, Lp, eos, logp_tok, logp);
    EM_CHECK_LAUNCH();
  }
  return EM_OK;
}
