// The sorted-trie lookups of the back-off n-gram (EmNgramModel), shared by the label-synchronous scorer (csrc/ngram.hip)
// and the time-synchronous CTC search (csrc/ctc_tsync.hip).  Two forms of every lookup: by a whole wave (64 probes per round)
// and by one lane (a binary search) - the same entry found, the same f32 additions in the same order.
#pragma once
#include "em_common.h"

namespace {

constexpr int NG_MAX = EM_NGRAM_MAX_ORDER;

__host__ __device__ inline int ng_ld(const EmNgramModel& m) { return m.order > 1 ? m.order - 1 : 1; }

// word id of a token (a token id outside [0, V) reads as <unk>)
__device__ __forceinline__ int tok_word(const EmNgramModel& m, int t) { return (unsigned)t < (unsigned)m.vocab ? m.tok2word[t] : m.unk; }

// index of word w in the sorted range a[lo, hi), or -1; wave-uniform arguments, every lane gets the answer
__device__ __forceinline__ int wave_find(const int32_t* __restrict__ a, int lo, int hi, int w, int lane) {
  while (hi - lo > 64) {
    const long len = hi - lo;
    const int pos = lo + (int)(((long)(lane + 1) * len) / 65);  // 64 strictly increasing probes inside [lo, hi)
    const unsigned long long le = __ballot(a[pos] <= w);
    const int c = __popcll(le);  // a prefix of the lanes: w lies in [probe c-1, probe c)
    const int nlo = c > 0 ? lo + (int)(((long)c * len) / 65) : lo;
    const int nhi = c < 64 ? lo + (int)(((long)(c + 1) * len) / 65) : hi;
    lo = nlo;
    hi = nhi;
  }
  const int i = lo + lane;
  const unsigned long long hit = __ballot(i < hi && a[i] == w);
  return hit ? lo + __ffsll((long long)hit) - 1 : -1;
}

// node of context length k+1 after appending word w to a history whose nodes are prev[0 .. N-2] (start: <s> alone)
__device__ __forceinline__ int advance_one(const EmNgramModel& m, int k, bool start, const int32_t* prev, int w, int lane) {
  if (start) return k == 0 ? m.bos : -1;
  if (k == 0) return w;
  if (!prev) return -1;
  const int pn = prev[k - 1];
  if (pn < 0) return -1;
  const int lo = m.next[k - 1][pn], hi = m.next[k - 1][pn + 1];
  return hi > lo ? wave_find(m.wid[k], lo, hi, w, lane) : -1;
}

// log10 score of word w after the history with context nodes `node` [N-1] (LDS), by one wave
__device__ __forceinline__ float wave_score(const EmNgramModel& m, const int32_t* node, int w, int lane) {
  float p = m.prob[0][w];
  int js = 0;
  for (int L = 1; L < m.order; ++L) {
    const int nd = node[L - 1];
    if (nd < 0) continue;
    const int lo = m.next[L - 1][nd], hi = m.next[L - 1][nd + 1];
    if (hi <= lo) continue;
    const int f = wave_find(m.wid[L], lo, hi, w, lane);
    if (f >= 0) {
      p = m.prob[L][f];
      js = L;
    }
  }
  float acc = p;
  for (int L = js + 1; L < m.order; ++L)
    if (node[L - 1] >= 0) acc += m.bow[L - 1][node[L - 1]];
  return acc;
}

// ---- the same lookups by ONE lane (each lane of a wave its own hypothesis and word)
// index of word w in the sorted range a[lo, hi), or -1; at most 32 halvings
__device__ __forceinline__ int lane_find(const int32_t* __restrict__ a, int lo, int hi, int w) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    const int v = a[mid];
    if (v == w) return mid;
    if (v < w) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// advance_one by one lane (never the start: the caller sets <s> itself)
__device__ __forceinline__ int lane_advance_one(const EmNgramModel& m, int k, const int32_t* prev, int w) {
  if (k == 0) return w;
  const int pn = prev[k - 1];
  if (pn < 0) return -1;
  const int lo = m.next[k - 1][pn], hi = m.next[k - 1][pn + 1];
  return hi > lo ? lane_find(m.wid[k], lo, hi, w) : -1;
}

// wave_score by one lane
__device__ __forceinline__ float lane_score(const EmNgramModel& m, const int32_t* node, int w) {
  float p = m.prob[0][w];
  int js = 0;
  for (int L = 1; L < m.order; ++L) {
    const int nd = node[L - 1];
    if (nd < 0) continue;
    const int lo = m.next[L - 1][nd], hi = m.next[L - 1][nd + 1];
    if (hi <= lo) continue;
    const int f = lane_find(m.wid[L], lo, hi, w);
    if (f >= 0) {
      p = m.prob[L][f];
      js = L;
    }
  }
  float acc = p;
  for (int L = js + 1; L < m.order; ++L)
    if (node[L - 1] >= 0) acc += m.bow[L - 1][node[L - 1]];
  return acc;
}

}  // namespace
