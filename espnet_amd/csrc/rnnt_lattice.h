// The transducer (RNN-T) lattice as the likelihood (transducer_nll.hip, sum-product) and the forced alignment
// (transducer_align.hip, Viterbi) see it: the caps, which nodes of a ragged batch exist, and the forward walk over them.
//
// lat [N][T][Lmax + 1][2] (em_transducer_lattice_logp) holds the blank's and the label's log-probability of node (t, u)
// of candidate n, which belongs to utterance m = mem_of[n] (n itself without mem_of) and has the nodes t < Tb = xlens[m],
// u <= U = ylens[n] - all three as `clamp` returns them, to the launch that fills the lattice and to the two that read it.
//
// Layout of the work.  One workgroup per candidate, thread u owns column u and the anti-diagonals d = t + u pass in
// sequence: cell (t, u) takes b[t-1][u] over its own value and e[t][u-1] over thread u - 1's of diagonal d - 1 (a missing
// neighbour is -inf), which crosses through a double-buffered LDS row with ONE barrier per diagonal; the two
// log-probabilities of diagonal d + 1 are loaded before the chain of diagonal d.  The recursions differ in the cell only:
//   float node(int t, float stay, float emit)   the value of node (t, u) from stay = v[t-1][u] + b[t-1][u] and emit =
//                                               v[t][u-1] + e[t][u-1]; once per node of the column, frames in order,
//                                               node (0, 0) too (both terms -inf): the walk puts 0 in its place.
#pragma once
#include "em_common.h"

namespace rnnt_lattice {

constexpr int MAX_L = 1023;           // one thread per lattice column u <= Lmax: 1 024 threads
constexpr long MAX_NODES = 1L << 28;  // N * T * (Lmax + 1): node numbers stay inside 31 bits, lat inside 2 GiB

static inline bool shape_ok(int N, int T, int Lmax) {
  return N > 0 && T > 0 && Lmax >= 0 && Lmax <= MAX_L && (long)N * T * (Lmax + 1) <= MAX_NODES;
}

struct Cand {  // candidate n: its utterance, the extent of its lattice and the number of its nodes
  int m, Tb, U;
  __device__ __forceinline__ int nodes() const { return Tb * (U + 1); }
};
__device__ __forceinline__ Cand clamp(const int32_t* xlens, const int32_t* ylens, const int32_t* mem_of, int Bm, int T,
                                      int Lmax, int n) {
  const int m = mem_of ? min(max(mem_of[n], 0), Bm - 1) : n;
  return Cand{m, min(max(xlens[m], 0), T), min(max(ylens[n], 0), Lmax)};
}

// The forward pass over the Tb x (U + 1) nodes at `base` (row stride Lmax + 1 nodes), Tb >= 1, by blockDim.x > U threads;
// `row` is the kernel's LDS.  Returns the thread's last value: thread U holds node (Tb - 1, U)'s.  Ends behind a barrier.
template <class Cell>
__device__ __forceinline__ float walk(const float* base, int Lmax, int Tb, int U, float (*row)[MAX_L + 1], Cell cell) {
  const int u = threadIdx.x;
  const size_t ld = (size_t)(Lmax + 1) * 2;
  const bool mine = u <= U;
  // the terms that cell (t, u) adds: b[t-1][u] (t >= 1) and e[t][u-1] (u >= 1); a missing neighbour is -inf
  auto load_b = [&](int t) { return mine && t >= 1 && t < Tb ? base[(size_t)(t - 1) * ld + 2 * u] : -INFINITY; };
  auto load_e = [&](int t) { return mine && u >= 1 && t >= 0 && t < Tb ? base[(size_t)t * ld + 2 * (u - 1) + 1] : -INFINITY; };
  float v = -INFINITY;  // v[d - 1 - u][u] while diagonal d runs
  float nb = load_b(0 - u), ne = load_e(0 - u);
  for (int d = 0; d < Tb + U; ++d) {
    const int t = d - u;
    const float b = nb, e = ne;
    nb = load_b(t + 1), ne = load_e(t + 1);  // diagonal d + 1, in flight during this diagonal's chain
    const float left = u >= 1 ? row[(d + 1) & 1][u - 1] : -INFINITY;  // v[t][u-1], written on diagonal d - 1
    const bool on = mine && t >= 0 && t < Tb;
    if (on) v = cell.node(t, v + b, left + e);
    if (on && d == 0) v = 0.f;  // the seed, node (0, 0)
    row[d & 1][u] = on ? v : -INFINITY;
    __syncthreads();
  }
  return v;
}

}  // namespace rnnt_lattice
