// espnet_amd — transducer (RNN-T) forced alignment on gfx950: the best (max-product) path of a given transcript through
// the lattice that em_transducer_lattice_logp wrote, with its back-trace, for a ragged batch of candidates in one launch
// (contract: include/espnet_amd.h, "transducer forced alignment").  It is the Viterbi twin of seq_nll_kernel
// (csrc/transducer_nll.hip), as csrc/ctc_align.hip is of the CTC forward recursion.
//
//   seq_align_kernel   a workgroup per candidate: csrc/rnnt_lattice.h's walk with the Viterbi cell, back-trace, outputs.
//
// Back-pointers are one bit per node, set when the label move (from (t, u-1)) is strictly better than the blank move
// (from (t-1, u)).  The store is u-major, bp[n][u][t / 32]: thread u meets the frames of its column in order, one per
// diagonal, so it gathers 32 of them in a register and flushes the word with one plain store at t % 32 == 31 and at
// t == T_b - 1.  A word has one writer, is written whole (the bits of frames >= T_b are zero) and exactly once; the
// words (u <= U, t / 32 <= (T_b - 1) / 32) are all the back-trace can read, so nothing depends on what the workspace
// held on entry.
//
// The back-trace runs in the same launch on thread 0: inside column u the path came over blank moves from the highest
// set bit at or below the current frame, a masked find-last-set per 32-frame word - at most U + T_b / 32 dependent
// loads, not T_b + U.  It leaves the frame of every token in LDS; all threads then write the outputs: thread u its
// token's frame and log-probability, frame_u[t] = the number of tokens whose frame is <= t by a binary search.
#include <math.h>

#include "em_common.h"
#include "rnnt_lattice.h"

namespace {

struct AlignArgs {
  const float* lat;
  const int32_t *xlens, *ylens, *mem_of;
  int32_t Bm, T, Lmax;
  int32_t *tok_frame, *frame_u;
  float *tok_logp, *total;
  uint32_t* bp;  // [N][Lmax + 1][(T + 31) / 32] back-pointer words
};

struct ViterbiCell {  // the max-product cell of rnnt_lattice::walk, with the back-pointer store described above
  uint32_t* col;  // bp[n][u]
  int last;       // Tb - 1
  uint32_t word;  // the bits of the frames 32 * (t / 32) .. t
  __device__ __forceinline__ float node(int t, float stay, float emit) {
    const bool label = emit > stay;  // the tie rule: equal values keep the blank move
    word |= (uint32_t)label << (t & 31);
    if ((t & 31) == 31 || t == last) {
      col[t >> 5] = word;
      word = 0;
    }
    return label ? emit : stay;
  }
};

__global__ __launch_bounds__(1024) void seq_align_kernel(const AlignArgs a) {
  __shared__ float row[2][rnnt_lattice::MAX_L + 1];
  __shared__ int32_t tf[rnnt_lattice::MAX_L + 1];  // the frame of token u, found by the back-trace
  __shared__ float s_total;
  __shared__ int s_ok;
  const int n = blockIdx.x, u = threadIdx.x, NT = blockDim.x;
  const int T = a.T, Lmax = a.Lmax;
  const rnnt_lattice::Cand cand = rnnt_lattice::clamp(a.xlens, a.ylens, a.mem_of, a.Bm, T, Lmax, n);
  const int Tb = cand.Tb, U = cand.U;
  int32_t* tok_frame = a.tok_frame + (size_t)n * Lmax;
  float* tok_logp = a.tok_logp + (size_t)n * Lmax;
  int32_t* frame_u = a.frame_u + (size_t)n * T;
  // no frame, no path: the whole row reads as padding
  auto no_path = [&]() {
    for (int i = u; i < Lmax; i += NT) {
      tok_frame[i] = -1;
      tok_logp[i] = 0.f;
    }
    for (int t = u; t < T; t += NT) frame_u[t] = -1;
    if (u == 0) a.total[n] = -INFINITY;
  };
  if (Tb == 0) {  // (workgroup-uniform)
    no_path();
    return;
  }
  const size_t ld = (size_t)(Lmax + 1) * 2;
  const float* base = a.lat + (size_t)n * T * ld;
  const int W = (T + 31) >> 5;
  uint32_t* bpn = a.bp + (size_t)n * (Lmax + 1) * W;
  const float v = rnnt_lattice::walk(base, Lmax, Tb, U, row, ViterbiCell{bpn + (size_t)u * W, Tb - 1, 0});
  if (u == U) s_total = v + base[(size_t)(Tb - 1) * ld + 2 * U];  // the closing blank
  __syncthreads();  // (and the back-pointer words of every column are visible to the workgroup)
  const float tot = s_total;
  if (!(tot > -INFINITY)) {  // (workgroup-uniform) no path of finite value
    no_path();
    return;
  }
  if (u == 0) {
    int t = Tb - 1, ok = 1;
    for (int k = U; k >= 1; --k) {
      const uint32_t* c = bpn + (size_t)k * W;
      int w = t >> 5;
      uint32_t x = c[w] & (0xffffffffu >> (31 - (t & 31)));
      while (x == 0 && w > 0) x = c[--w];
      if (x == 0) {  // (a finite path enters every column k >= 1 by a label move; kept as a bound on the walk)
        ok = 0;
        break;
      }
      t = (w << 5) + 31 - __clz(x);
      tf[k - 1] = t;
    }
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) {  // (workgroup-uniform)
    no_path();
    return;
  }
  for (int i = u; i < Lmax; i += NT) {
    const bool tok = i < U;
    tok_frame[i] = tok ? tf[i] : -1;
    tok_logp[i] = tok ? base[(size_t)tf[i] * ld + 2 * i + 1] : 0.f;
  }
  for (int t = u; t < T; t += NT) {
    int lo = 0;
    if (t < Tb) {  // the number of tokens with tf <= t (tf is non-decreasing)
      int hi = U;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tf[mid] <= t) lo = mid + 1; else hi = mid;
      }
    }
    frame_u[t] = t < Tb ? lo : -1;
  }
  if (u == 0) a.total[n] = tot;
}

}  // namespace

extern "C" size_t em_transducer_seq_align_workspace_bytes(int32_t N, int32_t T, int32_t Lmax) {
  if (!rnnt_lattice::shape_ok(N, T, Lmax)) return 0;
  const size_t words = (size_t)N * (Lmax + 1) * ((T + 31) / 32);
  return (words * sizeof(uint32_t) + 255) & ~(size_t)255;
}

extern "C" int em_transducer_seq_align(const float* lat, const int32_t* xlens, int32_t Bm, int32_t T, int32_t Lmax,
                                       const int32_t* ylens, const int32_t* mem_of, int32_t N, int32_t* tok_frame,
                                       float* tok_logp, int32_t* frame_u, float* total, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (!lat || !xlens || !ylens || !frame_u || !total || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0) return EM_ERR_BAD_ARG;
  if (Lmax > 0 && (!tok_frame || !tok_logp)) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if (!rnnt_lattice::shape_ok(N, T, Lmax)) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < em_transducer_seq_align_workspace_bytes(N, T, Lmax)) return EM_ERR_WORKSPACE;
  const AlignArgs a{lat, xlens, ylens, mem_of, Bm, T, Lmax, tok_frame, frame_u, tok_logp, total, (uint32_t*)ws};
  hipLaunchKernelGGL(seq_align_kernel, dim3(N), dim3(64 * em_cdiv(Lmax + 1, 64)), 0, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
