// The forward walk over the CTC trellis that the forced alignment (ctc_align.hip, Viterbi) and the likelihood
// (ctc_nll.hip, sum-product) share: who owns which states, where the emissions come from, how neighbours exchange
// alpha, and how the last two states are collected.  The two differ in the cell only, which a policy supplies.
//
// Layout of the work.  One workgroup per trellis, the Tb frames in sequence, the S = 2 L + 1 states spread over the
// lanes: thread i owns the 8 states 8 i .. 8 i + 7 in registers, that is four blanks and the four tokens
// y[4 i .. 4 i + 3].  Of its neighbours a thread needs only alpha[8 i - 1] (state 8 i is a blank: stay or one; state
// 8 i + 1 skips from 8 i - 1), which is one lane shift (DPP wave_shr:1) per frame and, across waves, one LDS word and
// one barrier per frame.  S <= 512 runs as ONE wave64 with no workgroup barrier anywhere; longer transcripts run as
// ceil(S / 512) <= 16 waves, so the largest transcript taken is L = MAX_L = 4 095 tokens.
//
// Emissions come straight from lpT [V][ldT] (em_ctc_log_probs_t): a token's row is frame-contiguous, so one 16-byte
// load brings four frames of it; every lane loads the same four frames of the blank row (one request per wave).  The
// loads of frame group k + 1 are issued before the chain of group k, so the per-frame chain is the cells and the
// shift.  (Rows whose stride or base is not 16-byte aligned take 4-byte loads, same values.)
//
// A cell policy has
//   static f32x4 prepare(f32x4 e)                                   what is done to four loaded emissions;
//   float blank(int j, float stay, float one, float e)              alpha[t] of the blank state j (even) of this thread;
//   float token(int j, float stay, float one, float two, float e)   ... of the token state j (odd); `two` is already
//                                                                   -inf where the move by two states is not allowed;
//   void frame(int t)                                               once per thread and frame t >= 1, behind its 8 cells.
#pragma once
#include "em_common.h"

namespace ctc_trellis {

constexpr int SPL = 8;                                  // states per lane
constexpr int MAX_WAVES = 16;                           // 1 024 threads
constexpr int MAX_L = (MAX_WAVES * 64 * SPL - 1) / 2;   // 4 095 tokens (S = 8 191 <= 8 192)
constexpr float NINF = -INFINITY;

static inline int waves(int Lmax) { return em_cdiv(2 * Lmax + 1, 64 * SPL); }

// four consecutive columns c0 .. c0 + 3 of one lpT row
__device__ __forceinline__ f32x4 load4(const float* row, long c0, bool vec, long ldT) {
  if (vec) return *(const f32x4*)(row + c0);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = c0 + i < ldT ? row[c0 + i] : 0.f;
  return r;
}

template <bool MULTI>
__device__ __forceinline__ void group_sync() {
  if (MULTI) {
    __syncthreads();
  } else {  // one wave: LDS and global traffic of its own lanes, ordered without a barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

// alpha over the frames 0 .. Tb - 1 of the columns colb .. of lpT for the transcript y[0 .. L).  xch and fin are the
// kernel's LDS; behind the call every thread may read fin[0] = alpha[Tb - 1][S - 1] and fin[1] = alpha[Tb - 1][S - 2]
// (-inf: no such state, or Tb == 0).
template <bool MULTI, class Cell>
__device__ __forceinline__ void forward(const float* lpT, long ldT, long colb, bool vec, const int32_t* y, int L, int Tb,
                                        int blank, float (*xch)[MAX_WAVES], float* fin, Cell& cell) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = 2 * L + 1;

  if (tid < 2) fin[tid] = NINF;
  group_sync<MULTI>();

  float al[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) al[j] = NINF;
  if (Tb > 0) {
    const float* rows[4];
    float cap[4];  // +inf where the move by two states is allowed, -inf where not
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * tid + q;
      const int lab = i < L ? y[i] : blank;
      rows[q] = lpT + (size_t)lab * ldT;
      cap[q] = (i >= 1 && i < L && y[i - 1] != lab) ? INFINITY : NINF;
    }
    const float* rowb = lpT + (size_t)blank * ldT;
    const long col0 = vec ? (colb & ~3L) : colb;
    const int off = (int)(colb - col0);
    const int NG = (off + Tb + 3) >> 2;

    f32x4 cur[5], nxt[5];
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = Cell::prepare(load4(rows[q], col0, vec, ldT));
    cur[4] = Cell::prepare(load4(rowb, col0, vec, ldT));
#pragma unroll
    for (int q = 0; q < 5; ++q) nxt[q] = cur[q];
    for (int k = 0; k < NG; ++k) {
      if (k + 1 < NG) {
        const long c = col0 + 4L * (k + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q] = Cell::prepare(load4(rows[q], c, vec, ldT));
        nxt[4] = Cell::prepare(load4(rowb, c, vec, ldT));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = 4 * k + i - off;
        if (t < 0 || t >= Tb) continue;  // the same in every thread of the workgroup
        const float eb = cur[4][i];
        if (t == 0) {
          if (tid == 0) {
            al[0] = eb;
            if (L > 0) al[1] = cur[0][i];
          }
        } else {
          // alpha[t-1] of the state below this thread's run
          float p7 = __builtin_bit_cast(
              float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, NINF), __builtin_bit_cast(int, al[7]), 0x138,
                                                 0xf, 0xf, false));  // wave_shr:1; lane 0 keeps -inf
          if (MULTI) {
            if (lane == 0 && wave > 0) p7 = xch[(t - 1) & 1][wave - 1];
          }
          float nw[SPL];
#pragma unroll
          for (int j = 0; j < SPL; ++j) {
            const float one = j == 0 ? p7 : al[j - 1];
            if (j & 1) {
              const float two = fminf(j == 1 ? p7 : al[j - 2], cap[j >> 1]);
              nw[j] = cell.token(j, al[j], one, two, cur[j >> 1][i]);
            } else {
              nw[j] = cell.blank(j, al[j], one, eb);
            }
          }
#pragma unroll
          for (int j = 0; j < SPL; ++j) al[j] = nw[j];
          cell.frame(t);
        }
        if (MULTI) {
          if (lane == 63) xch[t & 1][wave] = al[7];
          __syncthreads();
        }
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) cur[q] = nxt[q];
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      const int s = SPL * tid + j;
      if (s == S - 1) fin[0] = al[j];
      if (s == S - 2) fin[1] = al[j];
    }
  }
  group_sync<MULTI>();
}

}  // namespace ctc_trellis
