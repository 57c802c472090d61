// CTC likelihood of given transcripts: the forward (sum-product) trellis of CTC through the CTC log-posteriors, for a
// ragged batch of candidate transcripts in one launch.  Reference: CTC.forward with reduce=False under the builtin
// ctc_loss, espnet2/asr/ctc.py (torch.nn.functional.ctc_loss, reduction "none"); the contract (states, recursion, what an
// impossible transcript gives) is include/espnet_amd.h's.
//
// Layout of the work: the forced alignment's (csrc/ctc_align.hip).  One workgroup per candidate, the T_b frames of its
// utterance in sequence, the S = 2 L + 1 states spread over the lanes: thread i owns the 8 states 8 i .. 8 i + 7 in
// registers (four blanks and the tokens y[4 i .. 4 i + 3]) and needs of its neighbour only alpha[8 i - 1], one lane shift
// (DPP wave_shr:1) per frame and, across waves, one LDS word and one barrier per frame.  S <= 512 runs as ONE wave64
// with no workgroup barrier; longer transcripts as ceil(S / 512) <= 16 waves (L <= 4 095).  Emissions come from the
// token's frame-contiguous lpT row four frames per 16-byte load, the loads of frame group k + 1 issued before the chain
// of group k.  Several candidates may read one utterance's columns (mem_of): nothing is written but nll[n], so there
// is no back-pointer tier, no workspace and no back-trace.
//
// The chain per cell.  The trellis is kept in the base-2 logarithm: an emission is multiplied by log2(e) once when it is
// loaded (one rounded f32 product, 5 per frame and lane), and a cell is
//     hi = max3, lo = min3, mid = med3 of its (up to) three predecessors,
//     alpha = hi + log2(1 + 2^(mid - hi) + 2^(lo - hi)) + emission
// - the largest term is an exact 1, so a token state costs two v_exp_f32 and one v_log_f32 (a blank state one and one)
// where exp / log of the natural form cost a multiplication more each and one more exponential.  The subtrahend is hi
// clamped to -FLT_MAX, so predecessors that are all -inf give 2^(-inf) = 0, log2(1) = 0 and alpha = -inf + 0 + emission
// = -inf: no NaN anywhere.  nll = -ln(2) * log2-sum of the last two states, +inf when no path reaches them.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (ROCm 7.2):
//   ctc_nll_kernel<false> (one wave)  : 81 VGPRs, 56 SGPRs, 0 bytes of scratch, no spills, 8 B of LDS, no s_barrier
//   ctc_nll_kernel<true>  (2-16 waves): 74 VGPRs, 60 SGPRs, 0 bytes of scratch, no spills, 136 B of LDS
#include <cfloat>

#include "em_common.h"

namespace {

constexpr int CN_SPL = 8;                                        // states per lane
constexpr int CN_MAX_WAVES = 16;                                 // 1 024 threads
constexpr int CN_MAX_L = (CN_MAX_WAVES * 64 * CN_SPL - 1) / 2;   // 4 095 tokens, em_ctc_forced_align_max_tokens()
constexpr float CN_LOG2E = 1.44269504088896340736f;
constexpr float CN_LN2 = 0.69314718055994530942f;
constexpr float NINF = -INFINITY;

struct NllArgs {
  const float* lpT;
  const int32_t *xlens, *targets, *ylens, *mem_of;
  int32_t ldT, Lmax, T, Bm, blank, vec;
  float* nll;
};

static inline int cn_waves(int Lmax) { return em_cdiv(2 * Lmax + 1, 64 * CN_SPL); }

// four consecutive columns c0 .. c0 + 3 of one lpT row, times log2(e) (__fmul_rn: never contracted into a later add, so
// both kernel forms and both load forms round alike)
__device__ __forceinline__ f32x4 load4s(const float* row, long c0, bool vec, long ldT) {
  f32x4 r;
  if (vec) {
    r = *(const f32x4*)(row + c0);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = c0 + i < ldT ? row[c0 + i] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __fmul_rn(r[i], CN_LOG2E);
  return r;
}

// log2(2^a + 2^b) and log2(2^a + 2^b + 2^c); -inf terms (all of them too) give -inf, never NaN
__device__ __forceinline__ float lse2(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  const float s = 1.f + __builtin_amdgcn_exp2f(lo - fmaxf(hi, -FLT_MAX));
  return hi + __builtin_amdgcn_logf(s);
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float hi = __builtin_fmaxf(__builtin_fmaxf(a, b), c), lo = __builtin_fminf(__builtin_fminf(a, b), c);
  const float mid = __builtin_amdgcn_fmed3f(a, b, c);
  const float sh = fmaxf(hi, -FLT_MAX);
  const float s = (1.f + __builtin_amdgcn_exp2f(mid - sh)) + __builtin_amdgcn_exp2f(lo - sh);
  return hi + __builtin_amdgcn_logf(s);
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_nll_kernel(const NllArgs a) {
  __shared__ float xch[2][CN_MAX_WAVES];
  __shared__ float fin[2];

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, blank = a.blank, Lmax = a.Lmax;
  const int u = a.mem_of ? min(max(a.mem_of[n], 0), a.Bm - 1) : n;
  const int Tb = min(max(a.xlens[u], 0), T);
  const int L = min(max(a.ylens[n], 0), Lmax);
  const int S = 2 * L + 1;
  const int32_t* y = a.targets + (size_t)n * Lmax;
  const long ldT = a.ldT, colb = (long)u * T;

  if (tid < 2) fin[tid] = NINF;
  if (MULTI) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }

  float al[CN_SPL];
#pragma unroll
  for (int j = 0; j < CN_SPL; ++j) al[j] = NINF;
  if (Tb > 0) {
    const float* rows[4];
    float cap[4];  // +inf where the move by two states is allowed, -inf where not
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * tid + q;
      const int lab = i < L ? y[i] : blank;
      rows[q] = a.lpT + (size_t)lab * ldT;
      cap[q] = (i >= 1 && i < L && y[i - 1] != lab) ? INFINITY : NINF;
    }
    const float* rowb = a.lpT + (size_t)blank * ldT;
    const bool vec = a.vec != 0;
    const long col0 = vec ? (colb & ~3L) : colb;
    const int off = (int)(colb - col0);
    const int NG = (off + Tb + 3) >> 2;

    f32x4 cur[5], nxt[5];
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = load4s(rows[q], col0, vec, ldT);
    cur[4] = load4s(rowb, col0, vec, ldT);
#pragma unroll
    for (int q = 0; q < 5; ++q) nxt[q] = cur[q];
    for (int k = 0; k < NG; ++k) {
      if (k + 1 < NG) {
        const long c = col0 + 4L * (k + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q] = load4s(rows[q], c, vec, ldT);
        nxt[4] = load4s(rowb, c, vec, ldT);
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
          float nw[CN_SPL];
#pragma unroll
          for (int j = 0; j < CN_SPL; ++j) {
            const float one = j == 0 ? p7 : al[j - 1];
            if (j & 1) {
              const float two = fminf(j == 1 ? p7 : al[j - 2], cap[j >> 1]);
              nw[j] = lse3(al[j], one, two) + cur[j >> 1][i];
            } else {
              nw[j] = lse2(al[j], one) + eb;
            }
          }
#pragma unroll
          for (int j = 0; j < CN_SPL; ++j) al[j] = nw[j];
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
    for (int j = 0; j < CN_SPL; ++j) {
      const int s = CN_SPL * tid + j;
      if (s == S - 1) fin[0] = al[j];
      if (s == S - 2) fin[1] = al[j];
    }
  }
  if (MULTI) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  if (tid == 0) {
    const float tot = lse2(fin[0], fin[1]);  // (L == 0: fin[1] is -inf and the sum is alpha[0] exactly)
    a.nll[n] = tot > NINF ? -__fmul_rn(tot, CN_LN2) : INFINITY;
  }
}

}  // namespace

extern "C" int em_ctc_seq_nll(const float* lpT, int32_t ldT, const int32_t* xlens, int32_t Bm, int32_t T,
                              const int32_t* targets, int32_t Lmax, const int32_t* ylens, const int32_t* mem_of, int32_t N,
                              int32_t blank, float* nll, void* stream) {
  if (!lpT || !xlens || !ylens || !nll || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0 || blank < 0) return EM_ERR_BAD_ARG;
  if (Lmax > 0 && !targets) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if ((long)ldT < (long)Bm * T) return EM_ERR_BAD_ARG;
  if (Lmax > CN_MAX_L) return EM_ERR_UNSUPPORTED;
  const int nw = cn_waves(Lmax);
  NllArgs a;
  a.lpT = lpT; a.xlens = xlens; a.targets = targets; a.ylens = ylens; a.mem_of = mem_of;
  a.ldT = ldT; a.Lmax = Lmax; a.T = T; a.Bm = Bm; a.blank = blank;
  a.vec = (ldT % 4 == 0) && (((uintptr_t)lpT & 15) == 0);
  a.nll = nll;
  if (nw == 1)
    hipLaunchKernelGGL(ctc_nll_kernel<false>, dim3(N), dim3(64), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ctc_nll_kernel<true>, dim3(N), dim3(64 * nw), 0, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
