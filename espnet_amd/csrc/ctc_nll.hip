// CTC likelihood of given transcripts: the forward (sum-product) trellis of CTC through the CTC log-posteriors, for a
// ragged batch of candidate transcripts in one launch.  Reference: CTC.forward with reduce=False under the builtin
// ctc_loss, espnet2/asr/ctc.py (torch.nn.functional.ctc_loss, reduction "none"); the contract (states, recursion, what an
// impossible transcript gives) is include/espnet_amd.h's.
//
// Layout of the work: the shared trellis walk of ctc_trellis.h, which the forced alignment (ctc_align.hip) runs too -
// one workgroup per candidate, the T_b frames of its utterance in sequence, 8 states per lane, one wave up to S = 512
// and up to 16 waves beyond (L <= 4 095).  Several candidates may read one utterance's columns (mem_of): nothing is
// written but nll[n], so there is no back-pointer tier, no workspace and no back-trace.
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
//   ctc_nll_kernel<false> (one wave)  : 72 VGPRs, 54 SGPRs, 0 bytes of scratch, no spills, 8 B of LDS, no s_barrier
//   ctc_nll_kernel<true>  (2-16 waves): 76 VGPRs, 58 SGPRs, 0 bytes of scratch, no spills, 136 B of LDS
#include <cfloat>

#include "ctc_trellis.h"

namespace {

using ctc_trellis::NINF;
constexpr float CN_LOG2E = 1.44269504088896340736f;
constexpr float CN_LN2 = 0.69314718055994530942f;

struct NllArgs {
  const float* lpT;
  const int32_t *xlens, *targets, *ylens, *mem_of;
  int32_t ldT, Lmax, T, Bm, blank, vec;
  float* nll;
};

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

// the sum-product cell in the base-2 logarithm; nothing is kept per frame
struct SumCell {
  // times log2(e) (__fmul_rn: never contracted into a later add, so both kernel forms and both load forms round alike)
  static __device__ __forceinline__ f32x4 prepare(f32x4 e) {
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = __fmul_rn(e[i], CN_LOG2E);
    return e;
  }
  __device__ __forceinline__ float blank(int, float stay, float one, float e) { return lse2(stay, one) + e; }
  __device__ __forceinline__ float token(int, float stay, float one, float two, float e) {
    return lse3(stay, one, two) + e;
  }
  __device__ __forceinline__ void frame(int) {}
};

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_nll_kernel(const NllArgs a) {
  __shared__ float xch[2][ctc_trellis::MAX_WAVES];
  __shared__ float fin[2];

  const int n = blockIdx.x, T = a.T, Lmax = a.Lmax;
  const int u = a.mem_of ? min(max(a.mem_of[n], 0), a.Bm - 1) : n;
  const int Tb = min(max(a.xlens[u], 0), T);
  const int L = min(max(a.ylens[n], 0), Lmax);

  SumCell cell;
  ctc_trellis::forward<MULTI>(a.lpT, a.ldT, (long)u * T, a.vec != 0, a.targets + (size_t)n * Lmax, L, Tb, a.blank, xch, fin,
                              cell);
  if (threadIdx.x == 0) {
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
  if (Lmax > ctc_trellis::MAX_L) return EM_ERR_UNSUPPORTED;  // em_ctc_forced_align_max_tokens()
  const int nw = ctc_trellis::waves(Lmax);
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
