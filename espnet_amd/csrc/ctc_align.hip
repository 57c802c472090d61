// CTC forced alignment: the Viterbi path of a given transcript through the CTC log-posteriors, for a ragged batch in
// one launch.  Reference: CTC.forced_align, espnet2/asr/ctc.py (a wrapper of torchaudio.functional.forced_align, one
// utterance per call on the CPU); the contract (states, recursion, tie rule, outputs) is include/espnet_amd.h's.
//
// Layout of the work.  One workgroup per utterance, the T frames in sequence, the S = 2 L + 1 trellis states spread
// over the lanes: thread i owns the 8 states 8 i .. 8 i + 7 in registers, that is four blanks and the four tokens
// y[4 i .. 4 i + 3].  Of its neighbours a thread needs only alpha[8 i - 1] (state 8 i is a blank: stay or one; state
// 8 i + 1 skips from 8 i - 1), which is one lane shift (DPP wave_shr:1) per frame and, across waves, one LDS word and
// one barrier per frame.  S <= 512 runs as ONE wave64 with no workgroup barrier anywhere; longer transcripts run as
// ceil(S / 512) <= 16 waves, so the largest transcript taken is L = CA_MAX_L = 4 095 tokens.
//
// Emissions come straight from lpT [V][ldT] (em_ctc_log_probs_t): a token's row is frame-contiguous, so one 16-byte
// load brings four frames of it; every lane loads the same four frames of the blank row (one request per wave).  The
// loads of frame group k + 1 are issued before the chain of group k, so the per-frame chain is compare / select / add
// and the shift.  (Rows whose stride or base is not 16-byte aligned take 4-byte loads, same values.)
//
// Back-pointers are 2 bits per (t, s): the 8 of a thread in one 16-bit store per frame, to LDS when T * threads * 2
// bytes fit CA_LDS_BP_BYTES (T = 249, one wave: 31.9 KB), else to the caller's workspace.  The back-trace walks
// CA_CH frames at a time: at frame t - k the path lies in [s - 2 k, s], so the chunk's window of the workspace (at most
// CA_WIN 16-bit words per frame) is first copied to LDS by all threads, one thread walks it, then all threads turn
// the chunk's path into align / frame_lp / span boundaries in parallel.  tok_lp sums each token's own (frame-
// contiguous) row over its span, one thread per token: a span of n frames is n dependent adds behind cached loads of
// one row, the order the contract fixes; a token that lasts thousands of frames (long form) is accepted as that.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (ROCm 7.2):
//   ctc_align_kernel<false> (one wave)  : 84 VGPRs, 101 SGPRs, 0 bytes of scratch, no spills, 8 976 B of LDS, no s_barrier
//   ctc_align_kernel<true>  (2-16 waves): 86 VGPRs, 105 SGPRs, 0 bytes of scratch, no spills, 9 104 B of LDS
// (LDS: the static part; the one-wave form adds T * 128 bytes of back-pointers, 31.9 KB at T = 249.)
#include "em_common.h"

namespace {

constexpr int CA_SPL = 8;                                        // states per lane
constexpr int CA_MAX_WAVES = 16;                                 // 1 024 threads
constexpr int CA_MAX_L = (CA_MAX_WAVES * 64 * CA_SPL - 1) / 2;   // 4 095 tokens (S = 8 191 <= 8 192)
constexpr int CA_LDS_BP_BYTES = 48 * 1024;                       // back-pointers kept in LDS up to this size
constexpr int CA_CH = 128;                                       // frames per back-trace chunk
constexpr int CA_WIN = 2 * CA_CH / CA_SPL + 2;                   // 16-bit words per frame that a chunk's window can span

struct AlignArgs {
  const float* lpT;
  const int32_t *xlens, *targets, *ylens;
  int32_t ldT, Lmax, T, blank, lds_bp, vec;
  int32_t *align, *tok_start, *tok_end;
  float *frame_lp, *tok_lp, *total;
  unsigned short* ws;  // [B][T][threads] back-pointer words when !lds_bp
};

constexpr float NINF = -INFINITY;

static inline int ca_waves(int Lmax) { return em_cdiv(2 * Lmax + 1, 64 * CA_SPL); }

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

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_align_kernel(const AlignArgs a) {
  extern __shared__ unsigned short bp_lds[];  // [T][NT] when a.lds_bp
  __shared__ unsigned short win[CA_CH * CA_WIN];
  __shared__ unsigned short pth[CA_CH + 1];
  __shared__ float xch[2][CA_MAX_WAVES];
  __shared__ float fin[2];
  __shared__ int s_carry;

  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, blank = a.blank, Lmax = a.Lmax;
  const int Tb = min(max(a.xlens[b], 0), T);
  const int L = min(max(a.ylens[b], 0), Lmax);
  const int S = 2 * L + 1;
  const int32_t* y = a.targets + (size_t)b * Lmax;
  const long ldT = a.ldT, colb = (long)b * T;
  unsigned short* wsb = a.lds_bp ? nullptr : a.ws + (size_t)b * T * NT;

  if (tid < 2) fin[tid] = NINF;
  group_sync<MULTI>();

  // ---- forward pass
  float al[CA_SPL];
#pragma unroll
  for (int j = 0; j < CA_SPL; ++j) al[j] = NINF;
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
    for (int q = 0; q < 4; ++q) cur[q] = load4(rows[q], col0, vec, ldT);
    cur[4] = load4(rowb, col0, vec, ldT);
#pragma unroll
    for (int q = 0; q < 5; ++q) nxt[q] = cur[q];
    for (int k = 0; k < NG; ++k) {
      if (k + 1 < NG) {
        const long c = col0 + 4L * (k + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q] = load4(rows[q], c, vec, ldT);
        nxt[4] = load4(rowb, c, vec, ldT);
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
          float nw[CA_SPL];
          unsigned bp = 0;
#pragma unroll
          for (int j = 0; j < CA_SPL; ++j) {
            const float one = j == 0 ? p7 : al[j - 1];
            float best = al[j];
            unsigned mv = 0;
            if (one > best) {
              best = one;
              mv = 1;
            }
            if (j & 1) {
              const float two = fminf(j == 1 ? p7 : al[j - 2], cap[j >> 1]);
              if (two > best) {
                best = two;
                mv = 2;
              }
              nw[j] = best + cur[j >> 1][i];
            } else {
              nw[j] = best + eb;
            }
            bp |= mv << (2 * j);
          }
#pragma unroll
          for (int j = 0; j < CA_SPL; ++j) al[j] = nw[j];
          if (a.lds_bp)
            bp_lds[(size_t)t * NT + tid] = (unsigned short)bp;
          else
            wsb[(size_t)t * NT + tid] = (unsigned short)bp;
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
    for (int j = 0; j < CA_SPL; ++j) {
      const int s = CA_SPL * tid + j;
      if (s == S - 1) fin[0] = al[j];
      if (s == S - 2) fin[1] = al[j];
    }
  }
  group_sync<MULTI>();

  // ---- outputs: the padding first (the output pointers are formed only here: the forward loop is short of scalar registers)
  int32_t* align = a.align + (size_t)b * T;
  float* frame_lp = a.frame_lp + (size_t)b * T;
  int32_t* tok_start = a.tok_start + (size_t)b * Lmax;
  int32_t* tok_end = a.tok_end + (size_t)b * Lmax;
  float* tok_lp = a.tok_lp + (size_t)b * Lmax;
  for (int t = Tb + tid; t < T; t += NT) {
    align[t] = -1;
    frame_lp[t] = 0.f;
  }
  for (int i = L + tid; i < Lmax; i += NT) {
    tok_start[i] = -1;
    tok_end[i] = -1;
    tok_lp[i] = 0.f;
  }
  // ---- where the path ends
  const float a1 = fin[0], a2 = fin[1];
  const int s_end = (L == 0 || a1 > a2) ? S - 1 : S - 2;
  const float tot = s_end == S - 1 ? a1 : a2;
  if (tid == 0) a.total[b] = (Tb > 0 && tot > NINF) ? tot : NINF;
  if (!(Tb > 0 && tot > NINF)) {  // no path (or no frame): labels -1, spans -1, scores 0
    for (int t = tid; t < Tb; t += NT) {
      align[t] = -1;
      frame_lp[t] = 0.f;
    }
    for (int i = tid; i < L; i += NT) {
      tok_start[i] = -1;
      tok_end[i] = -1;
      tok_lp[i] = 0.f;
    }
    return;
  }

  // ---- back-trace, CA_CH frames at a time from the last frame
  int s_top = s_end;  // the path's state at frame t_hi - 1
  for (int t_hi = Tb; t_hi > 0; t_hi -= CA_CH) {
    const int t_lo = max(t_hi - CA_CH, 0), n = t_hi - t_lo;
    const int w_lo = max(s_top - 2 * (n - 1), 0) >> 3, W = (s_top >> 3) - w_lo + 1;  // W <= CA_WIN
    if (!a.lds_bp) {
      for (int idx = tid; idx < n * W; idx += NT) {
        const int r = idx / W, c = idx - r * W;
        if (t_lo + r > 0) win[r * CA_WIN + c] = wsb[(size_t)(t_lo + r) * NT + w_lo + c];  // (frame 0 has no back-pointers)
      }
    }
    group_sync<MULTI>();
    auto move_at = [&](int t, int s) -> int {  // the move recorded for state s at frame t >= 1
      const unsigned w = a.lds_bp ? bp_lds[(size_t)t * NT + (s >> 3)] : win[(t - t_lo) * CA_WIN + (s >> 3) - w_lo];
      return (w >> (2 * (s & 7))) & 3;
    };
    if (tid == 0) {
      const unsigned short after = t_hi < Tb ? pth[0] : (unsigned short)0xffff;  // the state at frame t_hi
      int s = s_top;
      for (int t = t_hi - 1; t >= t_lo; --t) {
        pth[t - t_lo] = (unsigned short)s;
        if (t > 0) s -= move_at(t, s);
      }
      pth[n] = after;
      s_carry = s;
    }
    group_sync<MULTI>();
    for (int r = tid; r < n; r += NT) {
      const int t = t_lo + r, p = pth[r];
      const int lab = (p & 1) ? y[p >> 1] : blank;
      align[t] = lab;
      frame_lp[t] = a.lpT[(size_t)lab * ldT + colb + t];
      if (p & 1) {
        if (pth[r + 1] != p) tok_end[p >> 1] = t + 1;
        if (t == 0 || move_at(t, p) != 0) tok_start[p >> 1] = t;
      }
    }
    s_top = s_carry;
    group_sync<MULTI>();
  }

  // ---- mean log-prob of each token's span, in frame order (the spans were stored by other threads of this workgroup:
  // the sync above orders them)
  for (int i = tid; i < L; i += NT) {
    const int st = tok_start[i], en = tok_end[i];
    const float* row = a.lpT + (size_t)y[i] * ldT + colb;
    float sum = 0.f;
    for (int t = st; t < en; ++t) sum += row[t];
    tok_lp[i] = sum / (float)(en - st);
  }
}

}  // namespace

extern "C" int32_t em_ctc_forced_align_max_tokens(void) { return CA_MAX_L; }

extern "C" size_t em_ctc_forced_align_workspace_bytes(int32_t B, int32_t T, int32_t Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0 || Lmax > CA_MAX_L) return 0;
  const size_t per_utt = (size_t)T * ca_waves(Lmax) * 64 * sizeof(unsigned short);
  return per_utt <= (size_t)CA_LDS_BP_BYTES ? 0 : per_utt * B;
}

extern "C" int em_ctc_forced_align(const float* lpT, int32_t ldT, const int32_t* xlens, const int32_t* targets,
                                   int32_t Lmax, const int32_t* ylens, int32_t B, int32_t T, int32_t blank,
                                   int32_t* align, float* frame_lp, int32_t* tok_start, int32_t* tok_end,
                                   float* tok_lp, float* total, void* ws, size_t ws_bytes, void* stream) {
  if (!lpT || !xlens || !ylens || !align || !frame_lp || !total || B <= 0 || T <= 0 || Lmax < 0 || blank < 0)
    return EM_ERR_BAD_ARG;
  if (Lmax > 0 && (!targets || !tok_start || !tok_end || !tok_lp)) return EM_ERR_BAD_ARG;
  if ((long)ldT < (long)B * T) return EM_ERR_BAD_ARG;
  if (Lmax > CA_MAX_L) return EM_ERR_UNSUPPORTED;
  const size_t need = em_ctc_forced_align_workspace_bytes(B, T, Lmax);
  if (need > 0 && (!ws || ws_bytes < need)) return EM_ERR_WORKSPACE;
  const int nw = ca_waves(Lmax);
  AlignArgs a;
  a.lpT = lpT; a.xlens = xlens; a.targets = targets; a.ylens = ylens;
  a.ldT = ldT; a.Lmax = Lmax; a.T = T; a.blank = blank;
  a.lds_bp = need == 0;
  a.vec = (ldT % 4 == 0) && (((uintptr_t)lpT & 15) == 0);
  a.align = align; a.tok_start = tok_start; a.tok_end = tok_end;
  a.frame_lp = frame_lp; a.tok_lp = tok_lp; a.total = total;
  a.ws = (unsigned short*)ws;
  const size_t dyn = a.lds_bp ? (size_t)T * nw * 64 * sizeof(unsigned short) : 0;
  if (nw == 1)
    hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(B), dim3(64), dyn, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(B), dim3(64 * nw), dyn, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
