// CTC forced alignment: the Viterbi path of a given transcript through the CTC log-posteriors, for a ragged batch in
// one launch.  Reference: CTC.forced_align, espnet2/asr/ctc.py (a wrapper of torchaudio.functional.forced_align, one
// utterance per call on the CPU); the contract (states, recursion, tie rule, outputs) is include/espnet_amd.h's.
//
// Layout of the work: the shared trellis walk of ctc_trellis.h - one workgroup per utterance, 8 states per lane, one
// wave up to S = 512 and up to 16 waves beyond (L <= 4 095), emissions from the frame-contiguous lpT rows four frames
// per load - with the Viterbi cell: of stay / one / two the first strictly larger predecessor wins, its move is 2 bits.
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
//   ctc_align_kernel<false> (one wave)  : 86 VGPRs, 88 SGPRs, 0 bytes of scratch, no spills, 8 976 B of LDS, no s_barrier
//   ctc_align_kernel<true>  (2-16 waves): 89 VGPRs, 90 SGPRs, 0 bytes of scratch, no spills, 9 104 B of LDS
// (LDS: the static part; the one-wave form adds T * 128 bytes of back-pointers, 31.9 KB at T = 249.)
#include "ctc_trellis.h"

namespace {

using ctc_trellis::group_sync;
using ctc_trellis::NINF;
constexpr int CA_SPL = ctc_trellis::SPL;                         // states per lane: 2 bits each in a 16-bit word
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

// the Viterbi cell: the best of stay / one / two in this order under strict >, and the 8 moves of a thread's frame in
// one 16-bit store, to LDS or to the workspace
struct ViterbiCell {
  unsigned short *bp_lds, *wsb;  // [T][NT] back-pointer words: LDS when lds_bp, else the workspace
  int lds_bp, NT, tid;
  unsigned bp = 0;
  static __device__ __forceinline__ f32x4 prepare(f32x4 e) { return e; }
  __device__ __forceinline__ float blank(int j, float stay, float one, float e) { return token(j, stay, one, NINF, e); }
  __device__ __forceinline__ float token(int j, float stay, float one, float two, float e) {
    float best = stay;
    unsigned mv = 0;
    if (one > best) {
      best = one;
      mv = 1;
    }
    if (two > best) {
      best = two;
      mv = 2;
    }
    bp |= mv << (2 * j);
    return best + e;
  }
  __device__ __forceinline__ void frame(int t) {
    if (lds_bp)
      bp_lds[(size_t)t * NT + tid] = (unsigned short)bp;
    else
      wsb[(size_t)t * NT + tid] = (unsigned short)bp;
    bp = 0;
  }
};

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_align_kernel(const AlignArgs a) {
  extern __shared__ unsigned short bp_lds[];  // [T][NT] when a.lds_bp
  __shared__ unsigned short win[CA_CH * CA_WIN];
  __shared__ unsigned short pth[CA_CH + 1];
  __shared__ float xch[2][ctc_trellis::MAX_WAVES];
  __shared__ float fin[2];
  __shared__ int s_carry;

  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int T = a.T, blank = a.blank, Lmax = a.Lmax;
  const int Tb = min(max(a.xlens[b], 0), T);
  const int L = min(max(a.ylens[b], 0), Lmax);
  const int S = 2 * L + 1;
  const int32_t* y = a.targets + (size_t)b * Lmax;
  const long ldT = a.ldT, colb = (long)b * T;
  unsigned short* wsb = a.lds_bp ? nullptr : a.ws + (size_t)b * T * NT;

  // ---- forward pass
  ViterbiCell cell{bp_lds, wsb, a.lds_bp, NT, tid};
  ctc_trellis::forward<MULTI>(a.lpT, ldT, colb, a.vec != 0, y, L, Tb, blank, xch, fin, cell);

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

extern "C" int32_t em_ctc_forced_align_max_tokens(void) { return ctc_trellis::MAX_L; }

extern "C" size_t em_ctc_forced_align_workspace_bytes(int32_t B, int32_t T, int32_t Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0 || Lmax > ctc_trellis::MAX_L) return 0;
  const size_t per_utt = (size_t)T * ctc_trellis::waves(Lmax) * 64 * sizeof(unsigned short);
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
  if (Lmax > ctc_trellis::MAX_L) return EM_ERR_UNSUPPORTED;
  const size_t need = em_ctc_forced_align_workspace_bytes(B, T, Lmax);
  if (need > 0 && (!ws || ws_bytes < need)) return EM_ERR_WORKSPACE;
  const int nw = ctc_trellis::waves(Lmax);
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
