// CTC segmentation: where the utterances of a long text lie in a long recording - the banded Viterbi trellis over the
// ground-truth COLUMNS (no separate blank states) of the ctc_segmentation package as espnet2/bin/asr_align.py uses it,
// for a ragged batch of recordings in one launch.  The contract (band, recursion, tie rule, end, back-trace, outputs) is
// include/espnet_amd.h's; the reference package was not at hand, the header's text governs.
//
// Layout of the work: one workgroup per recording, the frames in sequence.  SL = threads * 8 slots hold the band: column
// c lives in slot c mod SL, thread i owns the slots 8 i .. 8 i + 7 in registers.  The band [lo, lo + W_b), W_b <= SL,
// slides to the right: the slot whose column fell below lo takes the column SL further on, with k = -inf.  A thread
// needs of its neighbours only k[t-1] of the slot below its run: one lane rotation (DPP wave_ror:1) in one wave, a lane
// shift plus one LDS word per wave and one barrier per frame in 2 .. 16 waves; the last slot wraps to slot 0.  A
// neighbour counts only where its column was inside the band of row t - 1.  W <= 512 runs as ONE wave64 without a
// workgroup barrier in the forward pass.
//
// Emissions come from lpT [V][ldT] (em_ctc_log_probs_t): four frames of a column's token row per 16-byte load, the loads
// of frame group g + 1 issued before the chain of group g (ctc_trellis.h's scheme and its load4).  A slot whose column
// changes inside or in front of a group loads the old and the new row and takes each frame from the one the band has
// then; the new column's id is a dependent load in front of that (one or two slots of the workgroup per group).
//
// Back-pointers are 1 bit per (row, slot): a thread's 8 in one byte store per frame, to LDS when T * threads bytes fit
// CS_LDS_BP_BYTES, else to the caller's workspace [B][T][threads].  The back-trace walks CS_CH rows at a time: the path
// loses at most one column per row, so the chunk's window (CS_WIN bytes per row) is first copied to LDS by all threads,
// one thread walks it, then all threads turn the chunk's path into frame_col / frame_lp / first_frame and the clipped
// flag in parallel.  The arg-max over t of the last column is kept by the thread that owns its slot.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (ROCm 7.2):
//   ctc_segment_kernel<false> (one wave)  : 132 VGPRs, 106 SGPRs, 0 bytes of scratch, no VGPR spills, 9 752 B of LDS, no s_barrier in the forward pass
//   ctc_segment_kernel<true>  (2-16 waves): 128 VGPRs, 106 SGPRs, 0 bytes of scratch, no VGPR spills, 9 880 B of LDS
// (16 / 20 scalar registers are kept in lanes of a VGPR, none in memory.  LDS: the static part; back-pointers in LDS add
// T * threads bytes, 44.8 KB at T = 700 in one wave.  The multi-wave form sits at the 128-VGPR line of 1 024 threads:
// the cells are computed in place from the last slot down, and the output pointers are formed behind the forward pass.)
//
// Measured on an MI355X (tools/ctc_segment_bench.py, V 5 000): 1 x (T 90 000, C 45 000, W 8 192, 16 waves) 237 ms, 2.6 us
// per frame; 8 x (T 7 500, C 3 000, 6 waves) 10.2 ms, 1.4 us per frame.
#include "ctc_trellis.h"

namespace {

using ctc_trellis::group_sync;
using ctc_trellis::load4;
using ctc_trellis::NINF;
constexpr int CS_SPL = 8;                        // slots per lane: 1 bit each in a byte
constexpr int CS_MAX_WAVES = 16;                 // 1 024 threads
constexpr int CS_MAX_W = CS_MAX_WAVES * 64 * CS_SPL;  // 8 192 columns of band
constexpr int CS_LDS_BP_BYTES = 48 * 1024;       // back-pointers kept in LDS up to this size (ctc_align.hip's budget)
constexpr int CS_CH = 256;                       // rows per back-trace chunk
constexpr int CS_WIN = CS_CH / CS_SPL + 2;       // bytes per row that a chunk's window can span

struct SegArgs {
  const float* lpT;
  const int32_t *xlens, *gt, *clens;
  int32_t ldT, Cmax, T, blank, W, flags, lds_bp, vec;
  int32_t *first_frame, *frame_col, *t_end, *status;
  float *frame_lp, *total;
  unsigned char* ws;  // [B][T][threads] back-pointer bytes when !lds_bp
};

static inline int seg_waves(int Cmax, int W) { return em_cdiv(W < Cmax ? W : Cmax, 64 * CS_SPL); }

// the band's lowest column from q = floor(t C / T)
__device__ __forceinline__ int band_lo(int q, int Wb, int C) { return min(max(q - (Wb >> 1), 0), C - Wb); }

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_segment_kernel(const SegArgs a) {
  extern __shared__ unsigned char bp_lds[];  // [T][NT] when a.lds_bp
  __shared__ unsigned char win[CS_CH * CS_WIN];
  __shared__ int pth[CS_CH];
  __shared__ float xch[2][CS_MAX_WAVES];
  __shared__ float fin_v[2];
  __shared__ int fin_t, s_carry_c, s_carry_t, s_clip;

  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
  const int SL = NT * CS_SPL;
  const int T = a.T, blank = a.blank, Cmax = a.Cmax;
  const int Tb = min(max(a.xlens[b], 0), T);
  const int C = min(max(a.clens[b], 0), Cmax);
  const int Wb = min(a.W, C);
  const bool pf = a.flags & 1, from_last = a.flags & 2;
  const int32_t* gt = a.gt + (size_t)b * Cmax;
  const long ldT = a.ldT, colb = (long)b * T;
  const float* lpT = a.lpT;
  unsigned char* bp = a.lds_bp ? bp_lds : a.ws + (size_t)b * T * NT;  // row t >= 1 at [(t - 1) * NT + tid]

  bool route = C >= 2 && Tb > 0;
  int t_end = 0;
  float total = NINF;

  if (route) {
    // ---- forward pass
    if (tid < 2) fin_v[tid] = NINF;
    if (tid == 0) fin_t = 0;
    if (MULTI) {
      if (tid < 2 * CS_MAX_WAVES) (&xch[0][0])[tid] = NINF;
    }
    group_sync<MULTI>();

    const int qC = C / Tb, rC = C % Tb;  // floor(t C / Tb) = q, t C mod Tb = acc, one row at a time
    const int s0 = CS_SPL * tid;
    const int slot_last = (C - 1) % SL, tid_last = slot_last >> 3, j_last = slot_last & 7;
    // the column of slot s under a band that begins at lo: the one of [lo, lo + SL) that is s mod SL
    auto col_of = [&](int s, int qlo, int rlo) { return s + SL * (qlo + (s < rlo ? 1 : 0)); };
    auto id_of = [&](int c) { return (c >= 1 && c < C) ? gt[c] : blank; };  // (column 0's value is never read)

    float k[CS_SPL];
    int tok[CS_SPL];  // the id of the slot's column at the last row the prefetch has seen
#pragma unroll
    for (int j = 0; j < CS_SPL; ++j) {
      k[j] = (s0 + j == 0) ? 0.f : NINF;
      tok[j] = id_of(s0 + j);
    }
    const float* rowb = lpT + (size_t)blank * ldT;
    const long col0 = a.vec ? (colb & ~3L) : colb;
    const int off = (int)(colb - col0);
    const int NG = (off + Tb + 3) >> 2;

    // prefetch cursor: the band of the rows t = f + 1 of a group's frames
    int pq = 0, pacc = 0, p_t = 0;      // q and acc of row p_t, the last row the cursor has passed
    int p_qlo = 0, p_rlo = 0;           // lo of that row, split by SL
    struct Rows { int qlo[4], rlo[4]; };  // lo = qlo * SL + rlo
    Rows cr, nr;
    f32x4 cur[CS_SPL + 1], nxt[CS_SPL + 1];

    auto fetch = [&](int g, Rows& r, f32x4* dst) {
      const long c = col0 + 4L * g;
      const int pq0 = p_qlo, pr0 = p_rlo;  // the band of the row in front of this group
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = 4 * g + i - off + 1;
        if (t >= 1 && t <= Tb) {
          while (p_t < t) {
            pq += qC;
            pacc += rC;
            if (pacc >= Tb) {
              pacc -= Tb;
              ++pq;
            }
            ++p_t;
          }
          const int lo = band_lo(pq, Wb, C);
          p_rlo += lo - (p_qlo * SL + p_rlo);  // lo never falls: split it by SL without a division
          while (p_rlo >= SL) {
            p_rlo -= SL;
            ++p_qlo;
          }
        }
        r.qlo[i] = p_qlo;
        r.rlo[i] = p_rlo;
      }
      dst[CS_SPL] = load4(rowb, c, a.vec, ldT);
#pragma unroll
      for (int j = 0; j < CS_SPL; ++j) {
        const int s = s0 + j;
        const int c_old = col_of(s, pq0, pr0), c_new = col_of(s, r.qlo[3], r.rlo[3]);
        f32x4 e = load4(lpT + (size_t)tok[j] * ldT, c, a.vec, ldT);
        if (c_new != c_old) {
          tok[j] = id_of(c_new);
          const f32x4 en = load4(lpT + (size_t)tok[j] * ldT, c, a.vec, ldT);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (col_of(s, r.qlo[i], r.rlo[i]) == c_new) e[i] = en[i];
        }
        dst[j] = e;
      }
    };

    fetch(0, cr, cur);
    nr = cr;
#pragma unroll
    for (int q = 0; q <= CS_SPL; ++q) nxt[q] = cur[q];

    int lo_prev = 0;  // the band of row t - 1
    float best = NINF, lastv = NINF;
    int best_t = 0;
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) fetch(g + 1, nr, nxt);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = 4 * g + i - off + 1;  // the row of frame t - 1
        if (t < 1 || t > Tb) continue;      // the same in every thread of the workgroup
        const int qlo = cr.qlo[i], rlo = cr.rlo[i], lo = qlo * SL + rlo;
        const float eb = cur[CS_SPL][i];
        // k[t-1] of the slot below this thread's run (the last slot's for slot 0)
        float p7;
        if (MULTI) {
          p7 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, NINF),
                                                                     __builtin_bit_cast(int, k[7]), 0x138, 0xf, 0xf,
                                                                     false));  // wave_shr:1
          if (lane == 0) p7 = xch[(t - 1) & 1][wave == 0 ? NW - 1 : wave - 1];
        } else {
          p7 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, NINF),
                                                                     __builtin_bit_cast(int, k[7]), 0x13C, 0xf, 0xf,
                                                                     false));  // wave_ror:1
        }
        unsigned bits = 0;
        // the cells from the thread's last slot down, so that k[j - 1] still holds row t - 1 when slot j reads it.
        // a wave whose every column lies inside the band of both rows, with its left neighbour, runs the bare cell
        const int c0 = col_of(s0, qlo, rlo), c7 = col_of(s0 + 7, qlo, rlo);
        if (__all(c7 == c0 + 7 && c0 > lo_prev && c7 < lo_prev + Wb && c7 < lo + Wb)) {
#pragma unroll
          for (int j = CS_SPL - 1; j >= 0; --j) {
            const float left = j == 0 ? p7 : k[j - 1];
            const float e = cur[j][i];
            const float stay = k[j] + fmaxf(eb, e);
            const float sw = left + e;
            const bool mv = sw > stay;
            k[j] = mv ? sw : stay;
            bits |= mv ? (1u << j) : 0u;
          }
        } else {
#pragma unroll
          for (int j = CS_SPL - 1; j >= 0; --j) {
            const int c = col_of(s0 + j, qlo, rlo);
            const float left = j == 0 ? p7 : k[j - 1];
            // the values of row t - 1: -inf where the column was outside that row's band
            const float kp = (unsigned)(c - lo_prev) < (unsigned)Wb ? k[j] : NINF;
            const float lp1 = (unsigned)(c - 1 - lo_prev) < (unsigned)Wb ? left : NINF;
            const float e = cur[j][i];
            const float stay = kp + fmaxf(eb, e);
            const float sw = lp1 + e;
            const bool mv = sw > stay;
            float v = mv ? sw : stay;
            if (c == 0) v = pf ? 0.f : kp + eb;
            const bool in = c < lo + Wb;
            k[j] = in ? v : NINF;
            bits |= (mv && in && c != 0) ? (1u << j) : 0u;
          }
        }
        bp[(size_t)(t - 1) * NT + tid] = (unsigned char)bits;
        if (tid == tid_last) {
          float v = k[0];
#pragma unroll
          for (int j = 1; j < CS_SPL; ++j) v = j == j_last ? k[j] : v;
          if (lo + Wb != C) v = NINF;  // the slot holds an earlier column, or the last column lies outside the band
          if (v > best) {
            best = v;
            best_t = t;
          }
          lastv = v;
        }
        lo_prev = lo;
        if (MULTI) {
          if (lane == 63) xch[t & 1][wave] = k[7];
          __syncthreads();
        }
      }
#pragma unroll
      for (int q = 0; q <= CS_SPL; ++q) cur[q] = nxt[q];
      cr = nr;
    }
    if (tid == tid_last) {
      fin_v[0] = from_last ? lastv : best;
      fin_t = from_last ? Tb : best_t;
    }
    group_sync<MULTI>();
    total = fin_v[0];
    t_end = fin_t;
    route = total > NINF;
  }

  // ---- outputs: the pads, and everything when there is no route (the output pointers are formed only here: the
  // forward loop is short of registers)
  int32_t* first_frame = a.first_frame + (size_t)b * Cmax;
  int32_t* frame_col = a.frame_col + (size_t)b * T;
  float* frame_lp = a.frame_lp + (size_t)b * T;
  if (!route) {
    t_end = 0;
    total = NINF;
  }
  for (int t = max(t_end, route ? Tb : 0) + tid; t < T; t += NT) {
    frame_col[t] = -1;
    frame_lp[t] = 0.f;
  }
  for (int i = (route ? C : 0) + tid; i < Cmax; i += NT) first_frame[i] = -1;
  if (!route) {
    if (tid == 0) {
      a.total[b] = NINF;
      a.t_end[b] = 0;
      a.status[b] = 1;
    }
    return;
  }
  for (int t = t_end + tid; t < Tb; t += NT) {  // trailing frames at or after t_end
    frame_col[t] = -1;
    frame_lp[t] = 0.f;
  }
  if (tid == 0) s_clip = 0;

  // ---- back-trace, CS_CH rows at a time from (t_end, C - 1), while t > 0 and c > 0
  const float* rowb = lpT + (size_t)blank * ldT + colb;
  int t_hi = t_end, c_top = C - 1;  // the path's cell the chunk starts from
  while (t_hi > 0 && c_top > 0) {
    const int t_lo = max(t_hi - CS_CH, 0), n = t_hi - t_lo;  // the rows t_lo + 1 .. t_hi
    const int w_lo = max(c_top - n, 0) >> 3, WN = (c_top >> 3) - w_lo + 1;  // byte columns c >> 3; WN <= CS_WIN
    if (!a.lds_bp) {
      for (int idx = tid; idx < n * WN; idx += NT) {
        const int r = idx / WN, w = idx - r * WN;
        win[r * CS_WIN + w] = bp[(size_t)(t_lo + r) * NT + (w_lo + w) % NT];
      }
    }
    group_sync<MULTI>();
    auto move_at = [&](int t, int c) -> int {  // the move bit of column c at row t >= 1
      const unsigned w = a.lds_bp ? bp_lds[(size_t)(t - 1) * NT + (c >> 3) % NT] : win[(t - 1 - t_lo) * CS_WIN + (c >> 3) - w_lo];
      return (w >> (c & 7)) & 1;
    };
    if (tid == 0) {
      int c = c_top, t = t_hi;
      for (; t > t_lo && c > 0; --t) {
        pth[t - 1 - t_lo] = c;
        c -= move_at(t, c);
      }
      s_carry_c = c;
      s_carry_t = t;
    }
    group_sync<MULTI>();
    const int t_stop = s_carry_t;  // the rows t_stop + 1 .. t_hi were visited
    int clip = 0;
    for (int r = t_stop - t_lo + tid; r < n; r += NT) {
      const int t = t_lo + 1 + r, f = t - 1, c = pth[r];
      const int lo = band_lo((int)(((long long)t * C) / Tb), Wb, C);
      if ((c == lo && lo > 0) || (c == lo + Wb - 1 && lo + Wb < C)) clip = 1;
      const float e = lpT[(size_t)gt[c] * ldT + colb + f];
      frame_col[f] = c;
      if (move_at(t, c)) {
        frame_lp[f] = e;
        first_frame[c] = f;
      } else {
        frame_lp[f] = fmaxf(rowb[f], e);
      }
    }
    if (clip) atomicOr(&s_clip, 2);
    t_hi = t_stop;
    c_top = s_carry_c;
    group_sync<MULTI>();
  }
  // the preamble: the frames in front of the path, and the columns a path that ran out of rows never reached
  for (int t = tid; t < t_hi; t += NT) {
    frame_col[t] = -1;
    frame_lp[t] = 0.f;
  }
  for (int i = 1 + tid; i <= c_top; i += NT) first_frame[i] = -1;
  if (tid == 0) {
    first_frame[0] = 0;
    a.total[b] = total;
    a.t_end[b] = t_end;
    a.status[b] = s_clip;
  }
}

}  // namespace

extern "C" int32_t em_ctc_segment_max_window(void) { return CS_MAX_W; }

extern "C" size_t em_ctc_segment_workspace_bytes(int32_t B, int32_t T, int32_t Cmax, int32_t W) {
  if (B <= 0 || T <= 0 || Cmax < 2 || W < 1 || W > CS_MAX_W) return 0;
  const size_t per_rec = (size_t)T * seg_waves(Cmax, W) * 64;
  return per_rec <= (size_t)CS_LDS_BP_BYTES ? 0 : per_rec * B;
}

extern "C" int em_ctc_segment(const float* lpT, int32_t ldT, const int32_t* xlens, const int32_t* gt, int32_t Cmax,
                              const int32_t* clens, int32_t B, int32_t T, int32_t blank, int32_t W, int32_t flags,
                              int32_t* first_frame, int32_t* frame_col, float* frame_lp, int32_t* t_end, float* total,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!lpT || !xlens || !gt || !clens || !first_frame || !frame_col || !frame_lp || !t_end || !total || !status ||
      B <= 0 || T <= 0 || Cmax < 2 || blank < 0 || W < 1 || (flags & ~3))
    return EM_ERR_BAD_ARG;
  if ((long)ldT < (long)B * T) return EM_ERR_BAD_ARG;
  if (W > CS_MAX_W) return EM_ERR_UNSUPPORTED;
  const size_t need = em_ctc_segment_workspace_bytes(B, T, Cmax, W);
  if (need > 0 && (!ws || ws_bytes < need)) return EM_ERR_WORKSPACE;
  const int nw = seg_waves(Cmax, W);
  SegArgs a;
  a.lpT = lpT; a.xlens = xlens; a.gt = gt; a.clens = clens;
  a.ldT = ldT; a.Cmax = Cmax; a.T = T; a.blank = blank; a.W = W; a.flags = flags;
  a.lds_bp = need == 0;
  a.vec = (ldT % 4 == 0) && (((uintptr_t)lpT & 15) == 0);
  a.first_frame = first_frame; a.frame_col = frame_col; a.t_end = t_end; a.status = status;
  a.frame_lp = frame_lp; a.total = total;
  a.ws = (unsigned char*)ws;
  const size_t dyn = a.lds_bp ? (size_t)T * nw * 64 : 0;
  if (nw == 1)
    hipLaunchKernelGGL(ctc_segment_kernel<false>, dim3(B), dim3(64), dyn, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ctc_segment_kernel<true>, dim3(B), dim3(64 * nw), dyn, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
