// CTC forward-backward: the state occupancies gamma[t][s] = alpha[t][s] * beta[t][s] / (p[t][lab s] * P(y|x)) of given
// transcripts, reduced per token on the fly to the expected number of frames (occ), the largest occupancy (peak: the
// token's confidence) and its frame (peak_t), for a ragged batch of candidates in one launch.  The contract is
// include/espnet_amd.h's ("CTC token posteriors"); alpha, nll and the candidate batching (mem_of) are em_ctc_seq_nll's.
//
// Layout of the work.  The dependent chain over the frames is the cost, so both directions run at once: one workgroup
// per candidate, two wave groups (threadIdx.y).  Group A walks alpha from frame 0 upward (ctc_trellis::forward), group B
// walks beta from frame T_b - 1 downward (ctc_trellis::backward), each with the state-to-lane mapping of ctc_trellis.h
// (8 states per lane, one wave per direction up to S = 512, ceil(S / 512) waves beyond).  With h = (T_b - 1) / 2, A
// stores its rows of the frames 0 .. h and B its rows of the frames h + 1 .. T_b - 1 into the workspace - float32,
// ceil(T / 2) + 1 rows of RS = 2 Lmax + 1 (rounded up to 8) states per direction and candidate - then they meet (ONE
// barrier) and each goes on through the other's half: A combines its running row with the stored beta row of the
// frames h + 1 .., B with the stored alpha row of the frames h .. 0, into gamma, which lives in registers only: a lane
// owns the tokens 4 i .. 4 i + 3 and keeps their sum, maximum and arg-max.  Neither a [T][S] alpha nor any gamma
// reaches memory.  P(y|x) is the sum over s of alpha * beta / p at ANY frame, so each group takes it at its first
// combined frame (one reduction over the group) and normalises as it goes.  The stored rows are read through a
// register ring RING frames ahead of their use (started at the first combined frame), so their latency is not in the chain.  At the end B hands its three
// values per token to A through the output arrays themselves (one more barrier) and A writes the merged result.
//
// Two directions of up to 8 waves fit a workgroup.  Above S = 4 096 (9 .. 16 waves per direction) the same cells run in
// ONE group of waves as three walks in sequence - alpha storing its half, beta storing and combining, alpha once more
// combining - with the same arithmetic in the same order, so a candidate's values do not depend on the form.
//
// blank_post (optional) is a sum over all blank states of a frame, that is over the lanes: a wave reduces it and, with
// more waves than one, leaves its part in the workspace ([T][waves] behind the rows); the parts are added in wave order
// after the walks.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (ROCm 7.2): see DESIGN.md 4ac.
#include "ctc_post_common.h"

namespace {

using ctc_trellis::lse2;
using ctc_trellis::lse3;
using ctc_trellis::MAX_WAVES;
using ctc_trellis::NINF;
using ctc_trellis::SPL;
using namespace ctc_post_common;  // CP_DUAL_WAVES, the row geometry, lse_merge, TokAcc
// frames a stored row is loaded ahead of its use: what the registers allow (128 per lane in a 1 024-thread workgroup)
template <bool MULTI>
constexpr int CP_RING = MULTI ? 1 : 3;

struct PostArgs {
  const float* lpT;
  const int32_t *xlens, *targets, *ylens, *mem_of;
  int32_t ldT, Lmax, T, Bm, blank, vec, RS, R;
  float *nll, *occ, *peak, *blank_post;
  int32_t* peak_t;
  float* ws;
};

// floats per candidate: the rows of both directions, then blank_post's parts [T][waves] (more waves than one), 16-byte whole
__host__ __device__ static inline size_t ws_floats_per_cand(int R, int RS, int T, int nw) {
  return (size_t)2 * R * RS + (nw > 1 ? ((size_t)T * nw + 3) & ~(size_t)3 : 0);
}

// The sum-product cell of ctc_nll.hip, with the row's fate behind it.  UP: the alpha direction (frames ascending).
// A frame of the own half is stored (do_store), at the frame h the groups meet, a frame of the other half is combined
// with the stored row of the opposite direction (do_combine).
template <bool MULTI, bool UP>
struct PostCell {
  float* mine;         // this direction's rows of the candidate, [R][RS]
  const float* other;  // the opposite direction's
  float* bpart;        // blank_post of the candidate: [T] (one wave) or the parts [T][waves]; null: not wanted
  float (*red)[2];     // LDS [MAX_WAVES][2]: the reduction of P over the waves of this direction
  int RS, h, Tb, tid, nwaves;
  bool do_store, do_combine, meet_barrier;

  float v[SPL], e[SPL];  // the frame's cells and their emissions as the walk computed them
  static constexpr int RING = CP_RING<MULTI>;
  f32x4 ring[RING][2];
  float P = 0.f;
  bool dead = false;
  TokAcc acc;

  static __device__ __forceinline__ f32x4 prepare(f32x4 x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __fmul_rn(x[i], ctc_trellis::LOG2E);
    return x;
  }
  __device__ __forceinline__ float blank(int j, float stay, float one, float em) {
    e[j] = em;
    return v[j] = lse2(stay, one) + em;
  }
  __device__ __forceinline__ float token(int j, float stay, float one, float two, float em) {
    e[j] = em;
    return v[j] = lse3(stay, one, two) + em;
  }

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc.occ[q] = 0.f, acc.peak[q] = 0.f, acc.pt[q] = -1;
  }
  __device__ __forceinline__ bool owns() const { return SPL * tid < RS; }
  // the workspace row of frame t: alpha rows by frame, beta rows from the frame behind the meeting frame
  __device__ __forceinline__ size_t own_row(int t) const { return (size_t)(UP ? t : t - (h + 1)) * RS + SPL * tid; }
  __device__ __forceinline__ size_t other_row(int t) const { return (size_t)(UP ? t - (h + 1) : t) * RS + SPL * tid; }
  __device__ __forceinline__ void load(int k, int t) {
    const bool in = owns() && (UP ? t < Tb : t >= 0);
    const f32x4 ninf = {NINF, NINF, NINF, NINF};
    ring[k][0] = in ? *(const f32x4*)(other + other_row(t)) : ninf;
    ring[k][1] = in ? *(const f32x4*)(other + other_row(t) + 4) : ninf;
  }
  __device__ __forceinline__ void store(int t) {
    if (!owns()) return;
    f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    *(f32x4*)(mine + own_row(t)) = a;
    *(f32x4*)(mine + own_row(t) + 4) = b;
  }
  // behind the last stored row of this direction: wait for the other direction's.  Upward the opposite rows are read
  // from the NEXT frame on (combine starts the ring there): with h == 0 this barrier stands in front of forward's
  // opening one, where the other direction has not stored yet - a frame later a barrier of the walk lies in between.
  __device__ __forceinline__ void meet() {
    if (meet_barrier) __syncthreads();
  }

  // log2 P(y|x) from the products of this frame, over all lanes of the direction
  __device__ __forceinline__ void total(const float (&x)[SPL]) {
    float m = NINF, s = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) m = fmaxf(m, x[j]);
    const float sh = fmaxf(m, -FLT_MAX);
#pragma unroll
    for (int j = 0; j < SPL; ++j) s += __builtin_amdgcn_exp2f(x[j] - sh);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
    if (MULTI) {
      if ((tid & 63) == 0) red[tid >> 6][0] = m, red[tid >> 6][1] = s;
      __syncthreads();
      m = red[0][0], s = red[0][1];
      for (int w = 1; w < nwaves; ++w) lse_merge(m, s, red[w][0], red[w][1]);
      __syncthreads();
    }
    dead = !(m > NINF);
    P = m + __builtin_amdgcn_logf(s);
  }

  __device__ __forceinline__ void combine(int t) {
    const bool first = t == (UP ? h + 1 : h);  // the first combined frame of this direction
    if (first) {
#pragma unroll
      for (int k = 0; k < RING; ++k) load(k, UP ? t + k : t - k);
    }
    const float o[SPL] = {ring[0][0][0], ring[0][0][1], ring[0][0][2], ring[0][0][3],
                          ring[0][1][0], ring[0][1][1], ring[0][1][2], ring[0][1][3]};
#pragma unroll
    for (int k = 0; k + 1 < RING; ++k) ring[k][0] = ring[k + 1][0], ring[k][1] = ring[k + 1][1];
    load(RING - 1, UP ? t + RING : t - RING);
    float x[SPL];  // log2 of alpha * beta / p: both rows carry the frame's emission
#pragma unroll
    for (int j = 0; j < SPL; ++j) x[j] = (v[j] + o[j]) - fmaxf(e[j], -FLT_MAX);
    if (first) total(x);
    float g[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) g[j] = dead ? 0.f : __builtin_amdgcn_exp2f(x[j] - P);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float gq = g[2 * q + 1];
      acc.occ[q] += gq;
      // the lowest frame wins equal values: upward a later frame must be strictly larger, downward it may be equal
      if (UP ? gq > acc.peak[q] : (gq >= acc.peak[q] && gq > 0.f)) acc.peak[q] = gq, acc.pt[q] = t;
    }
    if (bpart) {
      float b = (g[0] + g[2]) + (g[4] + g[6]);
#pragma unroll
      for (int o2 = 32; o2 > 0; o2 >>= 1) b += __shfl_xor(b, o2);
      if ((tid & 63) == 0) bpart[MULTI ? (size_t)t * nwaves + (tid >> 6) : (size_t)t] = b;
    }
  }

  __device__ __forceinline__ void frame(int t) {
    const bool own = UP ? t <= h : t > h;
    if (own) {
      if (do_store) store(t);
      if (UP && t == h) meet();
    } else {
      if (!UP && t == h) meet();
      if (do_combine) combine(t);
    }
  }
};

template <bool MULTI, bool DUAL>
__global__ __launch_bounds__(MULTI ? 1024 : 128) void ctc_post_kernel(const PostArgs a) {
  __shared__ float xa[2][MAX_WAVES];
  __shared__ float xb[2][MAX_WAVES][2];
  __shared__ float fin[2];
  __shared__ float red[2][MAX_WAVES][2];

  const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, T = a.T, Lmax = a.Lmax, RS = a.RS;
  const int dir = DUAL ? __builtin_amdgcn_readfirstlane((int)threadIdx.y) : 0;  // wave-uniform: whole waves per direction
  const int NALL = DUAL ? 2 * NT : NT, tall = dir * NT + tid;
  const int u = a.mem_of ? min(max(a.mem_of[n], 0), a.Bm - 1) : n;
  const int Tb = min(max(a.xlens[u], 0), T);
  const int L = min(max(a.ylens[n], 0), Lmax);
  const int nwaves = NT >> 6, h = (Tb - 1) >> 1;
  const int32_t* y = a.targets + (size_t)n * Lmax;
  const long ldT = a.ldT, colb = (long)u * T;
  const bool vec = a.vec != 0;

  const size_t rows = (size_t)a.R * RS;
  float* wsn = a.ws + (size_t)n * ws_floats_per_cand(a.R, RS, T, nwaves);
  float* bp_out = a.blank_post ? a.blank_post + (size_t)n * T : nullptr;
  float* bpart = !bp_out ? nullptr : MULTI ? wsn + 2 * rows : bp_out;
  float* occ = a.occ + (size_t)n * Lmax;
  float* peak = a.peak + (size_t)n * Lmax;
  int32_t* peak_t = a.peak_t + (size_t)n * Lmax;

  // the padding, and everything of a candidate without a frame
  for (int i = (Tb > 0 ? L : 0) + tall; i < Lmax; i += NALL) occ[i] = 0.f, peak[i] = 0.f, peak_t[i] = i < L ? -1 : 0;
  if (bp_out)
    for (int t = Tb + tall; t < T; t += NALL) bp_out[t] = 0.f;
  if (Tb == 0) {
    if (tall == 0) a.nll[n] = INFINITY;
    return;
  }

  PostCell<MULTI, true> ca{wsn, wsn + rows, bpart, red[0], RS, h, Tb, tid, nwaves, true, DUAL, DUAL};
  PostCell<MULTI, false> cb{wsn + rows, wsn, bpart, red[1], RS, h, Tb, tid, nwaves, true, true, DUAL};
  ca.init();
  cb.init();

  // frame 0 of alpha does not pass through the cell: its row is the two emissions
  auto alpha_row0 = [&]() {
#pragma unroll
    for (int j = 0; j < SPL; ++j) ca.v[j] = NINF;
    if (tid == 0) {
      ca.v[0] = __fmul_rn(a.lpT[(size_t)a.blank * ldT + colb], ctc_trellis::LOG2E);
      if (L > 0) ca.v[1] = __fmul_rn(a.lpT[(size_t)y[0] * ldT + colb], ctc_trellis::LOG2E);
    }
    if (ca.do_store) ca.store(0);
    if (h == 0) ca.meet();
  };
  auto alpha_walk = [&]() {
    alpha_row0();
    ctc_trellis::forward<MULTI>(a.lpT, ldT, colb, vec, y, L, Tb, a.blank, xa, fin, ca);
    if (MULTI && Tb == 1) {  // no frame of the other half: the barriers of the reduction this direction never ran
      __syncthreads();
      __syncthreads();
    }
  };

  if (DUAL) {
    if (dir == 0)
      alpha_walk();
    else
      ctc_trellis::backward<MULTI>(a.lpT, ldT, colb, vec, y, L, Tb, a.blank, xb, cb);
  } else {
    ca.do_combine = false;
    alpha_walk();
    ctc_trellis::backward<MULTI>(a.lpT, ldT, colb, vec, y, L, Tb, a.blank, xb, cb);
    ca.do_store = false, ca.do_combine = true;
    alpha_walk();
  }

  // ---- B's values reach A through the output arrays (DUAL), or sit in the same thread
  TokAcc lo = cb.acc;
  if (DUAL) {
    if (dir == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * tid + q;
        if (i < L) occ[i] = lo.occ[q], peak[i] = lo.peak[q], peak_t[i] = lo.pt[q];
      }
    }
    __syncthreads();
    if (dir == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * tid + q;
        if (i < L) lo.occ[q] = occ[i], lo.peak[q] = peak[i], lo.pt[q] = peak_t[i];
      }
    }
  }
  const float tot = lse2(fin[0], fin[1]);  // as em_ctc_seq_nll has it
  const bool path = tot > NINF;
  if (dir == 0) {
    if (tid == 0) a.nll[n] = path ? -__fmul_rn(tot, ctc_trellis::LN2) : INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * tid + q;
      if (i >= L) continue;
      const bool up = ca.acc.peak[q] > lo.peak[q];  // equal: the lower half's frame
      occ[i] = path ? lo.occ[q] + ca.acc.occ[q] : 0.f;
      peak[i] = path ? (up ? ca.acc.peak[q] : lo.peak[q]) : 0.f;
      peak_t[i] = path ? (up ? ca.acc.pt[q] : lo.pt[q]) : -1;
    }
  }
  if (bp_out && MULTI) {  // the waves' parts of every frame, in wave order (both directions wrote before the barrier)
    if (!DUAL) __syncthreads();
    for (int t = tall; t < Tb; t += NALL) {
      float s = bpart[(size_t)t * nwaves];
      for (int w = 1; w < nwaves; ++w) s += bpart[(size_t)t * nwaves + w];
      bp_out[t] = s;
    }
  }
}

}  // namespace

extern "C" size_t em_ctc_seq_posteriors_workspace_bytes(int32_t N, int32_t T, int32_t Lmax) {
  if (N <= 0 || T <= 0 || Lmax < 0 || Lmax > ctc_trellis::MAX_L) return 0;
  return (size_t)N * ws_floats_per_cand(ws_rows(T), row_states(Lmax), T, ctc_trellis::waves(Lmax)) * sizeof(float);
}

extern "C" int em_ctc_seq_posteriors(const float* lpT, int32_t ldT, const int32_t* xlens, int32_t Bm, int32_t T,
                                     const int32_t* targets, int32_t Lmax, const int32_t* ylens, const int32_t* mem_of,
                                     int32_t N, int32_t blank, float* nll, float* occ, float* peak, int32_t* peak_t,
                                     float* blank_post, void* ws, size_t ws_bytes, void* stream) {
  if (!lpT || !xlens || !ylens || !nll || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0 || blank < 0) return EM_ERR_BAD_ARG;
  if (Lmax > 0 && (!targets || !occ || !peak || !peak_t)) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if ((long)ldT < (long)Bm * T) return EM_ERR_BAD_ARG;
  if (Lmax > ctc_trellis::MAX_L) return EM_ERR_UNSUPPORTED;  // em_ctc_forced_align_max_tokens()
  if (ws && ((uintptr_t)ws & 15)) return EM_ERR_BAD_ARG;
  if (!ws || ws_bytes < em_ctc_seq_posteriors_workspace_bytes(N, T, Lmax)) return EM_ERR_UNSUPPORTED;
  const int nw = ctc_trellis::waves(Lmax);
  PostArgs a;
  a.lpT = lpT; a.xlens = xlens; a.targets = targets; a.ylens = ylens; a.mem_of = mem_of;
  a.ldT = ldT; a.Lmax = Lmax; a.T = T; a.Bm = Bm; a.blank = blank;
  a.vec = (ldT % 4 == 0) && (((uintptr_t)lpT & 15) == 0);
  a.RS = row_states(Lmax); a.R = ws_rows(T);
  a.nll = nll; a.occ = occ; a.peak = peak; a.peak_t = peak_t; a.blank_post = blank_post;
  a.ws = (float*)ws;
  if (nw == 1)
    hipLaunchKernelGGL((ctc_post_kernel<false, true>), dim3(N), dim3(64, 2), 0, (hipStream_t)stream, a);
  else if (nw <= CP_DUAL_WAVES)
    hipLaunchKernelGGL((ctc_post_kernel<true, true>), dim3(N), dim3(64 * nw, 2), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((ctc_post_kernel<true, false>), dim3(N), dim3(64 * nw), 0, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
