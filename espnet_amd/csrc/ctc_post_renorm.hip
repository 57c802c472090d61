// CTC forward-backward for long recordings: ctc_post.hip's token posteriors with alpha and beta RENORMALISED as the
// walks go.  The contract is include/espnet_amd.h's ("CTC token posteriors, renormalised"); the work split is
// ctc_post.hip's (one workgroup per candidate, the two directions in two wave groups that meet at one barrier, half
// trellises of f32 rows in the workspace read through a register ring, three walks in one group above S = 4 096).
//
// What differs.  A row of ctc_post.hip is an f32 logarithm of magnitude |nll|, so gamma = exp2(alpha + beta - e - P)
// loses |nll| * 2^-24 in every term.  Here a row is held RELATIVE to an integer offset O[t] (base-2 logarithm, so the
// shifts are exact): the cell of frame t is  lse(previous row) + (e - s[t]),  s[t] = O[t] - O[t-1] a wave-uniform
// integer, and  gamma = exp2((v + o - e) + float(Oa[t] + Ob[t] - Poff) - P_rel).  The bracket of offsets is a small
// exact integer; nothing of magnitude |nll| ever meets an f32.  A stored row goes to the workspace with its O[t] (one
// int32 per row, behind the rows), and comes back through the ring with it.
//
// The shift is off the dependent chain.  Per frame t (begin_frame, in front of the frame's cells):
//   * the lane maxima of frame t - 1 (taken behind its cells, over the states s < S only: the lanes above S hold values
//     that depend on the launch's width) are reduced over the wave by DPP into a scalar;
//   * with more waves than one that scalar goes to LDS (slot t & 1), and the scalars of frame t - 2 of all waves, which
//     lie behind the barrier the walk has per frame anyway, are read from the other slot and reduced (16 lanes, DPP);
//     one wave holds its scalar a frame longer instead, so that every form shifts alike;
//   * g = that maximum of frame t - 2, relative to O[t-2]:  s[t+1] = rint(g) - s[t] - s[t-1], that is
//     O[t+1] = O[t-2] + rint(g): the row of frame t + 1 is relative to the (rounded) maximum of frame t - 2.
// So a row's magnitude is what the maximum drifts in three frames (plus the row's own spread), every frame, and nothing
// a frame's cells wait for is younger than two frames.  The shifts are integer sums in SGPRs; e - s[t] is eight
// subtractions beside the chain.  A shift is clamped to +-8 192 (emissions below -5 000 nats per frame leave the row
// less than normalised, never wrong: O is exact whatever it is), so O fits an int32 for T up to 262 144.
// The schedule depends on the frame's position in its walk and on the candidate's own states only: a candidate's bits
// are the same in every form, beside any companions.
//
// nll = -ln 2 * (log2 of the last alpha row's two end states, relative, + O[T_b-1]), added in double once per candidate.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (ROCm 7.2): see DESIGN.md 4ad.
#include "ctc_post_common.h"

namespace {

using ctc_trellis::lse2;
using ctc_trellis::lse3;
using ctc_trellis::MAX_WAVES;
using ctc_trellis::NINF;
using ctc_trellis::SPL;
using namespace ctc_post_common;  // CP_DUAL_WAVES, the row geometry, lse_merge, TokAcc
// frames a stored row (and its offset) is loaded ahead of its use
template <bool MULTI>
constexpr int RN_RING = MULTI ? 1 : 3;
constexpr int RN_MAX_SHIFT = 8192;

struct RenormArgs {
  const float* lpT;
  const int32_t *xlens, *targets, *ylens, *mem_of;
  int32_t ldT, Lmax, T, Bm, blank, vec, RS, R;
  float *nll, *occ, *peak, *blank_post;
  int32_t* peak_t;
  float* ws;
};

// floats per candidate: the rows of both directions, blank_post's parts [T][waves] (more waves than one), the rows'
// offsets [2][R] (int32); each part 16-byte whole
__host__ __device__ static inline size_t rn_bparts(int T, int nw) { return nw > 1 ? ((size_t)T * nw + 3) & ~(size_t)3 : 0; }
__host__ __device__ static inline size_t rn_floats_per_cand(int R, int RS, int T, int nw) {
  return (size_t)2 * R * RS + rn_bparts(T, nw) + (((size_t)2 * R + 3) & ~(size_t)3);
}

__device__ __forceinline__ float uniform(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// max(x, x of the lane the DPP control names); a lane without such a source sees -inf
template <int CTRL>
__device__ __forceinline__ float dpp_max(float x) {
  const float y = __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, NINF), __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
  return fmaxf(x, y);
}
// lane 15 of every row of 16 lanes: the row's maximum
__device__ __forceinline__ float row_max(float x) {
  x = dpp_max<0x111>(x);  // row_shr:1
  x = dpp_max<0x112>(x);  // row_shr:2
  x = dpp_max<0x114>(x);  // row_shr:4
  return dpp_max<0x118>(x);  // row_shr:8
}
// the maximum over the 64 lanes, as a scalar
__device__ __forceinline__ float wave_max(float x) {
  x = row_max(x);
  x = dpp_max<0x142>(x);  // row_bcast:15: lane 15 of a row to the row above
  x = dpp_max<0x143>(x);  // row_bcast:31: lane 31 to the upper half
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// ctc_post.hip's cell with the row relative to O.  UP: the alpha direction (frames ascending).
template <bool MULTI, bool UP>
struct RenormCell {
  float* mine;           // this direction's rows of the candidate, [R][RS]
  const float* other;    // the opposite direction's
  int32_t* moff;         // this direction's offsets [R]
  const int32_t* ooff;   // the opposite direction's
  float* bpart;          // blank_post of the candidate: [T] (one wave) or the parts [T][waves]; null: not wanted
  float (*red)[2];       // LDS [MAX_WAVES][2]: the reduction of P over the waves of this direction
  float (*mx)[MAX_WAVES];  // LDS [2][MAX_WAVES]: the waves' row maxima, two frames in flight (MULTI)
  int RS, h, Tb, tid, nwaves, S;
  bool do_store, do_combine, meet_barrier;

  float v[SPL], e[SPL];  // the frame's cells (relative to O) and their emissions as loaded
  static constexpr int RING = RN_RING<MULTI>;
  f32x4 ring[RING][2];
  int ringo[RING];
  // the renormalisation: all wave-uniform
  int O, s_cur, s_prev, s_next, par;
  float shf, lm, held;
  // P(y|x) = 2^(P + Poff), taken at the first combined frame
  float P = 0.f;
  int Poff = 0;
  bool dead = false;
  TokAcc acc;

  static __device__ __forceinline__ f32x4 prepare(f32x4 x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __fmul_rn(x[i], ctc_trellis::LOG2E);
    return x;
  }

  // in front of a walk: offsets at 0, nothing in flight (the walk's opening barrier lies behind the LDS writes)
  __device__ __forceinline__ void begin() {
    O = s_cur = s_prev = s_next = par = 0;
    shf = 0.f, lm = NINF, held = NINF;
    if (MULTI && tid < 2 * MAX_WAVES) (&mx[0][0])[tid] = NINF;
  }
  // the lane's maximum of the row in v, over the states of the transcript
  __device__ __forceinline__ void lane_max() {
    const int nv = S - SPL * tid;
    float m = NINF;
#pragma unroll
    for (int j = 0; j < SPL; ++j) m = fmaxf(m, j < nv ? v[j] : NINF);
    lm = m;
  }
  // in front of the cells of a frame t: O becomes O[t]; the maximum of frame t - 2 decides s[t+1]
  __device__ __forceinline__ void begin_frame() {
    const float wm = wave_max(lm);  // frame t - 1
    float g;
    if (MULTI) {
      if ((tid & 63) == 0) mx[par][tid >> 6] = wm;
      // frame t - 2, every wave's (a row of 16 lanes holds them all; the slots of waves that do not run stay -inf)
      g = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, row_max(mx[par ^ 1][tid & 15])), 15));
      par ^= 1;
    } else {
      g = held;
      held = wm;
    }
    s_prev = s_cur;
    s_cur = s_next;
    O += s_cur;
    shf = uniform((float)s_cur);
    const float gc = fminf(fmaxf(g, -2.f * RN_MAX_SHIFT), 2.f * RN_MAX_SHIFT);  // -inf: a row without a live state
    const int want = __builtin_amdgcn_readfirstlane((int)__builtin_rintf(gc)) - s_cur - s_prev;
    s_next = g > NINF ? min(max(want, -RN_MAX_SHIFT), RN_MAX_SHIFT) : 0;
  }

  __device__ __forceinline__ float blank(int j, float stay, float one, float em) {
    if (j == 0) begin_frame();
    e[j] = em;
    return v[j] = lse2(stay, one) + (em - shf);
  }
  __device__ __forceinline__ float token(int j, float stay, float one, float two, float em) {
    e[j] = em;
    return v[j] = lse3(stay, one, two) + (em - shf);
  }

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc.occ[q] = 0.f, acc.peak[q] = 0.f, acc.pt[q] = -1;
  }
  __device__ __forceinline__ bool owns() const { return SPL * tid < RS; }
  // the workspace row of frame t: alpha rows by frame, beta rows from the frame behind the meeting frame
  __device__ __forceinline__ int own_row(int t) const { return UP ? t : t - (h + 1); }
  __device__ __forceinline__ int other_row(int t) const { return UP ? t - (h + 1) : t; }
  __device__ __forceinline__ void load(int k, int t) {
    const bool there = UP ? t < Tb : t >= 0, in = owns() && there;
    const f32x4 ninf = {NINF, NINF, NINF, NINF};
    const float* row = other + (size_t)other_row(t) * RS + SPL * tid;
    ring[k][0] = in ? *(const f32x4*)row : ninf;
    ring[k][1] = in ? *(const f32x4*)(row + 4) : ninf;
    ringo[k] = there ? ooff[other_row(t)] : 0;
  }
  __device__ __forceinline__ void store(int t) {
    if (tid == 0) moff[own_row(t)] = O;
    if (!owns()) return;
    f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    float* row = mine + (size_t)own_row(t) * RS + SPL * tid;
    *(f32x4*)row = a;
    *(f32x4*)(row + 4) = b;
  }
  // behind the last stored row of this direction: wait for the other direction's (ctc_post.hip's meet)
  __device__ __forceinline__ void meet() {
    if (meet_barrier) __syncthreads();
  }

  // log2 P(y|x), relative to the offsets of this frame, from its products over all lanes of the direction
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
    const int off = O + __builtin_amdgcn_readfirstlane(ringo[0]);  // of both rows of this frame
#pragma unroll
    for (int k = 0; k + 1 < RING; ++k) ring[k][0] = ring[k + 1][0], ring[k][1] = ring[k + 1][1], ringo[k] = ringo[k + 1];
    load(RING - 1, UP ? t + RING : t - RING);
    float x[SPL];  // log2 of alpha * beta / p, relative to off: both rows carry the frame's emission
#pragma unroll
    for (int j = 0; j < SPL; ++j) x[j] = (v[j] + o[j]) - fmaxf(e[j], -FLT_MAX);
    if (first) {
      total(x);
      Poff = off;
    }
    const float c = (float)(off - Poff) - P;  // a small exact integer, less the relative log2 P
    float g[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) g[j] = dead ? 0.f : __builtin_amdgcn_exp2f(x[j] + c);
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
    lane_max();
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
__global__ __launch_bounds__(MULTI ? 1024 : 128) void ctc_post_renorm_kernel(const RenormArgs a) {
  __shared__ float xa[2][MAX_WAVES];
  __shared__ float xb[2][MAX_WAVES][2];
  __shared__ float fin[2];
  __shared__ float red[2][MAX_WAVES][2];
  __shared__ float mx[2][2][MAX_WAVES];

  const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, T = a.T, Lmax = a.Lmax, RS = a.RS;
  const int dir = DUAL ? __builtin_amdgcn_readfirstlane((int)threadIdx.y) : 0;  // wave-uniform: whole waves per direction
  const int NALL = DUAL ? 2 * NT : NT, tall = dir * NT + tid;
  const int u = a.mem_of ? min(max(a.mem_of[n], 0), a.Bm - 1) : n;
  const int Tb = min(max(a.xlens[u], 0), T);
  const int L = min(max(a.ylens[n], 0), Lmax);
  const int nwaves = NT >> 6, h = (Tb - 1) >> 1, S = 2 * L + 1;
  const int32_t* y = a.targets + (size_t)n * Lmax;
  const long ldT = a.ldT, colb = (long)u * T;
  const bool vec = a.vec != 0;

  const size_t rows = (size_t)a.R * RS;
  float* wsn = a.ws + (size_t)n * rn_floats_per_cand(a.R, RS, T, nwaves);
  int32_t* offs = (int32_t*)(wsn + 2 * rows + rn_bparts(T, nwaves));
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

  RenormCell<MULTI, true> ca{wsn, wsn + rows, offs, offs + a.R, bpart, red[0], mx[0], RS, h, Tb, tid, nwaves, S, true, DUAL, DUAL};
  RenormCell<MULTI, false> cb{wsn + rows, wsn, offs + a.R, offs, bpart, red[1], mx[1], RS, h, Tb, tid, nwaves, S, true, true, DUAL};
  ca.init();
  cb.init();

  // frame 0 of alpha does not pass through the cell: its row is the two emissions, its offset 0
  auto alpha_walk = [&]() {
    ca.begin();
#pragma unroll
    for (int j = 0; j < SPL; ++j) ca.v[j] = NINF;
    if (tid == 0) {
      ca.v[0] = __fmul_rn(a.lpT[(size_t)a.blank * ldT + colb], ctc_trellis::LOG2E);
      if (L > 0) ca.v[1] = __fmul_rn(a.lpT[(size_t)y[0] * ldT + colb], ctc_trellis::LOG2E);
    }
    ca.lane_max();
    if (ca.do_store) ca.store(0);
    if (h == 0) ca.meet();
    ctc_trellis::forward<MULTI>(a.lpT, ldT, colb, vec, y, L, Tb, a.blank, xa, fin, ca);
    if (MULTI && Tb == 1) {  // no frame of the other half: the barriers of the reduction this direction never ran
      __syncthreads();
      __syncthreads();
    }
  };
  auto beta_walk = [&]() {
    cb.begin();
    ctc_trellis::backward<MULTI>(a.lpT, ldT, colb, vec, y, L, Tb, a.blank, xb, cb);
  };

  if (DUAL) {
    if (dir == 0)
      alpha_walk();
    else
      beta_walk();
  } else {
    ca.do_combine = false;
    alpha_walk();
    beta_walk();
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
  const float tot = lse2(fin[0], fin[1]);  // relative to alpha's last offset
  const bool path = tot > NINF;
  if (dir == 0) {
    // the one sum of magnitude |nll|: in double, so that the relative part is not lost
    if (tid == 0) a.nll[n] = path ? (float)(-0.69314718055994530942 * ((double)tot + (double)ca.O)) : INFINITY;
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

extern "C" size_t em_ctc_seq_posteriors_renorm_workspace_bytes(int32_t N, int32_t T, int32_t Lmax) {
  if (N <= 0 || T <= 0 || Lmax < 0 || Lmax > ctc_trellis::MAX_L) return 0;
  return (size_t)N * rn_floats_per_cand(ws_rows(T), row_states(Lmax), T, ctc_trellis::waves(Lmax)) * sizeof(float);
}

extern "C" int em_ctc_seq_posteriors_renorm(const float* lpT, int32_t ldT, const int32_t* xlens, int32_t Bm, int32_t T,
                                            const int32_t* targets, int32_t Lmax, const int32_t* ylens, const int32_t* mem_of,
                                            int32_t N, int32_t blank, float* nll, float* occ, float* peak, int32_t* peak_t,
                                            float* blank_post, void* ws, size_t ws_bytes, void* stream) {
  if (!lpT || !xlens || !ylens || !nll || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0 || blank < 0) return EM_ERR_BAD_ARG;
  if (Lmax > 0 && (!targets || !occ || !peak || !peak_t)) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if ((long)ldT < (long)Bm * T) return EM_ERR_BAD_ARG;
  if (Lmax > ctc_trellis::MAX_L) return EM_ERR_UNSUPPORTED;  // em_ctc_forced_align_max_tokens()
  if (ws && ((uintptr_t)ws & 15)) return EM_ERR_BAD_ARG;
  if (!ws || ws_bytes < em_ctc_seq_posteriors_renorm_workspace_bytes(N, T, Lmax)) return EM_ERR_UNSUPPORTED;
  const int nw = ctc_trellis::waves(Lmax);
  RenormArgs a;
  a.lpT = lpT; a.xlens = xlens; a.targets = targets; a.ylens = ylens; a.mem_of = mem_of;
  a.ldT = ldT; a.Lmax = Lmax; a.T = T; a.Bm = Bm; a.blank = blank;
  a.vec = (ldT % 4 == 0) && (((uintptr_t)lpT & 15) == 0);
  a.RS = row_states(Lmax); a.R = ws_rows(T);
  a.nll = nll; a.occ = occ; a.peak = peak; a.peak_t = peak_t; a.blank_post = blank_post;
  a.ws = (float*)ws;
  if (nw == 1)
    hipLaunchKernelGGL((ctc_post_renorm_kernel<false, true>), dim3(N), dim3(64, 2), 0, (hipStream_t)stream, a);
  else if (nw <= CP_DUAL_WAVES)
    hipLaunchKernelGGL((ctc_post_renorm_kernel<true, true>), dim3(N), dim3(64 * nw, 2), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((ctc_post_renorm_kernel<true, false>), dim3(N), dim3(64 * nw), 0, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
