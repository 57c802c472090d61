// espnet_amd — the vocabulary head that never materialises the [M][V] logits, on gfx950 (contracts: include/espnet_amd.h,
// "language model over whole sentences" and "Mask-CTC"; the format: DESIGN.md, "The vocabulary head").
//
//   y[r][v] = rows[r] . w[v] + bias[v],  rows = LayerNorm(x; g, be, eps 1e-12) of the f32 residual rows (LN) or the
//   activations as they are,
// and of a row's V logits only a record leaves a vocabulary tile: the maximum, the sum of exp(logit - maximum) and one
// more word.  The kernels are written once over the record `Rec`, a policy in the style of the cells of
// csrc/rnnt_lattice.h:
//   Rec::Out                       what the caller hands in and gets back (a kernel argument)
//   Rec::key(out, r, M)            what the record has to know of row r: its target, or nothing.  An int beside the
//                                  records, not a member: the 16 records of a lane stay three words each
//   Rec::init()                    the record before the first column
//   a.push<FAST>(val, col, key)    one more logit; a lane or thread meets its columns in ascending order
//   Rec::merge<FAST>(a, b)         the record of the union of two column sets
//   a.shfl_xor(o), a.pack(), Rec::unpack(float4)
//   Rec::skip(key)                 (f32) the row has nothing to compute: finish at once
//   a.meet4(red)                   (f32) the row's record from its four waves' records
//   a.finish(out, r, key)          the merged record of row r -> the outputs
// FAST: __expf (the bf16 path) against expf (the f32 parity path).  Two records exist:
//   TargetRec  + the logit of the row's target  -> em_lm_head_nll (nll = log-sum-exp - target logit);
//   TopRec     + the lowest arg-max             -> em_lm_head_top1 (max logit, arg-max) behind the LayerNorm,
//                                                  em_ctc_frame_top (arg-max, probability = 1 / sum-exp) without it.
// The transducer's joint keeps its own kernel (csrc/transducer.hip: a runner-up in the record, one column tile per
// workgroup, the waves split the joint dimension).
#include <limits.h>
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

using em_host::LN_EPS;

// ---- the part every record shares: (m, s) = (maximum, sum of exp(logit - m)) of a set of columns
template <bool FAST>
__device__ __forceinline__ void lse_push(float& m, float& s, float val) {
  if (FAST) {  // ONE exp per logit
    const float dlt = val - m;  // m = -inf at first: dlt = +inf, e = 0, s = 1
    const float e = __expf(-fabsf(dlt));
    s = dlt > 0.f ? s * e + 1.f : s + e;
    m = fmaxf(m, val);
  } else {
    const float mm = fmaxf(m, val);
    s = s * expf(m - mm) + expf(val - mm);  // m = -inf: 0 * 0
    m = mm;
  }
}
// the sum of the union; rm = fmaxf(am, bm)
template <bool FAST>
__device__ __forceinline__ float lse_merge(float am, float as, float bm, float bs, float rm) {
  const float ea = FAST ? __expf(am - rm) : expf(am - rm), eb = FAST ? __expf(bm - rm) : expf(bm - rm);
  return (am == -INFINITY ? 0.f : as * ea) + (bm == -INFINITY ? 0.f : bs * eb);
}

// ---- the target's logit (-inf while the target's column has not been met); the key is the row's target
struct TargetRec {
  struct Out {
    const int32_t* target;  // [M], < 0: the row is not scored
    float* nll;             // [M]
  };
  float m, s, t;
  static __device__ __forceinline__ int key(const Out& o, int r, int M) { return r < M ? o.target[r] : -1; }
  static __device__ __forceinline__ TargetRec init() { return TargetRec{-INFINITY, 0.f, -INFINITY}; }
  template <bool FAST>
  __device__ __forceinline__ void push(float val, int col, int tgt) {
    if (col == tgt) t = val;
    lse_push<FAST>(m, s, val);
  }
  template <bool FAST>
  static __device__ __forceinline__ TargetRec merge(TargetRec a, TargetRec b) {
    const float rm = fmaxf(a.m, b.m);
    return TargetRec{rm, lse_merge<FAST>(a.m, a.s, b.m, b.s, rm), fmaxf(a.t, b.t)};
  }
  __device__ __forceinline__ TargetRec shfl_xor(int o) const {
    return TargetRec{__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(t, o, 64)};
  }
  __device__ __forceinline__ float4 pack() const { return make_float4(m, s, t, 0.f); }
  static __device__ __forceinline__ TargetRec unpack(float4 p) { return TargetRec{p.x, p.y, p.z}; }
  static __device__ __forceinline__ bool skip(int tgt) { return tgt < 0; }
  // the maximum of the four first, then one sum
  __device__ __forceinline__ void meet4(const float (*red)[3]) {
    float mm = -INFINITY, tt = -INFINITY, ss = 0.f;
    for (int i = 0; i < 4; ++i) mm = fmaxf(mm, red[i][0]), tt = fmaxf(tt, red[i][2]);
    for (int i = 0; i < 4; ++i) ss += red[i][0] == -INFINITY ? 0.f : red[i][1] * expf(red[i][0] - mm);
    m = mm, s = ss, t = tt;
  }
  __device__ __forceinline__ void finish(const Out& o, int r, int tgt) const {
    o.nll[r] = tgt < 0 ? 0.f : (m + logf(s)) - t;
  }
};

// ---- the lowest column that holds the maximum (csrc/transducer.hip Top without the runner-up)
struct TopRec {
  struct Out {
    float* val;    // [M] the maximum logit, or (as_prob) the probability the maximum has under the softmax
    int32_t* idx;  // [M] the arg-max
    int as_prob;
  };
  float m, s;
  int i;
  static __device__ __forceinline__ int key(const Out&, int, int) { return 0; }
  static __device__ __forceinline__ TopRec init() { return TopRec{-INFINITY, 0.f, INT_MAX}; }
  template <bool FAST>
  __device__ __forceinline__ void push(float val, int col, int) {
    if (val > m) i = col;  // columns in ascending order: `>` keeps the lowest of equals
    lse_push<FAST>(m, s, val);
  }
  template <bool FAST>
  static __device__ __forceinline__ TopRec merge(TopRec a, TopRec b) {
    const float rm = fmaxf(a.m, b.m);
    return TopRec{rm, lse_merge<FAST>(a.m, a.s, b.m, b.s, rm), (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b.i : a.i};
  }
  __device__ __forceinline__ TopRec shfl_xor(int o) const {
    return TopRec{__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(i, o, 64)};
  }
  __device__ __forceinline__ float4 pack() const { return make_float4(m, s, __int_as_float(i), 0.f); }
  static __device__ __forceinline__ TopRec unpack(float4 p) { return TopRec{p.x, p.y, __float_as_int(p.z)}; }
  static __device__ __forceinline__ bool skip(int) { return false; }
  // pairwise, wave 0 first
  __device__ __forceinline__ void meet4(const float (*red)[3]) {
    *this = unpack(make_float4(red[0][0], red[0][1], red[0][2], 0.f));
    for (int w = 1; w < 4; ++w) *this = merge<false>(*this, unpack(make_float4(red[w][0], red[w][1], red[w][2], 0.f)));
  }
  __device__ __forceinline__ void finish(const Out& o, int r, int) const {
    o.val[r] = o.as_prob ? 1.0f / s : m;
    o.idx[r] = i;
  }
};

// a record in three words of LDS
template <class Rec>
__device__ __forceinline__ void put3(float* dst, Rec a) {
  const float4 p = a.pack();
  dst[0] = p.x;
  dst[1] = p.y;
  dst[2] = p.z;
}
template <class Rec>
__device__ __forceinline__ Rec get3(const float* src) {
  return Rec::unpack(make_float4(src[0], src[1], src[2], 0.f));
}

// mean and 1 / standard deviation of the row xr [d] by one wave (transformer/layer_norm.py, eps 1e-12)
__device__ __forceinline__ void row_stats(const float* xr, int d, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c];
  mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float t = xr[c] - mean;
    q += t * t;
  }
  rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
}

constexpr int HEAD_ROWS = 64;    // rows of a workgroup: four 16-row MFMA tiles
constexpr int HEAD_SLICE = 512;  // vocabulary columns of a workgroup: 8 tiles of 16 for each of its 4 waves
constexpr int HEAD_DMAX = 1024;  // 64 rows of d + 8 bf16 stay inside the 160 KiB of LDS

// bf16: workgroup (slice, row block) = 64 rows x 512 vocabulary columns.  The rows enter LDS once as bf16 (LN: normalised
// from the f32 residual rows; otherwise copied from the bf16 activations), rows padded by 16 bytes against bank conflicts;
// wave w then takes the column tiles w, w + 4, ... of the slice: the weight fragment of a k-step comes straight from global
// memory and meets the four row tiles' fragments from LDS.  A lane keeps the records of its 16 (row, column lr) pairs across
// tiles with ONE exp per logit; the 16 lanes of a row group, then the four waves, merge once at the end and part[row][slice]
// receives the record.  Columns >= V count as -inf, rows >= M are zeros and never stored.
template <class Rec, bool LN>
__global__ __launch_bounds__(256) void head_rows_bf16_kernel(const void* __restrict__ xv, const float* __restrict__ g,
                                                             const float* __restrict__ be, const bf16* __restrict__ w,
                                                             const float* __restrict__ bias, const typename Rec::Out out,
                                                             int M, int V, int d, float4* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
  __shared__ float red[4][HEAD_ROWS][3];
  bf16* xs = (bf16*)head_smem;
  const int ldx = d + 8;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int r0 = blockIdx.y * HEAD_ROWS;
  for (int i = 0; i < 16; ++i) {
    const int rl = wave * 16 + i, r = r0 + rl;
    bf16* dst = xs + (size_t)rl * ldx;
    if (r >= M) {
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)0.f;
    } else if (LN) {
      const float* xr = (const float*)xv + (size_t)r * d;
      float mean, rstd;
      row_stats(xr, d, lane, mean, rstd);
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)((xr[c] - mean) * rstd * g[c] + be[c]);
    } else {
      const bf16* xr = (const bf16*)xv + (size_t)r * d;
      for (int c = lane; c < d; c += 64) dst[c] = xr[c];
    }
  }
  __syncthreads();
  Rec rec[4][4];
  int key[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rec[rt][q] = Rec::init();
      key[rt][q] = Rec::key(out, r0 + rt * 16 + lg * 4 + q, M);
    }
  const int vs0 = blockIdx.x * HEAD_SLICE;
  const int nk = d / 32;
  for (int t = wave; t < HEAD_SLICE / 16; t += 4) {
    const int v0 = vs0 + t * 16;
    if (v0 >= V) break;
    const int col = v0 + lr;
    const bf16* wrow = w + (size_t)min(col, V - 1) * d + lg * 8;
    const bf16* arow = xs + (size_t)lr * ldx + lg * 8;
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nk; ++s) {
      const bf16x8 bf = *(const bf16x8*)(wrow + s * 32);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt] = Mma<bf16>::mma(*(const bf16x8*)(arow + (size_t)rt * 16 * ldx + s * 32), bf, acc[rt]);
    }
    if (col < V) {
      const float bb = bias[col];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) rec[rt][q].template push<true>(acc[rt][q] + bb, col, key[rt][q]);
    }
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Rec a = rec[rt][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) a = Rec::template merge<true>(a, a.shfl_xor(o));
      if (lr == 0) put3(red[wave][rt * 16 + lg * 4 + q], a);
    }
  __syncthreads();
  if (threadIdx.x < HEAD_ROWS && r0 + (int)threadIdx.x < M) {
    const int rl = threadIdx.x;
    Rec a = get3<Rec>(red[0][rl]);
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) a = Rec::template merge<true>(a, get3<Rec>(red[wv][rl]));
    part[(size_t)(r0 + rl) * gridDim.x + blockIdx.x] = a.pack();
  }
}

// a row's per-slice records -> its outputs
template <class Rec>
__global__ void head_merge_kernel(const float4* __restrict__ part, const typename Rec::Out out, int M, int nsl) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  Rec a = Rec::init();
  for (int i = 0; i < nsl; ++i) a = Rec::template merge<true>(a, Rec::unpack(part[(size_t)r * nsl + i]));
  a.finish(out, r, Rec::key(out, r, M));
}

// f32 (parity path): a workgroup per row, the (normalised) row in LDS, thread t walks the columns t, t + 256, ...
template <class Rec, bool LN>
__global__ __launch_bounds__(256) void head_rows_f32_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ be, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const typename Rec::Out out,
                                                            int V, int d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
  __shared__ float red[4][3];
  __shared__ float stat[2];
  float* xn = (float*)head_smem;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int key = Rec::key(out, r, r + 1);  // (the grid is the M rows)
  Rec a = Rec::init();
  if (Rec::skip(key)) {  // (workgroup-uniform)
    if (tid == 0) a.finish(out, r, key);
    return;
  }
  const float* xr = x + (size_t)r * d;
  if (LN) {
    if (wave == 0) {
      float mean, rstd;
      row_stats(xr, d, lane, mean, rstd);
      if (lane == 0) {
        stat[0] = mean;
        stat[1] = rstd;
      }
    }
    __syncthreads();
    for (int c = tid; c < d; c += 256) xn[c] = (xr[c] - stat[0]) * stat[1] * g[c] + be[c];
  } else {
    for (int c = tid; c < d; c += 256) xn[c] = xr[c];
  }
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    const float* wr = w + (size_t)v * d;
    float s = 0.f;
    for (int c = 0; c < d; ++c) s += xn[c] * wr[c];
    a.template push<false>(s + bias[v], v, key);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) a = Rec::template merge<false>(a, a.shfl_xor(o));
  if (lane == 0) put3(red[wave], a);
  __syncthreads();
  if (tid == 0) {
    a.meet4(red);
    a.finish(out, r, key);
  }
}

int head_slices(int V) { return em_cdiv(V, HEAD_SLICE); }

// part [M][slices] float4
size_t head_ws_bytes(int dtype, int32_t M, int32_t V) {
  if (dtype != EM_BF16 || M <= 0 || V <= 0) return 0;
  return (size_t)M * head_slices(V) * sizeof(float4);
}

// the rows x [M][d] (LN: f32 residual rows through LayerNorm(g, be); otherwise rows in the compute dtype) -> out
template <class Rec, bool LN>
int head_launch(int dtype, const void* x, const float* g, const float* be, const void* w, const float* bias,
                const typename Rec::Out& out, int M, int V, int d, void* ws, size_t ws_bytes, void* stream) {
  static EmLdsCap cap;  // (one per instantiation)
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_F32) {
    if ((size_t)d * 4 > 64 * 1024) return EM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((head_rows_f32_kernel<Rec, LN>), dim3(M), dim3(256), (size_t)d * 4, s, (const float*)x, g, be,
                       (const float*)w, bias, out, V, d);
    EM_CHECK_LAUNCH();
    return EM_OK;
  }
  if (dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (d % 32 || d > HEAD_DMAX) return EM_ERR_UNSUPPORTED;
  const int nsl = head_slices(V);
  if (em_cdiv(M, HEAD_ROWS) > 65535) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < head_ws_bytes(dtype, M, V)) return EM_ERR_WORKSPACE;
  const size_t lds = (size_t)HEAD_ROWS * (d + 8) * 2;
  EM_TRY(em_raise_lds_cap((const void*)head_rows_bf16_kernel<Rec, LN>, lds, &cap));
  hipLaunchKernelGGL((head_rows_bf16_kernel<Rec, LN>), dim3(nsl, em_cdiv(M, HEAD_ROWS)), dim3(256), lds, s, x, g, be,
                     (const bf16*)w, bias, out, M, V, d, (float4*)ws);
  hipLaunchKernelGGL(head_merge_kernel<Rec>, dim3(em_cdiv(M, 256)), dim3(256), 0, s, (const float4*)ws, out, M, nsl);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" size_t em_lm_head_nll_workspace_bytes(int dtype, int32_t M, int32_t V) { return head_ws_bytes(dtype, M, V); }

extern "C" int em_lm_head_nll(int dtype, const float* xrows, const float* norm_g, const float* norm_b, const void* out_w,
                              const float* out_b, const int32_t* target, int32_t M, int32_t V, int32_t d, float* nll,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!xrows || !norm_g || !norm_b || !out_w || !out_b || !target || !nll || M <= 0 || V <= 0 || d <= 0)
    return EM_ERR_BAD_ARG;
  return head_launch<TargetRec, true>(dtype, xrows, norm_g, norm_b, out_w, out_b, {target, nll}, M, V, d, ws, ws_bytes,
                                      stream);
}

extern "C" size_t em_lm_head_top1_workspace_bytes(int dtype, int32_t M, int32_t V) { return head_ws_bytes(dtype, M, V); }

extern "C" int em_lm_head_top1(int dtype, const float* xrows, const float* norm_g, const float* norm_b, const void* out_w,
                               const float* out_b, int32_t M, int32_t V, int32_t d, float* smax, int32_t* amax, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!xrows || !norm_g || !norm_b || !out_w || !out_b || !smax || !amax || M <= 0 || V <= 0 || d <= 0) return EM_ERR_BAD_ARG;
  return head_launch<TopRec, true>(dtype, xrows, norm_g, norm_b, out_w, out_b, {smax, amax, 0}, M, V, d, ws, ws_bytes,
                                   stream);
}

extern "C" size_t em_ctc_frame_top_workspace_bytes(int dtype, int32_t M, int32_t V) { return head_ws_bytes(dtype, M, V); }

extern "C" int em_ctc_frame_top(int dtype, const void* enc_act, const void* ctc_w, const float* ctc_b, int32_t M, int32_t V,
                                int32_t d, int32_t* ids, float* prob, void* ws, size_t ws_bytes, void* stream) {
  if (!enc_act || !ctc_w || !ctc_b || !ids || !prob || M <= 0 || V <= 0 || d <= 0) return EM_ERR_BAD_ARG;
  return head_launch<TopRec, false>(dtype, enc_act, nullptr, nullptr, ctc_w, ctc_b, {prob, ids, 1}, M, V, d, ws, ws_bytes,
                                    stream);
}
