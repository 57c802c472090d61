// espnet_amd — the TransformerLM over whole sentences on gfx950: per-token negative log-likelihoods of a batch in one
// enqueue (contract: include/espnet_amd.h, "language model over whole sentences").  Reference:
// espnet2/lm/espnet_model.py ESPnetLanguageModel.nll, espnet2/lm/transformer_lm.py TransformerLM.forward (Encoder with
// input_layer="linear", `_target_mask`: query j sees the keys k <= j whose token id is not 0).
//
// The search's step path (csrc/search.hip lm_step) feeds one position per call, ~6 launches per layer and position.  A
// sentence that is known beforehand needs none of that chain: everything but the attention is row-local, so the
// M = B * Lp rows go through the library's GEMMs at once, and two kernels here do the rest:
//   lm_causal_attn_*  causal self-attention with the id-0 key mask, a wave per 16 queries of one (sentence, head);
//   lm_head_nll_*     after_norm + vocabulary projection + log-sum-exp + the target's logit: the [M][V] logits never
//                     exist, a row's running (max, sum-exp, target logit) is all that leaves a vocabulary tile.
#include <math.h>

#include "em_common.h"
#include "enc_host.h"

namespace {

using em_host::Bump;
using em_host::gemm;
using em_host::LN_EPS;

// ---- input layer tail on all rows: torch LayerNorm(1e-5) -> ReLU -> optional x * sqrt(d) + pe[row % Lp], in place on
// x [M][d] f32 (csrc/decoder.hip lm_input_norm_kernel with the position taken from the row).  One wave per row.
__global__ __launch_bounds__(256) void lm_seq_input_norm_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                                const float* __restrict__ b, const float* __restrict__ pe,
                                                                int M, int d, int Lp) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int pos = row % Lp;
  float* xr = x + (size_t)row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float t = xr[c] - mean;
    q += t * t;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + 1e-5f);
  const float xs = sqrtf((float)d);
  for (int c = lane; c < d; c += 64) {
    float v = fmaxf((xr[c] - mean) * rstd * g[c] + b[c], 0.f);
    if (pe) v = v * xs + pe[(size_t)pos * d + c];
    xr[c] = v;
  }
}

// ---- causal self-attention, bf16 on the matrix cores.  One wave owns 16 queries q0 .. q0 + 15 of one (sentence, head) and
// walks the keys 0 .. q0 + 15 in tiles of 32, no further (the diagonal).  Both products are taken transposed so that a
// lane's query never changes:
//   S^T[key][query] = K . Q^T   A = K rows (straight from global memory), B = Q (registers): lane (lr, lg) ends up with the
//                               scores of query q0 + lr against the keys 16 kt + 4 lg + reg, kt = 0 | 1;
//   O^T[dv][query]  = V^T . P^T B = the lane's own eight probabilities (element 4 kt + reg of lane group lg is key
//                               16 kt + 4 lg + reg - the A operand uses the same numbering, so no value changes lanes),
//                               A = V^T read from the 32 x DK tile of V in LDS.
// The running maximum is shared by the four lane groups of a query (they all scale the same accumulators), the running sum is
// per lane and meets at the end.  A masked key (beyond the diagonal, id 0, or past Lp) takes p = 0.0 exactly; a query with no
// visible key writes zeros.  LDS: one V tile, 4.5 KiB at DK = 64, whatever Lp is.
// CAUSAL = false (em_dec_full_attention, the MLM decoder): no diagonal, x [B] holds the sentences' lengths and query (b, j)
// sees the keys below x[b]; the V rows of the keys behind it enter LDS as zeros (0.0 * whatever lies there would not be 0).
template <int DK, bool CAUSAL>
__global__ __launch_bounds__(64) void lm_causal_attn_bf16_kernel(const bf16* __restrict__ qkv, const int32_t* __restrict__ x,
                                                                 int Lp, int d, bf16* __restrict__ ctx) {
  constexpr int NC = DK / 32, ND = DK / 16, VLD = DK + 8;
  __shared__ __attribute__((aligned(16))) bf16 vs[32 * VLD];
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const size_t row0 = (size_t)b * Lp;
  const size_t ld = (size_t)3 * d;
  const int qi = q0 + lr;
  const bf16* qrow = qkv + (row0 + min(qi, Lp - 1)) * ld + h * DK + lg * 8;
  bf16x8 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) qf[c] = *(const bf16x8*)(qrow + c * 32);
  const float scale = 1.0f / sqrtf((float)DK);
  float m = -INFINITY, l = 0.f;
  f32x4 acc[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int kend = CAUSAL ? min(q0 + 16, Lp) : min(max(x[b], 0), Lp);
  for (int k0 = 0; k0 < kend; k0 += 32) {
    __syncthreads();  // the previous tile's V is read
    for (int i = lane; i < 32 * (DK / 8); i += 64) {
      const int kr = i / (DK / 8), cc = i % (DK / 8);
      const bf16* src = qkv + (row0 + min(k0 + kr, Lp - 1)) * ld + 2 * d + h * DK + cc * 8;
      bf16x8 v = *(const bf16x8*)src;
      if (!CAUSAL && k0 + kr >= kend) v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      *(bf16x8*)(vs + kr * VLD + cc * 8) = v;
    }
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const bf16* krow = qkv + (row0 + min(k0 + kt * 16 + lr, Lp - 1)) * ld + d + h * DK + lg * 8;
#pragma unroll
      for (int c = 0; c < NC; ++c) s[kt] = Mma<bf16>::mma(*(const bf16x8*)(krow + c * 32), qf[c], s[kt]);
    }
    float sc[8];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + (j >> 2) * 16 + lg * 4 + (j & 3);
      const bool ok = CAUSAL ? key <= qi && key < Lp && x[row0 + min(key, Lp - 1)] != 0 : key < kend;
      sc[j] = ok ? s[j >> 2][j & 3] * scale : -INFINITY;
      tmax = fmaxf(tmax, sc[j]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __expf(m - m_use);  // m = -inf: 0
    m = m_new;
    bf16x8 pf;
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = sc[j] == -INFINITY ? 0.f : __expf(sc[j] - m_use);
      psum += p;
      pf[j] = (bf16)p;
    }
    l = l * alpha + psum;
    __syncthreads();  // the V tile is in LDS
#pragma unroll
    for (int t = 0; t < ND; ++t) {
      bf16x8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = vs[((j >> 2) * 16 + lg * 4 + (j & 3)) * VLD + t * 16 + lr];
      acc[t] = Mma<bf16>::mma(vf, pf, acc[t] * alpha);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi >= Lp) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  bf16* out = ctx + (row0 + qi) * (size_t)d + h * DK + lg * 4;
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (bf16)(acc[t][r] * inv);
    *(bf16x4*)(out + t * 16) = o;
  }
}

// ---- the same attention in f32, plain (parity path): one wave per (query, head, sentence).  Pass 1 finds the row maximum,
// pass 2 recomputes the scores 64 keys at a time and lets lane c < dk accumulate channel c of the context.  CAUSAL = false:
// the keys below the sentence's length x[b], whatever the query.
template <bool CAUSAL>
__global__ __launch_bounds__(64) void lm_causal_attn_f32_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ x,
                                                                int Lp, int d, int dk, float* __restrict__ ctx) {
  const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const size_t row0 = (size_t)b * Lp;
  const size_t ld = (size_t)3 * d;
  const float* q = qkv + (row0 + j) * ld + h * dk;
  const float scale = 1.0f / sqrtf((float)dk);
  float* out = ctx + (row0 + j) * (size_t)d + h * dk;
  const int nkey = CAUSAL ? j + 1 : min(max(x[b], 0), Lp);  // the keys 0 .. nkey - 1 can be seen
  float m = -INFINITY;
  for (int k = lane; k < nkey; k += 64) {
    if (CAUSAL && x[row0 + k] == 0) continue;
    const float* kr = qkv + (row0 + k) * ld + d + h * dk;
    float s = 0.f;
    for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
    m = fmaxf(m, s * scale);
  }
  m = wave_max(m);
  if (m == -INFINITY) {  // no visible key
    if (lane < dk) out[lane] = 0.f;
    return;
  }
  float lsum = 0.f, acc = 0.f;
  for (int k0 = 0; k0 < nkey; k0 += 64) {
    const int k = k0 + lane;
    float p = 0.f;
    if (k < nkey && (!CAUSAL || x[row0 + k] != 0)) {
      const float* kr = qkv + (row0 + k) * ld + d + h * dk;
      float s = 0.f;
      for (int c = 0; c < dk; ++c) s += q[c] * kr[c];
      p = expf(s * scale - m);
    }
    lsum += p;
    const int n = min(64, nkey - k0);
    for (int kk = 0; kk < n; ++kk) {
      const float pk = __shfl(p, kk, 64);
      if (lane < dk) acc += pk * qkv[(row0 + k0 + kk) * ld + 2 * d + h * dk + lane];
    }
  }
  lsum = wave_sum(lsum);
  if (lane < dk) out[lane] = acc / lsum;
}

// ---- vocabulary head.  A row's record over a set of columns: the maximum logit, the sum of exp(logit - maximum) and the
// target's logit (-inf while the target's column has not been met).
struct Lse {
  float m, s, t;
};
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
  Lse r;
  r.m = fmaxf(a.m, b.m);
  r.t = fmaxf(a.t, b.t);
  r.s = (a.m == -INFINITY ? 0.f : a.s * __expf(a.m - r.m)) + (b.m == -INFINITY ? 0.f : b.s * __expf(b.m - r.m));
  return r;
}
__device__ __forceinline__ Lse lse_shfl_xor(Lse v, int o) {
  return Lse{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64), __shfl_xor(v.t, o, 64)};
}

constexpr int HEAD_ROWS = 64;    // rows of a workgroup: four 16-row MFMA tiles
constexpr int HEAD_SLICE = 512;  // vocabulary columns of a workgroup: 8 tiles of 16 for each of its 4 waves
constexpr int HEAD_DMAX = 1024;  // 64 rows of d + 8 bf16 stay inside the 160 KiB of LDS

// bf16: workgroup (slice, row block) = 64 rows x 512 vocabulary columns.  The rows are normalised once (after_norm) into
// LDS as bf16, rows padded by 16 bytes against bank conflicts; wave w then takes the column tiles w, w + 4, ... of the slice:
// the weight fragment of a k-step comes straight from global memory and meets the four row tiles' fragments from LDS.  A lane
// keeps the records of its 16 (row, column lr) pairs across tiles with ONE exp per logit; the 16 lanes of a row group, then the
// four waves, merge once at the end and part[row][slice] receives the record.  Columns >= V count as -inf, rows >= M are zeros
// and never stored.
__global__ __launch_bounds__(256) void lm_head_nll_bf16_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                               const float* __restrict__ be, const bf16* __restrict__ w,
                                                               const float* __restrict__ bias, const int32_t* __restrict__ target,
                                                               int M, int V, int d, float4* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_head_smem[];
  __shared__ float red[4][HEAD_ROWS][3];
  bf16* xs = (bf16*)lm_head_smem;
  const int ldx = d + 8;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int r0 = blockIdx.y * HEAD_ROWS;
  for (int i = 0; i < 16; ++i) {
    const int rl = wave * 16 + i, r = r0 + rl;
    bf16* dst = xs + (size_t)rl * ldx;
    if (r < M) {
      const float* xr = x + (size_t)r * d;
      float s = 0.f;
      for (int c = lane; c < d; c += 64) s += xr[c];
      const float mean = wave_sum(s) / (float)d;
      float q = 0.f;
      for (int c = lane; c < d; c += 64) {
        const float t = xr[c] - mean;
        q += t * t;
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)((xr[c] - mean) * rstd * g[c] + be[c]);
    } else {
      for (int c = lane; c < d; c += 64) dst[c] = (bf16)0.f;
    }
  }
  __syncthreads();
  Lse rec[4][4];
  int tg[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + rt * 16 + lg * 4 + q;
      rec[rt][q] = Lse{-INFINITY, 0.f, -INFINITY};
      tg[rt][q] = r < M ? target[r] : -1;
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
        for (int q = 0; q < 4; ++q) {
          const float val = acc[rt][q] + bb;
          Lse& a = rec[rt][q];
          if (col == tg[rt][q]) a.t = val;
          const float dlt = val - a.m;  // a.m = -inf at first: dlt = +inf, e = 0, s = 1
          const float e = __expf(-fabsf(dlt));
          a.s = dlt > 0.f ? a.s * e + 1.f : a.s + e;
          a.m = fmaxf(a.m, val);
        }
    }
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Lse a = rec[rt][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) a = lse_merge(a, lse_shfl_xor(a, o));
      if (lr == 0) {
        float* dst = red[wave][rt * 16 + lg * 4 + q];
        dst[0] = a.m;
        dst[1] = a.s;
        dst[2] = a.t;
      }
    }
  __syncthreads();
  if (threadIdx.x < HEAD_ROWS && r0 + (int)threadIdx.x < M) {
    const int rl = threadIdx.x;
    Lse a{red[0][rl][0], red[0][rl][1], red[0][rl][2]};
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) a = lse_merge(a, Lse{red[wv][rl][0], red[wv][rl][1], red[wv][rl][2]});
    part[(size_t)(r0 + rl) * gridDim.x + blockIdx.x] = make_float4(a.m, a.s, a.t, 0.f);
  }
}

// nll[r] = logsumexp - target logit from the row's per-slice records; target < 0: 0.0
__global__ void lm_head_merge_kernel(const float4* __restrict__ part, const int32_t* __restrict__ target, int M, int nsl,
                                     float* __restrict__ nll) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  if (target[r] < 0) {
    nll[r] = 0.f;
    return;
  }
  Lse a{-INFINITY, 0.f, -INFINITY};
  for (int i = 0; i < nsl; ++i) {
    const float4 p = part[(size_t)r * nsl + i];
    a = lse_merge(a, Lse{p.x, p.y, p.z});
  }
  nll[r] = (a.m + logf(a.s)) - a.t;
}

// f32 (parity path): a workgroup per row.  The normalised row sits in LDS, thread t walks the columns t, t + 256, ...
__global__ __launch_bounds__(256) void lm_head_nll_f32_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                              const float* __restrict__ be, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const int32_t* __restrict__ target,
                                                              int V, int d, float* __restrict__ nll) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_head_smem[];
  __shared__ float red[4][3];
  __shared__ float stat[2];
  float* xn = (float*)lm_head_smem;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tgt = target[r];
  if (tgt < 0) {  // (workgroup-uniform)
    if (tid == 0) nll[r] = 0.f;
    return;
  }
  const float* xr = x + (size_t)r * d;
  if (wave == 0) {
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float t = xr[c] - mean;
      q += t * t;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
    if (lane == 0) {
      stat[0] = mean;
      stat[1] = rstd;
    }
  }
  __syncthreads();
  for (int c = tid; c < d; c += 256) xn[c] = (xr[c] - stat[0]) * stat[1] * g[c] + be[c];
  __syncthreads();
  Lse a{-INFINITY, 0.f, -INFINITY};
  for (int v = tid; v < V; v += 256) {
    const float* wr = w + (size_t)v * d;
    float s = 0.f;
    for (int c = 0; c < d; ++c) s += xn[c] * wr[c];
    const float val = s + bias[v];
    if (v == tgt) a.t = val;
    const float mm = fmaxf(a.m, val);
    a.s = a.s * expf(a.m - mm) + expf(val - mm);  // a.m = -inf: 0 * 0
    a.m = mm;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Lse b = lse_shfl_xor(a, o);
    Lse m;
    m.m = fmaxf(a.m, b.m);
    m.t = fmaxf(a.t, b.t);
    m.s = (a.m == -INFINITY ? 0.f : a.s * expf(a.m - m.m)) + (b.m == -INFINITY ? 0.f : b.s * expf(b.m - m.m));
    a = m;
  }
  if (lane == 0) {
    red[wave][0] = a.m;
    red[wave][1] = a.s;
    red[wave][2] = a.t;
  }
  __syncthreads();
  if (tid == 0) {
    float mm = -INFINITY, t = -INFINITY, s = 0.f;
    for (int i = 0; i < 4; ++i) mm = fmaxf(mm, red[i][0]), t = fmaxf(t, red[i][2]);
    for (int i = 0; i < 4; ++i) s += red[i][0] == -INFINITY ? 0.f : red[i][1] * expf(red[i][0] - mm);
    nll[r] = (mm + logf(s)) - t;
  }
}

EmLdsCap head_cap;

int head_slices(int V) { return em_cdiv(V, HEAD_SLICE); }

struct SeqWs {
  size_t e, x, xn, qkv, ctx, h, head, total;
};
SeqWs seq_layout(int dtype, const EmLmWeights* lm, size_t M) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  Bump b;
  SeqWs s;
  s.e = b.take(M * lm->embed_unit * es);
  s.x = b.take(M * lm->d * 4);
  s.xn = b.take(M * lm->d * es);
  s.qkv = b.take(M * 3 * lm->d * es);
  s.ctx = b.take(M * lm->d * es);
  s.h = b.take(M * lm->ff * es);
  s.head = b.take(em_lm_head_nll_workspace_bytes(dtype, (int32_t)M, lm->vocab));
  s.total = b.o;
  return s;
}

// M rows and the widest activation row stay inside 31-bit element offsets (the GEMMs' buffer resources)
bool seq_shape_ok(const EmLmWeights* lm, int B, int Lp) {
  if (B <= 0 || Lp <= 0 || B > 65535) return false;
  const size_t wide = (size_t)(lm->ff > 3 * lm->d ? lm->ff : 3 * lm->d);
  return (size_t)B * Lp * wide * 4 < ((size_t)1 << 31);
}

// the launch of both attentions: x is the token array of the causal form, the lengths of the full one
template <bool CAUSAL>
int seq_attention(int dtype, const void* qkv, const int32_t* x, int32_t B, int32_t Lp, int32_t d, int32_t heads, void* ctx,
                  void* stream) {
  if (!qkv || !x || !ctx || B <= 0 || Lp <= 0 || d <= 0 || heads <= 0 || d % heads) return EM_ERR_BAD_ARG;
  const int dk = d / heads;
  if (dk != 32 && dk != 64) return EM_ERR_UNSUPPORTED;
  if (B > 65535 || heads > 65535) return EM_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) {
    const dim3 grid(em_cdiv(Lp, 16), heads, B);
    if (dk == 64)
      hipLaunchKernelGGL((lm_causal_attn_bf16_kernel<64, CAUSAL>), grid, dim3(64), 0, s, (const bf16*)qkv, x, Lp, d,
                         (bf16*)ctx);
    else
      hipLaunchKernelGGL((lm_causal_attn_bf16_kernel<32, CAUSAL>), grid, dim3(64), 0, s, (const bf16*)qkv, x, Lp, d,
                         (bf16*)ctx);
  } else if (dtype == EM_F32) {
    hipLaunchKernelGGL(lm_causal_attn_f32_kernel<CAUSAL>, dim3(Lp, heads, B), dim3(64), 0, s, (const float*)qkv, x, Lp, d, dk,
                       (float*)ctx);
  } else {
    return EM_ERR_BAD_ARG;
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" int em_lm_causal_attention(int dtype, const void* qkv, const int32_t* x, int32_t B, int32_t Lp, int32_t d,
                                      int32_t heads, void* ctx, void* stream) {
  return seq_attention<true>(dtype, qkv, x, B, Lp, d, heads, ctx, stream);
}

// (contract: include/espnet_amd.h, "Mask-CTC")
extern "C" int em_dec_full_attention(int dtype, const void* qkv, const int32_t* lens, int32_t B, int32_t Lp, int32_t d,
                                     int32_t heads, void* ctx, void* stream) {
  return seq_attention<false>(dtype, qkv, lens, B, Lp, d, heads, ctx, stream);
}

extern "C" size_t em_lm_head_nll_workspace_bytes(int dtype, int32_t M, int32_t V) {
  if (dtype != EM_BF16 || M <= 0 || V <= 0) return 0;
  return (size_t)M * head_slices(V) * sizeof(float4);
}

extern "C" int em_lm_head_nll(int dtype, const float* xrows, const float* norm_g, const float* norm_b, const void* out_w,
                              const float* out_b, const int32_t* target, int32_t M, int32_t V, int32_t d, float* nll,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!xrows || !norm_g || !norm_b || !out_w || !out_b || !target || !nll || M <= 0 || V <= 0 || d <= 0)
    return EM_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_F32) {
    if ((size_t)d * 4 > 64 * 1024) return EM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lm_head_nll_f32_kernel, dim3(M), dim3(256), (size_t)d * 4, s, xrows, norm_g, norm_b,
                       (const float*)out_w, out_b, target, V, d, nll);
    EM_CHECK_LAUNCH();
    return EM_OK;
  }
  if (dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (d % 32 || d > HEAD_DMAX) return EM_ERR_UNSUPPORTED;
  const int nsl = head_slices(V);
  if (em_cdiv(M, HEAD_ROWS) > 65535) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < em_lm_head_nll_workspace_bytes(dtype, M, V)) return EM_ERR_WORKSPACE;
  const size_t lds = (size_t)HEAD_ROWS * (d + 8) * 2;
  EM_TRY(em_raise_lds_cap((const void*)lm_head_nll_bf16_kernel, lds, &head_cap));
  hipLaunchKernelGGL(lm_head_nll_bf16_kernel, dim3(nsl, em_cdiv(M, HEAD_ROWS)), dim3(256), lds, s, xrows, norm_g, norm_b,
                     (const bf16*)out_w, out_b, target, M, V, d, (float4*)ws);
  hipLaunchKernelGGL(lm_head_merge_kernel, dim3(em_cdiv(M, 256)), dim3(256), 0, s, (const float4*)ws, target, M, nsl, nll);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" size_t em_lm_seq_nll_workspace_bytes(int dtype, const EmLmWeights* lm, int32_t B, int32_t Lp) {
  if (!lm || lm->kind != EM_LM_TRANSFORMER || !seq_shape_ok(lm, B, Lp)) return 0;
  return seq_layout(dtype, lm, (size_t)B * Lp).total;
}

extern "C" int em_lm_seq_nll(int dtype, const EmLmWeights* lm, const int32_t* x, const int32_t* target, int32_t B, int32_t Lp,
                             float* nll, void* ws, size_t ws_bytes, void* stream) {
  if (!lm || !x || !target || !nll || B <= 0 || Lp <= 0) return EM_ERR_BAD_ARG;
  if (dtype != EM_BF16 && dtype != EM_F32) return EM_ERR_BAD_ARG;
  if (lm->kind != EM_LM_TRANSFORMER || !lm->layers) return EM_ERR_BAD_ARG;
  if (!seq_shape_ok(lm, B, Lp)) return EM_ERR_UNSUPPORTED;
  const int M = B * Lp, V = lm->vocab, d = lm->d, ff = lm->ff, eu = lm->embed_unit;
  const SeqWs o = seq_layout(dtype, lm, (size_t)M);
  if (!ws || ws_bytes < o.total) return EM_ERR_WORKSPACE;
  unsigned char* base = (unsigned char*)ws;
  void *e = base + o.e, *xn = base + o.xn, *qkv = base + o.qkv, *ctx = base + o.ctx, *hb = base + o.h;
  float* xf = (float*)(base + o.x);
  EM_TRY(em_lm_embed(dtype, lm->embed, x, M, V, eu, nullptr, 0, e, stream));
  EM_TRY(gemm(dtype, EM_EPI_SCALE_F32, e, lm->in_w, xf, lm->in_b, M, d, eu, eu, d, 1.f, stream));
  hipLaunchKernelGGL(lm_seq_input_norm_kernel, dim3(em_cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, xf, lm->in_ln_g,
                     lm->in_ln_b, lm->pe, M, d, Lp);
  EM_CHECK_LAUNCH();
  for (int l = 0; l < lm->num_blocks; ++l) {
    const EmLmLayer& q = lm->layers[l];
    EM_TRY(em_layernorm(dtype, xf, q.norm1_g, q.norm1_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_STORE, xn, q.wqkv, qkv, q.bqkv, M, 3 * d, d, d, 3 * d, 1.f, stream));
    EM_TRY(em_lm_causal_attention(dtype, qkv, x, B, Lp, d, lm->heads, ctx, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, ctx, q.wout, xf, q.bout, M, d, d, d, d, 1.f, stream));
    EM_TRY(em_layernorm(dtype, xf, q.norm2_g, q.norm2_b, M, d, LN_EPS, xn, nullptr, stream));
    EM_TRY(gemm(dtype, EM_EPI_RELU, xn, q.w1, hb, q.b1, M, ff, d, d, ff, 1.f, stream));
    EM_TRY(gemm(dtype, EM_EPI_RESID_F32, hb, q.w2, xf, q.b2, M, d, ff, ff, d, 1.f, stream));
  }
  return em_lm_head_nll(dtype, xf, lm->after_norm_g, lm->after_norm_b, lm->out_w, lm->out_b, target, M, V, d, nll,
                        base + o.head, o.total - o.head, stream);
}
