// Plain (absolute-position) multi-head self-attention over whole utterances, for the Transformer encoder
// (csrc/transformer.hip).
//
// Reference: MultiHeadedAttention.forward (espnet2/legacy/nets/pytorch_backend/transformer/attention.py:
// forward_qkv + forward_attention) in eval mode with a key-padding mask:
//     P = softmax_j(q_i . k_j / sqrt(d_k)) over keys j < klens[b] (masked probabilities 0),   ctx_i = sum_j P[i][j] v_j
// d_k = 64.  No length limit: keys are walked in LDS super-tiles with the softmax carried online.
//
// Two kernels:
//   abs_attn_kernel       bf16 MFMA (f32 accumulate, f32 softmax) over the per-head operands the projection GEMM
//                         writes for csrc/attention2.hip (EM_EPI_QK_HEADS / EM_EPI_VT_HEADS);
//   abs_attn_rows_kernel  f32 (the exact-f32 parity mode) and the bf16 fall-back, reading q | k | v rows [B*T][3d].
//
// abs_attn_kernel follows attention2.hip without the position window.  One workgroup = (utterance, head, 128 queries),
// 8 waves x 16 queries.  Scores are computed TRANSPOSED, S^T[key][query] = K . Q^T, so that in the MFMA C/D layout a lane
// holds 4 keys of ONE query: the softmax statistics are per-lane scalars (reduced over the 4 lane groups with two
// register swaps) and the probabilities are already the B operand of O^T[dk][query] = V^T . P^T.  The denominator is a
// fifth "V^T fragment" of ones on the matrix core.  K and V^T of 256 keys are LDS-resident (32 KiB each), loaded once per
// super-tile and read by all eight waves.
//
// LDS budget.  attention2.hip spends 157 KiB of the CU's 160 KiB, 48 KiB of it on the 383 position rows the window
// reaches, and so runs one workgroup per CU.  Without the window a 256-key super-tile is 64 KiB, and the freed LDS buys
// OCCUPANCY rather than longer super-tiles: two workgroups (16 waves, four per SIMD) fit on a CU, so one workgroup's
// staging and barrier stalls run under the other's MFMAs - the staging here is plain register loads with no software
// pipeline of its own.  A 512-key super-tile (128 KiB, one workgroup per CU) would only pay for inputs over 10 s
// (T > 256 frames after 4x subsampling); at the 10 s shape every key fits in one 256-key super-tile already.
// More queries per workgroup (16 waves) would halve the K / V^T traffic from L2, which at 2 x 32 KiB per 128 queries is
// not what bounds this kernel (each K / V^T byte feeds 128 queries' MFMAs).
#include <math.h>
#include <stdlib.h>

#include "em_common.h"

namespace {

constexpr int QB = 128;          // queries per workgroup
constexpr int KSUP = 256;        // keys per LDS super-tile
constexpr int SK_OFF = 0;        // [256 keys][128 B], 16-byte chunks XOR-swizzled by (row & 7)
constexpr int SV_OFF = 32768;    // [4 key tiles][64 dk][128 B], chunks XOR-swizzled by (row >> 1) & 7
constexpr int SMEM_BYTES = 65536;

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__global__ __launch_bounds__(512, 4) void abs_attn_kernel(const bf16* __restrict__ qh, const bf16* __restrict__ kh,
                                                          const bf16* __restrict__ vt, const int* __restrict__ klens,
                                                          int T, int Tpad, int H, bf16* __restrict__ ctx) {
  using MM = Mma<bf16>;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4, swz = lr & 7;
  const int hh = blockIdx.y, b = blockIdx.z, iw0 = blockIdx.x * QB + 16 * wave;
  const int klen = klens[b] < T ? klens[b] : T;
  const size_t bh = (size_t)b * H + hh;
  const bf16* kb = kh + bh * Tpad * 64;
  const bf16* vb = vt + bh * 64 * Tpad;

  // query fragments (B operand: column = query iw0 + lr, k-slice lg), scaled by 1 / sqrt(64): a power of two, exact
  bf16x8 qf[2];
  {
    const bf16* qrow = qh + (bh * Tpad + iw0 + lr) * 64 + lg * 8;  // (iw0 + lr < Tpad: the grid covers T rounded to 128)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 raw = *(const bf16x8*)(qrow + 32 * ks);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[ks][e] = (bf16)((float)raw[e] * 0.125f);
    }
  }

  // K rows and V^T columns of keys js .. js + 255; keys >= klen are staged as zeros (so that masked probabilities meet
  // zeros, whatever the padding frames of the operands hold)
  auto stage = [&](int js) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = tid + 512 * u, row = q >> 3, c = q & 7;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (js + row < klen) v = *(const u32x4*)(kb + (size_t)(js + row) * 64 + c * 8);
      *(u32x4*)(smem + SK_OFF + row * 128 + ((c ^ (row & 7)) << 4)) = v;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = tid + 512 * u, row = q >> 5, kc = q & 31, t = kc >> 3, c = kc & 7;
      const int key0 = js + 8 * kc;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (key0 < klen) {
        v = *(const u32x4*)(vb + (size_t)row * Tpad + key0);  // (key0 + 7 < js + 256 <= Tpad)
        if (key0 + 8 > klen) {
          bf16x8 x = __builtin_bit_cast(bf16x8, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = key0 + e < klen ? x[e] : (bf16)0.f;
          v = __builtin_bit_cast(u32x4, x);
        }
      }
      *(u32x4*)(smem + SV_OFF + t * 8192 + row * 128 + ((c ^ ((row >> 1) & 7)) << 4)) = v;
    }
  };

  f32x4 acc_o[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc_o[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 acc_l = (f32x4){0.f, 0.f, 0.f, 0.f};
  float row_m = -INFINITY;
  const bf16x8 ones = {(bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f};
  constexpr float LOG2E = 1.4426950408889634f;

  for (int js = 0; js < klen; js += KSUP) {
    if (js > 0) __syncthreads();  // every wave is done with the previous super-tile
    stage(js);
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < KSUP / 64; ++kt) {
      const int j0 = js + 64 * kt;
      if (j0 >= klen) break;  // (uniform)
      // ---- S^T[key j0 + 16 n + 4 lg + r][query lr]
      f32x4 sc[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) sc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const unsigned char* sk = smem + SK_OFF + (64 * kt + lr) * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int coff = ((ks * 4 + lg) ^ swz) << 4;
#pragma unroll
        for (int n = 0; n < 4; ++n) sc[n] = MM::mma(*(const bf16x8*)(sk + n * 2048 + coff), qf[ks], sc[n]);
      }
      if (j0 + 64 > klen) {  // (uniform: only the tile that holds the utterance's end masks anything)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) sc[n][r] = (j0 + 16 * n + 4 * lg + r < klen) ? sc[n][r] : -INFINITY;
      }
      float tm = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) tm = fmaxf(tm, sc[n][r]);
      // ---- online softmax; this lane's query is iw0 + lr, its keys the 16 (n, r) of lane group lg
      tm = wave_xor16_max(tm);
      tm = wave_xor32_max(tm);
      const float mn = fmaxf(row_m, tm);  // (finite: key j0 < klen is in this tile)
      const float alpha = __expf(row_m - mn);
      row_m = mn;
      const float mnl = mn * LOG2E;
      unsigned pbu[2][4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[n][2 * h], LOG2E, -mnl));
          const float e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[n][2 * h + 1], LOG2E, -mnl));
          pbu[n >> 1][(n & 1) * 2 + h] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){e0, e1}, bf16x2));
        }
      bf16x8 pb[2];
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) pb[jp] = __builtin_bit_cast(bf16x8, (u32x4){pbu[jp][0], pbu[jp][1], pbu[jp][2], pbu[jp][3]});
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        acc_o[f][0] *= alpha; acc_o[f][1] *= alpha; acc_o[f][2] *= alpha; acc_o[f][3] *= alpha;
      }
      acc_l[0] *= alpha;  // (the other rows of the ones fragment carry the same sum; only this one is read)
      // ---- O^T += V^T . P^T.  Slots 0..3 of lane group lg hold keys 32 jp + 4 lg + (0..3), slots 4..7 keys
      // 32 jp + 16 + 4 lg + (0..3): V^T is read to match with two 8-byte loads (chunk c = keys 8 c .. 8 c + 7 of the tile)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        acc_l = MM::mma(ones, pb[jp], acc_l);
        const int c0 = 4 * jp + (lg >> 1);
        const int sw = (lr >> 1) & 7;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const unsigned char* sv = smem + SV_OFF + kt * 8192 + (16 * f + lr) * 128 + (lg & 1) * 8;
          const bf16x4 a0 = *(const bf16x4*)(sv + ((c0 ^ sw) << 4));
          const bf16x4 a1 = *(const bf16x4*)(sv + (((c0 + 2) ^ sw) << 4));
          const bf16x8 vf = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
          acc_o[f] = MM::mma(vf, pb[jp], acc_o[f]);
        }
      }
    }
  }

  // ---- normalise and store ctx[b*T + i][hh*64 + 16 f + 4 lg + r]
  const int i = iw0 + lr;
  if (i < T) {
    const float row_l = acc_l[0];
    const float inv = row_l > 0.f ? 1.0f / row_l : 0.f;
    bf16* o = ctx + ((size_t)b * T + i) * (H * 64) + hh * 64 + 4 * lg;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const bf16x4 pk = {(bf16)(acc_o[f][0] * inv), (bf16)(acc_o[f][1] * inv), (bf16)(acc_o[f][2] * inv),
                         (bf16)(acc_o[f][3] * inv)};
      *(bf16x4*)(o + 16 * f) = pk;
    }
  }
}

// ---- f32 / fall-back form: one thread per query (its q and output row in registers), 128 queries per workgroup,
// K / V tiles of 32 keys in LDS read by every lane at the same address (broadcast).  f32 arithmetic throughout,
// libm exp: this is the parity mode's kernel, not a fast path.
constexpr int RQ = 128, RK = 32;

template <typename T>
__global__ __launch_bounds__(RQ) void abs_attn_rows_kernel(const T* __restrict__ qkv, const int* __restrict__ klens,
                                                           int Tn, int H, T* __restrict__ ctx) {
  __shared__ float sk[RK][64], sv[RK][64];
  const int tid = threadIdx.x, hh = blockIdx.y, b = blockIdx.z, i = blockIdx.x * RQ + tid;
  const int d = H * 64, ld = 3 * d;
  const int klen = klens[b] < Tn ? klens[b] : Tn;
  float q[64], acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    q[c] = i < Tn ? to_f32(qkv[((size_t)b * Tn + i) * ld + hh * 64 + c]) * 0.125f : 0.f;
    acc[c] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < klen; j0 += RK) {
    __syncthreads();
    for (int u = tid; u < RK * 64; u += RQ) {
      const int jj = u >> 6, c = u & 63, key = j0 + jj;
      float kv = 0.f, vv = 0.f;
      if (key < klen) {
        const size_t row = ((size_t)b * Tn + key) * ld + hh * 64 + c;
        kv = to_f32(qkv[row + d]);
        vv = to_f32(qkv[row + 2 * d]);
      }
      sk[jj][c] = kv;
      sv[jj][c] = vv;
    }
    __syncthreads();
    float s[RK], tm = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < RK; ++jj) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < 64; ++c) a = fmaf(q[c], sk[jj][c], a);
      s[jj] = j0 + jj < klen ? a : -INFINITY;
      tm = fmaxf(tm, s[jj]);
    }
    const float mn = fmaxf(m, tm), alpha = expf(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] *= alpha;
#pragma unroll
    for (int jj = 0; jj < RK; ++jj) {
      const float p = expf(s[jj] - mn);
      l += p;
#pragma unroll
      for (int c = 0; c < 64; ++c) acc[c] = fmaf(p, sv[jj][c], acc[c]);
    }
  }
  if (i < Tn) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    T* o = ctx + ((size_t)b * Tn + i) * d + hh * 64;
#pragma unroll
    for (int c = 0; c < 64; ++c) o[c] = from_f32<T>(acc[c] * inv);
  }
}

}  // namespace

extern "C" int em_abs_attention_bf16(const void* qh, const void* kh, const void* vt, const int32_t* klens, int32_t B,
                                     int32_t T, int32_t Tpad, int32_t h, void* ctx, void* stream) {
  if (!qh || !kh || !vt || !klens || !ctx) return EM_ERR_BAD_ARG;
  if (B <= 0 || T <= 0 || h <= 0) return EM_ERR_BAD_ARG;
  if (Tpad % KSUP != 0 || Tpad < T || B > 65535 || h > 65535) return EM_ERR_UNSUPPORTED;
  static EmLdsCap cap = {};
  if (em_raise_lds_cap((const void*)abs_attn_kernel, SMEM_BYTES, &cap) != EM_OK) return EM_ERR_LAUNCH;
  const bool rec = em_prof_begin(stream);
  hipLaunchKernelGGL(abs_attn_kernel, dim3(em_cdiv(T, QB), h, B), dim3(512), SMEM_BYTES, (hipStream_t)stream,
                     (const bf16*)qh, (const bf16*)kh, (const bf16*)vt, klens, T, Tpad, h, (bf16*)ctx);
  if (rec) em_prof_end(stream, 4.0 * B * h * (double)T * T * 64, EM_PROF_ATTN);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" int em_abs_attention(int dtype, const void* qkv, const int32_t* klens, int32_t B, int32_t T, int32_t h,
                                int32_t dk, void* ctx, void* stream) {
  if (!qkv || !klens || !ctx) return EM_ERR_BAD_ARG;
  if (B <= 0 || T <= 0 || h <= 0) return EM_ERR_BAD_ARG;
  if (dk != 64 || B > 65535 || h > 65535) return EM_ERR_UNSUPPORTED;
  const dim3 grid(em_cdiv(T, RQ), h, B);
  if (dtype == EM_F32)
    hipLaunchKernelGGL(abs_attn_rows_kernel<float>, grid, dim3(RQ), 0, (hipStream_t)stream, (const float*)qkv, klens, T, h,
                       (float*)ctx);
  else if (dtype == EM_BF16)
    hipLaunchKernelGGL(abs_attn_rows_kernel<bf16>, grid, dim3(RQ), 0, (hipStream_t)stream, (const bf16*)qkv, klens, T, h,
                       (bf16*)ctx);
  else
    return EM_ERR_BAD_ARG;
  EM_CHECK_LAUNCH();
  return EM_OK;
}
