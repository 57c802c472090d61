// Host layer shared by the launch sequences (no device code): what encoder.hip, transformer.hip and ebranchformer.hip
// each used to define for themselves, and the pieces of it the streaming encoders, the search and the transducer use.
//   - EM_TRY, LN_EPS, align_up, gemm(): the conveniences of every launch sequence;
//   - Bump: workspace layouts as one call per slot;
//   - tpad256 / head_slab_bytes / project_heads / clear_head_slabs: the per-head operand format of the LDS-resident
//     attention kernels (csrc/attention2.hip, csrc/abs_attn.hip): q, k [B][H][Tpad][64], V^T [B][H][64][Tpad], bf16;
//   - rows_ffn_ok / head_operands_ok: the two rules that pick the 512-wide models' launch forms.
#pragma once
#include <stddef.h>

#include "em_common.h"
#include "switches.h"

#define EM_TRY(expr)                \
  do {                              \
    const int rc__ = (expr);        \
    if (rc__ != EM_OK) return rc__; \
  } while (0)

namespace em_host {

constexpr float LN_EPS = 1e-12f;  // transformer/layer_norm.py:23

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Workspace layout: every slot starts on a 256-byte boundary.  `s.x = b.take(bytes)` per slot, `b.o` is the total.
struct Bump {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += align_up(bytes);
    return at;
  }
};

// C = epi(A W^T + bias) * scale on plain row-major operands
inline int gemm(int dtype, int epi, const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda,
                int ldc, float scale, void* stream) {
  EmGemmArgs a = {};
  a.A = A; a.W = W; a.C = C; a.bias = bias;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.scale = scale;
  return em_gemm(dtype, epi, EM_A_PLAIN, &a, stream);
}

// ---- per-head operands of the batch encoders' attention: Tpad frames per (utterance, head), a multiple of 256
inline int tpad256(int T) { return (T + 255) / 256 * 256; }
inline size_t head_slab_bytes(int B, int d, int Tpad, size_t es) { return (size_t)B * d * Tpad * es; }

// The shared part of "attention reads per-head operands": bf16, d_k = 64, offsets inside the slabs fit 32 bits
// (ESPNET_AMD_NO_ATTN2_LARGE=1: developer A/B switch).  What differs between the callers stays at their call sites.
inline bool head_operands_ok(int dtype, int d, int h, int B, int Tpad) {
  return dtype == EM_BF16 && !em_sw().no_attn2_large && d == 64 * h && (size_t)B * d * Tpad * 4 < ((size_t)1 << 32) - 64;
}

// The projection GEMMs write the operands themselves, no repacking pass: q | k of xn [M = B*T][d] through EM_EPI_QK_HEADS
// (k follows q at B * d * Tpad elements), V^T as the swapped product W_v . xn^T through EM_EPI_VT_HEADS.
// wqkv [3d][d]: the q, k, v rows; bqkv [3d].
inline int project_heads(int dtype, const void* xn, const void* wqkv, const float* bqkv, void* qh, void* vt, int M, int d, int h,
                         int T, int Tpad, void* stream) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  EmGemmArgs a = {};
  a.A = xn; a.W = wqkv; a.C = qh; a.bias = bqkv;
  a.M = M; a.N = 2 * d; a.K = d; a.lda = d; a.ldc = 64; a.scale = 1.f;
  a.T1 = T; a.T2 = Tpad; a.F1 = h; a.d = d;
  EM_TRY(em_gemm(dtype, EM_EPI_QK_HEADS, EM_A_PLAIN, &a, stream));
  a.A = (const unsigned char*)wqkv + (size_t)2 * d * d * es; a.W = xn; a.C = vt; a.bias = bqkv + 2 * d;
  a.M = d; a.N = M; a.ldc = Tpad;
  return em_gemm(dtype, EM_EPI_VT_HEADS, EM_A_PLAIN, &a, stream);
}

// Zero `bytes` of the slabs from `first` on: frames >= T of a (b, head) slab are masked, not skipped, so they must be finite.
inline int clear_head_slabs(void* first, size_t bytes, void* stream) {
  return hipMemsetAsync(first, 0, bytes, (hipStream_t)stream) == hipSuccess ? EM_OK : EM_ERR_LAUNCH;
}

// ---- a 512-wide bf16 model runs its feed-forward modules as row-block launches of 64-row workgroups (csrc/ffn_rows.hip)
// when the shape fits, nothing switches them off (EM_ENC_NO_FUSED; ESPNET_AMD_NO_FFN_ROWS=1: developer switch) and a round
// of workgroups fills its share of the chip (em_rows_fill_ok, csrc/encoder.hip).  The caller still checks that the host
// packed the operand streams.  espnet_amd/asr/encoder/_subsampled_base.py: rows_ffn_packable mirrors the shape part.
inline bool rows_ffn_ok(int dtype, int d, int ff, int flags, long M) {
  return dtype == EM_BF16 && d == 512 && ff % 128 == 0 && ff >= 256 && !(flags & EM_ENC_NO_FUSED) && !em_sw().no_ffn_rows &&
         em_rows_fill_ok(M, flags);
}

}  // namespace em_host
