// What the two CTC forward-backward kernels (ctc_post.hip: f32 logarithms as they are; ctc_post_renorm.hip: rows kept
// relative to integer offsets) share: the workspace's row geometry, the merge of shifted sums and
// what a direction keeps per token.
#pragma once
#include <cfloat>

#include "ctc_trellis.h"

namespace ctc_post_common {

constexpr int CP_DUAL_WAVES = 8;  // waves per direction up to which both directions share a workgroup (1 024 threads)

static inline int row_states(int Lmax) { return (2 * Lmax + 1 + 7) & ~7; }
static inline int ws_rows(int T) { return (T + 1) / 2 + 1; }

// (m, s): a sum s * 2^m of terms kept relative to their maximum m; merging is symmetric, so a butterfly gives every
// lane the same bits, and a part (-inf, 0) changes nothing
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
  const float mm = fmaxf(m, mo), sh = fmaxf(mm, -FLT_MAX);
  s = s * __builtin_amdgcn_exp2f(m - sh) + so * __builtin_amdgcn_exp2f(mo - sh);
  m = mm;
}

// what a direction keeps per token of the lane
struct TokAcc {
  float occ[4], peak[4];
  int pt[4];
};

}  // namespace ctc_post_common
