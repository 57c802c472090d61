// espnet_amd — the transducer (RNN-T) likelihood of given transcripts on gfx950: the joint network over every lattice node
// of a ragged batch of candidates, and the forward (sum-product) recursion over that lattice (contract: include/
// espnet_amd.h, "transducer likelihood of given transcripts").  Reference: espnet2/asr/espnet_model.py
// `_calc_transducer_loss` (the forward value of the RNN-T loss), espnet2/asr_transducer/joint_network.py.
//
// The decoding kernels (csrc/transducer.hip) have at most 64 rows against a weight matrix that is streamed once.  Here the
// rows are the lattice nodes (n, t, u) of N candidates - about 10^6 at 64 candidates x 249 frames x 40-80 tokens - and of
// the V logits of a node exactly two are wanted, so neither the logits nor the (node, jp) hidden layer z may reach memory:
//   lattice_rows_kernel   one launch: the number of valid nodes T_b * (U + 1) of every candidate and their running sum,
//                         the compacted row list that the tiles are cut from (padding nodes form no rows);
//   lattice_bf16_kernel   a workgroup of eight waves owns 64 consecutive rows of that list and ALL vocabulary columns:
//                         z = tanh(enc_proj + dec_proj) is made ONCE per row, rounded to bf16 into LDS (rows padded by
//                         16 bytes); wave w takes the pairs of 16-column tiles w, w + 8, ... of lin_out, its fragments straight
//                         from global memory (L2), one chunk of k ahead, against the four row tiles' fragments from LDS.  A lane keeps the record
//                         (max, sum-exp, blank logit, label logit) of its 16 (row, column lr) pairs across tiles with one
//                         exp per logit; the 16 lanes of a row group, then the eight waves merge once at the end and the
//                         two log-probabilities of the node are stored.  No partial records in memory, no merge launch;
//   lattice_f32_kernel    the parity path: a workgroup per node, z in LDS as f32, thread i walks the columns i, i + 256, ..;
//   seq_nll_kernel        a workgroup per candidate: the walk of csrc/rnnt_lattice.h with the sum cell, the closing blank.
// A node's values depend on its own two projection rows and the weights only: the operations on a row are the same
// whichever tile, row slot and companions it has (an MFMA row sees its own A row only; the merges run in a fixed order
// over columns), so they are bit for bit the same for any N, Lmax and mem_of.
#include <cfloat>
#include <math.h>

#include "em_common.h"
#include "enc_host.h"
#include "rnnt_lattice.h"

namespace {

constexpr int LT_ROWS = 64;      // rows of a workgroup: four 16-row MFMA tiles
constexpr int LT_WAVES = 8;      // waves of a workgroup: the 16-column tiles of the vocabulary are dealt round robin
constexpr int LT_JP_MAX = 1024;  // bf16: 64 rows of jp + 8 bf16 stay inside the 160 KiB of LDS
constexpr int LT_JP_MAX_F32 = 8192;

struct LatArgs {
  const float *enc_proj, *dec_proj, *out_b;
  const void* lin_out;
  const int32_t *xlens, *targets, *ylens, *mem_of, *off;
  int32_t Bm, T, Lmax, N, V, jp, blank;
  float* lat;
};

// ---- the compacted row list: off[n] = number of valid nodes of the candidates before n, off[N] = all of them.  One
// workgroup; thread i sums a contiguous run of candidates, thread 0 chains the 1 024 run totals.
__global__ __launch_bounds__(1024) void lattice_rows_kernel(const int32_t* __restrict__ xlens, const int32_t* __restrict__ ylens,
                                                            const int32_t* __restrict__ mem_of, int N, int Bm, int T, int Lmax,
                                                            int32_t* __restrict__ off) {
  __shared__ int32_t run[1024];
  const int tid = threadIdx.x;
  const int per = (N + 1023) / 1024;
  const int n0 = min(tid * per, N), n1 = min(n0 + per, N);
  int sum = 0;
  for (int n = n0; n < n1; ++n) sum += rnnt_lattice::clamp(xlens, ylens, mem_of, Bm, T, Lmax, n).nodes();
  run[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int i = 0; i < 1024; ++i) {
      const int v = run[i];
      run[i] = acc;
      acc += v;
    }
    off[N] = acc;
  }
  __syncthreads();
  int acc = run[tid];
  for (int n = n0; n < n1; ++n) {
    off[n] = acc;
    acc += rnnt_lattice::clamp(xlens, ylens, mem_of, Bm, T, Lmax, n).nodes();
  }
}

// where row g of the compacted list lives
struct Node {
  int enc_row;   // m * T + t: row of enc_proj
  int dec_row;   // u * N + n: row of dec_proj
  int label;     // targets[n][u], or -1 at u == U
  int lat_node;  // (n * T + t) * (Lmax + 1) + u
};
__device__ __forceinline__ Node find_node(const LatArgs& a, int g) {
  int lo = 0, hi = a.N - 1;  // the last n with off[n] <= g (candidates without nodes repeat an offset: the last one counts)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int n = lo;
  const rnnt_lattice::Cand c = rnnt_lattice::clamp(a.xlens, a.ylens, a.mem_of, a.Bm, a.T, a.Lmax, n);
  const int local = g - a.off[n];
  const int t = local / (c.U + 1), u = local - t * (c.U + 1);
  Node r;
  r.enc_row = c.m * a.T + t;
  r.dec_row = u * a.N + n;
  r.label = u < c.U ? a.targets[(size_t)n * a.Lmax + u] : -1;
  r.lat_node = (n * a.T + t) * (a.Lmax + 1) + u;
  return r;
}

// A row's record over a set of columns: the maximum logit, the sum of exp(logit - maximum), the blank's logit and the
// label's (-inf while their columns have not been met).  FAST: the bf16 path's __expf; the parity path keeps expf.
struct Rec {
  float m, s, b, l;
};
template <bool FAST = true>
__device__ __forceinline__ Rec rec_merge(Rec x, Rec y) {
  Rec r;
  r.m = fmaxf(x.m, y.m);
  r.b = fmaxf(x.b, y.b);
  r.l = fmaxf(x.l, y.l);
  const float ex = FAST ? __expf(x.m - r.m) : expf(x.m - r.m), ey = FAST ? __expf(y.m - r.m) : expf(y.m - r.m);
  r.s = (x.m == -INFINITY ? 0.f : x.s * ex) + (y.m == -INFINITY ? 0.f : y.s * ey);
  return r;
}
__device__ __forceinline__ Rec rec_shfl_xor(Rec v, int o) {
  return Rec{__shfl_xor(v.m, o, 64), __shfl_xor(v.s, o, 64), __shfl_xor(v.b, o, 64), __shfl_xor(v.l, o, 64)};
}

__device__ __forceinline__ void store_node(const LatArgs& a, const Node& nd, Rec r, float lse) {
  f32x2 o;
  o[0] = r.b - lse;
  o[1] = nd.label >= 0 ? r.l - lse : -INFINITY;
  *(f32x2*)(a.lat + (size_t)nd.lat_node * 2) = o;
}

__global__ __launch_bounds__(64 * LT_WAVES) void lattice_bf16_kernel(const LatArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lt_smem[];
  __shared__ Node nodes[LT_ROWS];
  __shared__ float red[LT_WAVES][LT_ROWS][4];
  bf16* zs = (bf16*)lt_smem;
  const int jp = a.jp, ldz = jp + 8, V = a.V;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int total = a.off[a.N];
  const int g0 = blockIdx.x * LT_ROWS;
  if (g0 >= total) return;  // (workgroup-uniform: the grid is cut for N * T * (Lmax + 1) rows)
  if (threadIdx.x < LT_ROWS) {
    Node nd{0, 0, -1, -1};
    if (g0 + (int)threadIdx.x < total) nd = find_node(a, g0 + threadIdx.x);
    nodes[threadIdx.x] = nd;
  }
  __syncthreads();
  // z: wave w makes the rows w, w + 8, ...; a lane four channels at a time
  for (int rl = wave; rl < LT_ROWS; rl += LT_WAVES) {
    const Node nd = nodes[rl];
    bf16* dst = zs + (size_t)rl * ldz;
    if (nd.lat_node >= 0) {
      const float* e = a.enc_proj + (size_t)nd.enc_row * jp;
      const float* d = a.dec_proj + (size_t)nd.dec_row * jp;
      for (int c = lane * 4; c < jp; c += 256) {
        const f32x4 ev = *(const f32x4*)(e + c), dv = *(const f32x4*)(d + c);
        bf16x4 z;
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = (bf16)tanhf(ev[i] + dv[i]);
        *(bf16x4*)(dst + c) = z;
      }
    } else {
      for (int c = lane * 4; c < jp; c += 256) *(bf16x4*)(dst + c) = (bf16x4){(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
    }
  }
  __syncthreads();
  Rec rec[4][4];
  int tg[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rec[rt][q] = Rec{-INFINITY, 0.f, -INFINITY, -INFINITY};
      tg[rt][q] = nodes[rt * 16 + lg * 4 + q].label;
    }
  const bf16* w = (const bf16*)a.lin_out;
  const int nk = jp / 32, ntiles = (V + 15) >> 4, blank = a.blank;
  const bf16* arow = zs + (size_t)lr * ldz + lg * 8;
  // A wave walks PAIRS of column tiles (2 tp, 2 tp + 1), tp = wave, wave + 8, ..: a row-tile fragment read from LDS meets
  // two weight fragments, which halves the LDS traffic per MFMA (at one column tile the eight waves asked the LDS for
  // twice what it delivers in the MFMAs' time).  The contraction goes in chunks of two k-steps (jp % 64 == 0), the four
  // weight fragments of the NEXT chunk - of the next tile pair at a pair's end - in flight during the 16 MFMAs of this one:
  // without that every k-step waited a whole L2 round trip for its one fragment.
  const int ntp = (ntiles + 1) >> 1, nch = nk >> 1;
  const int steps = wave < ntp ? ((ntp - wave + LT_WAVES - 1) / LT_WAVES) * nch : 0;
  auto load_chunk = [&](int tp, int c, bf16x8(&f)[2][2]) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int col = (2 * tp + ct) * 16 + lr;
      const bf16* wrow = w + (size_t)min(col, V - 1) * jp + lg * 8 + c * 64;
      f[ct][0] = *(const bf16x8*)wrow;
      f[ct][1] = *(const bf16x8*)(wrow + 32);
    }
  };
  bf16x8 cur[2][2], nxt[2][2];
  int tp = wave, c = 0;
  if (steps > 0) load_chunk(tp, 0, cur);
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int i = 0; i < 2; ++i) nxt[ct][i] = cur[ct][i];
  f32x4 acc[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < steps; ++it) {
    int tpn = tp, cn = c + 1;
    if (cn == nch) {
      cn = 0;
      tpn += LT_WAVES;
    }
    if (it + 1 < steps) load_chunk(tpn, cn, nxt);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        const bf16x8 af = *(const bf16x8*)(arow + (size_t)rt * 16 * ldz + (c * 2 + i) * 32);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct][rt] = Mma<bf16>::mma(af, cur[ct][i], acc[ct][rt]);
      }
    if (cn == 0) {  // the tile pair is complete: its 2 x 16 logits of every row go into the records
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = (2 * tp + ct) * 16 + lr;
        if (col < V) {
          const float bb = a.out_b[col];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float val = acc[ct][rt][q] + bb;
              Rec& r = rec[rt][q];
              if (col == blank) r.b = val;
              if (col == tg[rt][q]) r.l = val;
              const float dlt = val - r.m;  // r.m = -inf at first: dlt = +inf, e = 0, s = 1
              const float e = __expf(-fabsf(dlt));
              r.s = dlt > 0.f ? r.s * e + 1.f : r.s + e;
              r.m = fmaxf(r.m, val);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 2; ++i) cur[ct][i] = nxt[ct][i];
    tp = tpn;
    c = cn;
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Rec r = rec[rt][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) r = rec_merge(r, rec_shfl_xor(r, o));
      if (lr == 0) {
        float* dst = red[wave][rt * 16 + lg * 4 + q];
        dst[0] = r.m;
        dst[1] = r.s;
        dst[2] = r.b;
        dst[3] = r.l;
      }
    }
  __syncthreads();
  if (threadIdx.x < LT_ROWS) {
    const int rl = threadIdx.x;
    const Node nd = nodes[rl];
    if (nd.lat_node < 0) return;
    Rec r{red[0][rl][0], red[0][rl][1], red[0][rl][2], red[0][rl][3]};
#pragma unroll
    for (int wv = 1; wv < LT_WAVES; ++wv) r = rec_merge(r, Rec{red[wv][rl][0], red[wv][rl][1], red[wv][rl][2], red[wv][rl][3]});
    store_node(a, nd, r, r.m + logf(r.s));
  }
}

// f32 (parity path): a workgroup per node.  z sits in LDS, thread i walks the columns i, i + 256, ...
__global__ __launch_bounds__(256) void lattice_f32_kernel(const LatArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lt_smem[];
  __shared__ float red[4][4];
  float* z = (float*)lt_smem;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (g >= a.off[a.N]) return;  // (workgroup-uniform)
  const Node nd = find_node(a, g);
  const int jp = a.jp, V = a.V;
  const float* e = a.enc_proj + (size_t)nd.enc_row * jp;
  const float* d = a.dec_proj + (size_t)nd.dec_row * jp;
  for (int c = tid; c < jp; c += 256) z[c] = tanhf(e[c] + d[c]);
  __syncthreads();
  const float* w = (const float*)a.lin_out;
  Rec r{-INFINITY, 0.f, -INFINITY, -INFINITY};
  for (int v = tid; v < V; v += 256) {
    const float* wr = w + (size_t)v * jp;
    float s = 0.f;
    for (int c = 0; c < jp; ++c) s += z[c] * wr[c];
    const float val = s + a.out_b[v];
    if (v == a.blank) r.b = val;
    if (v == nd.label) r.l = val;
    const float mm = fmaxf(r.m, val);
    r.s = r.s * expf(r.m - mm) + expf(val - mm);  // r.m = -inf: 0 * 0
    r.m = mm;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) r = rec_merge<false>(r, rec_shfl_xor(r, o));
  if (lane == 0) {
    red[wave][0] = r.m;
    red[wave][1] = r.s;
    red[wave][2] = r.b;
    red[wave][3] = r.l;
  }
  __syncthreads();
  if (tid == 0) {
    Rec t{-INFINITY, 0.f, -INFINITY, -INFINITY};
    for (int i = 0; i < 4; ++i) t.m = fmaxf(t.m, red[i][0]), t.b = fmaxf(t.b, red[i][2]), t.l = fmaxf(t.l, red[i][3]);
    for (int i = 0; i < 4; ++i) t.s += red[i][0] == -INFINITY ? 0.f : red[i][1] * expf(red[i][0] - t.m);
    store_node(a, nd, t, t.m + logf(t.s));
  }
}

// ---- the forward recursion.  log(exp(x) + exp(y)) shifted by the larger term; -inf terms (both too) give -inf, never NaN
__device__ __forceinline__ float logaddexp_(float x, float y) {
  const float hi = fmaxf(x, y), lo = fminf(x, y);
  return hi + log1pf(expf(lo - fmaxf(hi, -FLT_MAX)));
}

struct SeqArgs {
  const float* lat;
  const int32_t *xlens, *ylens, *mem_of;
  int32_t Bm, T, Lmax;
  float* nll;
};

struct SumCell {  // the sum-product cell of rnnt_lattice::walk
  __device__ __forceinline__ float node(int, float stay, float emit) { return logaddexp_(stay, emit); }
};

__global__ __launch_bounds__(1024) void seq_nll_kernel(const SeqArgs a) {
  __shared__ float row[2][rnnt_lattice::MAX_L + 1];
  const int n = blockIdx.x, u = threadIdx.x;
  const rnnt_lattice::Cand c = rnnt_lattice::clamp(a.xlens, a.ylens, a.mem_of, a.Bm, a.T, a.Lmax, n);
  if (c.Tb == 0) {  // (workgroup-uniform)
    if (u == 0) a.nll[n] = INFINITY;
    return;
  }
  const size_t ld = (size_t)(a.Lmax + 1) * 2;
  const float* base = a.lat + (size_t)n * a.T * ld;
  const float alpha = rnnt_lattice::walk(base, a.Lmax, c.Tb, c.U, row, SumCell{});
  if (u == c.U) a.nll[n] = -(alpha + base[(size_t)(c.Tb - 1) * ld + 2 * c.U]);  // the closing blank
}

int check_weights(int dtype, const EmTransducerWeights* w) {
  if (!w || (dtype != EM_F32 && dtype != EM_BF16)) return EM_ERR_BAD_ARG;
  if (!w->lin_out || !w->out_b) return EM_ERR_BAD_ARG;
  if (w->vocab < 2 || w->joint < 1 || w->blank < 0 || w->blank >= w->vocab) return EM_ERR_BAD_ARG;
  if (w->jp % 64 != 0 || w->jp < w->joint) return EM_ERR_UNSUPPORTED;
  if (w->jp > (dtype == EM_BF16 ? LT_JP_MAX : LT_JP_MAX_F32)) return EM_ERR_UNSUPPORTED;
  return EM_OK;
}

EmLdsCap lattice_cap;

}  // namespace

extern "C" int32_t em_transducer_seq_nll_max_tokens(void) { return rnnt_lattice::MAX_L; }

extern "C" size_t em_transducer_lattice_logp_workspace_bytes(int dtype, const EmTransducerWeights* w, int32_t N, int32_t T,
                                                             int32_t Lmax) {
  if (check_weights(dtype, w) != EM_OK || !rnnt_lattice::shape_ok(N, T, Lmax)) return 0;
  return (((size_t)N + 1) * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int em_transducer_lattice_logp(int dtype, const EmTransducerWeights* w, const float* enc_proj, const int32_t* xlens,
                                          int32_t Bm, int32_t T, const float* dec_proj, const int32_t* targets, int32_t Lmax,
                                          const int32_t* ylens, const int32_t* mem_of, int32_t N, float* lat, void* ws,
                                          size_t ws_bytes, void* stream) {
  EM_TRY(check_weights(dtype, w));
  if (!enc_proj || !xlens || !dec_proj || !ylens || !lat || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0) return EM_ERR_BAD_ARG;
  if (Lmax > 0 && !targets) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if (!rnnt_lattice::shape_ok(N, T, Lmax) || (long)Bm * T > rnnt_lattice::MAX_NODES) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < em_transducer_lattice_logp_workspace_bytes(dtype, w, N, T, Lmax)) return EM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  LatArgs a;
  a.enc_proj = enc_proj; a.dec_proj = dec_proj; a.out_b = w->out_b; a.lin_out = w->lin_out;
  a.xlens = xlens; a.targets = targets; a.ylens = ylens; a.mem_of = mem_of; a.off = (const int32_t*)ws;
  a.Bm = Bm; a.T = T; a.Lmax = Lmax; a.N = N; a.V = w->vocab; a.jp = w->jp; a.blank = w->blank;
  a.lat = lat;
  hipLaunchKernelGGL(lattice_rows_kernel, dim3(1), dim3(1024), 0, s, xlens, ylens, mem_of, N, Bm, T, Lmax, (int32_t*)ws);
  const long rows = (long)N * T * (Lmax + 1);
  if (dtype == EM_BF16) {
    const size_t lds = (size_t)LT_ROWS * (w->jp + 8) * 2;
    EM_TRY(em_raise_lds_cap((const void*)lattice_bf16_kernel, lds, &lattice_cap));
    hipLaunchKernelGGL(lattice_bf16_kernel, dim3((unsigned)((rows + LT_ROWS - 1) / LT_ROWS)), dim3(64 * LT_WAVES), lds, s, a);
  } else {
    hipLaunchKernelGGL(lattice_f32_kernel, dim3((unsigned)rows), dim3(256), (size_t)w->jp * 4, s, a);
  }
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" int em_transducer_seq_nll(const float* lat, const int32_t* xlens, int32_t Bm, int32_t T, int32_t Lmax,
                                     const int32_t* ylens, const int32_t* mem_of, int32_t N, float* nll, void* stream) {
  if (!lat || !xlens || !ylens || !nll || N <= 0 || Bm <= 0 || T <= 0 || Lmax < 0) return EM_ERR_BAD_ARG;
  if (!mem_of && N > Bm) return EM_ERR_BAD_ARG;
  if (!rnnt_lattice::shape_ok(N, T, Lmax)) return EM_ERR_UNSUPPORTED;
  const SeqArgs a{lat, xlens, ylens, mem_of, Bm, T, Lmax, nll};
  hipLaunchKernelGGL(seq_nll_kernel, dim3(N), dim3(64 * em_cdiv(Lmax + 1, 64)), 0, (hipStream_t)stream, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
