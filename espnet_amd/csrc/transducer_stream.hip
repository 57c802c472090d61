// espnet_amd — the RESUMABLE greedy transducer walk for streams on gfx950 (contract: include/espnet_amd.h, "transducer
// on streams").  A stream's whole memory between two calls is one slot of a state slab: the prediction network's states,
// its lin_dec row, the running score, the frame and label counts and the label list.  A call (a tick) feeds stream s its
// next nframes[s] <= F encoder frames.
//
// The one-shot walk (csrc/transducer.hip) moves frame by frame: four dependent launches and one pass over lin_out per
// frame.  While a hypothesis emits blanks its prediction-network state does not change, so here the decisions of ALL
// remaining frames of the chunk are taken against the current state in one launch, only the first non-blank frame is
// committed, the state advances once and the rest is redone.  A tick is a stream-ordered chain of rounds, no read-back:
//   head     the rows (s, f), f at or after stream s's cursor, as tiles of 64 rows x slices of ST_SLICE vocabulary
//            columns.  A workgroup of five waves makes z = tanh(enc_proj[s, f] + dec_proj[s]) of its 64 rows ONCE into
//            LDS (bf16, rows padded by 16 bytes), then every wave owns one pair of 16-column tiles of lin_out: its
//            fragments go from global memory straight into MFMA operands, one chunk of k ahead, against the four row
//            tiles' fragments from LDS.  A lane folds its (row, column) logits into a record (max, arg-max, runner-up,
//            sum-exp), the 16 lanes of a row group merge, then the five waves, and ONE float4 per (row, slice) is stored:
//            neither z nor a logit reaches memory.  float32 takes the parity kernel: a workgroup per row, z in LDS as
//            f32, thread i the columns i, i + 256, ...;
//   commit   one wave per stream, lane j the frame cursor + j: merges the slices' records in slice order, finds the first
//            frame whose arg-max is a label, adds the log-probabilities of the frames up to it to the slot's score (in
//            frame order, in double), appends the label, hands tok / mask to the advance and moves the cursor behind that
//            frame (at most one label per frame); with no label left it adds the blanks and ends the stream's tick;
//   advance  the row kernels of csrc/transducer_rows.h (dec_rows) for the masked streams, in slices of 64 rows.
// F rounds are enqueued (a stream that emits on every frame needs them all).  Two device counters per round - streams that
// still have rows, streams that advance - make the launches behind the last needed round return at once (`live` of
// transducer_rows.h).
//
// A row's record depends on its own two projection rows and the weights only: an MFMA row sees its own A row, the
// column order of every merge is fixed, the slice width is a constant - never on S, F, the tile slot or the companions.
// The commit's sums run in frame order in double.  So any chunking of the same frames leaves the same bits in the slot.
#include <math.h>

#include "em_common.h"
#include "transducer_rows.h"
#include "enc_host.h"

namespace {

constexpr int ST_ROWS = 64;              // rows of a head workgroup: four 16-row MFMA tiles
constexpr int ST_WAVES = 5;              // its waves: one pair of 16-column tiles each
constexpr int ST_SLICE = ST_WAVES * 32;  // 160 vocabulary columns per workgroup (why 160)
constexpr int ST_MAX_S = 1024;           // streams of one call
constexpr int ST_MAX_F = 64;             // new frames per stream and call: the lanes of the commit's wave
constexpr int ST_LABELS = 2048;          // labels a slot holds
constexpr int ST_JP_MAX = 1024;          // bf16: 64 rows of jp + 8 bf16 stay inside the 160 KiB of LDS
constexpr int ST_JP_MAX_F32 = 8192;

struct SlotHdr {  // 32 bytes; all zero: a fresh stream
  double score;
  int32_t frames, nlabels, status, started, pad[2];
};
struct SlotLayout {
  size_t dproj, cs, hs, labels, total;
};
SlotLayout slot_layout(int dtype, const EmTransducerWeights* w) {
  const size_t es = dtype == EM_BF16 ? 2 : 4, n = (size_t)w->num_layers * w->d;
  SlotLayout o;
  o.dproj = sizeof(SlotHdr);
  o.cs = o.dproj + (size_t)w->jp * 4;
  o.hs = o.cs + n * 4;
  o.labels = o.hs + n * es;  // (d is a multiple of 64: the labels stay 4-byte aligned)
  o.total = em_host::align_up(o.labels + (size_t)ST_LABELS * 4);
  return o;
}

struct Tick {
  unsigned char* slab;
  SlotLayout lay;
  const int32_t *slot_ids, *nframes;
  const float *enc_proj, *out_b;
  const void* lin_out;
  int32_t n_slots, S, F, V, jp, blank, L, d, nslices;
  // workspace
  float4* part;    // [S][F][nslices]
  float* dproj;    // [S][jp]
  int32_t *tok, *nfr, *cursor, *nl0, *mask0;  // [S]
  int32_t* masks;      // [F][S]: round r's advancing streams
  int32_t* rows_live;  // [F + 1]: streams with rows left at the start of round r (r >= 1)
  int32_t* adv_live;   // [F]: streams that advance in round r
  // outputs
  double* out_score;
  int32_t *out_info, *out_labels, *tr_tok;
  float *tr_top, *tr_margin;
};

__device__ __forceinline__ unsigned char* slot_of(const Tick& a, int s) {
  const int id = a.slot_ids[s];
  return id >= 0 && id < a.n_slots ? a.slab + (size_t)id * a.lay.total : nullptr;
}
__device__ __forceinline__ bool row_live(const Tick& a, int g) {
  if (g >= a.S * a.F) return false;
  const int s = g / a.F, f = g - s * a.F;
  return f >= a.cursor[s] && f < a.nfr[s];
}

// ---- a tick begins: the slots' states become rows [layer][s][d] of the advance's buffers, the tick's per-stream words
// are set, block 0 clears the rounds' masks and counters
template <typename T>
__global__ __launch_bounds__(256) void begin_kernel(const Tick a, T* __restrict__ hs, float* __restrict__ cs) {
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s == 0) {
    for (int i = tid; i < a.F * a.S; i += 256) a.masks[i] = 0;
    for (int i = tid; i <= a.F; i += 256) a.rows_live[i] = 0;
    for (int i = tid; i < a.F; i += 256) a.adv_live[i] = 0;
  }
  unsigned char* slot = slot_of(a, s);
  const T* sh = (const T*)(slot + a.lay.hs);
  const float* sc = (const float*)(slot + a.lay.cs);
  const float* sp = (const float*)(slot + a.lay.dproj);
  for (int l = 0; l < a.L; ++l)
    for (int c = tid; c < a.d; c += 256) {
      const size_t o = ((size_t)l * a.S + s) * a.d + c;
      hs[o] = slot ? sh[l * a.d + c] : from_f32<T>(0.f);
      cs[o] = slot ? sc[l * a.d + c] : 0.f;
    }
  for (int c = tid; c < a.jp; c += 256) a.dproj[(size_t)s * a.jp + c] = slot ? sp[c] : 0.f;
  if (tid != 0) return;
  SlotHdr* h = (SlotHdr*)slot;
  const int n = min(max(a.nframes[s], 0), a.F);
  a.nfr[s] = h && h->status == 0 ? n : 0;
  a.cursor[s] = 0;
  a.nl0[s] = h ? h->nlabels : 0;
  a.tok[s] = a.blank;
  a.mask0[s] = h && h->started == 0;  // a fresh stream: the blank from the zero state, as the one-shot walk begins
  if (h) h->started = 1;
}

__device__ __forceinline__ float fast_tanh(float x) {  // |error| ~ 1e-7, far below the bf16 rounding that follows
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x));
}

// ---- the head, bf16: grid (row tiles, vocabulary slices)
__global__ __launch_bounds__(64 * ST_WAVES) void head_bf16_kernel(const Tick a, const int32_t* __restrict__ live) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
  __shared__ int alive[ST_ROWS];
  __shared__ float4 red[ST_WAVES][ST_ROWS];
  if (live && *live == 0) return;
  bf16* zs = (bf16*)st_smem;
  const int jp = a.jp, ldz = jp + 8, V = a.V;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int g0 = blockIdx.x * ST_ROWS;
  int mine = 0;
  if (threadIdx.x < ST_ROWS) alive[threadIdx.x] = mine = row_live(a, g0 + threadIdx.x);
  if (!__syncthreads_or(mine)) return;  // (workgroup-uniform: no row of this tile is left)
  // z: wave w makes the rows w, w + 5, ...; a lane four channels at a time
  for (int rl = wave; rl < ST_ROWS; rl += ST_WAVES) {
    bf16* dst = zs + (size_t)rl * ldz;
    if (alive[rl]) {
      const int g = g0 + rl;
      const float* e = a.enc_proj + (size_t)g * jp;
      const float* d = a.dproj + (size_t)(g / a.F) * jp;
      for (int c = lane * 4; c < jp; c += 256) {
        const f32x4 ev = *(const f32x4*)(e + c), dv = *(const f32x4*)(d + c);
        bf16x4 z;
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = (bf16)fast_tanh(ev[i] + dv[i]);
        *(bf16x4*)(dst + c) = z;
      }
    } else {
      for (int c = lane * 4; c < jp; c += 256) *(bf16x4*)(dst + c) = (bf16x4){(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
    }
  }
  __syncthreads();
  const int tp = blockIdx.y * ST_WAVES + wave;  // this wave's pair of column tiles: columns tp * 32 .. + 31
  f32x4 acc[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (tp * 32 < V) {  // (wave-uniform)
    const bf16* w = (const bf16*)a.lin_out;
    const bf16* arow = zs + (size_t)lr * ldz + lg * 8;
    const int nch = jp >> 6;  // chunks of two k-steps (jp % 64 == 0)
    auto load_chunk = [&](int c, bf16x8(&f)[2][2]) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = (2 * tp + ct) * 16 + lr;
        const bf16* wrow = w + (size_t)min(col, V - 1) * jp + lg * 8 + c * 64;
        f[ct][0] = *(const bf16x8*)wrow;
        f[ct][1] = *(const bf16x8*)(wrow + 32);
      }
    };
    bf16x8 cur[2][2], nxt[2][2];
    load_chunk(0, cur);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 2; ++i) nxt[ct][i] = cur[ct][i];
    for (int c = 0; c < nch; ++c) {
      if (c + 1 < nch) load_chunk(c + 1, nxt);  // the next chunk's fragments fly during this chunk's 16 MFMAs
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          const bf16x8 af = *(const bf16x8*)(arow + (size_t)rt * 16 * ldz + (c * 2 + i) * 32);
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) acc[ct][rt] = Mma<bf16>::mma(af, cur[ct][i], acc[ct][rt]);
        }
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int i = 0; i < 2; ++i) cur[ct][i] = nxt[ct][i];
    }
  }
  float bias[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) bias[ct] = a.out_b[min((2 * tp + ct) * 16 + lr, V - 1)];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Top t{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = (2 * tp + ct) * 16 + lr;
        if (col < V) t = top_merge(t, Top{acc[ct][rt][q] + bias[ct], col, -INFINITY, 1.f});
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) t = top_merge(t, top_shfl_xor(t, o));  // the 16 lanes of one row group
      if (lr == 0) red[wave][rt * 16 + lg * 4 + q] = make_float4(t.m1, __int_as_float(t.i1), t.m2, t.s);
    }
  __syncthreads();
  if (threadIdx.x < ST_ROWS && alive[threadIdx.x]) {
    const int rl = threadIdx.x;
    Top t{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
#pragma unroll
    for (int wv = 0; wv < ST_WAVES; ++wv) {
      const float4 p = red[wv][rl];
      t = top_merge(t, Top{p.x, __float_as_int(p.y), p.z, p.w});
    }
    a.part[(size_t)(g0 + rl) * a.nslices + blockIdx.y] = make_float4(t.m1, __int_as_float(t.i1), t.m2, t.s);
  }
}

// ---- the head, f32 (parity path): a workgroup per row, one record per row (nslices == 1)
__global__ __launch_bounds__(256) void head_f32_kernel(const Tick a, const int32_t* __restrict__ live) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
  __shared__ float4 red[4];
  if (live && *live == 0) return;
  float* z = (float*)st_smem;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!row_live(a, g)) return;  // (workgroup-uniform)
  const int jp = a.jp, V = a.V;
  const float* e = a.enc_proj + (size_t)g * jp;
  const float* d = a.dproj + (size_t)(g / a.F) * jp;
  for (int c = tid; c < jp; c += 256) z[c] = tanhf(e[c] + d[c]);
  __syncthreads();
  const float* w = (const float*)a.lin_out;
  Top t{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
  for (int v = tid; v < V; v += 256) {
    const float* wr = w + (size_t)v * jp;
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < jp; c += 4) {
      const f32x4 wv = *(const f32x4*)(wr + c), zv = *(const f32x4*)(z + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[i] = fmaf(zv[i], wv[i], sum[i]);
    }
    t = top_merge(t, Top{((sum[0] + sum[1]) + (sum[2] + sum[3])) + a.out_b[v], v, -INFINITY, 1.f});
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) t = top_merge(t, top_shfl_xor(t, o));
  if (lane == 0) red[wave] = make_float4(t.m1, __int_as_float(t.i1), t.m2, t.s);
  __syncthreads();
  if (tid != 0) return;
  Top r{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
  for (int i = 0; i < 4; ++i) r = top_merge(r, Top{red[i].x, __float_as_int(red[i].y), red[i].z, red[i].w});
  a.part[(size_t)g * a.nslices] = make_float4(r.m1, __int_as_float(r.i1), r.m2, r.s);
}

// ---- the commit of round r: one wave per stream, lane j the frame cursor + j
__global__ __launch_bounds__(64) void commit_kernel(const Tick a, int r) {
  __shared__ float lps[64];
  if (r > 0 && a.rows_live[r] == 0) return;
  const int s = blockIdx.x, lane = threadIdx.x;
  const int cur = a.cursor[s], n = a.nfr[s];
  if (cur >= n) return;  // (no rows: never a slot that is out of range, whose nfr is 0)
  unsigned char* slot = slot_of(a, s);
  SlotHdr* h = (SlotHdr*)slot;
  const int nl = h->nlabels;
  const int f = cur + lane;
  const bool valid = f < n;
  Top t{-INFINITY, 0x7fffffff, -INFINITY, 0.f};
  if (valid) {
    const float4* p = a.part + (size_t)(s * a.F + f) * a.nslices;
    for (int i = 0; i < a.nslices; ++i) t = top_merge(t, Top{p[i].x, __float_as_int(p[i].y), p[i].z, p[i].w});
  }
  const float lp = valid ? -logf(t.s) : 0.f;  // logit_max - logsumexp
  lps[lane] = lp;
  const unsigned long long em = __ballot(valid && t.i1 != a.blank);
  const int fe = em ? __ffsll((long long)em) - 1 : -1;  // the lane of the first label, if any
  const bool full = fe >= 0 && nl >= ST_LABELS;       // no room for it: the stream stops in front of that frame
  const int ncommit = fe < 0 ? n - cur : full ? fe : fe + 1;
  const int label = __shfl(t.i1, fe < 0 ? 0 : fe, 64);
  __syncthreads();
  if (a.tr_tok && lane < ncommit) {
    const size_t o = (size_t)s * a.F + f;
    a.tr_tok[o] = t.i1;
    a.tr_top[o] = lp;
    a.tr_margin[o] = t.m1 - t.m2;
  }
  if (lane != 0) return;
  double sc = h->score;
  for (int j = 0; j < ncommit; ++j) sc += (double)lps[j];
  h->score = sc;
  h->frames += ncommit;
  int next = n;
  if (full) {
    h->status = 1;
  } else if (fe >= 0) {
    ((int32_t*)(slot + a.lay.labels))[nl] = label;
    h->nlabels = nl + 1;
    a.tok[s] = label;
    a.masks[(size_t)r * a.S + s] = 1;
    atomicAdd(a.adv_live + r, 1);
    next = cur + fe + 1;
    if (next < n) atomicAdd(a.rows_live + r + 1, 1);
  }
  a.cursor[s] = next;
}

// ---- a tick ends: the states go back to their slots, the tick's results to the outputs
template <typename T>
__global__ __launch_bounds__(256) void end_kernel(const Tick a, const T* __restrict__ hs, const float* __restrict__ cs) {
  const int s = blockIdx.x, tid = threadIdx.x;
  unsigned char* slot = slot_of(a, s);
  if (slot) {
    T* sh = (T*)(slot + a.lay.hs);
    float* sc = (float*)(slot + a.lay.cs);
    float* sp = (float*)(slot + a.lay.dproj);
    for (int l = 0; l < a.L; ++l)
      for (int c = tid; c < a.d; c += 256) {
        const size_t o = ((size_t)l * a.S + s) * a.d + c;
        sh[l * a.d + c] = hs[o];
        sc[l * a.d + c] = cs[o];
      }
    for (int c = tid; c < a.jp; c += 256) sp[c] = a.dproj[(size_t)s * a.jp + c];
  }
  const SlotHdr* h = (const SlotHdr*)slot;
  const int nl0 = a.nl0[s], nl = h ? h->nlabels : 0;
  const int32_t* labels = (const int32_t*)(slot + a.lay.labels);
  for (int j = tid; j < a.F; j += 256) a.out_labels[(size_t)s * a.F + j] = nl0 + j < nl ? labels[nl0 + j] : -1;
  if (tid != 0) return;
  int rounds = 1;
  for (int r = 1; r < a.F; ++r) rounds += a.rows_live[r] > 0;
  a.out_score[s] = h ? h->score : 0.0;
  int32_t* o = a.out_info + (size_t)s * 5;
  o[0] = nl0;
  o[1] = nl;
  o[2] = h ? h->status : 3;
  o[3] = h ? h->frames : 0;
  o[4] = rounds;
}

// ---- lin_enc on the new frames: out[r][j] = x[r] . w[j] + b[j].  em_gemm picks its kernel by the number of rows, and
// with the kernel the order of a row's sum; a tick's rows must not depend on how many travel together.  The shape of
// proj_kernel with a grid over row tiles: a workgroup owns 16 columns of 64 rows, the waves split D, wave w finishes row
// tile w - one MFMA row per row, the same k order whatever M is.
template <typename T>
__global__ __launch_bounds__(256) void enc_proj_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                       const float* __restrict__ b, int M, int D, int jp,
                                                       float* __restrict__ out) {
  using MM = Mma<T>;
  __shared__ f32x4 red[4][MAXRT][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int r0 = blockIdx.y * MAXROWS;
  const int n = min(MAXROWS, M - r0), nrt = (n + 15) >> 4;
  const int j = blockIdx.x * 16 + lr;  // (jp is a multiple of 16: always a column)
  const T* arow[MAXRT];
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt) arow[rt] = x + (size_t)(r0 + min(rt * 16 + lr, n - 1)) * D + lg * MM::EPL;
  f32x4 acc[MAXRT];
  zero_acc(acc);
  mma_span<T>(arow, w + (size_t)j * D + lg * MM::EPL, wave, 4, D / MM::K, nrt, acc);
#pragma unroll
  for (int rt = 0; rt < MAXRT; ++rt)
    if (rt < nrt) red[wave][rt][lane] = acc[rt];
  __syncthreads();
  if (wave >= nrt) return;
  const f32x4 v = (red[0][wave][lane] + red[1][wave][lane]) + (red[2][wave][lane] + red[3][wave][lane]);
  const float bias = b[j];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 16 + lg * 4 + q;
    if (r < n) out[(size_t)(r0 + r) * jp + j] = v[q] + bias;
  }
}

int check_stream(int dtype, const EmTransducerWeights* w) {
  EM_TRY(check_weights(dtype, w));
  if (w->jp > (dtype == EM_BF16 ? ST_JP_MAX : ST_JP_MAX_F32)) return EM_ERR_UNSUPPORTED;
  return EM_OK;
}

// workspace of a tick: the carve-up below and em_transducer_greedy_extend_workspace_bytes must agree
struct TickWs {
  size_t part, dproj, hs, cs, words, masks, counters, total;
};
TickWs tick_layout(int dtype, const EmTransducerWeights* w, int S, int F) {
  const size_t es = dtype == EM_BF16 ? 2 : 4;
  const int nslices = dtype == EM_BF16 ? em_cdiv(w->vocab, ST_SLICE) : 1;
  TickWs o;
  em_host::Bump b;
  o.part = b.take((size_t)S * F * nslices * sizeof(float4));
  o.dproj = b.take((size_t)S * w->jp * 4);
  o.hs = b.take((size_t)2 * w->num_layers * S * w->d * es);
  o.cs = b.take((size_t)2 * w->num_layers * S * w->d * 4);
  o.words = b.take((size_t)5 * S * 4);
  o.masks = b.take((size_t)F * S * 4);
  o.counters = b.take((size_t)(2 * F + 1) * 4);
  o.total = b.o;
  return o;
}

EmLdsCap head_cap;

template <typename T>
int extend_t(int dtype, const EmTransducerWeights* w, Tick a, unsigned char* ws, hipStream_t s) {
  const int S = a.S, F = a.F;
  const TickWs o = tick_layout(dtype, w, S, F);
  a.part = (float4*)(ws + o.part);
  a.dproj = (float*)(ws + o.dproj);
  int32_t* words = (int32_t*)(ws + o.words);
  a.tok = words; a.nfr = words + S; a.cursor = words + 2 * S; a.nl0 = words + 3 * S; a.mask0 = words + 4 * S;
  a.masks = (int32_t*)(ws + o.masks);
  a.rows_live = (int32_t*)(ws + o.counters);
  a.adv_live = a.rows_live + F + 1;
  T* hs = (T*)(ws + o.hs);
  float* cs = (float*)(ws + o.cs);
  const size_t ls = (size_t)S * w->d, buf = ls * w->num_layers;
  int cur = 0;
  // the masked streams' prediction network and lin_dec, S > 64 in slices of 64 rows
  auto advance = [&](const int32_t* mask, const int32_t* live) -> int {
    for (int r0 = 0; r0 < S; r0 += MAXROWS) {
      const int m = S - r0 < MAXROWS ? S - r0 : MAXROWS;
      const size_t q = (size_t)r0 * w->d;
      EM_TRY(dec_rows<T>(w, a.tok + r0, mask + r0, m, ls, hs + cur * buf + q, cs + cur * buf + q, hs + (cur ^ 1) * buf + q,
                         cs + (cur ^ 1) * buf + q, nullptr, a.dproj + (size_t)r0 * w->jp, nullptr, 0, 0, (T*)nullptr, s, live));
    }
    cur ^= 1;
    return EM_OK;
  };
  hipLaunchKernelGGL(begin_kernel<T>, dim3(S), dim3(256), 0, s, a, hs, cs);
  EM_TRY(advance(a.mask0, nullptr));  // fresh streams: the blank from the zero state
  const size_t lds = dtype == EM_BF16 ? (size_t)ST_ROWS * (w->jp + 8) * 2 : (size_t)w->jp * 4;
  if (dtype == EM_BF16) EM_TRY(em_raise_lds_cap((const void*)head_bf16_kernel, lds, &head_cap));
  for (int r = 0; r < F; ++r) {
    const int32_t* live = r ? a.rows_live + r : nullptr;
    if (dtype == EM_BF16)
      hipLaunchKernelGGL(head_bf16_kernel, dim3(em_cdiv(S * F, ST_ROWS), a.nslices), dim3(64 * ST_WAVES), lds, s, a, live);
    else
      hipLaunchKernelGGL(head_f32_kernel, dim3(S * F), dim3(256), lds, s, a, live);
    hipLaunchKernelGGL(commit_kernel, dim3(S), dim3(64), 0, s, a, r);
    EM_TRY(advance(a.masks + (size_t)r * S, a.adv_live + r));
  }
  hipLaunchKernelGGL(end_kernel<T>, dim3(S), dim3(256), 0, s, a, (const T*)(hs + cur * buf), (const float*)(cs + cur * buf));
  EM_CHECK_LAUNCH();
  return EM_OK;
}

}  // namespace

extern "C" size_t em_transducer_stream_slot_bytes(int dtype, const EmTransducerWeights* w) {
  return check_stream(dtype, w) == EM_OK ? slot_layout(dtype, w).total : 0;
}

extern "C" void em_transducer_stream_limits(int32_t* S_max, int32_t* F_max, int32_t* labels_max) {
  if (S_max) *S_max = ST_MAX_S;
  if (F_max) *F_max = ST_MAX_F;
  if (labels_max) *labels_max = ST_LABELS;
}

extern "C" int em_transducer_stream_enc_proj(int dtype, const void* enc, const void* lin_enc, const float* enc_b, int32_t M,
                                             int32_t D, int32_t jp, float* enc_proj, void* stream) {
  if (dtype != EM_F32 && dtype != EM_BF16) return EM_ERR_BAD_ARG;
  if (!enc || !lin_enc || !enc_b || !enc_proj || M < 1 || D < 1 || jp < 1) return EM_ERR_BAD_ARG;
  if (D % 64 != 0 || jp % 64 != 0 || M > ST_MAX_S * ST_MAX_F) return EM_ERR_UNSUPPORTED;
  const dim3 grid(jp / 16, em_cdiv(M, MAXROWS));
  if (dtype == EM_BF16)
    hipLaunchKernelGGL(enc_proj_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)enc, (const bf16*)lin_enc,
                       enc_b, M, D, jp, enc_proj);
  else
    hipLaunchKernelGGL(enc_proj_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)enc,
                       (const float*)lin_enc, enc_b, M, D, jp, enc_proj);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" size_t em_transducer_greedy_extend_workspace_bytes(int dtype, const EmTransducerWeights* w, int32_t S, int32_t F) {
  if (check_stream(dtype, w) != EM_OK || S < 1 || S > ST_MAX_S || F < 1 || F > ST_MAX_F) return 0;
  return tick_layout(dtype, w, S, F).total;
}

extern "C" int em_transducer_greedy_extend(int dtype, const EmTransducerWeights* w, void* slab, int32_t n_slots,
                                           const int32_t* slot_ids, const float* enc_proj, const int32_t* nframes, int32_t S,
                                           int32_t F, double* out_score, int32_t* out_info, int32_t* out_labels,
                                           int32_t* frame_tok, float* frame_top, float* frame_margin, void* ws,
                                           size_t ws_bytes, void* stream) {
  EM_TRY(check_stream(dtype, w));
  if (!slab || n_slots < 1 || !slot_ids || !enc_proj || !nframes || !out_score || !out_info || !out_labels) return EM_ERR_BAD_ARG;
  if (frame_tok && (!frame_top || !frame_margin)) return EM_ERR_BAD_ARG;
  if (S < 1 || F < 1) return EM_ERR_BAD_ARG;
  if (S > ST_MAX_S || F > ST_MAX_F) return EM_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < tick_layout(dtype, w, S, F).total) return EM_ERR_WORKSPACE;
  Tick a = {};
  a.slab = (unsigned char*)slab;
  a.lay = slot_layout(dtype, w);
  a.slot_ids = slot_ids; a.nframes = nframes; a.enc_proj = enc_proj; a.out_b = w->out_b; a.lin_out = w->lin_out;
  a.n_slots = n_slots; a.S = S; a.F = F; a.V = w->vocab; a.jp = w->jp; a.blank = w->blank; a.L = w->num_layers; a.d = w->d;
  a.nslices = dtype == EM_BF16 ? em_cdiv(w->vocab, ST_SLICE) : 1;
  a.out_score = out_score; a.out_info = out_info; a.out_labels = out_labels;
  a.tr_tok = frame_tok; a.tr_top = frame_top; a.tr_margin = frame_margin;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EM_BF16) return extend_t<bf16>(dtype, w, a, (unsigned char*)ws, s);
  return extend_t<float>(dtype, w, a, (unsigned char*)ws, s);
}
