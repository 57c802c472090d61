// Time-synchronous CTC prefix beam search with n-gram fusion (BeamSearchTimeSync of espnet/nets/beam_search_timesync.py for
// ctc_weight = 1, restated in include/espnet_amd.h at em_ctc_tsync_search), in two launches:
//
//   frame_topk_kernel   one wave per frame: the K best (id, log-prob) pairs of a row, descending, ties to the lower id, and
//                       the row's blank log-prob.  Every lane keeps the best not-yet-taken element of its own columns; a
//                       round is one wave arg-max and a rescan of the winning lane's V / 64 columns: V + K V / 64 loads per
//                       row, no sort, no LDS.
//   tsync_kernel        one workgroup per utterance walks all its frames; nothing is read back and no workgroup waits for
//                       another.  ONE body, two instantiations: <false> is em_ctc_tsync_search (the whole utterance from the
//                       empty prefix, everything between two frames in LDS and scratch), <true> is em_ctc_tsync_extend (the
//                       frames of one call, between two calls everything in the row's PERSISTENT slot, see "The slot").
//
// The walk.  The beam holds at most W prefixes; a frame proposes the fixed grid of W (K + 1) SLOTS: slot (i, j < K) is beam
// entry i extended by candidate j, slot (i, K) is entry i itself (its blank and repeat mass).  Two extension slots never
// hold the same sequence (the beam's sequences are distinct), an extension slot equals at most one beam entry (then its
// mass is MERGED into that entry's own slot, one contributor at most), so every member of the frame owns one slot and no
// sum depends on the order in which threads arrive: the result is bit-reproducible.
//
// Prefix identity is by token sequence.  A sequence is (parent node, last token) over an append-only arena of nodes
// (parent, token); a beam entry that enters at frame t with rank r takes node 1 + t W + r, so a prefix that left the beam
// and is created again gets ANOTHER node: nodes are never compared by id alone.  Two sequences are equal when their
// 64-bit rolling hashes, lengths and last tokens agree AND the lock-step walk of both parent chains meets (the same node:
// the rest is shared) or reaches both roots with equal tokens all the way; the hash only finds the entry.
//   l2 in hyps: a scan of the W beam entries;
//   l2 in dp:   an open-addressed table in LDS (linear probing, at most half full, rebuilt every frame from the members of
//               the frame that did not stay in the beam) over the slot records (hash, parent, token, length, p_nb, p_b).
// Every loop is bounded at launch: frames (xlens / n_new), slots, K, W, probes (<= table size), chain steps (<= T + 1, for
// the resumable form max_frames + 1), binary search halvings (32).
//
// The slot (em_ctc_tsync_extend).  What the one-shot walk carries from one frame to the next is the beam (LDS), the slot
// records of the last frame's members that left the beam (scratch; the LDS table only indexes them) and the node arena
// (scratch).  A slot of the state slab holds exactly that, at offsets that depend on (K, W, max_frames) alone:
//   header  16 words: magic, frames consumed, beam count, parity of the (p_nb, p_b) halves, K, W, max_frames as first used
//   the one-shot scratch layout for T = max_frames: dp_hash, the arena (node ids 1 + t W + r with the ABSOLUTE frame t),
//           v_nb / v_b [2][S], v_ng, dp_par / dp_tok / dp_ntok
//   the beam entries: hash, node, par, tok, ntok, nb, b, prev, ng, ctx[]
//   a flag byte per grid slot: a member of the last frame that left the beam (the table is rebuilt from these on entry;
//           which entry of the table a record lands in depends on the insertion order, what a probe FINDS does not: the
//           members of a frame are distinct sequences and a hit compares the whole sequence)
// Nothing in a slot is an address or a slot index, so a slot may be copied anywhere.  A row with reset != 0 reads nothing
// of its slot; emission (the <eos> term, the final order) works on LDS copies and never changes the slot.
#include "em_common.h"
#include "ngram_trie.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int TS_W_MAX = 32, TS_K_MAX = 64;
constexpr int TS_S_MAX = TS_W_MAX * (TS_K_MAX + 1);
constexpr int TS_CAP_MAX = 8192;  // the power of two >= 2 * TS_S_MAX
constexpr int TS_THREADS = 512;
constexpr int TS_LD = NG_MAX - 1;
static_assert(TS_CAP_MAX >= 2 * TS_S_MAX, "the prefix table must stay at most half full");

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------- per-frame top K
__device__ __forceinline__ bool tk_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(256) void frame_topk_kernel(const float* __restrict__ lp, int M, int V, int K, int blank,
                                                         int32_t* __restrict__ cand_id, float* __restrict__ cand_lp,
                                                         float* __restrict__ blank_lp) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // (wave-uniform)
  const float* x = lp + row * V;
  if (lane == 0) blank_lp[row] = x[blank];
  float pv = INFINITY, bv;  // the lane's last pick and its best element after it
  int pi = -1, bi;
  for (int r = 0; r < K; ++r) {
    if (r == 0 || pi >= 0) {  // (only the lane whose element was taken last round rescans)
      bv = -INFINITY;
      bi = INT_MAX;
      for (int v = lane; v < V; v += 64) {
        const float e = x[v];
        if (tk_better(pv, pi, e, v) && tk_better(e, v, bv, bi)) {
          bv = e;
          bi = v;
        }
      }
      pi = -1;
    }
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (tk_better(ov, oi, wv, wi)) {
        wv = ov;
        wi = oi;
      }
    }
    if (wi == bi && bi != INT_MAX) {  // taken: this lane's next round starts behind it
      pv = bv;
      pi = bi;
    }
    if (lane == 0) {
      cand_id[row * K + r] = wi == INT_MAX ? 0 : wi;  // (nothing left: a row holding NaN)
      cand_lp[row * K + r] = wi == INT_MAX ? -INFINITY : wv;
    }
  }
}

// ---------------------------------------------------------------------------------------------- the walk
struct TsArgs {
  const int32_t* cand_id;
  const float *cand_lp, *blank_lp;
  const int32_t* xlens;
  int T, K, W, nbest, sos, blank, cap, has_ng;
  int Tn;  // frames the node arena and a tokens row hold: T (one shot) or max_frames (resumable)
  float w_ctc, w_ng, pen;
  int32_t *tokens, *lens, *count;
  float *score, *score_ctc, *score_ng, *score_len;
  char* ws;  // one shot: scratch, ws_per per utterance; resumable: the state slab, ws_per = slot_bytes
  size_t ws_per;
  // the resumable form only
  const int32_t *n_new, *slot, *reset;
  int32_t *frames, *status;
  int n_slots;
};

constexpr int TS_MAGIC = 0x54535931, TS_HDR_WORDS = 16;
enum { TS_H_MAGIC = 0, TS_H_FRAMES, TS_H_COUNT, TS_H_PARITY, TS_H_K, TS_H_W, TS_H_TMAX };

__host__ __device__ inline size_t ts_ws_per(long T, long K, long W) {
  const long S = W * (K + 1), NN = T * W + 1;
  return (size_t)(40 * S + 8 * NN);
}

__host__ __device__ inline size_t ts_beam_bytes(long W) { return (size_t)((W * (8 + 4 * 8 + 4 * TS_LD) + 7) & ~7L); }
// a slot: header | the one-shot layout for T = max_frames | beam entries | a flag byte per grid slot
__host__ __device__ inline size_t ts_state_per(long Tn, long K, long W) {
  return (size_t)((4 * TS_HDR_WORDS + ts_ws_per(Tn, K, W) + ts_beam_bytes(W) + W * (K + 1) + 15) & ~15L);
}

__device__ __forceinline__ float lae(float a, float b) {  // logaddexp, shifted by the larger term; -inf, -inf -> -inf
  const float m = fmaxf(a, b);
  if (!(m > -INFINITY)) return -INFINITY;
  return m + log1pf(expf(fminf(a, b) - m));
}

__device__ __forceinline__ u64 ts_hash(u64 h, int c) {
  h ^= (u64)(unsigned)c + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

// are the sequences ending in the nodes a and b (of equal length) equal?  At most T + 1 steps.
__device__ __forceinline__ bool chain_equal(const int32_t* par, const int32_t* tok, int a, int b, int T) {
  for (int st = 0; st <= T; ++st) {
    if (a == b) return true;  // the same node (or both behind the root): the rest is shared
    if (a < 0 || b < 0) return false;
    if (tok[a] != tok[b]) return false;
    a = par[a];
    b = par[b];
  }
  return false;
}

__device__ __forceinline__ float ts_total(float w_ctc, float lse, float w_ng, float ng, float pen, int ntok) {
  if (!(lse > -INFINITY)) return -INFINITY;
  return w_ctc * lse + w_ng * ng + pen * (float)ntok;
}

template <bool RS>
__global__ __launch_bounds__(TS_THREADS) void tsync_kernel(EmNgramModel m, TsArgs a) {
  __shared__ int32_t s_tab[TS_CAP_MAX];
  __shared__ float s_score[TS_S_MAX];
  __shared__ unsigned char s_keep[TS_S_MAX];
  __shared__ int h_node[2][TS_W_MAX], h_par[2][TS_W_MAX], h_tok[2][TS_W_MAX], h_ntok[2][TS_W_MAX];
  __shared__ u64 h_hash[2][TS_W_MAX];
  __shared__ float h_nb[2][TS_W_MAX], h_b[2][TS_W_MAX], h_prev[2][TS_W_MAX], h_ng[2][TS_W_MAX];
  __shared__ int32_t h_ctx[2][TS_W_MAX][TS_LD];
  __shared__ float s_merge[TS_W_MAX];
  __shared__ int s_merged[TS_W_MAX], s_sel[TS_W_MAX];
  __shared__ int s_cand[TS_K_MAX];
  __shared__ float s_clp[TS_K_MAX];
  __shared__ float f_final[TS_W_MAX], f_ng[TS_W_MAX];
  __shared__ int s_count;

  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int T = a.T, Tn = a.Tn, K = a.K, W = a.W, K1 = a.K + 1, S = a.W * K1, cap = a.cap, blank = a.blank;
  const int nord = a.has_ng ? m.order - 1 : 0;  // context nodes carried per entry
  // t0 frames are behind this row, Tb are walked now; st: the row's status; fresh: the walk starts from the empty prefix
  int Tb, t0 = 0, cnt0 = 0, st = 0;
  bool fresh = true;
  char* ws;
  int32_t* hdr = nullptr;
  if (RS) {
    const int sl = a.slot[b];
    Tb = a.n_new[b];
    fresh = a.reset[b] != 0;
    if (sl < 0 || sl >= a.n_slots) {
      st = 3;
      ws = a.ws;  // (never dereferenced)
    } else {
      hdr = (int32_t*)(a.ws + (size_t)sl * a.ws_per);
      ws = (char*)(hdr + TS_HDR_WORDS);
      if (!fresh) {  // (every thread reads the same words; the header is rewritten behind the last barrier only)
        if (hdr[TS_H_MAGIC] != TS_MAGIC || hdr[TS_H_K] != K || hdr[TS_H_W] != W || hdr[TS_H_TMAX] != Tn) st = 2;
        else {
          t0 = hdr[TS_H_FRAMES];
          cnt0 = hdr[TS_H_COUNT];
          t0 = t0 < 0 ? 0 : (t0 > Tn ? Tn : t0);
          cnt0 = cnt0 < 0 ? 0 : (cnt0 > W ? W : cnt0);
        }
      }
    }
  } else {
    Tb = a.xlens[b];
    ws = a.ws + (size_t)b * a.ws_per;
  }
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  if (RS) {
    if (st >= 2) Tb = 0;
    else if (t0 + Tb > Tn) {  // all or nothing
      st = 1;
      Tb = 0;
    }
  }

  const long NN = (long)Tn * W + 1;
  u64* dp_hash = (u64*)ws;
  int32_t* node_par = (int32_t*)(dp_hash + S);
  int32_t* node_tok = node_par + NN;
  float* v_nb = (float*)(node_tok + NN);  // [2][S]
  float* v_b = v_nb + 2 * S;              // [2][S]
  float* v_ng = v_b + 2 * S;              // [S]
  int32_t* dp_par = (int32_t*)(v_ng + S);
  int32_t* dp_tok = dp_par + S;
  int32_t* dp_ntok = dp_tok + S;
  // (the resumable form's beam entries and flags, behind the one-shot layout)
  u64* g_hash = (u64*)(dp_ntok + S);
  int32_t* g_i = (int32_t*)(g_hash + W);  // node, par, tok, ntok [W] each
  float* g_f = (float*)(g_i + 4 * W);     // nb, b, prev, ng [W] each
  int32_t* g_ctx = (int32_t*)(g_f + 4 * W);
  unsigned char* g_left = (unsigned char*)g_hash + ts_beam_bytes(W);

  if (RS && st >= 2) {
    if (tid == 0) s_count = 0;
  } else if (RS && !fresh) {
    if (tid < cnt0) {
      const int i = tid;
      h_hash[0][i] = g_hash[i];
      h_node[0][i] = g_i[i];
      h_par[0][i] = g_i[W + i];
      h_tok[0][i] = g_i[2 * W + i];
      h_ntok[0][i] = g_i[3 * W + i];
      h_nb[0][i] = g_f[i];
      h_b[0][i] = g_f[W + i];
      h_prev[0][i] = g_f[2 * W + i];
      h_ng[0][i] = g_f[3 * W + i];
      for (int k = 0; k < TS_LD; ++k) h_ctx[0][i][k] = g_ctx[i * TS_LD + k];
    }
    if (tid == 0) s_count = cnt0;
  } else if (tid == 0) {
    h_node[0][0] = 0;
    h_par[0][0] = -1;
    h_tok[0][0] = a.sos;
    h_ntok[0][0] = 0;
    h_hash[0][0] = ts_hash(0x243F6A8885A308D3ull, a.sos);
    h_nb[0][0] = -INFINITY;
    h_b[0][0] = 0.f;
    h_prev[0][0] = 0.f;
    h_ng[0][0] = 0.f;
    for (int k = 0; k < TS_LD; ++k) h_ctx[0][0][k] = (k == 0 && a.has_ng) ? m.bos : -1;  // the context <s> alone
    node_par[0] = -1;
    node_tok[0] = a.sos;
    s_count = 1;
  }
  for (int e = tid; e < cap; e += nthr) s_tab[e] = -1;
  __syncthreads();
  if (RS && !fresh && st < 2 && t0 > 0) {  // the table of the frame before this call, from the slot's records
    for (int s = tid; s < S; s += nthr) {
      if (!g_left[s]) continue;
      int pos = (int)(dp_hash[s] & (u64)(cap - 1));
      for (int pr = 0; pr < cap; ++pr) {
        if (atomicCAS(&s_tab[pos], -1, s) == -1) break;
        pos = (pos + 1) & (cap - 1);
      }
    }
    __syncthreads();
  }

  // the beam buffer; the (p_nb, p_b) half this frame WRITES is vb, the last frame's vb ^ 1 (vb = the frame's parity)
  int cur = 0, vb = RS && !fresh && st < 2 ? (hdr[TS_H_PARITY] & 1) : 0;
  for (int tl = 0; tl < Tb; ++tl) {
    const int t = t0 + tl;  // the absolute frame: node ids
    const int count = s_count;
    const size_t fr = (size_t)b * T + tl;
    if (tid < K) {
      s_cand[tid] = a.cand_id[fr * K + tid];
      s_clp[tid] = a.cand_lp[fr * K + tid];
    }
    if (tid < W) {
      s_merge[tid] = -INFINITY;
      s_merged[tid] = 0;
      s_sel[tid] = -1;
    }
    const float lpb = a.blank_lp[fr];
    float* nb_w = v_nb + vb * S;
    float* b_w = v_b + vb * S;
    const float* nb_r = v_nb + (vb ^ 1) * S;
    const float* b_r = v_b + (vb ^ 1) * S;
    __syncthreads();

    // A. the extension slots
    for (int s = tid; s < S; s += nthr) {
      const int i = s / K1, j = s - i * K1;
      if (j == K) continue;
      float sc = -INFINITY;
      const int c = s_cand[j];
      if (i < count && c != blank) {
        const float lpc = s_clp[j];
        float nb = lpc + (c == h_tok[cur][i] ? h_b[cur][i] : h_prev[cur][i]);
        float bb = -INFINITY;
        const u64 h2 = ts_hash(h_hash[cur][i], c);
        const int nt = h_ntok[cur][i] + 1, node_i = h_node[cur][i];
        int hit = -1;
        for (int i2 = 0; i2 < count; ++i2)
          if (h_ntok[cur][i2] == nt && h_tok[cur][i2] == c && h_hash[cur][i2] == h2 &&
              chain_equal(node_par, node_tok, h_par[cur][i2], node_i, Tn)) {
            hit = i2;
            break;
          }
        if (hit >= 0) {  // the prefix is in the beam: its own slot takes this mass (the only contributor it can have)
          s_merge[hit] = nb;
          s_merged[hit] = 1;
        } else {
          int pos = (int)(h2 & (u64)(cap - 1));
          for (int pr = 0; pr < cap; ++pr) {  // last frame's members that left the beam
            const int idx = s_tab[pos];
            if (idx < 0) break;
            if (dp_hash[idx] == h2 && dp_ntok[idx] == nt && dp_tok[idx] == c &&
                chain_equal(node_par, node_tok, dp_par[idx], node_i, Tn)) {
              const float pnb = nb_r[idx], pb = b_r[idx];
              bb = lpb + lae(pnb, pb);
              nb = lae(nb, lpc + pnb);
              break;
            }
            pos = (pos + 1) & (cap - 1);
          }
          const float ng = a.has_ng ? h_ng[cur][i] + lane_score(m, h_ctx[cur][i], tok_word(m, c)) : 0.f;
          sc = ts_total(a.w_ctc, lae(nb, bb), a.w_ng, ng, a.pen, nt);
          nb_w[s] = nb;
          b_w[s] = bb;
          v_ng[s] = ng;
        }
      }
      s_score[s] = sc;
    }
    __syncthreads();

    // B. the beam entries' own slots: blank, repeat and merged mass
    if (tid < W) {
      const int i = tid, s = i * K1 + K;
      float sc = -INFINITY;
      if (i < count) {
        bool blank_in = false;
        int rep = -1;
        for (int j = 0; j < K; ++j) {
          if (s_cand[j] == blank) blank_in = true;
          else if (s_cand[j] == h_tok[cur][i]) rep = j;
        }
        const float pb = blank_in ? lpb + h_prev[cur][i] : -INFINITY;
        float pnb = rep >= 0 ? s_clp[rep] + h_nb[cur][i] : -INFINITY;
        if (s_merged[i]) pnb = lae(pnb, s_merge[i]);
        if (blank_in || rep >= 0 || s_merged[i]) {
          sc = ts_total(a.w_ctc, lae(pnb, pb), a.w_ng, h_ng[cur][i], a.pen, h_ntok[cur][i]);
          nb_w[s] = pnb;
          b_w[s] = pb;
          v_ng[s] = h_ng[cur][i];
        }
      }
      s_score[s] = sc;
    }
    __syncthreads();

    // C. the W best members: a slot's rank is the number of slots that beat it (ties to the lower slot)
    for (int s = tid; s < S; s += nthr) {
      const float v = s_score[s];
      unsigned char keep = 0;
      if (v > -INFINITY) {
        int rank = 0;
        for (int s2 = 0; s2 < S; ++s2) {
          const float v2 = s_score[s2];
          rank += (v2 > v || (v2 == v && s2 < s)) ? 1 : 0;
        }
        if (rank < W) {
          s_sel[rank] = s;
          keep = 1;
        }
      }
      s_keep[s] = keep;
    }
    __syncthreads();

    // D. the new beam, in rank order; meanwhile the table is emptied
    const int nxt = cur ^ 1;
    if (tid < W) {
      const int r = tid, s = s_sel[r];
      if (s >= 0) {
        const int i = s / K1, j = s - i * K1;
        const float nb = nb_w[s], bb = b_w[s];
        h_nb[nxt][r] = nb;
        h_b[nxt][r] = bb;
        h_prev[nxt][r] = lae(nb, bb);
        h_ng[nxt][r] = v_ng[s];
        if (j == K) {
          h_node[nxt][r] = h_node[cur][i];
          h_par[nxt][r] = h_par[cur][i];
          h_tok[nxt][r] = h_tok[cur][i];
          h_ntok[nxt][r] = h_ntok[cur][i];
          h_hash[nxt][r] = h_hash[cur][i];
          for (int k = 0; k < TS_LD; ++k) h_ctx[nxt][r][k] = h_ctx[cur][i][k];
        } else {
          const int c = s_cand[j], node = 1 + t * W + r;
          node_par[node] = h_node[cur][i];
          node_tok[node] = c;
          h_node[nxt][r] = node;
          h_par[nxt][r] = h_node[cur][i];
          h_tok[nxt][r] = c;
          h_ntok[nxt][r] = h_ntok[cur][i] + 1;
          h_hash[nxt][r] = ts_hash(h_hash[cur][i], c);
          const int w = a.has_ng ? tok_word(m, c) : 0;
          for (int k = 0; k < TS_LD; ++k) h_ctx[nxt][r][k] = k < nord ? lane_advance_one(m, k, h_ctx[cur][i], w) : -1;
        }
      }
    }
    if (tid == 0) {
      int n = 0;
      while (n < W && s_sel[n] >= 0) ++n;
      s_count = n;
    }
    for (int e = tid; e < cap; e += nthr) s_tab[e] = -1;
    __syncthreads();

    // E. dp of the next frame: the members that did not stay in the beam, found by their hash
    for (int s = tid; s < S; s += nthr) {
      const bool left = s_score[s] > -INFINITY && !s_keep[s];
      if (RS && tl == Tb - 1) g_left[s] = left ? 1 : 0;
      if (!left) continue;
      const int i = s / K1, j = s - i * K1;
      u64 h;
      if (j == K) {
        h = h_hash[cur][i];
        dp_par[s] = h_par[cur][i];
        dp_tok[s] = h_tok[cur][i];
        dp_ntok[s] = h_ntok[cur][i];
      } else {
        h = ts_hash(h_hash[cur][i], s_cand[j]);
        dp_par[s] = h_node[cur][i];
        dp_tok[s] = s_cand[j];
        dp_ntok[s] = h_ntok[cur][i] + 1;
      }
      dp_hash[s] = h;
      int pos = (int)(h & (u64)(cap - 1));
      for (int pr = 0; pr < cap; ++pr) {
        if (atomicCAS(&s_tab[pos], -1, s) == -1) break;
        pos = (pos + 1) & (cap - 1);
      }
    }
    __syncthreads();
    cur = nxt;
    vb ^= 1;
  }

  if (RS && st < 2 && (fresh || Tb > 0)) {  // the slot takes the beam; the records and the arena are in it already
    const int n = s_count;
    if (tid < n) {
      const int i = tid;
      g_hash[i] = h_hash[cur][i];
      g_i[i] = h_node[cur][i];
      g_i[W + i] = h_par[cur][i];
      g_i[2 * W + i] = h_tok[cur][i];
      g_i[3 * W + i] = h_ntok[cur][i];
      g_f[i] = h_nb[cur][i];
      g_f[W + i] = h_b[cur][i];
      g_f[2 * W + i] = h_prev[cur][i];
      g_f[3 * W + i] = h_ng[cur][i];
      for (int k = 0; k < TS_LD; ++k) g_ctx[i * TS_LD + k] = h_ctx[cur][i][k];
    }
    if (tid == 0) {
      hdr[TS_H_MAGIC] = TS_MAGIC;
      hdr[TS_H_FRAMES] = t0 + Tb;
      hdr[TS_H_COUNT] = n;
      hdr[TS_H_PARITY] = vb;
      hdr[TS_H_K] = K;
      hdr[TS_H_W] = W;
      hdr[TS_H_TMAX] = Tn;
      for (int k = TS_H_TMAX + 1; k < TS_HDR_WORDS; ++k) hdr[k] = 0;
    }
  }
  if (RS && tid == 0) {
    a.frames[b] = t0 + Tb;
    a.status[b] = st;
  }

  // the end: the <eos> term of the n-gram, the final order, the n-best rows
  const int count = s_count, nbest = a.nbest;
  const size_t ob = (size_t)b * nbest;
  for (long e = tid; e < (long)nbest * Tn; e += nthr) a.tokens[ob * Tn + e] = -1;
  for (int e = tid; e < nbest; e += nthr) {
    a.lens[ob + e] = 0;
    a.score[ob + e] = 0.f;
    a.score_ctc[ob + e] = 0.f;
    a.score_ng[ob + e] = 0.f;
    a.score_len[ob + e] = 0.f;
  }
  if (tid < count) {
    const int i = tid;
    const float core = ts_total(a.w_ctc, h_prev[cur][i], a.w_ng, h_ng[cur][i], a.pen, h_ntok[cur][i]);
    const float e = (a.has_ng && t0 + Tb > 0) ? lane_score(m, h_ctx[cur][i], tok_word(m, a.sos)) : 0.f;
    f_ng[i] = h_ng[cur][i] + e;
    f_final[i] = core + a.w_ng * e;
  }
  __syncthreads();
  if (tid < count) {
    const int i = tid;
    const float v = f_final[i];
    int rank = 0;
    for (int i2 = 0; i2 < count; ++i2) rank += (f_final[i2] > v || (f_final[i2] == v && i2 < i)) ? 1 : 0;
    if (rank < nbest) {
      const int n = h_ntok[cur][i];
      a.lens[ob + rank] = n;
      a.score[ob + rank] = v;
      a.score_ctc[ob + rank] = h_prev[cur][i];
      a.score_ng[ob + rank] = f_ng[i];
      a.score_len[ob + rank] = (float)n;
      int node = h_node[cur][i];
      for (int k = n - 1; k >= 0 && node > 0; --k) {  // (n <= t0 + Tb <= Tn tokens; the root holds <sos>, not a token)
        a.tokens[(ob + rank) * Tn + k] = node_tok[node];
        node = node_par[node];
      }
    }
  }
  if (tid == 0) a.count[b] = count < nbest ? count : nbest;
}

int ts_check_model(const EmNgramModel* m) {
  if (m->order < 1 || m->order > NG_MAX || m->vocab <= 0 || !m->tok2word || m->unk < 0 || m->unk >= m->count[0] ||
      m->bos >= m->count[0])
    return EM_ERR_BAD_ARG;
  for (int k = 0; k < m->order; ++k) {
    if (m->count[k] < 0 || !m->wid[k] || !m->prob[k] || !m->bow[k]) return EM_ERR_BAD_ARG;
    if (k < m->order - 1 && !m->next[k]) return EM_ERR_BAD_ARG;
  }
  return EM_OK;
}

}  // namespace

extern "C" int em_ctc_frame_topk(const float* lp, int32_t M, int32_t V, int32_t K, int32_t blank, int32_t* cand_id,
                                 float* cand_lp, float* blank_lp, void* stream) {
  if (M < 0 || V <= 0 || K < 1 || K > V || blank < 0 || blank >= V) return EM_ERR_BAD_ARG;
  if (M == 0) return EM_OK;
  if (!lp || !cand_id || !cand_lp || !blank_lp) return EM_ERR_BAD_ARG;
  if ((long)M * K > INT_MAX || (long)M * V > (1L << 40)) return EM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(frame_topk_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, lp, M, V, K, blank,
                     cand_id, cand_lp, blank_lp);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" void em_ctc_tsync_limits(int32_t* W_max, int32_t* K_max) {
  if (W_max) *W_max = TS_W_MAX;
  if (K_max) *K_max = TS_K_MAX;
}

extern "C" size_t em_ctc_tsync_search_workspace_bytes(int32_t B, int32_t T, int32_t K, int32_t W) {
  if (B <= 0 || T <= 0 || K < 1 || K > TS_K_MAX || W < 1 || W > TS_W_MAX) return 0;
  if ((long)T * W + 1 > INT_MAX / 2) return 0;
  return (size_t)B * ts_ws_per(T, K, W);
}

extern "C" int em_ctc_tsync_search(const int32_t* cand_id, const float* cand_lp, const float* blank_lp, const int32_t* xlens,
                                   int32_t B, int32_t T, int32_t K, int32_t W, int32_t nbest, int32_t sos, int32_t blank,
                                   float w_ctc, float w_ngram, float penalty, const EmNgramModel* ngram, int32_t* tokens,
                                   int32_t* lens, int32_t* count, float* score, float* score_ctc, float* score_ngram,
                                   float* score_len, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || T < 1 || K < 1 || W < 1 || nbest < 1 || sos < 0 || blank < 0 || sos == blank) return EM_ERR_BAD_ARG;
  if (K > TS_K_MAX || W > TS_W_MAX || (long)T * W + 1 > INT_MAX / 2 || (long)B * nbest * T > INT_MAX) return EM_ERR_UNSUPPORTED;
  if (B == 0) return EM_OK;
  if (!cand_id || !cand_lp || !blank_lp || !xlens || !tokens || !lens || !count || !score || !score_ctc || !score_ngram ||
      !score_len || !ws)
    return EM_ERR_BAD_ARG;
  if (ngram && ts_check_model(ngram) != EM_OK) return EM_ERR_BAD_ARG;
  if (ws_bytes < (size_t)B * ts_ws_per(T, K, W)) return EM_ERR_WORKSPACE;
  TsArgs a;
  a.cand_id = cand_id, a.cand_lp = cand_lp, a.blank_lp = blank_lp, a.xlens = xlens;
  a.T = T, a.Tn = T, a.K = K, a.W = W, a.nbest = nbest, a.sos = sos, a.blank = blank;
  a.n_new = a.slot = a.reset = nullptr, a.frames = a.status = nullptr, a.n_slots = 0;
  int cap = 16;
  while (cap < 2 * W * (K + 1)) cap <<= 1;
  a.cap = cap;
  a.has_ng = ngram ? 1 : 0;
  a.w_ctc = w_ctc, a.w_ng = ngram ? w_ngram : 0.f, a.pen = penalty;
  a.tokens = tokens, a.lens = lens, a.count = count;
  a.score = score, a.score_ctc = score_ctc, a.score_ng = score_ngram, a.score_len = score_len;
  a.ws = (char*)ws, a.ws_per = ts_ws_per(T, K, W);
  EmNgramModel m = {};
  if (ngram) m = *ngram;
  hipLaunchKernelGGL(tsync_kernel<false>, dim3(B), dim3(TS_THREADS), 0, (hipStream_t)stream, m, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}

extern "C" size_t em_ctc_tsync_state_bytes(int32_t max_frames, int32_t K, int32_t W) {
  if (max_frames < 1 || K < 1 || K > TS_K_MAX || W < 1 || W > TS_W_MAX) return 0;
  if ((long)max_frames * W + 1 > INT_MAX / 2) return 0;
  return ts_state_per(max_frames, K, W);
}

extern "C" int em_ctc_tsync_extend(const int32_t* cand_id, const float* cand_lp, const float* blank_lp, const int32_t* n_new,
                                   const int32_t* slot, const int32_t* reset, int32_t S, int32_t Tc, int32_t K, int32_t W,
                                   int32_t max_frames, int32_t nbest, int32_t sos, int32_t blank, float w_ctc, float w_ngram,
                                   float penalty, const EmNgramModel* ngram, void* state, int32_t n_slots, size_t slot_bytes,
                                   int32_t* tokens, int32_t* lens, int32_t* count, float* score, float* score_ctc,
                                   float* score_ngram, float* score_len, int32_t* frames, int32_t* status, void* stream) {
  if (S < 0 || Tc < 1 || K < 1 || W < 1 || max_frames < 1 || nbest < 1 || n_slots < 1 || sos < 0 || blank < 0 || sos == blank)
    return EM_ERR_BAD_ARG;
  if (K > TS_K_MAX || W > TS_W_MAX || (long)max_frames * W + 1 > INT_MAX / 2 || (long)S * nbest * max_frames > INT_MAX ||
      (long)S * Tc * K > INT_MAX)
    return EM_ERR_UNSUPPORTED;
  if (S == 0) return EM_OK;
  if (!cand_id || !cand_lp || !blank_lp || !n_new || !slot || !reset || !state || !tokens || !lens || !count || !score ||
      !score_ctc || !score_ngram || !score_len || !frames || !status)
    return EM_ERR_BAD_ARG;
  if (ngram && ts_check_model(ngram) != EM_OK) return EM_ERR_BAD_ARG;
  if (slot_bytes < ts_state_per(max_frames, K, W)) return EM_ERR_WORKSPACE;
  if (slot_bytes % 8 != 0 || (size_t)state % 8 != 0) return EM_ERR_BAD_ARG;  // (a slot starts with 64-bit records)
  TsArgs a;
  a.cand_id = cand_id, a.cand_lp = cand_lp, a.blank_lp = blank_lp, a.xlens = nullptr;
  a.T = Tc, a.Tn = max_frames, a.K = K, a.W = W, a.nbest = nbest, a.sos = sos, a.blank = blank;
  int cap = 16;
  while (cap < 2 * W * (K + 1)) cap <<= 1;
  a.cap = cap;
  a.has_ng = ngram ? 1 : 0;
  a.w_ctc = w_ctc, a.w_ng = ngram ? w_ngram : 0.f, a.pen = penalty;
  a.tokens = tokens, a.lens = lens, a.count = count;
  a.score = score, a.score_ctc = score_ctc, a.score_ng = score_ngram, a.score_len = score_len;
  a.ws = (char*)state, a.ws_per = slot_bytes;
  a.n_new = n_new, a.slot = slot, a.reset = reset, a.frames = frames, a.status = status, a.n_slots = n_slots;
  EmNgramModel m = {};
  if (ngram) m = *ngram;
  hipLaunchKernelGGL(tsync_kernel<true>, dim3(S), dim3(TS_THREADS), 0, (hipStream_t)stream, m, a);
  EM_CHECK_LAUNCH();
  return EM_OK;
}
