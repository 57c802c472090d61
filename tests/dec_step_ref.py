"""Float64 restatement of the decoder step kernels (csrc/decoder.hip), their inputs and case lists, shared by
tests/test_cpu_dec_step_ref.py and tests/test_gpu_dec_step_parity.py.  The budget, `worst` and `assert_in_budget` are
tests/attention_ref.py's, unchanged: |got - ref| <= 3 u A + f (1 + S) A for bf16, f (1 + S) A for f32, exactly zero where
A == 0, with A = sum P |v| and S = max |score| over the VISIBLE keys of the element's row and head.

  self_case / self_operands / ref_self   cached self-attention of one label step: row r attends to kc[j][anc[r][j]], j < pos,
                                         and to its own new key (dec_self_attn_kernel, dec_self_attn_tree_kernel)
  src_case / src_operands / ref_src      source attention of the B x W rows over the memory (dec_src_attn_kernel)
  attend                                 MultiHeadedAttention.forward_attention (attention.py:121-151) on gathered keys
  ref_dec_embed / ref_lm_input_norm      embedding.py:93 and encoder.py:132-139 in float64, with their f32 error bounds

Rounding points.  Operands are the values the device sees, already rounded to the activation dtype.  What the kernels round
before the first product: q * 1/8 -> bf16 in the tree kernel (a power of two: exact), q * rsqrt(d_k) in f32 in the per-row
kernel (exact for d_k = 64, one f32 rounding for d_k = 32, done here in float32), nothing in the source kernel (it scales
the f32 score; here the float64 score times the float32 value of rsqrt(d_k)).  Everything behind that is float64.  The
3 u A of the bf16 budget is derived for the source and tree kernels (probabilities rounded once, the denominator the sum of
the rounded values, one store rounding); the per-row kernel keeps f32 probabilities, spends only the store's u and is held
to the same budget.

Inputs.  q, k normals (q times 4 in the `sharp` regime).  v is sparse per key POSITION j: +-[0.5, 1.5] in channel j % d_k, a
normal in channel (7 j + 3) % d_k (6 j + 3 is odd: never the same channel for d_k = 64 or 32), zero elsewhere, so a channel
sums a few keys and every key shows at the level of the output.  What must not be read holds +-8 in EVERY channel of K and V
(finite: the source kernel multiplies a zero probability with it): cache positions >= pos (position pos is overwritten by
the step), cache rows no ancestor names (at every position one slot is kept free of ancestors, and the table of the other
step parity names exactly that slot), memory frames in [klens[b], T).

Measured on the CPU over every case below, both regimes (tests/test_cpu_dec_step_ref.py):
  F32_REF_MAX_DEC   the float32 torch restatement's worst error in units of 2^-24 (1 + S) A.  It stays under
                    attention_ref.F32_REF_MAX (13.47), so attention_ref.F is reused unchanged.
  SIM_ROW_BF16_MAX  a faithful per-row bf16 kernel (f32 probabilities, one store rounding): worst err / budget
  SIM_RND_BF16_MAX  a faithful rounded-probability bf16 kernel (source, tree): worst err / budget
"""
import math
from collections import namedtuple

import torch

from tests.attention_ref import REGIMES, Ref, assert_in_budget, budget, rd, worst  # noqa: F401 (re-exported to the tests)

F64 = torch.float64
POISON = 8.0

# measured maxima (see the module docstring; test_cpu_dec_step_ref.py holds the code to them)
# f32 operands: self 9.15 (sharp), token mask 6.17, source 7.50; bf16 operands: self 4.26, token mask 4.24, tree 3.36,
# source 4.77 (with torch's CPU matmul)
F32_REF_MAX_DEC = 9.15
SIM_ROW_BF16_MAX = 0.34  # per-row form: self 0.326, token mask 0.328, tree cases 0.330, source cases 0.332
SIM_RND_BF16_MAX = 0.68  # rounded probabilities: self cases 0.675, token mask 0.586, tree 0.651, source 0.672

# ------------------------------------------------------------------------------------------ case lists
# per-row self-attention: (dtype name, heads, d); a batch of the key loop is 64 positions for bf16 / d_k 64, 32 for f32 /
# d_k 64, 128 for bf16 / d_k 32, 64 for f32 / d_k 32, so the positions sit on, before and behind 8, 32, 64 and 128
SELF_N, SELF_GROUP, SELF_LMAX = 7, 3, 201
SELF_SHAPES = [(3, 192), (2, 64)]  # d_k = 64, d_k = 32
SELF_POS = [0, 1, 7, 8, 31, 32, 63, 64, 65, 127, 128, 129, 200]
SELF_SPLITS = [None, 1, 2, 4]  # ESPNET_AMD_SA_SPLIT: automatic, forced
TOK_POS = [0, 1, 8, 65, 130]   # token-mask cases
POSDEV_POS = [64, 129]         # an even and an odd device position
# beam tree (bf16, d_k = 64, two heads): W at and just above the bound of each WT instantiation (5, 10, 16), with the
# largest Lmax whose key list fits 64 KiB of LDS at that width, rounded down generously
TREE_B, TREE_HEADS, TREE_D = 2, 2, 128
TREE_W_LMAX = [(2, 512), (5, 512), (6, 512), (10, 400), (11, 400), (16, 300)]
TREE_KINDS = ["beam_tree", "random", "all_shared"]


def tree_positions(kind, W, Lmax):
    """phase 1 handles positions tid and tid + 256: 0, 255, 256, 257 and the last; with one shared path the key list is
    pos + W long: 63, 64, 65 keys, and a position whose W new keys straddle the first two 64-key tiles"""
    pos = [0, 255, 256, 257, Lmax - 1]
    if kind == "all_shared":
        pos += [63 - W, 64 - W, 65 - W, 64 - (W + 1) // 2]
    return sorted(set(pos))


TREE_POSDEV = 257  # an odd device position
# source attention: T crosses a 16-key tile, a 32-key fragment and the 128- (f32) / 256-key (bf16) batches of both loops
SRC_T = [1, 15, 16, 17, 31, 32, 33, 75, 129, 255, 256, 257, 300]
SRC_W = [1, 5, 16, 17, 20, 33]
SRC_SHAPES = [(3, 192), (2, 64)]
SRC_EXTRA_PAD_T = 75  # this T runs once more with Tpad 32 larger than needed


def src_klens(T):
    """the full length, T - 1, a tile edge, 1 and one klens[b] > T (the kernel clamps it)"""
    edge = max(1, (T - 1) // 16 * 16)
    return [T, max(1, T - 1), edge, 1, T + 3]


def src_cases():
    """(T, W, Tpad): every T with a W of the list in turn (every W at least twice), every W at T = 75, one padded case"""
    out = [(T, SRC_W[i % len(SRC_W)], (T + 31) // 32 * 32) for i, T in enumerate(SRC_T)]
    out += [(75, W, 96) for W in SRC_W if (75, W, 96) not in out]
    out.append((SRC_EXTRA_PAD_T, 20, 128))
    return out


LNQ_CASES = [(1, 17), (33, 17), (257, 17), (75, 5), (16, 33)]  # (T, W), d in {256, 512}


# ------------------------------------------------------------------------------------------ the attention itself
def attend(q, k, v, vis, post_scale=1.0):
    """q [R][h][c], k / v [R][L][h][c] (the keys of every row, gathered), vis [R][L] -> Ref(ctx, A, S), each [1][R][h * c]
    float64.  A row without a visible key gives zeros (A == 0 everywhere)."""
    assert q.dtype == F64 and k.dtype == F64 and v.dtype == F64
    R, L, h, c = k.shape
    sc = torch.einsum("rhc,rlhc->rhl", q, k) * post_scale
    hidden = ~vis[:, None, :]
    P = torch.softmax(sc.masked_fill(hidden, float("-inf")), -1)
    P = torch.where(vis.any(-1)[:, None, None], P, torch.zeros_like(P))
    ctx = torch.einsum("rhl,rlhc->rhc", P, v).reshape(1, R, h * c)
    A = torch.einsum("rhl,rlhc->rhc", P, v.abs()).reshape(1, R, h * c)
    S = sc.abs().masked_fill(hidden, 0.0).amax(-1).repeat_interleave(c, dim=-1).reshape(1, R, h * c)
    return Ref(ctx, A, S, P)


def sparse_v(shape_front, L_axis, dk, g):
    """v [..][dk] with the position index on axis `L_axis` of shape_front"""
    mag = (0.5 + torch.rand(*shape_front, generator=g)) * (torch.randint(0, 2, shape_front, generator=g).float() * 2 - 1)
    second = torch.randn(*shape_front, generator=g)
    view = [1] * (len(shape_front) + 1)
    view[L_axis] = shape_front[L_axis]
    j = torch.arange(shape_front[L_axis]).reshape(view).expand(*shape_front, 1)
    v = torch.zeros(*shape_front, dk)
    v.scatter_(-1, j % dk, mag.unsqueeze(-1))
    v.scatter_(-1, (7 * j + 3) % dk, second.unsqueeze(-1))
    return v


def poison(shape, g):
    return (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * POISON


# ------------------------------------------------------------------------------------------ self-attention
SelfCase = namedtuple("SelfCase", "n W h dk d Lmax dtype regime qkv kc vc anc other tok")
_SELF = {}


def self_case(n, W, h, d, Lmax, regime, dtype, kind="random", tok=False):
    """One set of inputs per shape, shared and left unchanged.  Rows are n / W beams of W consecutive rows; a row's
    ancestors are slots of its own beam.  At every position one slot per beam (`other`) is named by no row of the beam:
    it holds +-8, and `other` is the ancestor table of the wrong step parity.  kc / vc are [Lmax][n][d] with every position
    filled (at_position() poisons positions >= pos); qkv [n][3 d]; tok [Lmax][n] token ids or None.
    kind: `random` independent slots, `all_shared` one path per beam, `beam_tree` a beam walked forward (rows continue a
    parent row and coalesce).  With tok the last row keeps a slot of its own that holds id 0 at every position (a row
    whose keys are all masked), ids 0 are scattered over the other slots, and row 2's current token is id 0."""
    key = (n, W, h, d, Lmax, regime, dtype, kind, tok)
    if key in _SELF:
        return _SELF[key]
    assert regime in REGIMES and n % W == 0 and W >= 2
    dk, B = d // h, n // W
    seed = 7 * n + 13 * W + 1000 * d + 31 * Lmax + REGIMES.index(regime) + 100003 * TREE_KINDS.index(kind) + (5 if tok else 0)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3, h, dk, generator=g)
    qkv[:, 0] *= 4.0 if regime == "sharp" else 1.0
    kc = torch.randn(Lmax, n, h, dk, generator=g)
    vc = sparse_v((Lmax, n, h), 0, dk, g)
    # the free slot of every (beam, position), never the beam's last slot (the all-masked row's own one in the tok cases)
    pool = W - 1 if tok else W
    free = torch.randint(0, pool, (B, Lmax), generator=g)

    def dodge(slot, fr):  # slots in [0, pool - 1) -> [0, pool) without `fr`
        return slot + (slot >= fr).long()

    if kind == "random":
        anc = dodge(torch.randint(0, pool - 1, (B, W, Lmax), generator=g), free[:, None, :])
    elif kind == "all_shared":
        anc = dodge(torch.randint(0, pool - 1, (B, 1, Lmax), generator=g), free[:, None, :]).expand(B, W, Lmax).clone()
    else:
        assert kind == "beam_tree" and not tok
        anc = torch.zeros(B, W, Lmax, dtype=torch.long)
        for j in range(Lmax):
            parent = torch.minimum(torch.randint(0, W, (B, W), generator=g), torch.randint(0, W, (B, W), generator=g))
            anc = torch.gather(anc, 1, parent[:, :, None].expand(B, W, Lmax)).clone()
            own = torch.arange(W)[None, :].expand(B, W)
            fr = free[:, j, None]
            anc[:, :, j] = torch.where(own == fr, (own + 1) % W, own)  # (the row that would write the free slot shares its neighbour's)
    ids = None
    if tok:
        anc[:, W - 1, :] = W - 1
        ids = torch.randint(1, 50, (Lmax, n), generator=g)
        ids[torch.rand(Lmax, n, generator=g) < 0.25] = 0
        ids.view(Lmax, B, W)[:, :, W - 1] = 0
        ids[:, 2] = 0  # (row 2's own token at whichever position is the current one; as a cache slot it is masked as well)
    base = (torch.arange(B) * W)[:, None, None]
    other = (free[:, None, :].expand(B, W, Lmax) + base).reshape(n, Lmax).to(torch.int32)
    anc = (anc + base).reshape(n, Lmax).to(torch.int32)
    # poison every slot no row names
    named = torch.zeros(Lmax, n, dtype=torch.bool)
    named[torch.arange(Lmax)[None, :].expand(n, Lmax), anc.long()] = True
    kc = torch.where(named[:, :, None, None], kc, poison((Lmax, n, h, dk), g))
    vc = torch.where(named[:, :, None, None], vc, poison((Lmax, n, h, dk), g))
    case = SelfCase(n, W, h, dk, d, Lmax, dtype, regime, rd(qkv.reshape(n, 3 * d), dtype), rd(kc.reshape(Lmax, n, d), dtype),
                    rd(vc.reshape(Lmax, n, d), dtype), anc, other, None if ids is None else ids.to(torch.int32))
    _SELF[key] = case
    return case


def at_position(case, pos):
    """(qkv, kc, vc) of the step at `pos`: the new token's v is sparse for position pos, the caches hold +-8 from pos on."""
    g = torch.Generator().manual_seed(977 * pos + case.n + case.d)
    n, h, dk, d = case.n, case.h, case.dk, case.d
    qkv = case.qkv.clone()
    mag = (0.5 + torch.rand(n, h, generator=g)) * (torch.randint(0, 2, (n, h), generator=g).float() * 2 - 1)
    v = torch.zeros(n, h, dk)
    v[:, :, pos % dk] = mag
    v[:, :, (7 * pos + 3) % dk] = torch.randn(n, h, generator=g)
    qkv[:, 2 * d:] = rd(v.reshape(n, d), case.dtype)
    kc, vc = case.kc.clone(), case.vc.clone()
    kc[pos:] = poison((case.Lmax - pos, n, d), g)
    vc[pos:] = poison((case.Lmax - pos, n, d), g)
    return qkv, kc, vc


def self_query(case, qkv, kernel):
    """the query as the kernel's first product sees it, float64 [n][h][dk]"""
    q = qkv[:, :case.d]
    if kernel == "tree":
        q = rd(q * 0.125, torch.bfloat16)  # (d_k = 64, bf16: exact)
    else:
        q = q * torch.tensor(1.0 / math.sqrt(case.dk), dtype=torch.float32)  # f32 product, as q[e] *= scale
    return q.reshape(case.n, case.h, case.dk).to(F64)


def self_operands(case, pos, step, anc=None, kernel="row"):
    """(q [n][h][dk], k, v [n][pos + 1][h][dk], vis [n][pos + 1]) in float64 for the step `step` = at_position(case, pos);
    `anc` defaults to the case's table."""
    qkv, kc, vc = step
    n, h, dk, d = case.n, case.h, case.dk, case.d
    anc = (case.anc if anc is None else anc).long()
    jj = torch.arange(pos)[None, :].expand(n, pos)
    sl = anc[:, :pos]
    k = torch.cat([kc[jj, sl], qkv[:, None, d:2 * d]], 1).reshape(n, pos + 1, h, dk).to(F64)
    v = torch.cat([vc[jj, sl], qkv[:, None, 2 * d:]], 1).reshape(n, pos + 1, h, dk).to(F64)
    vis = torch.ones(n, pos + 1, dtype=torch.bool)
    if case.tok is not None:
        vis = torch.cat([case.tok[jj, sl], case.tok[pos][:, None]], 1) != 0
    return self_query(case, qkv, kernel), k, v, vis


def ref_self(case, pos, step, kernel="row"):
    return attend(*self_operands(case, pos, step, kernel=kernel))


# ------------------------------------------------------------------------------------------ source attention
SrcCase = namedtuple("SrcCase", "B W T klens h dk d dtype regime qs kv")
_SRC = {}


def src_case(T, W, h, d, regime, dtype):
    """qs [B W][d], kv [B T][2 d] (K | V rows of the memory, frames >= klens[b] hold +-8), klens = src_klens(T)"""
    key = (T, W, h, d, regime, dtype)
    if key in _SRC:
        return _SRC[key]
    klens = src_klens(T)
    B, dk = len(klens), d // h
    g = torch.Generator().manual_seed(1000 * T + 10 * W + d + REGIMES.index(regime))
    qs = torch.randn(B * W, d, generator=g) * (4.0 if regime == "sharp" else 1.0)
    k = torch.randn(B, T, h, dk, generator=g)
    v = sparse_v((B, T, h), 1, dk, g)
    dead = (torch.arange(T)[None, :] >= torch.tensor(klens)[:, None])[:, :, None, None]
    k = torch.where(dead, poison((B, T, h, dk), g), k)
    v = torch.where(dead, poison((B, T, h, dk), g), v)
    kv = torch.cat([k.reshape(B * T, d), v.reshape(B * T, d)], 1)
    _SRC[key] = SrcCase(B, W, T, klens, h, dk, d, dtype, regime, rd(qs, dtype), rd(kv, dtype))
    return _SRC[key]


def src_operands(case, qs=None, klens=None):
    """(q [B W][h][dk], k, v [B W][T][h][dk], vis [B W][T], post_scale): every row with the memory of its utterance"""
    B, W, T, h, dk, d = case.B, case.W, case.T, case.h, case.dk, case.d
    qs = case.qs if qs is None else qs
    kl = torch.tensor(case.klens if klens is None else klens).clamp(max=T)
    mem = case.kv.reshape(B, T, 2, h, dk).to(F64)
    rows = torch.arange(B).repeat_interleave(W)
    vis = (torch.arange(T)[None, :] < kl[:, None])[rows]
    scale = float(torch.tensor(1.0 / math.sqrt(dk), dtype=torch.float32))
    return qs.reshape(B * W, h, dk).to(F64), mem[rows, :, 0], mem[rows, :, 1], vis, scale


def ref_src(case, qs=None):
    return attend(*src_operands(case, qs))


def want_vt(case, Tpad):
    """em_dec_transpose_v: vT[b][c][t] = kv[b T + t][d + c], zero for t in [T, Tpad)"""
    vt = torch.zeros(case.B, case.d, Tpad)
    vt[:, :, :case.T] = case.kv.reshape(case.B, case.T, 2 * case.d)[:, :, case.d:].transpose(1, 2)
    return vt


# ------------------------------------------------------------------------------------------ embeddings, LM input norm
F32_U = 2.0 ** -24


def clamp_ids(tok, V):
    return tok.long().clamp(0, V - 1)


def ref_dec_embed(embed, pe, tok, pos):
    """x = embed[tok] * sqrt(d) + pe[pos] (embedding.py:93) in float64, and the f32 bound: the kernel rounds sqrt(d), the
    product and the sum once each (two roundings where the compiler contracts to an fma): 2^-24 (2 |e| sqrt(d) + |x|)."""
    d = embed.shape[1]
    e = embed.to(F64)[clamp_ids(tok, embed.shape[0])] * math.sqrt(d)
    x = e + pe.to(F64)[pos]
    return x, F32_U * (2 * e.abs() + x.abs()) * (1 + 2 ** -20)


def ref_lm_input_norm(x, g, b, pe, pos):
    """LayerNorm(eps 1e-5) -> ReLU -> optional x * sqrt(d) + pe[pos] (encoder.py:132-139) in float64, and the f32 bound.
    The kernel sums d values as d / 64 per lane and six exchange levels (depth s = d / 64 + 6) for the mean and again for
    the variance, and spends eight more roundings (the two divisions by d, x - mean, + eps, sqrt, the reciprocal, the two
    multiplications and the bias sum, one of them shared).  Every one is relative 2^-24 to a term no larger than
    |g| rstd (|x - mean| + mean |x|) + |b|  (the mean's error enters x - mean absolutely, hence mean |x|), so the bound is
    (s + 8) 2^-24 of that, times sqrt(d) when the positional encoding follows, plus two roundings of the result."""
    d = x.shape[1]
    x, g, b = x.to(F64), g.to(F64), b.to(F64)
    mean = x.mean(-1, keepdim=True)
    t = x - mean
    rstd = 1.0 / torch.sqrt((t * t).mean(-1, keepdim=True) + 1e-5)
    y = torch.relu(t * rstd * g + b)
    bound = (d / 64 + 6 + 8) * F32_U * (g.abs() * rstd * (t.abs() + x.abs().mean(-1, keepdim=True)) + b.abs())
    if pe is not None:
        y = y * math.sqrt(d) + pe.to(F64)[pos]
        bound = bound * math.sqrt(d)
    return y, bound + 2 * F32_U * y.abs()
