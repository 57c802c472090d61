"""Float64 restatement of encoder self-attention, the inputs and the per-element error budget that the CPU and the GPU
parity tests share (tests/test_cpu_attention_ref.py, tests/test_gpu_attention_parity.py, tests/test_gpu_block.py).

  attention_cases   seeded q / k / position table / biases and a SPARSE v, for one (T, klens, h, regime)
  ref_rel           RelPositionMultiHeadedAttention (attention.py:416-459): AC + BD, BD[i][j] = (q_i + v) . p[T-1-i+j]
  ref_legacy        LegacyRelPositionMultiHeadedAttention (attention.py:268-360): the square pad-and-reshape, literally
  ref_abs           MultiHeadedAttention: q . k / 8
  budget            the one tolerance: 3 u A + f (1 + S) A for bf16, f (1 + S) A for f32
  worst / assert_in_budget   err / budget per element, the worst element named

Rounding points.  Operands are the values the device sees (already rounded to the activation dtype).  The roundings the
kernels do BEFORE the first matrix product are done here in float32 exactly as the per-kernel tests do them and then
widened: q(qq + u), q(qq + v) (csrc/attention.hip), q((qq + u) * 0.125) (csrc/attention2.hip, the attention phase of
csrc/block.hip), q * 0.125 (csrc/abs_attn.hip; a power of two, exact).  A float64 sum rounded once can differ from the
float32 sum the kernels round by a bf16 ulp, which would eat the budget.  Everything behind these points is float64:
scores, mask, softmax, P . V.

Besides ctx the reference returns, per element (row i, channel c),
    A[i][c] = sum_j P[i][j] |v[j][c]|        S[i] = max_{j < klen} |score[i][j]|
and the budget is stated in them:

  bf16   |got - ref| <= 3 u A + f (1 + S) A,  u = 2^-8.  Derived, not measured: every probability is rounded once (at
         most u A in the numerator), the denominator is the sum of the rounded probabilities (at most u relative, i.e.
         u |ctx| <= u A), the store rounds once (u |ctx|).  A CPU simulation of exactly these roundings (64-key online
         tiles, float32 elsewhere: tests/test_cpu_attention_ref.py::test_bf16_simulation_inside_budget) reaches
         SIM_BF16_MAX of the budget over the case list.
  f32    |got - ref| <= f (1 + S) A,  f = 4 * F32_REF_MAX * 2^-24.  F32_REF_MAX is the worst error of the float32 torch
         restatement of the same formula over the case list, in units of 2^-24 (1 + S) A.  It was meant to stay under 10
         (then f = 40 * 2^-24) and does (9.87 at most) except in the sharp (130, [130, 129, 128, 2]) cases, in their
         utterance of two keys: 13.47 with one head, 12.00 with three.  There S, the larger of two scores (it can be
         under 1), says little about the 128 products of magnitude ~4 that each score sums.  So f is four times the
         measured maximum; the factor is for the kernels' online softmax, which rescales per tile, and the hardware exp.
  A == 0 the output is exactly zero.  With the sparse v this holds wherever no valid key maps to the channel, so any leak
         from a masked key or a padding frame shows.
"""
from collections import namedtuple

import torch

DK = 64
LB = 3  # the position table holds linear_pos of LB blocks side by side (ldp = LB * d); the middle one is used

U_BF16 = 2.0 ** -8       # unit roundoff of bf16
F32_UNIT = 2.0 ** -24
# The float32 torch restatement's worst error in units of 2^-24 (1 + S) A, measured over every case below in both regimes
# (tests/test_cpu_attention_ref.py::test_float32_restatement_is_where_f_comes_from): float32 operands 13.47 (rel and
# legacy), 12.13 (abs), all three in the two-key utterance of T = 130; 9.87 on every other case; bf16 operands 4.93
# (rel, legacy), 4.03 (abs).
F32_REF_MAX = 13.47
F = 4 * F32_REF_MAX * F32_UNIT
# The simulated faithful bf16 kernel's worst err / budget (test_bf16_simulation_inside_budget), i.e. 2.1 u A of the
# 3 u A: 0.66 (rel), 0.69 (legacy), 0.68 (rel, 1 / 8 in the operand), 0.67 (abs).
SIM_BF16_MAX = 0.69

# (T, klens): the smallest shapes that touch each tile edge
COMMON_CASES = [(1, [1]), (17, [17, 16, 1]), (65, [65, 64, 63, 33]), (130, [130, 129, 128, 2]), (300, [300, 257, 256, 255])]
CLAMP_CASE = (65, [72, 64])                  # klens[b] > T: the stand-alone launchers clamp it
SUPER_TILE_CASE = (520, [520, 513, 512, 511])  # crosses the second 256-key super-tile boundary (Tpad = 768)
GROUPED_CASE = (40, [40, 39, 38, 37, 3, 2, 1, 40, 17])  # nine utterances: another workgroup -> utterance map in block<ATT|C>
REGIMES = ("flat", "sharp")
# (T, klens, h) per route: h = 3 (d = 192), one case again with a single head; block<ATT|C> is fixed at four heads
STANDALONE_CASES = [(T, kl, 3) for T, kl in COMMON_CASES] + [(*CLAMP_CASE, 3), (*COMMON_CASES[3], 1)]
SUPER_TILE_CASES = STANDALONE_CASES + [(*SUPER_TILE_CASE, 3)]
FUSED_CASES = [(T, kl, 4) for T, kl in COMMON_CASES + [SUPER_TILE_CASE, GROUPED_CASE]]

Case = namedtuple("Case", "T klens h dtype q k v pall u vb")
Ref = namedtuple("Ref", "ctx A S P")


def rd(t, dtype):
    """Round to the activation dtype and come back to float32 (what the kernel sees)."""
    return t.to(dtype).to(torch.float32)


def attention_cases(T, klens, h, regime, seed, dtype=torch.bfloat16):
    """q, k, v [B][T][h][64], the position table pall [2T-1][LB * h * 64] (the legacy scheme uses its first T rows), the
    biases u, vb [h][64] (float32, scaled by 0.3 as in the per-kernel tests).  q, k and the table are normals rounded to
    `dtype`; q has scale 1 (`flat`: |score| <~ 8) or 4 (`sharp`: |score| reaches ~30, so the running maximum of the online
    softmax takes large steps).  v is sparse: v[j] holds +-[0.5, 1.5] in channel j % 64 and a normal in channel
    (7 j + 3) % 64 (never the same channel: 6 j + 3 is odd), so a channel sums a few keys and every key shows at the level
    of the output, not at 1 / T of it."""
    assert regime in REGIMES, regime
    g = torch.Generator().manual_seed(seed)
    B = len(klens)
    q = rd(torch.randn(B, T, h, DK, generator=g) * (4.0 if regime == "sharp" else 1.0), dtype)
    k = rd(torch.randn(B, T, h, DK, generator=g), dtype)
    pall = rd(torch.randn(2 * T - 1, LB * h * DK, generator=g), dtype)
    u = torch.randn(h, DK, generator=g) * 0.3
    vb = torch.randn(h, DK, generator=g) * 0.3
    mag = 0.5 + torch.rand(B, T, h, generator=g)
    sign = torch.randint(0, 2, (B, T, h), generator=g).float() * 2 - 1
    second = torch.randn(B, T, h, generator=g)
    j = torch.arange(T)
    v = torch.zeros(B, T, h, DK)
    v.scatter_(-1, (j % DK).reshape(1, T, 1, 1).expand(B, T, h, 1), (mag * sign).unsqueeze(-1))
    v.scatter_(-1, ((7 * j + 3) % DK).reshape(1, T, 1, 1).expand(B, T, h, 1), second.unsqueeze(-1))
    return Case(T, list(klens), h, dtype, q, k, rd(v, dtype), pall, u, vb)


_CASES = {}
SHARP_SCORE = 20.0  # a sharp case with more than 64 keys has |score| >= 20 under every score definition


def case_for(T, klens, h, regime, dtype=torch.bfloat16):
    """The one set of inputs of a (T, klens, h, regime, dtype), shared (and left unchanged) by every test that uses it.
    The seed follows from the shape.  q . k / 8 alone has 1 / sqrt(2) of the spread of AC + BD and with the first seed
    stops just short of 20 on some shapes (18.5 .. 19.9), so a sharp case takes the first seed of its sequence whose
    absolute-position scores reach SHARP_SCORE; AC + BD then reaches 25 and more."""
    key = (T, tuple(klens), h, regime, dtype)
    if key not in _CASES:
        seed = 1000 * T + 10 * h + REGIMES.index(regime)
        case = attention_cases(T, klens, h, regime, seed, dtype)
        if regime == "sharp" and T > 64:
            for attempt in range(1, 200):
                if float(finish(abs_scores(case), case.v, key_counts(case)).S.max()) >= SHARP_SCORE:
                    break
                case = attention_cases(T, klens, h, regime, seed + 100000 * attempt, dtype)
            else:
                raise AssertionError(f"no sharp inputs for T={T} h={h}")
        _CASES[key] = case
    return _CASES[key]


def key_counts(case):
    """klens as the kernels use them: clamped to T."""
    return torch.tensor([min(n, case.T) for n in case.klens])


# ------------------------------------------------------------------------------------------ operands and scores
def heads(t):
    """[B][T][h][64] float32 -> [B][h][T][64] float64"""
    return t.transpose(1, 2).to(torch.float64)


def biased_queries(case, pre):
    """(q + u, q + v) with the kernel's rounding point, and the factor still to be applied to the scores.
    pre = "sum": q(qq + u), scores / 8 afterwards;  pre = "scaled": q((qq + u) * 0.125), 1 / 8 rides in the operand."""
    if pre == "sum":
        return heads(rd(case.q + case.u, case.dtype)), heads(rd(case.q + case.vb, case.dtype)), 0.125
    assert pre == "scaled", pre
    return heads(rd((case.q + case.u) * 0.125, case.dtype)), heads(rd((case.q + case.vb) * 0.125, case.dtype)), 1.0


def position_rows(case, rows):
    """the middle block of the table, [h][rows][64] float64"""
    d = case.h * DK
    return case.pall[:rows, d:2 * d].reshape(rows, case.h, DK).transpose(0, 1).to(torch.float64)


def rel_bd(q_v, p):
    """BD[i][j] = q_v[i] . p[T-1-i+j]  (q_v [B][h][T][c], p [h][2T-1][c])"""
    T = q_v.shape[2]
    full = q_v @ p.transpose(-2, -1)  # [B][h][T][2T-1]
    idx = T - 1 - torch.arange(T).reshape(T, 1) + torch.arange(T).reshape(1, T)
    return full.gather(-1, idx.expand(*full.shape[:2], T, T))


def legacy_shift(x):
    """attention.py:296-316 with zero_triu = False, literally: a zero column in front, the (T, T+1) matrix re-read as
    (T+1, T), its first row dropped.  Gives x[i][T-1-i+j] for j <= i, 0 at j == i+1 and row i+1's entries behind it."""
    B, h, T, _ = x.shape
    padded = torch.cat([x.new_zeros(B, h, T, 1), x], dim=-1)
    return padded.reshape(B, h, T + 1, T)[:, :, 1:, :]


def legacy_bd(q_v, p):
    """q_v [B][h][T][c], p [h][T][c]"""
    return legacy_shift(q_v @ p.transpose(-2, -1))


def rel_scores(case, pre):
    q_u, q_v, scale = biased_queries(case, pre)
    return (q_u @ heads(case.k).transpose(-2, -1) + rel_bd(q_v, position_rows(case, 2 * case.T - 1))) * scale


def legacy_scores(case):
    q_u, q_v, scale = biased_queries(case, "sum")
    return (q_u @ heads(case.k).transpose(-2, -1) + legacy_bd(q_v, position_rows(case, case.T))) * scale


def abs_scores(case):
    return heads(rd(case.q * 0.125, case.dtype)) @ heads(case.k).transpose(-2, -1)


# ------------------------------------------------------------------------------------------ softmax, P . V, A, S
def rows(t):
    """[B][h][T][64] -> [B][T][h * 64]"""
    B, h, T, c = t.shape
    return t.transpose(1, 2).reshape(B, T, h * c)


def finish(scores, v, kl, keep_p=False):
    """scores [B][h][T][T] float64, v [B][T][h][64], kl [B] key counts -> Ref(ctx, A, S [, P]); ctx, A, S are [B][T][h * 64]
    (S repeated over a head's channels).  Rows past the key count attend over the valid keys like any other row."""
    assert scores.dtype == torch.float64
    T = scores.shape[-1]
    masked = (torch.arange(T)[None, :] >= kl[:, None])[:, None, None, :]
    P = torch.softmax(scores.masked_fill(masked, float("-inf")), dim=-1)
    vh = heads(v)
    S = scores.abs().masked_fill(masked, 0.0).amax(-1)  # [B][h][T]
    S = S.transpose(1, 2).repeat_interleave(DK, dim=-1)
    return Ref(rows(P @ vh), rows(P @ vh.abs()), S, P if keep_p else None)


def ref_rel(case, pre="sum", keep_p=False):
    return finish(rel_scores(case, pre), case.v, key_counts(case), keep_p)


def ref_legacy(case, keep_p=False):
    return finish(legacy_scores(case), case.v, key_counts(case), keep_p)


def ref_abs(case, keep_p=False):
    return finish(abs_scores(case), case.v, key_counts(case), keep_p)


# ------------------------------------------------------------------------------------------ the budget
def budget(ref, dtype):
    f32_term = F * (1.0 + ref.S) * ref.A
    return f32_term if dtype == torch.float32 else 3.0 * U_BF16 * ref.A + f32_term


def worst(got, ref, dtype):
    """(err / budget of the worst element, its index into [B][T][h * 64]); an element with A == 0 must be exactly zero (its
    ratio is inf otherwise), a NaN counts as inf."""
    got = got.detach().cpu().to(torch.float64).reshape(ref.ctx.shape)
    err = (got - ref.ctx).abs()
    bud = budget(ref, dtype)
    ratio = torch.where(bud > 0, err / bud.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    flat = int(ratio.argmax())
    return float(ratio.reshape(-1)[flat]), tuple(int(x) for x in torch.unravel_index(torch.tensor(flat), ratio.shape))


def assert_in_budget(got, ref, dtype, what, dk=DK):
    """Holds every element of got [B][T][h * dk] to the budget; returns the worst err / budget."""
    r, (b, i, c) = worst(got, ref, dtype)
    g = float(got.detach().cpu().to(torch.float64).reshape(ref.ctx.shape)[b, i, c])
    assert r <= 1.0, (f"{what}: err / budget = {r:.3g} at utterance {b}, head {c // dk}, row {i}, channel {c % dk}: got {g!r}, "
                      f"reference {float(ref.ctx[b, i, c])!r}, A {float(ref.A[b, i, c]):.3e}, S {float(ref.S[b, i, c]):.3g}")
    return r
