"""The float64 attention reference, its inputs and its budget (tests/attention_ref.py), checked without a GPU: the reference
against the oracle's literal rel_shift / legacy_rel_shift formulation in float64, where the float32 constant of the budget
comes from, that the inputs make every key and the online-softmax rescale visible, and that the budget is sharp enough: six
wrong variants of the reference each break it by ten times.  The variants live here only; nothing mutates a kernel."""
import math

import pytest
import torch

from oracle import conformer as oc
from tests import attention_ref as ar

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DK = ar.DK

# (score definition, rounding point, cases): what the GPU tests run
KINDS = {
    "rel": ("sum", ar.STANDALONE_CASES),                            # csrc/attention.hip
    "legacy": ("sum", ar.STANDALONE_CASES),                         # csrc/attention.hip, LEGACY
    "rel_scaled": ("scaled", ar.SUPER_TILE_CASES + ar.FUSED_CASES),  # csrc/attention2.hip, block<ATT|C>
    "abs": (None, ar.SUPER_TILE_CASES),                             # csrc/abs_attn.hip
}
PARAMS = [pytest.param(kind, T, kl, h, regime, id=f"{kind}-T{T}x{len(kl)}-h{h}-{regime}")
          for kind, (_, cases) in KINDS.items() for T, kl, h in cases for regime in ar.REGIMES]
F32_PARAMS = [p for p in PARAMS if p.values[0] != "rel_scaled"]  # the routes that have a float32 form

_REFS = {}


def compute(kind, case, keep_p=False):
    if kind == "legacy":
        return ar.ref_legacy(case, keep_p)
    return ar.ref_abs(case, keep_p) if kind == "abs" else ar.ref_rel(case, KINDS[kind][0], keep_p)


def reference(kind, case):
    """the float64 reference of the bf16 inputs with its probabilities, once per (kind, case)"""
    key = (kind, id(case))
    if key not in _REFS:
        _REFS[key] = compute(kind, case, True)
    return _REFS[key]


def restated(kind, case, dt):
    """The oracle's formulation on the same operands in `dt`, as the per-kernel GPU tests state it: scores [B][h][T][T]."""
    qq, kk = case.q, case.k.transpose(1, 2).to(dt)
    if kind == "abs":
        return ar.rd(qq * 0.125, case.dtype).transpose(1, 2).to(dt) @ kk.transpose(-2, -1)
    rows = case.T if kind == "legacy" else 2 * case.T - 1
    d = case.h * DK
    pp = case.pall[:rows, d:2 * d].reshape(1, rows, case.h, DK).transpose(1, 2).to(dt)
    if kind == "rel_scaled":
        q_u = ar.rd((qq + case.u) * 0.125, case.dtype).transpose(1, 2).to(dt)
        q_v = ar.rd((qq + case.vb) * 0.125, case.dtype).transpose(1, 2).to(dt)
        return q_u @ kk.transpose(-2, -1) + oc.rel_shift(q_v @ pp.transpose(-2, -1))
    q_u = ar.rd(qq + case.u, case.dtype).transpose(1, 2).to(dt)
    q_v = ar.rd(qq + case.vb, case.dtype).transpose(1, 2).to(dt)
    shift = oc.legacy_rel_shift if kind == "legacy" else oc.rel_shift
    return (q_u @ kk.transpose(-2, -1) + shift(q_v @ pp.transpose(-2, -1))) / math.sqrt(DK)


def restated_ctx(kind, case, dt):
    """forward_attention (attention.py:121-151) on the restated scores"""
    scores = restated(kind, case, dt)
    mask = oc.make_pad_mask(ar.key_counts(case), case.T)[:, None, None, :]
    attn = torch.softmax(scores.masked_fill(mask, torch.finfo(dt).min), -1).masked_fill(mask, 0.0)
    return (attn @ case.v.transpose(1, 2).to(dt)).transpose(1, 2).reshape(len(case.klens), case.T, case.h * DK)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind,T,klens,h,regime", PARAMS)
def test_reference_equals_oracle_formulation_in_float64(kind, T, klens, h, regime, dtype):
    case = ar.case_for(T, klens, h, regime, dtype)
    ref = reference(kind, case) if dtype == BF else compute(kind, case)
    want = restated_ctx(kind, case, F64)
    assert ref.ctx.dtype == F64 and ref.ctx.shape == want.shape
    err = (ref.ctx - want).abs()
    allow = 16 * 2.0 ** -53 * (1 + ref.S) * ref.A  # a few float64 ulps of what the element sums
    assert bool((err <= allow).all()), float((err / allow.clamp_min(1e-300)).max())
    assert bool((ref.ctx[ref.A == 0] == 0).all())


def test_legacy_shift_is_what_the_kernel_comment_says():
    """csrc/attention.hip states the square shift as an index formula; the reference implements the shift literally and
    must agree with it: x[i][T-1-i+j] for j <= i, 0 at j == i+1, x[i+1][j-i-2] behind."""
    T = 7
    x = torch.arange(T * T, dtype=F64).reshape(1, 1, T, T) + 1
    y = ar.legacy_shift(x)
    for i in range(T):
        for j in range(T):
            want = x[0, 0, i, T - 1 - i + j] if j <= i else 0.0 if j == i + 1 else x[0, 0, i + 1, j - i - 2]
            assert y[0, 0, i, j] == want, (i, j)
    assert torch.equal(y, oc.legacy_rel_shift(x))


def test_inputs_are_as_stated():
    case = ar.case_for(130, [130, 129, 128, 2], 3, "sharp")
    for t in (case.q, case.k, case.v, case.pall):
        assert torch.equal(t, ar.rd(t, BF))
    nz = case.v != 0
    assert bool((nz.sum(-1) == 2).all())
    j = torch.arange(130)
    main = case.v.gather(-1, (j % 64).reshape(1, -1, 1, 1).expand(4, 130, 3, 1)).abs()
    assert 0.5 <= float(main.min()) and float(main.max()) <= 1.5
    assert bool(nz.gather(-1, ((7 * j + 3) % 64).reshape(1, -1, 1, 1).expand(4, 130, 3, 1)).all())
    flat = ar.case_for(130, [130, 129, 128, 2], 3, "flat")
    assert 3.5 < float(case.q.std() / flat.q.std()) < 4.5
    assert ar.case_for(130, [130, 129, 128, 2], 3, "sharp") is case  # one set of inputs per case, shared


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind,T,klens,h,regime", F32_PARAMS)
def test_float32_restatement_is_where_f_comes_from(kind, T, klens, h, regime, dtype):
    """f is four times the worst error of the float32 torch restatement of the formula, in units of 2^-24 (1 + S) A
    (attention_ref.F32_REF_MAX, 13.47 as measured with torch's CPU matmul).  The figure moves a little with the summation
    order of the CPU's matrix product, so the restatement is held to twice the recorded maximum, half of f."""
    case = ar.case_for(T, klens, h, regime, dtype)
    ref = reference(kind, case) if dtype == BF else compute(kind, case)
    got = restated_ctx(kind, case, F32).to(F64)
    unit = ar.F32_UNIT * (1 + ref.S) * ref.A
    err = (got - ref.ctx).abs()
    assert bool((err[unit == 0] == 0).all())
    worst = float((err / unit.clamp_min(1e-300)).max())
    print(f"f32 restatement {kind} T={T} h={h} {regime} {dtype}: {worst:.2f} x 2^-24 (1 + S) A")
    assert ar.F == 4 * ar.F32_REF_MAX * ar.F32_UNIT
    assert worst <= 2 * ar.F32_REF_MAX


def simulate_bf16_kernel(kind, case):
    """A faithful bf16 kernel on the CPU: float32 scores, 64-key tiles with the online softmax, every probability rounded to
    bf16 before P . V and before the denominator sums it, float32 accumulation, one rounding at the store."""
    scores = restated(kind, case, F32)
    kl = ar.key_counts(case)
    B, h, T, _ = scores.shape
    masked = (torch.arange(T)[None, :] >= kl[:, None])[:, None, None, :]
    scores = scores.masked_fill(masked, float("-inf"))
    vh = case.v.transpose(1, 2)
    m = torch.full((B, h, T, 1), float("-inf"))
    l = torch.zeros(B, h, T, 1)
    acc = torch.zeros(B, h, T, DK)
    for j0 in range(0, T, 64):
        s = scores[..., j0:j0 + 64]
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        live = torch.isfinite(mn)  # (an utterance's tiles past its end: nothing to add)
        alpha = torch.where(torch.isfinite(m), torch.exp(m - mn), torch.zeros_like(m))
        p = torch.where(live, torch.exp(s - torch.where(live, mn, torch.zeros_like(mn))), torch.zeros_like(s))
        p = ar.rd(p, BF)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + p @ vh[:, :, j0:j0 + 64]
        m = mn
    return ar.rd(acc / l, BF).transpose(1, 2).reshape(B, T, h * DK)


@pytest.mark.parametrize("kind,T,klens,h,regime", PARAMS)
def test_bf16_simulation_inside_budget(kind, T, klens, h, regime):
    """The budget is reachable: the simulated faithful kernel stays inside it (worst value: attention_ref.SIM_BF16_MAX)."""
    case = ar.case_for(T, klens, h, regime)
    r, where = ar.worst(simulate_bf16_kernel(kind, case), reference(kind, case), BF)
    print(f"bf16 simulation {kind} T={T} h={h} {regime}: err / budget {r:.3f} at {where}")
    assert r <= 1.0


@pytest.mark.parametrize("kind,T,klens,h,regime", PARAMS)
def test_every_key_counts(kind, T, klens, h, regime):
    """For every valid key j there is a row and a head where its own term P[i][j] |v[j][j % 64]| is ten times the budget of
    that element: a kernel that loses or misplaces any single key fails the parity test."""
    case = ar.case_for(T, klens, h, regime)
    ref = reference(kind, case)
    B = len(klens)
    j = torch.arange(T)
    main = ar.heads(case.v).gather(-1, (j % DK).reshape(1, 1, T, 1).expand(B, h, T, 1)).abs().squeeze(-1)  # [B][h][key]
    term = ref.P * main[:, :, None, :]                                                                    # [B][h][row][key]
    bud = ar.budget(ref, BF).reshape(B, T, h, DK).permute(0, 2, 1, 3)                                      # [B][h][row][channel]
    bud_at = bud.gather(-1, (j % DK).reshape(1, 1, 1, T).expand(B, h, T, T))
    seen = (term / bud_at).amax(dim=(1, 2))                                                                # [B][key]
    valid = j[None, :] < ar.key_counts(case)[:, None]
    assert bool((seen[valid] >= 10).all()), (float(seen[valid].min()), int((seen[valid] < 10).sum()))


@pytest.mark.parametrize("kind,T,klens,h,regime", [p for p in PARAMS if p.values[4] == "sharp" and p.values[1] > 64])
def test_sharp_is_sharp(kind, T, klens, h, regime):
    """The sharp regime makes the running maximum move: some row's largest score is in the first 64-key tile and some row's
    in the last, and |score| reaches 20 under every score definition."""
    case = ar.case_for(T, klens, h, regime)
    ref = reference(kind, case)
    kl = ar.key_counts(case)
    first = last = False
    for b in range(len(klens)):
        n = int(kl[b])
        if n <= 64:
            continue
        top = ref.P[b, :, :, :n].argmax(-1)
        first |= bool((top < 64).any())
        last |= bool((top >= (n - 1) // 64 * 64).any())
    assert first and last
    assert float(ref.S.max()) >= 20


# ------------------------------------------------------------------------------------------ wrong variants
def _scores_of(kind, case, bd_edit=None):
    """the reference's scores, with the position term passed through bd_edit(bd, q_v, p) -> bd"""
    if kind == "abs":
        assert bd_edit is None
        return ar.abs_scores(case)
    q_u, q_v, scale = ar.biased_queries(case, KINDS[kind][0])
    legacy = kind == "legacy"
    p = ar.position_rows(case, case.T if legacy else 2 * case.T - 1)
    term = ar.legacy_bd if legacy else ar.rel_bd
    bd = term(q_v, p)
    if bd_edit is not None:
        bd = bd_edit(bd, lambda qv2, p2: term(qv2, p2), q_v, p)
    return (q_u @ ar.heads(case.k).transpose(-2, -1) + bd) * scale


def _next_row(p):
    """the position table read one row too far (clamped at its end)"""
    return torch.cat([p[:, 1:], p[:, -1:]], dim=1)


def v_unmask_one(kind, case, kl):
    if not bool((kl < case.T).any()):
        return None
    return ar.finish(_scores_of(kind, case), case.v, torch.where(kl < case.T, kl + 1, kl))


def _drop(kind, case, kl, key_of):
    scores = _scores_of(kind, case)
    hit = False
    for b in range(len(kl)):
        j = key_of(int(kl[b]))
        if j is not None:
            scores[b, :, :, j] = float("-inf")
            hit = True
    return ar.finish(scores, case.v, kl) if hit else None


def v_drop_last(kind, case, kl):
    return _drop(kind, case, kl, lambda n: n - 1 if n >= 2 else None)


def v_drop_key_64(kind, case, kl):
    return _drop(kind, case, kl, lambda n: 64 if n > 64 else None)


def v_bd_shift_from_256(kind, case, kl):
    if kind == "abs" or not bool((kl > 256).any()):
        return None

    def edit(bd, term, q_v, p):
        out = bd.clone()
        out[..., 256:] = term(q_v, _next_row(p))[..., 256:]
        return out
    return ar.finish(_scores_of(kind, case, edit), case.v, kl)


def v_bd_shift_last_16_queries(kind, case, kl):
    if kind == "abs" or case.T < 2:
        return None
    i0 = (case.T - 1) // 16 * 16

    def edit(bd, term, q_v, p):
        out = bd.clone()
        out[:, :, i0:] = term(q_v, _next_row(p))[:, :, i0:]
        return out
    return ar.finish(_scores_of(kind, case, edit), case.v, kl)


def v_56_channels_last_key(kind, case, kl):
    if kind == "abs" or not bool((kl >= 2).any()):
        return None

    def edit(bd, term, q_v, p):
        short = term(q_v[..., :56], p[..., :56])
        out = bd.clone()
        for b in range(len(kl)):
            if int(kl[b]) >= 2:
                out[b, :, :, int(kl[b]) - 1] = short[b, :, :, int(kl[b]) - 1]
        return out
    return ar.finish(_scores_of(kind, case, edit), case.v, kl)


VARIANTS = [v_unmask_one, v_drop_last, v_drop_key_64, v_bd_shift_from_256, v_bd_shift_last_16_queries, v_56_channels_last_key]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v.__name__[2:] for v in VARIANTS])
@pytest.mark.parametrize("kind,T,klens,h,regime", PARAMS)
def test_wrong_variants_break_the_budget(kind, T, klens, h, regime, variant):
    """Each wrong variant of the reference is at least ten times over the bf16 budget on some element, in every case it
    applies to (a case it cannot apply to - no key past klen, no key 64, ... - passes vacuously)."""
    case = ar.case_for(T, klens, h, regime)
    ref = reference(kind, case)
    wrong = variant(kind, case, ar.key_counts(case))
    if wrong is None:
        return
    r, where = ar.worst(wrong.ctx, ref, BF)
    print(f"variant {variant.__name__[2:]} {kind} T={T} h={h} {regime}: {r:.1f} x budget at {where}")
    assert r >= 10, (r, where)
