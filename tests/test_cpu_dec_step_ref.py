"""The float64 reference of the decoder step kernels (tests/dec_step_ref.py), checked without a GPU: it equals a literal
float64 MultiHeadedAttention (attention.py:121-151) over the gathered prefix or memory on every case; where the float32
constant of the budget comes from; a faithful bf16 kernel of either form stays inside the budget; and the budget is sharp
enough: a dropped key, a key from another cache slot, klens off by one, an unmasked id-0 key and the ancestor table of the
wrong step parity each leave it in every case.  The faults live here only; nothing mutates a kernel."""
import pytest
import torch

from tests import attention_ref as ar
from tests import dec_step_ref as dr

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = {"bf16": BF, "f32": F32}
FAMILIES = ["self", "tok", "tree", "src"]
PARAMS = [pytest.param(fam, name, regime, id=f"{fam}-{name}-{regime}") for fam in FAMILIES for name in DTYPES
          for regime in dr.REGIMES if not (fam == "tree" and name == "f32")]


def items(family, dtype, regime):
    """(label, operands (q, k, v, vis, post_scale), (case, pos, step) or (case,)) of every case of a family"""
    if family in ("self", "tok"):
        for h, d in dr.SELF_SHAPES:
            case = dr.self_case(dr.SELF_N, dr.SELF_N, h, d, dr.SELF_LMAX, regime, dtype, tok=family == "tok")
            for pos in (dr.SELF_POS if family == "self" else dr.TOK_POS):
                step = dr.at_position(case, pos)
                yield f"{family} d_k={d // h} pos={pos}", (*dr.self_operands(case, pos, step), 1.0), (case, pos, step)
    elif family == "tree":
        for W, Lmax in dr.TREE_W_LMAX:
            for kind in dr.TREE_KINDS:
                case = dr.self_case(dr.TREE_B * W, W, dr.TREE_HEADS, dr.TREE_D, Lmax, regime, dtype, kind)
                for pos in dr.tree_positions(kind, W, Lmax):
                    step = dr.at_position(case, pos)
                    ops = dr.self_operands(case, pos, step, kernel="tree")
                    yield f"tree W={W} {kind} pos={pos}", (*ops, 1.0), (case, pos, step)
    else:
        for h, d in dr.SRC_SHAPES:
            for T, W, _ in dr.src_cases():
                case = dr.src_case(T, W, h, d, regime, dtype)
                yield f"src d_k={d // h} T={T} W={W}", dr.src_operands(case), (case,)


def literal(q, k, v, vis, post, dt):
    """forward_attention (attention.py:121-151) per row: scores [R][h][1][L], masked_fill(min), softmax, masked_fill(0)"""
    R, L, h, c = k.shape
    scores = (q.to(dt)[:, :, None, :] @ k.to(dt).permute(0, 2, 3, 1)) * post
    mask = ~vis[:, None, None, :]
    attn = torch.softmax(scores.masked_fill(mask, torch.finfo(dt).min), -1).masked_fill(mask, 0.0)
    return (attn @ v.to(dt).permute(0, 2, 1, 3)).reshape(1, R, h * c)


@pytest.mark.parametrize("family,name,regime", PARAMS)
def test_reference_equals_literal_attention_in_float64(family, name, regime):
    for label, ops, _ in items(family, DTYPES[name], regime):
        ref = dr.attend(*ops)
        want = literal(*ops, F64)
        err = (ref.ctx - want).abs()
        allow = 16 * 2.0 ** -53 * (1 + ref.S) * ref.A  # a few float64 ulps of what the element sums
        assert bool((err <= allow).all()), (label, float((err / allow.clamp_min(1e-300)).max()))
        assert bool((ref.ctx[ref.A == 0] == 0).all()), label
        assert bool(torch.isfinite(ref.ctx).all()), label


def test_inputs_are_as_stated():
    case = dr.self_case(dr.SELF_N, dr.SELF_N, 3, 192, dr.SELF_LMAX, "flat", BF, tok=True)
    pos = 130
    qkv, kc, vc = dr.at_position(case, pos)
    for t in (qkv, kc, vc):
        assert torch.equal(t, ar.rd(t, BF))
    assert bool((kc[pos:].abs() == dr.POISON).all()) and bool((vc[pos:].abs() == dr.POISON).all())
    named = torch.zeros(case.Lmax, case.n, dtype=torch.bool)
    named[torch.arange(case.Lmax)[None, :].expand(case.n, case.Lmax), case.anc.long()] = True
    assert bool((~named).any(1).all())                                    # a free slot at every position
    assert bool((kc[:pos][~named[:pos]].abs() == dr.POISON).all())        # ... which holds the poison
    assert not bool(named[torch.arange(case.Lmax)[None, :].expand(case.n, case.Lmax), case.other.long()].any())
    live = vc[:pos][named[:pos]].reshape(-1, case.h, case.dk)
    assert bool(((live != 0).sum(-1) == 2).all())
    _, _, _, vis = dr.self_operands(case, pos, (qkv, kc, vc))
    assert not bool(vis[case.n - 1].any()) and not bool(vis[2, pos]) and bool(vis[:case.n - 1].any(1).all())
    assert dr.self_case(dr.SELF_N, dr.SELF_N, 3, 192, dr.SELF_LMAX, "flat", BF, tok=True) is case
    # 1 / 8 in the operand (tree kernel) and in f32 (per-row kernel) are the same numbers for d_k = 64
    tree = dr.self_case(10, 5, 2, 128, 512, "sharp", BF, "beam_tree")
    step = dr.at_position(tree, 257)
    assert torch.equal(dr.self_query(tree, step[0], "tree"), dr.self_query(tree, step[0], "row"))
    src = dr.src_case(33, 5, 3, 192, "flat", F32)
    kvv = src.kv.reshape(src.B, src.T, 2, src.d)
    for b, kl in enumerate(src.klens):
        assert bool((kvv[b, min(kl, src.T):].abs() == dr.POISON).all())
    assert sorted({W for _, W, _ in dr.src_cases()}) == dr.SRC_W and {T for T, _, _ in dr.src_cases()} == set(dr.SRC_T)
    assert any(Tp == (T + 31) // 32 * 32 + 32 for T, _, Tp in dr.src_cases())


@pytest.mark.parametrize("family,name,regime", PARAMS)
def test_float32_restatement_is_where_f_comes_from(family, name, regime):
    """The float32 torch restatement's worst error over the decoder's cases, in units of 2^-24 (1 + S) A, stays under
    attention_ref.F32_REF_MAX, so the decoder is held to attention_ref.F unchanged.  The figure moves a little with the
    summation order of the CPU's matrix product: it is held to twice the recorded maximum as well."""
    top = 0.0
    for label, ops, _ in items(family, DTYPES[name], regime):
        ref = dr.attend(*ops)
        unit = ar.F32_UNIT * (1 + ref.S) * ref.A
        err = (literal(*ops, F32).to(F64) - ref.ctx).abs()
        assert bool((err[unit == 0] == 0).all()), label
        top = max(top, float((err / unit.clamp_min(1e-300)).max()))
    print(f"f32 restatement {family} {name} {regime}: {top:.2f} x 2^-24 (1 + S) A")
    assert top <= ar.F32_REF_MAX
    assert top <= 2 * dr.F32_REF_MAX_DEC


def simulate(q, k, v, vis, post, rounded):
    """A faithful bf16 kernel on the CPU: float32 scores, exp(s - max) in float32; `rounded`: every probability rounded to
    bf16 before P . V and before the denominator sums it (source and tree kernels), otherwise float32 probabilities (the
    per-row kernel); float32 accumulation, one rounding at the store."""
    R, L, h, c = k.shape
    s = torch.einsum("rhc,rlhc->rhl", q.to(F32), k.to(F32)) * post
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.where(torch.isfinite(m), torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(s))
    if rounded:
        p = ar.rd(p, BF)
    l = p.sum(-1, keepdim=True)
    acc = torch.einsum("rhl,rlhc->rhc", p, v.to(F32))
    out = torch.where(l > 0, acc / l.clamp_min(1e-30), torch.zeros_like(acc))
    return ar.rd(out, BF).reshape(1, R, h * c)


@pytest.mark.parametrize("family,name,regime", [p for p in PARAMS if p.values[1] == "bf16"])
def test_bf16_simulations_inside_budget(family, name, regime):
    """The budget is reachable by both forms (worst values: dec_step_ref.SIM_ROW_BF16_MAX, SIM_RND_BF16_MAX)."""
    top = {False: 0.0, True: 0.0}
    for label, ops, _ in items(family, BF, regime):
        ref = dr.attend(*ops)
        for rounded in (False, True):
            r, where = ar.worst(simulate(*ops, rounded), ref, BF)
            assert r <= 1.0, (label, rounded, r, where)
            top[rounded] = max(top[rounded], r)
    print(f"bf16 simulation {family} {regime}: per-row form {top[False]:.3f}, rounded probabilities {top[True]:.3f} of the budget")
    assert top[False] <= min(1.0, 1.5 * dr.SIM_ROW_BF16_MAX) and top[True] <= min(1.0, 1.5 * dr.SIM_RND_BF16_MAX)


# ------------------------------------------------------------------------------------------ faults
def drop_last(ops):
    q, k, v, vis, post = ops
    vis = vis.clone()
    L = vis.shape[1]
    last = (vis * torch.arange(1, L + 1)[None, :]).amax(1) - 1  # (-1: no visible key)
    rows = torch.nonzero(last >= 0).squeeze(1)
    vis[rows, last[rows]] = False
    return q, k, v, vis, post


def self_faults(case, pos, step, ops, kernel):
    """name -> operands of the faulty attention"""
    out = {"last key dropped": drop_last(ops)}
    vis = ops[3]
    if pos >= 1:
        # one prefix key of every row (its first visible one) from the next slot of the beam at the same position
        first = (vis[:, :pos].long() * torch.arange(pos, 0, -1)[None, :]).argmax(1)
        has = vis[:, :pos].any(1)
        anc = case.anc.clone()
        rows = torch.nonzero(has).squeeze(1)
        base = (rows // case.W * case.W).to(torch.int32)
        anc[rows, first[rows]] = base + (anc[rows, first[rows]] - base + 1) % case.W
        out["key from another slot"] = (*dr.self_operands(case, pos, step, anc, kernel), 1.0)
        out["table of the wrong parity"] = (*dr.self_operands(case, pos, step, case.other, kernel), 1.0)
    if case.tok is not None:
        hidden = ~vis
        L = vis.shape[1]
        firsth = (hidden.long() * torch.arange(L, 0, -1)[None, :]).argmax(1)
        rows = torch.nonzero(hidden.any(1)).squeeze(1)
        v2 = vis.clone()
        v2[rows, firsth[rows]] = True
        out["id-0 key unmasked"] = (ops[0], ops[1], ops[2], v2, ops[4])
    return out


def src_faults(case, ops):
    T = case.T
    kl = [min(n, T) for n in case.klens]
    out = {"last key dropped": drop_last(ops)}
    out["klens one more"] = dr.src_operands(case, klens=[min(n + 1, T) for n in kl])
    out["klens one less"] = dr.src_operands(case, klens=[max(n - 1, 1) for n in kl])
    return out


@pytest.mark.parametrize("family,name,regime", PARAMS)
def test_every_fault_leaves_the_budget(family, name, regime):
    """Each fault, applied to the reference, is outside the budget in every case in which it changes the keys of a row
    that has at least two visible keys."""
    dtype = DTYPES[name]
    seen = set()
    for label, ops, extra in items(family, dtype, regime):
        ref = dr.attend(*ops)
        two = ops[3].sum(1) >= 2
        if family == "src":
            faults = src_faults(extra[0], ops)
        else:
            faults = self_faults(*extra, ops, "tree" if family == "tree" else "row")
        for fault, fops in faults.items():
            changed = (fops[3] != ops[3]).any(1) | (fops[1] != ops[1]).flatten(1).any(1)
            if not bool((changed & two).any()):
                continue
            r, where = ar.worst(dr.attend(*fops).ctx, ref, dtype)
            assert r > 1.0, (label, fault, r, where)
            seen.add(fault)
    want = {"self": {"last key dropped", "key from another slot", "table of the wrong parity"},
            "tree": {"last key dropped", "key from another slot", "table of the wrong parity"},
            "tok": {"last key dropped", "key from another slot", "table of the wrong parity", "id-0 key unmasked"},
            "src": {"last key dropped", "klens one more", "klens one less"}}[family]
    assert seen == want, seen
