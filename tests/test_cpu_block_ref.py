"""The float64 block reference, its probes and its budget (tests/block_ref.py), checked without a GPU: where the two measured
constants come from, that a faithful float32 restatement (two summation orders) stays inside the budget on every probe and
case, that the budget is at most 1 / 100 of the tolerance it replaces, and that fifteen wrong variants of the restatement each
break it.  The variants live here only; nothing mutates a kernel."""
import pytest
import torch
import torch.nn.functional as F

from tests import block_ref as br

F32, F64 = torch.float32, torch.float64
D = br.D
ORDERS = ("torch", "chunk")


def cases_of(name):
    return br.CASE_PARAMS if br.PROBES[name][1] else br.UNMASKED_PARAMS


PROBE_PARAMS = [pytest.param(name, *c, id=f"{name}-B{c[0]}T{c[1]}ff{c[3]}{'m' if c[2] else ''}") for name in br.PROBES for c in cases_of(name)]

_RUNS = {}


def stored(outs):
    """the restatement's outputs as a kernel stores them: the bf16 ones rounded"""
    return {k: v if k in br.Probe.F32_OUT else br.q(v) for k, v in outs.items()}


def runs(name, case):
    """probe, {order: restatement outputs}, {order: reference outputs with the restatement's own x as the shared stage's input}"""
    key = (name, case[0], case[1], tuple(case[2]) if case[2] else None, case[3])
    if key not in _RUNS:
        p = br.probe_for(name, *case)
        sim = {o: stored(p.run(br.SimOps(o))) for o in ORDERS}
        ref = {o: p.run(br.RefOps(), mid=sim[o].get("x")) for o in ORDERS}
        _RUNS[key] = (p, sim, ref)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------ the constants
def _unit_ratio(got, exact, unit):
    err = (got.to(F64) - exact).abs()
    assert bool((err[unit == 0] == 0).all())
    return float((err / unit.clamp_min(1e-300)).max())


def measure_constants(B, T, tlens, ff):
    """(c_acc, c_conv, c_ln) of one case"""
    seed = 300000 + 1000 * T + 10 * B + ff
    ly = br.Layer(seed, ff)
    rows = B * T
    acc = cv = ln_ = 0.0
    a256 = br.q(br.rnd(rows, D, seed=seed + 100))
    aff = br.q(F.silu(br.rnd(rows, ff, seed=seed + 101)))
    x = br.rnd(rows, D, seed=seed + 102) * br.row_scale(B, T, tlens)
    g = br.q(br.rnd(rows, D, seed=seed + 103))
    zero = br.RefOps(c_acc=0.0, c_ln=0.0, c_conv=0.0)
    for o in ORDERS:
        sim = br.SimOps(o)
        for a, W, b in ((a256, ly.ffm_w1, ly.ffm_b1), (aff, ly.ffm_w2, ly.ffm_b2), (a256, ly.wqkv, ly.bqkv), (a256, ly.wout, ly.bout),
                        (a256, ly.pw1, ly.pw1_b), (a256, ly.pw2, ly.pw2_b), (a256, ly.ff_w1, ly.ff_b1), (aff, ly.ff_w2, ly.ff_b2)):
            exact = a.to(F64) @ W.to(F64).t() + b.to(F64)
            unit = br.F32_UNIT * (a.to(F64).abs() @ W.to(F64).abs().t() + b.to(F64).abs())
            acc = max(acc, _unit_ratio(sim.mm(a, W, b), exact, unit))
        exact = zero.conv(zero.inp(g), ly.dw_w, ly.dw_b, B, T, tlens).v
        unit = br.RefOps(c_conv=0.25).conv(zero.inp(g), ly.dw_w, ly.dw_b, B, T, tlens).e  # 4 * 0.25 * 2^-24 * (|w||g| + |b|)
        cv = max(cv, _unit_ratio(sim.conv(g, ly.dw_w, ly.dw_b, B, T, tlens), exact, unit))
        for gg, bb in (ly.ln_mac, ly.ln_mha, ly.ln_conv, ly.ln_ff, ly.ln_final):
            exact = zero.ln(zero.inp(x), gg, bb).v
            unit = br.RefOps(c_acc=0.0, c_ln=0.25).ln(zero.inp(x), gg, bb).e
            ln_ = max(ln_, _unit_ratio(sim.ln(x, gg, bb), exact, unit))
    print(f"CONSTANTS B={B} T={T} ff={ff} masked={tlens is not None}: c_acc {acc:.2f}  c_conv {cv:.2f}  c_ln {ln_:.2f}")
    return acc, cv, ln_


def test_constants_are_measured():
    """C_ACC, C_CONV and C_LN are the worst error of the float32 restatement, both summation orders, in units of
    2^-24 (|W||a| + |b|) resp. 2^-24 (|g| (|yh| + mean|x| / sigma) + |b|), over every matrix, resp. the depthwise conv, resp. every LayerNorm of a layer at
    every case's shape (inputs: bf16 normals; Swish of normals in front of the second FFN matrix; rows of scale 1 and 3 for
    the LayerNorm).  The recorded constants are the maxima over the cases: the figures move a little with
    the CPU's summation order, so the measurement is held to twice the recorded value (half of the factor 4 the budget uses),
    and the recorded value to 1.1 times the measurement - a constant cannot be enlarged without the measurement following."""
    worst = [max(m) for m in zip(*(measure_constants(*c) for c in br.CASE_PARAMS))]
    for name, rec, got in zip(("C_ACC", "C_CONV", "C_LN"), (br.C_ACC, br.C_CONV, br.C_LN), worst):
        assert got <= 2 * rec and rec <= 1.1 * got, (name, rec, got)


def test_sigmoid_bound_covers_float32_sigmoid():
    """sigmoid_rel is derived for the hardware sequence; the float32 torch sigmoid (correctly rounded exp, IEEE division) has
    to sit inside it as well, over the whole range the activations take."""
    v = torch.linspace(-30, 30, 200001, dtype=F32)
    rel = ((torch.sigmoid(v).to(F64) - torch.sigmoid(v.to(F64))) / torch.sigmoid(v.to(F64))).abs()
    assert bool((rel <= br.sigmoid_rel(v.to(F64))).all())


def test_rounding_rule():
    """bf16 rounding point: the value of an unambiguous element is torch's bf16 conversion, an element is ambiguous exactly
    when a rounding boundary is within e, and every f32 within e of an element rounds to a bf16 inside its bound (to the
    same bf16 where the element is unambiguous)."""
    ops = br.RefOps()
    v = (br.rnd(4096, seed=5) * 3).to(F64)  # (float32 values: no second rounding on the way to bf16)
    e = torch.full_like(v, 1e-4)
    out = ops.rb(br.BV(v, e), "t")
    amb = ops.masks["t"]
    assert torch.equal(out.v[~amb], br.q(v.to(F32)).to(F64)[~amb])
    near = amb & (4 * e < br.bf16_ulp(v))
    assert bool(((out.v - v).abs() <= e)[near].all()) and int(near.sum()) > 0  # an ambiguous element's value is the boundary itself
    assert torch.equal(out.v[amb & ~near], br.q(v.to(F32)).to(F64)[amb & ~near])  # (the fall-back: bf16(v) with ulp + e)
    assert 0 < int(amb.sum()) < 400
    for d in (-1.0, 1.0):
        moved = br.q((v + d * e * 0.999).to(F32)).to(F64)
        assert torch.equal(moved[~amb], out.v[~amb])
        assert bool(((moved - out.v).abs() <= out.e)[amb].all())
    assert bool((out.e[~amb] == 0).all())
    z = ops.rb(br.BV(torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64)), "z")
    assert bool((z.v == 0).all()) and bool((z.e == 0).all()) and not bool(ops.masks["z"].any())


# ------------------------------------------------------------------------------------------ the faithful restatement
@pytest.mark.parametrize("name,B,T,tlens,ff", PROBE_PARAMS)
def test_faithful_restatement_in_budget(name, B, T, tlens, ff):
    """The budget is sound: the float32 restatement, in both summation orders, is inside it on every output of every probe
    (worst ratios per probe: block_ref.SIM_WORST; near 1 where a single ambiguous element flips - one ulp against a budget
    of one ulp plus its incoming bound)."""
    p, sim, ref = runs(name, (B, T, tlens, ff))
    for o in ORDERS:
        for out, r in ref[o].items():
            ratio, where = br.worst(sim[o][out], r, out in br.Probe.F32_OUT)
            print(f"FAITHFUL {name} B={B} T={T} ff={ff} masked={tlens is not None} {o} {out}: err / budget {ratio:.3f} at {where}")
            br.assert_in_budget(sim[o][out], r, p, out, f"float32 restatement ({o})")


@pytest.mark.parametrize("name", list(br.PROBES))
def test_budget_is_sharp(name):
    """Per probe and output, the median bound in front of the store - over the elements of all its cases - is at most 1 / 100
    of 4e-3 max|ref|, the tolerance it replaces.  (A bf16 output's budget adds the store's own half ulp, u |v|: the precision
    of the format, which no test can go below; the condition is on what the reference contributes.)

    The issue states the condition per probe; each single case is held to 1 / 50 besides, so that one shape cannot go loose
    behind the others: a case's median may be twice the probe's at most.  (1 / 100 per case is out of reach at ff = 1024 on
    enc_out, which sits behind two more LayerNorms: the expected contribution of the ambiguous level is
    sum_j |w2_j| |f'(h_j)| e_h, e_h = 4 C_ACC 2^-24 (|W1||xn| + |b1|), linear in the measured constant and in ff.)  The test
    prints every figure; the mutants below are caught on every case."""
    pool = {}
    for c in cases_of(name):
        _, _, ref = runs(name, c)
        for out, r in ref["torch"].items():
            med, old = float(r.e.median()), 4e-3 * float(r.v.abs().max())
            print(f"SHARP {name} B={c[0]} T={c[1]} ff={c[3]} masked={c[2] is not None} {out}: median bound {med:.3e} = 1 / {old / max(med, 1e-300):.0f} of {old:.3e}")
            assert med <= old / 50, (c, out, med, old)
            pool.setdefault(out, []).append(r)
    for out, rs in pool.items():
        med = float(torch.cat([r.e.flatten() for r in rs]).median())
        old = 4e-3 * max(float(r.v.abs().max()) for r in rs)
        print(f"SHARP {name} {out}: median bound {med:.3e} = 1 / {old / max(med, 1e-300):.0f} of {old:.3e}")
        assert med <= old / 100, (out, med, old)


def test_probe_inputs_are_as_stated():
    p = br.probe_for("df_ffn", 3, 70, [70, 33, 32], 1024)
    assert br.probe_for("df_ffn", 3, 70, [70, 33, 32], 1024) is p  # one set of inputs per case, shared
    g3 = p.glu.reshape(3, 70, D)
    assert bool((g3[1, :33] == 0).all()) and bool((g3[0] == 0).all()) and 2.0 < float(g3[1, 33:].std()) < 4.0
    assert torch.equal(p.glu, br.q(p.glu)) and bool((p.l0.dw_b == 0).all())
    ops = br.RefOps()
    p.run(ops)
    assert not bool(ops.masks["ln_ff"].any()) and not bool(ops.masks["conv"].any())  # LN-clean rows, exact conv phase
    assert bool(ops.masks["ff_h"].any())                                               # the one ambiguous level
    p = br.probe_for("df_conv", 3, 70, [70, 33, 32], 1024)
    x3 = p.x0.reshape(3, 70, D)
    assert 2.5 < float(x3[2, 32:].std() / x3[2, :32].std()) < 3.5
    assert bool((p.l0.ff_w2 == 0).all()) and torch.equal(p.glu, br.q(p.glu))
    for c in br.CASE_PARAMS:  # the D part hands the macaron module an exact, LN-clean row: one ambiguous level on every case
        p = br.probe_for("da_mac", *c)
        ops = br.RefOps()
        p.run(ops)
        assert not bool(ops.masks["ln_mac"].any()) and not bool(ops.masks["conv"].any()), c
    p = br.probe_for("attc", 3, 70, None, 1024)
    assert torch.equal(p.ctx.reshape(3, 70, D)[1, 69], p.v0[1]) and torch.equal(p.ctx, br.q(p.ctx))


def test_clean_rows_fail_loudly():
    with pytest.raises(AssertionError, match="LN-clean"):
        br.clean_rows(torch.ones(8, 1), 1, lambda x: torch.ones(x.shape, dtype=torch.bool))


# ------------------------------------------------------------------------------------------ wrong variants
class Mutant(br.SimOps):
    """the torch-order restatement with one stage edited; `applies` says whether the case has what the edit needs"""
    probes = ()

    def __init__(self, probe):
        super().__init__("torch")
        self.p = probe

    def applies(self):
        return True


def _tap_drop(frame, tap):
    """y[0][frame][c] loses tap `tap` (which reads frame + tap - 15), c = the channel where that term is largest"""
    class TapDrop(Mutant):
        probes = ("df_conv", "da_conv", "cda_conv", "cdf_conv")

        def applies(self):
            return 0 <= frame + tap - br.HALF < min(self.p.T, self.p.tlens[0] if self.p.tlens else self.p.T) and frame < self.p.T

        def conv(self, g, w, b, B, T, tlens, tag=None):
            g3 = self.conv_input(g, B, T, tlens)
            y = self.conv_of(g3, w, b)
            term = w[tap] * g3[0, frame + tap - br.HALF]
            c = int(term.abs().argmax())
            y[0, frame, c] -= term[c]
            return y.reshape(B * T, D)
    return TapDrop


class MaskOffByOne(Mutant):
    probes = ("df_conv", "da_conv", "cda_conv", "cdf_conv")

    def applies(self):
        return self.p.tlens is not None and any(n < self.p.T for n in self.p.tlens)

    def conv(self, g, w, b, B, T, tlens, tag=None):
        return super().conv(g, w, b, B, T, [min(n + 1, T) for n in tlens])


class ConvFlattened(Mutant):
    probes = ("df_conv", "da_conv", "cda_conv", "cdf_conv")

    def applies(self):
        return self.p.B > 1

    def conv(self, g, w, b, B, T, tlens, tag=None):
        g3 = self.conv_input(g, B, T, tlens)
        return self.conv_of(g3.reshape(1, B * T, D), w, b).reshape(B * T, D)


def _hidden_drop(tag_w2, probes_):
    class HiddenDrop(Mutant):
        probes = probes_

        def mm(self, a, W, b, tag=None):
            if tag == tag_w2:
                a = a.clone()
                a[0, int((a[0].abs() * W.abs().sum(0)).argmax())] = 0
            return super().mm(a, W, b)
    return HiddenDrop


def _b1_last_chunk(tag_w1, probes_):
    class B1LastChunk(Mutant):
        probes = probes_

        def applies(self):
            return self.p.ff in (192, 64)

        def mm(self, a, W, b, tag=None):
            if tag == tag_w1:
                b = b.clone()
                b[-64:] = 0
            return super().mm(a, W, b)
    return B1LastChunk


class Pw2BiasMissing(Mutant):
    probes = ("df_conv", "df_ffn", "da_conv", "da_ffn", "cda_conv", "cda_ffn", "cdf_conv", "cdf_ffn")  # (da_mac: a zero norm_final gain hides the whole D part, by design)

    def mm(self, a, W, b, tag=None):
        return super().mm(a, W, torch.zeros_like(b) if tag == "pw2" else b)


def _ln_gain_neighbour(tag_ln, other, probes_):
    """the gain of the channel where the two differ most comes from the LayerNorm next to it in the parameter group"""
    class LnGainNeighbour(Mutant):
        probes = probes_

        def ln(self, x, g, b, tag=None):
            if tag == tag_ln:
                ly = self.p.l0 if tag_ln in ("ln_ff", "ln_conv") else self.p.l1
                og = getattr(ly, other)[0]
                c = int((g - og).abs().argmax())
                g = g.clone()
                g[c] = og[c]
            return super().ln(x, g, b)
    return LnGainNeighbour


class KHeadSwapped(Mutant):
    probes = ("a", "da_conv", "da_ffn", "da_mac")

    def mm(self, a, W, b, tag=None):
        y = super().mm(a, W, b)
        if tag == "wqkv":
            y[:, D:D + 64], y[:, D + 64:D + 128] = y[:, D + 64:D + 128].clone(), y[:, D:D + 64].clone()
        return y


class GluGateMispaired(Mutant):
    probes = ("c", "attc")

    def glu(self, y, tag=None):
        y = y.clone()
        y[:, D + 7] = y[:, D + 8]
        return super().glu(y)


MUTANTS = {
    "tap_tile_first_frame": _tap_drop(br.TILE, br.HALF - 1),       # frame 32 reads frame 31: the previous tile
    "tap_tile_last_frame": _tap_drop(br.TILE - 1, br.HALF + 1),    # frame 31 reads frame 32: the next tile
    "tap_frame_0": _tap_drop(0, br.HALF),
    "conv_mask_off_by_one": MaskOffByOne,
    "conv_flattened": ConvFlattened,
    "hidden_unit_dropped": _hidden_drop("ff_w2", ("df_ffn", "da_ffn", "cda_ffn", "cdf_ffn")),
    "hidden_unit_dropped_macaron": _hidden_drop("ffm_w2", ("a", "da_mac")),
    "b1_last_chunk_missing": _b1_last_chunk("ff_w1", ("df_ffn", "da_ffn", "cda_ffn", "cdf_ffn")),
    "b1_last_chunk_missing_macaron": _b1_last_chunk("ffm_w1", ("a", "da_mac")),
    "pw2_bias_missing": Pw2BiasMissing,
    "ln_ff_gain_from_ln_final": _ln_gain_neighbour("ln_ff", "ln_final", ("df_ffn", "da_ffn")),
    "ln_mha_gain_from_ln_mac": _ln_gain_neighbour("ln_mha", "ln_mac", ("a",)),
    "ln_conv_gain_from_ln_ff": _ln_gain_neighbour("ln_conv", "ln_ff", ("c", "attc")),
    "k_head_swapped": KHeadSwapped,
    "glu_gate_mispaired": GluGateMispaired,
}
MUTANT_PARAMS = [pytest.param(m, name, *c, id=f"{m}-{name}-B{c[0]}T{c[1]}ff{c[3]}{'m' if c[2] else ''}")
                 for m, cls in MUTANTS.items() for name in cls.probes for c in cases_of(name)]


@pytest.mark.parametrize("mutant,name,B,T,tlens,ff", MUTANT_PARAMS)
def test_wrong_variants_break_the_budget(mutant, name, B, T, tlens, ff):
    """Each wrong variant of the restatement exceeds the budget on at least one element of some output, in every case it
    applies to (a case it cannot apply to - one tile, one utterance, no masked frame, ff = 1024 - passes vacuously).  The
    reference takes the variant's own x as the shared stage's input, exactly as the GPU test takes the device's."""
    p, _, _ = runs(name, (B, T, tlens, ff))
    ops = MUTANTS[mutant](p)
    if not ops.applies():
        return
    got = stored(p.run(ops))
    ref = p.run(br.RefOps(), mid=got.get("x"))
    r = max(br.worst(got[out], ref[out], out in br.Probe.F32_OUT)[0] for out in ref)
    print(f"MUTANT {mutant} {name} B={B} T={T} ff={ff} masked={tlens is not None}: {r:.1f} x budget")
    assert r > 1.0, r
