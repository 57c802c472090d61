"""Float64 restatement of the row-local phases of the fused Conformer block kernels (csrc/block.hip) that carries a
per-element error bound, the probes that observe one phase at a time, and the budget the CPU and the GPU parity tests share
(tests/test_cpu_block_ref.py, tests/test_gpu_block.py).

  Layer            random weights of one EncoderLayer, its host packing and the float32 torch restatements of the full chains
  RefOps           the stages in float64 on bounded values BV(v, e): a faithful kernel (float32 arithmetic on bf16 operands,
                   any summation order) is within e of v, element by element
  SimOps           the same stages in float32, in two summation orders: the faithful restatement the budget is proved on
  part_a / part_c / part_d / after_norm   the chains, written once over either set of stages
  probe_for        the inputs and the (edited) weights that make ONE phase visible, per (probe, case, masked)
  worst / assert_in_budget   err / budget per element, the worst element named

The rules of the bound (RefOps):

  matrix product   y = W a + b, f32 accumulate:  e_y = |W| e_a + 4 C_ACC 2^-24 (|W||a| + |b|); the depthwise conv is the same
                   form over its 31 taps, |w||g| + |b|, with a constant of its own (C_CONV: 31 terms summed one by one
                   behave differently from 256 .. 1024 summed in blocks, and one constant for both would be the conv's -
                   three times the matrix products' - on every matrix).  Both are MEASURED: the worst error of the float32
                   restatement (torch's summation order, and K in chunks of 32 accumulated in sequence / the conv tap by
                   tap) in units of 2^-24 (|W||a| + |b|); the factor 4 is the margin tests/attention_ref.py gives for the
                   hardware's accumulation order.
  residual add     e = e_x + e_y + 2^-24 |sum| (nothing where the addend is exactly zero: x + 0 is exact)
  LayerNorm        first order in e:  e_y = |g| / sigma (e + mean(e) + |yh| mean(|yh| e)) (1 + 4 max(e) / sigma)
                                            + 4 C_LN 2^-24 (|g| (|yh| + mean|x| / sigma) + |b|),   yh = (x - mean) / sigma.
                   The first part is the exact first-order term, d yh_c = (d_c - mean(d) - yh_c mean(yh d)) / sigma, bounded
                   term by term (mean(|yh| e) <= rms(e), so it is never above e + mean(e) + |yh| (rms(e) + mean(e))); the
                   factor behind it covers the second order, which is (max(e) / sigma) times the first.
                   The float32 term has one part more than |yh g| + |b|: the float32 mean is off by a few 2^-24 mean|x|
                   ABSOLUTE, which reaches every element of the row as (that) / sigma however small its own yh is.  Without
                   it the unit vanishes where yh g and b happen to cancel, the measured constant is an outlier statistic (209
                   instead of 3.5) and no row is ever LN-clean; with it the bound is 60 times tighter on the typical element.
                   C_LN is measured like C_ACC.
  Swish, GLU       e_out = Lip e + (r(v) + 2^-24) |f(v)|, Lip the Lipschitz constant ON [v - e, v + e]: |f'(v)| + max|f''| e
                   (never above the global 1.1 of v s(v) and 1 / 4 of s(v); a negative pre-activation, where Swish is flat,
                   passes on a tenth of its bound); r(v) is the relative error of the kernels' sigmoid, see sigmoid_rel.
  bf16 rounding    r = bf16(v).  Where v is farther than e from the nearest rounding boundary (the midpoint of two
                   neighbouring bf16 numbers) every value within e rounds to the same r: e_out = 0.  Otherwise the element is
                   AMBIGUOUS: the kernel's value is one of the two bf16 numbers either side of that boundary m, so the
                   reference takes m itself with e_out = ulp / 2 - half of what r with ulp + e allows, and as sound (where
                   4 e reaches a whole ulp, which no probe does, it falls back to r and ulp + e, ulp of the binade of
                   |v| + e).  This is what keeps the budget sharp: behind a rounding point the error is exactly zero on all
                   but a few elements.
  stored outputs   f32: e.  bf16: e + u |v| against the UNROUNDED v, u = 2^-8 (attention_ref.U_BF16).

A chain of three rounding points cannot be bounded sharply, so every probe has at most one ambiguous level in front of its
output: the stage in front of the observed phase is made exact (zero weights, or LN-clean rows: rows where the reference
flags no ambiguous element at that LayerNorm - decided by the reference alone), and a stage shared by two outputs takes the
device's own f32 result as the reference's input (the q / k / v projections start from the x the launch wrote).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from espnet_amd.lib import EM_BLOCK_PARAM_GROUP as G  # floats per parameter group
from oracle import conformer as oc
from tests.attention_ref import F32_UNIT, U_BF16

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
D = 256
EPS = 1e-12
KW, HALF = 31, 15
TILE = 32  # frames per workgroup; the conv reads HALF frames either side

# The float32 restatement's worst error over every matrix, the conv and every LayerNorm of a layer at every case's shape,
# both summation orders, in units of 2^-24 (|W||a| + |b|) resp. 2^-24 (|g| (|yh| + mean|x| / sigma) + |b|):
# tests/test_cpu_block_ref.py::test_constants_are_measured reproduces them.  Measured on the CPU, never fitted to GPU output.
C_ACC = 2.37   # (B = 3, T = 70, ff = 1024; 2.00 .. 2.20 on the other cases)
C_CONV = 5.00  # (B = 1, T = 32, tap by tap; 3.48 .. 4.21 on the other cases)
C_LN = 3.46   # (B = 3, T = 70; 2.88 .. 3.31 on the other cases)
# Worst err / budget of the float32 restatement per probe, over the cases and both summation orders, on the float32 outputs
# (tests/test_cpu_block_ref.py::test_faithful_restatement_in_budget prints them; they move with the CPU's summation order
# wherever an ambiguous element flips: half an ulp against a budget of half an ulp plus the accumulate terms, hence 0.999).
# The bf16 outputs reach 0.97 .. 0.995 on every probe: the store's own half ulp
# against u |v| at the bottom of a binade.
SIM_WORST = {"a": 0.999, "c": 0.198, "df_conv": 0.518, "df_ffn": 0.513, "da_conv": 0.780, "da_ffn": 0.798,
             "da_mac": 0.863, "cda_conv": 0.772, "cda_ffn": 0.794, "cdf_conv": 0.552, "cdf_ffn": 0.477, "attc": 0.156}
# The kernels on an MI355X (tests/test_gpu_block.py::test_block_*_parity print them), float32 outputs; bf16 outputs 0.995 at most.
GPU_WORST = {"a": 0.999, "c": 0.098, "df_conv": 0.518, "df_ffn": 0.513, "da_conv": 0.780, "da_ffn": 0.798, "da_mac": 0.862,
             "cda_conv": 0.772, "cda_ffn": 0.794, "cdf_conv": 0.552, "cdf_ffn": 0.477, "attc": 0.092}

SWISH_CURV, SIGMOID_CURV = 0.5, 0.1  # max |f''| of v s(v) (0.5, at 0) and of s(v) (0.0962)

# (B, T, tlens, ff): two tile edges with a masked tail ending on a tile edge and one frame past it; a partial tile with a
# one-frame utterance; exactly one tile with an odd ff / 64 (the zero-padded b1 slots)
CASES = [(3, 70, [70, 33, 32], 1024), (2, 31, [31, 1], 64), (1, 32, None, 192)]
CASE_PARAMS = [(B, T, tl if m else None, ff) for B, T, tl, ff in CASES for m in ((False, True) if tl else (False,))]
CASE_IDS = [f"B{B}T{T}ff{ff}{'m' if tl else ''}" for B, T, tl, ff in CASE_PARAMS]
UNMASKED_PARAMS = [(B, T, None, ff) for B, T, _, ff in CASES]
UNMASKED_IDS = [f"B{B}T{T}ff{ff}" for B, T, _, ff in UNMASKED_PARAMS]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def q(t):
    return t.to(BF).to(torch.float32)


def ln(x, g, b):
    return F.layer_norm(x, (D,), g, b, EPS)


def group(*vecs):
    v = torch.cat([t.reshape(-1).float() for t in vecs])
    return F.pad(v, (0, G - v.numel()))


def pad_ff(b):
    return F.pad(b, (0, 1024 - b.numel()))


# ------------------------------------------------------------------------------------------ weights
class Layer:
    """Random weights of one EncoderLayer (bf16-rounded matrices, f32 vectors) + its host packing."""

    def __init__(self, seed, ff):
        s = iter(range(seed, seed + 100))
        self.ff = ff
        w = lambda n, k: q(rnd(n, k, seed=next(s), scale=k ** -0.5))
        vb = lambda n: rnd(n, seed=next(s), scale=0.1)
        lng = lambda: (1 + 0.1 * rnd(D, seed=next(s)), 0.1 * rnd(D, seed=next(s)))
        self.ln_mac, self.ln_mha, self.ln_conv, self.ln_ff, self.ln_final = lng(), lng(), lng(), lng(), lng()
        self.ffm_w1, self.ffm_b1, self.ffm_w2, self.ffm_b2 = w(ff, D), vb(ff), w(D, ff), vb(D)
        self.ff_w1, self.ff_b1, self.ff_w2, self.ff_b2 = w(ff, D), vb(ff), w(D, ff), vb(D)
        self.wqkv, self.bqkv = w(3 * D, D), vb(3 * D)
        self.wout, self.bout = w(D, D), vb(D)
        self.pw1, self.pw1_b = w(2 * D, D), vb(2 * D)
        self.dw_w, self.dw_b = rnd(31, D, seed=next(s), scale=0.25), vb(D)  # [k][d], BatchNorm already folded
        self.pw2, self.pw2_b = w(D, D), vb(D)

    # torch fp32 restatements with the bf16 rounding points of the bf16 path
    def part_a(self, x):
        xn = q(ln(x, *self.ln_mac))
        x = x + 0.5 * (q(oc.swish(xn @ self.ffm_w1.t() + self.ffm_b1)) @ self.ffm_w2.t() + self.ffm_b2)
        qkv = q(ln(x, *self.ln_mha)) @ self.wqkv.t() + self.bqkv
        return x, qkv

    def part_c(self, x, ctx):
        x = x + ctx @ self.wout.t() + self.bout
        y = q(ln(x, *self.ln_conv)) @ self.pw1.t() + self.pw1_b
        return x, y[:, :D] * torch.sigmoid(y[:, D:])

    def part_d(self, x, glu, B, T, tlens=None):
        g3 = q(glu).reshape(B, T, D).clone()
        if tlens is not None:
            for b, n in enumerate(tlens):
                g3[b, n:] = 0
        conv = F.conv1d(g3.transpose(1, 2), self.dw_w.t().reshape(D, 1, 31), self.dw_b, padding=15, groups=D)
        c = q(oc.swish(conv.transpose(1, 2).reshape(B * T, D)))
        x = x + c @ self.pw2.t() + self.pw2_b
        xn = q(ln(x, *self.ln_ff))
        x = x + 0.5 * (q(oc.swish(xn @ self.ff_w1.t() + self.ff_b1)) @ self.ff_w2.t() + self.ff_b2)
        return ln(x, *self.ln_final)

    def a_groups(self):
        return [group(*self.ln_mac, pad_ff(self.ffm_b1), self.ffm_b2), group(*self.ln_mha, self.bqkv)]

    def d_groups(self):
        return [group(self.pw2_b, *self.ln_ff), group(pad_ff(self.ff_b1), self.ff_b2, *self.ln_final)]

    def perm(self):
        return torch.cat([torch.cat([torch.arange(64 * j, 64 * j + 64), torch.arange(D + 64 * j, D + 64 * j + 64)])
                          for j in range(4)])

    def c_group(self):
        return group(self.bout, *self.ln_conv, self.pw1_b[self.perm()])


# ------------------------------------------------------------------------------------------ bounded float64 stages
BV = namedtuple("BV", "v e")  # float64 value and the bound e >= 0 on a faithful kernel's distance from it


def sigmoid_rel(v):
    """Relative error bound of the kernels' sigmoid, rcp(1 + __expf(-v)) (csrc/em_common.h: sigmoidf_), derived from how it
    is built:
      __expf(x) is v_exp_f32(x * log2(e)).  The float32 constant log2(e) is within 2^-24 relative of the true one and the
      product rounds once: the argument t of the hardware 2^t is off by at most 2 * 2^-24 |t| ABSOLUTE, which is
      2 * 2^-24 |t| ln 2 = 2 * 2^-24 |v| RELATIVE in 2^t (this is the part that grows with |v|); v_exp_f32 is good to one
      ulp, 2^-23 relative.  So E = exp(-v) (1 + d_E), |d_E| <= 2^-24 (2 |v| + 2).
      1 + E rounds once (2^-24), and d_E reaches the sum with weight E / (1 + E) = 1 - s(v).
      v_rcp_f32 is good to one ulp (2^-23).
    r(v) = (1 - s(v)) 2^-24 (2 |v| + 2) + 3 * 2^-24.  (An E below the normal range is flushed to zero: |v| > 87, where 1 + E
    is 1 either way.)  The product with the other factor (Swish: v, GLU: the value half) rounds once more: + 2^-24, added
    by the callers."""
    s = torch.sigmoid(v)
    return (1.0 - s) * F32_UNIT * (2.0 * v.abs() + 2.0) + 3.0 * F32_UNIT


def bf16_ulp(a):
    """ulp of the bf16 binade of |a| (float64 in, float64 out); the binade of 0 is taken as [2^-1, 1)"""
    _, ex = torch.frexp(a.abs())
    return torch.ldexp(torch.ones_like(a), ex - 8)


class RefOps:
    """The stages on BV.  `masks[tag]` is the ambiguity mask of every bf16 rounding point the chain went through."""

    def __init__(self, c_acc=None, c_ln=None, c_conv=None):
        self.ca = 4.0 * (C_ACC if c_acc is None else c_acc) * F32_UNIT
        self.cc = 4.0 * (C_CONV if c_conv is None else c_conv) * F32_UNIT
        self.cl = 4.0 * (C_LN if c_ln is None else c_ln) * F32_UNIT
        self.masks = {}

    def inp(self, t):
        t = t.detach().cpu().to(F64)
        return BV(t, torch.zeros_like(t))

    def mm(self, a, W, b, tag=None):
        W, b = W.to(F64), b.to(F64)
        Wa = W.abs().t()
        return BV(a.v @ W.t() + b, a.e @ Wa + self.ca * (a.v.abs() @ Wa + b.abs()))

    def conv(self, g, w, b, B, T, tlens, tag=None):
        """depthwise, kernel 31, zero outside [0, tlens[b]) of each utterance: y[t] = b + sum_k w[k] g[t + k - 15]"""
        w, b = w.to(F64), b.to(F64)
        gv, ge = g.v.reshape(B, T, D).clone(), g.e.reshape(B, T, D).clone()
        if tlens is not None:
            for i, n in enumerate(tlens):
                gv[i, n:] = 0
                ge[i, n:] = 0
        gv, ge = F.pad(gv, (0, 0, HALF, HALF)), F.pad(ge, (0, 0, HALF, HALF))
        v = b.expand(B, T, D).clone()
        mag, e = b.abs().expand(B, T, D).clone(), torch.zeros(B, T, D, dtype=F64)
        for k in range(KW):
            v += w[k] * gv[:, k:k + T]
            mag += w[k].abs() * gv[:, k:k + T].abs()
            e += w[k].abs() * ge[:, k:k + T]
        return BV(v.reshape(B * T, D), (e + self.cc * mag).reshape(B * T, D))

    def add(self, x, y, scale=1.0, tag=None):
        v = x.v + scale * y.v
        zero = (y.v == 0) & (y.e == 0)
        return BV(v, x.e + scale * y.e + torch.where(zero, 0.0, F32_UNIT * v.abs()))

    def ln(self, x, g, b, tag=None):
        g, b = g.to(F64), b.to(F64)
        mean = x.v.mean(-1, keepdim=True)
        sig = ((x.v - mean).square().mean(-1, keepdim=True) + EPS).sqrt()
        yh = (x.v - mean) / sig
        me, corr = x.e.mean(-1, keepdim=True), (yh.abs() * x.e).mean(-1, keepdim=True)
        second = 1.0 + 4.0 * x.e.amax(-1, keepdim=True) / sig
        spread = x.v.abs().mean(-1, keepdim=True) / sig
        e = g.abs() / sig * (x.e + me + yh.abs() * corr) * second + self.cl * (g.abs() * (yh.abs() + spread) + b.abs())
        return BV(yh * g + b, torch.where(g == 0, 0.0, e))  # (a zero gain: 0 * finite + b is b, no rounding)

    def swish(self, h, tag=None):
        v = h.v * torch.sigmoid(h.v)
        s = torch.sigmoid(h.v)
        lip = (s * (1.0 + h.v * (1.0 - s))).abs() + SWISH_CURV * h.e
        return BV(v, lip * h.e + (sigmoid_rel(h.v) + F32_UNIT) * v.abs())

    def glu(self, y, tag=None):
        a, gt = BV(y.v[:, :D], y.e[:, :D]), BV(y.v[:, D:], y.e[:, D:])
        s = torch.sigmoid(gt.v)
        es = (s * (1.0 - s) + SIGMOID_CURV * gt.e) * gt.e + sigmoid_rel(gt.v) * s
        v = a.v * s
        return BV(v, a.e * s + a.v.abs() * es + a.e * es + F32_UNIT * v.abs())

    def rb(self, x, tag):
        a = x.v.abs()
        ulp = bf16_ulp(a)
        s = a / ulp  # in [128, 256): exact, a power-of-two scaling
        dist = ((s - s.floor()) - 0.5).abs() * ulp
        amb = dist <= x.e
        r = torch.sign(x.v) * torch.round(s) * ulp  # (half to even, as the hardware conversion)
        self.masks[tag] = amb
        # ambiguous and 4 e < ulp: what the kernel rounds lies within 2 e < ulp / 2 of the boundary m, so it becomes one of the
        # two bf16 numbers either side of m, both ulp / 2 from it (just above a power of two the lower neighbour's spacing is
        # ulp / 2: within ulp / 2 of m nothing beyond the power of two itself is reached, so the two neighbours are still it)
        m = torch.sign(x.v) * (s.floor() + 0.5) * ulp
        near = amb & (4.0 * x.e < ulp)
        return BV(torch.where(near, m, r), torch.where(near, 0.5 * ulp, torch.where(amb, bf16_ulp(a + x.e) + x.e, 0.0)))


# ------------------------------------------------------------------------------------------ float32 restatement
class SimOps:
    """The same stages in float32 on the same operands: order = "torch" (torch's CPU kernels) or "chunk" (K in chunks of 32
    accumulated in sequence, the conv tap by tap, the LayerNorm sums in chunks of 32)."""

    def __init__(self, order):
        assert order in ("torch", "chunk"), order
        self.order = order

    def inp(self, t):
        return t.detach().cpu().to(F32)

    def mm(self, a, W, b, tag=None):
        if self.order == "torch":
            return a @ W.t() + b
        acc = torch.zeros(a.shape[0], W.shape[0])
        for k0 in range(0, W.shape[1], 32):
            acc = acc + a[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
        return acc + b

    def conv_input(self, g, B, T, tlens):
        g3 = g.reshape(B, T, D).clone()
        if tlens is not None:
            for i, n in enumerate(tlens):
                g3[i, n:] = 0
        return g3

    def conv_of(self, g3, w, b):
        """[B][T][D] already masked -> [B][T][D]"""
        T = g3.shape[1]
        if self.order == "torch":
            return F.conv1d(g3.transpose(1, 2), w.t().reshape(D, 1, KW), b, padding=HALF, groups=D).transpose(1, 2)
        gp = F.pad(g3, (0, 0, HALF, HALF))
        acc = b.expand(g3.shape).clone()
        for k in range(KW):
            acc = acc + w[k] * gp[:, k:k + T]
        return acc

    def conv(self, g, w, b, B, T, tlens, tag=None):
        return self.conv_of(self.conv_input(g, B, T, tlens), w, b).reshape(B * T, D)

    def add(self, x, y, scale=1.0, tag=None):
        return x + scale * y

    def ln(self, x, g, b, tag=None):
        if self.order == "torch":
            return ln(x, g, b)
        s = torch.zeros(x.shape[0], 1)
        for k0 in range(0, D, 32):
            s = s + x[:, k0:k0 + 32].sum(-1, keepdim=True)
        mean = s * (1.0 / D)
        dx = x - mean
        ss = torch.zeros(x.shape[0], 1)
        for k0 in range(0, D, 32):
            ss = ss + dx[:, k0:k0 + 32].square().sum(-1, keepdim=True)
        return dx * torch.rsqrt(ss * (1.0 / D) + EPS) * g + b

    def swish(self, h, tag=None):
        return h * torch.sigmoid(h)

    def glu(self, y, tag=None):
        return y[:, :D] * torch.sigmoid(y[:, D:])

    def rb(self, x, tag):
        return q(x)


# ------------------------------------------------------------------------------------------ the chains
def ffn(ops, x, xn, w1, b1, w2, b2, tag):
    h = ops.rb(ops.swish(ops.mm(xn, w1, b1, tag=tag + "_w1"), tag=tag), tag=tag + "_h")
    return ops.add(x, ops.mm(h, w2, b2, tag=tag + "_w2"), 0.5, tag=tag)


def qkv_of(ops, ly, x):
    return ops.mm(ops.rb(ops.ln(x, *ly.ln_mha, tag="ln_mha"), tag="ln_mha"), ly.wqkv, ly.bqkv, tag="wqkv")


def part_a(ops, ly, x, mid=None):
    """x after the macaron FFN, and q | k | v [rows][768] of norm_mha(x) - of `mid` (the device's own x) where given"""
    x = ffn(ops, x, ops.rb(ops.ln(x, *ly.ln_mac, tag="ln_mac"), tag="ln_mac"), ly.ffm_w1, ly.ffm_b1, ly.ffm_w2, ly.ffm_b2, "ffm")
    return x, qkv_of(ops, ly, x if mid is None else ops.inp(mid))


def part_c(ops, ly, x, ctx, mid=None):
    """x + linear_out(ctx), and GLU(pointwise_conv1(norm_conv(x))) - of `mid` where given"""
    x = ops.add(x, ops.mm(ctx, ly.wout, ly.bout, tag="wout"), tag="wout")
    xm = x if mid is None else ops.inp(mid)
    y = ops.mm(ops.rb(ops.ln(xm, *ly.ln_conv, tag="ln_conv"), tag="ln_conv"), ly.pw1, ly.pw1_b, tag="pw1")
    return x, ops.glu(y, tag="glu")


def part_d(ops, ly, x, glu, B, T, tlens=None):
    """conv module behind the GLU + feed-forward module + norm_final"""
    c = ops.rb(ops.swish(ops.conv(glu, ly.dw_w, ly.dw_b, B, T, tlens, tag="dw"), tag="dw"), tag="conv")
    x = ops.add(x, ops.mm(c, ly.pw2, ly.pw2_b, tag="pw2"), tag="pw2")
    x = ffn(ops, x, ops.rb(ops.ln(x, *ly.ln_ff, tag="ln_ff"), tag="ln_ff"), ly.ff_w1, ly.ff_b1, ly.ff_w2, ly.ff_b2, "ff")
    return ops.ln(x, *ly.ln_final, tag="ln_final")


def after_norm(ops, x, g, b):
    return ops.ln(x, g, b, tag="after_norm")


# ------------------------------------------------------------------------------------------ probes
class Probe:
    """One (probe, case): mode ("A", "C", "DF", "DA", "CDF", "CDA"), the layers with the probe's edits (l0: the C / D part, l1: the A part),
    the inputs, and run(ops, mid) -> {output name: value}; `mid` is the x the device (or the restatement) produced, the input
    of the stage shared behind it.  F32_OUT names the float32 outputs, the others are stored as bf16."""
    F32_OUT = ("x", "enc_out")

    def __init__(self, name, mode, B, T, tlens, ff, seed):
        self.name, self.mode, self.B, self.T, self.tlens, self.ff, self.seed = name, mode, B, T, tlens, ff, seed
        self.l0 = self.l1 = self.x0 = self.glu = self.ctx = self.ag = self.ab = None

    def run(self, ops, mid=None):
        x0 = ops.inp(self.x0)
        if self.mode == "A":
            x, qkv = part_a(ops, self.l1, x0, mid)
            return dict(x=x, **split_qkv(qkv))
        if self.mode in ("C", "ATTC"):
            x, glu = part_c(ops, self.l0, x0, ops.inp(self.ctx), mid)
            return dict(x=x, glu=glu)
        if self.mode in ("CDF", "CDA"):  # folded: the C part inside the launch, its GLU output rounded into the conv tile
            x1, glu = part_c(ops, self.l0, x0, ops.inp(self.ctx))
            xf = part_d(ops, self.l0, x1, ops.rb(glu, tag="glu"), self.B, self.T, self.tlens)
        else:
            xf = part_d(ops, self.l0, x0, ops.inp(self.glu), self.B, self.T, self.tlens)
        if self.mode in ("DF", "CDF"):
            out = after_norm(ops, xf, self.ag, self.ab)
            return dict(enc_out=out, enc_act=out)
        x, qkv = part_a(ops, self.l1, xf, mid)
        return dict(x=x, **split_qkv(qkv))


def split_qkv(qkv):
    cut = lambda t, i: t[:, i * D:(i + 1) * D]
    if isinstance(qkv, BV):
        return {n: BV(cut(qkv.v, i), cut(qkv.e, i)) for i, n in enumerate("qkv")}
    return {n: cut(qkv, i) for i, n in enumerate("qkv")}


def row_scale(B, T, tlens):
    """1 on valid frames, 3 on the frames at and past tlens[b]: those hold finite junk, not zeros, so that a read past the
    mask or across an utterance boundary shows"""
    s = torch.ones(B, T)
    if tlens is not None:
        for b, n in enumerate(tlens):
            s[b, n:] = 3.0
    return s.reshape(B * T, 1)


def clean_rows(scale, seed, amb_of):
    """Seeded rows x[i] = scale[i] * normal, only rows where amb_of(x) -> [rows][D] flags nothing (LN-clean: decided by the
    reference alone).  Draws 4x the rows needed and fails loudly if that does not suffice."""
    n = scale.shape[0]
    cand = rnd(4 * n, D, seed=seed)
    clean = {s: ~amb_of(cand * s).any(-1) for s in sorted(set(scale.reshape(-1).tolist()))}
    rows, j = [], 0
    for i in range(n):
        s = float(scale[i])
        while j < 4 * n and not bool(clean[s][j]):
            j += 1
        assert j < 4 * n, f"clean_rows: {i} of {n} LN-clean rows within 4x oversampling (seed {seed})"
        rows.append(cand[j] * s)
        j += 1
    return torch.stack(rows)


def _zero_ff(ly):
    ly.ff_w2, ly.ff_b2 = torch.zeros_like(ly.ff_w2), torch.zeros_like(ly.ff_b2)


def _zero_ffm(ly):
    ly.ffm_w2, ly.ffm_b2 = torch.zeros_like(ly.ffm_w2), torch.zeros_like(ly.ffm_b2)


def _after_conv_zero(ops, ly, x):
    """the D part up to the residual in front of norm_ff when the conv output is exactly zero: x + pw2 bias"""
    zero = ops.inp(torch.zeros(x.shape[0], D))
    return ops.add(ops.inp(x), ops.mm(zero, ly.pw2, ly.pw2_b, tag="pw2"), tag="pw2")


def _after_linear_out_zero(ops, ly, x):
    """the folded C part's residual when ctx = 0: x + linear_out bias"""
    zero = ops.inp(torch.zeros(x.shape[0], D))
    return ops.add(ops.inp(x), ops.mm(zero, ly.wout, ly.bout, tag="wout"), tag="wout")


PROBES = {  # name -> (mode, takes tlens)
    "a": ("A", False),           # block<A>: x behind the macaron FFN (LN-clean rows), q / k / v from the device's x
    "c": ("C", False),           # block<C>: x + linear_out(ctx) (no rounding point), glu from the device's x
    "df_conv": ("DF", True),     # block<D|FINAL>, ff_w2 = 0: the conv module through norm_final and after_norm
    "df_ffn": ("DF", True),      # block<D|FINAL>, glu = 0, dw_b = 0: the feed-forward module on rows LN-clean at norm_ff
    "da_conv": ("DA", True),     # block<D|A>, macaron w2 = 0: x shows the D part; q / k / v from the device's x
    "da_ffn": ("DA", True),
    "da_mac": ("DA", True),      # block<D|A>, D part exact (conv zero, ff_w2 = 0, norm_final gain 0): the macaron FFN
    # folded, ctx = 0 (x1 = x + linear_out bias, so that rows can be LN-clean behind it).  conv: pointwise_conv1's value half
    # is the identity and its gate is sigmoid(30) = 1 in float32, so the GLU output is q(norm_conv(x1)) exactly on LN-clean
    # rows - ALL rows, the halo frames are computed too; ffn: pointwise_conv1 = 0, so the conv output is exactly zero
    "cda_conv": ("CDA", True),
    "cda_ffn": ("CDA", True),
    "cdf_conv": ("CDF", True),
    "cdf_ffn": ("CDF", True),
    # block<ATT|C>, every utterance with ONE key: the softmax is 1 on key 0, so the context the attention phase hands to
    # linear_out is v[b][0] exactly, in every row; then as "c"
    "attc": ("ATTC", False),
}
_PROBES = {}


def probe_for(name, B, T, tlens, ff):
    """The one probe of a (name, case), shared and left unchanged by every test that uses it; seeds follow from the case."""
    key = (name, B, T, tuple(tlens) if tlens else None, ff)
    if key in _PROBES:
        return _PROBES[key]
    mode, masked_ok = PROBES[name]
    assert masked_ok or tlens is None, name
    seed = 200000 + 1000 * T + 10 * B + ff * 7 + 3 * list(PROBES).index(name)
    p = Probe(name, mode, B, T, tlens, ff, seed)
    scale = row_scale(B, T, tlens)

    def amb_at(tag, chain):
        def amb_of(x):
            ops = RefOps()
            chain(ops, x)
            return ops.masks[tag]
        return amb_of

    if mode == "A":
        p.l1 = Layer(seed, ff)
        p.x0 = clean_rows(scale, seed + 500, amb_at("ln_mac", lambda ops, x: ops.rb(ops.ln(ops.inp(x), *p.l1.ln_mac), tag="ln_mac")))
    elif mode == "C":
        p.l0 = Layer(seed, ff)
        p.x0, p.ctx = rnd(B * T, D, seed=seed + 500), q(rnd(B * T, D, seed=seed + 501))
    elif mode == "ATTC":
        p.l0 = Layer(seed, ff)
        p.x0 = rnd(B * T, D, seed=seed + 500)
        p.v0 = q(rnd(B, D, seed=seed + 501))  # v[b][0], all heads side by side
        p.ctx = p.v0.repeat_interleave(T, dim=0)
    elif mode in ("CDA", "CDF"):
        p.l0 = Layer(seed, ff)
        if mode == "CDA":
            p.l1 = Layer(seed + 200, ff)
            _zero_ffm(p.l1)
        else:
            p.ag, p.ab = 1 + 0.1 * rnd(D, seed=seed + 502), 0.1 * rnd(D, seed=seed + 503)
        p.ctx = torch.zeros(B * T, D)
        if name.endswith("_conv"):
            _zero_ff(p.l0)
            p.l0.pw1 = torch.cat([torch.eye(D), torch.zeros(D, D)])
            p.l0.pw1_b = torch.cat([torch.zeros(D), torch.full((D,), 30.0)])
            chain = lambda ops, x: ops.rb(ops.ln(_after_linear_out_zero(ops, p.l0, x), *p.l0.ln_conv), tag="ln_conv")
            p.x0 = clean_rows(scale, seed + 500, amb_at("ln_conv", chain))
        else:
            p.l0.pw1, p.l0.dw_b = torch.zeros(2 * D, D), torch.zeros(D)
            p.l0.pw1_b = torch.cat([torch.zeros(D), p.l0.pw1_b[D:]])

            def chain(ops, x):
                zero = ops.inp(torch.zeros(x.shape[0], D))
                x2 = ops.add(_after_linear_out_zero(ops, p.l0, x), ops.mm(zero, p.l0.pw2, p.l0.pw2_b, tag="pw2"), tag="pw2")
                return ops.rb(ops.ln(x2, *p.l0.ln_ff), tag="ln_ff")
            p.x0 = clean_rows(scale, seed + 500, amb_at("ln_ff", chain))
    else:
        p.l0 = Layer(seed, ff)
        if mode == "DA":
            p.l1 = Layer(seed + 200, ff)
        else:
            p.ag, p.ab = 1 + 0.1 * rnd(D, seed=seed + 502), 0.1 * rnd(D, seed=seed + 503)
        junk = q(rnd(B * T, D, seed=seed + 501)) * (scale == 3.0)  # only past tlens; 3 * bf16 is not bf16, so round again
        if name.endswith("_conv"):
            _zero_ff(p.l0)
            if mode == "DA":
                _zero_ffm(p.l1)
            p.x0 = rnd(B * T, D, seed=seed + 500) * scale
            p.glu = q(q(rnd(B * T, D, seed=seed + 501)) * scale)
        else:
            p.l0.dw_b = torch.zeros(D)
            p.glu = q(junk * 3.0)
            if name.endswith("_ffn"):
                if mode == "DA":
                    _zero_ffm(p.l1)
                chain = lambda ops, x: ops.rb(ops.ln(_after_conv_zero(ops, p.l0, x), *p.l0.ln_ff), tag="ln_ff")
                p.x0 = clean_rows(scale, seed + 500, amb_at("ln_ff", chain))
            else:
                # norm_final always stands between the D part and the A part, and a float32 LayerNorm is never exact: behind
                # it and norm_macaron's first-order rule one row in ten is LN-clean.  With a ZERO norm_final gain the D part
                # hands over its bias vector, exactly (0 * finite + b), in every row: the macaron module of every row and
                # tile is held to the one LN-clean input.  This probe therefore checks ONE row's arithmetic, repeated in every
                # row and tile position: an error that depends on the row's content or mixes rows (a wrong LDS row, a wave or
                # tile mix-up) does not show here - the macaron module on distinct rows is block<A>'s probe "a" to show, the
                # row -> output mapping of block<D|A> da_conv's and da_ffn's.
                _zero_ff(p.l0)
                chain = lambda ops, x: ops.rb(ops.ln(ops.inp(x), *p.l1.ln_mac), tag="ln_mac")
                p.l0.ln_final = (torch.zeros(D), clean_rows(torch.ones(1, 1), seed + 504, amb_at("ln_mac", chain))[0])
                p.x0 = rnd(B * T, D, seed=seed + 500) * scale
    _PROBES[key] = p
    return p


# ------------------------------------------------------------------------------------------ the budget
def budget(ref, f32):
    return ref.e if f32 else ref.e + U_BF16 * ref.v.abs()


def worst(got, ref, f32):
    """(err / budget of the worst element, (row, channel)); a zero budget demands equality, a NaN counts as inf"""
    got = got.detach().cpu().to(F64).reshape(ref.v.shape)
    err, bud = (got - ref.v).abs(), budget(ref, f32)
    ratio = torch.where(bud > 0, err / bud.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    flat = int(ratio.argmax())
    return float(ratio.reshape(-1)[flat]), (flat // ref.v.shape[1], flat % ref.v.shape[1])


def assert_in_budget(got, ref, probe, out, what):
    """Holds every element of got [B * T][256] to the budget of output `out` of the probe; returns the worst err / budget."""
    f32 = out in Probe.F32_OUT
    r, (row, c) = worst(got, ref, f32)
    g = float(got.detach().cpu().to(F64).reshape(ref.v.shape)[row, c])
    assert r <= 1.0, (f"{what} probe {probe.name} {out}: err / budget = {r:.3g} at utterance {row // probe.T}, frame {row % probe.T}, "
                      f"channel {c}: got {g!r}, reference {float(ref.v[row, c])!r}, budget {float(budget(ref, f32)[row, c]):.3e} "
                      f"(bound in front of the store {float(ref.e[row, c]):.3e})")
    return r
