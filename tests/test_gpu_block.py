"""GPU parity tests of the fused per-block path (csrc/block.hip, csrc/attention2.hip), through the C ABI.

Every fused kernel is checked against a torch fp32 restatement of the reference operators it replaces
(conformer/encoder_layer.py:79-179, conformer/convolution.py:56-79, attention.py:391-459), computed FROM THE
SAME bf16-ROUNDED operands and with the same bf16 rounding points the unfused bf16 path has (LayerNorm output,
FFN hidden activation, GLU output, depthwise-conv output, q / k / v), so what is checked is the kernel, not the
rounding.  Tolerances: 4e-3 of the output scale for the f32 residual stream (same class as
test_ffn_fused_bf16), 2e-2 for bf16 outputs (one bf16 ulp is 0.8 %).  Then the whole encoder: fused vs the
per-operator launch sequence on the reference goldens.  The attention phase of block<ATT|C> is also observed directly
(test_block_att_c_attention_parity): per element against the float64 reference and budget of tests/attention_ref.py.
The row-local phases (LayerNorm, the two FFNs, linear_out, pointwise_conv1 + GLU, the depthwise conv + Swish,
pointwise_conv2, the q / k / v projections) are each observed on their own as well (test_block_*_parity): per element against
the float64 reference of tests/block_ref.py, whose budget follows the roundings and is zero behind an unambiguous one.
"""
import math

import pytest
import torch

from espnet_amd import lib as L
from espnet_amd.asr.encoder.conformer_encoder import pack_k_units, pack_w1, pack_w2
from oracle import conformer as oc
from tests import attention_ref as ar
from tests import block_ref as br
from tests.block_ref import Layer, group, ln, q, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, H, G = 256, 4, L.EM_BLOCK_PARAM_GROUP


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


_KEEP = []


def dev(t):
    t = t.contiguous().cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def assert_close(got, ref, tol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def tpad(T):
    return (T + 255) // 256 * 256


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("T,klens", [(49, [49, 20]), (128, [128]), (249, [249, 130, 1]), (256, [256, 255]),
                                     (300, [300, 257]), (700, [700, 513])])
def test_relpos_attention2(lib, T, klens):
    """em_relpos_attention2_bf16 against the literal rel_shift formulation (the same reference as
    test_relpos_attention), on per-head operand layouts; T > 256 exercises the super-tile loop."""
    B, dk = len(klens), 64
    d = H * dk
    Tp = tpad(T)
    qq = q(rnd(B, T, H, dk, seed=26))
    kk = q(rnd(B, T, H, dk, seed=27))
    vv = q(rnd(B, T, H, dk, seed=28))
    Lb = 3  # the table holds linear_pos of several blocks side by side (ldp = Lb * d); use the middle one
    pall = q(rnd(2 * T - 1, Lb * d, seed=29))
    p = pall[:, d:2 * d]
    u, v = rnd(H, dk, seed=30, scale=0.3), rnd(H, dk, seed=31, scale=0.3)
    q_u = q(qq + u).transpose(1, 2)
    q_v = q(qq + v).transpose(1, 2)
    pp = p.reshape(1, 2 * T - 1, H, dk).transpose(1, 2)
    ac = q_u @ kk.transpose(1, 2).transpose(-2, -1)
    bd = oc.rel_shift(q_v @ pp.transpose(-2, -1))
    scores = (ac + bd) / math.sqrt(dk)
    mask = oc.make_pad_mask(torch.tensor(klens), T)[:, None, None, :]
    attn = torch.softmax(scores.masked_fill(mask, torch.finfo(torch.float32).min), -1).masked_fill(mask, 0.0)
    ref = (attn @ vv.transpose(1, 2)).transpose(1, 2).reshape(B, T, d)

    qh = torch.full((B, H, Tp, dk), float("nan"), dtype=BF)  # rows >= T: never read into a stored output
    kh = torch.full((B, H, Tp, dk), float("nan"), dtype=BF)  # keys >= klen: masked by select, never by arithmetic
    vt = torch.zeros(B, H, dk, Tp, dtype=BF)                 # V^T padding must be finite (0 * x)
    qh[:, :, :T] = qq.transpose(1, 2).to(BF)
    kh[:, :, :T] = kk.transpose(1, 2).to(BF)
    vt[:, :, :, :T] = vv.permute(0, 2, 3, 1).to(BF)
    ctx = torch.zeros(B, T, d, dtype=BF, device="cuda")
    palld = dev(pall.to(BF))
    L.check(lib.em_relpos_attention2_bf16(L.ptr(dev(qh)), L.ptr(dev(kh)), L.ptr(dev(vt)),
                                          palld.data_ptr() + d * 2, Lb * d, L.ptr(dev(u)), L.ptr(dev(v)),
                                          L.ptr(dev(torch.tensor(klens, dtype=torch.int32))), B, T, Tp, H,
                                          L.ptr(ctx), L.current_stream_ptr()), "attention2")
    assert_close(ctx, ref, 2e-2, f"attention2 T={T}")


# ------------------------------------------------------------------------------------------ block kernels
def block_args(B, T, ff, **ptrs):
    a = L.EmBlockArgs(B=B, T=T, Tpad=tpad(T), d=D, ff=ff, kernel=31, eps=1e-12)
    for k, v in ptrs.items():
        setattr(a, k, v.data_ptr() if v is not None else None)
    return a


def split_heads(buf, B, T):
    """[B][H][Tpad][64] -> [B*T][256]"""
    return buf[:, :, :T].permute(0, 2, 1, 3).reshape(B * T, D)


def _k_frag_index(Tp):
    """key index of K'[jt][n][ks][lane][e] (EmBlockArgs.kv_frag): [Tp/64, 4, 1, 64, 1] broadcastable."""
    jt = torch.arange(Tp // 64).reshape(-1, 1, 1, 1, 1)
    n = torch.arange(4).reshape(1, -1, 1, 1, 1)
    lane = torch.arange(64).reshape(1, 1, 1, -1, 1)
    lr = lane % 16
    return 64 * jt + 32 * (n // 2) + 8 * (lr // 4) + 4 * (n % 2) + (lr % 4)


def k_to_frag(kh):
    """[B][H][Tp][64] row-major -> the fragment-major K of EmBlockArgs.kv_frag (same shape, other order)."""
    B, Hh, Tp, _ = kh.shape
    key = _k_frag_index(Tp).expand(Tp // 64, 4, 2, 64, 8)
    ks = torch.arange(2).reshape(1, 1, -1, 1, 1)
    lg = (torch.arange(64) // 16).reshape(1, 1, 1, -1, 1)
    col = (32 * ks + 8 * lg + torch.arange(8).reshape(1, 1, 1, 1, -1)).expand(Tp // 64, 4, 2, 64, 8)
    return kh[:, :, key, col].reshape(B, Hh, Tp, 64)


def k_from_frag(kf):
    B, Hh, Tp, _ = kf.shape
    key = _k_frag_index(Tp).expand(Tp // 64, 4, 2, 64, 8)
    ks = torch.arange(2).reshape(1, 1, -1, 1, 1)
    lg = (torch.arange(64) // 16).reshape(1, 1, 1, -1, 1)
    col = (32 * ks + 8 * lg + torch.arange(8).reshape(1, 1, 1, 1, -1)).expand(Tp // 64, 4, 2, 64, 8)
    out = torch.zeros_like(kf)
    out[:, :, key, col] = kf.reshape(B, Hh, Tp // 64, 4, 2, 64, 8)
    return out


def _vt_frag_index(Tp):
    jt = torch.arange(Tp // 64).reshape(-1, 1, 1, 1, 1)
    f = torch.arange(4).reshape(1, -1, 1, 1, 1)
    jp = torch.arange(2).reshape(1, 1, -1, 1, 1)
    lane = torch.arange(64).reshape(1, 1, 1, -1, 1)
    e = torch.arange(8).reshape(1, 1, 1, 1, -1)
    row = (16 * f + lane % 16).expand(Tp // 64, 4, 2, 64, 8)
    key = (64 * jt + 32 * jp + 8 * (lane // 16) + e).expand(Tp // 64, 4, 2, 64, 8)
    return row, key


def vt_to_frag(vt):
    """[B][H][64][Tp] (V transposed, row-major) -> the fragment-major V^T of EmBlockArgs.kv_frag."""
    B, Hh, _, Tp = vt.shape
    row, key = _vt_frag_index(Tp)
    return vt[:, :, row, key].reshape(B, Hh, 64, Tp)


def vt_from_frag(vf):
    B, Hh, _, Tp = vf.shape
    row, key = _vt_frag_index(Tp)
    out = torch.zeros_like(vf)
    out[:, :, row, key] = vf.reshape(B, Hh, Tp // 64, 4, 2, 64, 8)
    return out


SHAPES = [(2, 249, 1024), (3, 70, 256), (1, 32, 1024), (2, 31, 64), (1, 40, 192), (2, 100, 576)]  # ff / 64 even, 1, odd


@pytest.mark.parametrize("B,T,ff", SHAPES)
@pytest.mark.parametrize("kv_frag", [0, 1])
def test_block_a(lib, B, T, ff, kv_frag):
    """kv_frag = 1 (round 6): K and V^T written fragment-major for block<ATT|C>; unpacked here and held to the same reference."""
    ly = Layer(100, ff)
    x0 = rnd(B * T, D, seed=1)
    x_ref, qkv_ref = ly.part_a(x0)
    Tp = tpad(T)
    xd = dev(x0.clone())
    qh, kh = (torch.zeros(B, H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
    vt = torch.zeros(B, H, 64, Tp, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=xd, qh=qh, kh=kh, vt=vt, ffm_w1=dev(pack_w1(ly.ffm_w1).to(BF)), ffm_w2=dev(pack_w2(ly.ffm_w2).to(BF)),
                   wqkv=dev(pack_k_units(ly.wqkv).to(BF)), params=dev(torch.cat(ly.a_groups())))
    a.kv_frag = kv_frag
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_A, a, L.current_stream_ptr()), "block<A>")
    if kv_frag:
        kh, vt = k_from_frag(kh.cpu()), vt_from_frag(vt.cpu())
    assert_close(xd, x_ref, 4e-3, "block<A> x")
    assert_close(split_heads(qh, B, T), qkv_ref[:, :D], 2e-2, "block<A> q")
    assert_close(split_heads(kh, B, T), qkv_ref[:, D:2 * D], 2e-2, "block<A> k")
    v_got = vt[:, :, :, :T].permute(0, 3, 1, 2).reshape(B * T, D)
    assert_close(v_got, qkv_ref[:, 2 * D:], 2e-2, "block<A> v")
    assert torch.isfinite(vt.float()).all()


@pytest.mark.parametrize("B,T,ff", SHAPES)
def test_block_c(lib, B, T, ff):
    ly = Layer(200, ff)
    x0, ctx = rnd(B * T, D, seed=2), q(rnd(B * T, D, seed=3))
    x_ref, glu_ref = ly.part_c(x0, ctx)
    xd = dev(x0.clone())
    glu = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=xd, ctx=dev(ctx.to(BF)), glu=glu, wout=dev(pack_k_units(ly.wout).to(BF)),
                   pw1f=dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)), params=dev(ly.c_group()))
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_C, a, L.current_stream_ptr()), "block<C>")
    assert_close(xd, x_ref, 4e-3, "block<C> x")
    assert_close(glu, glu_ref, 2e-2, "block<C> glu")


def _attention_inputs(B, T, klens, seed):
    """Per-head operands of the attention as block<A> writes them, and the torch restatement of the context."""
    dk = 64
    qq = q(rnd(B, T, H, dk, seed=seed))
    kk = q(rnd(B, T, H, dk, seed=seed + 1))
    vv = q(rnd(B, T, H, dk, seed=seed + 2))
    Lb = 3  # linear_pos of several blocks side by side (ldp = Lb * d); the middle one is this block's
    pall = q(rnd(2 * T - 1, Lb * D, seed=seed + 3))
    p = pall[:, D:2 * D]
    u, v = rnd(H, dk, seed=seed + 4, scale=0.3), rnd(H, dk, seed=seed + 5, scale=0.3)
    q_u = q((qq + u) * 0.125).transpose(1, 2)  # (1 / sqrt(d_k) rides in the operands: a power of two, exact)
    q_v = q((qq + v) * 0.125).transpose(1, 2)
    pp = p.reshape(1, 2 * T - 1, H, dk).transpose(1, 2)
    scores = q_u @ kk.transpose(1, 2).transpose(-2, -1) + oc.rel_shift(q_v @ pp.transpose(-2, -1))
    mask = oc.make_pad_mask(torch.tensor(klens), T)[:, None, None, :]
    attn = torch.softmax(scores.masked_fill(mask, torch.finfo(torch.float32).min), -1).masked_fill(mask, 0.0)
    ctx = (attn @ vv.transpose(1, 2)).transpose(1, 2).reshape(B * T, D)
    Tp = tpad(T)
    qh = torch.full((B, H, Tp, dk), float("nan"), dtype=BF)  # rows >= T: never read into a stored output
    kh = torch.full((B, H, Tp, dk), float("nan"), dtype=BF)  # keys >= klen: masked by select, never by arithmetic
    vt = torch.zeros(B, H, dk, Tp, dtype=BF)                 # V^T padding must be finite (0 * x)
    qh[:, :, :T] = qq.transpose(1, 2).to(BF)
    kh[:, :, :T] = kk.transpose(1, 2).to(BF)
    vt[:, :, :, :T] = vv.permute(0, 2, 3, 1).to(BF)
    return dict(qh=qh, kh=kh, vt=vt, pall=pall, u=u, v=v, ctx=ctx, Lb=Lb)


def packed_pos(lib, palld, T, Lb):
    """em_relpos_pack_pos_bf16 of a [2T-1][Lb * 256] table, checked against its definition (include/espnet_amd.h)."""
    npg = lib.em_relpos_pos_fragments(T)
    assert npg == 2 * ((T + 31) // 32) + 4 * ((T + 63) // 64) + 2
    out = torch.full((Lb, 4, npg, 2, 64, 8), float("nan"), dtype=BF, device="cuda")
    L.check(lib.em_relpos_pack_pos_bf16(L.ptr(palld), Lb * D, T, Lb, L.ptr(out), L.current_stream_ptr()), "pack_pos")
    gx = (T + 31) // 32
    g = torch.arange(npg).reshape(-1, 1, 1, 1)
    lane = torch.arange(64).reshape(1, 1, -1, 1)
    row = (16 * g + T - 32 * gx - 32 + lane % 16).clamp(0, 2 * T - 2).expand(npg, 2, 64, 8)
    col = (32 * torch.arange(2).reshape(1, -1, 1, 1) + 8 * (lane // 16) + torch.arange(8).reshape(1, 1, 1, -1)).expand(npg, 2, 64, 8)
    p = palld.cpu()
    for l in range(Lb):
        for h in range(4):
            assert torch.equal(out[l, h].cpu(), p[row, l * D + h * 64 + col]), (l, h)
    _KEEP.append(out)
    return out, npg


ATT_SHAPES = [(2, 249, [249, 130]), (3, 70, [70, 1, 33]), (1, 32, [32]), (2, 31, [31, 7]), (1, 128, [128]), (2, 256, [256, 255]),
              (1, 300, [257]), (2, 700, [700, 513]), (9, 40, [40, 39, 38, 37, 3, 2, 1, 40, 17]), (16, 65, list(range(50, 66)))]


@pytest.mark.parametrize("B,T,klens", ATT_SHAPES)
def test_block_att_c(lib, B, T, klens):
    """Round 6, block<ATT|C>: relative-position attention of a workgroup's 32 queries + linear_out + residual + norm_conv +
    pointwise_conv1 + GLU in ONE launch, against the torch restatement of attention.py:416-459 followed by part_c, and
    against the two-launch form (em_relpos_attention2_bf16 + block<C>) on the same operands.  Shapes: key counts that end
    inside / on a 64-key tile, odd and even tile counts, more than 256 keys, utterances of one frame, batches that do and
    do not fill groups of 8 utterances (the workgroup -> (utterance, query block) map differs)."""
    ly = Layer(1100, 256)
    at = _attention_inputs(B, T, klens, 40)
    x0 = rnd(B * T, D, seed=2)
    x_ref, glu_ref = ly.part_c(x0, q(at["ctx"]))
    Tp = tpad(T)
    palld = dev(at["pall"].to(BF))
    qh, kh, vt = dev(at["qh"]), dev(at["kh"]), dev(at["vt"])
    khf, vtf = dev(k_to_frag(at["kh"])), dev(vt_to_frag(at["vt"]))  # the layouts the A part writes with kv_frag = 1
    ppk, npg = packed_pos(lib, palld, T, at["Lb"])
    u, v, kl = dev(at["u"]), dev(at["v"]), dev(torch.tensor(klens, dtype=torch.int32))
    wout, pw1f, par = dev(pack_k_units(ly.wout).to(BF)), dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)), dev(ly.c_group())
    xd = dev(x0.clone())
    glu = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a = block_args(B, T, 256, x=xd, glu=glu, qh=qh, kh=khf, vt=vtf, wout=wout, pw1f=pw1f, params=par, pos_u=u, pos_v=v, klens=kl)
    a.pos, a.ldp, a.kv_frag = ppk.data_ptr() + 4 * npg * 2048, npg, 1  # (the middle block of the table)
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_ATT | L.EM_BLOCK_C, a, L.current_stream_ptr()), "block<ATT|C>")
    # rows of an utterance past its key count attend over the valid keys like any other row (the reference masks keys only)
    assert_close(xd, x_ref, 4e-3, "block<ATT|C> x")
    assert_close(glu, glu_ref, 2e-2, "block<ATT|C> glu")
    # the two-launch form on the same operands: same rounding points, so the two agree far inside the tolerance above
    ctx2 = torch.zeros(B * T, D, dtype=BF, device="cuda")
    L.check(lib.em_relpos_attention2_bf16(L.ptr(qh), L.ptr(kh), L.ptr(vt), palld.data_ptr() + D * 2, at["Lb"] * D, L.ptr(u),
                                          L.ptr(v), L.ptr(kl), B, T, Tp, H, L.ptr(ctx2), L.current_stream_ptr()), "attention2")
    x2 = dev(x0.clone())
    glu2 = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a2 = block_args(B, T, 256, x=x2, ctx=ctx2, glu=glu2, wout=wout, pw1f=pw1f, params=par)
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_C, a2, L.current_stream_ptr()), "block<C>")
    assert_close(xd, x2, 1e-3, "block<ATT|C> vs attention2 + block<C>: x")
    assert_close(glu, glu2, 1.6e-2, "block<ATT|C> vs attention2 + block<C>: glu")  # (a bf16 ulp where a rounding falls the other way)
    # missing operands are refused
    a.klens = None
    assert lib.em_conformer_block_fused(L.EM_BLOCK_ATT | L.EM_BLOCK_C, a, L.current_stream_ptr()) == L.EM_ERR_BAD_ARG


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T,klens,h", ar.FUSED_CASES, ids=[f"T{T}x{len(kl)}" for T, kl, _ in ar.FUSED_CASES])
def test_block_att_c_attention_parity(lib, T, klens, h, regime):
    """The attention phase of block<ATT|C> observed directly.  With linear_out = identity, no bias and a zero residual the x
    the launch writes back is the attention context itself, bit for bit as the kernel rounds it to bf16 in front of linear_out
    (the products with 1 and the sums with 0 are exact in f32), so it is held per element to the float64 reference and the
    bf16 budget of tests/attention_ref.py (3 u A + f (1 + S) A, exactly zero where no valid key reaches a channel) on the
    tile-edge cases of tests/test_gpu_attention_parity.py, on all rows of every utterance.  (klens[b] > T is left out; glu
    is not asserted here: test_block_att_c holds it.)
    Measured on an MI355X, the worst err / budget over these cases: 0.673 (T = 40, nine utterances, sharp; exactly 0 at T = 1)."""
    assert h == H
    B = len(klens)
    case = ar.case_for(T, klens, H, regime)
    ly = Layer(1100, 256)
    ly.wout, ly.bout = torch.eye(D), torch.zeros(D)
    Tp = tpad(T)
    qh = torch.full((B, H, Tp, 64), float("nan"), dtype=BF)  # rows >= T: never read into a stored output
    kh = torch.full((B, H, Tp, 64), float("nan"), dtype=BF)  # keys >= klen: masked by select, never by arithmetic
    vt = torch.zeros(B, H, 64, Tp, dtype=BF)                 # V^T padding must be finite (0 * x)
    qh[:, :, :T] = case.q.transpose(1, 2).to(BF)
    kh[:, :, :T] = case.k.transpose(1, 2).to(BF)
    vt[:, :, :, :T] = case.v.permute(0, 2, 3, 1).to(BF)
    palld = dev(case.pall.to(BF))
    ppk, npg = packed_pos(lib, palld, T, ar.LB)
    xd = dev(torch.zeros(B * T, D))
    glu = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a = block_args(B, T, 256, x=xd, glu=glu, qh=dev(qh), kh=dev(k_to_frag(kh)), vt=dev(vt_to_frag(vt)),
                   wout=dev(pack_k_units(ly.wout).to(BF)), pw1f=dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)), params=dev(ly.c_group()),
                   pos_u=dev(case.u), pos_v=dev(case.vb), klens=dev(torch.tensor(klens, dtype=torch.int32)))
    a.pos, a.ldp, a.kv_frag = ppk.data_ptr() + 4 * npg * 2048, npg, 1  # (the middle block of the table)
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_ATT | L.EM_BLOCK_C, a, L.current_stream_ptr()), "block<ATT|C>")
    r = ar.assert_in_budget(xd.reshape(B, T, D), ar.ref_rel(case, "scaled"), BF, f"block<ATT|C> attention T={T} klens={klens} {regime}")
    print(f"PARITY block<ATT|C> T={T} B={B} {regime}: err / budget {r:.3f}")


def test_block_att_c_repeatable_at_bench_shape(lib):
    """block<ATT|C> at B = 32 x T = 249 twenty times back to back: bit-identical outputs (operands are requested a tile ahead on
    counted waits; a read that raced its request would show up as run-to-run differences)."""
    B, T = 32, 249
    ly = Layer(1200, 256)
    at = _attention_inputs(B, T, [T - (b % 5) * 11 for b in range(B)], 60)
    x0 = rnd(B * T, D, seed=3)
    palld = dev(at["pall"].to(BF))
    x0d, xd = dev(x0), dev(x0.clone())
    glu = torch.zeros(B * T, D, dtype=BF, device="cuda")
    ppk, npg = packed_pos(lib, palld, T, at["Lb"])
    a = block_args(B, T, 256, x=xd, glu=glu, qh=dev(at["qh"]), kh=dev(k_to_frag(at["kh"])), vt=dev(vt_to_frag(at["vt"])),
                   wout=dev(pack_k_units(ly.wout).to(BF)),
                   pw1f=dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)), params=dev(ly.c_group()), pos_u=dev(at["u"]), pos_v=dev(at["v"]),
                   klens=dev(torch.tensor([T - (b % 5) * 11 for b in range(B)], dtype=torch.int32)))
    a.pos, a.ldp, a.kv_frag = ppk.data_ptr() + 4 * npg * 2048, npg, 1
    first = None
    for it in range(20):
        xd.copy_(x0d)
        L.check(lib.em_conformer_block_fused(L.EM_BLOCK_ATT | L.EM_BLOCK_C, a, L.current_stream_ptr()), "block<ATT|C>")
        got = (xd.clone(), glu.clone())
        if first is None:
            first = got
            x_ref, glu_ref = ly.part_c(x0, q(at["ctx"]))
            assert_close(xd, x_ref, 4e-3, "block<ATT|C> x at B=32")
            assert_close(glu, glu_ref, 2e-2, "block<ATT|C> glu at B=32")
        else:
            for g0, g1 in zip(first, got):
                assert torch.equal(g0, g1), f"run {it} differs from run 0"


@pytest.mark.parametrize("B,T,ff", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_block_d_final(lib, B, T, ff, masked):
    ly = Layer(300, ff)
    x0, glu = rnd(B * T, D, seed=4), q(rnd(B * T, D, seed=5))
    tl = [max(1, T - 7 * b - 3) for b in range(B)] if masked else None
    ag, ab = 1 + 0.1 * rnd(D, seed=6), 0.1 * rnd(D, seed=7)
    xf = ly.part_d(x0, glu, B, T, tl)
    ref = ln(xf, ag, ab)
    xd = dev(x0.clone())
    out = torch.zeros(B * T, D, dtype=torch.float32, device="cuda")
    act = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=xd, glu=dev(glu.to(BF)), enc_out=out, enc_act=act, pw2=dev(pack_k_units(ly.pw2).to(BF)),
                   ff_w1=dev(pack_w1(ly.ff_w1).to(BF)), ff_w2=dev(pack_w2(ly.ff_w2).to(BF)), dw_w=dev(ly.dw_w), dw_b=dev(ly.dw_b),
                   tlens=dev(torch.tensor(tl, dtype=torch.int32)) if masked else None,
                   params=dev(torch.cat(ly.d_groups() + [group(ag, ab), torch.zeros(G)])))
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_D | L.EM_BLOCK_FINAL, a, L.current_stream_ptr()), "block<D|F>")
    assert_close(out, ref, 4e-3, "block<D|FINAL> enc_out")
    assert_close(act, ref, 2e-2, "block<D|FINAL> enc_act")


@pytest.mark.parametrize("B,T,ff", SHAPES)
def test_block_da(lib, B, T, ff):
    l0, l1 = Layer(400, ff), Layer(500, ff)
    x0, glu = rnd(B * T, D, seed=8), q(rnd(B * T, D, seed=9))
    x_ref, qkv_ref = l1.part_a(l0.part_d(x0, glu, B, T))
    Tp = tpad(T)
    xd = dev(x0.clone())
    qh, kh = (torch.zeros(B, H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
    vt = torch.zeros(B, H, 64, Tp, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=xd, glu=dev(glu.to(BF)), qh=qh, kh=kh, vt=vt, pw2=dev(pack_k_units(l0.pw2).to(BF)),
                   ff_w1=dev(pack_w1(l0.ff_w1).to(BF)), ff_w2=dev(pack_w2(l0.ff_w2).to(BF)), dw_w=dev(l0.dw_w), dw_b=dev(l0.dw_b),
                   ffm_w1=dev(pack_w1(l1.ffm_w1).to(BF)), ffm_w2=dev(pack_w2(l1.ffm_w2).to(BF)), wqkv=dev(pack_k_units(l1.wqkv).to(BF)),
                   params=dev(torch.cat(l0.d_groups() + l1.a_groups())))
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_D | L.EM_BLOCK_A, a, L.current_stream_ptr()), "block<D|A>")
    assert_close(xd, x_ref, 6e-3, "block<D|A> x")
    assert_close(split_heads(qh, B, T), qkv_ref[:, :D], 3e-2, "block<D|A> q")
    assert_close(split_heads(kh, B, T), qkv_ref[:, D:2 * D], 3e-2, "block<D|A> k")
    assert_close(vt[:, :, :, :T].permute(0, 3, 1, 2).reshape(B * T, D), qkv_ref[:, 2 * D:], 3e-2, "block<D|A> v")


@pytest.mark.parametrize("B,T,ff", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_block_cda_folded(lib, B, T, ff, masked):
    """Round 4: block<C|D|A> - the C part computed inside the launch that consumes it, for the workgroup's 32 frames and
    the depthwise conv's halo either side; the residual stream goes x -> x_out.  Same restatement as the three-launch
    sequence (part_c -> part_d -> next layer's part_a), utterance boundaries and a masked tail (tlens) included."""
    l0, l1 = Layer(800, ff), Layer(900, ff)
    x0, ctx = rnd(B * T, D, seed=12), q(rnd(B * T, D, seed=13))
    tl = [max(1, T - 7 * b - 3) for b in range(B)] if masked else None
    xc, glu_ref = l0.part_c(x0, ctx)
    x_ref, qkv_ref = l1.part_a(l0.part_d(xc, glu_ref, B, T, tl))
    Tp = tpad(T)
    xd, xo = dev(x0.clone()), torch.full((B * T, D), float("nan"), device="cuda")
    qh, kh = (torch.zeros(B, H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
    vt = torch.zeros(B, H, 64, Tp, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=xd, x_out=xo, ctx=dev(ctx.to(BF)), qh=qh, kh=kh, vt=vt,
                   wout=dev(pack_k_units(l0.wout).to(BF)), pw1f=dev(pack_k_units(l0.pw1[l0.perm()]).to(BF)),
                   params_c=dev(l0.c_group()), pw2=dev(pack_k_units(l0.pw2).to(BF)),
                   ff_w1=dev(pack_w1(l0.ff_w1).to(BF)), ff_w2=dev(pack_w2(l0.ff_w2).to(BF)), dw_w=dev(l0.dw_w), dw_b=dev(l0.dw_b),
                   ffm_w1=dev(pack_w1(l1.ffm_w1).to(BF)), ffm_w2=dev(pack_w2(l1.ffm_w2).to(BF)), wqkv=dev(pack_k_units(l1.wqkv).to(BF)),
                   tlens=dev(torch.tensor(tl, dtype=torch.int32)) if masked else None,
                   params=dev(torch.cat(l0.d_groups() + l1.a_groups())))
    mode = L.EM_BLOCK_C | L.EM_BLOCK_D | L.EM_BLOCK_A
    L.check(lib.em_conformer_block_fused(mode, a, L.current_stream_ptr()), "block<C|D|A>")
    assert torch.equal(xd.cpu(), x0), "the folded kernel must not write its input residual"
    assert_close(xo, x_ref, 8e-3, "block<C|D|A> x_out")
    assert_close(split_heads(qh, B, T), qkv_ref[:, :D], 3e-2, "block<C|D|A> q")
    assert_close(split_heads(kh, B, T), qkv_ref[:, D:2 * D], 3e-2, "block<C|D|A> k")
    assert_close(vt[:, :, :, :T].permute(0, 3, 1, 2).reshape(B * T, D), qkv_ref[:, 2 * D:], 3e-2, "block<C|D|A> v")
    # in place is refused: a neighbour workgroup reads these rows as its halo
    a.x_out = a.x
    assert lib.em_conformer_block_fused(mode, a, L.current_stream_ptr()) == L.EM_ERR_BAD_ARG


@pytest.mark.parametrize("B,T,ff", [(2, 249, 1024), (3, 70, 256), (2, 31, 64)])
def test_block_cd_final_folded(lib, B, T, ff):
    ly = Layer(1000, ff)
    x0, ctx = rnd(B * T, D, seed=14), q(rnd(B * T, D, seed=15))
    ag, ab = 1 + 0.1 * rnd(D, seed=16), 0.1 * rnd(D, seed=17)
    ref = ln(ly.part_d(*ly.part_c(x0, ctx), B, T), ag, ab)
    out = torch.zeros(B * T, D, dtype=torch.float32, device="cuda")
    act = torch.zeros(B * T, D, dtype=BF, device="cuda")
    a = block_args(B, T, ff, x=dev(x0.clone()), ctx=dev(ctx.to(BF)), enc_out=out, enc_act=act,
                   wout=dev(pack_k_units(ly.wout).to(BF)), pw1f=dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)),
                   params_c=dev(ly.c_group()), pw2=dev(pack_k_units(ly.pw2).to(BF)),
                   ff_w1=dev(pack_w1(ly.ff_w1).to(BF)), ff_w2=dev(pack_w2(ly.ff_w2).to(BF)), dw_w=dev(ly.dw_w), dw_b=dev(ly.dw_b),
                   params=dev(torch.cat(ly.d_groups() + [group(ag, ab), torch.zeros(G)])))
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_C | L.EM_BLOCK_D | L.EM_BLOCK_FINAL, a, L.current_stream_ptr()),
            "block<C|D|FINAL>")
    assert_close(out, ref, 6e-3, "block<C|D|FINAL> enc_out")
    assert_close(act, ref, 2e-2, "block<C|D|FINAL> enc_act")


def test_block_fused_rejects_outside_its_shapes(lib):
    x = torch.zeros(64, D, device="cuda")
    par = torch.zeros(4 * G, device="cuda")
    a = block_args(1, 64, 2048, x=x, params=par)
    assert lib.em_conformer_block_fused(L.EM_BLOCK_A, a, L.current_stream_ptr()) == L.EM_ERR_UNSUPPORTED
    a = block_args(1, 64, 1024, x=x, params=par)  # missing operands
    assert lib.em_conformer_block_fused(L.EM_BLOCK_A, a, L.current_stream_ptr()) == L.EM_ERR_BAD_ARG
    assert lib.em_conformer_block_fused(3, a, L.current_stream_ptr()) == L.EM_ERR_BAD_ARG


def test_block_repeatable_under_load(lib):
    """The weight stream runs three units ahead of the MFMAs on counted vmcnt waits, the H tiles and LayerNorm partials
    change hands between waves at barriers, and the L2 warm-up's share depends on arrival order: run the D|A kernel
    many times back to back at the bench shape and require bit-identical outputs (a read that raced its producer
    would show up as run-to-run differences)."""
    B, T, ff = 32, 249, 1024
    l0, l1 = Layer(600, ff), Layer(700, ff)
    x0, glu = rnd(B * T, D, seed=10), dev(q(rnd(B * T, D, seed=11)).to(BF))
    Tp = tpad(T)
    qh, kh = (torch.zeros(B, H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
    vt = torch.zeros(B, H, 64, Tp, dtype=BF, device="cuda")
    xd = dev(x0.clone())
    x0d = dev(x0)
    a = block_args(B, T, ff, x=xd, glu=glu, qh=qh, kh=kh, vt=vt, pw2=dev(pack_k_units(l0.pw2).to(BF)),
                   ff_w1=dev(pack_w1(l0.ff_w1).to(BF)), ff_w2=dev(pack_w2(l0.ff_w2).to(BF)), dw_w=dev(l0.dw_w), dw_b=dev(l0.dw_b),
                   ffm_w1=dev(pack_w1(l1.ffm_w1).to(BF)), ffm_w2=dev(pack_w2(l1.ffm_w2).to(BF)), wqkv=dev(pack_k_units(l1.wqkv).to(BF)),
                   params=dev(torch.cat(l0.d_groups() + l1.a_groups())))
    first = None
    for it in range(20):
        xd.copy_(x0d)
        L.check(lib.em_conformer_block_fused(L.EM_BLOCK_D | L.EM_BLOCK_A, a, L.current_stream_ptr()), "block<D|A>")
        got = (xd.clone(), qh.clone(), kh.clone(), vt.clone())
        if first is None:
            first = got
            x_ref, _ = l1.part_a(l0.part_d(x0, glu.float().cpu(), B, T))
            assert_close(xd, x_ref, 6e-3, "block<D|A> x at B=32")
        else:
            for g0, g1 in zip(first, got):
                assert torch.equal(g0, g1), f"run {it} differs from run 0"


# ------------------------------------------------------------------------------------------ one phase at a time, per element
def launch_probe(lib, p, kv_frag=0):
    """The launch of a tests/block_ref.py probe -> {output name: [B * T][256] tensor}, q / k / v unpacked."""
    B, T, ff, Tp = p.B, p.T, p.ff, tpad(p.T)
    bf = lambda t: dev(t.to(BF))
    ptrs, out = dict(x=dev(p.x0.clone())), {}
    if p.mode == "C":
        out["glu"] = torch.zeros(B * T, D, dtype=BF, device="cuda")
        ptrs.update(ctx=bf(p.ctx), glu=out["glu"], wout=bf(pack_k_units(p.l0.wout)), pw1f=bf(pack_k_units(p.l0.pw1[p.l0.perm()])),
                    params=dev(p.l0.c_group()))
        mode = L.EM_BLOCK_C
    if p.mode == "ATTC":
        # one valid key per utterance, v[b][0] = p.v0[b]; everything past it is masked: NaN keys (masked by select), finite junk
        # in V^T (0 * x), random queries and position table
        qh = torch.full((B, H, Tp, 64), float("nan"), dtype=BF)
        kh = torch.full((B, H, Tp, 64), float("nan"), dtype=BF)
        vt = torch.zeros(B, H, 64, Tp, dtype=BF)
        qh[:, :, :T] = rnd(B, H, T, 64, seed=p.seed + 600).to(BF)
        kh[:, :, :1] = rnd(B, H, 1, 64, seed=p.seed + 601).to(BF)
        vt[:, :, :, :T] = rnd(B, H, 64, T, seed=p.seed + 602).to(BF)
        vt[:, :, :, 0] = p.v0.reshape(B, H, 64).to(BF)
        ppk, npg = packed_pos(lib, bf(rnd(2 * T - 1, ar.LB * D, seed=p.seed + 603)), T, ar.LB)
        out["glu"] = torch.zeros(B * T, D, dtype=BF, device="cuda")
        ptrs.update(glu=out["glu"], qh=dev(qh), kh=dev(k_to_frag(kh)), vt=dev(vt_to_frag(vt)), wout=bf(pack_k_units(p.l0.wout)),
                    pw1f=bf(pack_k_units(p.l0.pw1[p.l0.perm()])), params=dev(p.l0.c_group()),
                    pos_u=dev(rnd(H, 64, seed=p.seed + 604, scale=0.3)), pos_v=dev(rnd(H, 64, seed=p.seed + 605, scale=0.3)),
                    klens=dev(torch.ones(B, dtype=torch.int32)))
        mode, ff, kv_frag = L.EM_BLOCK_ATT | L.EM_BLOCK_C, 256, 1  # (the C part has no ff; the fused launch is built at 256)
    if p.mode in ("CDF", "CDA"):  # folded: x is read only (a neighbour workgroup reads these rows as its halo)
        ptrs.update(ctx=bf(p.ctx), wout=bf(pack_k_units(p.l0.wout)), pw1f=bf(pack_k_units(p.l0.pw1[p.l0.perm()])), params_c=dev(p.l0.c_group()))
    elif p.mode in ("DF", "DA"):
        ptrs.update(glu=bf(p.glu))
    if p.mode in ("DF", "DA", "CDF", "CDA"):
        ptrs.update(pw2=bf(pack_k_units(p.l0.pw2)), ff_w1=bf(pack_w1(p.l0.ff_w1)), ff_w2=bf(pack_w2(p.l0.ff_w2)),
                    dw_w=dev(p.l0.dw_w), dw_b=dev(p.l0.dw_b), tlens=dev(torch.tensor(p.tlens, dtype=torch.int32)) if p.tlens else None)
    if p.mode in ("DF", "CDF"):
        out["enc_out"] = torch.zeros(B * T, D, dtype=torch.float32, device="cuda")
        out["enc_act"] = torch.zeros(B * T, D, dtype=BF, device="cuda")
        ptrs.update(enc_out=out["enc_out"], enc_act=out["enc_act"],
                    params=dev(torch.cat(p.l0.d_groups() + [group(p.ag, p.ab), torch.zeros(G)])))
        mode = L.EM_BLOCK_D | L.EM_BLOCK_FINAL | (L.EM_BLOCK_C if p.mode == "CDF" else 0)
    if p.mode in ("A", "DA", "CDA"):
        qh, kh = (torch.zeros(B, H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
        vt = torch.zeros(B, H, 64, Tp, dtype=BF, device="cuda")
        ptrs.update(qh=qh, kh=kh, vt=vt, ffm_w1=bf(pack_w1(p.l1.ffm_w1)), ffm_w2=bf(pack_w2(p.l1.ffm_w2)), wqkv=bf(pack_k_units(p.l1.wqkv)),
                    params=dev(torch.cat((p.l0.d_groups() if p.mode != "A" else []) + p.l1.a_groups())))
        mode = L.EM_BLOCK_A | (L.EM_BLOCK_D if p.mode != "A" else 0) | (L.EM_BLOCK_C if p.mode == "CDA" else 0)
        if p.mode == "CDA":
            ptrs["x_out"] = torch.full((B * T, D), float("nan"), device="cuda")
    a = block_args(B, T, ff, **ptrs)
    a.kv_frag = kv_frag
    if p.mode == "ATTC":
        a.pos, a.ldp = ppk.data_ptr() + 4 * npg * 2048, npg  # (the middle block of the table)
    L.check(lib.em_conformer_block_fused(mode, a, L.current_stream_ptr()), f"block<{p.mode}> probe {p.name}")
    if p.mode in ("CDF", "CDA"):
        assert torch.equal(ptrs["x"].cpu(), p.x0), "the folded kernel must not write its input residual"
    if p.mode not in ("DF", "CDF"):
        out["x"] = ptrs["x_out" if p.mode == "CDA" else "x"]
    if p.mode in ("A", "DA", "CDA"):
        if kv_frag:
            kh, vt = k_from_frag(kh.cpu()), vt_from_frag(vt.cpu())
        assert torch.isfinite(vt.float()).all(), "V^T columns >= T must be finite"
        out.update(q=split_heads(qh, B, T), k=split_heads(kh, B, T), v=vt[:, :, :, :T].permute(0, 3, 1, 2).reshape(B * T, D))
    return out


def hold_probe(lib, name, B, T, tlens, ff, kv_frag=0):
    """Every output of the probe inside the budget, per element; the stage shared behind x takes the x the device wrote."""
    p = br.probe_for(name, B, T, tlens, ff)
    got = launch_probe(lib, p, kv_frag)
    ref = p.run(br.RefOps(), mid=got.get("x"))
    for o in ref:
        r = br.assert_in_budget(got[o], ref[o], p, o, f"block<{p.mode}> B={B} T={T} ff={ff} tlens={tlens} kv_frag={kv_frag}")
        print(f"PARITY block<{p.mode}> {name} {o} B={B} T={T} ff={ff} masked={tlens is not None} kv_frag={kv_frag}: err / budget {r:.3f}")


@pytest.mark.parametrize("kv_frag", [0, 1])
@pytest.mark.parametrize("B,T,tlens,ff", br.UNMASKED_PARAMS, ids=br.UNMASKED_IDS)
def test_block_a_parity(lib, B, T, tlens, ff, kv_frag):
    """block<A>, two probes in one launch.  x behind the macaron FFN: the input rows are LN-clean at norm_macaron, the hidden
    activation's rounding is the one ambiguous level.  q / k / v: of norm_mha of the x the launch wrote, both K / V^T layouts.
    (Worst err / budget measured on an MI355X: block_ref.GPU_WORST.)"""
    hold_probe(lib, "a", B, T, tlens, ff, kv_frag)


@pytest.mark.parametrize("B,T,tlens,ff", br.UNMASKED_PARAMS, ids=br.UNMASKED_IDS)
def test_block_c_parity(lib, B, T, tlens, ff):
    """block<C>.  x + linear_out(ctx): float32, no rounding point - the accumulate term alone, on every element.  glu: of
    norm_conv of the x the launch wrote.  Measured on an MI355X, worst err / budget: x 0.098, glu 0.989."""
    hold_probe(lib, "c", B, T, tlens, ff)


@pytest.mark.parametrize("name", ["df_conv", "df_ffn"])
@pytest.mark.parametrize("B,T,tlens,ff", br.CASE_PARAMS, ids=br.CASE_IDS)
def test_block_d_final_parity(lib, B, T, tlens, ff, name):
    """block<D|FINAL>, enc_out (f32) and enc_act (bf16).  df_conv: ff_w2 = 0, so the conv module is seen through two float32
    LayerNorms, the conv output's rounding the one ambiguous level; frames at and past tlens hold junk of magnitude 3.
    df_ffn: glu = 0 on the valid frames and dw_b = 0, so the conv output is exactly zero and the feed-forward module runs
    on x + pw2 bias, rows LN-clean at norm_ff.
    (Worst err / budget measured on an MI355X: block_ref.GPU_WORST.)"""
    hold_probe(lib, name, B, T, tlens, ff)


@pytest.mark.parametrize("name", ["da_conv", "da_ffn", "da_mac"])
@pytest.mark.parametrize("B,T,tlens,ff", br.CASE_PARAMS, ids=br.CASE_IDS)
def test_block_da_parity(lib, B, T, tlens, ff, name):
    """block<D|A>.  da_conv, da_ffn: the two D probes with the macaron w2 = 0, x shows the D part; da_mac: the D part exact
    (zero conv, ff_w2 = 0, norm_final gain 0), the macaron FFN live.  q / k / v of the x the launch wrote, every time.
    (Worst err / budget measured on an MI355X: block_ref.GPU_WORST.)"""
    hold_probe(lib, name, B, T, tlens, ff)


@pytest.mark.parametrize("name", ["cda_conv", "cda_ffn", "cdf_conv", "cdf_ffn"])
@pytest.mark.parametrize("B,T,tlens,ff", br.CASE_PARAMS, ids=br.CASE_IDS)
def test_block_folded_parity(lib, B, T, tlens, ff, name):
    """block<C|D|A> and block<C|D|FINAL>, ctx = 0.  conv probes: pointwise_conv1's value half is the identity and its gate
    sigmoid(30) = 1, so the GLU rows that reach the conv tile - own rows and halo rows - are q(norm_conv(x + bout)) exactly,
    every row LN-clean; ffn probes: pointwise_conv1 = 0, the conv output exactly zero, rows LN-clean at norm_ff.  x comes back
    untouched, x_out (NaN before the launch) fully written.
    (Worst err / budget measured on an MI355X: block_ref.GPU_WORST.)"""
    hold_probe(lib, name, B, T, tlens, ff)


@pytest.mark.parametrize("B,T,tlens,ff", br.UNMASKED_PARAMS, ids=br.UNMASKED_IDS)
def test_block_att_c_rowlocal_parity(lib, B, T, tlens, ff):
    """block<ATT|C>, every utterance with one valid key: the attention phase hands v[b][0] to linear_out exactly, in every
    row, so the row-local phases of the fused launch are held as block<C>'s: x + linear_out(ctx) on the accumulate term alone,
    glu of norm_conv of the x the launch wrote.  (Worst err / budget measured on an MI355X: block_ref.GPU_WORST.)"""
    hold_probe(lib, "attc", B, T, tlens, ff)
