"""Where the row-block kernels' row stores go (csrc/block.hip, store_x_counted): block<A>, block<D|A> and block<ATT|C>
write x UNCONDITIONALLY, through a buffer resource whose range ends with frame T - 1 of the workgroup's utterance - a lane
of a row >= T asks for an offset past that range and the store is dropped; glu, enc_out, enc_act and the CTC ids of
block<D|FINAL|CTC> are stored under the row mask.
What can go wrong with either is an address: a masked row written somewhere real, a clamped duplicate on frame T - 1, a
range that is one utterance off.  So every output here lives between two sentinel-filled guard regions, and every row
0 .. T - 1 of every utterance (the layout is [B * T][256]: a masked row of utterance b that leaked would land on the first
rows of utterance b + 1, or in the guard behind the last one) is held to the torch restatement of tests/test_gpu_block.py
within that file's bounds: 4e-3 of the output scale for the f32 residual stream and enc_out (6e-3 behind the two modules
of block<D|A>), 2e-2 for bf16 outputs (3e-2 in block<D|A>).  Frame T - 1 of every utterance is checked on its own against
the same bound.  A second launch on the same inputs must give the same bits.

Shapes (d = 256, 4 heads, ff = 1024, k = 31): B = 1, T = 33 - the second row block has one valid row and 31 masked ones;
B = 3, T = 64 - no masked rows, plain workgroup order in block<ATT|C>; B = 9, T = 40 - eight utterances in the dealt order
of block<ATT|C>, the ninth plain, 24 masked rows per utterance.  The CTC head has 1, 2 and 6 weight units over the three
shapes: fewer units than the three requested ahead, and more than one group of four in the walk.

CTC ids: the kernel's logits are f32 sums of 256 products of the bf16 rows it stored (enc_act) with the bf16 weights; the
reference sums the same products in float64.  An f32 sum of n terms is off by at most n * 2^-24 * sum |term|, so two
logits can swap order only if the reference separates them by less than 2 * 256 * 2^-24 * S, S the largest sum of
absolute products of the frame: every frame with a larger top-2 margin must carry the reference's id."""
import math

import pytest
import torch

from espnet_amd import lib as L
from espnet_amd.asr.encoder.conformer_encoder import pack_k_units, pack_w1, pack_w2
from tests import test_gpu_block as TB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, H, G, FF = TB.D, TB.H, TB.G, 1024
GUARD, SENTINEL = 4096, 0xA5
SHAPES = [(1, 33), (3, 64), (9, 40)]
KLENS = {33: [33], 64: [64, 17, 1], 40: [40, 39, 38, 37, 3, 2, 1, 40, 17]}
VOCAB = {33: 40, 64: 100, 40: 330}  # 1, 2 and 6 units of 64 labels


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    TB._KEEP.clear()


class Guarded:
    """A device tensor between two guard regions of GUARD sentinel bytes."""

    def __init__(self, shape, dtype, init=None):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.raw = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(init.to(dtype))

    def check(self, what):
        front, back = self.raw[:GUARD], self.raw[GUARD + self.n:]
        assert bool((front == SENTINEL).all()), f"{what}: the guard in front was written"
        assert bool((back == SENTINEL).all()), f"{what}: the guard behind was written"


def close(got, ref, tol, what, B, T):
    """test_gpu_block.assert_close, and frame T - 1 of every utterance by name against the same bound."""
    got, ref = got.float().cpu(), ref.float().cpu()
    TB.assert_close(got, ref, tol, what)
    scale = max(ref.abs().max().item(), 1e-6)
    last = torch.arange(B) * T + T - 1
    err = (got[last] - ref[last]).abs().max().item()
    assert err <= tol * scale, f"{what}, frame T - 1: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def run_twice(lib, mode, a, what, xg, x0, outs):
    """Launch, check the guards, launch again on the same inputs: equal bits.  Returns nothing; `outs` hold the results."""
    L.check(lib.em_conformer_block_fused(mode, a, L.current_stream_ptr()), what)
    torch.cuda.synchronize()
    for name, g in outs.items():
        g.check(f"{what} {name}")
    first = {name: g.t.clone() for name, g in outs.items()}
    xg.t.copy_(x0)  # (x is updated in place where the mode stores it)
    L.check(lib.em_conformer_block_fused(mode, a, L.current_stream_ptr()), what)
    torch.cuda.synchronize()
    for name, g in outs.items():
        g.check(f"{what} {name}, second launch")
        assert torch.equal(first[name], g.t), f"{what} {name}: the second launch gave other bits"


def qkv_buffers(B, T):
    Tp = TB.tpad(T)
    return Guarded((B, H, Tp, 64), BF), Guarded((B, H, Tp, 64), BF), Guarded((B, H, 64, Tp), BF)


def check_qkv(qh, kh, vt, qkv_ref, tol, what, B, T):
    close(TB.split_heads(qh.t, B, T), qkv_ref[:, :D], tol, f"{what} q", B, T)
    close(TB.split_heads(kh.t, B, T), qkv_ref[:, D:2 * D], tol, f"{what} k", B, T)
    close(vt.t[:, :, :, :T].permute(0, 3, 1, 2).reshape(B * T, D), qkv_ref[:, 2 * D:], tol, f"{what} v", B, T)


@pytest.mark.parametrize("B,T", SHAPES)
def test_block_a_store_order(lib, B, T):
    ly = TB.Layer(100, FF)
    x0 = TB.rnd(B * T, D, seed=1)
    x_ref, qkv_ref = ly.part_a(x0)
    xg = Guarded((B * T, D), torch.float32, x0)
    qh, kh, vt = qkv_buffers(B, T)
    a = TB.block_args(B, T, FF, x=xg.t, qh=qh.t, kh=kh.t, vt=vt.t, ffm_w1=TB.dev(pack_w1(ly.ffm_w1).to(BF)),
                      ffm_w2=TB.dev(pack_w2(ly.ffm_w2).to(BF)), wqkv=TB.dev(pack_k_units(ly.wqkv).to(BF)),
                      params=TB.dev(torch.cat(ly.a_groups())))
    run_twice(lib, L.EM_BLOCK_A, a, "block<A>", xg, x0, dict(x=xg, q=qh, k=kh, v=vt))
    close(xg.t, x_ref, 4e-3, "block<A> x", B, T)
    check_qkv(qh, kh, vt, qkv_ref, 2e-2, "block<A>", B, T)


@pytest.mark.parametrize("B,T", SHAPES)
def test_block_da_store_order(lib, B, T):
    l0, l1 = TB.Layer(400, FF), TB.Layer(500, FF)
    x0, glu = TB.rnd(B * T, D, seed=8), TB.q(TB.rnd(B * T, D, seed=9))
    x_ref, qkv_ref = l1.part_a(l0.part_d(x0, glu, B, T))
    xg = Guarded((B * T, D), torch.float32, x0)
    qh, kh, vt = qkv_buffers(B, T)
    a = TB.block_args(B, T, FF, x=xg.t, glu=TB.dev(glu.to(BF)), qh=qh.t, kh=kh.t, vt=vt.t, pw2=TB.dev(pack_k_units(l0.pw2).to(BF)),
                      ff_w1=TB.dev(pack_w1(l0.ff_w1).to(BF)), ff_w2=TB.dev(pack_w2(l0.ff_w2).to(BF)), dw_w=TB.dev(l0.dw_w),
                      dw_b=TB.dev(l0.dw_b), ffm_w1=TB.dev(pack_w1(l1.ffm_w1).to(BF)), ffm_w2=TB.dev(pack_w2(l1.ffm_w2).to(BF)),
                      wqkv=TB.dev(pack_k_units(l1.wqkv).to(BF)), params=TB.dev(torch.cat(l0.d_groups() + l1.a_groups())))
    run_twice(lib, L.EM_BLOCK_D | L.EM_BLOCK_A, a, "block<D|A>", xg, x0, dict(x=xg, q=qh, k=kh, v=vt))
    close(xg.t, x_ref, 6e-3, "block<D|A> x", B, T)
    check_qkv(qh, kh, vt, qkv_ref, 3e-2, "block<D|A>", B, T)


@pytest.mark.parametrize("B,T", SHAPES)
def test_block_att_c_store_order(lib, B, T):
    ly = TB.Layer(1100, FF)
    at = TB._attention_inputs(B, T, KLENS[T], 40)
    x0 = TB.rnd(B * T, D, seed=2)
    x_ref, glu_ref = ly.part_c(x0, TB.q(at["ctx"]))
    palld = TB.dev(at["pall"].to(BF))
    ppk, npg = TB.packed_pos(lib, palld, T, at["Lb"])
    xg = Guarded((B * T, D), torch.float32, x0)
    glu = Guarded((B * T, D), BF)
    a = TB.block_args(B, T, FF, x=xg.t, glu=glu.t, qh=TB.dev(at["qh"]), kh=TB.dev(TB.k_to_frag(at["kh"])),
                      vt=TB.dev(TB.vt_to_frag(at["vt"])), wout=TB.dev(pack_k_units(ly.wout).to(BF)),
                      pw1f=TB.dev(pack_k_units(ly.pw1[ly.perm()]).to(BF)), params=TB.dev(ly.c_group()), pos_u=TB.dev(at["u"]),
                      pos_v=TB.dev(at["v"]), klens=TB.dev(torch.tensor(KLENS[T], dtype=torch.int32)))
    a.pos, a.ldp, a.kv_frag = ppk.data_ptr() + 4 * npg * 2048, npg, 1  # (the middle block of the table)
    run_twice(lib, L.EM_BLOCK_ATT | L.EM_BLOCK_C, a, "block<ATT|C>", xg, x0, dict(x=xg, glu=glu))
    close(xg.t, x_ref, 4e-3, "block<ATT|C> x", B, T)
    close(glu.t, glu_ref, 2e-2, "block<ATT|C> glu", B, T)


@pytest.mark.parametrize("B,T", SHAPES)
def test_block_d_final_ctc_store_order(lib, B, T):
    ly = TB.Layer(300, FF)
    V = VOCAB[T]
    units = (V + 63) // 64
    x0, glu = TB.rnd(B * T, D, seed=4), TB.q(TB.rnd(B * T, D, seed=5))
    ag, ab = 1 + 0.1 * TB.rnd(D, seed=6), 0.1 * TB.rnd(D, seed=7)
    ref = TB.ln(ly.part_d(x0, glu, B, T), ag, ab)
    cw, cb = TB.q(TB.rnd(V, D, seed=10, scale=D ** -0.5)), TB.rnd(V, seed=11, scale=0.1)
    wt = torch.zeros(units * 64, D)
    wt[:V] = cw
    bt = torch.full((units * 64,), -3.0e38)
    bt[:V] = cb
    xg = Guarded((B * T, D), torch.float32, x0)
    out, act, ids = Guarded((B * T, D), torch.float32), Guarded((B * T, D), BF), Guarded((B * T,), torch.int32)
    ids.t.fill_(-1)
    a = TB.block_args(B, T, FF, x=xg.t, glu=TB.dev(glu.to(BF)), enc_out=out.t, enc_act=act.t, pw2=TB.dev(pack_k_units(ly.pw2).to(BF)),
                      ff_w1=TB.dev(pack_w1(ly.ff_w1).to(BF)), ff_w2=TB.dev(pack_w2(ly.ff_w2).to(BF)), dw_w=TB.dev(ly.dw_w),
                      dw_b=TB.dev(ly.dw_b), params=TB.dev(torch.cat(ly.d_groups() + [TB.group(ag, ab), torch.zeros(G)])),
                      ctc_w=TB.dev(pack_k_units(wt).to(BF)), ctc_b=TB.dev(bt), ctc_ids=ids.t)
    a.ctc_units = units
    mode = L.EM_BLOCK_D | L.EM_BLOCK_FINAL | L.EM_BLOCK_CTC
    run_twice(lib, mode, a, "block<D|FINAL|CTC>", xg, x0, dict(x=xg, enc_out=out, enc_act=act, ctc_ids=ids))
    assert torch.equal(xg.t.cpu(), x0), "block<D|FINAL|CTC> does not store x"
    close(out.t, ref, 4e-3, "block<D|FINAL|CTC> enc_out", B, T)
    close(act.t, ref, 2e-2, "block<D|FINAL|CTC> enc_act", B, T)
    # the ids: arg-max over the logits of the rows the kernel stored, float64 (see the module docstring for the margin)
    rows = act.t.cpu().to(torch.float64)
    logits = rows @ cw.to(torch.float64).t() + cb.to(torch.float64)
    S = (rows.abs() @ cw.to(torch.float64).abs().t() + cb.to(torch.float64).abs()).max(dim=-1).values
    top2 = logits.topk(2, dim=-1)
    margin = top2.values[:, 0] - top2.values[:, 1]
    got = ids.t.cpu().to(torch.int64)
    assert int(got.min()) >= 0 and int(got.max()) < V
    decided = margin >= 2 * 256 * 2.0 ** -24 * S
    assert torch.equal(got[decided], top2.indices[:, 0][decided]), "block<D|FINAL|CTC> ctc_ids"
    assert int(decided.sum()) >= (B * T * 9) // 10  # (the margin excuses round-off ties only)
