"""Per-element float64 parity of every stand-alone encoder self-attention entry point, through the C ABI:

  em_relpos_attention          f32, bf16   csrc/attention.hip
  em_legacy_relpos_attention   f32, bf16   csrc/attention.hip (LEGACY)
  em_relpos_attention2_bf16    bf16        csrc/attention2.hip
  em_abs_attention_bf16        bf16        csrc/abs_attn.hip (MFMA form)
  em_abs_attention             f32, bf16   csrc/abs_attn.hip (row form)

(the attention phase of block<ATT|C> is held to the same budget in tests/test_gpu_block.py::test_block_att_c_attention_parity).
Reference, inputs and the one tolerance are tests/attention_ref.py: a float64 restatement from the operands the device sees,
a sparse v that makes every key visible in the output, and |got - ref| <= 3 u A + f (1 + S) A per element for bf16,
f (1 + S) A for f32, exactly zero where no valid key reaches the channel.  tests/test_cpu_attention_ref.py shows that six
wrong variants of the reference (a key too many, a key dropped, the position term shifted by one or summed over 56
channels) each break that budget by more than ten times.

Shapes (attention_ref.*_CASES) are the smallest that touch each edge: T = 1; key counts that end on, one before and one
behind a 16-row fragment, a 64-key tile and a 256-key super-tile; an utterance of one or two keys in the batch;
klens[b] > T (clamped by the launchers); T = 520 with Tpad = 768 for the routes with 256-key super-tiles.  Three heads
(one case again with one), the position table with ldp = 3 d and the middle block, as the encoder calls it.  Each case
runs flat (|score| <~ 8) and sharp (|score| ~ 30: large steps of the running maximum between tiles).  Padding frames of the
per-head layouts hold NaN in Q and K everywhere, in V^T NaN for em_abs_attention_bf16 and zeros for
em_relpos_attention2_bf16, as their contracts say.

Measured on an MI355X, the worst err / budget per route over all its cases (the CPU simulation of a faithful bf16 kernel
reaches 0.69, attention_ref.SIM_BF16_MAX; no route needed a rounding point added to the reference):
  em_relpos_attention          f32 0.257 (T = 130, h = 1, sharp)    bf16 0.660 (T = 130, sharp)
  em_legacy_relpos_attention   f32 0.257 (T = 130, h = 1, sharp)    bf16 0.686 (T = 300, sharp)
  em_relpos_attention2_bf16    0.675 (T = 520, sharp)
  em_abs_attention_bf16        0.673 (T = 130, sharp)
  em_abs_attention             f32 0.201 (T = 130, h = 1, sharp)    bf16 0.332 (T = 130, flat; its probabilities stay f32)
  block<ATT|C>, attention      0.673 (T = 40, nine utterances, sharp)
"""
import pytest
import torch

from espnet_amd import lib as L
from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DT = {"f32": (L.EM_F32, torch.float32), "bf16": (L.EM_BF16, torch.bfloat16)}
DK = ar.DK


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


_KEEP = []


def dev(t):
    """Copy to the GPU and keep the tensor alive until the test ends (raw pointers go to the C ABI)."""
    t = t.contiguous().cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


_REFS = {}


def reference(kind, case):
    """the float64 reference, computed once per (score definition, inputs) and shared by the routes that use it"""
    key = (kind, id(case))
    if key not in _REFS:
        _REFS[key] = {"rel": lambda: ar.ref_rel(case, "sum"), "rel_scaled": lambda: ar.ref_rel(case, "scaled"),
                      "legacy": lambda: ar.ref_legacy(case), "abs": lambda: ar.ref_abs(case)}[kind]()
    return _REFS[key]


def ids(cases):
    return [f"T{T}x{len(kl)}-h{h}" + ("-clamp" if max(kl) > T else "") for T, kl, h in cases]


def tpad(T):
    return (T + 255) // 256 * 256


def klens_dev(case):
    return dev(torch.tensor(case.klens, dtype=torch.int32))  # (as given: the launchers clamp klens[b] > T)


def qkv_rows(case):
    """q | k | v rows [B][T][3 d] in the activation dtype"""
    B, T, d = len(case.klens), case.T, case.h * DK
    return dev(torch.cat([t.reshape(B, T, d) for t in (case.q, case.k, case.v)], -1).to(case.dtype))


def per_head(case, vt_pad):
    """Q, K [B][h][Tpad][64] with NaN padding frames and V^T [B][h][64][Tpad] padded with `vt_pad`"""
    B, T, h, Tp = len(case.klens), case.T, case.h, tpad(case.T)
    qh = torch.full((B, h, Tp, DK), float("nan"), dtype=torch.bfloat16)
    kh = torch.full((B, h, Tp, DK), float("nan"), dtype=torch.bfloat16)
    vt = torch.full((B, h, DK, Tp), vt_pad, dtype=torch.bfloat16)
    qh[:, :, :T] = case.q.transpose(1, 2).to(torch.bfloat16)
    kh[:, :, :T] = case.k.transpose(1, 2).to(torch.bfloat16)
    vt[:, :, :, :T] = case.v.permute(0, 2, 3, 1).to(torch.bfloat16)
    return dev(qh), dev(kh), dev(vt), Tp


def out_buffer(case):
    return torch.full((len(case.klens), case.T, case.h * DK), float("nan"), dtype=case.dtype, device="cuda")


def hold(route, got, kind, case, regime):
    r = ar.assert_in_budget(got, reference(kind, case), case.dtype, f"{route} T={case.T} klens={case.klens} h={case.h} {regime}")
    print(f"PARITY {route} T={case.T} B={len(case.klens)} h={case.h} {regime}: err / budget {r:.3f}")


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T,klens,h", ar.STANDALONE_CASES, ids=ids(ar.STANDALONE_CASES))
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("legacy", [False, True], ids=["rel", "legacy"])
def test_relpos_attention_parity(lib, legacy, prec, T, klens, h, regime):
    """em_relpos_attention / em_legacy_relpos_attention: the table is handed over as the encoder does, ldp = 3 d and a base
    offset of d (the legacy scheme reads its first T rows)."""
    dt, tdt = DT[prec]
    case = ar.case_for(T, klens, h, regime, tdt)
    d = h * DK
    table = dev((case.pall[:T] if legacy else case.pall).to(tdt))
    ctx = out_buffer(case)
    fn = lib.em_legacy_relpos_attention if legacy else lib.em_relpos_attention
    L.check(fn(dt, L.ptr(qkv_rows(case)), table.data_ptr() + d * table.element_size(), ar.LB * d, L.ptr(dev(case.u)),
               L.ptr(dev(case.vb)), L.ptr(klens_dev(case)), len(klens), T, h, DK, L.ptr(ctx), L.current_stream_ptr()))
    name = "legacy" if legacy else "rel"
    hold(f"em_{'legacy_' if legacy else ''}relpos_attention[{prec}]", ctx, name, case, regime)


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T,klens,h", ar.SUPER_TILE_CASES, ids=ids(ar.SUPER_TILE_CASES))
def test_relpos_attention2_parity(lib, T, klens, h, regime):
    case = ar.case_for(T, klens, h, regime)
    d = h * DK
    qh, kh, vt, Tp = per_head(case, 0.0)  # V^T padding must be finite (0 * x)
    table = dev(case.pall.to(torch.bfloat16))
    ctx = out_buffer(case)
    L.check(lib.em_relpos_attention2_bf16(L.ptr(qh), L.ptr(kh), L.ptr(vt), table.data_ptr() + d * 2, ar.LB * d, L.ptr(dev(case.u)),
                                          L.ptr(dev(case.vb)), L.ptr(klens_dev(case)), len(klens), T, Tp, h, L.ptr(ctx),
                                          L.current_stream_ptr()), "attention2")
    hold("em_relpos_attention2_bf16", ctx, "rel_scaled", case, regime)


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T,klens,h", ar.SUPER_TILE_CASES, ids=ids(ar.SUPER_TILE_CASES))
def test_abs_attention_bf16_parity(lib, T, klens, h, regime):
    case = ar.case_for(T, klens, h, regime)
    qh, kh, vt, Tp = per_head(case, float("nan"))  # keys >= klen are staged as zeros whatever the padding holds
    ctx = out_buffer(case)
    L.check(lib.em_abs_attention_bf16(L.ptr(qh), L.ptr(kh), L.ptr(vt), L.ptr(klens_dev(case)), len(klens), T, Tp, h, L.ptr(ctx),
                                      L.current_stream_ptr()), "em_abs_attention_bf16")
    hold("em_abs_attention_bf16", ctx, "abs", case, regime)


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("T,klens,h", ar.STANDALONE_CASES, ids=ids(ar.STANDALONE_CASES))
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_abs_attention_rows_parity(lib, prec, T, klens, h, regime):
    dt, tdt = DT[prec]
    case = ar.case_for(T, klens, h, regime, tdt)
    ctx = out_buffer(case)
    L.check(lib.em_abs_attention(dt, L.ptr(qkv_rows(case)), L.ptr(klens_dev(case)), len(klens), T, h, DK, L.ptr(ctx),
                                 L.current_stream_ptr()), "em_abs_attention")
    hold(f"em_abs_attention[{prec}]", ctx, "abs", case, regime)
