"""The feed-forward module of the 256-wide block kernels (csrc/block.hip, `ffn`) after the move of its cross-wave exchange
from the K-split partial sums (once per module, behind the loop) to the hidden tile (once per chunk pair, inside the loop):
W2 is dealt to the four waves by output columns, every wave reads all four waves' slices of the pair's hidden tile from a
double-buffered LDS slot.

  parity        every ff width at which the loop takes another path, through the float64 probes of tests/block_ref.py
  routing       integers through the exchange: a slot read from the wrong slice, buffer or frame half is a wrong integer
  determinism   two launches, the same bits
  streaming     the RELU / global-bias / split-FFN instantiations (ff = 2048) against the per-operator sequence

All at B = 2, T = 33: two workgroups per utterance, the second with one valid row.
"""
import os

import numpy as np
import pytest
import torch

from espnet_amd import lib as L
from espnet_amd.asr.encoder.conformer_encoder import pack_k_units, pack_w1, pack_w2
from tests import block_ref as br
from tests import test_gpu_block as tb
from tests.block_ref import Layer

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 256
B, T = 2, 33
# one chunk padded to a pair, no loop iteration; one pair; an odd chunk count (a zero chunk); the first buffer switch; the bench width
WIDTHS = [64, 128, 192, 256, 1024]

lib = tb.lib
_release_kept_tensors = tb._release_kept_tensors


@pytest.mark.parametrize("name", ["a", "da_ffn", "da_mac", "df_ffn"])
@pytest.mark.parametrize("ff", WIDTHS)
def test_ffn_widths_parity(lib, ff, name):
    """block<A> (a), block<D|A> (da_ffn: the D part's module live, da_mac: the macaron module live) and block<D|FINAL> (df_ffn):
    every output element inside block_ref's own budget.  probe_for accepts every width up to 1024 (the parameter group holds
    1024 first-bias slots), so none is left out."""
    tb.hold_probe(lib, name, B, T, None, ff)


def _swish_inverse(y):
    """v with v * sigmoid(v) = y (y >= 1), float64 Newton"""
    v = y.clone().double() + 0.5
    for _ in range(60):
        s = torch.sigmoid(v)
        v = v - (v * s - y) / (s + v * s * (1 - s))
    return v


def _hidden_id(j):
    """1 + j // 4: names hidden column j's (pair, chunk of the pair, slice = wave, lane group); at most 256, exact in bf16"""
    return 1 + j // 4


@pytest.mark.parametrize("ff", [256, 1024])
def test_ffn_exact_routing(lib, ff):
    """block<A> with W1 = 0, so the hidden activation is swish(b1[j]) in every row, and b1 chosen so that it rounds in bf16 to
    the integer 1 + j // 4; W2 one-hot (output column c takes hidden column sel[c]), b2 = 0 and a zero residual: x must be
    0.5 * (1 + sel[c] // 4) exactly (0.5: the macaron module's scale; halves of integers up to 256 are exact in f32)."""
    ly = Layer(900 + ff, ff)
    j = torch.arange(ff)
    ids = _hidden_id(j).double()
    ly.ffm_b1 = _swish_inverse(ids).float()
    h = ly.ffm_b1 * torch.sigmoid(ly.ffm_b1)  # (the kernel's sigmoid is off by a few 2^-24 relative, a bf16 rounding boundary by 2^-9)
    assert torch.equal(h.to(BF).double(), ids) and float((h.double() / ids - 1).abs().max()) < 1e-5
    ly.ffm_w1 = torch.zeros(ff, D)
    ly.ffm_b2 = torch.zeros(D)
    np_ = ff // 128
    pairs = sorted({0, np_ // 2, np_ - 1})
    c = torch.arange(D)
    # 37 is odd: (37 c + 11) % 128 visits every column of a pair twice over the 256 outputs, and with the pair chosen by
    # c % len(pairs) every (pair, slice, lane group) of the chosen pairs is taken by some output column
    sel = 128 * torch.tensor(pairs)[c % len(pairs)] + (37 * c + 11) % 128
    if ff == 256:
        sel = (37 * c + 11) % 256  # (every hidden column once)
    seen = {(int(s) // 128, (int(s) % 64) // 16) for s in sel}
    assert seen == {(p, w) for p in pairs for w in range(4)}, "one column from every slice of the first, a middle and the last pair"
    ly.ffm_w2 = torch.zeros(D, ff)
    ly.ffm_w2[c, sel] = 1.0
    Tp = tb.tpad(T)
    xd = tb.dev(torch.zeros(B * T, D))
    qh, kh = (torch.zeros(B, tb.H, Tp, 64, dtype=BF, device="cuda") for _ in range(2))
    vt = torch.zeros(B, tb.H, 64, Tp, dtype=BF, device="cuda")
    a = tb.block_args(B, T, ff, x=xd, qh=qh, kh=kh, vt=vt, ffm_w1=tb.dev(pack_w1(ly.ffm_w1).to(BF)), ffm_w2=tb.dev(pack_w2(ly.ffm_w2).to(BF)),
                      wqkv=tb.dev(pack_k_units(ly.wqkv).to(BF)), params=tb.dev(torch.cat(ly.a_groups())))
    L.check(lib.em_conformer_block_fused(L.EM_BLOCK_A, a, L.current_stream_ptr()), "block<A>")
    got = 2.0 * xd.cpu().double()
    want = _hidden_id(sel).double().expand(B * T, D)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} elements; first: row {int(bad[0, 0])}, column {int(bad[0, 1])} (wave {int(bad[0, 1]) % 64 // 16}) "
                              f"got id {float(got[bad[0, 0], bad[0, 1]])}, hidden column {int(sel[bad[0, 1]])} has id {float(want[0, bad[0, 1]])}")


@pytest.mark.parametrize("name", ["a", "da_ffn", "da_mac"])
def test_ffn_two_launches_same_bits(lib, name):
    """ff = 1024, block<A> and block<D|A> (either module live): a read of a slot that raced its writer would differ run to run"""
    p = br.probe_for(name, B, T, None, 1024)
    first, second = tb.launch_probe(lib, p), tb.launch_probe(lib, p)
    for o in first:
        assert torch.equal(first[o], second[o]), f"probe {name}, output {o}: the second launch differs"


def test_streaming_relu_global_bias_and_split():
    """The streaming instantiations run the same lambda: block<A | RELU>, block<D | RELU> (k = 15) at ff = 2048, first bias from
    global memory, unsplit (ESPNET_AMD_STREAM_FFN_SPLIT=1) and in two shares, on one short call (one block: the smallest
    shape the entry takes), against the per-operator sequence of the same bf16 weights with the bound of
    tests/test_gpu_streaming.py::test_streaming_fused_layers_match_per_operator_sequence."""
    from tests.helpers import load_stream_golden, stream_feats
    from tests.test_gpu_streaming import build

    g = load_stream_golden("stream_small_6s")
    assert g["conf"]["linear_units"] == 2048
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"]))[None, :100].cuda()
    enc = build(g, "bfloat16")
    assert enc._fusable()

    def run(split):
        os.environ["ESPNET_AMD_STREAM_FFN_SPLIT"] = str(split)
        L.load().em_dev_switches_reload()
        enc.invalidate()
        y, _, _ = enc(feats, torch.tensor([100]), None, is_final=True, infer_mode=True)
        return y.float().cpu()

    try:
        os.environ.pop("ESPNET_AMD_STREAM_FUSED_MIN", None)
        fused = {s: run(s) for s in (1, 2)}
        assert torch.equal(fused[2], run(2)), "two shares: not repeatable"
        enc.fused = False
        ref = run(1)
    finally:
        os.environ.pop("ESPNET_AMD_STREAM_FFN_SPLIT", None)
        L.load().em_dev_switches_reload()
    for s, y in fused.items():
        d = (y - ref).abs()
        print(f"[stream fused, ffn_split {s}, vs per-operator] max {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert np.isfinite(y.numpy()).all()
        assert d.max().item() < 8e-2 and d.mean().item() < 8e-3, s
