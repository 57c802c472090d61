"""Whole-transcript scoring with the attention decoder, the parts that need no GPU: the float64 restatement the device is
held against (tests/dec_seq_ref.py) agrees with the step oracle fed token by token, the host function that builds the
sentence pair of ESPnetASRModel.nll, the host-side refusals, and the proof that the bounds of tests/dec_seq_cases.py are
tight enough: each of the restatement's four defects moves some scored nll of every model by more than four times the
largest bf16 bound."""
import math

import pytest
import torch

from oracle.beam_search import DecoderOracle
from tests import dec_seq_cases as K
from tests import dec_seq_ref as R


def _params(name):
    return R.Params(K.state_dict(name), K.MODELS[name][1])


@pytest.mark.parametrize("name", sorted(K.MODELS))
def test_restatement_equals_the_step_oracle(name):
    """DecoderOracle.step (the K/V-cached label step the search tests rest on) fed token by token on the valid frames of
    each memory, float64, against the whole-sequence restatement: log-probs of every position within 1e-9."""
    V, heads, _ = K.MODELS[name]
    p = _params(name)
    mem, hl = K.make_memory(7)
    text, lens = K.make_text(17, V)
    ys_in, _, in_lens = R.sentence_pair(text, lens, V - 1, V - 1)
    logp = torch.log_softmax(R.forward(p, mem.double(), hl, ys_in, in_lens), dim=-1)
    worst = 0.0
    for b in range(3):
        orc = DecoderOracle(p.sd, mem[b, : int(hl[b])].double(), heads, K.LAYERS, 32)
        cache = orc.init_cache()
        for j in range(int(in_lens[b])):
            step, cache = orc.step(ys_in[b, j : j + 1], j, cache)
            worst = max(worst, float((step[0] - logp[b, j]).abs().max()))
    print(f"\nrestatement vs step oracle {name}: {worst:.3e}")
    assert worst <= 1e-9


def test_sentence_pair_by_hand():
    from espnet_amd.asr.espnet_model import build_dec_nll_batch

    sos = eos = 9
    ys = torch.tensor([[3, 4, 5], [7, -1, -1], [-1, 99, -1]])  # (whatever lies behind a length is not looked at)
    lens = torch.tensor([3, 1, 0])
    x, km, t = build_dec_nll_batch(ys, lens, sos, eos, vocab_size=10)
    assert x.dtype == km.dtype == t.dtype == torch.int32
    assert x.tolist() == [[9, 3, 4, 5], [9, 7, 9, 9], [9, 9, 9, 9]]
    assert km.tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0]]
    assert t.tolist() == [[3, 4, 5, 9], [7, 9, -1, -1], [9, -1, -1, -1]]
    # the restatement's own builder says the same
    ys_in, ys_out, in_lens = R.sentence_pair(ys, lens, sos, eos)
    assert ys_in.tolist() == x.tolist() and ys_out.tolist() == t.tolist() and in_lens.tolist() == [4, 2, 1]
    # a wider ys_pad is cut to the longest transcript; empty transcripts alone give one position
    x2, km2, t2 = build_dec_nll_batch(torch.zeros(2, 5, dtype=torch.long), torch.tensor([0, 0]), sos, eos, vocab_size=10)
    assert x2.tolist() == [[9], [9]] and km2.tolist() == [[1], [1]] and t2.tolist() == [[9], [9]]


def test_host_refusals():
    from espnet_amd.asr.espnet_model import build_dec_nll_batch

    ys = torch.tensor([[3, 4, 5], [7, 0, 0]])
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        build_dec_nll_batch(ys, torch.tensor([3, 1]), 4, 4, vocab_size=5)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        build_dec_nll_batch(torch.tensor([[3, -2]]), torch.tensor([2]), 9, 9, vocab_size=10)
    with pytest.raises(ValueError):
        build_dec_nll_batch(ys, torch.tensor([4, 1]), 9, 9, vocab_size=10)  # a length beyond ys_pad
    with pytest.raises(ValueError):
        build_dec_nll_batch(ys, torch.tensor([3]), 9, 9, vocab_size=10)
    # a model without an attention decoder names the reason before anything touches a device
    from espnet_amd.asr.espnet_model import ESPnetASRModel
    from oracle.weights import token_list

    kw = dict(frontend=None, specaug=None, normalize=None, preencoder=None, encoder=None, postencoder=None)
    m = K.build_model("h2")
    ctc_only = ESPnetASRModel(300, token_list(300), decoder=m.decoder, ctc=torch.nn.Identity(), ctc_weight=1.0, **kw)
    enc = torch.zeros(1, 4, K.D)
    with pytest.raises(RuntimeError, match="ctc_weight == 1.0"):
        ctc_only.nll(enc, torch.tensor([4]), ys[:1], torch.tensor([3]))
    with pytest.raises(RuntimeError, match="ctc_weight == 1.0"):
        ctc_only.batchify_nll(enc, torch.tensor([4]), ys[:1], torch.tensor([3]), batch_size=1)
    ctc_only.use_transducer_decoder = True
    with pytest.raises(RuntimeError, match="transducer"):
        ctc_only.nll(enc, torch.tensor([4]), ys[:1], torch.tensor([3]))
    # token ids are checked on the host: no GPU is needed to be refused
    with pytest.raises(ValueError, match=r"\[0, 300\)"):
        m.nll(enc, torch.tensor([4]), torch.tensor([[3, 300]]), torch.tensor([2]))


@pytest.mark.parametrize("name", sorted(K.MODELS))
def test_defects_are_visible(name):
    """Each defect moves some scored nll of the chain tests' inputs (Lp = 17) by more than four times the largest bf16
    bound: a device path with that defect could not pass tests/test_gpu_dec_seq.py."""
    V, heads, _ = K.MODELS[name]
    p = _params(name)
    mem, hl = K.make_memory(1000 + 17)
    text, lens = K.make_text(17, V)
    good, in_lens = R.nll(p, mem.double(), hl, text, lens, V - 1, V - 1)
    need = 4 * max(K.E_NLL.values())
    for defect in R.DEFECTS:
        bad, _ = R.nll(p, mem.double(), hl, text, lens, V - 1, V - 1, defect=defect)
        moved = float((bad - good).abs().max())
        print(f"\n{name} defect {defect}: largest movement of a scored nll {moved:.3f} (needed > {need:.3f})")
        assert math.isfinite(moved) and moved > need, defect
