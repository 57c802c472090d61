"""Transducer likelihood of given transcripts without a GPU: the float64 restatement of the contract
(tests/transducer_nll_ref.py) against brute-force path enumeration, its -inf handling, the host refusals of
`ESPnetASRModel.transducer_nll` and `Speech2Text.batch_transducer_nll`, and the bindings of the new entry points."""
import math
import types

import numpy as np
import pytest
import torch

from tests.transducer_nll_ref import brute_force_nll, forward_nll


def _random_lattice(rng, T, U, V=6):
    """A lattice whose nodes are honest distributions: log-softmax of random logits, blank = column 0, label = column 1."""
    logits = rng.normal(size=(T, U + 1, V)) * 2.0
    lp = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
    lat = np.stack([lp[..., 0], lp[..., 1]], -1)
    lat[:, U, 1] = -np.inf
    return lat


def test_recursion_equals_path_enumeration():
    rng = np.random.default_rng(5)
    cells = 0
    for T in range(1, 6):
        for U in range(0, 4):
            lat = _random_lattice(rng, T, U)
            got, want = forward_nll(lat, T, U), brute_force_nll(lat, T, U)
            assert math.isfinite(want) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (T, U, got, want)
            cells += 1
    assert cells == 20
    # U == 0: the blanks of column 0 alone; T == 1: every label on the one frame, then the blank
    lat = _random_lattice(rng, 4, 0)
    assert abs(forward_nll(lat, 4, 0) + lat[:, 0, 0].sum()) <= 1e-12
    lat = _random_lattice(rng, 1, 3)
    assert abs(forward_nll(lat, 1, 3) + lat[0, :3, 1].sum() + lat[0, 3, 0]) <= 1e-12


def test_recursion_reads_its_own_nodes_only():
    """A larger array around the lattice, full of NaN outside (T_b, U): the value does not change."""
    rng = np.random.default_rng(6)
    lat = _random_lattice(rng, 4, 2)
    big = np.full((7, 5, 2), np.nan)
    big[:4, :3] = lat
    assert forward_nll(big, 4, 2) == forward_nll(lat, 4, 2)


def test_minus_infinity_is_a_value_not_an_error():
    rng = np.random.default_rng(7)
    assert forward_nll(np.zeros((0, 1, 2)), 0, 0) == math.inf  # no frame: no path
    lat = _random_lattice(rng, 4, 2)
    blocked = lat.copy()
    blocked[:, 1, 1] = -np.inf  # label 1 can never be emitted: no path reaches u = 2
    assert forward_nll(blocked, 4, 2) == math.inf and brute_force_nll(blocked, 4, 2) == math.inf
    row = lat.copy()
    row[2] = -np.inf  # frame 2 neither emits nor moves on
    assert forward_nll(row, 4, 2) == math.inf
    some = lat.copy()
    some[1, 0, 0] = -np.inf  # one blocked move: the other paths remain
    got, want = forward_nll(some, 4, 2), brute_force_nll(some, 4, 2)
    assert math.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
    assert got > forward_nll(lat, 4, 2)
    allinf = np.full((3, 2, 2), -np.inf)
    assert forward_nll(allinf, 3, 1) == math.inf


def _model_without_device(monkeypatch, transducer=True):
    """An ESPnetASRModel shell whose every path to the shared library fails the test."""
    from espnet_amd import lib as L
    from espnet_amd.asr.espnet_model import ESPnetASRModel

    def boom(*a, **k):
        raise AssertionError("the library was reached before the host checks")

    monkeypatch.setattr(L, "load", boom)
    monkeypatch.setattr(L, "require_gpu", boom)
    m = ESPnetASRModel.__new__(ESPnetASRModel)
    torch.nn.Module.__init__(m)
    m.use_transducer_decoder, m.vocab_size, m.blank_id = transducer, 10, 0
    m.decoder = m.joint_network = None
    return m


def test_model_refusals_need_no_device(monkeypatch):
    enc, lens = torch.zeros(2, 3, 8), torch.tensor([3, 3])
    with pytest.raises(RuntimeError, match="joint network"):
        _model_without_device(monkeypatch, transducer=False).transducer_nll(enc, lens, torch.tensor([[1]]), torch.tensor([1]))
    m = _model_without_device(monkeypatch)
    with pytest.raises(ValueError, match="<blank>"):
        m.transducer_nll(enc, lens, torch.tensor([[1, 0], [1, 2]]), torch.tensor([2, 2]))
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        m.transducer_nll(enc, lens, torch.tensor([[1, 10], [1, 2]]), torch.tensor([2, 2]))
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        m.transducer_nll(enc, lens, torch.tensor([[1, -1]]), torch.tensor([2]), mem_of=[1])
    with pytest.raises(ValueError, match="ys_pad_lens"):
        m.transducer_nll(enc, lens, torch.tensor([[1, 2]]), torch.tensor([3]))
    with pytest.raises(ValueError, match="encoder_out_lens"):
        m.transducer_nll(enc, torch.tensor([3, 4]), torch.tensor([[1, 2]]), torch.tensor([2]))
    with pytest.raises(ValueError, match="need mem_of"):
        m.transducer_nll(enc, lens, torch.tensor([[1], [2], [3]]), torch.tensor([1, 1, 1]))
    with pytest.raises(ValueError, match="mem_of"):
        m.transducer_nll(enc, lens, torch.tensor([[1], [2], [3]]), torch.tensor([1, 1, 1]), mem_of=[0, 1, 2])
    with pytest.raises(ValueError, match="batch_size"):
        m.batchify_transducer_nll(enc, lens, torch.tensor([[1], [2]]), torch.tensor([1, 1]), batch_size=0)
    # a blank behind a row's length is padding: the host checks pass and the device is asked for
    with pytest.raises(AssertionError, match="library was reached"):
        m.transducer_nll(enc, lens, torch.tensor([[1, 0], [1, 1]]), torch.tensor([1, 2]))


def _bare_s2t(transducer=True):
    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.text.token_id_converter import TokenIDConverter

    def no_encode(*a, **k):
        raise AssertionError("encoded before the checks")

    model = types.SimpleNamespace(blank_id=0, sos=3, eos=3, vocab_size=4, use_transducer_decoder=transducer,
                                  encode_device=no_encode)
    s2t = Speech2Text.__new__(Speech2Text)
    s2t.asr_model, s2t.tokenizer, s2t.device = model, None, "cuda"
    s2t.converter = TokenIDConverter(token_list=["<blank>", "a", "<unk>", "<sos/eos>"])
    s2t.ctc_greedy, s2t.beam_search, s2t.ngram, s2t.lm_model = False, None, None, None
    return s2t


def test_batch_transducer_nll_refusals_need_no_device():
    speech = torch.zeros(1, 1600)
    with pytest.raises(RuntimeError, match="joint network"):
        _bare_s2t(transducer=False).batch_transducer_nll(speech, [1600], [[1]])
    s2t = _bare_s2t()
    with pytest.raises(ValueError, match="transcript entries"):
        s2t.batch_transducer_nll(speech, [1600], [[1], [2]])
    with pytest.raises(ValueError, match="<blank>"):
        s2t.batch_transducer_nll(speech, [1600], [[[1], [1, 0]]])
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        s2t.batch_transducer_nll(speech, [1600], [[1, 7]])
    with pytest.raises(ValueError, match="tokenizer"):
        s2t.batch_transducer_nll(speech, [1600], ["a a"])


def test_the_other_scorers_still_refuse_a_transducer_model():
    s2t = _bare_s2t()
    with pytest.raises(RuntimeError, match="transducer"):
        s2t.batch_rescore(torch.zeros(1, 1600), [1600], [[1]])


def test_signatures_are_bound():
    import ctypes as C

    from espnet_amd import lib as L

    res, args = L._SIGNATURES["em_transducer_lattice_logp"]
    assert res is C.c_int and len(args) == 16 and args[14] is C.c_size_t and args[4] is C.c_int32
    assert isinstance(args[1], type(C.POINTER(L.EmTransducerWeights)))
    res, args = L._SIGNATURES["em_transducer_lattice_logp_workspace_bytes"]
    assert res is C.c_size_t and len(args) == 5
    res, args = L._SIGNATURES["em_transducer_seq_nll"]
    assert res is C.c_int and len(args) == 10 and args[0] is C.c_void_p and args[2] is C.c_int32
    assert L._SIGNATURES["em_transducer_seq_nll_max_tokens"] == (C.c_int32, [])
