"""CTC likelihood of given transcripts without a GPU: the float64 restatement of the contract (tests/ctc_nll_ref.py)
pinned against torch's ctc_loss, against brute-force enumeration and against the Viterbi restatement; the host-side
checks of CTC.nll / nll_device and batch_rescore's refusals (which raise before any library call), and the binding."""
import math
import random
import types

import pytest
import torch

from tests.ctc_align_ref import feasible, forced_align_ref
from tests.ctc_nll_ref import brute_force_nll, ctc_nll_ref

V = 50


def synth_lp(T, seed, vocab=V):
    return torch.log_softmax(torch.randn(T, vocab, generator=torch.Generator().manual_seed(seed)), dim=-1)


def synth_y(L, seed, distinct=False, vocab=V):
    g = torch.Generator().manual_seed(1000 + seed)
    if distinct:
        return (torch.randperm(vocab - 1, generator=g)[:L] + 1).tolist()
    return torch.randint(1, vocab, (L,), generator=g).tolist()


def tiny_rows():
    """The tiny ragged batch of the device test, infeasible rows included: (T, y)."""
    a = 7
    return [(1, []), (1, [3]), (5, []), (2, [4]), (7, synth_y(7, 1, distinct=True)), (5, [a, a, a]), (3, [9]),
            (17, synth_y(5, 2)), (2, [a, a]), (1, [3, 4])]


def test_restatement_matches_torch_ctc_loss_in_float64():
    for i, (T, y) in enumerate(tiny_rows() + [(40, synth_y(12, 3)), (60, [5, 5, 6, 6, 6, 7])]):
        lp = synth_lp(T, 31 * i + T).to(torch.float64)
        want = torch.nn.functional.ctc_loss(lp.unsqueeze(1), torch.tensor([y], dtype=torch.long).reshape(1, len(y)),
                                            torch.tensor([T]), torch.tensor([len(y)]), blank=0, reduction="none",
                                            zero_infinity=False)[0]
        got = ctc_nll_ref(lp, y)
        if not feasible(T, y):
            assert got == math.inf and float(want) == math.inf, (T, y)
        else:
            assert abs(got - float(want)) <= 1e-12 * max(abs(float(want)), 1.0), (T, y, got, float(want))
        if not y:
            assert got == pytest.approx(-float(lp[:, 0].sum()), rel=1e-14)


def test_restatement_matches_brute_force():
    """V = 3, T <= 5, L <= 2, a repeated token and infeasible rows included: -log of the summed probability of ALL label
    sequences that collapse to y."""
    rng = random.Random(11)
    n, repeats, inf = 0, 0, 0
    for T in range(1, 6):
        for L in range(0, 3):
            for rep in range(3):
                y = [rng.choice([1, 2]) for _ in range(L)]
                if L == 2 and rep == 0:
                    y = [1, 1]
                lp = torch.log_softmax(torch.randn(T, 3, generator=torch.Generator().manual_seed(100 * T + 10 * L + rep)),
                                       dim=-1).to(torch.float64)
                got, want = ctc_nll_ref(lp, y), brute_force_nll(lp, y)
                if feasible(T, y):
                    assert abs(got - want) <= 1e-12 * max(abs(want), 1.0), (T, y, got, want)
                else:
                    assert got == math.inf and want == math.inf, (T, y)
                    inf += 1
                n += 1
                repeats += L == 2 and y[0] == y[1]
    assert n == 45 and repeats >= 5 and inf >= 3


def test_forward_value_is_never_worse_than_the_viterbi_path():
    for i, (T, y) in enumerate(tiny_rows() + [(130, synth_y(33, 33)), (249, synth_y(60, 9))]):
        if not feasible(T, y):
            continue
        lp = synth_lp(T, 31 * i + T)
        total = float(forced_align_ref(lp, y)["total"])
        nll = ctc_nll_ref(lp, y)
        assert nll <= -total + 1e-5 * max(abs(total), 1.0), (T, y, nll, -total)  # (total is an f32 sum)
        if T == 1:
            assert nll == pytest.approx(-total, rel=1e-6)  # one frame: one path


def test_empty_and_minus_inf_rows():
    assert ctc_nll_ref(torch.zeros(0, 3), []) == math.inf  # no frame: no path
    lp = synth_lp(6, 5)
    lp[:, 4] = float("-inf")
    assert ctc_nll_ref(lp, [4]) == math.inf
    assert math.isfinite(ctc_nll_ref(lp, [3]))
    with pytest.raises(ValueError):
        ctc_nll_ref(lp, [1, 0])


def _ctc_without_library(monkeypatch):
    """A CTC head whose every path to the shared library fails the test."""
    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC

    def boom(*a, **k):
        raise AssertionError("the library was reached before the host checks")

    monkeypatch.setattr(L, "load", boom)
    monkeypatch.setattr(L, "require_gpu", lambda *a, **k: None)
    return CTC(odim=10, encoder_output_size=8, compute_dtype="float32")


def test_host_checks_raise_before_any_library_call(monkeypatch):
    ctc = _ctc_without_library(monkeypatch)
    enc = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="blank"):
        ctc.nll(enc, torch.tensor([3, 3]), torch.tensor([[1, 0], [1, 2]]), torch.tensor([2, 2]))
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        ctc.nll(enc, [3, 3], [[1, 10], [1, 2]], [2, 2])
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        ctc.nll_device(enc, [3, 3], [[1, -1]], [2], 0, mem_of=[1])
    with pytest.raises(ValueError, match="entries"):
        ctc.nll_device(enc, [3], [[1], [2]], [1, 1], 0)
    with pytest.raises(ValueError, match="outside its row"):
        ctc.nll_device(enc, [3, 4], [[1], [2]], [1, 1], 0)  # 4 frames of 3
    with pytest.raises(ValueError, match="outside its row"):
        ctc.nll_device(enc, [3, 3], [[1], [2]], [1, 2], 0)
    with pytest.raises(ValueError, match="mem_of"):
        ctc.nll_device(enc, [3, 3], [[1], [2], [3]], [1, 1, 1], 0, mem_of=[0, 1, 2])
    with pytest.raises(ValueError, match="need mem_of"):
        ctc.nll_device(enc, [3, 3], [[1], [2], [3]], [1, 1, 1], 0)
    # a blank behind a row's length is padding, and too few frames are no error (the value is +inf): both reach the library
    with pytest.raises(AssertionError, match="library was reached"):
        ctc.nll(enc, [3, 3], [[1, 0], [1, 1]], [1, 2], blank_idx=0)
    with pytest.raises(AssertionError, match="library was reached"):
        ctc.nll_device(enc, [3, 1], [[1, 2, 3, 4], [5, 5, 0, 0], [6, 0, 0, 0]], [4, 2, 1], 0, mem_of=[0, 1, 1])


def _bare_s2t(**kw):
    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.text.token_id_converter import TokenIDConverter

    def no_encode(*a, **k):
        raise AssertionError("encoded before the checks")

    model = types.SimpleNamespace(blank_id=0, sos=3, eos=3, ctc=object(), encode_device=no_encode)
    s2t = Speech2Text.__new__(Speech2Text)
    s2t.asr_model, s2t.tokenizer, s2t.device = model, None, "cuda"
    s2t.converter = TokenIDConverter(token_list=["<blank>", "a", "<unk>", "<sos/eos>"])
    s2t.ctc_greedy, s2t.beam_search, s2t.ngram, s2t.lm_model = False, None, None, None
    for k, v in kw.items():
        setattr(s2t, k, v)
    return s2t


def test_batch_rescore_refusals_need_no_device():
    speech = torch.zeros(1, 1600)
    with pytest.raises(RuntimeError, match="ctc_greedy"):
        _bare_s2t(ctc_greedy=True).batch_rescore(speech, [1600], [[1]])
    with pytest.raises(RuntimeError, match="transducer"):
        _bare_s2t().batch_rescore(speech, [1600], [[1]])
    search = types.SimpleNamespace(scorers=dict(decoder=None, ctc=None), weights=dict(decoder=0.7, ctc=0.3))
    with pytest.raises(NotImplementedError, match="ngram_file"):
        _bare_s2t(beam_search=search, ngram=object()).batch_rescore(speech, [1600], [[1]])
    s2t = _bare_s2t(beam_search=search)
    with pytest.raises(ValueError, match="transcript entries"):
        s2t.batch_rescore(speech, [1600], [[1], [2]])
    with pytest.raises(ValueError, match="<blank>"):
        s2t.batch_rescore(speech, [1600], [[[1], [1, 0]]])
    with pytest.raises(ValueError, match="tokenizer"):
        s2t.batch_rescore(speech, [1600], ["a a"])


def test_signature_is_bound():
    import ctypes as C

    from espnet_amd import lib as L

    res, args = L._SIGNATURES["em_ctc_seq_nll"]
    assert res is C.c_int and len(args) == 13 and args[1] is C.c_int32 and args[0] is C.c_void_p
