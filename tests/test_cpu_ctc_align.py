"""CTC forced alignment without a GPU: the CPU restatement of the contract (tests/ctc_align_ref.py) against brute-force
enumeration, the two tie fixtures of the contract, the host-side checks (which raise before any library call) and the
bindings."""
import random
import types

import pytest
import torch

from tests.ctc_align_ref import brute_force_best, collapse, feasible, forced_align_ref


def _cases():
    rng = random.Random(7)
    out = []
    for T in range(1, 7):
        for L in range(0, 4):
            for rep in range(3):
                y = [rng.choice([1, 2]) for _ in range(L)]
                if feasible(T, y):
                    out.append((T, y, 100 * T + 10 * L + rep))
    return out


CASES = _cases()


def test_restatement_matches_brute_force():
    """V = 3, T <= 6, L <= 3, repeated tokens included: the path collapses to y, sums to `total`, and `total` is the
    maximum over ALL label sequences that collapse to y."""
    assert len(CASES) >= 40 and any(len(y) >= 2 and y[0] == y[1] for _, y, _ in CASES)
    for T, y, seed in CASES:
        lp = torch.log_softmax(torch.randn(T, 3, generator=torch.Generator().manual_seed(seed)), dim=-1)
        r = forced_align_ref(lp, y, blank=0)
        assert collapse(r["align"].tolist(), 0) == y, (T, y)
        acc = r["frame_lp"][0].clone()
        for t in range(1, T):
            acc = acc + r["frame_lp"][t]
        assert torch.equal(acc, r["total"]), (T, y)
        best = brute_force_best(lp, y, 0)
        assert best is not None and torch.equal(best, r["total"]), (T, y, float(best), float(r["total"]))
        for i in range(len(y)):
            s, e = int(r["tok_start"][i]), int(r["tok_end"][i])
            assert 0 <= s < e <= T and r["align"][s:e].tolist() == [y[i]] * (e - s)


@pytest.mark.parametrize("y, T, want", [([1, 2], 5, [1, 2, 2, 2, 2]), ([1, 1], 4, [1, 0, 1, 1])])
def test_tie_fixtures_on_uniform_log_probs(y, T, want):
    """All paths score the same: the smallest move wins every tie, and the path ends in S-2 unless S-1 is strictly
    better - so tokens start as early as they can and the last token runs to the end."""
    lp = torch.full((T, 3), float(torch.log(torch.tensor(1.0 / 3.0))))
    assert forced_align_ref(lp, y, 0)["align"].tolist() == want


def test_infeasible_rows_raise_in_the_restatement():
    lp = torch.zeros(2, 3)
    with pytest.raises(ValueError):
        forced_align_ref(lp, [1, 1], 0)  # a repeat needs a blank between: 3 frames
    with pytest.raises(ValueError):
        forced_align_ref(lp, [1, 0], 0)


def _ctc_without_library(monkeypatch):
    """A CTC head whose every path to the shared library fails the test."""
    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC

    def boom(*a, **k):
        raise AssertionError("the library was reached before the host checks")

    monkeypatch.setattr(L, "load", boom)
    monkeypatch.setattr(L, "require_gpu", lambda *a, **k: None)
    return CTC(odim=10, encoder_output_size=8)


def test_host_checks_raise_before_any_library_call(monkeypatch):
    ctc = _ctc_without_library(monkeypatch)
    enc = torch.zeros(1, 3, 8)
    with pytest.raises(ValueError, match="frames cannot carry"):
        ctc.forced_align_device(enc, [3], [[1, 2, 3, 4]], [4], 0)
    with pytest.raises(ValueError, match="frames cannot carry"):
        ctc.forced_align_device(enc, [3], [[1, 1, 2]], [3], 0)  # 3 tokens + 1 repeat = 4 frames
    with pytest.raises(ValueError, match="blank"):
        ctc.forced_align_device(enc, [3], [[1, 0]], [2], 0)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        ctc.forced_align_device(enc, [3], [[1, 10]], [2], 0)
    with pytest.raises(ValueError, match="rows"):
        ctc.forced_align_device(enc, [3, 3], [[1]], [1], 0)
    with pytest.raises(AssertionError, match="library was reached"):  # a good row does go on to the library
        ctc.forced_align_device(enc, [3], [[1, 2]], [2], 0)


def test_speech2text_target_checks(monkeypatch):
    """A string without a tokenizer, blank and <sos/eos> in the target, a model without CTC head: ValueError, and
    nothing is encoded."""
    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.text.token_id_converter import TokenIDConverter

    tokens = ["<blank>", "a", "<unk>", "<sos/eos>"]

    def no_encode(*a, **k):
        raise AssertionError("encoded before the checks")

    model = types.SimpleNamespace(blank_id=0, sos=3, eos=3, ctc=object(), encode_device=no_encode)
    s2t = Speech2Text.__new__(Speech2Text)
    s2t.asr_model, s2t.tokenizer, s2t.converter, s2t.device = model, None, TokenIDConverter(token_list=tokens), "cuda"
    speech = torch.zeros(1, 1600)
    with pytest.raises(ValueError, match="tokenizer"):
        s2t.batch_align(speech, [1600], ["a b"])
    with pytest.raises(ValueError, match="<blank>"):
        s2t.batch_align(speech, [1600], [[1, 0, 2]])
    with pytest.raises(ValueError, match="<sos/eos>"):
        s2t.align(speech[0], [1, 3])
    with pytest.raises(ValueError, match="transcripts"):
        s2t.batch_align(speech, [1600], [[1], [2]])
    model.ctc = None
    with pytest.raises(ValueError, match="CTC head"):
        s2t.batch_align(speech, [1600], [[1]])
    assert s2t._target_ids(torch.tensor([1, 2])) == [1, 2]


def test_signatures_are_bound():
    import ctypes as C

    from espnet_amd import lib as L

    res, args = L._SIGNATURES["em_ctc_forced_align"]
    assert res is C.c_int and len(args) == 18 and args[16] is C.c_size_t
    res, args = L._SIGNATURES["em_ctc_forced_align_workspace_bytes"]
    assert res is C.c_size_t and args == [C.c_int32] * 3
    assert L._SIGNATURES["em_ctc_forced_align_max_tokens"] == (C.c_int32, [])
