"""Shallow fusion in the transducer's beam search without a GPU: the float64 restatement tests/transducer_lm_ref.py held
to a literal transcription of the reference loop, its LM step held to torch.nn.LSTM / GRU, the new C-ABI entries, and
what BeamSearchTransducer(lm=...) and Speech2Text refuse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import transducer_lm_ref as LR
from tests import transducer_ref as R
from tests.test_cpu_transducer_beam import random_logits
from tests.transducer_beam_margins import beam_search_margins

REPO = Path(__file__).resolve().parent.parent
NEW = ("em_transducer_lm_step", "em_transducer_beam_search_lm", "em_transducer_beam_workspace_bytes_lm")


def test_new_symbols_are_declared_bound_and_exported():
    from espnet_amd import lib as L

    hdr = (REPO / "include" / "espnet_amd.h").read_text()
    declared = set(re.findall(r"\b(em_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    table = subprocess.run(["nm", "-D", "--defined-only", str(L.library_path())], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in table.splitlines() if ln.strip()}
    for name in NEW:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name) and name in exported, name
    assert "typedef struct EmTransducerLmWeights" in hdr
    res, args = L._SIGNATURES["em_transducer_beam_search_lm"]
    old = L._SIGNATURES["em_transducer_beam_search"][1]
    assert res is C.c_int and len(args) == len(old) + 3 and args[3] is C.c_double and args[-2] is C.c_size_t
    assert L._SIGNATURES["em_transducer_beam_workspace_bytes_lm"][0] is C.c_size_t
    assert len(L._SIGNATURES["em_transducer_lm_step"][1]) == 11
    # the struct as the header lays it out: six int32, then four pointers
    names = [n for n, _ in L.EmTransducerLmWeights._fields_]
    assert names == ["kind", "vocab", "nhid", "d", "embed_unit", "num_layers", "embed", "rnn", "out_w", "out_b"]
    assert L.EmTransducerLmWeights.embed.offset == 24 and C.sizeof(L.EmTransducerLmWeights) == 56


# ---------------------------------------------------------------------- the restatement's LM step is torch's
@pytest.mark.parametrize("kind,nlayers,unit,nhid", [("lstm", 1, 8, 8), ("gru", 2, 6, 10), ("lstm", 2, 5, 7)])
def test_lm_step_restates_torch_rnn(kind, nlayers, unit, nhid):
    """`lm_step` over sos and three labels against torch.nn.Embedding -> LSTM / GRU -> Linear -> log_softmax in float64."""
    V = 11
    torch.manual_seed(3)
    emb = torch.nn.Embedding(V, unit).double()
    rnn = getattr(torch.nn, kind.upper())(unit, nhid, nlayers, batch_first=True).double()
    out = torch.nn.Linear(nhid, V).double()
    sd = {"encoder.weight": emb.weight, "decoder.weight": out.weight, "decoder.bias": out.bias}
    sd.update({"rnn." + k: v for k, v in rnn.state_dict().items()})
    p = LR.LmParams(sd, kind)
    toks = [p.sos, 4, 1, 9]
    with torch.no_grad():
        hs, _ = rnn(emb(torch.tensor([toks])))
        want = torch.log_softmax(out(hs[0]), -1)
    state = p.init_state()
    for i, tk in enumerate(toks):
        logp, state, _ = LR.lm_step(p, tk, state)
        assert float((logp - want[i]).abs().max()) < 1e-12
    fn = LR.model_lm_fn(p)
    assert np.allclose(fn((0, 4, 1, 9)), want[3].numpy(), atol=1e-12) and np.allclose(fn((0,)), want[0].numpy(), atol=1e-12)


# ---------------------------------------------------------------------- the restatement is the reference's loop
def _stateful_lm(seed, V, levels=None):
    """An LM whose state is the tuple of the tokens it has read: (lm_score(token, state), lm_fn(yseq)) giving the same
    rows, the first as the reference calls its LM, the second as the restatement does."""
    def row(read):
        g = np.random.default_rng([seed, 7, len(read)] + list(read))
        x = g.standard_normal(V)
        if levels:
            x = np.round(x * (levels / 4.0)) * (4.0 / levels)
        return R.log_softmax(torch.as_tensor(x)).numpy()

    def lm_score(token, state):
        read = (state or ()) + (token,)
        return row(read), read

    return lm_score, (lambda y: row((V - 1,) + tuple(y[1:])))


@pytest.mark.parametrize("lm_weight", [0.3, 1.0])
@pytest.mark.parametrize("levels", [None, 2])
@pytest.mark.parametrize("V,T,beam", [(3, 6, 2), (4, 5, 4), (8, 6, 4), (8, 4, 10), (6, 1, 3)])
def test_restatement_equals_the_reference_loop(V, T, beam, levels, lm_weight):
    """Random and quantised (exact ties abound) joint logits and LM rows: the same lists with equal - not close - scores."""
    differs = 0
    for seed in range(4):
        fn = random_logits(seed, V, levels)
        lm_score, lm_fn = _stateful_lm(seed, V, levels)
        for score_norm in (True, False):
            got = LR.beam_search_lm_from_logits(fn, lm_fn, lm_weight, T, V, beam, nbest=64, score_norm=score_norm)
            want = LR.reference_loop(fn, lm_score, lm_weight, T, V, beam, nbest=64, score_norm=score_norm)
            assert [y for _, y in got] == [y for _, y in want], (seed, score_norm)
            assert [s for s, _ in got] == [s for s, _ in want]
            marg, _, _ = LR.beam_search_lm_margins(fn, lm_fn, lm_weight, T, V, beam, 64, score_norm=score_norm)
            assert marg == got
        plain = R.beam_search_from_logits(fn, T, V, beam, nbest=64)
        differs += [y for _, y in plain] != [y for _, y in LR.beam_search_lm_from_logits(fn, lm_fn, lm_weight, T, V, beam, nbest=64)]
    assert differs >= 1 or T == 1  # the LM term does change the lists


def test_all_tied_logits_and_zero_weight():
    """All-equal joint logits and LM rows (every rank round and pop an exact tie): as the reference loop; and with
    lm_weight 0.0 the restatement is, bit for bit, the search without an LM, margins included."""
    flat = lambda t, y: np.zeros(4)  # noqa: E731
    flat_row = R.log_softmax(torch.zeros(4, dtype=torch.float64)).numpy()
    got = LR.beam_search_lm_from_logits(flat, lambda y: flat_row, 0.5, 3, 4, 3, nbest=16)
    assert got == LR.reference_loop(flat, lambda tk, st: (flat_row, None), 0.5, 3, 4, 3, nbest=16)
    for seed in range(3):
        fn = random_logits(seed, 6)
        _, lm_fn = _stateful_lm(seed, 6)
        assert LR.beam_search_lm_from_logits(fn, lm_fn, 0.0, 4, 6, 3, nbest=16) == R.beam_search_from_logits(fn, 4, 6, 3, nbest=16)
        a = LR.beam_search_lm_margins(fn, lm_fn, 0.0, 4, 6, 3, 3)
        b = beam_search_margins(fn, 4, 6, 3, 3)
        assert a == b


def test_margins_count_the_lm_term_with_its_weight():
    """The LM term enters the margins as lm_weight x the LM row: rows scaled by 4 at a quarter of the weight give the same
    lists and the same margins (4 and 1/4 are exact in binary, so the products are the same numbers); and a hand-built
    frame - V = 3, beam 1, one label far ahead on the joint row - whose end test is decided by the LM term alone."""
    for seed in range(3):
        fn = random_logits(seed, 6)
        _, lm_fn = _stateful_lm(seed, 6)
        a = LR.beam_search_lm_margins(fn, lm_fn, 0.5, 4, 6, 3, 3)
        b = LR.beam_search_lm_margins(fn, lambda y: 4.0 * lm_fn(y), 0.125, 4, 6, 3, 3)
        assert a == b and a[0] is not None and np.isfinite(a[1])
    # blank 0.4, label 1 0.5, label 2 0.1: without an LM the child [0, 1] (log 0.5) beats the kept [0] (log 0.4) and the
    # frame goes on; with the LM row giving label 1 log 0.25 at weight 1 the child stands at log 0.125 and the frame ends
    # after one expansion, with the end-test margin (log 0.4 - log 0.125) over its 1 + 1 + 1 terms
    logits = lambda t, y: np.log(np.array([0.4, 0.5, 0.1]))  # noqa: E731
    lm = lambda y: np.log(np.array([0.5, 0.25, 0.25]))  # noqa: E731
    res, margin, most = LR.beam_search_lm_margins(logits, lm, 1.0, 1, 3, 1, 1)
    assert most == 1 and res[0][1] == [0]
    assert abs(margin - min((np.log(0.4) - np.log(0.125)) / 3, (np.log(0.5) - np.log(0.1)) / 2)) < 1e-12
    _, _, most0 = beam_search_margins(logits, 1, 3, 1, 1)
    assert most0 > 1


# ---------------------------------------------------------------------- refusals
def _parts(V=10):
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.transducer.joint_network import JointNetwork

    return TransducerDecoder(V, hidden_size=16), JointNetwork(V, 64, 16, joint_space_size=16)


def test_refusals_name_their_option():
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer, beam_limits
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from espnet_amd.lm.transformer_lm import TransformerLM

    dec, jn = _parts()
    with pytest.raises(NotImplementedError, match="lm"):
        BeamSearchTransducer(dec, jn, beam_size=2, lm=object())
    with pytest.raises(NotImplementedError, match=r"lm.*TransformerLM"):
        BeamSearchTransducer(dec, jn, beam_size=2, lm=TransformerLM(10, att_unit=64, head=1, unit=64, layer=1))
    with pytest.raises(NotImplementedError, match=r"lm.*rnn_tanh"):
        BeamSearchTransducer(dec, jn, beam_size=2, lm=SequentialRNNLM(10, unit=16, nlayers=1, rnn_type="rnn_tanh"))
    lim = beam_limits()["beam"]
    with pytest.raises(NotImplementedError, match=rf"lm.*beam_size={lim + 1}.*{lim}"):
        BeamSearchTransducer(dec, jn, beam_size=lim + 1, lm=SequentialRNNLM(10, unit=16, nlayers=1))
    with pytest.raises(ValueError, match="lm"):
        BeamSearchTransducer(dec, jn, beam_size=2, lm=SequentialRNNLM(11, unit=16, nlayers=1))
    for kind in ("lstm", "gru"):  # accepted, with unit != nhid and tied weights
        bs = BeamSearchTransducer(dec, jn, beam_size=lim, lm=SequentialRNNLM(10, unit=16, nhid=24, nlayers=2, rnn_type=kind),
                                  lm_weight=0.3)
        assert bs.lm_weight == 0.3 and bs.sos == 9
    BeamSearchTransducer(dec, jn, beam_size=2, lm=SequentialRNNLM(10, unit=16, nlayers=1, tie_weights=True))


def test_greedy_with_an_lm_logs_that_it_is_unused(caplog):
    import logging

    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM

    dec, jn = _parts()
    with caplog.at_level(logging.INFO, logger="espnet_amd.asr.transducer.beam_search_transducer"):
        BeamSearchTransducer(dec, jn, beam_size=1, lm=SequentialRNNLM(10, unit=16, nlayers=1))
    assert sum("does not use the lm" in r.getMessage() for r in caplog.records) == 1


def test_workspace_query_refuses_what_the_search_refuses():
    """em_transducer_beam_workspace_bytes_lm runs without a GPU: NULL for the LM is the query without one, an LM adds its
    slots' states, and shapes outside one call - the LM's too - return 0."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    w = L.EmTransducerWeights()
    w.kind, w.vocab, w.nhid, w.d, w.num_layers, w.joint, w.jp, w.blank = L.EM_LM_LSTM, 50, 64, 64, 1, 64, 64, 0
    w.embed = w.lin_dec = w.lin_out = w.out_b = 64  # (non-NULL; the query reads the shape only)
    w.rnn = C.cast(C.pointer(L.EmRnnLayer()), C.POINTER(L.EmRnnLayer))

    def lm(**kw):
        m = L.EmTransducerLmWeights()
        m.kind, m.vocab, m.nhid, m.d, m.embed_unit, m.num_layers = L.EM_LM_LSTM, 50, 200, 256, 128, 2
        m.embed = m.out_w = m.out_b = 64
        m.rnn = C.cast(C.pointer(L.EmRnnLayer()), C.POINTER(L.EmRnnLayer))
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    lib = L.load()
    q, q0 = lib.em_transducer_beam_workspace_bytes_lm, lib.em_transducer_beam_workspace_bytes
    lim = beam_limits()["beam"]
    plain = int(q0(L.EM_BF16, C.byref(w), 5, 16, 4))
    assert plain > 0 and int(q(L.EM_BF16, C.byref(w), None, 5, 16, 4)) == plain
    with_lm = int(q(L.EM_BF16, C.byref(w), C.byref(lm()), 5, 16, 4))
    slots = 5 * 256 * 2 * 256 * (2 + 4)  # B x 256 slots x layers x d x (act + f32 master state)
    assert slots <= with_lm - plain <= slots + 64 * 1024  # (+ the per-step rows: two state sets, tokens, one V-wide row)
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm()), 64, 16, lim)) > 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm()), 65, 16, 4)) == 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm()), 5, 16, lim + 1)) == 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm()), 5, 0, 4)) == 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm(vocab=51)), 5, 16, 4)) == 0  # another vocabulary
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm(d=250)), 5, 16, 4)) == 0  # not padded
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm(embed_unit=96)), 5, 16, 4)) == 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm(kind=L.EM_LM_RNN_TANH)), 5, 16, 4)) == 0
    assert int(q(L.EM_F32, C.byref(w), C.byref(lm(out_w=None)), 5, 16, 4)) == 0


def test_speech2text_checks_the_beam_before_it_opens_the_lm(tmp_path):
    """A transducer model with lm_train_config at a beam above the walk's limit: NotImplementedError naming the option, the
    beam and the limit, raised before the (missing) LM file is looked at; ngram_file keeps raising."""
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits
    from espnet_amd.bin import asr_inference as A

    class _Model:
        use_transducer_decoder = True

    lim = beam_limits()["beam"]
    with pytest.raises(NotImplementedError, match=rf"lm_train_config.*beam_size={lim + 4}.*{lim}"):
        A.check_transducer_lm(_Model(), lm_train_config=str(tmp_path / "missing.yaml"), ngram_file=None, beam_size=lim + 4)
    with pytest.raises(NotImplementedError, match="ngram_file"):
        A.check_transducer_lm(_Model(), lm_train_config=None, ngram_file="x.arpa", beam_size=4)
    A.check_transducer_lm(_Model(), lm_train_config=str(tmp_path / "missing.yaml"), ngram_file=None, beam_size=lim)
    A.check_transducer_lm(_Model(), lm_train_config=None, ngram_file=None, beam_size=lim + 4)
