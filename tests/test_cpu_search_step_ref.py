"""Pins tests/search_step_ref.py (the float64 restatement of one device label step) on the CPU: driven from <sos> to the
end on its own, with the full scorers' rows taken from the oracle's decoder / LM (float32, promoted), it must return
`oracle.beam_search.beam_search`'s n-best - the same token sequences, scores within the oracle's float32 round-off.

The bound.  The restatement is float64 on float32 inputs, so the difference is the ORACLE's own rounding.  A hypothesis'
score is a sum over its L label steps; the CTC part telescopes (sum of psi_i - psi_{i-1}), so what remains is (a) the
error of the last log psi, whose forward variables come out of a recurrence of up to T sequential float32
log-add-exp + add steps, each rounding to half an ulp of the variable's magnitude: <= T/2 ulp, and (b) two float32 adds
per step into the running sums (the scorer's own and the total), each <= 1/2 ulp twice over: <= 2 L ulp.  With R the
largest magnitude of any log quantity of the search (log psi, totals): |score - oracle| <= (T/2 + 2 L) * ulp32(R).
At T = 40, L = 40, R = 200 that is 1.5e-3 - the size of the 2e-3 the GPU tests grant a whole f32 search."""
import json

import numpy as np
import pytest
import torch

from oracle import beam_search as ob
from oracle import conformer as oc
from tests import search_step_ref as ref
from tests.helpers import golden_speech, golden_state_dict, hparams, load_golden


def bound(T, L, R):
    return (T / 2 + 2 * L) * float(np.spacing(np.float32(R)))


def check_nbest(mine, want, T, R, keys):
    assert len(mine) == len(want), (len(mine), len(want))
    # the oracle's list is sorted by float32 scores: compare as sets of token sequences, then the order where the
    # oracle's own gap exceeds the bound
    by_seq = {tuple(h["yseq"]): h for h in mine}
    worst = 0.0
    for w in want:
        assert tuple(w["yseq"]) in by_seq, w["yseq"]
        h = by_seq[tuple(w["yseq"])]
        tol = bound(T, len(w["yseq"]), R)
        worst = max(worst, abs(h["score"] - w["score"]) / tol)
        assert abs(h["score"] - w["score"]) <= tol, (w["yseq"], h["score"], w["score"], tol)
        for k in keys:
            assert abs(h["scores"][k] - w["scores"][k]) <= tol, (k, h["scores"][k], w["scores"][k], tol)
    for a, b, ha in zip(want, want[1:], mine):
        if a["score"] - b["score"] > 2 * bound(T, len(a["yseq"]), R):
            assert ha["yseq"] == a["yseq"]
    return worst


@pytest.mark.parametrize("name", ["tiny_beam5", "tiny_beam4_early_eos", "tiny_beam4_minlen", "tiny_beam5_lm"])
def test_restatement_returns_the_oracles_nbest_on_the_golden_models(name):
    g = load_golden(name)
    sd = golden_state_dict(g)
    lm_kw = {}
    if "lm_conf" in g:
        from oracle.weights import recipe_state_dict

        shapes = {"lm." + k: tuple(v) for k, v in json.loads(str(g["lm_state_shapes"])).items()}
        sd.update(recipe_state_dict(shapes, int(g["wseed"]), skip=()))
        lm_kw = dict(lm_weight=float(g["lm_weight"]), lm_conf=json.loads(str(g["lm_conf"])))
    hp = hparams(g)
    speech, lens = golden_speech(g)
    with torch.no_grad():
        enc, olens = oc.encode(sd, speech, lens, hp["heads"], hp["num_blocks"], hp["n_fft"], hp["win_length"], hp["hop"])
        e = enc[0, : int(olens[0])]
        V = int(g["vocab"])
        dc = g["config"]["decoder_conf"]
        kw = {k: float(g[k]) for k in ("maxlenratio", "minlenratio", "penalty") if k in g}
        want = ob.beam_search(sd, e, dc["attention_heads"], dc["num_blocks"], int(g["beam"]), float(g["ctc_weight"]),
                              sos=V - 1, eos=V - 1, **kw, **lm_kw)
    mine, p, R = ref.run_search(sd, e, dc["attention_heads"], dc["num_blocks"], int(g["beam"]), float(g["ctc_weight"]),
                                **kw, **lm_kw)
    assert len(want) > 0
    worst = check_nbest(mine, want, e.size(0), R, list(want[0]["scores"]))
    print(f"[{name}] {len(want)} hypotheses, S {p['S']}, largest |log quantity| {R:.1f}, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("ctc_weight,penalty", [(1.0, 0.0), (1.0, 0.5), (0.0, 0.0)])
def test_restatement_ctc_only_and_attention_only(ctc_weight, penalty):
    """ctc_weight 1.0: all-vocabulary mode (no pre-beam, no decoder); 0.0: no CTC state at all."""
    g = load_golden("tiny_beam5")
    sd = golden_state_dict(g)
    V = int(g["vocab"])
    dc = g["config"]["decoder_conf"]
    d = g["config"]["encoder_conf"]["output_size"]
    torch.manual_seed(7)
    e = torch.randn(21, d) * 0.7
    with torch.no_grad():
        want = ob.beam_search(sd, e, dc["attention_heads"], dc["num_blocks"], 5, ctc_weight, sos=V - 1, eos=V - 1,
                              penalty=penalty)
    mine, p, R = ref.run_search(sd, e, dc["attention_heads"], dc["num_blocks"], 5, ctc_weight, penalty=penalty)
    assert p["S"] == V and p["NC"] == V and len(want) > 0
    check_nbest(mine, want, e.size(0), max(R, 1.0), list(want[0]["scores"]))
