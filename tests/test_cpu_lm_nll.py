"""Whole-sentence scoring with the language model, the parts that need no GPU: the float64 restatement the GPU tests measure
against (tests/lm_seq_ref.py) agrees with the step oracle, the host functions of ESPnetLanguageModel.nll / batchify_nll and
of the perplexity tool do what espnet2/lm/espnet_model.py and espnet2/bin/lm_calc_perplexity.py state, and the defects the
GPU tests' bounds are meant to catch are larger than those bounds."""
import math

import numpy as np
import pytest
import torch

from oracle.beam_search import TransformerLMOracle
from tests import lm_nll_cases as K
from tests import lm_seq_ref as R


def _sd64(model):
    return {k: v.detach().to(torch.float64) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name", sorted(K.MODELS))
def test_restatement_equals_the_step_oracle(name):
    """nll of the whole-sequence restatement against TransformerLMOracle fed token by token (float64 state dict): 1e-9.
    The sentences of width 65 carry ids 0 inside the first and the third, which no later position may attend."""
    V, heads, pos_enc, _ = K.MODELS[name]
    model = K.build_model(name)
    text, lens = K.make_text(65, V)
    assert (text[0, 1 : lens[0]] == 0).sum() >= 1
    p = R.Params(model.state_dict(), heads, pos_enc is not None)
    got, xl = R.nll(p, text, lens)
    x, t, _ = R.sentence_pair(text, lens, V - 1, V - 1)
    orc = TransformerLMOracle(_sd64(model), heads, K.LAYERS, pos_enc is not None, x.size(1))
    worst = 0.0
    for b in range(3):
        cache = orc.init_cache()
        for j in range(int(xl[b])):
            logp, cache = orc.step(x[b : b + 1, : j + 1], cache)
            worst = max(worst, abs(float(-logp[0, t[b, j]]) - float(got[b, j])))
        assert (got[b, int(xl[b]):] == 0).all()
    assert worst <= 1e-9, worst


def test_sentence_pair_builder():
    from espnet_amd.lm.transformer_lm import build_nll_batch

    text = torch.tensor([[5, 6, 7, 9], [8, 0, 3, 3], [4, 9, 9, 9]])
    lens = torch.tensor([3, 2, 1])
    x, t, xl = build_nll_batch(text, lens, sos=11, eos=12, ignore_id=0)
    assert x.tolist() == [[11, 5, 6, 7], [11, 8, 0, 3], [11, 4, 9, 9]]  # cut to the longest sentence, sos in front
    assert t.tolist() == [[5, 6, 7, 12], [8, 0, 12, 0], [4, 12, 9, 0]]  # eos at the length, ignore_id appended
    assert xl.tolist() == [4, 3, 2]
    # max_length above the longest sentence: the width follows max_length (all four columns of text)
    x, t, xl = build_nll_batch(text, lens, 11, 12, 0, max_length=4)
    assert x.shape == (3, 5) and t.shape == (3, 5) and xl.tolist() == [4, 3, 2]
    assert t[0].tolist() == [5, 6, 7, 12, 0] and x[0].tolist() == [11, 5, 6, 7, 9]
    # ... and beyond the columns there are: the columns there are
    assert build_nll_batch(text, lens, 11, 12, 0, max_length=9)[0].shape == (3, 5)
    with pytest.raises(ValueError):
        build_nll_batch(text, lens, 11, 12, 0, max_length=2)
    # the restatement's own builder is the same function
    for ml in (None, 4):
        for a, b in zip(build_nll_batch(text, lens, 11, 12, 0, ml), R.sentence_pair(text, lens, 11, 12, 0, ml)):
            assert torch.equal(a, b)
    # an empty batch of sentences: one position, sos -> eos
    x, t, xl = build_nll_batch(torch.zeros(2, 0, dtype=torch.long), torch.tensor([0, 0]), 11, 12)
    assert x.tolist() == [[11], [11]] and t.tolist() == [[12], [12]] and xl.tolist() == [1, 1]


def test_batchify_nll_slices():
    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel

    calls = []

    class Stub(ESPnetLanguageModel):
        def __init__(self):
            torch.nn.Module.__init__(self)

        def nll(self, text, text_lengths, max_length=None):
            calls.append((text.clone(), text_lengths.clone(), max_length))
            L = int(text_lengths.max()) if max_length is None else max_length
            return text[:, :1].float().expand(-1, L + 1).clone(), text_lengths + 1

    text = torch.arange(5).unsqueeze(1).expand(5, 7).contiguous()
    lens = torch.tensor([3, 6, 2, 4, 1])
    m = Stub()
    nll, xl = m.batchify_nll(text, lens, batch_size=5)  # fits: one call, no max_length
    assert len(calls) == 1 and calls[0][2] is None and nll.shape == (5, 7)
    calls.clear()
    nll, xl = m.batchify_nll(text, lens, batch_size=2)
    assert [c[0].size(0) for c in calls] == [2, 2, 1] and all(c[2] == 6 for c in calls)
    assert [c[1].tolist() for c in calls] == [[3, 6], [2, 4], [1]]
    assert nll.shape == (5, 7) and nll[:, 0].tolist() == [0, 1, 2, 3, 4] and xl.tolist() == [4, 7, 3, 5, 2]


def test_nll_has_no_cpu_fallback():
    from espnet_amd.lib import EspnetAmdError

    model = K.build_model("h2")
    with pytest.raises(EspnetAmdError):
        model.nll(torch.tensor([[1, 2]]), torch.tensor([2]))
    with pytest.raises(EspnetAmdError):
        model.lm.sequence_nll(torch.tensor([[1, 2]]), torch.tensor([[2, 3]]))


def test_cli_parser_and_files(tmp_path):
    from espnet_amd.bin import lm_calc_perplexity as P

    a = P.get_parser().parse_args(["--output_dir", "o", "--data_path_and_name_and_type", "d/text,text,text_int",
                                   "--train_config", "c.yaml", "--model_file", "m.pth", "--log_base", "2",
                                   "--batch_size", "4", "--dtype", "bfloat16"])
    assert a.log_base == 2.0 and a.batch_size == 4 and a.data_path_and_name_and_type == [("d/text", "text", "text_int")]
    assert a.ngpu == 1 and a.key_file is None and a.seed == 0 and a.num_workers == 1
    assert P.get_parser().parse_args(["--output_dir", "o", "--data_path_and_name_and_type", "a,text,text",
                                      "--log_base", "none"]).log_base is None
    import inspect
    assert list(inspect.signature(P.calc_perplexity).parameters) == [
        "output_dir", "batch_size", "dtype", "ngpu", "seed", "num_workers", "log_level", "data_path_and_name_and_type",
        "key_file", "train_config", "model_file", "log_base", "allow_variable_data_keys"]
    with pytest.raises(NotImplementedError):
        P.calc_perplexity("o", 1, "float32", 2, 0, 1, "INFO", [("a", "text", "text_int")], None, None, None, None, False)

    # readers: ids, and text through the train config's tokenizer
    (tmp_path / "ids").write_text("u1 3 4 5\nu2 6\nu3\n")
    data = P.read_text_entries([(str(tmp_path / "ids"), "text", "text_int")])
    assert {k: v.tolist() for k, v in data.items()} == {"u1": [3, 4, 5], "u2": [6], "u3": []}
    (tmp_path / "txt").write_text("u1 b a x\nu2 a\n")
    import argparse
    args = argparse.Namespace(token_type="word", bpemodel=None, token_list=["<blank>", "<unk>", "a", "b", "<sos/eos>"])
    data_t = P.read_text_entries([(str(tmp_path / "txt"), "text", "text")], args)
    assert {k: v.tolist() for k, v in data_t.items()} == {"u1": [3, 2, 1], "u2": [2]}
    with pytest.raises(RuntimeError):
        P.read_text_entries([(str(tmp_path / "ids"), "speech", "sound")])

    # files: a stub model whose nll is 0.5 per scored token
    class Stub:
        def nll(self, text, text_lengths, max_length=None):
            xl = text_lengths + 1
            scored = torch.arange(int(text_lengths.max()) + 1).unsqueeze(0) < xl.unsqueeze(1)
            return scored.float() * 0.5, xl

    for base, out in ((None, tmp_path / "e"), (2.0, tmp_path / "two")):
        ppl = P.write_perplexity(Stub(), data, ["u1", "u3", "u2"], out, 2, base, torch.device("cpu"))
        want = math.exp(0.5) if base is None else 2.0 ** (0.5 / math.log(2.0))
        assert abs(ppl - want) < 1e-6
        assert (out / "utt2ntokens").read_text() == "u1 4\nu3 1\nu2 2\n"
        lines = (out / "utt2ppl").read_text().splitlines()
        assert [l.split()[0] for l in lines] == ["u1", "u3", "u2"]
        assert all(abs(float(l.split()[1]) - want) < 1e-6 for l in lines)
        assert abs(float((out / "ppl").read_text()) - want) < 1e-6
    assert abs(P.perplexity(3.0, 4, 10.0) - 10.0 ** (0.75 / np.log(10.0))) < 1e-12


def defect_deltas():
    """{(model, defect): the largest change of a scored nll} over the GPU tests' models and sentences (bf16-rounded
    weights, as the device's fast mode holds them)."""
    out = {}
    for name, (V, heads, pos_enc, _) in K.MODELS.items():
        p = R.Params(K.build_model(name).state_dict(), heads, pos_enc is not None, round_to=torch.bfloat16)
        for defect in R.DEFECTS:
            if defect == "pe0" and pos_enc is None:
                continue
            worst = 0.0
            for Lp in K.WIDTHS:
                text, lens = K.make_text(Lp, V)
                worst = max(worst, float((R.nll(p, text, lens, defect=defect)[0] - R.nll(p, text, lens)[0]).abs().max()))
            out[(name, defect)] = worst
    return out


def test_defects_are_visible():
    """An off-by-one causal mask, a missing id-0 mask and pe[0] at every position each move some scored nll of every model
    they apply to by more than four times every nll bound of the GPU tests.  Measured (this test prints them):
    see profiles/lm_nll_first_run.txt."""
    deltas = defect_deltas()
    for k, v in sorted(deltas.items()):
        print(f"\ndefect {k[0]:5s} {k[1]:7s}: largest nll change {v:.3e}")
    low = min(deltas.values())
    bound = max(max(K.E_NLL.values()), max(K.E_HEAD.values()))
    print(f"\nsmallest {low:.3e}; largest nll bound {bound:.3e}")
    assert bound < low / 4
