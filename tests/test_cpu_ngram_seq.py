"""Host logic of whole-sentence n-gram scoring that needs no device: the checks `sequence_logp` and `NgramLM.nll` make before
anything is launched, and the perplexity tool's choice between its two LM sources."""
import pytest
import torch

from tests.ngram_ref import synthetic_arpa


@pytest.mark.parametrize("ys, ylens", [([[2, 5, 3]], [3]), ([[2, -1, 3]], [3]), ([[2, 3, 3]], [4]), ([[2, 3, 3]], [-1]),
                                       ([2, 3], [2]), ([[2.0, 3.0]], [2])])
def test_bad_sentences_are_refused_on_the_host(tmp_path, ys, ylens):
    from espnet_amd.lm.ngram import NgramLM

    synthetic_arpa(tmp_path / "lm.arpa", 3, 2, [6], seed=1)
    lm = NgramLM(str(tmp_path / "lm.arpa"), ["<blank>", "<unk>", "w0", "w1", "<eos>"])  # V = 5
    with pytest.raises(ValueError):  # (a machine without a device gets this far and no further)
        lm.scorer.sequence_logp(torch.tensor(ys), torch.tensor(ylens))
    with pytest.raises(ValueError):
        lm.nll(torch.tensor(ys), torch.tensor(ylens))


def test_the_two_lm_sources_exclude_each_other():
    from espnet_amd.bin import lm_calc_perplexity as P

    base = ["--output_dir", "o", "--data_path_and_name_and_type", "d/text,text,text_int"]
    a = vars(P.get_parser().parse_args(base + ["--ngram_file", "lm.arpa", "--token_list", "tokens.txt", "--log_base", "10"]))
    assert a["ngram_file"] == "lm.arpa" and a["token_list"] == "tokens.txt" and a["log_base"] == 10.0 and a["token_type"] is None
    assert P.lm_source(a) == "ngram"
    assert P.lm_source(vars(P.get_parser().parse_args(base + ["--train_config", "c.yaml", "--model_file", "m.pth"]))) == "model"
    for extra in (["--ngram_file", "lm.arpa", "--token_list", "t", "--model_file", "m.pth"],
                  ["--ngram_file", "lm.arpa", "--token_list", "t", "--train_config", "c.yaml"],
                  ["--ngram_file", "lm.arpa"], ["--token_list", "t"]):
        with pytest.raises(ValueError):
            P.main(base + extra)  # refused before any file is opened
