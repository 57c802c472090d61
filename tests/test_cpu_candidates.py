"""CandidateBatch (espnet_amd/nets/candidates.py): the flattening, checking, slicing and regrouping of the candidate
transcripts that Speech2Text.batch_nll / batch_transducer_nll / batch_rescore share.  Host data only."""
import numpy as np
import pytest
import torch

from espnet_amd.nets.candidates import CandidateBatch, is_one_transcript

FORBIDDEN = {0: "<blank>", 9: "<sos/eos>"}


def to_ids(t):
    """What Speech2Text._target_ids does without a tokenizer."""
    if isinstance(t, str):
        raise ValueError("a text transcript needs a tokenizer (token_type / bpemodel); pass token ids instead")
    return [int(v) for v in (t.tolist() if hasattr(t, "tolist") else t)]


def words(t):
    """A converter with a tokenizer: one id per letter."""
    return [ord(c) - ord("a") + 1 for c in t.split()] if isinstance(t, str) else to_ids(t)


def test_what_counts_as_one_transcript():
    assert is_one_transcript("a b") and is_one_transcript([1, 2]) and is_one_transcript([])
    assert is_one_transcript(torch.tensor([1, 2])) and is_one_transcript(np.array([3])) and is_one_transcript([np.int64(4)])
    assert not is_one_transcript([[1], [2]]) and not is_one_transcript(["a", "b"]) and not is_one_transcript([[]])


def test_single_transcripts_and_candidate_lists():
    cb = CandidateBatch([[1, 2], [[3], [4, 5, 6]], torch.tensor([7])], 3, to_ids, vocab_size=10, forbidden=FORBIDDEN)
    assert cb.ids == [[1, 2], [3], [4, 5, 6], [7]] and cb.ylens == [2, 1, 3, 1]
    assert cb.mem_of == [0, 1, 1, 2] and cb.counts == [1, 2, 1] and len(cb) == 4


def test_a_string_gives_what_its_ids_give():
    a, b = CandidateBatch(["a c", ["b", [4]]], 2, words), CandidateBatch([[1, 3], [[2], [4]]], 2, words)
    assert a.ids == b.ids == [[1, 3], [2], [4]] and a.mem_of == b.mem_of and a.counts == b.counts == [1, 2]


def test_an_empty_sequence_is_one_empty_transcript():
    cb = CandidateBatch([[], [[]], [[], [1]]], 3, to_ids)
    assert cb.ids == [[], [], [], [1]] and cb.counts == [1, 1, 2] and cb.mem_of == [0, 1, 2, 2]
    only = list(cb.slices(100))
    assert len(only) == 1 and tuple(only[0].ys.shape) == (4, 1) and only[0].ylens == [0, 0, 0, 1]
    # a slice of empty transcripts: one zero column where a scorer needs one, none where it keeps its own width
    assert tuple(next(cb.slices(3)).ys.shape) == (3, 1) and tuple(next(cb.slices(3, min_width=0)).ys.shape) == (3, 0)
    # no utterance, no candidate: no slice, nothing to regroup
    none = CandidateBatch([], 0, to_ids)
    assert len(none) == 0 and list(none.slices(2)) == [] and none.regroup([]) == []


def test_slices_inside_an_utterance_and_across_two():
    """Groups of 3 and 1 in slices of 2: the first boundary falls inside utterance 0's list, the second slice spans both."""
    cands, other = [[5, 9, 11, 3], [5, 9], []], [7, 7, 30, 12, 4, 21]
    cb = CandidateBatch([cands, other], 2, to_ids, vocab_size=100)
    s0, s1 = cb.slices(2)
    assert (s0.u0, s0.u1, s0.mem_of, s0.mem_rel, s0.ylens) == (0, 1, [0, 0], [0, 0], [4, 2])
    assert s0.ids == cands[:2] and s0.ys.dtype == torch.long and s0.ys.tolist() == [[5, 9, 11, 3], [5, 9, 0, 0]]
    assert (s1.u0, s1.u1, s1.mem_of, s1.mem_rel, s1.ylens) == (0, 2, [0, 1], [0, 1], [0, 6])
    assert s1.ids == [[], other] and s1.ys.tolist() == [[0] * 6, other]  # each slice at its own longest length
    # groups of 1 and 3: the second slice lies in utterance 1 alone, and names it relative to itself
    t0, t1 = CandidateBatch([other, cands], 2, to_ids).slices(2)
    assert (t0.u0, t0.u1, t0.mem_of, t0.mem_rel) == (0, 2, [0, 1], [0, 1]) and tuple(t0.ys.shape) == (2, 6)
    assert (t1.u0, t1.u1, t1.mem_of, t1.mem_rel) == (1, 2, [1, 1], [0, 0]) and tuple(t1.ys.shape) == (2, 2)
    assert [len(s.ids) for s in cb.slices(3)] == [3, 1] and [len(s.ids) for s in cb.slices(100)] == [4]


def test_regroup_inverts_the_flattening():
    texts = [[[1], [2, 3], []], [4, 5], [[6]], [[7], [8]]]
    cb = CandidateBatch(texts, 4, to_ids)
    assert cb.regroup(cb.ids) == [[[1], [2, 3], []], [[4, 5]], [[6]], [[7], [8]]]
    assert cb.regroup(list(range(len(cb)))) == [[0, 1, 2], [3], [4], [5, 6]]
    flat = [v for s in cb.slices(2) for v in s.ylens]
    assert cb.regroup(flat) == [[1, 2, 0], [2], [1], [1, 1]]


def test_every_refusal_with_its_message():
    with pytest.raises(ValueError, match="2 transcript entries for 1 utterances"):
        CandidateBatch([[1], [2]], 1, to_ids)
    with pytest.raises(ValueError, match=r"token id 0 \(<blank>\) cannot be aligned"):
        CandidateBatch([[[1], [1, 0]]], 1, to_ids, vocab_size=10, forbidden=FORBIDDEN)
    with pytest.raises(ValueError, match=r"token id 9 \(<sos/eos>\) cannot be aligned"):
        CandidateBatch([[1], [2, 9]], 2, to_ids, vocab_size=10, forbidden=FORBIDDEN)
    with pytest.raises(ValueError, match="tokenizer"):
        CandidateBatch(["a a"], 1, to_ids, vocab_size=10)
    with pytest.raises(ValueError, match=r"token ids must lie in \[0, 10\)"):
        CandidateBatch([[1, 10]], 1, to_ids, vocab_size=10)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        CandidateBatch([[[1], [-1]]], 1, to_ids, vocab_size=10)
    assert CandidateBatch([[1, 10]], 1, to_ids).ids == [[1, 10]]  # no vocabulary given: the scorer's own check decides


def test_speech2text_builds_it_before_anything_is_encoded():
    """The three batch_* calls check through it: an id beyond the vocabulary is refused on the host, by batch_nll too."""
    import types

    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.text.token_id_converter import TokenIDConverter

    def no_encode(*a, **k):
        raise AssertionError("encoded before the checks")

    s2t = Speech2Text.__new__(Speech2Text)
    s2t.asr_model = types.SimpleNamespace(blank_id=0, sos=3, eos=3, vocab_size=4, use_transducer_decoder=False,
                                          encode_device=no_encode)
    s2t.tokenizer, s2t.device = None, "cuda"
    s2t.converter = TokenIDConverter(token_list=["<blank>", "a", "<unk>", "<sos/eos>"])
    speech = torch.zeros(1, 1600)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        s2t.batch_nll(speech, [1600], [[1, 7]])
    with pytest.raises(ValueError, match="<sos/eos>"):
        s2t.batch_nll(speech, [1600], [[[1], [3]]])
    with pytest.raises(ValueError, match="transcript entries"):
        s2t.batch_nll(speech, [1600], [[1], [2]])
    assert s2t.batch_nll(torch.zeros(0, 1600), [], []) == []  # nothing to score: nothing is encoded
