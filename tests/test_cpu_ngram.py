"""The n-gram scorer's host side without a GPU: the native ARPA reader (csrc/host_io.cpp em_arpa_count / em_arpa_load) into
the sorted trie of EmNgramModel, the token -> word tables, and the restatement of the scoring contract the GPU tests hold
the kernels to (tests/ngram_ref.py) on hand-computed values."""
import time

import numpy as np
import pytest

from espnet_amd.lm.ngram import load_arpa, token_tables
from tests.ngram_ref import RefNgram, synthetic_arpa, write_arpa

F = np.float32

HAND = {
    1: [("-1.0", "<unk>", "0"), ("-99", "<s>", "-0.5"), ("-0.7", "</s>", None), ("-0.6", "a", "-0.3"),
        ("-0.8", "b", "-0.25"), ("-0.9", "c", None)],
    2: [("-0.4", "<s> b", "-0.1"), ("-0.3", "a b", "-0.2"), ("-0.2", "<s> a", "-0.15"), ("-0.5", "b c", None),
        ("-0.35", "a </s>", None)],
    3: [("-0.1", "<s> a b", None), ("-0.05", "a b c", None), ("-0.12", "<s> b c", None)],
}
TOKENS = ["<blank>", "<unk>", "a", "b", "c", "d", "<eos>", "<sos/eos>"]


@pytest.fixture
def hand(tmp_path):
    p = tmp_path / "hand.arpa"
    write_arpa(p, HAND)
    return p


def test_reader_matches_the_hand_written_trie(hand):
    m = load_arpa(hand)
    assert m.order == 3 and m.counts == [6, 5, 3]
    assert m.words == ["<unk>", "<s>", "</s>", "a", "b", "c"] and m.unk == 0 and m.bos == 1
    np.testing.assert_array_equal(m.wid[0], np.arange(6))
    np.testing.assert_array_equal(m.prob[0], F([-1.0, -99, -0.7, -0.6, -0.8, -0.9]))
    np.testing.assert_array_equal(m.bow[0], F([0, -0.5, 0, -0.3, -0.25, 0]))  # missing back-off columns read 0
    # order 2 sorted by (prefix, word): <s> a, <s> b | a </s>, a b | b c
    np.testing.assert_array_equal(m.wid[1], [3, 4, 2, 4, 5])
    np.testing.assert_array_equal(m.prob[1], F([-0.2, -0.4, -0.35, -0.3, -0.5]))
    np.testing.assert_array_equal(m.bow[1], F([-0.15, -0.1, 0, -0.2, 0]))
    np.testing.assert_array_equal(m.next[0], [0, 0, 2, 2, 4, 5, 5])  # successor ranges of the unigrams
    # order 3: (<s> a) b | (<s> b) c | (a b) c
    np.testing.assert_array_equal(m.wid[2], [4, 5, 5])
    np.testing.assert_array_equal(m.prob[2], F([-0.1, -0.12, -0.05]))
    np.testing.assert_array_equal(m.bow[2], F([0, 0, 0]))
    np.testing.assert_array_equal(m.next[1], [0, 1, 2, 2, 3, 3])
    assert len(m.next) == 2


def test_token_tables(hand):
    m = load_arpa(hand)
    t2w, w2t, alias = token_tables(m, TOKENS)
    # <blank>, d, <sos/eos> are no unigram -> <unk>; <eos> reads as </s>
    np.testing.assert_array_equal(t2w, [0, 0, 3, 4, 5, 0, 2, 0])
    np.testing.assert_array_equal(w2t, [0, -1, 6, 2, 3, 4])
    np.testing.assert_array_equal(alias, [1, 5, 7])


def test_restatement_hand_values(hand, tmp_path):
    r = RefNgram(hand, TOKENS)
    a, b, c, d, eos, sos = 2, 3, 4, 5, 6, 7
    h_sa = r.history([sos, a])
    assert h_sa == ["<s>", "a"]
    assert r.score(h_sa, b) == F(-0.1)  # the 3-gram <s> a b
    assert r.score(h_sa, eos) == F(F(-0.35) + F(-0.15))  # <eos> -> </s>: back-off to the bigram a </s>
    assert r.score(h_sa, c) == F(F(F(-0.9) + F(-0.3)) + F(-0.15))  # back-off to the unigram
    h_sd = r.history([sos, d])  # d -> <unk>: the context <s> <unk> is absent, <unk> has bow 0
    assert h_sd == ["<s>", "<unk>"]
    assert r.score(h_sd, a) == F(F(-0.6) + F(0.0))
    h_s = r.history([sos])  # first step: <s> alone
    assert r.score(h_s, a) == F(-0.2)
    assert r.score(h_s, c) == F(F(-0.9) + F(-0.5))
    assert r.score(h_s, sos) == F(F(-1.0) + F(-0.5))  # <sos/eos> scores as <unk> (the reference's quirk)
    assert r.score(h_s, 0) == r.score(h_s, sos)  # <blank> too
    # only the last N-1 = 2 words: <s> a b c -> context (b c)
    assert r.score(r.history([sos, a, b, c]), a) == F(F(-0.6) + F(0.0))
    # the -100 fallback of a file without <unk>
    no_unk = {k: [g for g in v if g[1] != "<unk>"] for k, v in HAND.items()}
    p2 = tmp_path / "nounk.arpa"
    write_arpa(p2, no_unk)
    r2 = RefNgram(p2, TOKENS)
    assert r2.score(r2.history([sos]), d) == F(F(-100.0) + F(-0.5))
    m2 = load_arpa(p2)
    assert m2.words[-1] == "<unk>" and m2.prob[0][-1] == F(-100.0) and m2.bow[0][-1] == 0 and m2.unk == 5
    # the vectorised row form agrees with the per-token form
    for y in ([sos], [sos, a], [sos, d], [sos, a, b, c], [sos, b, eos]):
        row = r.row(r.history(y))
        assert [row[t] for t in range(len(TOKENS))] == [r.score(r.history(y), t) for t in range(len(TOKENS))]


def test_binary_gzip_and_order_seven_raise(tmp_path):
    b = tmp_path / "lm.bin"
    b.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0" + bytes(64))
    with pytest.raises(NotImplementedError, match=r"lm\.bin.*lm\.arpa"):
        load_arpa(b)
    gz = tmp_path / "lm.arpa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00" + bytes(32))
    with pytest.raises(NotImplementedError, match="gzip"):
        load_arpa(gz)
    g7 = {k: [("-1.0", " ".join(["a"] * k), None)] for k in range(1, 8)}
    g7[1] = [("-1.0", "a", "-0.1")]
    p7 = tmp_path / "o7.arpa"
    write_arpa(p7, g7)
    with pytest.raises(NotImplementedError, match="order"):
        load_arpa(p7)
    with pytest.raises(FileNotFoundError):
        load_arpa(tmp_path / "missing.arpa")
    bad = tmp_path / "bad.arpa"
    write_arpa(bad, {1: HAND[1], 2: [("-0.3", "a zz", None)]})  # a word that is no unigram
    with pytest.raises(ValueError):
        load_arpa(bad)


def test_two_million_ngrams_load_in_seconds(tmp_path):
    p = tmp_path / "big.arpa"
    synthetic_arpa(p, 5000, 4, [600_000, 800_000, 600_000], seed=3)
    t0 = time.perf_counter()
    m = load_arpa(p)
    dt = time.perf_counter() - t0
    assert m.order == 4 and sum(m.counts) > 1_900_000, m.counts
    # the trie invariants: successor ranges cover each order exactly once, words ascend inside every range
    for k in range(3):
        nx = m.next[k]
        assert nx[0] == 0 and nx[-1] == m.counts[k + 1] and (np.diff(nx) >= 0).all()
        w = m.wid[k + 1].astype(np.int64)
        key = np.repeat(np.arange(m.counts[k]), np.diff(nx)) * 10_000_000 + w
        assert (np.diff(key) > 0).all()
    print(f"loaded {sum(m.counts)} n-grams in {dt:.2f} s")
    assert dt < 30.0
