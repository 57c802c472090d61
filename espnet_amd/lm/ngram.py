"""Back-off n-gram language model (ARPA) for the n-gram scorers (espnet_amd/nets/scorers/ngram.py).

The reference scores an n-gram through kenlm (espnet2/legacy/nets/scorers/ngram.py, `Ngrambase`); here the file is read by
the native ARPA reader (csrc/host_io.cpp `em_arpa_count` / `em_arpa_load`) into the sorted trie the device kernels walk
(include/espnet_amd.h `EmNgramModel`, csrc/ngram.hip):
  - order-1 entry i is word id i (the file's 1-gram order; `<unk>` appended with log10 p = -100 when the file has none, as
    kenlm does);
  - the entries of order k + 1 are sorted by (index of their k-word prefix in order k, word id), so the successors of an
    entry - the n-grams that extend it - are one contiguous range `next[k-1][e] .. next[k-1][e+1]`.
Scores stay log10, as in the file and as kenlm returns them.

Tokens map to words as the reference's `chardict` does: `<eos>` reads as `</s>`, every other token as itself, and a string
that is no unigram of the file scores as `<unk>` (ESPnet2's `<sos/eos>` normally does: a reference quirk kept as is).
"""
import ctypes as C
from pathlib import Path
from typing import List, Sequence

import numpy as np

from espnet_amd import lib as L

MAX_ORDER = L.EM_NGRAM_MAX_ORDER


class ArpaModel:
    """Host arrays of one ARPA file in the trie layout of EmNgramModel: `words` (word id -> string), per order k (index
    k-1) `wid`, `prob`, `bow` and, below the highest order, `next`."""

    def __init__(self, path, order: int, words: List[str], wid, prob, bow, nxt):
        self.path = str(path)
        self.order = order
        self.words = words
        self.index = {w: i for i, w in enumerate(words)}
        self.wid, self.prob, self.bow, self.next = wid, prob, bow, nxt
        self.unk = self.index["<unk>"]
        self.bos = self.index.get("<s>", -1)

    @property
    def counts(self) -> List[int]:
        return [len(a) for a in self.wid]

    def __repr__(self):
        return f"ArpaModel({self.path!r}, order={self.order}, counts={self.counts})"


def _unsupported(path: Path) -> NotImplementedError:
    head = path.read_bytes()[:8] if path.is_file() else b""
    if head.startswith(b"mmap lm "):
        return NotImplementedError(
            f"{path}: a kenlm binary LM; this reader takes the plain-text ARPA file (asr.sh keeps it beside the binary, "
            f"e.g. {path.with_suffix('.arpa')})")
    if head.startswith(b"\x1f\x8b"):
        return NotImplementedError(f"{path}: a gzipped ARPA file; decompress it first (gunzip)")
    return NotImplementedError(f"{path}: not a plain-text ARPA file, or an n-gram order above {MAX_ORDER} "
                               "(kenlm's default maximum)")


def load_arpa(path) -> ArpaModel:
    """Read a plain-text ARPA file (two native passes: count, then fill).  kenlm binary files, gzipped ARPA files and
    orders above 6 raise NotImplementedError; a malformed file raises ValueError."""
    path = Path(path)
    lib = L.load()
    bpath = str(path).encode()
    order = C.c_int32()
    counts = (C.c_int32 * MAX_ORDER)()
    vbytes = C.c_int64()
    rc = lib.em_arpa_count(bpath, C.byref(order), counts, C.byref(vbytes))
    if rc == L.EM_ERR_UNSUPPORTED:
        raise _unsupported(path)
    if rc == L.EM_ERR_IO:
        raise FileNotFoundError(f"{path}: cannot read the n-gram file")
    if rc != L.EM_OK:
        raise ValueError(f"{path}: malformed ARPA file (header or 1-grams)")
    N = order.value
    cnt = [counts[k] for k in range(N)]
    vocab = np.zeros(max(vbytes.value, 1), dtype=np.uint8)
    wid = [np.empty(c, dtype=np.int32) for c in cnt]
    prob = [np.empty(c, dtype=np.float32) for c in cnt]
    bow = [np.empty(c, dtype=np.float32) for c in cnt]
    nxt = [np.empty(c + 1, dtype=np.int32) for c in cnt[:-1]]

    def ptrs(arrs, n):
        out = (C.c_void_p * n)()
        for k, a in enumerate(arrs):
            out[k] = a.ctypes.data
        return out

    rc = lib.em_arpa_load(bpath, N, counts, vocab.ctypes.data, ptrs(wid, N), ptrs(prob, N), ptrs(bow, N),
                          ptrs(nxt, max(N - 1, 1)))
    if rc == L.EM_ERR_UNSUPPORTED:
        raise _unsupported(path)
    if rc != L.EM_OK:
        raise ValueError(f"{path}: malformed ARPA file (counts that do not match, an n-gram whose prefix or word is "
                         "missing, or an n-gram listed twice)")
    words = bytes(vocab[: vbytes.value]).decode("utf-8").split("\0")[:-1]
    assert len(words) == cnt[0]
    return ArpaModel(path, N, words, wid, prob, bow, nxt)


def chardict(token_list: Sequence[str]) -> List[str]:
    """The reference's token -> ARPA word strings (Ngrambase.__init__)."""
    return [t if t != "<eos>" else "</s>" for t in token_list]


def token_tables(model: ArpaModel, token_list: Sequence[str]):
    """(tok2word [V], word2tok [words], alias) int32: the word id of every token (<unk> for strings that are no unigram),
    the lowest token id of every word (-1: none), and the tokens that are not their word's lowest token."""
    V = len(token_list)
    tok2word = np.array([model.index.get(w, model.unk) for w in chardict(token_list)], dtype=np.int32).reshape(V)
    word2tok = np.full(len(model.words), -1, dtype=np.int32)
    alias = []
    for t, w in enumerate(tok2word.tolist()):
        if word2tok[w] < 0:
            word2tok[w] = t
        else:
            alias.append(t)
    return tok2word, word2tok, np.array(alias, dtype=np.int32)
