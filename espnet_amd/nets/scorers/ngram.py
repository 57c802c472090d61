"""N-gram LM scorers (espnet2/legacy/nets/scorers/ngram.py: Ngrambase, NgramFullScorer, NgramPartScorer) on the MI355X.

`ngram_model` is the path of a plain-text ARPA file (or an `espnet_amd.lm.ngram.ArpaModel` already read); `token_list` the
ASR model's tokens.  Scores are kenlm's: raw log10 with back-off, not renormalised over the token vocabulary, weighted by
`ngram_weight` in the search.

Inside the fused device search (espnet_amd/nets/batch_beam_search.py, csrc/search.hip + csrc/ngram.hip) every hypothesis
row carries the trie node of each context length and the scorer runs on the device with the other scorers: the full
scorer scores all V tokens before the pre-beam, the part scorer only the pre-beam candidates after it.  `score` /
`batch_score` / `score_partial` / `select_state` are the reference's per-step scorer interface on the same kernels
(`em_ngram_score`); a state is the hypothesis' context nodes, an int32 device tensor, None before the first step.
"""
import ctypes as C
from typing import Any, List

import numpy as np
import torch

from espnet_amd import lib as L
from espnet_amd.lm.ngram import ArpaModel, load_arpa, token_tables
from espnet_amd.nets.scorer_interface import BatchScorerInterface, PartialScorerInterface
from espnet_amd.packing import PackedModule


class Ngrambase(PackedModule):
    """The model, the token -> word tables and their device pack (built once per device through espnet_amd/packing.py)."""

    part = False

    def __init__(self, ngram_model, token_list):
        super().__init__()
        self.model = ngram_model if isinstance(ngram_model, ArpaModel) else load_arpa(ngram_model)
        self.token_list = list(token_list)
        self.charlen = len(self.token_list)
        self.tok2word, self.word2tok, self.alias = token_tables(self.model, self.token_list)
        self.order = self.model.order
        self.state_len = max(self.order - 1, 1)

    def search_key(self):
        return ("ngram", self.order, self.part)

    def _build_pack(self, pk):
        m = L.EmNgramModel()
        md = self.model
        m.order, m.vocab, m.unk, m.bos = md.order, self.charlen, md.unk, md.bos
        m.n_alias = len(self.alias)

        def dev(a):  # (an empty order still gets a valid address)
            return pk.hold(torch.from_numpy(a if len(a) else np.zeros(1, dtype=a.dtype))).data_ptr()

        for k in range(md.order):
            m.count[k] = len(md.wid[k])
            m.wid[k], m.prob[k], m.bow[k] = dev(md.wid[k]), dev(md.prob[k]), dev(md.bow[k])
            if k < md.order - 1:
                m.next[k] = dev(md.next[k])
        m.tok2word, m.word2tok = dev(self.tok2word), dev(self.word2tok)
        m.alias = dev(self.alias)
        pk.w = m

    # ------------------------------------------------------------------ scorer interface (one call per step)
    def init_state(self, x: torch.Tensor) -> Any:
        return None

    def select_state(self, state: Any, i: int, new_id: int = None) -> Any:
        return state  # (the context of a hypothesis does not depend on the token scored after it)

    @torch.no_grad()
    def _score(self, ys: torch.Tensor, states: List[Any], dev, cand=None):
        """(scores (n, V) or (n, n_cand) f32 log10, new states list[n]) for prefixes ys (n, L)."""
        n, Lc = ys.shape
        pk = self.packed(dev)
        prev = torch.full((n, self.state_len), -1, dtype=torch.int32, device=dev)
        if Lc > 1:
            for r, s in enumerate(states if states is not None else [None] * n):
                if s is not None:
                    prev[r] = s
            last = ys[:, -1].to(device=dev, dtype=torch.int32)
        else:  # the first step: context <s> alone (BeginSentenceWrite)
            last = torch.full((n,), -1, dtype=torch.int32, device=dev)
        out_state = torch.empty(n, self.state_len, dtype=torch.int32, device=dev)
        if cand is None:
            out = torch.empty(n, self.charlen, dtype=torch.float32, device=dev)
            c_ptr, n_cand = None, 0
        else:
            cand = cand.to(device=dev, dtype=torch.int32).reshape(n, -1).contiguous()
            out = torch.empty(cand.shape, dtype=torch.float32, device=dev)
            c_ptr, n_cand = L.ptr(cand), cand.shape[1]
        L.check(L.load().em_ngram_score(C.byref(pk.w), n, L.ptr(prev), L.ptr(last), L.ptr(out_state), c_ptr, n_cand,
                                        L.ptr(out), L.current_stream_ptr()), "em_ngram_score")
        return out, [out_state[r] for r in range(n)]

    def _device(self, x):
        L.require_gpu(x, "x")
        return x.device


class NgramFullScorer(Ngrambase, BatchScorerInterface):
    """ngram.py NgramFullScorer: every token of the vocabulary (a full scorer: it takes part in the pre-beam)."""

    def score(self, y: torch.Tensor, state: Any, x: torch.Tensor):
        s, st = self._score(y.unsqueeze(0), [state], self._device(x))
        return s[0], st[0]

    def batch_score(self, ys: torch.Tensor, states: List[Any], xs: torch.Tensor):
        return self._score(ys, states, self._device(xs))


class NgramPartScorer(Ngrambase, PartialScorerInterface):
    """ngram.py NgramPartScorer: only the pre-beam candidates (added after the pre-beam, like the CTC prefix score)."""

    part = True

    def score_partial(self, y: torch.Tensor, next_tokens: torch.Tensor, state: Any, x: torch.Tensor):
        s, st = self._score(y.unsqueeze(0), [state], self._device(x), cand=next_tokens.reshape(1, -1))
        return s[0], st[0]
