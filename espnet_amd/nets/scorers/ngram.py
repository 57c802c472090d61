"""N-gram LM scorers (espnet2/legacy/nets/scorers/ngram.py: Ngrambase, NgramFullScorer, NgramPartScorer) on the MI355X.

`ngram_model` is the path of a plain-text ARPA file (or an `espnet_amd.lm.ngram.ArpaModel` already read); `token_list` the
ASR model's tokens.  Scores are kenlm's: raw log10 with back-off, not renormalised over the token vocabulary, weighted by
`ngram_weight` in the search.

Inside the fused device search (espnet_amd/nets/batch_beam_search.py, csrc/search.hip + csrc/ngram.hip) every hypothesis
row carries the trie node of each context length and the scorer runs on the device with the other scorers: the full
scorer scores all V tokens before the pre-beam, the part scorer only the pre-beam candidates after it.  `score` /
`batch_score` / `score_partial` / `select_state` are the reference's per-step scorer interface on the same kernels
(`em_ngram_score`); a state is the hypothesis' context nodes, an int32 device tensor, None before the first step.
`sequence_logp` scores GIVEN sentences, every position at once (`em_ngram_seq_logp`, csrc/ngram_seq.hip), with the same bits.
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

    # ------------------------------------------------------------------ whole sentences (one enqueue)
    @torch.no_grad()
    def sequence_logp(self, ys, ylens, eos: bool = True, device=None):
        """Every token of given sentences scored in one enqueue (`em_ngram_seq_logp`, csrc/ngram_seq.hip): ys (N, Lp)
        HOST token ids (the padding may hold anything), ylens (N,) host lengths; eos: `<eos>` (the last token of the list,
        as the search scores it) is scored behind each sentence.  Returns device tensors
          logp (N,) f64                the sum of the row's scored positions, in position order;
          logp_tok (N, Lp + 1) f32     log10 per position, bit for bit what `batch_score` returns step by step;
          order_tok (N, Lp + 1) i32    the n-gram order that matched after back-off;
        the two per-position tensors hold 0 where nothing is scored.  Ids and lengths are checked here, on the host
        (ValueError), before anything is launched; nothing is read back."""
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.EspnetAmdError(f"sequence_logp on {dev}: espnet_amd runs only on an MI355X (HIP) device")
        ids_h = torch.as_tensor(ys).cpu()
        len_h = torch.as_tensor(ylens).cpu()
        if ids_h.dim() != 2 or len_h.dim() != 1 or len_h.numel() != ids_h.size(0) or ids_h.is_floating_point() or \
                len_h.is_floating_point():
            raise ValueError(f"sequence_logp: integer ys (N, Lp) and ylens (N,) expected, got {tuple(ids_h.shape)} and "
                             f"{tuple(len_h.shape)}")
        n, Lp = ids_h.shape
        if n and (int(len_h.min()) < 0 or int(len_h.max()) > Lp):
            raise ValueError(f"sequence_logp: ylens must lie in [0, {Lp}]")
        scored = torch.arange(Lp).unsqueeze(0) < len_h.unsqueeze(1)
        if bool((scored & ((ids_h < 0) | (ids_h >= self.charlen))).any()):
            raise ValueError(f"sequence_logp: token ids must lie in [0, {self.charlen})")
        ids_h = ids_h.to(torch.int32).contiguous()
        len_h = len_h.to(torch.int32).contiguous()
        pk = self.packed(dev)
        ids_d, len_d = ids_h.to(dev, non_blocking=True), len_h.to(dev, non_blocking=True)
        logp = torch.empty(n, dtype=torch.float64, device=dev)
        logp_tok = torch.zeros(n, Lp + 1, dtype=torch.float32, device=dev)
        order_tok = torch.zeros(n, Lp + 1, dtype=torch.int32, device=dev)
        L.check(L.load().em_ngram_seq_logp(C.byref(pk.w), L.ptr(ids_d), L.ptr(len_d), L.ptr(ids_h), L.ptr(len_h), n, Lp,
                                           self.charlen - 1 if eos else -1, L.ptr(logp_tok), L.ptr(order_tok), L.ptr(logp),
                                           L.current_stream_ptr()), "em_ngram_seq_logp")
        return logp, logp_tok, order_tok

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
