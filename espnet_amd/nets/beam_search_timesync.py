"""Time-synchronous CTC prefix beam search (espnet/nets/beam_search_timesync.py: BeamSearchTimeSync, what the reference's
Speech2Text builds for `time_sync=True`) on the MI355X, for ctc_weight = 1.0: the scorers are CTC, an n-gram and the length
bonus.  Three enqueued steps and one D2H copy per batch, whatever the number of frames:

    CTC.log_softmax -> em_ctc_frame_topk (the K best tokens of every frame) -> em_ctc_tsync_search (one workgroup per
    utterance walks its frames; include/espnet_amd.h states the recursion, csrc/ctc_tsync.hip the data structures)

Differences from the reference class, both deliberate ("Time-synchronous CTC search"):
  * a frame has exactly K = min(int(pre_beam_ratio * beam_size), V) candidates, ties to the lower id (the reference admits
    every token tied with the K-th);
  * a prefix whose repeat or merged mass was written in a frame stays a member of that frame even when the blank is not
    among the candidates (the reference drops it);
and one extension: `scorers["ngram"]` (an NgramFullScorer / NgramPartScorer; the reference's class knows no n-gram).
Attention-decoder and neural-LM scoring inside this search are refused by name: they need decoder steps on prefixes of
different lengths in one batch, which the step kernels do not do."""
import ctypes as C
from typing import Any, Dict, List, Optional

import torch

from espnet_amd import lib as L
from espnet_amd.nets.beam_search import Hypothesis


def limits():
    """(W_max, K_max): the largest beam and per-frame candidate count one workgroup of the walk holds."""
    w, k = C.c_int32(0), C.c_int32(0)
    L.load().em_ctc_tsync_limits(C.byref(w), C.byref(k))
    return int(w.value), int(k.value)


class BeamSearchTimeSync:
    def __init__(self, sos: int, beam_size: int, scorers: Dict[str, Any], weights: Dict[str, float], token_list=None,
                 pre_beam_ratio: float = 1.5, blank: int = 0, force_lid: bool = False, temp: float = 1.0):
        if scorers.get("ctc") is None:
            raise ValueError("BeamSearchTimeSync needs scorers['ctc']")
        if scorers.get("decoder") is not None and float(weights.get("decoder", 0.0)) > 0.0:
            raise NotImplementedError("BeamSearchTimeSync: the scorer 'decoder' (attention decoder) is not scored "
                                      "time-synchronously on the MI355X path; use ctc_weight=1.0")
        if scorers.get("lm") is not None and float(weights.get("lm", 0.0)) > 0.0:
            raise NotImplementedError("BeamSearchTimeSync: the scorer 'lm' (neural LM) is not scored time-synchronously on "
                                      "the MI355X path; an n-gram (scorers['ngram']) is")
        if force_lid:
            raise NotImplementedError("BeamSearchTimeSync: force_lid is outside the MI355X hot path")
        if float(temp) != 1.0:
            raise NotImplementedError("BeamSearchTimeSync: temp != 1.0 (softmax temperature of the decoder) is outside the "
                                      "MI355X hot path")
        ctc = scorers["ctc"]
        self.ctc = getattr(ctc, "ctc", ctc)  # (a CTCPrefixScorer carries the CTC module, as in the reference)
        self.ngram = scorers.get("ngram")
        self.sos = self.eos = int(sos)
        self.blank = int(blank)
        self.beam_size = int(beam_size)
        self.pre_beam_ratio = float(pre_beam_ratio)
        self.token_list = token_list
        self.weights = dict(ctc=float(weights.get("ctc", 1.0)),
                            ngram=float(weights.get("ngram", 0.0)) if self.ngram is not None else 0.0,
                            length_bonus=float(weights.get("length_bonus", 0.0)))
        self.scorers = {k: v for k, v in (("ctc", ctc), ("ngram", self.ngram)) if v is not None}
        self.nbest = self.beam_size
        if self.beam_size < 1:
            raise ValueError("beam_size must be at least 1")

    def candidates_per_frame(self, V: int) -> int:
        return max(1, min(int(self.pre_beam_ratio * self.beam_size), int(V)))

    # ------------------------------------------------------------------ device part
    def _checked_k(self, V: int) -> int:
        W, K = self.beam_size, self.candidates_per_frame(V)
        W_max, K_max = limits()
        if W > W_max or K > K_max:
            raise NotImplementedError(f"BeamSearchTimeSync: beam_size {W} with {K} candidates per frame is above the limit of "
                                      f"the device walk (beam_size <= {W_max}, int(pre_beam_ratio * beam_size) <= {K_max})")
        return K

    def search_log_probs(self, lp: torch.Tensor, olens, nbest: Optional[int] = None):
        """The two launches on given log-probabilities lp (B, T, V) f32 on the device; olens: host ints or an int32 device
        tensor.  Returns the device outputs (tokens (B, nbest, T) i32, lens, count, score, score_ctc, score_ngram,
        score_len); only enqueues."""
        from espnet_amd.asr.ctc import CTC

        return self.search_candidates(*CTC.topk_log_probs(lp, self._checked_k(int(lp.shape[-1])), self.blank), olens, nbest)

    def search_candidates(self, cand_id, cand_lp, blank_lp, olens, nbest: Optional[int] = None, ws=None):
        """`em_ctc_tsync_search` on the per-frame candidate tables (B, T, K); `ws`: a caller's workspace (uint8, at least
        em_ctc_tsync_search_workspace_bytes) or None."""
        lib, dev = L.load(), cand_id.device
        B, T, K = (int(v) for v in cand_id.shape)
        W = self.beam_size
        nb = int(nbest or self.nbest)
        if torch.is_tensor(olens) and olens.is_cuda:
            xl = olens.to(torch.int32).contiguous()
        else:
            xl = torch.as_tensor([int(v) for v in olens], dtype=torch.int32).to(dev, non_blocking=True)
        need = int(lib.em_ctc_tsync_search_workspace_bytes(B, T, K, W))
        if ws is None:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        tokens = torch.empty(B, nb, T, dtype=torch.int32, device=dev)
        lens = torch.empty(B, nb, dtype=torch.int32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        sc = [torch.empty(B, nb, dtype=torch.float32, device=dev) for _ in range(4)]
        model = None
        if self.ngram is not None and self.weights["ngram"] != 0.0:
            model = C.byref(self.ngram.packed(dev).w)
        L.check(lib.em_ctc_tsync_search(L.ptr(cand_id), L.ptr(cand_lp), L.ptr(blank_lp), L.ptr(xl), B, T, K, W, nb, self.sos,
                                        self.blank, self.weights["ctc"], self.weights["ngram"], self.weights["length_bonus"],
                                        model, L.ptr(tokens), L.ptr(lens), L.ptr(count), L.ptr(sc[0]), L.ptr(sc[1]),
                                        L.ptr(sc[2]), L.ptr(sc[3]), L.ptr(ws), int(ws.numel()), L.current_stream_ptr()),
                "em_ctc_tsync_search")
        return (tokens, lens, count, *sc)

    # ------------------------------------------------------------------ host part
    def collect(self, outs) -> List[List[Hypothesis]]:
        """The one D2H copy and the n-best lists: per utterance Hypothesis(yseq = [sos] tokens [sos], score, scores)."""
        tokens, lens, count, score, s_ctc, s_ng, s_len = outs
        B, nb, T = tokens.shape
        # (one packed transfer: the int32 outputs and the f32 scores' bits side by side)
        flat = torch.cat([tokens.reshape(B, -1), lens, count.reshape(B, 1)] +
                         [s.view(torch.int32) for s in (score, s_ctc, s_ng, s_len)], dim=1).cpu()
        tok = flat[:, : nb * T].reshape(B, nb, T)
        o = nb * T
        ln, cnt = flat[:, o : o + nb], flat[:, o + nb]
        f = flat[:, o + nb + 1 :].contiguous().view(torch.float32).reshape(B, 4, nb)
        keys = ["ctc"] + (["ngram"] if self.ngram is not None else []) + ["length_bonus"]
        col = dict(ctc=1, ngram=2, length_bonus=3)
        res = []
        for b in range(B):
            hyps = []
            for r in range(int(cnt[b])):
                n = int(ln[b, r])
                y = torch.empty(n + 2, dtype=torch.int64)
                y[0] = y[n + 1] = self.sos
                y[1 : n + 1] = tok[b, r, :n]
                hyps.append(Hypothesis(yseq=y, score=float(f[b, 0, r]), scores={k: float(f[b, col[k], r]) for k in keys},
                                       states={}))
            res.append(hyps)
        return res

    @torch.no_grad()
    def search_batch(self, enc_act: torch.Tensor, olens, nbest: Optional[int] = None, **_ignored):
        """enc_act (B, T, d) encoder output on the device, olens the valid frames -> one n-best list per utterance, best
        first.  Enqueues `CTC.log_softmax`, the top-K launch and the walk, then makes one D2H copy."""
        L.require_gpu(enc_act, "enc_act")
        tabs = self.ctc.frame_topk_device(enc_act, self._checked_k(self.ctc.odim), self.blank)
        return self.collect(self.search_candidates(*tabs, olens, nbest))

    @torch.no_grad()
    def forward(self, x: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> List[Hypothesis]:
        """One utterance x (T, d); the length ratios are ignored, as in the reference."""
        return self.search_batch(x.unsqueeze(0), [int(x.shape[0])])[0]

    __call__ = forward
