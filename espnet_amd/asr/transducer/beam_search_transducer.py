"""BeamSearchTransducer: greedy and default beam search of a transducer model on the MI355X.

Mirrors espnet2/asr/transducer/beam_search_transducer.py (constructor keywords, `__call__(enc_out) -> [Hypothesis]` with
`yseq[0] == blank`).

  * beam_size <= 1 - greedy_search: at most one label per frame, so a ragged batch moves in lock-step and the whole walk
    is `em_transducer_greedy` (csrc/transducer.hip): a stream-ordered chain of launches per frame, nothing read back
    until it has ended.  `search_batch` is the batched entry, `__call__` the batch of one.
  * beam_size > 1, search_type="default" - default_beam_search, driven from the host over the two device primitives
    (`em_transducer_dec_step`, `em_transducer_joint_logp`), one launch pair and one read-back per expansion.
  * tsd / alsd / nsc / maes, a language model and multi-blank models raise NotImplementedError.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch

from espnet_amd import lib as L

MAX_WALK_ROWS = 64  # em_transducer_greedy: utterances per call
# default beam search: expansions of one frame before the search gives up.  The reference's loop has no cap: a model
# whose every context prefers some label to blank never leaves a frame.  Trained models leave one after a few
# expansions per beam entry; each expansion here is a pair of launches and a read-back, so the loop must end.
MAX_EXPANSIONS_PER_FRAME = 1000


@dataclass
class Hypothesis:
    """espnet2/asr/transducer/beam_search_transducer.py Hypothesis."""
    score: float
    yseq: List[int]
    dec_state: Any = None
    lm_state: Any = None


class BeamSearchTransducer:
    def __init__(self, decoder, joint_network, beam_size: int, lm=None, lm_weight: float = 0.1,
                 search_type: str = "default", max_sym_exp: int = 2, u_max: int = 50, nstep: int = 1,
                 prefix_alpha: int = 1, expansion_gamma: float = 2.3, expansion_beta: int = 2, score_norm: bool = True,
                 nbest: int = 1, token_list: Optional[List[str]] = None, multi_blank_durations: Sequence[int] = (),
                 **other):
        if lm is not None:
            raise NotImplementedError("BeamSearchTransducer(lm=...): language-model fusion is not on the device path")
        if multi_blank_durations:
            raise NotImplementedError("BeamSearchTransducer(multi_blank_durations=...): multi-blank transducers are not on "
                                      "the device path")
        for k, v in other.items():
            if v not in (None, False, [], (), {}):
                raise NotImplementedError(f"BeamSearchTransducer({k}={v!r}) is not on the device path")
        if beam_size > 1 and search_type != "default":
            raise NotImplementedError(f"search_type={search_type!r}: only the default beam search (and greedy, beam_size "
                                      "<= 1) is on the device path")
        self.decoder, self.joint_network = decoder, joint_network
        decoder.set_joint_network(joint_network)
        self.vocab_size = decoder.vocab_size
        self.blank_id = decoder.blank_id
        self.beam_size = int(beam_size)
        self.search_type = search_type
        self.score_norm, self.nbest = score_norm, nbest
        self.token_list = token_list
        self.keep_trace = False  # tests: the greedy walk's per-frame trace in `last_trace`
        self.last_trace = None

    # ------------------------------------------------------------------ greedy: the fused walk
    @torch.no_grad()
    def greedy_device(self, enc_act: torch.Tensor, olens_dev: torch.Tensor, trace: bool = False):
        """`em_transducer_greedy` for enc_act (B, T, D), olens_dev (B,) int32 on the device, B <= 64.  Returns device
        tensors (tokens (B, T) i32, ylens (B,) i32, score (B,) f32) and, with `trace`, (frame_tok, frame_top,
        frame_margin) (B, T) - entries the walk does not write read -1 / 0 / 0.  Enqueues only."""
        dec, jn = self.decoder, self.joint_network
        B, T, _ = enc_act.shape
        dev = enc_act.device
        w, keep = dec.weights(dev)
        enc_proj = jn.enc_proj_device(enc_act)
        lib = L.load()
        need = lib.em_transducer_greedy_workspace_bytes(dec.em_dtype, C.byref(w), B, T)
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
        tokens = torch.full((B, T), -1, dtype=torch.int32, device=dev)
        ylens = torch.zeros(B, dtype=torch.int32, device=dev)
        score = torch.zeros(B, dtype=torch.float32, device=dev)
        tr = None
        if trace:
            tr = (torch.full((B, T), -1, dtype=torch.int32, device=dev), torch.zeros(B, T, dtype=torch.float32, device=dev),
                  torch.zeros(B, T, dtype=torch.float32, device=dev))
        L.check(lib.em_transducer_greedy(dec.em_dtype, C.byref(w), L.ptr(enc_proj), L.ptr(olens_dev), B, T, L.ptr(tokens),
                                         L.ptr(ylens), L.ptr(score), L.ptr(tr[0]) if tr else None,
                                         L.ptr(tr[1]) if tr else None, L.ptr(tr[2]) if tr else None, L.ptr(ws), int(need),
                                         L.current_stream_ptr()), "em_transducer_greedy")
        return (tokens, ylens, score) + ((tr,) if trace else ())

    @torch.no_grad()
    def search_batch(self, enc_act: torch.Tensor, olens, **unused) -> List[List[Hypothesis]]:
        """The n-best list of every utterance of a batch: enc_act (B, T, D) on the device, olens host ints."""
        B = int(enc_act.shape[0])
        olens = [int(v) for v in olens]
        if self.beam_size > 1:
            return [self.default_beam_search(enc_act[b, : olens[b]], utt=b) for b in range(B)]
        out, traces = [], []
        for b0 in range(0, B, MAX_WALK_ROWS):
            b1 = min(B, b0 + MAX_WALK_ROWS)
            ol = torch.tensor(olens[b0:b1], dtype=torch.int32).to(enc_act.device)
            res = self.greedy_device(enc_act[b0:b1].contiguous(), ol, trace=self.keep_trace)
            tokens, ylens, score = (t.cpu() for t in res[:3])  # the read-back of the walk
            if self.keep_trace:
                traces.append(tuple(t.cpu() for t in res[3]))
            for b in range(b1 - b0):
                n = int(ylens[b])
                out.append([Hypothesis(score=float(score[b]), yseq=[self.blank_id] + tokens[b, :n].tolist())])
        self.last_trace = traces if self.keep_trace else None
        return out

    # ------------------------------------------------------------------ default beam search: host-driven
    @torch.no_grad()
    def default_beam_search(self, enc_out: torch.Tensor, utt: int = 0) -> List[Hypothesis]:
        """default_beam_search of the reference for one utterance, enc_out (T, D) on the device (`utt`: its index in the
        batch, for the error message).  A frame that is not left after MAX_EXPANSIONS_PER_FRAME expansions raises."""
        dec, jn = self.decoder, self.joint_network
        V = self.vocab_size
        beam = min(self.beam_size, V)
        beam_k = min(beam, V - 1)
        dev = enc_out.device
        enc_proj = jn.enc_proj_device(enc_out)  # (T, jpad): every frame at once
        kept = [Hypothesis(score=0.0, yseq=[self.blank_id], dec_state=dec.select_state(dec.init_state(1, dev), 0))]
        cache = {}
        for t in range(int(enc_out.shape[0])):
            hyps, kept = kept, []
            for expansion in range(MAX_EXPANSIONS_PER_FRAME + 1):
                if expansion == MAX_EXPANSIONS_PER_FRAME:
                    raise RuntimeError(f"default beam search: utterance {utt}, frame {t} not left after "
                                       f"{MAX_EXPANSIONS_PER_FRAME} expansions (labels beat blank in every context)")
                i_max = max(range(len(hyps)), key=lambda i: hyps[i].score)  # (first of equal scores, like max())
                h = hyps.pop(i_max)
                _, state, _ = dec.score(h, cache)
                dec_proj = cache["_".join(map(str, h.yseq))][2]
                logp = jn.logp_device(dec, enc_proj[t : t + 1], dec_proj.unsqueeze(0))[0].cpu().numpy()
                kept.append(Hypothesis(score=h.score + float(logp[0]), yseq=h.yseq[:], dec_state=h.dec_state))
                order = np.argsort(-logp[1:], kind="stable")[:beam_k]  # (ties: the lowest id first, like topk)
                for k in order:
                    hyps.append(Hypothesis(score=h.score + float(logp[1 + k]), yseq=h.yseq + [int(k) + 1], dec_state=state))
                best_left = max(x.score for x in hyps)
                most_prob = sorted([x for x in kept if x.score > best_left], key=lambda x: x.score)
                if len(most_prob) >= beam:
                    kept = most_prob
                    break
        return self.sort_nbest(kept)

    def sort_nbest(self, hyps: List[Hypothesis]) -> List[Hypothesis]:
        key = (lambda x: x.score / len(x.yseq)) if self.score_norm else (lambda x: x.score)
        return sorted(hyps, key=key, reverse=True)[: self.nbest]

    @torch.no_grad()
    def __call__(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, D) on the device -> the n-best hypotheses."""
        L.require_gpu(enc_out, "enc_out")
        act = enc_out.to(self.joint_network.act_dtype)
        if self.beam_size > 1:
            return self.default_beam_search(act)
        return self.search_batch(act.unsqueeze(0), [int(enc_out.shape[0])])[0]
