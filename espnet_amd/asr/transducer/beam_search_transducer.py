"""BeamSearchTransducer: greedy and default beam search of a transducer model on the MI355X.

Mirrors espnet2/asr/transducer/beam_search_transducer.py (constructor keywords, `__call__(enc_out) -> [Hypothesis]` with
`yseq[0] == blank`).

  * beam_size <= 1 - greedy_search: at most one label per frame, so a ragged batch moves in lock-step and the whole walk
    is `em_transducer_greedy` (csrc/transducer.hip): a stream-ordered chain of launches per frame, nothing read back
    until it has ended.  `search_batch` is the batched entry, `__call__` the batch of one.
  * beam_size > 1, search_type="default" - `beam_device`: `em_transducer_beam_search` (csrc/transducer_beam.hip) walks a
    batch of up to 64 utterances in lock-step, one expansion per live utterance and step, the steps enqueued in chunks
    with one small status read-back per chunk.  `default_beam_search` - driven from the host over the two device
    primitives (`em_transducer_dec_step`, `em_transducer_joint_logp`), one launch pair and one read-back per expansion -
    is the route of an utterance the walk stopped on (a capacity of `beam_limits()`, MAX_EXPANSIONS_PER_FRAME) and of
    beams above the walk's limit; both routes see the same log-probability bits and sum scores in double, so they
    return the same lists.
  * `lm=` a SequentialRNNLM (lstm / gru), beam_size > 1: shallow fusion as the reference's `use_lm` - the popped
    hypothesis goes through the LM once (fed sos = vocab - 1, then its labels), `lm_weight * lm_logp[k]` is added to
    the beam_k label children, which are still chosen on the joint log-probabilities alone; the blank extension gets no
    LM term.  The walk is `em_transducer_beam_search_lm`, the host route calls `em_transducer_lm_step` one row at a
    time (the same kernels, so the same bits) and both add the term in double.  LM fusion exists at the beams the walk
    holds (`beam_limits()["beam"]`); other LMs raise NotImplementedError.
  * tsd / alsd / nsc / maes and multi-blank models raise NotImplementedError.
"""
import ctypes as C
import logging
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch

from espnet_amd import lib as L

logger = logging.getLogger(__name__)

MAX_WALK_ROWS = 64  # em_transducer_greedy: utterances per call
# default beam search: expansions of one frame before the search gives up.  The reference's loop has no cap: a model
# whose every context prefers some label to blank never leaves a frame.  Trained models leave one after a few
# expansions per beam entry; each expansion here is a pair of launches and a read-back, so the loop must end.
MAX_EXPANSIONS_PER_FRAME = 1000


def beam_limits():
    """`em_transducer_beam_limits`: the device walk's capacities per utterance - the largest beam, open entries, kept
    entries, expansions of one frame, labels of one hypothesis (the leading blank included)."""
    v = [C.c_int32(0) for _ in range(5)]
    L.load().em_transducer_beam_limits(*(C.byref(x) for x in v))
    return dict(zip(("beam", "open", "kept", "expansions", "labels"), (int(x.value) for x in v)))


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
            from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM

            if not isinstance(lm, SequentialRNNLM) or lm.rnn_type not in ("LSTM", "GRU"):
                kind = f"SequentialRNNLM(rnn_type={lm.rnn_type.lower()!r})" if isinstance(lm, SequentialRNNLM) \
                    else type(lm).__name__
                raise NotImplementedError(f"BeamSearchTransducer(lm=...): lm is a {kind}; the transducer search fuses a "
                                          "SequentialRNNLM with rnn_type lstm or gru")
            if lm.vocab_size != decoder.vocab_size:
                raise ValueError(f"BeamSearchTransducer(lm=...): the lm has {lm.vocab_size} tokens, the transducer "
                                 f"{decoder.vocab_size}")
            if beam_size > beam_limits()["beam"]:
                raise NotImplementedError(f"BeamSearchTransducer(lm=...): lm fusion with beam_size={beam_size}; it runs at "
                                          f"the beams the device walk holds, up to {beam_limits()['beam']}")
            if beam_size <= 1:
                logger.info("BeamSearchTransducer: beam_size <= 1 is the greedy search, which does not use the lm")
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
        self.lm, self.lm_weight = lm, float(lm_weight)
        self.sos = self.vocab_size - 1  # (the reference's: what the LM reads before the first label)
        self.search_type = search_type
        self.score_norm, self.nbest = score_norm, nbest
        self.token_list = token_list
        self.keep_trace = False  # tests: the greedy walk's per-frame trace in `last_trace`
        self.last_trace = None
        self.last_beam = None  # beam_device: status rows, steps enqueued / needed
        self.last_routes = None  # search_batch, beam_size > 1: "device" or "host" per utterance

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

    # ------------------------------------------------------------------ default beam search: the device walk
    @torch.no_grad()
    def beam_device(self, enc_act: torch.Tensor, olens, max_steps: Optional[int] = None, trace: bool = False):
        """`em_transducer_beam_search` (csrc/transducer_beam.hip) for enc_act (B, T, D) on the device, olens host ints,
        B <= 64 and beam_size <= the library's limit (NotImplementedError beyond).  The steps - one expansion per live
        utterance each - are enqueued in chunks, the first of max(olens) x beam (what a search needs at least); after a
        chunk the (B, 4) status array is read, until every utterance has ended or stopped, then the results in one
        gathered copy.  Returns a list over the utterances: the n-best hypotheses (`sort_nbest`; `dec_state` is None on
        this route: the states stay on the device), or None for an utterance the walk stopped on - a capacity of
        `beam_limits()` or MAX_EXPANSIONS_PER_FRAME - or that has no frame; `search_batch` decodes those with
        `default_beam_search`.  `last_beam` holds the status rows, the steps enqueued and the steps needed.
        Tests: `max_steps` ends the walk after that many steps; `trace` enqueues step by step and keeps each step's
        (log-prob rows (B, V), trace rows (B, 4 + Lmax)) - with an LM also its rows (B, V) - in `last_beam["steps"]`."""
        dec, jn = self.decoder, self.joint_network
        L.require_gpu(enc_act, "enc_act")
        B, T, _ = enc_act.shape
        olens = [min(int(v), int(T)) for v in olens]
        lim = beam_limits()
        beam = min(self.beam_size, self.vocab_size)
        if B > MAX_WALK_ROWS:
            raise NotImplementedError(f"beam_device: {B} utterances, one call walks at most {MAX_WALK_ROWS}")
        if self.beam_size > lim["beam"]:
            raise NotImplementedError(f"beam_device: beam_size={self.beam_size}, the device walk holds beams up to "
                                      f"{lim['beam']} ({lim['open']} open and {lim['kept']} kept entries, "
                                      f"{lim['expansions']} expansions of one frame, {lim['labels']} labels of a hypothesis)")
        dev = enc_act.device
        w, keep = dec.weights(dev)
        lw, lm_keep = self.lm.transducer_lm_weights(dev) if self.lm is not None else (None, None)
        lw_ref = C.byref(lw) if lw is not None else None
        # lin_enc per utterance, on exactly the rows default_beam_search hands it: the same GEMM call, so the same bits
        enc_proj = torch.zeros(B, T, w.jp, dtype=torch.float32, device=dev)
        for b in range(B):
            if olens[b] > 0:
                enc_proj[b, : olens[b]] = jn.enc_proj_device(enc_act[b, : olens[b]])
        lib = L.load()
        need = int(lib.em_transducer_beam_workspace_bytes_lm(dec.em_dtype, C.byref(w), lw_ref, B, T, self.beam_size))
        if need == 0:
            raise NotImplementedError(f"em_transducer_beam_search: B={B}, T={T}, beam={self.beam_size} are outside one call")
        Tmax = max(olens + [1])
        Lmax = min(lim["labels"], 2 * Tmax + 16)
        ncap = lim["kept"]
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ol = torch.tensor(olens, dtype=torch.int32).to(dev)
        status = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        out_tok = torch.empty(B, ncap, Lmax, dtype=torch.int32, device=dev)
        out_len = torch.zeros(B, ncap, dtype=torch.int32, device=dev)
        out_score = torch.zeros(B, ncap, dtype=torch.float64, device=dev)
        out_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        step_logp = torch.zeros(B, self.vocab_size, dtype=torch.float32, device=dev) if trace else None
        step_tr = torch.zeros(B, 4 + Lmax, dtype=torch.int32, device=dev) if trace else None
        step_lm = torch.zeros(B, self.vocab_size, dtype=torch.float32, device=dev) if trace and lw is not None else None
        max_exp = int(MAX_EXPANSIONS_PER_FRAME)  # (read at call time: a test lowers it)

        def enqueue(first, steps):
            L.check(lib.em_transducer_beam_search_lm(dec.em_dtype, C.byref(w), lw_ref, self.lm_weight, L.ptr(enc_proj),
                                                     L.ptr(ol), B, T, self.beam_size, max_exp, Lmax, ncap, int(first),
                                                     int(steps), L.ptr(status), L.ptr(out_tok), L.ptr(out_len),
                                                     L.ptr(out_score), L.ptr(out_cnt), L.ptr(step_logp), L.ptr(step_tr),
                                                     L.ptr(step_lm), L.ptr(ws), need, L.current_stream_ptr()),
                    "em_transducer_beam_search_lm")

        enqueued, first, steps_kept = 0, True, []
        chunk = Tmax * beam
        while True:
            if max_steps is not None:
                chunk = min(chunk, max_steps - enqueued)
            if trace:
                for _ in range(chunk):
                    step_tr.zero_()
                    enqueue(first, 1)
                    first = False
                    steps_kept.append((step_logp.clone(), step_tr.clone()) + ((step_lm.clone(),) if lw is not None else ()))
            else:
                enqueue(first, chunk)
                first = False
            enqueued += chunk
            st = status.cpu()  # the read-back of this chunk
            if int((st[:, 0] == 0).sum()) == 0 or (max_steps is not None and enqueued >= max_steps):
                break
            chunk = max(Tmax * beam // 4, beam)
        cnt = out_cnt.cpu()
        done = [b for b in range(B) if int(st[b, 0]) == 1 and int(cnt[b]) > 0]
        out: List[Optional[List[Hypothesis]]] = [None] * B
        if done:
            rows = torch.tensor([b * ncap + i for b in done for i in range(int(cnt[b]))], dtype=torch.int64).to(dev)
            scores = out_score.view(-1)[rows].cpu().tolist()
            lens = out_len.view(-1)[rows].cpu().tolist()
            toks = out_tok.view(B * ncap, Lmax)[rows].cpu()
            k = 0
            for b in done:
                hyps = []
                for _ in range(int(cnt[b])):
                    hyps.append(Hypothesis(score=float(scores[k]), yseq=toks[k, : lens[k]].tolist()))
                    k += 1
                # the reference's final list: the qualifying kept entries by ascending score (a stable sort)
                out[b] = self.sort_nbest(sorted(hyps, key=lambda x: x.score))
        self.last_beam = dict(status=st, enqueued=enqueued, needed=int(st[:, 2].max()) if B else 0,
                              steps=[tuple(x.cpu() for x in st_) for st_ in steps_kept] if trace else None)
        return out

    @torch.no_grad()
    def search_batch(self, enc_act: torch.Tensor, olens, **unused) -> List[List[Hypothesis]]:
        """The n-best list of every utterance of a batch: enc_act (B, T, D) on the device, olens host ints.  With
        beam_size > 1 the batch goes through `beam_device` in slices of up to 64 utterances; an utterance the device
        walk stopped on is decoded by `default_beam_search` (`last_routes`: "device" or "host" per utterance)."""
        B = int(enc_act.shape[0])
        olens = [int(v) for v in olens]
        if self.beam_size > 1:
            if self.beam_size > beam_limits()["beam"]:
                self.last_routes = ["host"] * B
                return [self.default_beam_search(enc_act[b, : olens[b]], utt=b) for b in range(B)]
            out, routes = [], []
            for b0 in range(0, B, MAX_WALK_ROWS):
                b1 = min(B, b0 + MAX_WALK_ROWS)
                res = self.beam_device(enc_act[b0:b1], olens[b0:b1])
                for b, r in enumerate(res, b0):
                    routes.append("host" if r is None else "device")
                    out.append(self.default_beam_search(enc_act[b, : olens[b]], utt=b) if r is None else r)
            self.last_routes = routes
            return out
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
        lm = self.lm
        kept = [Hypothesis(score=0.0, yseq=[self.blank_id], dec_state=dec.select_state(dec.init_state(1, dev), 0),
                           lm_state=lm.init_rows_state(1, dev) if lm is not None else None)]
        cache, cache_lm = {}, {}
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
                kept.append(Hypothesis(score=h.score + float(logp[0]), yseq=h.yseq[:], dec_state=h.dec_state,
                                       lm_state=h.lm_state))
                order = np.argsort(-logp[1:], kind="stable")[:beam_k]  # (ties: the lowest id first, like topk)
                lm_logp = lm_state = None
                if lm is not None:  # one row per call: the bits the walk's row of this utterance carries
                    key = "_".join(map(str, h.yseq))
                    if key not in cache_lm:
                        tok = torch.full((1,), self.sos if len(h.yseq) == 1 else h.yseq[-1], dtype=torch.int32, device=dev)
                        row, st = lm.step_rows(tok, h.lm_state)
                        cache_lm[key] = (row[0].cpu().numpy(), st)
                    lm_logp, lm_state = cache_lm[key]
                for k in order:
                    score = h.score + float(logp[1 + k])
                    if lm is not None:  # (Python floats: the product and the sum are rounded one after the other)
                        score = score + self.lm_weight * float(lm_logp[1 + k])
                    hyps.append(Hypothesis(score=score, yseq=h.yseq + [int(k) + 1], dec_state=state, lm_state=lm_state))
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
        return self.search_batch(act.unsqueeze(0), [int(enc_out.shape[0])])[0]
