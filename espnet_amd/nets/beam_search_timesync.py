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
different lengths in one batch, which the step kernels do not do.

The streaming form (`stream_state`, `extend_candidates`, `extend`; `em_ctc_tsync_extend`): the same walk, RESUMABLE.  A
stream owns a slot of a persistent state slab (`TsyncStreamState`); a call feeds each row the next frames of its utterance
and returns the n-best list so far - bit for bit what the one-shot search returns for the frames fed so far, however they
were split into calls ("The time-synchronous search, resumable")."""
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


class TsyncStreamState:
    """The PERSISTENT memory of the resumable walk (`em_ctc_tsync_extend`): a slab of `n_slots` slots of `slot_bytes` each,
    one slot per live utterance, and the slots' allocator.  A slot holds no address and no slot index, so `grow()` copies
    the old slab into a larger one and every live stream keeps its slot number.  Plain Python over one uint8 tensor (which
    may live on the CPU: the allocator is tested there).  `frames[slot]`: the frames the host fed a live slot so far, counted
    when a call is enqueued (`collect` takes back what a refused row did not consume); `shape`: the (K, W, max_frames) the
    slot sizes were made for."""

    def __init__(self, n_slots: int, max_frames: int, slot_bytes: int, device, K: int, W: int):
        if n_slots < 1 or max_frames < 1 or slot_bytes < 1:
            raise ValueError("n_slots, max_frames and slot_bytes must be positive")
        self.n_slots, self.max_frames, self.slot_bytes = int(n_slots), int(max_frames), int(slot_bytes)
        self.shape = dict(K=int(K), W=int(W), max_frames=int(max_frames))
        self.slab = torch.empty(self.n_slots, self.slot_bytes, dtype=torch.uint8, device=device)
        self._free = list(range(self.n_slots))  # ascending: the lowest free slot goes first
        self.frames: Dict[int, int] = {}        # live slot -> frames fed so far
        self.first_use: Dict[int, dict] = {}    # slot -> the (K, W, max_frames) of the call that last reset it
        self.n_grown = 0

    @property
    def n_free(self) -> int:
        return len(self._free)

    @property
    def live(self):
        return sorted(self.frames)

    def acquire(self) -> int:
        """The lowest free slot (the slab doubles when none is left).  Its first `extend` must say reset."""
        if not self._free:
            self.grow()
        slot = self._free.pop(0)
        self.frames[slot] = 0
        return slot

    def release(self, slot: int) -> None:
        if slot not in self.frames:
            raise ValueError(f"slot {slot} is not in use")
        del self.frames[slot]
        self.first_use.pop(slot, None)
        self._free.append(int(slot))
        self._free.sort()

    def grow(self, n_slots: Optional[int] = None) -> None:
        """A new slab of `n_slots` (default: twice as many) slots; the old slots are copied to the same indices."""
        n = 2 * self.n_slots if n_slots is None else int(n_slots)
        if n <= self.n_slots:
            raise ValueError(f"grow({n}): the slab holds {self.n_slots} slots already")
        slab = torch.empty(n, self.slot_bytes, dtype=torch.uint8, device=self.slab.device)
        slab[: self.n_slots].copy_(self.slab)
        self._free += list(range(self.n_slots, n))
        self.slab, self.n_slots = slab, n
        self.n_grown += 1


class TsyncTick:
    """What one `extend_candidates` call enqueued: the nine device outputs (tokens (S, nbest, max_frames), lens, count, the
    four score columns, frames, status) and what `collect` needs on the host."""

    def __init__(self, outs, state, slots, n_new, shape):
        self.outs, self.state, self.slots, self.n_new, self.shape = outs, state, list(slots), list(n_new), shape
        self.frames: Optional[List[int]] = None  # per row, after collect
        self.used = int(outs[0].shape[2])        # the token columns that travel to the host
        self.hyps = None                         # per row the n-best list, after collect


class PendingCollect:
    """The queued D2H copy of a search's outputs (`BeamSearchTimeSync.collect_start`); `result()` waits for it."""

    def __init__(self, bs, tick, host, event, shape):
        self._bs, self._tick, self._host, self._event, self._shape, self._res = bs, tick, host, event, shape, None

    def done(self) -> bool:
        return self._res is not None or self._event.query()

    def result(self) -> List[List[Hypothesis]]:
        if self._res is None:
            self._event.synchronize()
            self._res = self._bs._collect_finish(self._tick, self._host, self._shape)
            self._host = None
        return self._res


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

    # ------------------------------------------------------------------ the resumable form (streams and pools)
    def stream_state(self, n_slots: int, max_frames: int, device, K: Optional[int] = None) -> TsyncStreamState:
        """The state slab for `n_slots` live utterances of at most `max_frames` encoder frames each (K: the candidates per
        frame, default: those of this search's CTC vocabulary)."""
        K = self._checked_k(self.ctc.odim) if K is None else int(K)
        W_max, K_max = limits()
        if self.beam_size > W_max or K > K_max:
            raise NotImplementedError(f"BeamSearchTimeSync: beam_size {self.beam_size} with {K} candidates per frame is above "
                                      f"the limit of the device walk (beam_size <= {W_max}, candidates <= {K_max})")
        per = int(L.load().em_ctc_tsync_state_bytes(int(max_frames), K, self.beam_size))
        if per <= 0:
            raise ValueError(f"em_ctc_tsync_state_bytes refuses max_frames {max_frames}, K {K}, beam_size {self.beam_size}")
        return TsyncStreamState(n_slots, max_frames, per, device, K=K, W=self.beam_size)

    def extend_candidates(self, cand_id, cand_lp, blank_lp, n_new, slots, reset, state: TsyncStreamState,
                          nbest: Optional[int] = None) -> TsyncTick:
        """`em_ctc_tsync_extend`: row r's first n_new[r] frames of the candidate tables (S, Tc, K) go to the utterance in
        slots[r] of `state` (reset[r]: it starts there); the n-best lists so far come back.  Only enqueues."""
        lib, dev = L.load(), cand_id.device
        S, Tc, K = (int(v) for v in cand_id.shape)
        slots, n_new, reset = [int(v) for v in slots], [int(v) for v in n_new], [int(bool(v)) for v in reset]
        if not (len(slots) == len(n_new) == len(reset) == S):
            raise ValueError(f"n_new, slots and reset must have one entry per row ({S})")
        if len(set(slots)) != S or any(s < 0 or s >= state.n_slots for s in slots):
            raise ValueError(f"slots must be distinct and inside [0, {state.n_slots}): {slots}")
        if state.slab.device != dev:
            raise ValueError("the state slab and the candidate tables live on different devices")
        nb, Tn = int(nbest or self.nbest), state.max_frames
        ctl = torch.tensor([n_new, slots, reset], dtype=torch.int32).to(dev, non_blocking=True)
        tokens = torch.empty(S, nb, Tn, dtype=torch.int32, device=dev)
        lens = torch.empty(S, nb, dtype=torch.int32, device=dev)
        count, frames, status = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
        sc = [torch.empty(S, nb, dtype=torch.float32, device=dev) for _ in range(4)]
        model = None
        if self.ngram is not None and self.weights["ngram"] != 0.0:
            model = C.byref(self.ngram.packed(dev).w)
        L.check(lib.em_ctc_tsync_extend(L.ptr(cand_id.contiguous()), L.ptr(cand_lp.contiguous()), L.ptr(blank_lp.contiguous()),
                                        L.ptr(ctl[0]), L.ptr(ctl[1]), L.ptr(ctl[2]), S, Tc, K, self.beam_size, Tn, nb,
                                        self.sos, self.blank, self.weights["ctc"], self.weights["ngram"],
                                        self.weights["length_bonus"], model, L.ptr(state.slab), state.n_slots,
                                        state.slot_bytes, L.ptr(tokens), L.ptr(lens), L.ptr(count), L.ptr(sc[0]), L.ptr(sc[1]),
                                        L.ptr(sc[2]), L.ptr(sc[3]), L.ptr(frames), L.ptr(status), L.current_stream_ptr()),
                "em_ctc_tsync_extend")
        shape = dict(K=K, W=self.beam_size, max_frames=Tn)
        used = 1
        for s, n, r in zip(slots, n_new, reset):
            if r:
                state.first_use[s] = shape  # (what the slot's header will carry: `collect` names a mismatch from it)
            if s in state.frames:  # (the host's own count of the frames it fed: ticks may be in flight)
                state.frames[s] = (0 if r else state.frames[s]) + max(0, min(n, Tc))
                used = max(used, state.frames[s])
            else:  # (a slot the allocator does not track: the whole row travels)
                used = Tn
        tick = TsyncTick((tokens, lens, count, *sc, frames, status), state, slots, n_new, shape)
        tick.used = min(used, Tn)
        return tick

    def extend(self, enc_act: torch.Tensor, n_new, slots, reset, state: TsyncStreamState, nbest: Optional[int] = None):
        """enc_act (S, Tc, d): this call's new encoder frames per row -> `CTC.frame_topk_device`, then `extend_candidates`."""
        L.require_gpu(enc_act, "enc_act")
        tabs = self.ctc.frame_topk_device(enc_act, state.shape["K"], self.blank)
        return self.extend_candidates(*tabs, n_new, slots, reset, state, nbest)

    @staticmethod
    def _raise_status(tick: TsyncTick, row: int, st: int, frames: int):
        slot = tick.slots[row]
        if st == 1:
            raise RuntimeError(f"time-synchronous stream search: row {row} (slot {slot}) holds {frames} frames and "
                               f"{tick.n_new[row]} more would exceed tsync_max_frames = {tick.state.max_frames}; the call "
                               "consumed nothing for it")
        if st == 2:
            first = tick.state.first_use.get(slot)
            diff = [] if first is None else [f"{k} (the slot was first used with {first[k]}, the call has {v})"
                                             for k, v in tick.shape.items() if first[k] != v]
            what = ", ".join(diff) if diff else "the slot was never reset"
            raise RuntimeError(f"time-synchronous stream search: row {row} (slot {slot}) does not match its slot's header: {what}")
        raise RuntimeError(f"time-synchronous stream search: row {row}: slot {slot} is outside the slab (status {st})")

    # ------------------------------------------------------------------ host part
    def _pack(self, outs):
        tick = outs if isinstance(outs, TsyncTick) else None
        extra = []
        if tick is not None:
            tokens, lens, count, score, s_ctc, s_ng, s_len, frames, status = tick.outs
            # (a hypothesis has at most as many tokens as its utterance has frames: what the host fed bounds the columns)
            tokens = tokens[:, :, : max(1, min(tick.used, tokens.shape[2]))]
            extra = [frames.reshape(-1, 1), status.reshape(-1, 1)]
        else:
            tokens, lens, count, score, s_ctc, s_ng, s_len = outs
        B, nb, T = tokens.shape
        # (one packed transfer: the int32 outputs and the f32 scores' bits side by side)
        flat = torch.cat([tokens.reshape(B, -1), lens, count.reshape(B, 1)] +
                         [s.view(torch.int32) for s in (score, s_ctc, s_ng, s_len)] + extra, dim=1)
        return tick, flat, (B, nb, T)

    def collect_start(self, outs) -> "PendingCollect":
        """The enqueued half of `collect`: the outputs packed side by side on the device and ONE copy of them queued into
        pinned host memory behind the launches, with an event.  Nothing waits."""
        tick, flat, shape = self._pack(outs)
        host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return PendingCollect(self, tick, host, event, shape)

    def collect(self, outs) -> List[List[Hypothesis]]:
        """The one D2H copy and the n-best lists: per utterance Hypothesis(yseq = [sos] tokens [sos], score, scores).  Of a
        TsyncTick, `frames` and `status` ride in the same copy: a nonzero status raises RuntimeError by name."""
        tick, flat, shape = self._pack(outs)
        return self._collect_finish(tick, flat.cpu(), shape)

    def _collect_finish(self, tick, flat, shape) -> List[List[Hypothesis]]:
        B, nb, T = shape
        if tick is not None:
            fr, stt = flat[:, -2].tolist(), flat[:, -1].tolist()
            flat = flat[:, :-2]
            tick.frames = [int(v) for v in fr]
            for r, st in enumerate(stt):
                if st != 0:  # (the row consumed nothing: the host's count of what it fed goes back)
                    if tick.slots[r] in tick.state.frames:
                        tick.state.frames[tick.slots[r]] -= tick.n_new[r]
            for r, st in enumerate(stt):
                if st != 0:
                    self._raise_status(tick, r, int(st), int(fr[r]))
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
        if tick is not None:
            tick.hyps = res
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
