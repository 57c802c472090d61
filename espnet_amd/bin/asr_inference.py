"""Speech2Text: the object API of the drop-in.

Mirrors espnet2/bin/asr_inference.py:73-677: same constructor keywords (those outside the hot
path are accepted and must keep their default), `__call__(speech) -> [(text, token, token_int,
Hypothesis)]` for ONE utterance, plus `batch_decode(...)` — the utterance-batched entry the
MI355X path adds (precedents in the reference: bin/asr_inference_k2.py:233-262,
bin/s2t_inference_ctc.py:700-749).

Decoding modes
  * ctc_greedy=True (G1): per-frame argmax + groupby + drop
    blank/sos/eos (asr_inference.py:574-575) — bit-exact integer contract, fully on device.
  * a transducer model (decoder: transducer): BeamSearchTransducer built from `transducer_conf` and `beam_size` -
    the fused greedy walk or the default beam search, espnet_amd/asr/transducer/.
  * time_sync=True with ctc_weight=1.0: the time-synchronous CTC prefix beam search with n-gram fusion
    (BeamSearchTimeSync, espnet_amd/nets/beam_search_timesync.py; csrc/ctc_tsync.hip).
  * otherwise: label-synchronous joint CTC/attention beam search (BatchBeamSearch semantics,
    espnet2/legacy/nets/batch_beam_search.py) — see espnet_amd/nets/.
The log markers "speech length: N" and "best hypo: ..." that utils/calculate_rtf.py parses are kept.
"""
import functools
import logging
from pathlib import Path
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from espnet_amd.lib import TooShortUttError
from espnet_amd.nets.beam_search import Hypothesis
from espnet_amd.nets.candidates import CandidateBatch, is_one_transcript
from espnet_amd.nets_utils import SUBSAMPLING_CONVS
from espnet_amd.tasks.asr import ASRTask
from espnet_amd.text.token_id_converter import TokenIDConverter, build_tokenizer

logger = logging.getLogger(__name__)


def resolve_dtype(dtype: str) -> str:
    """The reference's --dtype values onto the two MFMA modes: float32 (exact-f32 MFMA, the parity mode) and
    bfloat16 (bf16 MFMA, f32 accumulate).  float16 / float64 have no counterpart on this path: they run as the
    nearest mode and say so."""
    if dtype in ("float32", "bfloat16"):
        return dtype
    if dtype == "float16":
        logger.warning("dtype float16 runs as bfloat16 on the MI355X path (bf16 MFMA, f32 accumulate)")
        return "bfloat16"
    if dtype == "float64":
        logger.warning("dtype float64 runs as float32 on the MI355X path (exact-f32 MFMA)")
        return "float32"
    raise ValueError(f"unknown dtype {dtype!r}")


def check_transducer_lm(asr_model, lm_train_config, ngram_file, beam_size):
    """What a transducer model refuses of the LM options, decided before any LM file is opened: an n-gram, and a neural LM
    at a beam the device walk does not hold (the per-utterance host search with an LM takes tens of seconds per batch
    there; it is not a silent default)."""
    if not asr_model.use_transducer_decoder:
        return
    if ngram_file is not None:
        raise NotImplementedError("ngram_file with a transducer model: n-gram fusion in the transducer search is outside "
                                  "the MI355X hot path")
    if lm_train_config is not None:
        from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

        limit = beam_limits()["beam"]
        if beam_size > limit:
            raise NotImplementedError(f"lm_train_config with a transducer model at beam_size={beam_size}: language-model "
                                      f"fusion runs at the beams the device walk holds, up to {limit}")


def pack_modules(device, modules):
    """The weights of the modules a decode will use repacked for the kernels now, not inside the first decode call (an LM
    after the search has aligned its compute dtype with the decoder's)."""
    dev = torch.device(device if ":" in str(device) else f"{device}:{torch.cuda.current_device()}")
    for m in modules:
        if m is not None and hasattr(m, "packed"):
            m.packed(dev)


class Speech2Text:
    def __init__(self, asr_train_config: Union[Path, str, None] = None,
                 asr_model_file: Union[Path, str, None] = None, transducer_conf: Optional[Dict] = None,
                 lm_train_config: Union[Path, str, None] = None, lm_file: Union[Path, str, None] = None,
                 ngram_scorer: str = "full", ngram_file: Union[Path, str, None] = None,
                 token_type: Optional[str] = None, bpemodel: Optional[str] = None, device: str = "cuda",
                 maxlenratio: float = 0.0, minlenratio: float = 0.0, batch_size: int = 1,
                 dtype: str = "float32", beam_size: int = 20, ctc_weight: float = 0.5,
                 lm_weight: float = 1.0, ngram_weight: float = 0.9, penalty: float = 0.0,
                 nbest: int = 1, normalize_length: bool = False, streaming: bool = False,
                 ctc_greedy: bool = False, time_sync: bool = False, **unsupported):
        for k, v in unsupported.items():
            if v not in (None, False, {}, [], 0.99, 5, -1, ["Linear"], "qint8"):
                raise NotImplementedError(f"Speech2Text({k}={v!r}) is outside the MI355X hot path")
        if streaming:
            raise NotImplementedError("streaming=True (use Speech2TextStreaming)")
        if not str(device).startswith("cuda"):
            raise RuntimeError("espnet_amd.Speech2Text runs on an MI355X only (device='cuda'); no CPU fallback")
        if time_sync:  # asr_inference.py: BeamSearchTimeSync in place of the label-synchronous search
            if ctc_greedy:
                raise ValueError("time_sync=True and ctc_greedy=True are two different decoders: choose one")
            if float(ctc_weight) != 1.0:
                raise NotImplementedError(f"time_sync=True with ctc_weight={ctc_weight}: the attention decoder is not scored "
                                          "time-synchronously on the MI355X path; pass ctc_weight=1.0")
            if lm_train_config is not None:
                raise NotImplementedError("time_sync=True with lm_train_config: a neural LM is not scored time-synchronously "
                                          "on the MI355X path; an n-gram (ngram_file) is")
        # the reference's `dtype` is the model dtype; here it selects the MFMA mode
        dtype = resolve_dtype(dtype)
        asr_model, asr_train_args = ASRTask.build_model_from_file(
            asr_train_config, asr_model_file, device, compute_dtype=dtype)
        self.asr_model = asr_model
        self.asr_train_args = asr_train_args
        self.device, self.dtype = device, dtype
        self.beam_size, self.ctc_weight, self.penalty = beam_size, ctc_weight, penalty
        self.maxlenratio, self.minlenratio, self.nbest = maxlenratio, minlenratio, nbest
        self.normalize_length = normalize_length
        self.ctc_greedy = ctc_greedy
        self.time_sync = bool(time_sync)
        if time_sync and asr_model.use_transducer_decoder:
            raise NotImplementedError("time_sync=True with a transducer model: the time-synchronous search is CTC's "
                                      "(the transducer has its own searches: transducer_conf)")
        token_list = asr_model.token_list
        if token_type is None:
            token_type = getattr(asr_train_args, "token_type", None)
        if bpemodel is None:
            bpemodel = getattr(asr_train_args, "bpemodel", None)
        if token_type is None or (token_type == "bpe" and bpemodel is None):
            self.tokenizer = None
        else:
            self.tokenizer = build_tokenizer(token_type=token_type, bpemodel=bpemodel)
        self.converter = TokenIDConverter(token_list=token_list)
        self.beam_search = self.beam_search_transducer = self.beam_search_timesync = None
        self.lm = self.lm_model = self.ngram = None
        if time_sync:
            from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync
            from espnet_amd.nets.scorers.ctc import CTCPrefixScorer

            if ngram_file is not None:
                from espnet_amd.nets.scorers.ngram import NgramFullScorer, NgramPartScorer

                self.ngram = (NgramFullScorer if ngram_scorer == "full" else NgramPartScorer)(ngram_file, token_list)
            scorers = dict(ctc=CTCPrefixScorer(ctc=asr_model.ctc, eos=asr_model.eos))
            if self.ngram is not None:
                scorers["ngram"] = self.ngram
            self.beam_search_timesync = BeamSearchTimeSync(
                sos=asr_model.sos, beam_size=beam_size, scorers=scorers, token_list=token_list, blank=asr_model.blank_id,
                weights=dict(ctc=ctc_weight, ngram=ngram_weight if self.ngram is not None else 0.0, length_bonus=penalty))
        elif asr_model.use_transducer_decoder:  # asr_inference.py: BeamSearchTransducer in place of the joint search
            check_transducer_lm(asr_model, lm_train_config, ngram_file, beam_size)
            if ctc_greedy and lm_train_config is not None:
                logger.info("ctc_greedy=True decodes with the CTC head alone: lm_train_config is not used")
            if not ctc_greedy:
                from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

                lm_kw = {}
                if lm_train_config is not None:  # shallow fusion: BeamSearchTransducer(lm=..., lm_weight=...)
                    from espnet_amd.tasks.lm import LMTask

                    self.lm_model, _ = LMTask.build_model_from_file(lm_train_config, lm_file, device, compute_dtype=dtype)
                    self.lm = self.lm_model.lm
                    lm_kw = dict(lm=self.lm, lm_weight=lm_weight)
                self.beam_search_transducer = BeamSearchTransducer(
                    decoder=asr_model.decoder, joint_network=asr_model.joint_network, beam_size=beam_size,
                    nbest=nbest, token_list=token_list, **lm_kw, **(transducer_conf or {}))
        elif transducer_conf is not None:
            raise ValueError("transducer_conf was given, but the model has no joint network (decoder: transducer)")
        elif not ctc_greedy:  # (greedy CTC decodes without scorers: an n-gram does not apply there)
            from espnet_amd.nets.batch_beam_search import build_beam_search

            lm = None
            if lm_train_config is not None:  # asr_inference.py:179-191
                from espnet_amd.tasks.lm import LMTask

                lm_model, _ = LMTask.build_model_from_file(lm_train_config, lm_file, device, compute_dtype=dtype)
                lm = lm_model.lm
                self.lm_model = lm_model  # (its `nll`: the LM term of `batch_rescore`)
            self.lm = lm
            if ngram_file is not None:  # asr_inference.py:193-207
                from espnet_amd.nets.scorers.ngram import NgramFullScorer, NgramPartScorer

                cls = NgramFullScorer if ngram_scorer == "full" else NgramPartScorer
                self.ngram = cls(ngram_file, token_list)
            self.beam_search = build_beam_search(
                asr_model, beam_size=beam_size, ctc_weight=ctc_weight, penalty=penalty,
                lm_weight=lm_weight if lm is not None else 0.0, token_list=token_list,
                normalize_length=normalize_length, lm=lm, ngram=self.ngram,
                ngram_weight=ngram_weight if self.ngram is not None else 0.0)
        m = asr_model
        pack_modules(device, [m.frontend, m.encoder, m.ctc] +
                     ([] if ctc_greedy else [self.ngram] if time_sync else [m.decoder, m.joint_network, self.lm, self.ngram]))

    # ------------------------------------------------------------------ single utterance (reference API)
    @torch.no_grad()
    def __call__(self, speech: Union[torch.Tensor, np.ndarray]):
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        speech = speech.unsqueeze(0).to(torch.float32)  # (1, N), asr_inference.py:514
        logger.info("speech length: " + str(speech.size(1)))
        return self.batch_decode(speech, [speech.size(1)])[0]

    # ------------------------------------------------------------------ utterance batch (MI355X API)
    @torch.no_grad()
    def batch_decode(self, speech: torch.Tensor, speech_lengths: Sequence[int]):
        """speech (B, N) zero padded (host or device), lengths host ints.  Returns one reference-
        shaped result list per utterance; row b is what `__call__` returns for utterance b alone
        (isolated-utterance encoding: the reference decodes one utterance per call)."""
        speech = speech.to(self.device, torch.float32, non_blocking=True)
        st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
        if self.ctc_greedy:
            return self._finish_greedy(*self.decode_greedy_device(st))
        if self.beam_search_timesync is not None:
            hyps = self.beam_search_timesync.search_batch(st.enc_act, st.olens, nbest=self.nbest)
            return [self._format(h[: self.nbest]) for h in hyps]
        if self.beam_search_transducer is not None:
            hyps = self.beam_search_transducer.search_batch(st.enc_act, st.olens)
            return [self._format_transducer(h[: self.nbest]) for h in hyps]
        hyps = self.beam_search.search_batch(st.enc_act, st.olens, maxlenratio=self.maxlenratio,
                                             minlenratio=self.minlenratio)
        return [self._format(h[: self.nbest]) for h in hyps]

    @torch.no_grad()
    def batch_decode_async(self, speech: torch.Tensor, speech_lengths: Sequence[int]):
        """Like `batch_decode`, but for greedy CTC the device work is only ENQUEUED: the returned
        handle's `.result()` waits for this batch alone (an event after its D2H copy), so the caller can
        enqueue the next batch first and format this one while the GPU runs.  The beam search polls the
        device between step chunks and therefore completes inside this call."""
        if self.beam_search_transducer is not None or self.beam_search_timesync is not None:
            # (these walks read back once, at their end: complete inside this call)
            return _Done(self.batch_decode(speech, speech_lengths))
        if not self.ctc_greedy:
            # Round 6: several joint searches in flight (espnet_amd.nets.batch_beam_search.SearchLanes) - this batch is encoded
            # and its search started on a free lane's stream, the handle's `.result()` drives the lanes until it has ended.
            # A caller that submits batch n + 1 before it asks for batch n (the decode CLI does) keeps the lanes busy.
            lanes = self.__dict__.get("_lanes")
            if lanes is None:
                from espnet_amd.nets.batch_beam_search import SearchLanes

                # (four lanes, a host thread each: with ONE host thread two lanes already saturate the host's launch rate -
                # 2 / 3 / 4 lanes 60.4 / 60.3 / 60.9 ms per batch of 16 - with a thread per lane 4 lanes reach 48.0;
                # profiles/r06z_beam_lanes_threads_ab.txt.  `search_lanes` / `lane_threads` attributes: set before the first call)
                # (round 6, late: eight lanes while a search's launches leave most of the chip idle - up to ~200 rows = batch x beam:
                # 4 / 6 / 8 lanes 4 033 / 4 083 / 4 705 audio-s/s at 16 x beam 10; at 64 x beam 10 four lanes are as good as eight,
                # profiles/r06al_beam_lanes_sweep.txt)
                rows = int(speech.shape[0]) * int(getattr(self.beam_search, "beam_size", 10))
                n_lanes = max(1, int(getattr(self, "search_lanes", None) or (8 if rows <= 200 else 4)))
                lanes = self._lanes = SearchLanes([self.beam_search] + [self.beam_search.clone() for _ in range(n_lanes - 1)],
                                                  self.device, threaded=bool(getattr(self, "lane_threads", True)))
            k = lanes.free_lane()
            if k is None:  # (every lane carries a search nobody has asked for yet: finish this one on the calling stream)
                return _Done(self.batch_decode(speech, speech_lengths))
            with torch.cuda.stream(lanes.stream(k)):
                speech = speech.to(self.device, torch.float32, non_blocking=True)
                st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
            lanes.start(k, st.enc_act, st.olens, tag=(st, speech), maxlenratio=self.maxlenratio, minlenratio=self.minlenratio)
            return _PendingBeam(self, lanes, k)
        # (round 6: consecutive batches go to alternating HIP streams - every kernel of the greedy step takes the whole chip,
        # but one stream's launch fills the boundary between two dependent launches of the other: DESIGN.md 4g)
        pair = self.__dict__.get("_greedy_streams")
        if pair is None:
            pair = self._greedy_streams = [torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)]
            self._greedy_turn = 0
        stream = pair[self._greedy_turn & 1]
        self._greedy_turn += 1
        stream.wait_stream(torch.cuda.current_stream())  # (whatever produced `speech` on the caller's stream)
        with torch.cuda.stream(stream):
            speech = speech.to(self.device, torch.float32, non_blocking=True)
            st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
            tokens, tlens = self.decode_greedy_device(st)
            tok_h = torch.empty(tokens.shape, dtype=tokens.dtype).pin_memory()
            len_h = torch.empty(tlens.shape, dtype=tlens.dtype).pin_memory()
            tok_h.copy_(tokens, non_blocking=True)
            len_h.copy_(tlens, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return _PendingGreedy(self, tok_h, len_h, ev, (tokens, tlens, st, speech))

    # ------------------------------------------------------------------ forced alignment: token timestamps
    # texts=None: up to this many encoder frames the greedy tokens go to the trellis as they are, (B, T) - at most 255
    # tokens, one wave per utterance whatever their number - and nothing is read back before the launch
    align_no_sync_frames = 255

    @property
    def seconds_per_frame(self) -> float:
        """Duration of one encoder frame: subsampling x hop_length / fs (subsampling 4, 6 or 8 from the encoder's
        `input_layer`).  The receptive-field offset of the subsampling convolutions is NOT modelled: frame t is
        reported as [t, t + 1) x seconds_per_frame."""
        enc, fe = self.asr_model.encoder, self.asr_model.frontend
        layer = getattr(enc, "input_layer", "conv2d")
        if layer not in SUBSAMPLING_CONVS:
            raise ValueError(f"input_layer={layer!r}: no subsampling factor known for it")
        sub = 1
        for _, stride in SUBSAMPLING_CONVS[layer]:
            sub *= stride
        return sub * int(fe.hop_length) / float(fe.fs)

    def _target_ids(self, text):
        """A transcript (string or token ids) -> list of ids; ValueError for what cannot be aligned."""
        if isinstance(text, str):
            if self.tokenizer is None:
                raise ValueError("a text transcript needs a tokenizer (token_type / bpemodel); pass token ids instead")
            ids = self.converter.tokens2ids(self.tokenizer.text2tokens(text))
        else:
            ids = text.tolist() if hasattr(text, "tolist") else list(text)
        ids = [int(v) for v in ids]
        m = self.asr_model
        bad = {m.blank_id: "<blank>", m.sos: "<sos/eos>", m.eos: "<sos/eos>"}
        for v in ids:
            if v in bad:
                raise ValueError(f"token id {v} ({bad[v]}) cannot be aligned")
        return ids

    def _batch_of_one(self, batch, speech, text):
        """`batch`, one of the batch aligners, for one utterance."""
        speech = (torch.tensor(speech) if isinstance(speech, np.ndarray) else speech).unsqueeze(0).to(torch.float32)
        return batch(speech, [speech.size(1)], None if text is None else [text])[0]

    def _token_times(self, speech, speech_lengths, texts, check_ids, hypothesis, min_width, run, row_result):
        """The shared driver of the batch aligners behind their model-kind refusal: texts -> ids (check_ids(ids): what the
        aligner refuses beyond `_target_ids`), the encode, then run(st, ids, tokens, tlens) -> the aligner's output columns,
        (B, w) device tensors.  texts=None: ids is None and hypothesis(st) gives the own hypothesis as device (tokens (B, T),
        tlens (B,), no_sync); token rows wider than no_sync are cut to the longest hypothesis, at least min_width.  One D2H
        copy brings the columns and, behind them, `tlens | tokens`; row_result(cols, y, names, T_b, spf) formats
        utterance b from its row of every column, its ids and their token names, its encoder frames and
        `seconds_per_frame`."""
        B = int(speech.shape[0])
        ids = tokens = tlens = None
        if texts is not None:
            if len(texts) != B:
                raise ValueError(f"{len(texts)} transcripts for {B} utterances")
            ids = [self._target_ids(t) for t in texts]
            check_ids(ids)
        speech = speech.to(self.device, torch.float32, non_blocking=True)
        st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
        if ids is None:
            tokens, tlens, no_sync = hypothesis(st)
            if tokens.shape[1] > no_sync:
                # the row stride is the kernels' Lmax - the waves per utterance and the back-pointer workspace of the CTC
                # trellis, the steps of the prediction network and the threads of the lattice recursion up to its cap:
                # one small sync for the longest hypothesis
                tokens = tokens[:, : max(int(tlens.max()), min_width)].contiguous()
        cols = list(run(st, ids, tokens, tlens))
        n_out = len(cols)
        if tokens is not None:
            cols += [tlens[:, None], tokens]
        # the one D2H copy: everything as f32 columns of one matrix (frame counts and ids are far below 2**24)
        host = torch.cat([c.to(torch.float32) for c in cols], dim=1).cpu().numpy()
        parts = np.split(host, np.cumsum([int(c.shape[1]) for c in cols])[:-1], axis=1)
        spf = self.seconds_per_frame
        results = []
        for b in range(B):
            y = ids[b] if ids is not None else parts[-1][b, : int(parts[-2][b, 0])].astype(np.int64).tolist()
            results.append(row_result([c[b] for c in parts[:n_out]], y, self.converter.ids2tokens(y), st.olens[b], spf))
        return results

    @torch.no_grad()
    def align(self, speech: Union[torch.Tensor, np.ndarray], text=None):
        """Token timestamps of one utterance: `batch_align` for a batch of one."""
        return self._batch_of_one(self.batch_align, speech, text)

    @torch.no_grad()
    def batch_align(self, speech: torch.Tensor, speech_lengths: Sequence[int], texts=None):
        """CTC forced alignment (`CTC.forced_align_device`) of one transcript per utterance: speech (B, N) zero padded,
        lengths host ints, texts[b] a string (tokenised with this object's tokenizer) or a list of token ids;
        texts=None aligns every utterance's own greedy CTC tokens, so one call gives hypothesis and timings.  Needs
        only frontend, encoder and CTC head: works with and without `ctc_greedy`.

        Returns per utterance a dict: `tokens` = [(token, token_id, start_s, end_s, mean_logp)], `frame_labels` (the
        (T_b,) int64 label of every encoder frame), `total` (log-probability of the path).  Times are frame index x
        `seconds_per_frame`; the receptive-field offset of the subsampling convolutions is not modelled.  One D2H copy
        per batch (texts=None beyond `align_no_sync_frames` encoder frames: one more word, the longest hypothesis' length,
        is read first)."""
        m = self.asr_model
        if m.ctc is None:
            raise ValueError("forced alignment needs a CTC head (the model has ctc_weight == 0)")

        def hypothesis(st):
            return (*m.greedy_ctc_device(st)[1:], self.align_no_sync_frames)

        def run(st, ids, tokens, tlens):
            if ids is None:
                outs = m.ctc.forced_align_device(st.enc_act, st.olens_dev, tokens, tlens, m.blank_id)
            else:
                outs = m.ctc.forced_align_device(st.enc_act, st.olens, ids, [len(y) for y in ids], m.blank_id)
            align, _, tok_start, tok_end, tok_lp, total = outs
            return align, tok_start, tok_end, tok_lp, total[:, None]

        def row_result(cols, y, names, Tb, spf):
            align, s, e, lp, total = cols
            toks = [(names[i], int(y[i]), float(s[i]) * spf, float(e[i]) * spf, float(lp[i])) for i in range(len(y))]
            return dict(tokens=toks, frame_labels=torch.from_numpy(align[:Tb].astype(np.int64)), total=float(total[0]))

        return self._token_times(speech, speech_lengths, texts, lambda ids: None, hypothesis, 1, run, row_result)

    # ------------------------------------------------------------------ transducer forced alignment: token timestamps
    @torch.no_grad()
    def transducer_align(self, speech: Union[torch.Tensor, np.ndarray], text=None):
        """Token timestamps of one utterance under a transducer model: `batch_transducer_align` for a batch of one."""
        return self._batch_of_one(self.batch_transducer_align, speech, text)

    def _greedy_walk_device(self, st):
        """The greedy walk's (tokens (B, T) int32, ylens (B,) int32) of an encoded batch, left on the device."""
        from espnet_amd.asr.transducer.beam_search_transducer import MAX_WALK_ROWS, BeamSearchTransducer

        walker = self.beam_search_transducer or getattr(self, "_greedy_walker", None)
        if walker is None:  # (an object built with ctc_greedy=True has no search of its own)
            m = self.asr_model
            walker = self._greedy_walker = BeamSearchTransducer(decoder=m.decoder, joint_network=m.joint_network, beam_size=1)
        B = int(st.enc_act.shape[0])
        parts = [walker.greedy_device(st.enc_act[b0 : b0 + MAX_WALK_ROWS].contiguous(), st.olens_dev[b0 : b0 + MAX_WALK_ROWS])
                 for b0 in range(0, B, MAX_WALK_ROWS)]
        if len(parts) == 1:
            return parts[0][0], parts[0][1]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    @torch.no_grad()
    def batch_transducer_align(self, speech: torch.Tensor, speech_lengths: Sequence[int], texts=None):
        """Transducer forced alignment (`ESPnetASRModel.transducer_align`: the best path through the RNN-T lattice) of one
        transcript per utterance - the token timestamps of a model without CTC head, where `batch_align` has nothing to
        align with.  speech (B, N) zero padded, lengths host ints, texts[b] a string (tokenised with this object's
        tokenizer) or a list of token ids, an empty transcript allowed.  texts=None aligns every utterance's own
        GREEDY-WALK hypothesis (`BeamSearchTransducer.greedy_device`), whatever `beam_size` this object was built with - it
        is `batch_decode`'s hypothesis only for beam_size <= 1 - so one call gives hypothesis and timings; the walk's
        tokens stay on the device.

        Returns per utterance a dict: `tokens` = [(token, token_id, start_s, end_s, logp)] with start_s = frame x
        `seconds_per_frame` and end_s = (frame + 1) x `seconds_per_frame` of the encoder frame at which the token is
        emitted and logp its log-probability at that lattice node; `token_int` (the ids); `frame_u` (the (T_b,) int64
        number of tokens emitted when the path leaves each encoder frame); `total` (log-probability of the path).  An
        utterance without a path - no encoder frame - has total = -inf, and its tokens carry start_s = end_s = -1.0 and
        logp = 0.0: there is no time to report.  Several tokens may share a frame.  The receptive-field offset of the subsampling
        convolutions is not modelled.  One D2H copy per batch (texts=None beyond `align_no_sync_frames` encoder frames:
        one more word, the longest hypothesis' length, is read first)."""
        m = self.asr_model
        if not getattr(m, "use_transducer_decoder", False):
            raise RuntimeError("batch_transducer_align: the model has no joint network (decoder: transducer); the CTC head's "
                               "forced alignment is batch_align")

        def check_ids(ids):
            V = getattr(m, "vocab_size", None)
            if V is not None and any(v < 0 or v >= V for y in ids for v in y):
                raise ValueError(f"token ids must lie in [0, {V})")

        def hypothesis(st):
            from espnet_amd import lib as L

            return (*self._greedy_walk_device(st), min(self.align_no_sync_frames, int(L.load().em_transducer_seq_nll_max_tokens())))

        def run(st, ids, tokens, tlens):
            if ids is None:
                outs = m._transducer_align_rows(st.enc_act, st.olens_dev, tokens, tlens, checked=True)
            else:
                ys = torch.zeros(len(ids), max((len(y) for y in ids), default=0), dtype=torch.long)
                for b, y in enumerate(ids):
                    ys[b, : len(y)] = torch.tensor(y, dtype=torch.long)
                outs = m.transducer_align(st.enc_act, torch.tensor(st.olens), ys, torch.tensor([len(y) for y in ids]))
            tok_frame, tok_logp, frame_u, total = outs
            return frame_u, tok_frame, tok_logp, total[:, None]

        def row_result(cols, y, names, Tb, spf):
            frame_u, fr, lp, total = cols
            toks = [(names[i], int(y[i]), float(fr[i]) * spf, (float(fr[i]) + 1.0) * spf, float(lp[i])) if fr[i] >= 0 else
                    (names[i], int(y[i]), -1.0, -1.0, 0.0) for i in range(len(y))]  # (frame -1: no path)
            return dict(tokens=toks, token_int=[int(v) for v in y], frame_u=torch.from_numpy(frame_u[:Tb].astype(np.int64)),
                        total=float(total[0]))

        return self._token_times(speech, speech_lengths, texts, check_ids, hypothesis, 0, run, row_result)

    # ------------------------------------------------------------------ attention-decoder likelihood of given transcripts
    nll_rows_per_call = 100  # candidates per enqueue (ESPnetASRModel.batchify_nll's default slice)

    _is_one_transcript = staticmethod(is_one_transcript)

    def _candidates(self, speech, texts, lm: bool = False) -> CandidateBatch:
        """texts -> the checked candidate batch of the `batch_*` scorers: every ValueError of theirs, before any encode.
        The ids are bounded by the model's vocabulary (`lm`: and the LM's), so no scorer has to verify them on the device."""
        V = getattr(self.asr_model, "vocab_size", None)
        if lm and V is not None:
            V = min(V, getattr(self.lm_model.lm, "vocab_size", V))
        return CandidateBatch(texts, int(speech.shape[0]), self._target_ids, V)

    def _enqueue_candidates(self, speech, speech_lengths, cb: CandidateBatch, score, min_width: int = 1) -> torch.Tensor:
        """The shared driver of the `batch_*` scorers up to their one D2H copy: encodes the utterances once (as
        `batch_decode` does) and runs the candidates through score(st, olens, sl) in slices of `nll_rows_per_call` - st
        the EncoderState, olens its (B,) int32 host lengths, sl a `CandidateSlice`.  Returns the slices' device tensors
        concatenated; only enqueues."""
        speech = speech.to(self.device, torch.float32, non_blocking=True)
        st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
        olens = torch.tensor(st.olens, dtype=torch.int32)
        return torch.cat([score(st, olens, sl) for sl in cb.slices(self.nll_rows_per_call, min_width)])

    def _score_candidates(self, speech, speech_lengths, cb: CandidateBatch, score, min_width: int = 1) -> list:
        """`_enqueue_candidates` and the one D2H copy of a `batch_*` call: a value (or row of values) per candidate."""
        return self._enqueue_candidates(speech, speech_lengths, cb, score, min_width).cpu().tolist() if len(cb) else []

    @torch.no_grad()
    def batch_nll(self, speech: torch.Tensor, speech_lengths: Sequence[int], texts):
        """Teacher-forced negative log-likelihood of given transcripts under the attention decoder
        (`ESPnetASRModel.nll`): speech (B, N) zero padded, lengths host ints; texts[b] is one transcript or a list of
        candidate transcripts of utterance b (an n-best list to rescore), a transcript being a string (tokenised with
        this object's tokenizer) or a sequence of token ids - an empty one scores <eos> alone.  Returns one list of
        floats per utterance, a value per candidate.  The utterances are encoded as `batch_decode` encodes them; the
        candidates of an utterance share its one projected memory.  One D2H copy per call."""
        cb = self._candidates(speech, texts)
        return cb.regroup(self._score_candidates(speech, speech_lengths, cb, self._decoder_nll))

    def _decoder_nll(self, st, olens, sl):
        """A slice's candidates under the attention decoder, against the memories of the slice's own utterances (only
        those are projected).  The candidates are checked, the lengths are checked here: nothing is verified on the device."""
        if min(st.olens[sl.u0 : sl.u1]) < 1:
            raise ValueError("an utterance without encoder frames has no memory to attend to")
        return self.asr_model._nll_rows(st.enc_act[sl.u0 : sl.u1], olens[sl.u0 : sl.u1], sl.ys, torch.tensor(sl.ylens),
                                        mem_of=torch.tensor(sl.mem_rel, dtype=torch.int32), checked=True)

    # ------------------------------------------------------------------ transducer likelihood of given transcripts
    @torch.no_grad()
    def batch_transducer_nll(self, speech: torch.Tensor, speech_lengths: Sequence[int], texts):
        """-log p(y | x) of given transcripts under a transducer model (`ESPnetASRModel.transducer_nll`, the forward value of
        the RNN-T loss): speech, speech_lengths and texts as `batch_nll` takes them - texts[b] one transcript or a list of
        candidates of utterance b, strings or token ids, an empty transcript allowed.  Returns one list of floats per
        utterance, a value per candidate.  The utterances are encoded as `batch_decode` encodes them; the candidates go
        through in slices of `nll_rows_per_call` and share their utterance's joint-network projection.  One D2H copy per
        call."""
        m = self.asr_model
        if not getattr(m, "use_transducer_decoder", False):
            raise RuntimeError("batch_transducer_nll: the model has no joint network (decoder: transducer); the attention "
                               "decoder's likelihood is batch_nll")
        cb = self._candidates(speech, texts)
        enc_proj = []  # projected at the first slice, once for the batch: every slice reads the same rows

        def score(st, olens, sl):  # against the whole batch
            if not enc_proj:
                enc_proj.append(m.joint_network.enc_proj_device(st.enc_act))
            return m.transducer_nll(st.enc_act, olens, sl.ys, torch.tensor(sl.ylens),
                                    mem_of=torch.tensor(sl.mem_of, dtype=torch.int32), enc_proj=enc_proj[0])

        # (the transducer takes a slice of empty transcripts as zero columns)
        return cb.regroup(self._score_candidates(speech, speech_lengths, cb, score, min_width=0))

    # ------------------------------------------------------------------ the joint score of given transcripts
    @torch.no_grad()
    def batch_rescore(self, speech: torch.Tensor, speech_lengths: Sequence[int], texts):
        """The joint search's own score of given transcripts - an n-best list of another system, of a first pass with a
        small beam - from the three whole-sequence scorers: `CTC.nll_device`, `ESPnetASRModel.nll`'s decoder route and the
        LM's `nll`.  speech, speech_lengths and texts as `batch_nll` takes them.  Returns one list per utterance with a
        dict per candidate, in the caller's order (nothing is sorted, no length normalisation):
          token_int  the candidate's ids;
          scores     keys, sign and meaning of `Hypothesis.scores` as the search fills them: ctc = log p_ctc(y|x),
                     decoder = log p_att(y <eos>|x), lm = log p_lm(y <eos>), length_bonus = len(y) + 1; a scorer whose
                     weight is zero or that the model lacks is absent, as in the search;
          score      the sum of `scores` weighted with `self.beam_search.weights` (accumulated on the host, in key order).
        A candidate its utterance has too few frames for has ctc = -inf.  Needs an object built with the joint search;
        whole-sentence n-gram scoring does not exist (NotImplementedError for an object with `ngram_file`).  The
        utterances are encoded as `batch_decode` encodes them; the candidates go through in slices of
        `nll_rows_per_call`, a slice's candidates sharing their utterance's CTC log-probabilities and projected memory.
        Every scorer only enqueues; one D2H copy per call."""
        if self.ctc_greedy:
            raise RuntimeError("batch_rescore: this object decodes greedy CTC (ctc_greedy=True) and has no joint search whose "
                               "score it could give")
        if self.__dict__.get("beam_search_timesync") is not None:
            raise RuntimeError("batch_rescore: this object decodes with the time-synchronous CTC search (time_sync=True) and "
                               "has no joint search whose score it could give")
        if self.beam_search is None:
            raise RuntimeError("batch_rescore: this is a transducer model; the joint CTC/attention score needs the joint "
                               "search's scorers (the transducer's own likelihood: batch_transducer_nll)")
        if self.ngram is not None:
            raise NotImplementedError("batch_rescore with ngram_file: whole-sentence n-gram scoring is not implemented")
        bs = self.beam_search
        keys = self._rescore_keys()
        cb = self._candidates(speech, texts, lm="lm" in keys)
        vals = self._score_candidates(speech, speech_lengths, cb, functools.partial(self._rescore_columns, keys))
        res = []
        for y, row in zip(cb.ids, vals):
            scores = dict(zip(keys, row))
            res.append(dict(token_int=y, scores=scores, score=sum(float(bs.weights[k]) * v for k, v in scores.items())))
        return cb.regroup(res)

    def _rescore_keys(self):
        return [k for k in ("decoder", "ctc", "length_bonus", "lm") if k in self.beam_search.scorers]

    def _rescore_columns(self, keys, st, olens, sl):
        """A slice's (n, len(keys)) scores for `batch_rescore`, the columns in `keys` order."""
        m, dev = self.asr_model, self.device
        col = {}
        if "decoder" in keys:
            col["decoder"] = -self._decoder_nll(st, olens, sl)
        if "ctc" in keys:
            col["ctc"] = -m.ctc.nll_device(st.enc_act[sl.u0 : sl.u1].contiguous(), st.olens[sl.u0 : sl.u1], sl.ids, sl.ylens,
                                           m.blank_id, mem_of=sl.mem_rel)
        if "lm" in keys:
            col["lm"] = -self.lm_model.nll_of_checked(sl.ys, torch.tensor(sl.ylens), dev).sum(dim=1)
        if "length_bonus" in keys:
            col["length_bonus"] = torch.tensor([n + 1.0 for n in sl.ylens], dtype=torch.float32).to(dev, non_blocking=True)
        return torch.stack([col[k] for k in keys], dim=1)

    def decode_greedy_device(self, st):
        """Device-resident G1 result: (tokens (B,T) i32 padded with -1, token_lens (B,) i32)."""
        _, tokens, tlens = self.asr_model.greedy_ctc_device(st)
        return tokens, tlens

    def _finish_greedy(self, tokens, tlens):
        tokens, tlens = tokens.cpu(), tlens.cpu()  # the one D2H copy of the batch
        return self._finish_greedy_host(tokens, tlens)

    def _finish_greedy_host(self, tokens, tlens):
        """Host tensors (B, T) / (B,) of one batch -> reference-shaped results.  One (B, T+2) int64 matrix holds
        every `yseq` (<sos> ids <eos>); the per-utterance tensors are row views of it."""
        sos, eos = self.asr_model.sos, self.asr_model.eos
        tok, lens = tokens.numpy(), tlens.numpy().tolist()
        B, T = tok.shape
        y = np.empty((B, T + 2), dtype=np.int64)
        y[:, 0] = sos
        y[:, 1 : T + 1] = tok
        for b, n in enumerate(lens):
            y[b, n + 1] = eos
        yt = torch.from_numpy(y)
        return [self._format([Hypothesis(yseq=yt[b, : n + 2])]) for b, n in enumerate(lens)]

    def _format(self, nbest_hyps):
        """asr_inference.py:652-677: strip sos/eos, drop id 0, ids -> tokens -> text."""
        results = []
        for hyp in nbest_hyps:
            token_int = [x for x in hyp.yseq[1:-1].tolist() if x != 0]
            token = self.converter.ids2tokens(token_int)
            text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
            results.append((text, token, token_int, hyp))
        if results and logger.isEnabledFor(logging.INFO):
            logger.info("best hypo: " + "".join(results[0][1]) + "\n")
        return results

    def _format_transducer(self, nbest_hyps):
        """asr_inference.py, the transducer branch: token_int = yseq[1:] without blanks."""
        results = []
        for hyp in nbest_hyps:
            token_int = [x for x in hyp.yseq[1:] if x != 0]
            token = self.converter.ids2tokens(token_int)
            text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
            results.append((text, token, token_int, hyp))
        if results and logger.isEnabledFor(logging.INFO):
            logger.info("best hypo: " + "".join(results[0][1]) + "\n")
        return results

    @staticmethod
    def from_pretrained(model_tag: Optional[str] = None, **kwargs: Optional[Any]):
        if model_tag is not None:
            raise NotImplementedError("model zoo download needs network access (espnet_model_zoo)")
        return Speech2Text(**kwargs)


class _Done:
    def __init__(self, res):
        self._res = res

    def result(self):
        return self._res


class _PendingBeam:
    """A batch whose joint search is in flight on lane `k` of the Speech2Text's `SearchLanes`."""

    def __init__(self, s2t, lanes, k):
        self.s2t, self.lanes, self.k, self._res = s2t, lanes, k, None

    def result(self):
        if self._res is None:
            _tag, hyps = self.lanes.wait(self.k)
            self._res = [self.s2t._format(h[: self.s2t.nbest]) for h in hyps]
        return self._res


class _PendingGreedy:
    """Greedy batch whose kernels and D2H copy are enqueued; `keep` pins the device tensors until then."""

    def __init__(self, s2t, tok_h, len_h, ev, keep):
        self.s2t, self.tok_h, self.len_h, self.ev, self.keep = s2t, tok_h, len_h, ev, keep

    def result(self):
        self.ev.synchronize()
        self.keep = None
        return self.s2t._finish_greedy_host(self.tok_h, self.len_h)


# ---------------------------------------------------------------------- decode CLI (asr.sh stage 12)
def inference(output_dir: str, maxlenratio: float = 0.0, minlenratio: float = 0.0, batch_size: int = 1,
              dtype: str = "float32", beam_size: int = 20, ngpu: int = 1, seed: int = 0,
              ctc_weight: float = 0.5, lm_weight: float = 1.0, ngram_weight: float = 0.9,
              penalty: float = 0.0, nbest: int = 1, normalize_length: bool = False, num_workers: int = 1,
              log_level: Union[int, str] = "INFO", data_path_and_name_and_type=None,
              key_file: Optional[str] = None, asr_train_config: Optional[str] = None,
              asr_model_file: Optional[str] = None, lm_train_config: Optional[str] = None,
              lm_file: Optional[str] = None, word_lm_train_config: Optional[str] = None,
              word_lm_file: Optional[str] = None, ngram_file: Optional[str] = None,
              model_tag: Optional[str] = None, token_type: Optional[str] = None,
              bpemodel: Optional[str] = None, allow_variable_data_keys: bool = False,
              transducer_conf: Optional[dict] = None, streaming: bool = False, ctc_greedy: bool = False,
              bucket_window: int = 8, window_claim=None, **unsupported):
    """The reference's `inference()` (espnet2/bin/asr_inference.py:716-906) for the MI355X path: same
    keywords, same `output_dir/{n}best_recog/{token,token_int,score,text}` files in the key order of the
    input, same per-utterance TooShortUttError fallback (:851-858) — but `batch_size > 1` decodes
    length-bucketed utterance batches (`Speech2Text.batch_decode`) while reader threads load the next
    window.  Returns the RTF summary it also logs (`utils/calculate_rtf.py` reads the log markers)."""
    import time
    from collections import deque

    from espnet_amd.fileio.datadir_writer import DatadirWriter

    if word_lm_train_config is not None:
        raise NotImplementedError("Word LM is not implemented")
    if ngpu > 1:  # the reference raises here (:760-765) and scales by split key files in asr.sh; one node, one call:
        kw = dict(locals())
        kw.update(kw.pop("unsupported"))
        for k in ("time", "deque", "DatadirWriter"):
            kw.pop(k, None)
        return inference_multi_gpu(**kw)
    if ngpu < 1:
        raise RuntimeError("espnet_amd decodes on an MI355X only: pass --ngpu 1 (no CPU fallback)")
    logging.basicConfig(level=log_level,
                        format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    torch.manual_seed(seed)
    np.random.seed(seed)
    speech2text = Speech2Text.from_pretrained(
        model_tag=model_tag, asr_train_config=asr_train_config, asr_model_file=asr_model_file,
        transducer_conf=transducer_conf, lm_train_config=lm_train_config, lm_file=lm_file,
        ngram_file=ngram_file, token_type=token_type, bpemodel=bpemodel, device="cuda",
        maxlenratio=maxlenratio, minlenratio=minlenratio, dtype=dtype, beam_size=beam_size,
        ctc_weight=ctc_weight, lm_weight=lm_weight, ngram_weight=ngram_weight, penalty=penalty, nbest=nbest,
        normalize_length=normalize_length, streaming=streaming, ctc_greedy=ctc_greedy, **unsupported)
    loader = ASRTask.build_streaming_iterator(
        data_path_and_name_and_type, dtype="float32", batch_size=batch_size, key_file=key_file,
        num_workers=num_workers, preprocess_fn=ASRTask.build_preprocess_fn(speech2text.asr_train_args, False),
        collate_fn=ASRTask.build_collate_fn(speech2text.asr_train_args, False),
        allow_variable_data_keys=allow_variable_data_keys, inference=True, ngpu=ngpu,
        bucket_window=bucket_window, window_claim=window_claim)
    fs = 16000
    fconf = getattr(speech2text.asr_train_args, "frontend_conf", None) or {}
    if isinstance(fconf.get("fs", None), int):
        fs = fconf["fs"]

    def too_short():  # asr_inference.py:852-854
        hyp = Hypothesis(score=0.0, scores={}, states={}, yseq=[])
        return [(" ", ["<space>"], [2], hyp)] * nbest

    def submit(keys, batch):
        """Enqueue one batch; returns a zero-argument callable giving its per-utterance results."""
        speech, lens = batch["speech"], [int(n) for n in batch["speech_lengths"]]
        for k, n in zip(keys, lens):
            logger.info(f"speech length: {n}")  # one line per utterance, as :520
        try:
            return speech2text.batch_decode_async(speech, lens).result
        except TooShortUttError as e:
            # a short utterance must not take the batch down: placeholder rows for the short ones
            # (:851-858), the rest decoded as one smaller batch
            bad = set(e.indices if e.indices is not None else range(len(keys)))
            for i in sorted(bad):
                logger.warning(f"Utterance {[keys[i]]} {e if len(bad) == 1 else 'is too short for subsampling'}")
            good = [i for i in range(len(keys)) if i not in bad]
            out = [too_short() for _ in keys]
            if good:
                sub = speech2text.batch_decode(speech[good, : max(lens[i] for i in good)], [lens[i] for i in good])
                for i, r in zip(good, sub):
                    out[i] = r
            return lambda: out

    pending, written, n_samples = {}, 0, 0
    t0 = time.perf_counter()
    with DatadirWriter(output_dir) as writer:
        def drain(keys, get):
            nonlocal written
            for k, res in zip(keys, get()):
                pending[k] = res
            order = loader.key_order
            while written < len(order) and order[written] in pending:  # emit in input order
                key = order[written]
                for n, (text, token, token_int, hyp) in zip(range(1, nbest + 1), pending.pop(key)):
                    w = writer[f"{n}best_recog"]
                    w["token"][key] = " ".join(token)
                    w["token_int"][key] = " ".join(map(str, token_int))
                    w["score"][key] = str(hyp.score)
                    if text is not None:
                        w["text"][key] = text
                written += 1

        # batches stay enqueued on the GPU while earlier ones are formatted and written: one for greedy CTC (two batches in
        # flight on alternating streams), three for the joint search (four searches in flight, a host thread each)
        import collections

        lanes = getattr(speech2text, "search_lanes", None) or (8 if int(batch_size) * int(beam_size) <= 200 else 4)  # (as batch_decode_async)
        depth = 1 if getattr(speech2text, "ctc_greedy", False) else max(1, int(lanes) - 1)
        inflight = collections.deque()
        for keys, batch in loader:
            assert all(isinstance(s, str) for s in keys), keys
            assert len(keys) == batch["speech"].size(0)
            n_samples += int(batch["speech_lengths"].sum())
            inflight.append((keys, submit(keys, batch)))
            while len(inflight) > depth:
                drain(*inflight.popleft())
        while inflight:
            drain(*inflight.popleft())
        assert not pending, sorted(pending)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    audio_s = n_samples / fs
    summary = dict(utterances=written, audio_seconds=audio_s, wall_seconds=dt,
                   rtf=dt / audio_s if audio_s else float("nan"),
                   native_reader_windows=getattr(loader, "native_windows", 0),
                   reader_seconds=dict(getattr(getattr(loader, "_wav", None), "seconds", {})))
    logger.info("decoded %d utterances, %.1f audio-s in %.2f s: RTF %.5f (%.0f audio-s/s)", written, audio_s,
                dt, summary["rtf"], audio_s / dt if dt else float("nan"))
    return summary


# ---------------------------------------------------------------------- --ngpu N: one process per GPU
def _read_keys(data_path_and_name_and_type, key_file):
    path = key_file if key_file is not None else data_path_and_name_and_type[0][0]
    with open(path, encoding="utf-8") as f:
        return [ln.split(maxsplit=1)[0] for ln in f if ln.strip()]


def _first_float(text: str) -> float:
    """The score column as the writer formats it (`str(hyp.score)`: a float, or `tensor(-12.3, ...)`)."""
    import re

    m = re.search(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[-+]?(?:inf|nan)", text)
    return float(m.group(0)) if m else 0.0


def merge_shard_outputs(output_dir, keys, world: int, nbest: int):
    """`output_dir/output.{r+1}/{n}best_recog/{token,token_int,score,text}` of the ranks -> the same files under
    `output_dir`, rows in key order (asr.sh:1636-1648 does this with cat + sort -k1)."""
    from pathlib import Path

    out = Path(output_dir)
    for n in range(1, nbest + 1):
        for name in ("token", "token_int", "score", "text"):
            rows = {}
            for r in range(world):
                f = out / f"output.{r + 1}" / f"{n}best_recog" / name
                if f.exists():
                    for ln in f.read_text(encoding="utf-8").splitlines():
                        k, _, v = ln.partition(" ")
                        rows[k] = v
            if rows:
                (out / f"{n}best_recog").mkdir(parents=True, exist_ok=True)
                with (out / f"{n}best_recog" / name).open("w", encoding="utf-8") as w:
                    for k in keys:
                        if k in rows:
                            w.write(f"{k} {rows[k]}\n")


def sharded_decode_rank(decode_claimed, keys, output_dir, nbest: int, max_len: int, device, window: int = 1):
    """One rank of `--ngpu N`, DYNAMIC dispatch (round 4; was: one static contiguous slab per rank).  The key list is
    cut into windows of `window` utterances (the loader's read-ahead window); `decode_claimed(claim, shard_dir)` runs
    this rank's ONE decode loop over the windows `claim(w)` grants it (espnet_amd.distributed.WindowClaimer over a
    shared counter: a rank asks for its next window when it reaches the previous one, so a slow GPU or a run of long
    utterances takes fewer) into `output_dir/output.{rank+1}` and returns {key: (token ids, score)} of its 1-best.
    The records travel with their global utterance index and are collated ONCE, at the end
    (`gather_variable_records`); rank 0 merges the shard files in key order and cross-checks them against the
    collated records.  A failing rank makes every rank raise (no one is left inside a collective)."""
    from pathlib import Path

    import torch.distributed as dist

    from espnet_amd import distributed as D

    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    shard_dir = Path(output_dir) / f"output.{rank + 1}"
    work = D.work_store() if world > 1 else None
    win_key = D.call_key("asr_inference_windows", work, world)
    claim = D.WindowClaimer(D.SharedCounter(work, win_key))
    # rows of an earlier run into the same output_dir must not be taken for this rank's (the writer opens its files
    # lazily: a rank that claims no window would never truncate them)
    if shard_dir.is_dir():
        import shutil

        for sub in shard_dir.glob("*best_recog"):
            shutil.rmtree(sub, ignore_errors=True)
    err, stats, rec = None, {}, None
    try:
        mine, stats = decode_claimed(claim, shard_dir)
        index = {k: u for u, k in enumerate(keys)}
        ks = sorted(mine, key=index.__getitem__)
        rec = D.pack_indexed_records([index[k] for k in ks], [mine[k][0] for k in ks], [mine[k][1] for k in ks],
                                     max_len, device)
    except Exception as e:  # re-raised below, after the peers have been told
        err = e
    if world > 1:
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32, device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        failed = int(flag.item()) != 0
    else:
        failed = err is not None
    if err is not None:
        raise err
    if failed:
        raise RuntimeError(f"rank {rank}: another rank failed before the hypothesis collation; nothing was gathered")
    hyps = D.unpack_indexed_records(D.gather_variable_records(rec), len(keys))
    D.release_key(work, win_key, rank)  # (behind the collation: every rank is past its last claim)
    if dist.is_initialized():
        dist.barrier()
    if rank == 0:
        merge_shard_outputs(output_dir, keys, world, nbest)
        f = Path(output_dir) / "1best_recog" / "token_int"
        merged = {ln.partition(" ")[0]: [int(t) for t in ln.partition(" ")[2].split()]
                  for ln in f.read_text(encoding="utf-8").splitlines()} if f.exists() else {}
        for k, (toks, _) in zip(keys, hyps):
            assert merged.get(k, []) == toks, f"collated record of {k} differs from the merged shard file"
    return hyps, dict(stats, windows=list(claim.claimed))


def _multi_gpu_worker(rank: int, world: int, port: int, kw: dict, q):
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        res = _inference_rank(kw)
    except BaseException as e:  # tell the parent, then leave WITHOUT a collective: the peers are not in a matching one
        import traceback

        q.put((rank, RuntimeError(f"rank {rank}: {type(e).__name__}: {e}\n{traceback.format_exc()}")))
        try:
            dist.destroy_process_group()
        except Exception:
            pass
        raise SystemExit(1)
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _inference_rank(kw: dict):
    keys = _read_keys(kw["data_path_and_name_and_type"], kw["key_file"])
    nbest = kw["nbest"]
    window = max(1, int(kw.get("batch_size", 1))) * max(1, int(kw.get("bucket_window", 8)))

    def decode_claimed(claim, shard_dir):
        shard_dir.mkdir(parents=True, exist_ok=True)
        sub = dict(kw, output_dir=str(shard_dir), ngpu=1, window_claim=claim)  # the whole key list, claimed windows only
        st = inference(**sub)
        ti, sc = shard_dir / "1best_recog" / "token_int", shard_dir / "1best_recog" / "score"
        rows = {ln.partition(" ")[0]: ln.partition(" ")[2] for ln in ti.read_text().splitlines()} if ti.exists() else {}
        srow = {ln.partition(" ")[0]: ln.partition(" ")[2] for ln in sc.read_text().splitlines()} if sc.exists() else {}
        mine = {k for w in claim.claimed for k in keys[w * window : (w + 1) * window]}  # only what THIS call decoded
        return {k: ([int(t) for t in v.split()], _first_float(srow.get(k, "0"))) for k, v in rows.items() if k in mine}, st

    hyps, st = sharded_decode_rank(decode_claimed, keys, kw["output_dir"], nbest, 4096, torch.device("cuda"), window)
    return dict(st, utterances_total=len(hyps))


def _collect_ranks(procs, q, poll_s: float = 0.5):
    """One result per rank process from `q`, or an exception: a rank that reports a failure or dies without
    reporting (killed, out of memory in native code) ends the whole job - the surviving ranks are terminated
    instead of being left inside a collective nobody will complete (the reference's split-job flow surfaces a
    failed job the same way, asr.sh:1636-1648)."""
    import queue as _queue

    res, err = {}, None
    while len(res) < len(procs) and err is None:
        try:
            rank, r = q.get(timeout=poll_s)
        except _queue.Empty:
            dead = [i for i, p in enumerate(procs) if p.exitcode not in (None, 0) and i not in res]
            if dead:
                err = RuntimeError(f"rank process {dead[0]} exited with {procs[dead[0]].exitcode} before reporting")
            elif all(p.exitcode is not None for p in procs) and q.empty():
                err = RuntimeError("rank processes exited without reporting a result")
            continue
        if isinstance(r, BaseException):
            err = r
        else:
            res[rank] = r
    if err is not None:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
        raise RuntimeError(f"--ngpu {len(procs)}: {err}") from (err if isinstance(err, BaseException) else None)
    for p in procs:
        p.join()
        if p.exitcode != 0:
            raise RuntimeError(f"rank process exited with {p.exitcode}")
    return res


def inference_multi_gpu(ngpu: int, **kw):
    """`--ngpu N` on one node: N processes (one per MI355X) pull read-ahead windows of the key file from a shared
    counter (dynamic dispatch, `sharded_decode_rank`); the hypotheses are collated once at the end with
    `espnet_amd.distributed.gather_variable_records` (RCCL all-gather of fixed-width indexed records) and the
    per-rank files merged in key order.  Under torchrun (RANK / WORLD_SIZE set) this process is one of
    the ranks; otherwise the ranks are spawned here."""
    import os
    import socket

    import torch.distributed as dist

    kw = dict(kw, ngpu=ngpu)
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) == ngpu:
        local = int(os.environ.get("LOCAL_RANK", os.environ["RANK"]))
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        try:
            return _inference_rank(kw)
        finally:
            dist.barrier()
            dist.destroy_process_group()
    if torch.cuda.device_count() < ngpu:
        raise RuntimeError(f"--ngpu {ngpu} but {torch.cuda.device_count()} GPUs are visible")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = torch.multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_multi_gpu_worker, args=(r, ngpu, port, kw, q)) for r in range(ngpu)]
    for p in procs:
        p.start()
    res = _collect_ranks(procs, q)
    audio = sum(r.get("audio_seconds", 0.0) for r in res.values())
    wall = max(r.get("wall_seconds", 0.0) for r in res.values())
    return dict(utterances=sum(r.get("utterances", 0) for r in res.values()), audio_seconds=audio, wall_seconds=wall,
                rtf=wall / audio if audio else float("nan"), ranks=ngpu)


def _str2bool(v: str) -> bool:
    if v.lower() in ("true", "1", "yes", "y", "t"):
        return True
    if v.lower() in ("false", "0", "no", "n", "f"):
        return False
    raise ValueError(f"not a boolean: {v!r}")


def _str_or_none(v: str):
    return None if v.strip().lower() in ("none", "null", "nil", "") else v


def _str2triple_str(v: str):
    """`path,name,type` (espnet2/utils/types.py str2triple_str)."""
    parts = [p.strip().strip("()").strip("'\"") for p in v.split(",")]
    if len(parts) != 3:
        raise ValueError(f"expected 'path,name,type': {v!r}")
    return tuple(parts)


def get_parser():
    """Option names, types and defaults of espnet2/bin/asr_inference.py:911-1137 for the options this
    path implements; `--config` yaml files work like config_argparse; options of other tasks are
    accepted at their reference default and rejected otherwise (Speech2Text checks)."""
    import argparse

    p = argparse.ArgumentParser(description="ASR Decoding (MI355X)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--config", type=str, default=None, help="yaml file with option defaults")
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO",
                   choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--ngpu", type=int, default=1,
                   help="1 = this process decodes on one MI355X; N > 1 = N processes, one per GPU, each decoding a "
                        "slab of the key file (espnet_amd.distributed); 0 is rejected (no CPU fallback)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64", "bfloat16"],
                   help="Data type (the reference's option and default).  float32 = exact-f32 MFMA (the parity mode); "
                        "bfloat16 = bf16 MFMA with f32 accumulation (the fast mode); float16 runs as bfloat16 and "
                        "float64 as float32, with a warning")
    p.add_argument("--num_workers", type=int, default=1, help="audio reader threads")
    g = p.add_argument_group("Input data related")
    g.add_argument("--data_path_and_name_and_type", type=_str2triple_str, required=True, action="append")
    g.add_argument("--key_file", type=_str_or_none)
    g.add_argument("--allow_variable_data_keys", type=_str2bool, default=False)
    g = p.add_argument_group("The model configuration related")
    for name in ("asr_train_config", "asr_model_file", "lm_train_config", "lm_file", "word_lm_train_config",
                 "word_lm_file", "ngram_file", "model_tag"):
        g.add_argument(f"--{name}", type=str)
    g = p.add_argument_group("Beam-search related")
    g.add_argument("--batch_size", type=int, default=1, help="utterances per device batch")
    g.add_argument("--bucket_window", type=int, default=8,
                   help="read-ahead window, in batches, that is sorted by length before batching")
    g.add_argument("--nbest", type=int, default=1)
    g.add_argument("--beam_size", type=int, default=20)
    g.add_argument("--penalty", type=float, default=0.0)
    g.add_argument("--maxlenratio", type=float, default=0.0)
    g.add_argument("--minlenratio", type=float, default=0.0)
    g.add_argument("--ctc_weight", type=float, default=0.5)
    g.add_argument("--lm_weight", type=float, default=1.0)
    g.add_argument("--ngram_weight", type=float, default=0.9)
    g.add_argument("--streaming", type=_str2bool, default=False)
    g.add_argument("--normalize_length", type=_str2bool, default=False)
    g.add_argument("--ctc_greedy", type=_str2bool, default=False,
                   help="G1: arg-max + collapse on the device instead of the beam search")
    g = p.add_argument_group("Text converter related")
    g.add_argument("--token_type", type=_str_or_none, default=None, choices=["char", "bpe", "word", None])
    g.add_argument("--bpemodel", type=_str_or_none, default=None)
    g = p.add_argument_group("Options of other decoding modes (accepted at the reference default only)")
    for name, typ, default in _OTHER_MODE_OPTIONS:
        if typ == "list":
            g.add_argument(f"--{name}", type=str, nargs="*", default=default)
        else:
            g.add_argument(f"--{name}", type=typ, default=default)
    return p


def _yaml_or_none(v: str):
    import yaml

    return None if v.strip().lower() in ("none", "null", "") else yaml.safe_load(v)


# (name, type, reference default) of asr_inference.py:1010-1136 options that select other models
_OTHER_MODE_OPTIONS = [
    ("enh_s2t_task", _str2bool, False), ("multi_asr", _str2bool, False),
    ("quantize_asr_model", _str2bool, False), ("quantize_lm", _str2bool, False),
    ("quantize_modules", "list", ["Linear"]), ("quantize_dtype", str, "qint8"),
    ("transducer_conf", _yaml_or_none, None), ("hugging_face_decoder", _str2bool, False),
    ("hugging_face_decoder_conf", _yaml_or_none, {}), ("time_sync", _str2bool, False),
    ("prompt_token_file", _str_or_none, None), ("lang_prompt_token", _str_or_none, None),
    ("nlp_prompt_token", _str_or_none, None), ("partial_ar", _str2bool, False),
    ("threshold_probability", float, 0.99), ("max_seq_len", int, 5), ("max_mask_parallel", int, -1),
]


def main(cmd=None):
    import sys

    import yaml

    print(" ".join(sys.argv), file=sys.stderr)
    parser = get_parser()
    pre, _ = parser.parse_known_args(cmd)
    if pre.config is not None:  # config_argparse: yaml values become defaults, flags still win
        with open(pre.config, encoding="utf-8") as f:
            parser.set_defaults(**(yaml.safe_load(f) or {}))
    kwargs = vars(parser.parse_args(cmd))
    kwargs.pop("config", None)
    return inference(**kwargs)


if __name__ == "__main__":
    main()
