"""ESPnetASRModel (inference side) on the MI355X.

Mirrors espnet2/asr/espnet_model.py:45-467 for the attributes and methods the inference path
touches: `encode(speech, speech_lengths)`, `_extract_feats`, `.frontend/.normalize/.encoder/
.decoder/.ctc/.joint_network`, `.sos/.eos/.blank_id/.token_list/.vocab_size`, `.use_transducer_decoder`.  State-dict keys are the
reference's (`frontend.logmel.melmat`, `encoder.*`, `decoder.*`, `ctc.ctc_lo.*`).

`nll / batchify_nll` (the attention decoder's teacher-forced likelihood of given transcripts) keep the reference's
signatures and run as one enqueue per batch (TransformerDecoder.sequence_nll, csrc/dec_seq.hip).

`encode` keeps the reference signature (padded batch + lengths, any B); `encode_device` is the
batched device-resident entry the MI355X drop-in adds (precedent in the reference:
espnet2/bin/asr_inference_k2.py:233-262 and bin/s2t_inference_ctc.py:700-749).
"""
from typing import List, Optional, Tuple

import torch

from espnet_amd import lib as L


class EncoderState:
    """Device-resident result of one encode call."""

    __slots__ = ("enc_out", "enc_act", "olens", "olens_dev", "feats", "flens", "ctc_ids")

    def __init__(self, enc_out, enc_act, olens, olens_dev, feats, flens, ctc_ids=None):
        self.enc_out, self.enc_act = enc_out, enc_act
        self.olens, self.olens_dev = olens, olens_dev
        self.feats, self.flens = feats, flens
        self.ctc_ids = ctc_ids  # (B, T) i32 per-frame CTC arg-max when the encoder's last kernel produced it


def build_dec_nll_batch(ys_pad: torch.Tensor, ys_pad_lens: torch.Tensor, sos: int, eos: int,
                        vocab_size: Optional[int] = None):
    """The decoder's sentence pair of ESPnetASRModel.nll (espnet2/asr/espnet_model.py `nll`; add_sos_eos,
    espnet2/asr/../nets_utils), plain tensor work on whatever device `ys_pad` lives on: ys_pad (B, Lt) is cut to its
    longest transcript, then with Lp = longest + 1
        x       = [sos | y], <eos> behind a transcript's end (the reference pads ys_in with <eos> too);
        keymask = 1 at the positions below ys_in_lens = ys_pad_lens + 1, 0 behind;
        target  = [y | eos], -1 behind (the reference's ignore_id positions: nothing is scored there).
    Whatever ys_pad holds behind ys_pad_lens is not looked at.  An empty transcript is valid: it scores <eos> alone.
    With `vocab_size`, a token id outside [0, vocab_size) raises ValueError.  Returns (x, keymask, target), (B, Lp) int32."""
    if ys_pad.dim() != 2 or ys_pad_lens.dim() != 1 or ys_pad.size(0) != ys_pad_lens.size(0) or ys_pad.size(0) == 0:
        raise ValueError(f"ys_pad (B, L) and ys_pad_lens (B,) expected, got {tuple(ys_pad.shape)}, {tuple(ys_pad_lens.shape)}")
    dev = ys_pad.device
    lens = ys_pad_lens.to(device=dev, dtype=torch.long)
    longest, shortest = int(lens.max()), int(lens.min())
    if shortest < 0 or longest > ys_pad.size(1):
        raise ValueError(f"ys_pad_lens must lie in [0, {ys_pad.size(1)}], got {shortest} .. {longest}")
    B, Lp = ys_pad.size(0), longest + 1
    y = ys_pad[:, :longest].to(torch.long)
    pos = torch.arange(Lp, device=dev).unsqueeze(0)
    inside = pos[:, :longest] < lens.unsqueeze(1)
    if vocab_size is not None and bool((((y < 0) | (y >= vocab_size)) & inside).any()):
        raise ValueError(f"token ids must lie in [0, {vocab_size})")
    x = torch.full((B, Lp), eos, dtype=torch.long, device=dev)
    x[:, 0] = sos
    x[:, 1:] = torch.where(inside, y, torch.full_like(y, eos))
    target = torch.full((B, Lp), -1, dtype=torch.long, device=dev)
    target[:, :longest] = torch.where(inside, y, torch.full_like(y, -1))
    target.scatter_(1, lens.unsqueeze(1), eos)
    keymask = pos <= lens.unsqueeze(1)
    return x.to(torch.int32), keymask.to(torch.int32), target.to(torch.int32)


class ESPnetASRModel(torch.nn.Module):
    def __init__(self, vocab_size: int, token_list, frontend, specaug, normalize, preencoder,
                 encoder, postencoder, decoder, ctc, joint_network=None, aux_ctc: dict = None,
                 ctc_weight: float = 0.5, interctc_weight: float = 0.0, ignore_id: int = -1,
                 lsm_weight: float = 0.0, length_normalized_loss: bool = False,
                 report_cer: bool = True, report_wer: bool = True, sym_space: str = "<space>",
                 sym_blank: str = "<blank>", transducer_multi_blank_durations: List = [],
                 transducer_multi_blank_sigma: float = 0.05, sym_sos: str = "<sos/eos>",
                 sym_eos: str = "<sos/eos>", extract_feats_in_collect_stats: bool = True,
                 lang_token_id: int = -1, autocast_frontend: bool = False):
        assert 0.0 <= ctc_weight <= 1.0, ctc_weight
        assert 0.0 <= interctc_weight < 1.0, interctc_weight
        super().__init__()
        if specaug is not None or preencoder is not None or postencoder is not None:
            raise NotImplementedError("specaug/preencoder/postencoder are outside the hot path")
        if joint_network is not None and len(transducer_multi_blank_durations) > 0:
            raise NotImplementedError("transducer_multi_blank_durations: multi-blank transducers are outside the hot path")
        token_list = list(token_list)
        # espnet_model.py:76-87
        self.blank_id = token_list.index(sym_blank) if sym_blank in token_list else 0
        self.sos = token_list.index(sym_sos) if sym_sos in token_list else vocab_size - 1
        self.eos = token_list.index(sym_eos) if sym_eos in token_list else vocab_size - 1
        self.vocab_size = vocab_size
        self.ignore_id = ignore_id
        self.ctc_weight = ctc_weight
        self.interctc_weight = interctc_weight
        self.token_list = token_list.copy()
        self.frontend = frontend
        self.specaug = None
        self.normalize = normalize
        self.preencoder = None
        self.postencoder = None
        self.encoder = encoder
        self._len_cache = {}
        # espnet_model.py:167-192
        self.use_transducer_decoder = joint_network is not None
        if self.use_transducer_decoder:  # (the transducer branch of the reference: blank is label 0, the CTC head optional)
            self.blank_id = 0
            self.decoder = decoder
            self.joint_network = joint_network
            decoder.set_joint_network(joint_network)
        else:
            self.decoder = decoder if ctc_weight < 1.0 else None
            self.joint_network = None
        self.ctc = None if ctc_weight == 0.0 else ctc
        # the fused encoder path can take the CTC head's arg-max inside its last kernel (csrc/block.hip EM_BLOCK_CTC);
        # a plain attribute, not a submodule: the head's parameters stay under `ctc.` only
        if self.ctc is not None and hasattr(self.encoder, "_pack_fused_ctc"):
            object.__setattr__(self.encoder, "fused_ctc", self.ctc)

    # ------------------------------------------------------------------ packing
    def set_compute_dtype(self, dtype: str):
        """'float32' (exact-f32 MFMA parity mode) or 'bfloat16' (bf16 MFMA, f32 accumulate)."""
        for m in (self.encoder, self.ctc, self.decoder, self.joint_network):
            if m is not None and hasattr(m, "compute_dtype"):
                m.compute_dtype = dtype
                m.invalidate()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        for m in (self.frontend, self.encoder, self.ctc, self.decoder, self.joint_network):
            if m is not None and hasattr(m, "invalidate"):
                m.invalidate()
        return r

    # ------------------------------------------------------------------ encode
    def encode_device(self, speech: torch.Tensor, speech_lengths: List[int],
                      isolate: bool = False) -> EncoderState:
        """speech (B, N) f32 ON THE GPU (zero padded), speech_lengths host ints.  No host sync.
        isolate=False: the reference's padded-batch semantics (`encode`, espnet_model.py:380-448: STFT
        reflect padding at the padded end, unmasked depthwise conv).  isolate=True: batching is
        transparent — row b equals what `Speech2Text.__call__` computes for utterance b alone."""
        L.require_gpu(speech, "speech")
        nmax = max(int(n) for n in speech_lengths)
        speech = speech[:, :nmax].contiguous()  # espnet_model.py:454 (crop to the longest)
        dev = speech.device
        flens = self.frontend.feature_lengths(speech_lengths)
        # length vectors live on the device; the last few distinct ones are kept so a repeating batch
        # shape costs no H2D copy (and a captured hipGraph of the pass keeps valid pointers)
        ckey = (tuple(int(n) for n in speech_lengths), bool(isolate), dev)
        cached = self._len_cache.get(ckey)
        if cached is None:
            flens_dev = torch.tensor(flens, dtype=torch.int32).to(dev, non_blocking=True)
            wlens_dev = None
            if isolate and len(set(ckey[0])) > 1:
                if min(ckey[0]) <= self.frontend.n_fft // 2:
                    raise ValueError(f"an input of {min(ckey[0])} samples is too short for reflect padding "
                                     f"of {self.frontend.n_fft // 2}")  # torch.stft raises for it as well
                wlens_dev = torch.tensor(ckey[0], dtype=torch.int32).to(dev, non_blocking=True)
            if len(self._len_cache) >= 8:
                self._len_cache.pop(next(iter(self._len_cache)))
            self._len_cache[ckey] = (flens_dev, wlens_dev)
        else:
            flens_dev, wlens_dev = cached
        feats = self.frontend.forward_device(speech, flens_dev, wlens_dev)
        partial = None
        if self.normalize is not None:
            if hasattr(self.normalize, "partial_sums"):  # UtteranceMVN: subtraction fused into conv1
                partial = self.normalize.partial_sums(feats, flens_dev)
            else:  # GlobalMVN: in place
                feats = self.normalize.forward_device(feats, flens_dev)
        enc_out, enc_act, olens, olens_dev = self.encoder.forward_device(feats, flens, flens_dev, partial,
                                                                         isolate=isolate)
        return EncoderState(enc_out, enc_act, olens, olens_dev, feats, flens,
                            getattr(self.encoder, "last_ctc_ids", None))

    def encode(self, speech: torch.Tensor, speech_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Frontend + Encoder (espnet_model.py:380-448).  speech (B, N), speech_lengths (B,)."""
        assert speech_lengths.dim() == 1, speech_lengths.shape
        st = self.encode_device(speech.to(torch.float32), [int(v) for v in speech_lengths.tolist()])
        self._last_state = st
        return st.enc_out, torch.tensor(st.olens, dtype=torch.long, device=speech.device)

    def _extract_feats(self, speech: torch.Tensor, speech_lengths: torch.Tensor):
        """espnet_model.py:450-467."""
        speech = speech[:, : int(speech_lengths.max())]
        return self.frontend(speech, speech_lengths)

    # ------------------------------------------------------------------ attention-decoder likelihood of a transcript
    def _nll_rows(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of=None, checked=False) -> torch.Tensor:
        """(B,) f32: transcript b under the attention decoder given memory mem_of[b] (None: memory b).  `checked`: the
        caller vouches for HOST ys_pad (ids in the vocabulary), lengths in [1, T] and mem_of, so nothing is verified on
        the device and no verdict is read back - the call only enqueues."""
        if self.use_transducer_decoder:
            raise RuntimeError("nll: this is a transducer model (joint network); the teacher-forced attention likelihood "
                               "needs an attention decoder (the transducer's own likelihood: transducer_nll)")
        if self.decoder is None:
            raise RuntimeError("nll: the model has no attention decoder (ctc_weight == 1.0)")
        if not hasattr(self.decoder, "sequence_nll"):
            raise RuntimeError(f"nll: {type(self.decoder).__name__} has no whole-sequence scoring path")
        x, keymask, target = build_dec_nll_batch(ys_pad, ys_pad_lens, self.sos, self.eos, self.vocab_size)
        if checked:
            dev = encoder_out.device
            kl, xi, ki, ti, mo = (None if v is None else v.to(torch.int32).contiguous().to(dev, non_blocking=True)
                                  for v in (encoder_out_lens, x, keymask, target, mem_of))
            return self.decoder._sequence_nll(encoder_out.contiguous(), kl, xi, ki, ti, mo).sum(dim=1)
        return self.decoder.sequence_nll(encoder_out, encoder_out_lens, x, keymask, target, mem_of=mem_of).sum(dim=1)

    @torch.no_grad()
    def nll(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, ys_pad: torch.Tensor,
            ys_pad_lens: torch.Tensor) -> torch.Tensor:
        """espnet_model.py `nll`: the decoder's teacher-forced negative log-likelihood of every transcript given its
        encoder output, (B,) f32.  encoder_out (B, T, d) on the GPU, encoder_out_lens (B,), ys_pad (B, Lmax) token ids,
        ys_pad_lens (B,).  ys_in = [sos | y], ys_out = [y | eos], ys_in_lens = ys_pad_lens + 1; the memory is masked by
        encoder_out_lens; the per-token cross-entropy is summed over the ys_pad_lens + 1 scored positions.  One enqueue for
        the whole batch (TransformerDecoder.sequence_nll); the (B, L, V) scores of `decoder.forward` never exist."""
        return self._nll_rows(encoder_out, encoder_out_lens, ys_pad, ys_pad_lens)

    @torch.no_grad()
    def batchify_nll(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, ys_pad: torch.Tensor,
                     ys_pad_lens: torch.Tensor, batch_size: int = 100) -> torch.Tensor:
        """espnet_model.py `batchify_nll`: `nll` in slices of batch_size utterances, concatenated."""
        return self._in_slices(self.nll, batch_size, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens)

    @staticmethod
    def _in_slices(score, batch_size: int, encoder_out: torch.Tensor, *per_utt) -> torch.Tensor:
        """score(encoder_out, *per_utt) over slices of batch_size utterances, concatenated."""
        total_num = encoder_out.size(0)
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if total_num <= batch_size:
            return score(encoder_out, *per_utt)
        per_utt = [torch.as_tensor(v) for v in per_utt]
        return torch.cat([score(encoder_out[s : s + batch_size], *(v[s : s + batch_size] for v in per_utt))
                          for s in range(0, total_num, batch_size)])

    # ------------------------------------------------------------------ transducer likelihood of a transcript
    @torch.no_grad()
    def transducer_nll(self, encoder_out: torch.Tensor, encoder_out_lens, ys_pad, ys_pad_lens,
                       mem_of=None, enc_proj=None) -> torch.Tensor:
        """-log p(y | x) of every transcript under the transducer, the forward value of the RNN-T loss
        (espnet_model.py `_calc_transducer_loss`), (N,) f32 on the device.  encoder_out (Bm, T, d) on the GPU,
        encoder_out_lens (Bm,), ys_pad (N, Lmax) token ids, ys_pad_lens (N,); mem_of (N,) names the utterance of every
        transcript (None: transcript n belongs to utterance n), so the candidates of an n-best list share their
        utterance's projection.  A transcript may be empty; an utterance without frames gives +inf.  Token ids outside
        [0, vocab_size) or equal to blank inside a transcript raise ValueError on the host.  Everything is enqueued: the
        teacher-forced prediction network (`TransducerDecoder.teacher_forced_proj`), `em_transducer_lattice_logp` and
        `em_transducer_seq_nll`; the (N, T, U, V) joint output never exists.  A batch whose lattice is outside the
        shapes of one call goes through in slices of candidates.  `enc_proj`: `joint_network.enc_proj_device(encoder_out)`
        when the caller holds it already (several calls on one batch of utterances)."""
        parts = self._transducer_lattice_parts(
            "transducer_nll", "the attention decoder's likelihood is `nll`",
            lambda jn, lat, xl, yl, mem: jn.seq_nll_device(lat, xl, yl, mem),
            encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of, enc_proj)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def _check_transducer_candidates(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of):
        """The host checks of a batch of candidate transcripts: host tensors (ys cut to the longest length, ylens, xlens,
        mem_of or None) and the longest length, or ValueError."""
        ys = torch.as_tensor(ys_pad).detach().to("cpu", torch.long)
        ylens = torch.as_tensor(ys_pad_lens).detach().to("cpu", torch.long)
        xlens = torch.as_tensor(encoder_out_lens).detach().to("cpu", torch.long)
        if ys.dim() != 2 or ylens.dim() != 1 or ys.size(0) != ylens.size(0) or ys.size(0) == 0:
            raise ValueError(f"ys_pad (N, L) and ys_pad_lens (N,) expected, got {tuple(ys.shape)}, {tuple(ylens.shape)}")
        N, Bm, T = int(ys.size(0)), int(encoder_out.shape[0]), int(encoder_out.shape[1])
        if xlens.dim() != 1 or xlens.numel() != Bm or int(xlens.min()) < 0 or int(xlens.max()) > T:
            raise ValueError(f"encoder_out_lens must hold {Bm} lengths in [0, {T}]")
        longest, shortest = int(ylens.max()), int(ylens.min())
        if shortest < 0 or longest > ys.size(1):
            raise ValueError(f"ys_pad_lens must lie in [0, {ys.size(1)}], got {shortest} .. {longest}")
        ys = ys[:, :longest]
        inside = torch.arange(longest).unsqueeze(0) < ylens.unsqueeze(1)
        if bool((((ys < 0) | (ys >= self.vocab_size)) & inside).any()):
            raise ValueError(f"token ids must lie in [0, {self.vocab_size})")
        if bool(((ys == self.blank_id) & inside).any()):
            raise ValueError(f"token id {self.blank_id} (<blank>) cannot be part of a transcript")
        if mem_of is None:
            if N > Bm:
                raise ValueError(f"{N} transcripts for {Bm} utterances need mem_of")
            mo = None
        else:
            mo = torch.as_tensor(mem_of).detach().to("cpu", torch.long)
            if mo.dim() != 1 or mo.numel() != N or int(mo.min()) < 0 or int(mo.max()) >= Bm:
                raise ValueError(f"mem_of must hold {N} utterance numbers in [0, {Bm})")
        return ys, ylens, xlens, mo, longest

    def _transducer_lattice_parts(self, what, other_route, score, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens,
                                  mem_of, enc_proj, checked=False) -> list:
        """What `transducer_nll` and `transducer_align` share: the host checks of the candidates (every ValueError before
        anything is launched), the slicing over candidates when the lattice is outside the shapes of one call, and per
        slice the chain `teacher_forced_proj` -> `lattice_logp_device` -> score(joint_network, lat, xlens, ylens, mem_of),
        all on the device.  Returns the slices' results in order.  `what` names the caller in the messages.  `checked`:
        the caller vouches for the lengths and for ys_pad (ids of the vocabulary, no blank inside a transcript; all its
        columns become lattice columns) - they may then live on the device, as the greedy walk leaves them, and nothing
        is read back."""
        if not self.use_transducer_decoder:
            raise RuntimeError(f"{what}: the model has no joint network (decoder: transducer); {other_route}")
        if checked:
            ys, ylens, xlens, mo = ys_pad, ys_pad_lens, encoder_out_lens, mem_of
            N, T, longest = int(ys.shape[0]), int(encoder_out.shape[1]), int(ys.shape[1])
        else:
            ys, ylens, xlens, mo, longest = self._check_transducer_candidates(encoder_out, encoder_out_lens, ys_pad,
                                                                              ys_pad_lens, mem_of)
            N, T = int(ys.size(0)), int(encoder_out.shape[1])
        L.require_gpu(encoder_out, "encoder_out")
        dev, dec, jn = encoder_out.device, self.decoder, self.joint_network
        cap = int(L.load().em_transducer_seq_nll_max_tokens())
        if longest > cap:
            raise NotImplementedError(f"{what}: a transcript of {longest} tokens, the recursion takes up to {cap}")
        rows = N
        while rows > 1 and jn.lattice_workspace_bytes(dec, dev, rows, T, longest) == 0:
            rows = (rows + 1) // 2
        if jn.lattice_workspace_bytes(dec, dev, rows, T, longest) == 0:
            raise NotImplementedError(f"{what}: the lattice of one candidate, {T} frames x {longest} tokens, is "
                                      "outside the shapes of one call")
        if enc_proj is None:
            enc_proj = jn.enc_proj_device(encoder_out)
        xl = xlens.to(torch.int32).to(dev, non_blocking=True)
        parts = []
        for s in range(0, N, rows):
            e = min(s + rows, N)
            if mo is None and rows < N:  # (a slice of candidates that own their utterances: name them)
                mem = torch.arange(s, e, dtype=torch.int32).to(dev, non_blocking=True)
            else:
                mem = None if mo is None else mo[s:e].to(torch.int32).to(dev, non_blocking=True)
            yl = ylens[s:e].to(torch.int32).to(dev, non_blocking=True)
            tg = ys[s:e].to(torch.int32).contiguous().to(dev, non_blocking=True)
            dec_proj = dec.teacher_forced_proj(tg, yl, device=dev)
            lat = jn.lattice_logp_device(dec, enc_proj, xl, dec_proj, tg, yl, mem)
            parts.append(score(jn, lat, xl, yl, mem))
        return parts

    @torch.no_grad()
    def transducer_align(self, encoder_out: torch.Tensor, encoder_out_lens, ys_pad, ys_pad_lens,
                         mem_of=None, enc_proj=None):
        """WHEN the transducer emits each token of given transcripts: the best (Viterbi) path of every transcript through
        its lattice, `em_transducer_seq_align` - the max-product twin of `transducer_nll`, which sums over all paths.
        Arguments, host checks (every ValueError before anything is launched), the chain on the device
        (`TransducerDecoder.teacher_forced_proj`, `em_transducer_lattice_logp`, then the alignment launch) and the slicing
        over candidates are `transducer_nll`'s.  Returns device tensors, everything only enqueued:
          tok_frame (N, L) int32  the encoder frame at which token u is emitted, -1 behind the transcript (L: the longest
                                  transcript's length);
          tok_logp  (N, L) f32    the token's log-probability at that lattice node, 0 behind the transcript;
          frame_u   (N, T) int32  the number of tokens emitted when the path leaves frame t, -1 behind the utterance;
          total     (N,)   f32    the path's log-probability (<= -transducer_nll), -inf for an utterance without frames."""
        return self._transducer_align_rows(encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of, enc_proj)

    def _transducer_align_rows(self, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of=None, enc_proj=None,
                               checked=False):
        """`transducer_align`; `checked`: lengths and transcripts are the caller's own (`_transducer_lattice_parts`), on the
        device or the host, and nothing is verified or read back."""
        parts = self._transducer_lattice_parts(
            "transducer_align", "CTC forced alignment is `ctc.forced_align_device`",
            lambda jn, lat, xl, yl, mem: jn.seq_align_device(lat, xl, yl, mem),
            encoder_out, encoder_out_lens, ys_pad, ys_pad_lens, mem_of, enc_proj, checked=checked)
        return parts[0] if len(parts) == 1 else tuple(torch.cat(cols) for cols in zip(*parts))

    @torch.no_grad()
    def batchify_transducer_nll(self, encoder_out: torch.Tensor, encoder_out_lens, ys_pad, ys_pad_lens,
                                batch_size: int = 100) -> torch.Tensor:
        """`transducer_nll` in slices of batch_size utterances, concatenated (the shape of `batchify_nll`)."""
        return self._in_slices(self.transducer_nll, batch_size, encoder_out, encoder_out_lens, ys_pad, ys_pad_lens)

    # ------------------------------------------------------------------ greedy CTC (G1)
    def greedy_ctc_device(self, st: EncoderState, out=None):
        """argmax + groupby + drop blank/sos/eos (bin/asr_inference.py:574-575) for the whole batch
        on the device.  Returns (ids, tokens, token_lens) device tensors (int32); `out` = (tokens, token_lens)
        tensors to write into instead of fresh ones (the collation's record slot)."""
        if self.ctc is None:
            raise RuntimeError("model has no CTC head (ctc_weight == 0)")
        sos_eos = self.sos if self.sos == self.eos else -2
        if st.ctc_ids is not None:  # arg-max already taken inside the encoder's last kernel
            return self.ctc.collapse_device(st.ctc_ids, st.olens_dev, self.blank_id, sos_eos, out=out)
        return self.ctc.greedy_device(st.enc_act, st.olens_dev, self.blank_id, sos_eos, out=out)
