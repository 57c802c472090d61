"""TransformerLM as a beam-search scorer on the MI355X.

Mirrors espnet2/lm/transformer_lm.py:12-137 (constructor keywords, state-dict keys `embed`,
`encoder.embed.{0,1}`, `encoder.encoders.N.{self_attn,feed_forward,norm1,norm2}`,
`encoder.after_norm`, `decoder`) and espnet2/lm/espnet_model.py:13-22 (`ESPnetLanguageModel` with
`.lm`).  Inside the fused device search the LM step runs in csrc/search.hip `lm_step` over the same
token-tree K/V cache mechanism as the attention decoder; `batch_score` / `score` / `select_state` are the
reference's per-step scorer interface on the same code (`em_lm_step`).  The torch.nn layers are parameter
containers only.
"""
import ctypes as C
from typing import Optional

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table
from espnet_amd.asr.encoder.conformer_encoder import LayerNorm, _PositionwiseFeedForward
from espnet_amd.nets.scorer_interface import BatchScorerInterface
from espnet_amd.packing import PackedModule


class _MultiHeadedAttention(torch.nn.Module):
    def __init__(self, n_feat):
        super().__init__()
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)


class _EncoderLayer(torch.nn.Module):
    """Parameters of transformer/encoder_layer.py:17-63."""

    def __init__(self, size, ff):
        super().__init__()
        self.self_attn = _MultiHeadedAttention(size)
        self.feed_forward = _PositionwiseFeedForward(size, ff)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)


class _Encoder(torch.nn.Module):
    """Parameters of transformer/encoder.py Encoder(input_layer="linear") (:132-139, :200-330)."""

    def __init__(self, idim, d, ff, layers):
        super().__init__()
        # Linear, LayerNorm(eps 1e-5), Dropout, ReLU, pos-enc: indices 0 and 1 carry parameters
        self.embed = torch.nn.Sequential(torch.nn.Linear(idim, d), torch.nn.LayerNorm(d),
                                         torch.nn.Identity(), torch.nn.ReLU(), torch.nn.Identity())
        self.encoders = torch.nn.ModuleList([_EncoderLayer(d, ff) for _ in range(layers)])
        self.after_norm = LayerNorm(d)


class TransformerLM(PackedModule, BatchScorerInterface):
    pe_min = 1024  # rows of the positional table a pack carries at least (more when a search needs them)

    def __init__(self, vocab_size: int, pos_enc: Optional[str] = None, embed_unit: int = 128,
                 att_unit: int = 256, head: int = 2, unit: int = 1024, layer: int = 4,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 attention_dropout_rate: float = 0.1, compute_dtype: str = "bfloat16"):
        super().__init__()
        if pos_enc not in (None, "sinusoidal"):
            raise ValueError(f"unknown pos-enc option: {pos_enc}")
        if att_unit % 64 or att_unit // head not in (32, 64) or unit % 64:
            raise NotImplementedError("MI355X TransformerLM fast path: att_unit % 64 == 0, d_k in {32, 64}, unit % 64 == 0")
        self.vocab_size, self.pos_enc = vocab_size, pos_enc
        self.embed_unit, self.att_unit, self.head, self.unit, self.layer = embed_unit, att_unit, head, unit, layer
        self.compute_dtype = compute_dtype
        self.embed = torch.nn.Embedding(vocab_size, embed_unit)
        self.encoder = _Encoder(embed_unit, att_unit, unit, layer)
        self.decoder = torch.nn.Linear(att_unit, vocab_size)

    @property
    def em_dtype(self) -> int:
        return L.DTYPES[self.compute_dtype]

    def search_key(self):
        return ("transformer", self.att_unit, self.unit, self.layer, self.embed_unit)

    def search_buffers(self, n, V, Lmax, B, cap):
        """name -> shape of the EmSearchBuffers entries this scorer needs (nets/batch_beam_search.py)."""
        dl = self.att_unit
        return dict(lm_e=(n, self.embed_unit), lm_xn=(n, dl), lm_qkv=(n, 3 * dl), lm_ctx=(n, dl), lm_h=(n, self.unit),
                    lm_x=(n, dl), lm_logp=(n, V), lm_k=(self.layer, Lmax, n, dl), lm_v=(self.layer, Lmax, n, dl),
                    run_slm=(n,), end_slm=(B, cap))

    def _build_pack(self, pk):
        A, F = pk.A, pk.F
        kmult = 64 if self.em_dtype == L.EM_BF16 else 32
        if self.embed_unit % kmult:
            raise NotImplementedError(f"embed_unit must be a multiple of {kmult} in {self.compute_dtype} mode")
        w = L.EmLmWeights()
        w.d, w.heads, w.ff, w.num_blocks = self.att_unit, self.head, self.unit, self.layer
        w.vocab, w.embed_unit = self.vocab_size, self.embed_unit
        e = self.encoder
        top = dict(embed=F(self.embed.weight), in_w=A(e.embed[0].weight), in_b=F(e.embed[0].bias),
                   in_ln_g=F(e.embed[1].weight), in_ln_b=F(e.embed[1].bias),
                   after_norm_g=F(e.after_norm.weight), after_norm_b=F(e.after_norm.bias),
                   out_w=A(self.decoder.weight), out_b=F(self.decoder.bias))
        if self.pos_enc == "sinusoidal":
            top["pe"] = F(abs_pos_table(pk.pe_len, self.att_unit))
        pk.fill(w, top)
        layers = (L.EmLmLayer * self.layer)()
        for i, l in enumerate(e.encoders):
            sa, ff = l.self_attn, l.feed_forward
            lt = dict(norm1_g=F(l.norm1.weight), norm1_b=F(l.norm1.bias), norm2_g=F(l.norm2.weight),
                      norm2_b=F(l.norm2.bias),
                      wqkv=A(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)),
                      bqkv=F(torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0)),
                      wout=A(sa.linear_out.weight), bout=F(sa.linear_out.bias),
                      w1=A(ff.w_1.weight), b1=F(ff.w_1.bias), w2=A(ff.w_2.weight), b2=F(ff.w_2.bias))
            pk.fill(layers[i], lt)
        w.layers = C.cast(layers, C.POINTER(L.EmLmLayer))
        pk.w, pk.layers = w, layers

    # ------------------------------------------------------------------ scorer interface (one call per step)
    @torch.no_grad()
    def batch_score(self, ys: torch.Tensor, states, xs: torch.Tensor):
        """transformer_lm.py:103-137.  ys (n, L) int64 prefixes; states list[n] of None or this class's opaque
        cache (self-attention K/V of the prefix, (2, layers, L-1, att_unit) in the compute dtype); xs is only
        used for its device.  Returns (log-probs (n, V) f32, states list[n])."""
        from espnet_amd.lm.step import lm_step

        L.require_gpu(xs, "xs")
        dev = xs.device
        n, Lc = ys.shape
        pos, Lmax = Lc - 1, Lc + 1
        act = self.act_dtype
        kv = torch.zeros(2, self.layer, Lmax, n, self.att_unit, dtype=act, device=dev)
        if pos > 0:
            if states is None or any(s is None for s in states):
                raise ValueError("batch_score: a prefix longer than <sos> needs the state of its previous step")
            kv[:, :, :pos] = torch.stack(list(states), 0).permute(1, 2, 3, 0, 4)
        tok = torch.zeros(Lmax, n, dtype=torch.int32, device=dev)
        tok[:Lc] = ys.t().to(device=dev, dtype=torch.int32)
        logp, _ = lm_step(self, dev, n, Lmax, pos, tok, dict(lm_k=kv[0], lm_v=kv[1]))
        out = kv[:, :, :Lc].permute(3, 0, 1, 2, 4)
        return logp, [out[r] for r in range(n)]

    @torch.no_grad()
    def forward(self, input: torch.Tensor, hidden=None):
        """transformer_lm.py:59-75 (AbsLM.forward): input (B, L) int64 -> (logits (B, L, V) f32, None).  Causal
        self-attention makes position j depend on tokens <= j only, so the sequence is fed position by position
        through the step kernels over one K/V cache (inference-only class: no autograd)."""
        from espnet_amd.lm.step import lm_step

        L.require_gpu(input, "input")
        dev = input.device
        n, Lc = input.shape
        act = self.act_dtype
        kv = torch.zeros(2, self.layer, Lc + 1, n, self.att_unit, dtype=act, device=dev)
        tok = torch.zeros(Lc + 1, n, dtype=torch.int32, device=dev)
        tok[:Lc] = input.t().to(torch.int32)
        out = torch.empty(n, Lc, self.vocab_size, dtype=torch.float32, device=dev)
        for pos in range(Lc):
            out[:, pos] = lm_step(self, dev, n, Lc + 1, pos, tok, dict(lm_k=kv[0], lm_v=kv[1]), log_softmax=False)[0]
        return out, None

    def score(self, y: torch.Tensor, state, x: torch.Tensor):
        """transformer_lm.py:77-101: one hypothesis."""
        logp, st = self.batch_score(y.unsqueeze(0), [state], x.unsqueeze(0))
        return logp[0], st[0]

    @torch.no_grad()
    def sequence_nll(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """Per-token negative log-likelihoods of whole sentences in one enqueue (`em_lm_seq_nll`, csrc/lm_seq.hip; its
        head: csrc/vocab_head.hip): x (B, Lp) integer input tokens with 0 behind a sentence's end, target (B, Lp) the token
        scored at every position, negative where nothing is scored -> nll (B, Lp) f32, exactly 0.0 there.  What `forward`
        + cross-entropy compute position by position, over all B * Lp rows at once."""
        L.require_gpu(x, "x")
        L.require_gpu(target, "target")
        if x.dim() != 2 or x.shape != target.shape or x.numel() == 0:
            raise ValueError(f"sequence_nll: x and target must be equal, non-empty (B, Lp) tensors, got {tuple(x.shape)} "
                             f"and {tuple(target.shape)}")
        xi = x.to(torch.int32).contiguous()
        ti = target.to(torch.int32).contiguous()
        if bool(((xi < 0) | (xi >= self.vocab_size)).any() | (ti >= self.vocab_size).any()):
            raise ValueError(f"sequence_nll: token ids must lie in [0, {self.vocab_size})")
        return self._sequence_nll(xi, ti)

    def _sequence_nll(self, xi: torch.Tensor, ti: torch.Tensor) -> torch.Tensor:
        """`sequence_nll` behind its checks: contiguous int32 (B, Lp) device tensors taken as given (the caller has
        checked their values).  Only enqueues."""
        dev = xi.device
        B, Lp = xi.shape
        pk = self.packed(dev, Lp + 1)
        lib = L.load()
        need = lib.em_lm_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
        if need == 0:
            raise NotImplementedError(f"sequence_nll: a batch of {B} x {Lp} tokens is outside the device path's index "
                                      "range; score it in slices (ESPnetLanguageModel.batchify_nll)")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        nll = torch.empty(B, Lp, dtype=torch.float32, device=dev)
        L.check(lib.em_lm_seq_nll(pk.dtype, C.byref(pk.w), L.ptr(xi), L.ptr(ti), B, Lp, L.ptr(nll), L.ptr(ws), need,
                                  L.current_stream_ptr()), "em_lm_seq_nll")
        return nll


def build_nll_batch(text: torch.Tensor, text_lengths: torch.Tensor, sos: int, eos: int, ignore_id: int = 0,
                    max_length: Optional[int] = None):
    """The sentence pair of ESPnetLanguageModel.nll (espnet2/lm/espnet_model.py:38-66), plain tensor work on whatever
    device `text` lives on: text (B, Lt) is cut to its longest sentence (or to `max_length` columns), then
    x = [sos | text], t = [text | ignore_id] with t[i, text_lengths[i]] = eos, x_lengths = text_lengths + 1.
    Returns (x (B, L + 1), t (B, L + 1), x_lengths (B,)).  A sentence longer than `max_length` raises ValueError (the
    reference would write its eos out of range)."""
    if text.dim() != 2 or text_lengths.dim() != 1 or text.size(0) != text_lengths.size(0):
        raise ValueError(f"text (B, L) and text_lengths (B,) expected, got {tuple(text.shape)}, {tuple(text_lengths.shape)}")
    longest = int(text_lengths.max())
    width = longest if max_length is None else int(max_length)
    if longest > width or longest > text.size(1):
        raise ValueError(f"text_lengths up to {longest} exceed the {min(width, text.size(1))} columns of text that are scored")
    text = text[:, :width]
    x = torch.nn.functional.pad(text, [1, 0], "constant", sos)
    t = torch.nn.functional.pad(text, [0, 1], "constant", ignore_id)
    t[torch.arange(t.size(0), device=t.device), text_lengths.to(t.device).long()] = eos
    return x, t, text_lengths + 1


class ESPnetLanguageModel(torch.nn.Module):
    """espnet2/lm/espnet_model.py:13-120: the scorer's container (`.lm`, sos / eos / ignore_id) and the reference's two
    text-scoring calls, `nll` and `batchify_nll`, on the device."""

    def __init__(self, lm: TransformerLM, vocab_size: int, ignore_id: int = 0):
        super().__init__()
        self.lm = lm
        self.sos = self.eos = vocab_size - 1
        self.ignore_id = ignore_id

    def _masked_pair(self, text, text_lengths, max_length=None):
        """`build_nll_batch` on text's device, with x zeroed behind x_lengths -> (x, t, x_lengths, scored)."""
        x, t, x_lengths = build_nll_batch(text, text_lengths, self.sos, self.eos, self.ignore_id, max_length)
        x_lengths = x_lengths.to(x.device)
        scored = torch.arange(x.size(1), device=x.device).unsqueeze(0) < x_lengths.unsqueeze(1)
        x = torch.where(scored, x, torch.zeros_like(x))  # whatever the caller padded with: nothing behind the end is a key
        return x, t, x_lengths, scored

    @torch.no_grad()
    def nll_of_checked(self, text: torch.Tensor, text_lengths: torch.Tensor, device) -> torch.Tensor:
        """`nll`'s first result for HOST text / text_lengths whose ids the caller has checked against the vocabulary:
        the sentence pair is built on the host and the TransformerLM only enqueues (no verdict is read back).  A
        recurrent LM goes through `nll`."""
        if not isinstance(self.lm, TransformerLM):
            return self.nll(text.to(device, non_blocking=True), text_lengths)[0]
        x, t, _, scored = self._masked_pair(text, text_lengths)
        t = torch.where(scored, t, torch.full_like(t, -1))
        return self.lm._sequence_nll(*(v.to(torch.int32).contiguous().to(device, non_blocking=True) for v in (x, t)))

    @torch.no_grad()
    def nll(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None):
        """espnet_model.py:38-80.  text (B, Lt) int64, text_lengths (B,) -> (nll (B, L + 1) f32, x_lengths (B,)):
        nll[i, j] = -log_softmax(lm(x)[i, j])[t[i, j]] for j < x_lengths[i], exactly 0.0 behind.  The TransformerLM scores
        all rows in one enqueue (`sequence_nll`); a recurrent LM goes position by position through its `forward`."""
        L.require_gpu(text, "text")
        x, t, x_lengths, scored = self._masked_pair(text, text_lengths, max_length)
        if isinstance(self.lm, TransformerLM):
            return self.lm.sequence_nll(x, torch.where(scored, t, torch.full_like(t, -1))), x_lengths
        logits, _ = self.lm(x, None)
        B, Lp, V = logits.shape
        rows = logits.reshape(B * Lp, V)
        L.check(L.load().em_log_softmax_rows_f32(L.ptr(rows), B * Lp, V, L.current_stream_ptr()), "em_log_softmax_rows_f32")
        nll = -rows.gather(1, t.reshape(-1, 1).long()).reshape(B, Lp)
        return torch.where(scored, nll, torch.zeros_like(nll)), x_lengths

    @torch.no_grad()
    def batchify_nll(self, text: torch.Tensor, text_lengths: torch.Tensor, batch_size: int = 100):
        """espnet_model.py:82-120: `nll` over slices of `batch_size` sentences, every slice as wide as the longest
        sentence of the whole call, so that the slices concatenate."""
        total = text.size(0)
        if total <= batch_size:
            return self.nll(text, text_lengths)
        max_length = int(text_lengths.max())
        nlls, lens = [], []
        for s in range(0, total, batch_size):
            n, xl = self.nll(text[s:s + batch_size], text_lengths[s:s + batch_size], max_length=max_length)
            nlls.append(n)
            lens.append(xl)
        return torch.cat(nlls), torch.cat(lens)
