"""Float64 restatement of whole-transcript scoring with the attention decoder as include/espnet_amd.h ("attention decoder
over whole transcripts") states it: BaseTransformerDecoder.forward (espnet2/asr/decoder/transformer_decoder.py: embedding
* sqrt(d) + pe, pre-norm DecoderLayers under tgt_mask = key padding & subsequent mask and the memory mask of hlens,
after_norm, output_layer) over all positions at once, and ESPnetASRModel.nll (espnet2/asr/espnet_model.py: add_sos_eos,
ys_in_lens = ys_pad_lens + 1, per-token cross-entropy with ignore_id).  Plain torch on the CPU; nothing of espnet_amd is
imported.

Parameters are a state dict's `decoder.*` entries (reference keys), taken as float64.  `defect` restates one of four wrong
implementations, for tests that show a check would notice them:
  "memmask"  the memory mask is ignored (every query sees all T frames);
  "causal"   query j also sees key j + 1;
  "pe0"      pe[0] at every position;
  "noscale"  the embedding is not multiplied by sqrt(d).
"""
import math

import torch

DEFECTS = ("memmask", "causal", "pe0", "noscale")
LN_EPS = 1e-12


def pos_table(L, d):
    """PositionalEncoding.extend_pe (transformer/embedding.py:56-79), computed in float32 as the module does."""
    pe = torch.zeros(L, d)
    position = torch.arange(0, L, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.to(torch.float64)


class Params:
    def __init__(self, state_dict, heads, round_to=None):
        """round_to: torch.bfloat16 to restate on the weights as the device's bf16 mode holds them (the same inputs):
        the matrices live in the compute dtype, the embedding table, the vectors and the biases in f32."""
        self.sd = {}
        for k, t in state_dict.items():
            if not k.startswith("decoder."):
                continue
            t = t.detach().to(torch.float32)
            if round_to is not None and t.dim() >= 2 and k != "decoder.embed.0.weight":
                t = t.to(round_to).to(torch.float32)
            self.sd[k] = t.to(torch.float64)
        self.heads = heads
        self.V, self.d = self.sd["decoder.output_layer.weight"].shape
        self.layers = 0
        while f"decoder.decoders.{self.layers}.norm1.weight" in self.sd:
            self.layers += 1


def _ln(x, sd, pre):
    return torch.nn.functional.layer_norm(x, (x.size(-1),), sd[pre + "weight"], sd[pre + "bias"], LN_EPS)


def _lin(x, sd, pre):
    return torch.nn.functional.linear(x, sd[pre + "weight"], sd[pre + "bias"])


def _mha(q, k, v, ok, heads):
    """q (B, Lq, d), k / v (B, Lk, d) projected, ok (B, Lq, Lk) bool: softmax(q k^T / sqrt(dk)) v over the keys with ok, a
    masked key's probability exactly 0 (attention.py:121-151); a query without a visible key gives a zero row."""
    B, Lq, d = q.shape
    dk = d // heads
    qh, kh, vh = (t.reshape(B, t.size(1), heads, dk).transpose(1, 2) for t in (q, k, v))
    sc = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(dk)
    m = ~ok.unsqueeze(1)
    att = torch.softmax(sc.masked_fill(m, torch.finfo(sc.dtype).min), dim=-1).masked_fill(m, 0.0)
    return torch.matmul(att, vh).transpose(1, 2).reshape(B, Lq, d)


def src_attention(q, k, v, klens, heads, defect=None):
    """MultiHeadedAttention of src_attn on projected operands: q (B, Lp, d), k / v (B, T, d) the memory of each sentence,
    klens (B,) its valid frames: query (b, j) attends the frames t < klens[b]."""
    B, Lp, _ = q.shape
    T = k.size(1)
    ok = torch.arange(T).unsqueeze(0) < (torch.full_like(klens, T) if defect == "memmask" else klens).unsqueeze(1)
    return _mha(q, k, v, ok.unsqueeze(1).expand(B, Lp, T), heads)


def self_attention(q, k, v, lens, heads, defect=None):
    """tgt_mask (transformer_decoder.py:124-129): query j sees the keys k <= j that lie below the sentence's length."""
    B, Lp, _ = q.shape
    j = torch.arange(Lp)
    ok = j.unsqueeze(0) <= j.unsqueeze(1) + (1 if defect == "causal" else 0)  # [query][key]
    ok = ok.unsqueeze(0) & (j.unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1)
    return _mha(q, k, v, ok, heads)


def forward(p: Params, memory, hlens, ys_in, ys_in_lens, mem_of=None, defect=None):
    """memory (Bm, T, d) float64, hlens (Bm,), ys_in (B, Lp) int64 starting with <sos>, ys_in_lens (B,); mem_of (B,) the
    memory of each sentence (None: sentence b uses memory b) -> scores before the softmax (B, Lp, V) float64."""
    sd = p.sd
    if mem_of is not None:
        memory, hlens = memory[mem_of], hlens[mem_of]
    Lp = ys_in.size(1)
    pe = pos_table(Lp, p.d)
    x = sd["decoder.embed.0.weight"][ys_in] * (1.0 if defect == "noscale" else math.sqrt(p.d))
    x = x + (pe[:1] if defect == "pe0" else pe)
    for l in range(p.layers):
        pre = f"decoder.decoders.{l}."
        t = _ln(x, sd, pre + "norm1.")
        ctx = self_attention(_lin(t, sd, pre + "self_attn.linear_q."), _lin(t, sd, pre + "self_attn.linear_k."),
                             _lin(t, sd, pre + "self_attn.linear_v."), ys_in_lens, p.heads, defect)
        x = x + _lin(ctx, sd, pre + "self_attn.linear_out.")
        t = _ln(x, sd, pre + "norm2.")
        ctx = src_attention(_lin(t, sd, pre + "src_attn.linear_q."), _lin(memory, sd, pre + "src_attn.linear_k."),
                            _lin(memory, sd, pre + "src_attn.linear_v."), hlens, p.heads, defect)
        x = x + _lin(ctx, sd, pre + "src_attn.linear_out.")
        t = _ln(x, sd, pre + "norm3.")
        x = x + _lin(torch.relu(_lin(t, sd, pre + "feed_forward.w_1.")), sd, pre + "feed_forward.w_2.")
    return _lin(_ln(x, sd, "decoder.after_norm."), sd, "decoder.output_layer.")


def sentence_pair(ys_pad, ys_pad_lens, sos, eos):
    """add_sos_eos cut to the longest transcript: ys_in = [sos | y] (<eos> behind the end), ys_out = [y | eos] (-1 = ignore
    behind it), ys_in_lens = ys_pad_lens + 1."""
    B = ys_pad.size(0)
    L = int(ys_pad_lens.max())
    ys_in = torch.full((B, L + 1), eos, dtype=torch.long)
    ys_out = torch.full((B, L + 1), -1, dtype=torch.long)
    for b, n in enumerate(ys_pad_lens.tolist()):
        ys_in[b, 0] = sos
        ys_in[b, 1 : n + 1] = ys_pad[b, :n]
        ys_out[b, :n] = ys_pad[b, :n]
        ys_out[b, n] = eos
    return ys_in, ys_out, ys_pad_lens + 1


def nll(p: Params, memory, hlens, ys_pad, ys_pad_lens, sos, eos, mem_of=None, defect=None):
    """ESPnetASRModel.nll per token -> (nll (B, L + 1) float64, exactly 0 where nothing is scored; ys_in_lens).  The
    reference's value is the sum over a row."""
    ys_in, ys_out, ys_in_lens = sentence_pair(ys_pad, ys_pad_lens, sos, eos)
    logp = torch.log_softmax(forward(p, memory, hlens, ys_in, ys_in_lens, mem_of, defect), dim=-1)
    out = -logp.gather(2, ys_out.clamp(min=0).unsqueeze(2)).squeeze(2)
    return torch.where(ys_out < 0, torch.zeros_like(out), out), ys_in_lens
