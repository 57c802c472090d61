"""Float64 restatement of whole-sentence scoring with the TransformerLM as include/espnet_amd.h ("language model over whole
sentences") states it: TransformerLM.forward (espnet2/lm/transformer_lm.py: nn.Embedding -> Encoder(input_layer="linear")
-> nn.Linear, `_target_mask`) over all positions at once and ESPnetLanguageModel.nll (espnet2/lm/espnet_model.py).  Plain
torch on the CPU; nothing of espnet_amd is imported.

Parameters are a state dict's entries under `prefix` (reference keys), taken as float64.  `defect` restates one of three
wrong implementations, for tests that show a check would notice them:
  "causal"  query j also sees key j + 1;   "id0"  keys with token id 0 are not masked;   "pe0"  pe[0] at every position.
"""
import math

import torch

DEFECTS = ("causal", "id0", "pe0")


def pos_table(L, d):
    """PositionalEncoding.extend_pe (transformer/embedding.py:56-79), computed in float32 as the module does."""
    pe = torch.zeros(L, d)
    position = torch.arange(0, L, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.to(torch.float64)


class Params:
    def __init__(self, state_dict, heads, pos_enc, round_to=None, prefix="lm."):
        """round_to: torch.bfloat16 to restate on the weights as the device's bf16 mode holds them (the same inputs)."""
        self.sd = {}
        for k, t in state_dict.items():
            if not k.startswith(prefix):
                continue
            t = t.detach().to(torch.float32)
            if round_to is not None and t.dim() >= 2:  # matrices live in the compute dtype, vectors (biases) in f32
                t = t.to(round_to).to(torch.float32)
            self.sd[k[len(prefix):]] = t.to(torch.float64)
        self.heads, self.pos_enc = heads, pos_enc
        self.d = self.sd["decoder.weight"].shape[1]
        self.V = self.sd["decoder.weight"].shape[0]
        self.layers = 0
        while f"encoder.encoders.{self.layers}.norm1.weight" in self.sd:
            self.layers += 1


def _ln(x, sd, pre, eps):
    return torch.nn.functional.layer_norm(x, (x.size(-1),), sd[pre + "weight"], sd[pre + "bias"], eps)


def _lin(x, sd, pre):
    return torch.nn.functional.linear(x, sd[pre + "weight"], sd[pre + "bias"])


def attention(q, k, v, x, heads, defect=None):
    """q, k, v (B, L, d) projected; x (B, L) tokens.  softmax(q k^T / sqrt(dk)) v over the keys k' <= j with x != 0, a
    masked key's probability exactly 0 (attention.py:121-151 under _target_mask); a row without a visible key gives 0."""
    B, Lp, d = q.shape
    dk = d // heads
    qh, kh, vh = (t.view(B, Lp, heads, dk).transpose(1, 2) for t in (q, k, v))
    sc = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(dk)
    j = torch.arange(Lp)
    ok = j.unsqueeze(0) <= j.unsqueeze(1) + (1 if defect == "causal" else 0)  # [query][key]
    ok = ok.unsqueeze(0).expand(B, Lp, Lp)
    if defect != "id0":
        ok = ok & (x != 0).unsqueeze(1)
    m = ~ok.unsqueeze(1)
    att = torch.softmax(sc.masked_fill(m, torch.finfo(sc.dtype).min), dim=-1).masked_fill(m, 0.0)
    return torch.matmul(att, vh).transpose(1, 2).reshape(B, Lp, d)


def forward(p: Params, x, defect=None):
    """x (B, Lp) int64 -> logits (B, Lp, V) float64."""
    sd = p.sd
    h = _lin(sd["embed.weight"][x], sd, "encoder.embed.0.")
    h = torch.relu(_ln(h, sd, "encoder.embed.1.", 1e-5))
    if p.pos_enc:
        pe = pos_table(x.size(1), p.d)
        h = h * math.sqrt(p.d) + (pe[:1] if defect == "pe0" else pe)
    for l in range(p.layers):
        pre = f"encoder.encoders.{l}."
        t = _ln(h, sd, pre + "norm1.", 1e-12)
        ctx = attention(_lin(t, sd, pre + "self_attn.linear_q."), _lin(t, sd, pre + "self_attn.linear_k."),
                        _lin(t, sd, pre + "self_attn.linear_v."), x, p.heads, defect)
        h = h + _lin(ctx, sd, pre + "self_attn.linear_out.")
        t = _ln(h, sd, pre + "norm2.", 1e-12)
        h = h + _lin(torch.relu(_lin(t, sd, pre + "feed_forward.w_1.")), sd, pre + "feed_forward.w_2.")
    return _lin(_ln(h, sd, "encoder.after_norm.", 1e-12), sd, "decoder.")


def sentence_pair(text, text_lengths, sos, eos, ignore_id=0, max_length=None):
    """espnet_model.py:45-56: x = [sos | text], t = [text | ignore_id] with eos at text_lengths, x_lengths."""
    text = text[:, : int(text_lengths.max())] if max_length is None else text[:, :max_length]
    B, L = text.shape
    x = torch.cat([torch.full((B, 1), sos, dtype=text.dtype), text], 1)
    t = torch.cat([text, torch.full((B, 1), ignore_id, dtype=text.dtype)], 1)
    for i, l in enumerate(text_lengths.tolist()):
        t[i, l] = eos
    return x, t, text_lengths + 1


def nll(p: Params, text, text_lengths, max_length=None, defect=None, ignore_id=0):
    """ESPnetLanguageModel.nll -> (nll (B, L + 1) float64, 0 behind x_lengths; x_lengths).  x is zeroed behind a
    sentence's end as the host wrapper does (by causality no scored position changes)."""
    x, t, xl = sentence_pair(text, text_lengths, p.V - 1, p.V - 1, ignore_id, max_length)
    scored = torch.arange(x.size(1)).unsqueeze(0) < xl.unsqueeze(1)
    x = torch.where(scored, x, torch.zeros_like(x))
    logp = torch.log_softmax(forward(p, x, defect), dim=-1)
    out = -logp.gather(2, t.unsqueeze(2)).squeeze(2)
    return torch.where(scored, out, torch.zeros_like(out)), xl


def rows_nll(xrows, g, b, w, bias, target):
    """em_lm_head_nll: xrows (M, d), after_norm g / b, out_w (V, d), out_b, target (M,) -> nll (M,), 0 where target < 0."""
    y = torch.nn.functional.layer_norm(xrows, (xrows.size(1),), g, b, 1e-12) @ w.t() + bias
    out = torch.logsumexp(y, 1) - y.gather(1, target.clamp(min=0).unsqueeze(1)).squeeze(1)
    return torch.where(target < 0, torch.zeros_like(out), out)
