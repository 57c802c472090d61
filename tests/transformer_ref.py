"""CPU f32 restatement of TransformerEncoder.forward (espnet2/asr/encoder/transformer_encoder.py) in eval mode with
normalize_before=True, concat_after=False, the linear position-wise FFN with ReLU and PositionalEncoding:

    x = Conv2dSubsampling(feats) * sqrt(d) + pe[:T]
    per EncoderLayer:  x = x + MHA(norm1(x));  x = x + w_2(relu(w_1(norm2(x))))
    out = after_norm(x)

composed from pieces the reference fixtures already pin (oracle.conformer: frontend, MVN, subsampling, lengths,
LayerNorm, feed-forward; oracle.beam_search.abs_pos_table) plus MultiHeadedAttention written out here."""
import math

import torch
import torch.nn.functional as F

from oracle import conformer as oc
from oracle.beam_search import abs_pos_table


def attend(q, k, v, key_valid, h):
    """MultiHeadedAttention.forward_attention on projected q (B, Tq, d), k / v (B, Tk, d): softmax(q k^T / sqrt(d_k))
    over the keys with key_valid (B, Tk) True; masked scores filled with the dtype's minimum before the softmax and the
    probabilities with 0 after it, as the reference does.  key_valid None: no mask."""
    B, Tq, d = q.shape
    dk = d // h
    qh = q.view(B, Tq, h, dk).transpose(1, 2)
    kh = k.view(B, -1, h, dk).transpose(1, 2)
    vh = v.view(B, -1, h, dk).transpose(1, 2)
    scores = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(dk)
    if key_valid is not None:
        mask = ~key_valid[:, None, None, :]
        scores = scores.masked_fill(mask, torch.finfo(scores.dtype).min)
        attn = torch.softmax(scores, dim=-1).masked_fill(mask, 0.0)
    else:
        attn = torch.softmax(scores, dim=-1)
    return torch.matmul(attn, vh).transpose(1, 2).contiguous().view(B, Tq, d)


def mha(sd, x, key_valid, pre, h):
    """MultiHeadedAttention.forward (self-attention): linear_q / k / v, attend, linear_out."""
    def lin(name, t):
        return F.linear(t, sd[pre + name + ".weight"], sd[pre + name + ".bias"])

    return lin("linear_out", attend(lin("linear_q", x), lin("linear_k", x), lin("linear_v", x), key_valid, h))


def transformer_encoder(sd, feats, flens, heads, num_blocks):
    """TransformerEncoder.forward over (B, T_f, D) features -> (out (B, T, d), olens)."""
    kind = oc.subsampling_kind(sd)
    lim = oc.SHORT_LIMIT[kind]
    if feats.size(1) < lim:
        raise oc.TooShortUttError(f"has {feats.size(1)} frames and is too short for subsampling "
                                  f"(it needs more than {lim} frames), return empty results", feats.size(1), lim)
    x = oc.conv2d_subsampling(sd, feats)
    T, d = x.size(1), x.size(2)
    x = x * math.sqrt(d) + abs_pos_table(T, d)[None]  # PositionalEncoding.forward (dropout: eval)
    olens = oc.subsampled_lengths(flens, feats.size(1), kind)
    key_valid = ~oc.make_pad_mask(olens, T)
    for i in range(num_blocks):
        pre = f"encoder.encoders.{i}."
        x = x + mha(sd, oc.layer_norm(x, sd, pre + "norm1."), key_valid, pre + "self_attn.", heads)
        x = x + oc.feed_forward(sd, oc.layer_norm(x, sd, pre + "norm2."), pre + "feed_forward.", act=torch.relu)
    return oc.layer_norm(x, sd, "encoder.after_norm."), olens


def encode(sd, speech, speech_lengths, heads, num_blocks, n_fft=512, win_length=None, hop=160):
    """ESPnetASRModel.encode with DefaultFrontend + UtteranceMVN + TransformerEncoder."""
    feats, flens = oc.frontend_feats(speech, speech_lengths, sd["frontend.logmel.melmat"], n_fft, win_length, hop)
    feats = oc.utterance_mvn(feats, flens)
    return transformer_encoder(sd, feats, flens, heads, num_blocks)
