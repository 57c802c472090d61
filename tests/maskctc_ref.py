"""Float64 restatement of Mask-CTC decoding as include/espnet_amd.h ("Mask-CTC") states it: the greedy CTC pass with the
frames' winning probabilities, the collapse with confidence, the threshold, the mask-predict passes with the easiest-first
fill, and MLMDecoder.forward (a TransformerDecoder's layers with a self-attention WITHOUT the causal mask).  Written from
the contract, not from the device code; plain numpy / torch on the CPU, nothing of espnet_amd is imported.

Ties are fixed as the contract fixes them: the lowest id wins an arg-max, the lowest position wins among equal scores.

`pass_step` is the teacher-forced form: given the y_in a pass starts from it returns what the pass decides together with
the margins by which it decides, so that a caller can hold a lower-precision implementation to exactly the decisions that
are not near-ties.
"""
import math

import numpy as np
import torch

from tests.dec_seq_ref import Params, _lin, _ln, _mha, pos_table, src_attention  # noqa: F401  (Params: for the callers)


# ---------------------------------------------------------------------- steps 1-3
def ctc_frames(lp):
    """lp (T, V) float64 log-probabilities of the valid frames -> (ids (T,), p (T,)): arg-max (lowest id) and exp(max)."""
    lp = np.asarray(lp, dtype=np.float64).reshape(-1, np.shape(lp)[-1])
    ids = lp.argmax(axis=1) if len(lp) else np.zeros(0, dtype=np.int64)  # (numpy: the first, i.e. lowest, maximum)
    return ids.astype(np.int64), np.exp(lp.max(axis=1)) if len(lp) else np.zeros(0)


def collapse(ids, p, blank=0):
    """Maximal runs of equal id; every run whose id != blank is one token with the run's largest probability."""
    tokens, conf = [], []
    t, T = 0, len(ids)
    while t < T:
        u = t
        while u + 1 < T and ids[u + 1] == ids[t]:
            u += 1
        if ids[t] != blank:
            tokens.append(int(ids[t]))
            conf.append(float(max(p[t : u + 1])))
        t = u + 1
    return tokens, conf


def mask(tokens, conf, mask_token, p_thres):
    """-> (y_in, M)"""
    y_in = [mask_token if c < p_thres else t for t, c in zip(tokens, conf)]
    return y_in, sum(1 for v in y_in if v == mask_token)


def plan(M, K):
    """n_iter and n of an utterance with M masked positions (M > 0, K >= 1)."""
    n_iter = K if M >= K else M
    return n_iter, M // n_iter


# ---------------------------------------------------------------------- step 4, one pass
def pass_step(y_in, logits, mask_token, M0, K, p):
    """Pass p of an utterance that STARTS the pass with y_in (list) and whose decoder returned logits (L, V + 1) float64;
    M0: the masked positions after step 3.  Returns a dict:
      mode       "idle" | "partial" | "final";
      pos        the positions holding mask_token; s, a, margin: per such position the max logit, its arg-max and the
                 top-1 minus top-2 logit;
      taken      the positions filled in this pass (sorted);
      sel_gap    partial passes: the score gap between the last taken and the first not-taken position (inf if none is
                 left over);
      y_out      y_in after the pass."""
    y = list(y_in)
    out = dict(mode="idle", pos=[], s=[], a=[], margin=[], taken=[], sel_gap=math.inf, y_out=y)
    if M0 <= 0:
        return out
    n_iter, n = plan(M0, K)
    if p >= n_iter:
        return out
    logits = np.asarray(logits, dtype=np.float64)
    pos = [j for j, v in enumerate(y) if v == mask_token]
    s, a, mg = [], [], []
    for j in pos:
        row = logits[j]
        k = int(row.argmax())
        s.append(float(row[k]))
        a.append(k)
        mg.append(float(row[k] - np.delete(row, k).max()))
    out.update(mode="final" if p == n_iter - 1 else "partial", pos=pos, s=s, a=a, margin=mg)
    if out["mode"] == "final":
        take = list(range(len(pos)))
    else:
        order = sorted(range(len(pos)), key=lambda i: (-s[i], pos[i]))  # score descending, position ascending
        take = order[:n]
        if len(order) > n and n > 0:
            out["sel_gap"] = s[order[n - 1]] - s[order[n]]
    for i in take:
        y[pos[i]] = a[i]
    out["taken"] = sorted(pos[i] for i in take)
    return out


def decode(tokens, conf, logits_fn, mask_token, p_thres, K):
    """Steps 3-5 for one utterance: logits_fn(y_in list) -> (L, V + 1) logits of the MLM decoder.  Returns
    (yseq = [mask] + y + [mask], trace: the dict of `pass_step` per pass that ran)."""
    if K < 1:
        raise NotImplementedError("maskctc_n_iterations < 1")
    y, M = mask(tokens, conf, mask_token, p_thres)
    trace = []
    if M > 0 and len(y) > 0:
        n_iter, _ = plan(M, K)
        for p in range(n_iter):
            st = pass_step(y, logits_fn(y), mask_token, M, K, p)
            trace.append(st)
            y = st["y_out"]
    return [mask_token] + y + [mask_token], trace


def token_int(yseq):
    """Step 5: yseq[1:-1] with zeros removed."""
    return [v for v in yseq[1:-1] if v != 0]


# ---------------------------------------------------------------------- the MLM decoder
def full_attention(q, k, v, lens, heads):
    """Query (b, j) attends the keys below lens[b]: no causal mask."""
    B, Lp, _ = q.shape
    ok = (torch.arange(Lp).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1).expand(B, Lp, Lp)
    return _mha(q, k, v, ok, heads)


def mlm_forward(p, memory, hlens, ys, ylens):
    """MLMDecoder.forward: p a tests.dec_seq_ref.Params of the decoder (V + 1 rows), memory (B, T, d) float64, hlens (B,),
    ys (B, Lp) int64 (ids < 0 read row 0: the rows behind a sentence are don't-care), ylens (B,) -> (B, Lp, V + 1)."""
    sd = p.sd
    Lp = ys.size(1)
    x = sd["decoder.embed.0.weight"][ys.clamp(min=0)] * math.sqrt(p.d) + pos_table(Lp, p.d)
    for l in range(p.layers):
        pre = f"decoder.decoders.{l}."
        t = _ln(x, sd, pre + "norm1.")
        ctx = full_attention(_lin(t, sd, pre + "self_attn.linear_q."), _lin(t, sd, pre + "self_attn.linear_k."),
                             _lin(t, sd, pre + "self_attn.linear_v."), ylens, p.heads)
        x = x + _lin(ctx, sd, pre + "self_attn.linear_out.")
        t = _ln(x, sd, pre + "norm2.")
        ctx = src_attention(_lin(t, sd, pre + "src_attn.linear_q."), _lin(memory, sd, pre + "src_attn.linear_k."),
                            _lin(memory, sd, pre + "src_attn.linear_v."), hlens, p.heads)
        x = x + _lin(ctx, sd, pre + "src_attn.linear_out.")
        t = _ln(x, sd, pre + "norm3.")
        x = x + _lin(torch.relu(_lin(t, sd, pre + "feed_forward.w_1.")), sd, pre + "feed_forward.w_2.")
    return _lin(_ln(x, sd, "decoder.after_norm."), sd, "decoder.output_layer.")


def ctc_log_probs(enc, w, b):
    """CTC.log_softmax: enc (T, d), w (V, d), b (V,) float64 -> (T, V)."""
    return torch.log_softmax(enc @ w.t() + b, dim=-1)
