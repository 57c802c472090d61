"""Float64 restatement of transducer (RNN-T) decoding as include/espnet_amd.h ("transducer") states it: the prediction
network's step (espnet2/asr/decoder/transducer_decoder.py TransducerDecoder.score), the joint network
(espnet2/asr_transducer/joint_network.py JointNetwork.forward), and the greedy and default beam searches of
espnet2/asr/transducer/beam_search_transducer.py.  Plain torch / numpy on the CPU; nothing of espnet_amd is imported.

Parameters are a model state dict's entries under `decoder.` and `joint_network.` (reference keys), taken as float64.
A decoder state is a list over layers of (h, c) for the LSTM or (h,) for the GRU, each a float64 vector (H,).
"""
import numpy as np
import torch


class Params:
    def __init__(self, state_dict, rnn_type="lstm", blank=0, round_to=None):
        """round_to: torch.bfloat16 to restate on the weights as the device's bf16 mode holds them (the same inputs)."""
        def get(k):
            t = state_dict[k].detach().to(torch.float32)
            if round_to is not None and t.dim() >= 2:  # matrices live in the compute dtype, vectors (biases) in f32
                t = t.to(round_to).to(torch.float32)
            return t.to(torch.float64)

        self.rnn_type, self.blank = rnn_type, blank
        self.embed = get("decoder.embed.weight")
        self.layers = []
        l = 0
        while f"decoder.decoder.{l}.weight_ih_l0" in state_dict:
            self.layers.append(tuple(get(f"decoder.decoder.{l}.{k}_l0") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            l += 1
        self.enc_w, self.enc_b = get("joint_network.lin_enc.weight"), get("joint_network.lin_enc.bias")
        self.dec_w = get("joint_network.lin_dec.weight")
        self.out_w, self.out_b = get("joint_network.lin_out.weight"), get("joint_network.lin_out.bias")
        self.H, self.V = self.embed.shape[1], self.embed.shape[0]

    def init_state(self):
        z = torch.zeros(self.H, dtype=torch.float64)
        return [(z, z) if self.rnn_type == "lstm" else (z,) for _ in self.layers]


def dec_step(p: Params, label: int, state):
    """One step: embed `label`, run the layers from `state`.  Returns (dec_out (H,), new state)."""
    x = p.embed[label]
    new = []
    for (w_ih, w_hh, b_ih, b_hh), st in zip(p.layers, state):
        h = st[0]
        H = h.numel()
        gi, gh = w_ih @ x + b_ih, w_hh @ h + b_hh
        if p.rnn_type == "lstm":  # torch.nn.LSTM: i | f | g | o
            g = gi + gh
            i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H : 2 * H]), torch.tanh(g[2 * H : 3 * H]), torch.sigmoid(g[3 * H :])
            c = f * st[1] + i * gg
            h = o * torch.tanh(c)
            new.append((h, c))
        else:  # torch.nn.GRU: r | z | n
            r, z = torch.sigmoid(gi[:H] + gh[:H]), torch.sigmoid(gi[H : 2 * H] + gh[H : 2 * H])
            n = torch.tanh(gi[2 * H :] + r * gh[2 * H :])
            h = (1 - z) * n + z * h
            new.append((h,))
        x = h
    return x, new


def joint_logits(p: Params, enc, dec_out):
    """lin_out(tanh(lin_enc(enc) + lin_dec(dec))): enc (D,), dec_out (H,) -> logits (V,)."""
    return p.out_w @ torch.tanh(p.enc_w @ enc + p.enc_b + p.dec_w @ dec_out) + p.out_b


def log_softmax(x):
    return x - torch.logsumexp(x, 0)


def top2(x):
    """(arg-max with the lowest id on ties, top-1 minus top-2 value)."""
    x = x.numpy()
    i = int(np.argmax(x))  # (numpy: the first of equal maxima)
    rest = np.delete(x, i)
    return i, float(x[i] - rest.max())


def greedy(p: Params, enc_out, forced=None):
    """greedy_search: at most one label per frame.  enc_out (T, D) float64.  forced: per-frame decisions to follow
    instead of the own arg-max (teacher forcing; the trace still reports the own arg-max).  Returns a dict: yseq (with
    the leading blank), score, and per frame tok (own arg-max), top (its log-prob), margin (top-1 minus top-2 logit),
    lp_forced (the log-prob of the decision followed)."""
    state = p.init_state()
    yseq, score = [p.blank], 0.0
    dec_out, nxt = dec_step(p, p.blank, state)
    tr = dict(tok=[], top=[], margin=[], lp_forced=[])
    for t in range(enc_out.shape[0]):
        logits = joint_logits(p, enc_out[t], dec_out)
        logp = log_softmax(logits)
        own, margin = top2(logits)
        pred = own if forced is None else int(forced[t])
        tr["tok"].append(own), tr["top"].append(float(logp[own])), tr["margin"].append(margin)
        tr["lp_forced"].append(float(logp[pred]))
        if pred != p.blank:
            yseq.append(pred)
            score += float(logp[pred])
            state = nxt
            dec_out, nxt = dec_step(p, pred, state)
    return dict(yseq=yseq, score=score, **tr)


def greedy_from_logits(logits_fn, T, blank=0):
    """The walk alone on a caller's logits: logits_fn(t, yseq) -> (V,) array.  Returns (yseq, score)."""
    yseq, score = [blank], 0.0
    for t in range(T):
        logp = log_softmax(torch.as_tensor(np.asarray(logits_fn(t, tuple(yseq)), dtype=np.float64)))
        pred, _ = top2(logp)
        if pred != blank:
            yseq.append(pred)
            score += float(logp[pred])
    return yseq, score


def beam_search_from_logits(logits_fn, T, V, beam_size, nbest=1, score_norm=True, blank=0):
    """default_beam_search on a caller's logits: logits_fn(t, yseq) -> (V,).  Returns [(score, yseq)], best first."""
    beam = min(beam_size, V)
    beam_k = min(beam, V - 1)
    kept = [(0.0, [blank])]
    for t in range(T):
        hyps, kept = kept, []
        while True:
            i_max = max(range(len(hyps)), key=lambda i: hyps[i][0])
            s, y = hyps.pop(i_max)
            logp = log_softmax(torch.as_tensor(np.asarray(logits_fn(t, tuple(y)), dtype=np.float64))).numpy()
            kept.append((s + float(logp[blank]), list(y)))
            assert blank == 0
            for k in np.argsort(-logp[1:], kind="stable")[:beam_k]:  # top-k, ties to the lowest id
                hyps.append((s + float(logp[1 + k]), y + [int(k) + 1]))
            best_left = max(h[0] for h in hyps)
            most = sorted([h for h in kept if h[0] > best_left], key=lambda h: h[0])
            if len(most) >= beam:
                kept = most
                break
    key = (lambda h: h[0] / len(h[1])) if score_norm else (lambda h: h[0])
    return sorted(kept, key=key, reverse=True)[:nbest]


def model_logits_fn(p: Params, enc_out):
    """logits_fn of a model: the prediction network's output cached by label sequence (states by prefix)."""
    cache = {}

    def run(y):
        if y not in cache:
            if len(y) == 1:
                cache[y] = dec_step(p, y[-1], p.init_state())
            else:
                cache[y] = dec_step(p, y[-1], run(y[:-1])[1])
        return cache[y]

    return lambda t, y: joint_logits(p, enc_out[t], run(y)[0]).numpy()


def beam_search(p: Params, enc_out, beam_size, nbest=1, score_norm=True):
    return beam_search_from_logits(model_logits_fn(p, enc_out), enc_out.shape[0], p.V, beam_size, nbest, score_norm, p.blank)
