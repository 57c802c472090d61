"""default_beam_search restated in float64 (tests/transducer_ref.py `beam_search_from_logits`) with the margin of every
decision recorded, each divided by the number of log-probability terms in the scores it compares: a device whose
log-probabilities are within E of the restatement's takes the same decision wherever that ratio exceeds E.

    pop        the best open score against every other open score
    top-k      the k-th against the (k+1)-th log-probability of one row (two terms)
    end test   every kept score against the best open score
    final      neighbours of the n-best order (length-normalised scores: the terms are normalised alike)

Plain numpy / torch on the CPU; an expansion cap ends frames the model never leaves (the peaked model has such inputs).
"""
import numpy as np
import torch

from tests import transducer_ref as R


def terms(y, t):
    """Log-probability terms in the score of label sequence y (leading blank included) inside frame t: one per label and
    one blank per frame left."""
    return len(y) - 1 + t


def beam_search_margins(logits_fn, T, V, beam_size, nbest, score_norm=True, max_expansions=200):
    """Returns (n-best [(score, yseq)] or None when a frame is not left within max_expansions, the smallest
    margin-per-term seen, the largest expansion count of a frame)."""
    beam = min(beam_size, V)
    beam_k = min(beam, V - 1)
    kept = [(0.0, [0])]
    worst, most_exp = np.inf, 0
    for t in range(T):
        hyps, kept = kept, []
        for expansion in range(max_expansions + 1):
            if expansion == max_expansions:
                return None, worst, most_exp
            i_max = max(range(len(hyps)), key=lambda i: hyps[i][0])
            for i, (s2, y2) in enumerate(hyps):
                if i != i_max:
                    worst = min(worst, (hyps[i_max][0] - s2) / (terms(hyps[i_max][1], t) + terms(y2, t) + 2))
            s, y = hyps.pop(i_max)
            logp = R.log_softmax(torch.as_tensor(np.asarray(logits_fn(t, tuple(y)), dtype=np.float64))).numpy()
            kept.append((s + float(logp[0]), list(y)))
            order = np.argsort(-logp[1:], kind="stable")
            if beam_k < V - 1:
                worst = min(worst, float(logp[1 + order[beam_k - 1]] - logp[1 + order[beam_k]]) / 2)
            for k in order[:beam_k]:
                hyps.append((s + float(logp[1 + k]), y + [int(k) + 1]))
            best_left, y_left = max(hyps, key=lambda h: h[0])
            for s2, y2 in kept:
                worst = min(worst, abs(s2 - best_left) / (terms(y2, t + 1) + terms(y_left, t) + 1))
            most = sorted([h for h in kept if h[0] > best_left], key=lambda h: h[0])
            most_exp = max(most_exp, expansion + 1)
            if len(most) >= beam:
                kept = most
                break
    key = (lambda h: h[0] / len(h[1])) if score_norm else (lambda h: h[0])
    final = sorted(kept, key=key, reverse=True)
    for a, b in zip(final, final[1:nbest + 1]):
        na, nb = (len(a[1]), len(b[1])) if score_norm else (1, 1)
        worst = min(worst, (key(a) - key(b)) / (terms(a[1], T) / na + terms(b[1], T) / nb))
    return final[:nbest], worst, most_exp
