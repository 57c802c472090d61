"""CPU restatement of the CTC token-posterior contract (include/espnet_amd.h, `em_ctc_seq_posteriors`) in float64 NumPy:
plain forward-backward over a (T, V) log-probability matrix.  A helper module: tests import it, it holds no test."""
import math

import numpy as np


def _lse(rows):
    """Max-shifted logsumexp over axis 0; columns that are all -inf give -inf."""
    m = rows.max(axis=0)
    sh = np.where(np.isinf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return m + np.log(np.exp(rows - sh).sum(axis=0))


def ctc_post_ref(lp, y, blank=0):
    """lp (T, V) log-posteriors (taken as they are into float64), y a list of target ids (none == blank).  Returns
    (nll, gamma (T, S), occ (L,), peak (L,), peak_t (L,) int, blank_post (T,)); without a path: inf, zeros, peak_t -1."""
    lp = np.asarray(lp, dtype=np.float64)
    y = [int(v) for v in y]
    T, L = lp.shape[0], len(y)
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)  # the move s - 2 -> s
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    none = (math.inf, np.zeros((T, S)), np.zeros(L), np.zeros(L), np.full(L, -1, dtype=np.int64), np.zeros(T))
    if T == 0:
        return none
    em = lp[:, lab]
    ninf = np.full(2, -np.inf)
    alpha = np.full((T, S), -np.inf)
    beta = np.full((T, S), -np.inf)
    alpha[0, :2] = em[0, :2]
    beta[T - 1, max(S - 2, 0):] = em[T - 1, max(S - 2, 0):]
    for t in range(1, T):
        a = alpha[t - 1]
        two = np.where(skip, np.concatenate([ninf, a[:-2]])[:S], -np.inf)
        alpha[t] = _lse(np.stack([a, np.concatenate([ninf[:1], a[:-1]]), two])) + em[t]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        two = np.where(np.concatenate([skip[2:], [False, False]])[:S], np.concatenate([b[2:], ninf])[:S], -np.inf)
        beta[t] = _lse(np.stack([b, np.concatenate([b[1:], ninf[:1]]), two])) + em[t]
    logp = float(_lse(alpha[T - 1, max(S - 2, 0):].reshape(-1, 1))[0])
    if logp == -math.inf:
        return none
    with np.errstate(invalid="ignore"):
        gamma = np.exp(alpha + beta - np.where(np.isinf(em), 0.0, em) - logp)
    gamma = np.where(np.isinf(alpha) | np.isinf(beta), 0.0, gamma)
    tok = gamma[:, 1::2]
    return -logp, gamma, tok.sum(axis=0), tok.max(axis=0), tok.argmax(axis=0), gamma[:, 0::2].sum(axis=1)
