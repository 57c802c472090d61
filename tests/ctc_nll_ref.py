"""CPU restatement of the CTC likelihood contract (include/espnet_amd.h, `em_ctc_seq_nll`) in float64, and a brute-force
check of it for tiny shapes.  A helper module: tests import it, it holds no test of its own.  It does not call
torch.nn.functional.ctc_loss.

States s = 0 .. 2L, lab[s] = blank (s even) / y[s >> 1] (s odd); alpha[0][0] = lp[0][blank], alpha[0][1] = lp[0][y[0]];
alpha[t][s] = logsumexp(alpha[t-1][s], alpha[t-1][s-1], alpha[t-1][s-2]) + lp[t][lab[s]], the move by two only for odd
s >= 3 with lab[s] != lab[s-2]; nll = -logsumexp(alpha[T-1][S-1], alpha[T-1][S-2]) (-alpha[T-1][0] for L == 0); +inf when
no path exists or T == 0.  The loop runs over frames and is vectorised over states."""
import itertools
import math

import torch

from tests.ctc_align_ref import collapse

NINF = float("-inf")


def _lse(rows):
    """Max-shifted logsumexp over dim 0 of a (k, S) float64 stack; columns that are all -inf give -inf."""
    m = rows.max(dim=0).values
    sh = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return m + torch.log(torch.exp(rows - sh).sum(dim=0))  # (all -inf: m = -inf, the sum 0: -inf + -inf = -inf)


def ctc_nll_ref(lp, y, blank=0):
    """lp (T, V) log-posteriors (any float dtype, taken as they are into float64), y a list of target ids (none ==
    blank).  Returns the nll as a Python float (float64), math.inf when no path exists."""
    lp = lp.detach().cpu().to(torch.float64)
    y = [int(v) for v in y]
    if blank in y:
        raise ValueError("blank in the target")
    T, L = int(lp.shape[0]), len(y)
    if T == 0:
        return math.inf
    S = 2 * L + 1
    lab = torch.full((S,), blank, dtype=torch.long)
    lab[1::2] = torch.tensor(y, dtype=torch.long)
    allow2 = torch.zeros(S, dtype=torch.bool)
    for s in range(3, S, 2):
        allow2[s] = bool(lab[s] != lab[s - 2])
    ninf1 = torch.full((1,), NINF, dtype=torch.float64)
    ninf2 = torch.full((2,), NINF, dtype=torch.float64)
    alpha = torch.full((S,), NINF, dtype=torch.float64)
    alpha[0] = lp[0, blank]
    if L > 0:
        alpha[1] = lp[0, y[0]]
    em = lp[:, lab]  # (T, S)
    for t in range(1, T):
        one = torch.cat([ninf1, alpha[:-1]])
        two = torch.cat([ninf2, alpha[:-2]])[:S]
        two = torch.where(allow2, two, torch.full_like(two, NINF))
        alpha = _lse(torch.stack([alpha, one, two])) + em[t]
    last = alpha[S - 1 :] if L == 0 else alpha[S - 2 :]
    return -float(_lse(last.reshape(-1, 1))[0])


def ctc_nll_ref_batch(lps, ys, blank=0):
    """Rows -> (N,) float64 tensor."""
    return torch.tensor([ctc_nll_ref(lp, y, blank) for lp, y in zip(lps, ys)], dtype=torch.float64)


def brute_force_nll(lp, y, blank=0):
    """Enumerate all V**T label sequences of a tiny (T, V): -log of the summed probability of those that collapse to
    `y` (float64, plain sum of exp), math.inf if none does."""
    lp = lp.detach().cpu().to(torch.float64)
    T, V = lp.shape
    p = 0.0
    for pi in itertools.product(range(V), repeat=T):
        if collapse(pi, blank) == list(y):
            p += math.exp(sum(float(lp[t, pi[t]]) for t in range(T)))
    return -math.log(p) if p > 0.0 else math.inf
