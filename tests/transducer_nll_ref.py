"""Float64 restatement of the transducer likelihood of given transcripts as include/espnet_amd.h states it ("transducer
likelihood of given transcripts"): the joint network's two wanted log-probabilities at every lattice node and the
forward (sum-product) recursion over the lattice.  Plain numpy / torch on the CPU; nothing of espnet_amd is imported.
"""
import itertools
import math

import numpy as np
import torch

from tests.transducer_ref import Params, dec_step, joint_logits, log_softmax  # noqa: F401  (re-exported for the tests)


def _f64(x):
    return x.detach().cpu().to(torch.float64).numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def lattice(p: Params, enc_proj, dec_proj, targets, T_b=None, U=None, round_z=False):
    """One candidate.  enc_proj (T, jp) = lin_enc(enc) + bias of its utterance, dec_proj (>= U + 1, jp) = lin_dec of the
    prediction network after blank, y_0 .. y_{u-1} (columns past the joint space are zero padding and ignored), targets
    the token ids.  Returns lat (T_b, U + 1, 2) float64: [..., 0] = log p(blank), [..., 1] = log p(targets[u]) for u < U
    and -inf at u == U.  round_z: z is rounded once to bf16 (from float32, as the device rounds it)."""
    enc_proj, dec_proj = _f64(enc_proj), _f64(dec_proj)
    T_b = enc_proj.shape[0] if T_b is None else T_b
    U = len(targets) if U is None else U
    W, b = p.out_w.numpy(), p.out_b.numpy()
    J = W.shape[1]
    lat = np.full((T_b, U + 1, 2), -np.inf)
    for t in range(T_b):
        z = np.tanh(enc_proj[t, None, :J] + dec_proj[: U + 1, :J])  # (U + 1, J)
        if round_z:
            z = torch.from_numpy(z).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
        logits = z @ W.T + b
        mx = logits.max(axis=1, keepdims=True)
        lse = (mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True)))[:, 0]
        lat[t, :, 0] = logits[:, p.blank] - lse
        for u in range(U):
            lat[t, u, 1] = logits[u, int(targets[u])] - lse[u]
    return lat


def teacher_forced_dec_out(p: Params, y):
    """dec_out (len(y) + 1, H): the prediction network's output after blank, y_0 .. y_{u-1}."""
    out, st = dec_step(p, p.blank, p.init_state())
    rows = [out]
    for tok in y:
        out, st = dec_step(p, int(tok), st)
        rows.append(out)
    return torch.stack(rows)


def _logaddexp(x, y):
    hi, lo = max(x, y), min(x, y)
    if hi == -math.inf:
        return -math.inf
    return hi + math.log1p(math.exp(lo - hi))


def forward_nll(lat, T_b=None, U=None):
    """alpha[0][0] = 0; alpha[t][u] = logaddexp(alpha[t-1][u] + b[t-1][u], alpha[t][u-1] + e[t][u-1]);
    nll = -(alpha[T_b-1][U] + b[T_b-1][U]), +inf for T_b == 0.  lat (>= T_b, >= U + 1, 2)."""
    lat = _f64(lat)
    T_b = lat.shape[0] if T_b is None else T_b
    U = lat.shape[1] - 1 if U is None else U
    if T_b == 0:
        return math.inf
    alpha = np.full((T_b, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(T_b):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            stay = alpha[t - 1, u] + lat[t - 1, u, 0] if t > 0 else -math.inf
            emit = alpha[t, u - 1] + lat[t, u - 1, 1] if u > 0 else -math.inf
            alpha[t, u] = _logaddexp(float(stay), float(emit))
    return -(float(alpha[T_b - 1, U]) + float(lat[T_b - 1, U, 0]))


def brute_force_nll(lat, T_b, U):
    """-log of the sum over all monotone paths: the U label moves placed among the T_b - 1 frame moves, then the closing
    blank.  C(T_b + U - 1, U) paths."""
    lat = _f64(lat)
    if T_b == 0:
        return math.inf
    total = 0.0
    n = T_b - 1 + U
    for emits in itertools.combinations(range(n), U):
        t = u = 0
        lp = 0.0
        for i in range(n):
            if i in emits:
                lp += lat[t, u, 1]
                u += 1
            else:
                lp += lat[t, u, 0]
                t += 1
        assert t == T_b - 1 and u == U
        lp += lat[t, u, 0]
        total += math.exp(lp) if lp > -math.inf else 0.0
    return -math.log(total) if total > 0.0 else math.inf


def model_nll(p: Params, enc_out, y, round_z=False):
    """The whole chain in float64 from an utterance's encoder output (T_b, D): -log p(y | x)."""
    enc_out = torch.as_tensor(enc_out).to(torch.float64)
    enc_proj = enc_out @ p.enc_w.T + p.enc_b
    dec_proj = teacher_forced_dec_out(p, y) @ p.dec_w.T
    return forward_nll(lattice(p, enc_proj, dec_proj, y, round_z=round_z), enc_out.shape[0], len(y))
