"""Float64 restatement of transducer forced alignment as include/espnet_amd.h states it ("transducer forced alignment"):
the max-product recursion over a lattice of (blank, next label) log-probabilities with its tie rule and back-trace, and
a brute-force arg-max over all paths.  Plain numpy on the CPU; nothing of espnet_amd is imported.  Lattices come from
tests/transducer_nll_ref.py (`lattice`, `teacher_forced_dec_out`, re-exported).
"""
import itertools
import math

import numpy as np

from tests.transducer_nll_ref import _f64, forward_nll, lattice, teacher_forced_dec_out  # noqa: F401  (re-exported)


def _no_path(T_b, U):
    return dict(tok_frame=[-1] * U, tok_logp=[0.0] * U, frame_u=[-1] * T_b, total=-math.inf)


def _outputs(lat, T_b, U, tok_frame, total):
    """The contract's outputs of a path given by the frame of every token."""
    frame_u = [sum(1 for f in tok_frame if f <= t) for t in range(T_b)]
    return dict(tok_frame=list(tok_frame), tok_logp=[float(lat[f, u, 1]) for u, f in enumerate(tok_frame)],
                frame_u=frame_u, total=float(total))


def viterbi(lat, T_b=None, U=None):
    """v[0][0] = 0; v[t][u] = max(v[t-1][u] + b[t-1][u], v[t][u-1] + e[t][u-1]), the label move (from (t, u-1)) taken only
    if STRICTLY greater than the blank move (from (t-1, u)); total = v[T_b-1][U] + b[T_b-1][U]; the path is the back-trace
    from (T_b-1, U).  lat (>= T_b, >= U + 1, 2).  Returns dict(tok_frame [U], tok_logp [U], frame_u [T_b], total);
    T_b == 0 or total == -inf: frames -1, log-probabilities 0."""
    lat = _f64(lat)
    T_b = lat.shape[0] if T_b is None else T_b
    U = lat.shape[1] - 1 if U is None else U
    if T_b == 0:
        return _no_path(T_b, U)
    b, e = lat[:T_b, : U + 1, 0].tolist(), lat[:T_b, : U + 1, 1].tolist()  # (Python floats are float64)
    ninf = -math.inf
    label = []  # label[t][u]: node (t, u) is entered by the label move
    prev = None
    for t in range(T_b):
        cur, lab = [ninf] * (U + 1), [False] * (U + 1)
        for u in range(U + 1):
            if t == 0 and u == 0:
                cur[0] = 0.0
                continue
            stay = prev[u] + b[t - 1][u] if t > 0 else ninf
            emit = cur[u - 1] + e[t][u - 1] if u > 0 else ninf
            lab[u] = emit > stay
            cur[u] = emit if lab[u] else stay
        label.append(lab)
        prev = cur
    total = prev[U] + b[T_b - 1][U]
    if not total > ninf:
        return _no_path(T_b, U)
    tok_frame = [0] * U
    t, u = T_b - 1, U
    while (t, u) != (0, 0):
        if label[t][u]:
            u -= 1
            tok_frame[u] = t
        else:
            t -= 1
        assert t >= 0 and u >= 0
    return _outputs(lat, T_b, U, tok_frame, total)


def brute_force_best(lat, T_b, U):
    """The arg-max over all C(T_b + U - 1, U) monotone paths, each path's value its terms added in path order.  Among
    paths of equal value the one that the tie rule's back-trace finds: read backwards from (T_b-1, U), it takes the blank
    move at the first node where two best paths part.  Same outputs as `viterbi`."""
    lat = _f64(lat)
    if T_b == 0:
        return _no_path(T_b, U)
    n = T_b - 1 + U
    best = None
    for emits in itertools.combinations(range(n), U):
        t = u = 0
        val = 0.0
        frames, moves = [], []
        for i in range(n):
            if i in emits:
                val = val + lat[t, u, 1]
                frames.append(t)
                moves.append(1)
                u += 1
            else:
                val = val + lat[t, u, 0]
                moves.append(0)
                t += 1
        assert t == T_b - 1 and u == U
        val = val + lat[t, u, 0]
        key = (-val, tuple(reversed(moves)))  # larger value first, then blank moves first seen from the end
        if val > -math.inf and (best is None or key < best[0]):
            best = (key, frames, val)
    if best is None:
        return _no_path(T_b, U)
    return _outputs(lat, T_b, U, best[1], best[2])


def path_value(lat, T_b, U, tok_frame):
    """The value of the path that emits token u at frame tok_frame[u], its T_b + U terms added in path order (float64)."""
    lat = _f64(lat)
    assert len(tok_frame) == U and all(0 <= f < T_b for f in tok_frame)
    assert all(tok_frame[i] <= tok_frame[i + 1] for i in range(U - 1))
    val, u = 0.0, 0
    for t in range(T_b):
        while u < U and tok_frame[u] == t:
            val = val + lat[t, u, 1]
            u += 1
        val = val + lat[t, u, 0]
    assert u == U
    return float(val)
