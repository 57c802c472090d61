"""CPU restatement of the CTC forced-alignment contract (include/espnet_amd.h, `em_ctc_forced_align`) in torch f32, and
a brute-force check of it for tiny shapes.  A helper module: tests import it, it holds no test of its own.

States s = 0 .. 2L, lab[s] = blank (s even) / y[s >> 1] (s odd); alpha[t][s] = max(stay, one, two) + lp[t][lab[s]]
with ONE f32 add per cell; of equal maxima the smallest move is recorded; the path ends in state S-1 if its alpha is
strictly greater than that of S-2.  The loop runs over frames and is vectorised over states."""
import itertools

import torch

NINF = float("-inf")


def feasible(T, y):
    """T >= L + #{i : y[i] == y[i-1]}: a path through `y` exists."""
    y = list(y)
    return T >= len(y) + sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


def forced_align_ref(lp, y, blank=0):
    """lp (T, V) f32 CPU log-posteriors, y a list of target ids (none == blank).  Returns a dict with the six outputs
    of one utterance: align (T,) int32, frame_lp (T,) f32, total f32 scalar tensor, tok_start / tok_end (L,) int32,
    tok_lp (L,) f32 - plus `path` (T,) the state sequence.  Raises ValueError for an infeasible row."""
    lp = lp.to(torch.float32).cpu()
    y = [int(v) for v in y]
    T, L = int(lp.shape[0]), len(y)
    if blank in y:
        raise ValueError("blank in the target")
    if T < 1 or not feasible(T, y):
        raise ValueError(f"{T} frames cannot carry {L} tokens")
    S = 2 * L + 1
    lab = torch.full((S,), blank, dtype=torch.long)
    lab[1::2] = torch.tensor(y, dtype=torch.long)
    allow2 = torch.zeros(S, dtype=torch.bool)
    for s in range(3, S, 2):
        allow2[s] = bool(lab[s] != lab[s - 2])
    ninf1, ninf2 = torch.full((1,), NINF), torch.full((2,), NINF)
    alpha = torch.full((S,), NINF, dtype=torch.float32)
    alpha[0] = lp[0, blank]
    if L > 0:
        alpha[1] = lp[0, y[0]]
    moves = torch.zeros(T, S, dtype=torch.int8)
    em = lp[:, lab]  # (T, S)
    for t in range(1, T):
        one = torch.cat([ninf1, alpha[:-1]])
        two = torch.cat([ninf2, alpha[:-2]])[:S]
        two = torch.where(allow2, two, torch.full_like(two, NINF))
        best, mv = alpha, torch.zeros(S, dtype=torch.int8)
        m1 = one > best
        best, mv = torch.where(m1, one, best), torch.where(m1, torch.ones_like(mv), mv)
        m2 = two > best
        best, mv = torch.where(m2, two, best), torch.where(m2, torch.full_like(mv, 2), mv)
        alpha = best + em[t]
        moves[t] = mv
    end = S - 1 if (L == 0 or bool(alpha[S - 1] > alpha[S - 2])) else S - 2
    total = alpha[end].clone()
    path = torch.zeros(T, dtype=torch.long)
    s = end
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t > 0:
            s -= int(moves[t, s])
    assert s in (0, 1) and s < S, "the back-trace must start in state 0 or 1"
    align = lab[path].to(torch.int32)
    frame_lp = lp[torch.arange(T), align.long()]
    tok_start = torch.zeros(L, dtype=torch.int32)
    tok_end = torch.zeros(L, dtype=torch.int32)
    tok_lp = torch.zeros(L, dtype=torch.float32)
    for i in range(L):
        frames = (path == 2 * i + 1).nonzero().flatten().tolist()
        assert frames and frames == list(range(frames[0], frames[-1] + 1)), "every token has one non-empty span"
        tok_start[i], tok_end[i] = frames[0], frames[-1] + 1
        acc = torch.zeros((), dtype=torch.float32)
        for t in frames:  # frame order, one f32 add each
            acc = acc + frame_lp[t]
        tok_lp[i] = acc / torch.tensor(float(len(frames)), dtype=torch.float32)
    return dict(align=align, frame_lp=frame_lp, total=total, tok_start=tok_start, tok_end=tok_end, tok_lp=tok_lp,
                path=path)


def forced_align_ref_batch(lps, ys, T, Lmax, blank=0):
    """Rows of a ragged batch -> the padded (B, T) / (B, Lmax) / (B,) tensors the device entry writes: -1 for integer
    padding, 0 for float padding.  lps[b] is (T_b, V), ys[b] a list."""
    B = len(lps)
    out = dict(align=torch.full((B, T), -1, dtype=torch.int32), frame_lp=torch.zeros(B, T),
               total=torch.zeros(B), tok_start=torch.full((B, Lmax), -1, dtype=torch.int32),
               tok_end=torch.full((B, Lmax), -1, dtype=torch.int32), tok_lp=torch.zeros(B, Lmax))
    for b, (lp, y) in enumerate(zip(lps, ys)):
        r = forced_align_ref(lp, y, blank)
        Tb, L = lp.shape[0], len(y)
        out["align"][b, :Tb], out["frame_lp"][b, :Tb], out["total"][b] = r["align"], r["frame_lp"], r["total"]
        out["tok_start"][b, :L], out["tok_end"][b, :L], out["tok_lp"][b, :L] = r["tok_start"], r["tok_end"], r["tok_lp"]
    return out


def collapse(labels, blank=0):
    """Frame labels -> token sequence: merge repeats, drop blanks."""
    out, prev = [], None
    for v in labels:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


def brute_force_best(lp, y, blank=0):
    """Enumerate all V**T label sequences of a tiny (T, V): the largest left-to-right f32 sum of lp[t][pi_t] over the
    sequences that collapse to `y` (f32 rounding is monotone, so this is what the recursion's alpha holds), or None if
    no sequence does."""
    lp = lp.to(torch.float32)
    T, V = lp.shape
    best = None
    for pi in itertools.product(range(V), repeat=T):
        if collapse(pi, blank) != list(y):
            continue
        acc = lp[0, pi[0]].clone()
        for t in range(1, T):
            acc = acc + lp[t, pi[t]]
        if best is None or bool(acc > best):
            best = acc
    return best
