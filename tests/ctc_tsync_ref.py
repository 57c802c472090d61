"""A float64 restatement of the time-synchronous CTC prefix beam search (include/espnet_amd.h, `em_ctc_tsync_search`;
csrc/ctc_tsync.hip), independent of the kernels: prefixes are Python tuples, `dp` and `next` are dicts, the n-gram goes
through tests/ngram_ref.py::RefNgram (its own f32 sums, in `path_score`'s order).  A helper module: tests import it, it
holds no test of its own.

    hyps = [(sos,)];  dp = {(sos,): (p_nb = -inf, p_b = 0)}
    per frame: cands = the K best tokens (ties to the lower id); for l in hyps, c in cands: the blank branch, the repeat
    branch (which also feeds l itself), the plain extension, and the come-back of a prefix that last frame scored and
    pruned; every key written is a member; score = w_ctc * logaddexp(next[l]) + w_ng * NG(l) + pen * (len(l) - 1);
    hyps = the W members of largest score > -inf; dp = all members.
    final = score + w_ng * ngram(eos | l); the n-best by descending final.

Besides the n-best, a run reports
  margin    the smallest decision margin: the gap between the K-th and (K+1)-th log-prob of every frame, the gap between
            the W-th and (W+1)-th member score of every frame, the gaps of the final order;
  ceiling   8 T 2^-24 max(|score|, 1) over every score the run compared: what an f32 walk may be off by (a dp value is a
            max-shifted sum of at most five terms plus an add, the error accumulates linearly over the frames);
  counters  come-backs, merges of an extension into a beam entry, frames without the blank among the candidates, repeat
            updates, and returns of a prefix to the beam while one of its children stayed in it.
`cases` picks seeds by margin >= 2 * ceiling with this reference alone, the same on every machine."""
import math

import numpy as np

NINF = float("-inf")
SEED_WINDOW = 64


def lae(a, b):
    m = max(a, b)
    if m == NINF:
        return NINF
    return m + math.log1p(math.exp(min(a, b) - m))


def topk_ref(row, K):
    """ids of the K largest values, descending, ties to the lower id (a stable sort of the negated row)"""
    return np.argsort(-np.asarray(row, dtype=np.float64), kind="stable")[:K]


def gen_logprobs(T, V, seed, peak=3.0, noise=1.5):
    """CTC-like f32 log-probs (T, V): a random label path with blanks and repeats, a peak on it, Gaussian noise under it.
    Labels are drawn from 1 .. V-2 (0 is the blank, V-1 <sos/eos>)."""
    rng = np.random.default_rng(1000 + seed)
    path = []
    while len(path) < T:
        if rng.random() < 0.45:
            path.append(0)
        else:
            path += [int(rng.integers(1, max(V - 1, 2)))] * int(rng.integers(1, 3))
    logits = rng.normal(0.0, noise, size=(T, V))
    logits[np.arange(T), np.array(path[:T])] += peak
    logits -= logits.max(axis=1, keepdims=True)
    lp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    return lp.astype(np.float32)


class Result:
    def __init__(self):
        self.nbest = []      # (tokens list without sos, final, ctc, ngram with the eos term, len - 1)
        self.margin = math.inf
        self.ceiling = 0.0
        self.counters = dict(comebacks=0, merges=0, blank_out=0, repeats=0, returns_with_child=0)
        self.dp = {}         # prefix -> (p_nb, p_b) after the last frame (all members)

    def tokens(self):
        return [h[0] for h in self.nbest]


def tsync_ref(lp, W, K, sos, blank=0, w_ctc=1.0, w_ng=0.0, pen=0.0, ngram=None, T_valid=None):
    """lp (T, V) log-probs (taken into float64 as they are); only the first T_valid frames are walked."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    if T_valid is not None:
        T = int(T_valid)
    res = Result()
    F = np.float32
    ng_of = {(sos,): F(0.0)}

    def NG(l):
        if ngram is None:
            return 0.0
        v = ng_of.get(l)
        if v is None:
            v = ng_of[l] = F(NG(l[:-1]) + ngram.score(ngram.history(l[:-1]), l[-1]))
        return v

    smax = 1.0
    hyps = [(sos,)]
    dp = {(sos,): (NINF, 0.0)}
    was_in_beam = {(sos,)}
    for t in range(T):
        row = lp[t]
        order = np.argsort(-row, kind="stable")
        cands = [int(c) for c in order[:K]]
        if K < V:
            res.margin = min(res.margin, float(row[order[K - 1]] - row[order[K]]))
        if blank not in cands:
            res.counters["blank_out"] += 1
        nxt, members = {}, []

        def get(l):
            return nxt.get(l, (NINF, NINF))

        def add(l):
            if l not in nxt:
                members.append(l)

        hset = set(hyps)
        for l in hyps:
            pnb_l, pb_l = dp[l]
            prev = lae(pnb_l, pb_l)
            for c in cands:
                if c == blank:
                    nb, b = get(l)
                    add(l)
                    nxt[l] = (nb, lae(b, row[blank] + prev))
                    continue
                l2 = l + (c,)
                nb, b = get(l2)
                if c == l[-1]:
                    nb = lae(nb, row[c] + pb_l)
                    snb, sb = get(l)
                    add(l)
                    nxt[l] = (lae(snb, row[c] + pnb_l), sb)
                    res.counters["repeats"] += 1
                else:
                    nb = lae(nb, row[c] + prev)
                if l2 in hset:
                    res.counters["merges"] += 1
                elif l2 in dp:
                    b = lae(b, row[blank] + lae(*dp[l2]))
                    nb = lae(nb, row[c] + dp[l2][0])
                    res.counters["comebacks"] += 1
                add(l2)
                nxt[l2] = (nb, b)
        scored = []
        for l in members:
            s = lae(*nxt[l])
            if s == NINF:
                continue
            sc = w_ctc * s + w_ng * float(NG(l)) + pen * (len(l) - 1)
            scored.append((sc, l))
            smax = max(smax, abs(sc))
        scored.sort(key=lambda e: -e[0])
        if len(scored) > W:
            res.margin = min(res.margin, scored[W - 1][0] - scored[W][0])
        new = [l for _, l in scored[:W]]
        for l in new:  # a prefix that was in the beam, left it, and is back while one of its children stayed throughout
            if l in was_in_beam and l not in hset:
                if any(len(c) == len(l) + 1 and c[:-1] == l and c in hset for c in new):
                    res.counters["returns_with_child"] += 1
        was_in_beam.update(new)
        hyps, dp = new, nxt
    fin = []
    for l in hyps:
        ctc = lae(*dp[l])
        e = float(ngram.score(ngram.history(l), sos)) if (ngram is not None and T > 0) else 0.0
        core = w_ctc * ctc + w_ng * float(NG(l)) + pen * (len(l) - 1)
        ngt = float(F(NG(l) + F(e))) if ngram is not None else 0.0
        fin.append((list(l[1:]), core + w_ng * e, ctc, ngt, float(len(l) - 1)))
        smax = max(smax, abs(core + w_ng * e))
    fin.sort(key=lambda h: -h[1])
    for a, b in zip(fin, fin[1:]):
        res.margin = min(res.margin, a[1] - b[1])
    res.nbest = fin
    res.dp = dp
    res.ceiling = 8.0 * max(T, 1) * 2.0 ** -24 * max(smax, 1.0)
    return res


_CASES = {}


def cases(T, V, W, n, K=None, key=None, **kw):
    """The first n seeds (scanning 0, 1, ...) whose run has margin >= 2 * ceiling: [(seed, lp f32 (T, V), Result)].
    `kw`: the search's weights and n-gram; `key`: what distinguishes them in the cache (the n-gram is not hashable).
    Raises if the first SEED_WINDOW seeds do not hold n of them: nothing is skipped at run time."""
    K = min(int(1.5 * W), V) if K is None else K
    ck = (T, V, W, n, K, key)
    if ck not in _CASES:
        out = []
        for seed in range(SEED_WINDOW):
            lp = gen_logprobs(T, V, seed)
            r = tsync_ref(lp, W, K, V - 1, **kw)
            if r.margin >= 2.0 * r.ceiling:
                out.append((seed, lp, r))
                if len(out) == n:
                    break
        if len(out) < n:
            raise AssertionError(f"cases(T={T}, V={V}, W={W}, K={K}, {key}): only {len(out)} of {n} seeds with margin >= "
                                 f"2 x ceiling among the first {SEED_WINDOW}")
        _CASES[ck] = out
    return _CASES[ck]


def find_return_with_child(T, V, W, K, limit=SEED_WINDOW, peak=0.0, noise=1.0, **kw):
    """The first seed whose run has a prefix return to the beam while its child stays, with margin >= 2 * ceiling.  The
    event is rare under a peaked path (about 1 seed in 200 at T 24, V 12, W 4); flat log-probs over a tiny vocabulary
    (the defaults here, with T 20, V 4, W 6, K 3) show it in about one seed of four."""
    for seed in range(limit):
        lp = gen_logprobs(T, V, seed, peak=peak, noise=noise)
        r = tsync_ref(lp, W, K, V - 1, **kw)
        if r.counters["returns_with_child"] > 0 and r.margin >= 2.0 * r.ceiling:
            return seed, lp, r
    raise AssertionError(f"no seed below {limit} has a prefix leave the beam and return while its child stays")


# ------------------------------------------------------------------------------------------- what the GPU tests run
# name -> (T, V, W, K, n): tests/test_gpu_ctc_tsync.py walks exactly these, each without an n-gram and with the 3-gram of
# `ngram_setup` plus a length bonus; tests/test_cpu_ctc_tsync.py holds every one of them to the seed window.
WALK_CASES = {
    "short": (7, 12, 3, 4, 3),
    "branches": (24, 12, 4, 6, 3),       # every branch of the recursion fires (asserted from the counters)
    "default_beam": (24, 65, 20, 30, 1),  # the reference's default beam_size
    "limits": (16, 80, 32, 64, 1),        # W_max, K_max of em_ctc_tsync_limits
    "k_equals_v": (24, 12, 4, 12, 2),
    "beam_not_full": (2, 4, 32, 4, 2),    # fewer distinct prefixes (<= 13) than W: count < nbest
}
NG_WEIGHTS = dict(w_ng=0.5, pen=0.3)


def ngram_setup(tmp_dir, V, seed=11, tokens=None):
    """(path, tokens, RefNgram): a seeded 3-gram over most of the V token strings, as tests/test_gpu_ngram.py builds its
    files (the other tokens, <blank> and <sos/eos> are no unigrams and score as <unk>)."""
    from oracle.weights import token_list
    from tests.ngram_ref import RefNgram, synthetic_arpa

    tokens = token_list(V) if tokens is None else list(tokens)
    rng = np.random.default_rng(seed)
    words = [t for t in tokens[2:-1] if rng.random() < 0.85] + ["<unk>"]
    nw = len(words) + 2
    path = tmp_dir / f"tsync3_{V}.arpa"
    synthetic_arpa(path, 0, 3, [40 * nw, 25 * nw], seed, words=words, with_unk=False)
    return path, tokens, RefNgram(path, tokens)


def walk_cases(name, ngram=None):
    """The cases of WALK_CASES[name]: without an n-gram (ngram None) or with it and NG_WEIGHTS."""
    T, V, W, K, n = WALK_CASES[name]
    if ngram is None:
        return cases(T, V, W, n, K=K, key="plain")
    return cases(T, V, W, n, K=K, key="ngram", ngram=ngram, **NG_WEIGHTS)
