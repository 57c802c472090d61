"""A plain-Python restatement of the n-gram scorer's contract (espnet2/legacy/nets/scorers/ngram.py on kenlm), independent
of the native reader and the kernels: ARPA text parsed here, scores summed in np.float32 in kenlm's order.

  1. token -> word: `<eos>` reads as `</s>`; a string that is no unigram scores as `<unk>` (log10 p = -100 if the file has
     no `<unk>`);
  2. context: `<s>` followed by the hypothesis' words, the last N-1 of them;
  3. score(v | h) = p(c_j*, v) + bow(c_{j*+1}) + ... + bow(c_m), c_k = last k words, j* the longest k with (c_k, v) in the
     file, absent contexts / back-off columns 0; log10, probability first, then back-offs by increasing context length.

Also: writers of hand-made and seeded synthetic ARPA files for the tests."""
from collections import defaultdict

import numpy as np

F = np.float32


class RefNgram:
    def __init__(self, path, token_list):
        grams = defaultdict(dict)  # order -> words tuple -> (p, bow or None)
        order = 0
        sec = 0
        with open(path, encoding="utf-8") as f:
            for raw in f:
                line = raw.strip()
                if not line:
                    continue
                if line.startswith("\\") and line.endswith("-grams:"):
                    sec = int(line[1:].split("-")[0])
                    order = max(order, sec)
                    continue
                if line in ("\\data\\", "\\end\\") or line.startswith("ngram "):
                    sec = 0 if line != "\\end\\" else -1
                    continue
                if sec <= 0:
                    continue
                parts = line.split()
                p = F(parts[0])
                words = tuple(parts[1 : 1 + sec])
                bow = F(parts[1 + sec]) if len(parts) > 1 + sec else None
                grams[sec][words] = (p, bow)
        self.N = order
        self.grams = grams
        self.unigrams = grams[1]
        if ("<unk>",) not in self.unigrams:
            self.unigrams[("<unk>",)] = (F(-100.0), None)
        self.chardict = [t if t != "<eos>" else "</s>" for t in token_list]
        self.V = len(token_list)
        # successors of every context (for the vectorised row scores)
        self.succ = defaultdict(list)
        for k in range(2, order + 1):
            for words, (p, _) in grams[k].items():
                self.succ[words[:-1]].append((words[-1], p))
        self.words = [w for (w,) in self.unigrams]
        self.wix = {w: i for i, w in enumerate(self.words)}
        self.tok2w = np.array([self.wix.get(w, self.wix["<unk>"]) for w in self.chardict])

    def word(self, tok: int) -> str:
        w = self.chardict[tok]
        return w if (w,) in self.unigrams else "<unk>"

    def history(self, yseq):
        """words of the context of a hypothesis yseq = [sos, y1 .. yj]"""
        return ["<s>"] + [self.word(t) for t in list(yseq)[1:]]

    def _ctx(self, hist):
        h = hist[-(self.N - 1):] if self.N > 1 else []
        return [tuple(h[len(h) - k:]) for k in range(1, len(h) + 1)]  # c_1, c_2, ...

    def _bow(self, c):
        e = self.grams[len(c)].get(c)
        return None if e is None or e[1] is None else e[1]

    def score_word(self, hist, w: str) -> np.float32:
        ctx = self._ctx(hist)
        p, js = self.unigrams[(w,)][0], 0
        for k, c in enumerate(ctx, start=1):
            e = self.grams[k + 1].get(c + (w,))
            if e is not None:
                p, js = e[0], k
        acc = F(p)
        for c in ctx[js:]:
            b = self._bow(c)
            if b is not None:
                acc = F(acc + b)
        return acc

    def score(self, hist, tok: int) -> np.float32:
        return self.score_word(hist, self.word(tok))

    def row(self, hist) -> np.ndarray:
        """all V tokens at once: unigrams + back-offs, then the successors of c_1, c_2, ... overwrite"""
        ctx = self._ctx(hist)
        bows = [self._bow(c) for c in ctx]
        uni = np.array([self.unigrams[(w,)][0] for w in self.words], dtype=F)

        def tail(p, k0):
            acc = F(p)
            for b in bows[k0:]:
                if b is not None:
                    acc = F(acc + b)
            return acc

        out = uni.copy()
        for b in bows:  # (element-wise f32 additions: the same roundings as tail(uni[i], 0))
            if b is not None:
                out = (out + b).astype(F)
        for k, c in enumerate(ctx, start=1):
            for w, p in self.succ.get(c, ()):
                out[self.wix[w]] = tail(p, k)
        return out[self.tok2w]

    def path_score(self, yseq) -> np.float32:
        """teacher-forced sum of the unweighted scores of y1 .. yL (<eos> included), accumulated in f32"""
        y = list(yseq)
        acc = F(0.0)
        for j in range(1, len(y)):
            acc = F(acc + self.score(self.history(y[:j]), y[j]))
        return acc


def write_arpa(path, grams):
    """grams: {order: [(prob_text, "w1 w2 ..", bow_text or None), ...]} -> a plain-text ARPA file"""
    N = max(grams)
    lines = ["\\data\\"] + [f"ngram {k}={len(grams.get(k, []))}" for k in range(1, N + 1)] + [""]
    for k in range(1, N + 1):
        lines.append(f"\\{k}-grams:")
        for p, ws, b in grams.get(k, []):
            lines.append(f"{p}\t{ws}" + (f"\t{b}" if b is not None else ""))
        lines.append("")
    lines.append("\\end\\")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def synthetic_arpa(path, n_words, order, counts, seed, words=None, with_unk=True, dead_end=0.1):
    """A seeded ARPA file of about sum(counts) n-grams: counts[k] entries of order k+2 (k = 0 .. order-2), every n-gram's
    prefix present (what the format requires), 4-decimal values, a back-off column on most entries below the top order.
    `words`: the unigram strings (default w0 .. w{n-1} plus <s>, </s> and, with_unk, <unk>).  A fraction `dead_end` of the
    unigrams never starts a bigram."""
    rng = np.random.default_rng(seed)
    if words is None:
        words = [f"w{i}" for i in range(n_words)]
    words = list(words) + ["<s>", "</s>"] + (["<unk>"] if with_unk else [])
    nw = len(words)
    live = np.flatnonzero(rng.random(nw) >= dead_end)
    live = live[np.array([words[i] != "</s>" for i in live])]
    levels = [np.arange(nw).reshape(-1, 1)]
    for k, c in enumerate(counts[: order - 1]):
        prev = levels[-1] if k > 0 else levels[0][live]
        idx = (rng.random(int(c * 1.1) + 8) ** 3 * len(prev)).astype(np.int64)  # skewed: a few contexts with many successors
        nxt = rng.integers(0, nw, size=len(idx))
        g = np.concatenate([prev[idx], nxt.reshape(-1, 1)], axis=1)
        g = g[g[:, -1] != words.index("<s>")]
        g = np.unique(g, axis=0)
        if len(g) > c:
            g = g[np.sort(rng.choice(len(g), size=c, replace=False))]
        levels.append(g[rng.permutation(len(g))])  # (file order is not trie order: the reader sorts)

    def fmt(v):
        return [f"{x:.4f}" for x in v]

    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, g in enumerate(levels):
            f.write(f"ngram {k + 1}={len(g)}\n")
        f.write("\n")
        for k, g in enumerate(levels):
            f.write(f"\\{k + 1}-grams:\n")
            probs = fmt(-rng.random(len(g)) * 3.0 - 0.05)
            top = k == len(levels) - 1
            bows = fmt(-rng.random(len(g)) * 1.0)
            has_bow = (rng.random(len(g)) < 0.85) & (not top)
            wtxt = [" ".join(words[j] for j in row) for row in g.tolist()]
            if k == 0:
                probs[words.index("<s>")] = "-99"
            out = [f"{p}\t{w}\t{b}" if hb else f"{p}\t{w}" for p, w, b, hb in zip(probs, wtxt, bows, has_bow)]
            f.write("\n".join(out) + "\n\n")
        f.write("\\end\\\n")
    return words
