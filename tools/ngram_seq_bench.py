"""Whole-sentence n-gram scoring (em_ngram_seq_logp, csrc/ngram_seq.hip) against the route that existed before it.

    python tools/ngram_seq_bench.py [--reps 20] [--warmup 3] [--out profiles/ngram_seq_bench.json]

A seeded 3-gram of about 10^5 entries over V 5 000 (the synthetic ARPA of tools/ctc_tsync_bench.py) and two workloads:
64 ragged sentences of 40-80 tokens, and one sentence of 3 000 tokens.  The sentences string n-grams of the file together
with single random tokens in between, so that every matched order occurs (the mix is printed).  Per workload, in one process
on one GPU, the routes ALTERNATING inside every repetition (medians with min and max of `--reps` repetitions after
`--warmup`):
  * seq_launch_ms  em_ngram_seq_logp alone on device-resident ids (device events);
  * seq_call_ms    Ngrambase.sequence_logp from host ids on: the host checks, the two H2D copies, the output tensors and
                   the launch (host clock, synchronised before and after);
  * stepped_ms     the route that existed before: em_ngram_score position by position from the start state, the state
                   tensors handed from call to call on the device, the wanted column of every V-wide row gathered into the
                   result (host clock, synchronised before and after; called through the C ABI directly, without the
                   per-row state lists of `batch_score`, so this is the old route at its leanest).
Before anything is timed the two routes' per-position values are compared bit for bit; a difference ends the run."""
import argparse
import ctypes as C
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import summary  # noqa: E402
from tools.ctc_tsync_bench import events, wall  # noqa: E402


def sentences(scorer, lens, seed):
    """Token ids (len(lens), max(lens)) int32: n-grams of the model strung together, one random token in five draws."""
    md, rng, V = scorer.model, np.random.default_rng(seed), scorer.charlen
    ys = np.zeros((len(lens), max(lens)), dtype=np.int32)
    for r, n in enumerate(lens):
        y = []
        while len(y) < n:
            if rng.random() < 0.2:
                y.append(int(rng.integers(1, V - 1)))
                continue
            k = int(rng.integers(md.order))
            e, words = int(rng.integers(len(md.wid[k]))), []
            for lv in range(k, -1, -1):  # the entry's words, last first, through its ancestors
                words.append(int(md.wid[lv][e]))
                if lv:
                    e = int(np.searchsorted(md.next[lv - 1], e, side="right")) - 1
            y += [max(int(scorer.word2tok[w]), 1) for w in reversed(words)]
        ys[r, :n] = y[:n]
    return torch.from_numpy(ys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngram_seq_bench: no GPU (a timing needs the device)")

    from espnet_amd import lib as L
    from espnet_amd.nets.scorers.ngram import NgramFullScorer
    from oracle.weights import token_list
    from tests.ngram_ref import synthetic_arpa

    V = a.vocab
    tokens = token_list(V)
    with tempfile.TemporaryDirectory() as tmp:
        arpa = Path(tmp) / "bench3.arpa"
        synthetic_arpa(arpa, 0, 3, [60000, 35000], 7, words=tokens[2:-1] + ["<unk>"], with_unk=False)
        ng = NgramFullScorer(str(arpa), tokens)
    lib, dev = L.load(), torch.device("cuda")
    pk = ng.packed(dev)
    res = dict(reps=a.reps, warmup=a.warmup, vocab=V, order=ng.order, ngram_entries=int(sum(len(x) for x in ng.model.wid)),
               kernel_shares="not profiled")
    g = torch.Generator().manual_seed(7)
    loads = dict(ragged_64x40_80=torch.randint(40, 81, (64,), generator=g).tolist(), one_x_3000=[3000])
    for name, lens in loads.items():
        ys_h, len_h = sentences(ng, lens, 7), torch.tensor(lens, dtype=torch.int32)
        n, Lp = ys_h.shape
        ys_d, len_d = ys_h.cuda(), len_h.cuda()
        target = torch.cat([ys_d, ys_d.new_zeros(n, 1)], 1).long()
        target[torch.arange(n, device=dev), len_d.long()] = V - 1
        last = torch.cat([ys_d.new_full((n, 1), -1), ys_d, ys_d.new_zeros(n, 1)], 1).t().contiguous()  # [step][row]
        st = [torch.empty(n, ng.state_len, dtype=torch.int32, device=dev) for _ in range(2)]
        row, stepped_out = torch.empty(n, V, device=dev), torch.zeros(n, Lp + 1, device=dev)
        out = [torch.zeros(n, Lp + 1, device=dev), torch.zeros(n, Lp + 1, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.float64, device=dev)]
        stream = L.current_stream_ptr()

        def seq_launch():
            L.check(lib.em_ngram_seq_logp(C.byref(pk.w), L.ptr(ys_d), L.ptr(len_d), L.ptr(ys_h), L.ptr(len_h), n, Lp, V - 1,
                                          L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), stream), "em_ngram_seq_logp")

        def stepped():
            for j in range(Lp + 1):
                L.check(lib.em_ngram_score(C.byref(pk.w), n, L.ptr(st[j & 1]), L.ptr(last[j]), L.ptr(st[1 - (j & 1)]), None, 0,
                                           L.ptr(row), stream), "em_ngram_score")
                stepped_out[:, j] = row.gather(1, target[:, j:j + 1])[:, 0]

        seq_launch()
        stepped()
        live = torch.arange(Lp + 1, device=dev).unsqueeze(0) <= len_d.unsqueeze(1)
        if not torch.equal(out[0][live].view(torch.int32), stepped_out[live].view(torch.int32)):
            raise SystemExit(f"ngram_seq_bench: {name}: the two routes differ")
        orders = out[1][live]
        r = dict(sentences=n, positions=int(live.sum()), launches_stepped=Lp + 1,
                 matched_order_share={str(k): round(float((orders == k).float().mean()), 3) for k in range(1, ng.order + 1)})
        routes = dict(seq_launch_ms=lambda: events(seq_launch),
                      seq_call_ms=lambda: wall(lambda: ng.sequence_logp(ys_h, len_h, eos=True)),
                      stepped_ms=lambda: wall(stepped))
        ms = {k: [] for k in routes}
        for rep in range(a.warmup + a.reps):
            for k, fn in routes.items():  # (alternating: every repetition runs every route once)
                v = fn()
                if rep >= a.warmup:
                    ms[k].append(v)
        r.update({k: summary(v) for k, v in ms.items()})
        r["stepped_over_seq_call"] = round(r["stepped_ms"]["median"] / r["seq_call_ms"]["median"], 1)
        r["slowest_seq_call_vs_fastest_stepped"] = round(r["stepped_ms"]["min"] / r["seq_call_ms"]["max"], 1)
        res[name] = r
        print(json.dumps({name: r}), flush=True)

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
