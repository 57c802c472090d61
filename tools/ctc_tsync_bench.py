"""The time-synchronous CTC search (csrc/ctc_tsync.hip, espnet_amd/nets/beam_search_timesync.py) on the bench line's shape.

    python tools/ctc_tsync_bench.py [--reps 10] [--warmup 2] [--out profiles/ctc_tsync_bench.json]

32 utterances of T = 249 encoder frames (d 256, bf16 encoder output, V 5 000), the frames peaked on a seeded label path
(p ~ 0.9 on the path's token: what a trained CTC head gives), beam 10 and 20, each without an n-gram and with a seeded
3-gram of about 10^5 entries (weight 0.5, length bonus 0.3).  Per configuration, in one process on one GPU, the three
routes ALTERNATING inside every repetition (medians with min and max of `--reps` repetitions after `--warmup`):
  * topk_ms        em_ctc_frame_topk alone on ready log-probs (device events);
  * walk_ms        em_ctc_tsync_search alone on ready candidate tables (device events);
  * tsync_tail_ms  BeamSearchTimeSync.search_batch from the encoder output on: CTC.log_softmax, both launches, the one D2H
                   copy and the hypothesis objects (host clock, synchronised before and after);
  * label_sync_ms  the route that existed before for the same job: BatchBeamSearch with ctc (+ ngram) + length_bonus at the
                   same beam, from the same encoder output on (host clock);
  * greedy_ms      em_ctc_greedy and the D2H copy of its tokens (host clock).
Before anything is timed the best hypotheses of the new search and of the label-synchronous one are compared and the
agreement is printed: they are different algorithms, so this is information, not a check."""
import argparse
import json
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import summary  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_tsync_bench: no GPU (a timing needs the device)")

    from espnet_amd.asr.ctc import CTC
    from espnet_amd.nets.batch_beam_search import build_beam_search
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync
    from espnet_amd.nets.scorers.ngram import NgramFullScorer
    from oracle.weights import token_list
    from tests.ngram_ref import synthetic_arpa

    B, T, V, D = a.batch, a.frames, a.vocab, 256
    g = torch.Generator().manual_seed(7)
    tokens = token_list(V)
    res = dict(reps=a.reps, warmup=a.warmup,
               workload=f"{B} x (T {T}, d {D}, V {V}), bf16 encoder output, frames peaked on a seeded label path")
    with torch.no_grad():
        ctc = CTC(V, D, compute_dtype="bfloat16")
        w = torch.randn(V, D, generator=g) / D ** 0.5
        ctc.ctc_lo.weight.copy_(w)
        ctc.ctc_lo.bias.zero_()
        ctc.cuda().eval()
        path = torch.zeros(B, T, dtype=torch.long)  # blanks, and tokens held for one or two frames
        for b in range(B):
            t = 0
            while t < T:
                if torch.rand(1, generator=g).item() < 0.45:
                    t += 1
                    continue
                n = int(torch.randint(1, 3, (1,), generator=g))
                path[b, t : t + n] = int(torch.randint(1, V - 1, (1,), generator=g))
                t += n
        enc = (12.0 * w[path] + 0.3 * torch.randn(B, T, D, generator=g)).to(torch.bfloat16).cuda()
        olens = [T - (3 * b) % 40 for b in range(B)]
        olens_d = torch.tensor(olens, dtype=torch.int32, device="cuda")
        lp = ctc.log_softmax(enc)
        res["mean_top1_prob"] = round(float(lp.max(dim=-1).values.exp().mean()), 3)

        with tempfile.TemporaryDirectory() as tmp:
            arpa = Path(tmp) / "bench3.arpa"
            synthetic_arpa(arpa, 0, 3, [60000, 35000], 7, words=tokens[2:-1] + ["<unk>"], with_unk=False)
            ngram = NgramFullScorer(str(arpa), tokens)
        res["ngram_entries"] = int(sum(len(x) for x in ngram.model.wid))
        model = types.SimpleNamespace(decoder=None, ctc=ctc, sos=V - 1, eos=V - 1)

        def greedy():
            _, tok, tl = ctc.greedy_device(enc, olens_d, 0, V - 1)
            return tok.cpu(), tl.cpu()

        for beam in (10, 20):
            for with_ng in (False, True):
                w_ng, pen = (0.5, 0.3) if with_ng else (0.0, 0.0)
                ng = ngram if with_ng else None
                ts = BeamSearchTimeSync(sos=V - 1, beam_size=beam, scorers=dict(ctc=ctc, **({"ngram": ng} if ng else {})),
                                        weights=dict(ctc=1.0, ngram=w_ng, length_bonus=pen), token_list=tokens)
                ls = build_beam_search(model, beam_size=beam, ctc_weight=1.0, penalty=pen, token_list=tokens, ngram=ng,
                                       ngram_weight=w_ng)
                K = ts.candidates_per_frame(V)
                tabs = CTC.topk_log_probs(lp, K, 0)
                new = ts.search_batch(enc, olens)
                old = ls.search_batch(enc, olens)
                same = sum(1 for x, y in zip(new, old) if x and y and x[0].yseq.tolist() == y[0].yseq.tolist())
                gt, gl = greedy()
                same_g = sum(1 for b, x in enumerate(new) if x and x[0].yseq.tolist()[1:-1] == gt[b, : int(gl[b])].tolist())
                r = dict(beam=beam, candidates_per_frame=K, ngram=with_ng,
                         best_equal_to_label_sync=f"{same}/{B}", best_equal_to_greedy=f"{same_g}/{B}",
                         mean_tokens=round(statistics.mean(len(x[0].yseq) - 2 for x in new if x), 1))
                print(json.dumps(r), flush=True)
                routes = dict(topk_ms=lambda: events(lambda: CTC.topk_log_probs(lp, K, 0)),
                              walk_ms=lambda: events(lambda: ts.search_candidates(*tabs, olens_d)),
                              tsync_tail_ms=lambda: wall(lambda: ts.search_batch(enc, olens)),
                              label_sync_ms=lambda: wall(lambda: ls.search_batch(enc, olens)),
                              greedy_ms=lambda: wall(greedy))
                ms = {k: [] for k in routes}
                for rep in range(a.warmup + a.reps):
                    for k, fn in routes.items():  # (alternating: every repetition runs every route once)
                        v = fn()
                        if rep >= a.warmup:
                            ms[k].append(v)
                r.update({k: summary(v) for k, v in ms.items()})
                r["label_sync_over_tsync_tail"] = round(r["label_sync_ms"]["median"] / r["tsync_tail_ms"]["median"], 2)
                res[f"beam{beam}{'_ngram' if with_ng else ''}"] = r
                print(json.dumps(r), flush=True)

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
