"""The resumable time-synchronous CTC search (em_ctc_tsync_extend; BeamSearchTimeSync.extend) on a server's tick.

    python tools/ctc_tsync_stream_bench.py [--reps 5] [--warmup 1] [--out profiles/ctc_tsync_stream_bench.json] [--table]

S = 32 and 128 live streams, 16 new encoder frames per stream and tick (d 256, bf16 encoder output, V 5 000), the frames
peaked on a seeded label path as in tools/ctc_tsync_bench.py, 15 ticks per utterance (240 frames), beam 10 and 20, each
without an n-gram and with a seeded 3-gram of about 10^5 entries (weight 0.5, length bonus 0.3).  One process, one GPU; per
configuration every repetition runs every leg once, in turn (medians with min and max of `--reps` repetitions after
`--warmup`).  The host legs return the best hypothesis per stream (nbest 1, what `batch_call` hands out).
  (a) tick_ms            one tick: CTC.log_softmax + em_ctc_frame_topk on the 16 new frames, em_ctc_tsync_extend, the one D2H
                         copy and the hypothesis objects (host clock, synchronised before and after); over all 15 ticks of
                         an utterance, and `tick_last_ms` for the 15th alone (the longest token rows travel there);
  (b) walks15_ms         the 15 em_ctc_tsync_extend launches of an utterance on ready candidate tables (device events, summed)
      walk_one_shot_ms   ONE em_ctc_tsync_search over the same 240 frames (device events): the difference is the price of
                         saving and restoring the state 15 times;
  (c) rerun15_ms         the only route to beam partials before: BeamSearchTimeSync.search_batch over the accumulated
                         history at every tick, the 15-tick total (host clock);
  (d) greedy_tick_ms     the greedy tick's CTC.argmax on the same 16 frames and its D2H copy (host clock).
Before anything is timed, the 15 ticks' final outputs are compared with the one-shot search on the same tables, bit for
bit.  Not measured here: the kernel's shares inside a frame, trained models, the encoder in front of the tick."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import summary  # noqa: E402

TICK, TICKS = 16, 15


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


def table(res):
    """the DESIGN.md table: one row per configuration, medians (min-max) in ms"""
    def c(v):
        return f"{v['median']:.3f} ({v['min']:.3f}-{v['max']:.3f})"

    rows = ["| S | beam | n-gram | (a) tick | (a) 15th tick | (b) 15 walks | (b) one-shot walk | (c) re-run, 15 ticks | (d) greedy tick |",
            "|---|---|---|---|---|---|---|---|---|"]
    for k, r in res.items():
        if isinstance(r, dict) and "tick_ms" in r:
            rows.append(f"| {r['streams']} | {r['beam']} | {'yes' if r['ngram'] else 'no'} | {c(r['tick_ms'])} | {c(r['tick_last_ms'])} | "
                        f"{c(r['walks15_ms'])} | {c(r['walk_one_shot_ms'])} | {c(r['rerun15_ms'])} | {c(r['greedy_tick_ms'])} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", action="store_true", help="print the DESIGN.md table after the result line")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_tsync_stream_bench: no GPU (a timing needs the device)")

    from espnet_amd.asr.ctc import CTC
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync
    from espnet_amd.nets.scorers.ngram import NgramFullScorer
    from oracle.weights import token_list
    from tests.ngram_ref import synthetic_arpa

    V, D, T = a.vocab, 256, TICK * TICKS
    g = torch.Generator().manual_seed(7)
    tokens = token_list(V)
    res = dict(reps=a.reps, warmup=a.warmup,
               workload=f"S x {TICKS} ticks of {TICK} frames (d {D}, V {V}), bf16 encoder output, frames peaked on a seeded "
                        "label path; host legs with nbest 1")
    with torch.no_grad():
        ctc = CTC(V, D, compute_dtype="bfloat16")
        w = torch.randn(V, D, generator=g) / D ** 0.5
        ctc.ctc_lo.weight.copy_(w)
        ctc.ctc_lo.bias.zero_()
        ctc.cuda().eval()
        with tempfile.TemporaryDirectory() as tmp:
            arpa = Path(tmp) / "bench3.arpa"
            synthetic_arpa(arpa, 0, 3, [60000, 35000], 7, words=tokens[2:-1] + ["<unk>"], with_unk=False)
            ngram = NgramFullScorer(str(arpa), tokens)
        res["ngram_entries"] = int(sum(len(x) for x in ngram.model.wid))

        for S in a.streams:
            path = torch.zeros(S, T, dtype=torch.long)  # blanks, and tokens held for one or two frames
            for b in range(S):
                t = 0
                while t < T:
                    if torch.rand(1, generator=g).item() < 0.45:
                        t += 1
                        continue
                    n = int(torch.randint(1, 3, (1,), generator=g))
                    path[b, t : t + n] = int(torch.randint(1, V - 1, (1,), generator=g))
                    t += n
            enc = (12.0 * w[path] + 0.3 * torch.randn(S, T, D, generator=g)).to(torch.bfloat16).cuda()
            chunks = [enc[:, k * TICK : (k + 1) * TICK].contiguous() for k in range(TICKS)]
            hist = [enc[:, : (k + 1) * TICK].contiguous() for k in range(TICKS)]
            slots, full = list(range(S)), [TICK] * S

            for beam in (10, 20):
                for with_ng in (False, True):
                    w_ng, pen = (0.5, 0.3) if with_ng else (0.0, 0.0)
                    ts = BeamSearchTimeSync(sos=V - 1, beam_size=beam, weights=dict(ctc=1.0, ngram=w_ng, length_bonus=pen),
                                            scorers=dict(ctc=ctc, **({"ngram": ngram} if with_ng else {})), token_list=tokens)
                    K = ts.candidates_per_frame(V)
                    state = ts.stream_state(S, T, "cuda")
                    for _ in range(S):
                        state.acquire()
                    tabs = ctc.frame_topk_device(enc, K, 0)
                    tick_tabs = [tuple(x[:, k * TICK : (k + 1) * TICK].contiguous() for x in tabs) for k in range(TICKS)]

                    def ext(k, nbest=1):
                        return ts.extend_candidates(*tick_tabs[k], full, slots, [k == 0] * S, state, nbest)

                    # the defining property on this workload, before anything is timed
                    for k in range(TICKS):
                        last = ext(k, beam)
                    one = ts.search_candidates(*tabs, [T] * S, beam)
                    same = all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x,
                                           y.view(torch.int32) if y.is_floating_point() else y)
                               for x, y in zip(last.outs[:7], one))
                    if not same:
                        raise SystemExit(f"S {S} beam {beam} ngram {with_ng}: 15 ticks differ from the one-shot search")

                    def tick(k):
                        return ts.collect(ts.extend(chunks[k], full, slots, [k == 0] * S, state, nbest=1))

                    def greedy(k):
                        return ctc.argmax(chunks[k], as_int32=True).cpu()

                    ms = dict(tick_ms=[], tick_last_ms=[], walks15_ms=[], walk_one_shot_ms=[], rerun15_ms=[], greedy_tick_ms=[])
                    for rep in range(a.warmup + a.reps):
                        keep = rep >= a.warmup
                        va = [wall(lambda: tick(k)) for k in range(TICKS)]
                        vb = sum(events(lambda: ext(k)) for k in range(TICKS))
                        vo = events(lambda: ts.search_candidates(*tabs, [T] * S, 1))
                        vc = sum(wall(lambda: ts.search_batch(hist[k], [(k + 1) * TICK] * S, nbest=1)) for k in range(TICKS))
                        vd = [wall(lambda: greedy(k)) for k in range(TICKS)]
                        if keep:
                            ms["tick_ms"] += va
                            ms["tick_last_ms"].append(va[-1])
                            ms["walks15_ms"].append(vb)
                            ms["walk_one_shot_ms"].append(vo)
                            ms["rerun15_ms"].append(vc)
                            ms["greedy_tick_ms"] += vd
                    r = dict(streams=S, beam=beam, candidates_per_frame=K, ngram=with_ng, slot_bytes=state.slot_bytes,
                             ticks_equal_one_shot=True)
                    r.update({k: summary(v) for k, v in ms.items()})
                    r["walks15_over_one_shot"] = round(r["walks15_ms"]["median"] / r["walk_one_shot_ms"]["median"], 2)
                    r["tick_over_greedy_tick"] = round(r["tick_ms"]["median"] / r["greedy_tick_ms"]["median"], 2)
                    res[f"S{S}_beam{beam}{'_ngram' if with_ng else ''}"] = r
                    print(json.dumps(r), flush=True)

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    if a.table:
        print(table(res))


if __name__ == "__main__":
    main()
