"""Transducer default beam search, 32 x 10 s: Conformer-small encoder + LSTM 1 x 512 prediction network + joint 640 + V 5 000,
bf16, beam 5 and 10 - the device walk (em_transducer_beam_search) against the host-driven route.

    python tools/transducer_beam_bench.py [--batch 32] [--seconds 10] [--beams 5,10] [--reps 5] [--warmup 1] [--out FILE.json]

Reports per beam, in one process on one GPU (median and range of `--reps` runs after `--warmup`, wall clock around the
whole call with a synchronisation before and after, since both routes read back from the device as they go):
  * device_ms   `beam_device` for the batch: lin_enc per utterance, the steps in chunks with a status read-back per chunk,
                the gathered results;
  * host_ms     `default_beam_search` utterance by utterance: one launch pair and one read-back per expansion;
  * steps_needed / steps_enqueued of the device walk, the utterances it stopped on (`fallbacks`, by status) and the most
    expansions one frame took.
Weights are the recipe initialisation (oracle.weights, seed 7) made peaked - lin_out scaled, the blank's bias raised - so
that frames end after about `beam` expansions; the flat initialisation needs hundreds per frame at beam 10 and overflows
the walk's capacities.  Both routes run under the same expansion limit per frame (the walk's capacity), so an utterance
neither can finish costs both the same number of expansions; before anything is timed the two routes are checked to
return the same label sequences and scores for every utterance the walk ended.  Inputs are the BASELINE.md waveforms.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import transducer_small  # noqa: E402


def timed(fn, reps, warmup, tag):
    for _ in range(warmup):
        fn()
    ms = []
    for i in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        print(f"[{tag}] run {i + 1}/{reps}: {ms[-1]:.1f} ms", file=sys.stderr, flush=True)
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--beams", default="5,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out-scale", type=float, default=20.0)
    ap.add_argument("--blank-up", type=float, default=24.0)
    ap.add_argument("--out", default="profiles/transducer_beam_bench.json")
    a = ap.parse_args()

    from espnet_amd.asr.transducer import beam_search_transducer as M
    from oracle.weights import synth_waveform

    V, B = a.vocab, a.batch
    model, new = transducer_small(V, 0.0)
    new["joint_network.lin_out.weight"] *= a.out_scale
    new["joint_network.lin_out.bias"][0] += a.blank_up
    model.load_state_dict(new, strict=True)
    model.cuda().eval()
    lim = M.beam_limits()
    M.MAX_EXPANSIONS_PER_FRAME = lim["expansions"]  # the same limit on both routes
    n = int(a.seconds * 16000)
    speech = torch.stack([synth_waveform(b, n) for b in range(B)]).cuda()
    lens = [n] * B
    res = dict(workload=f"{B} x {a.seconds:g} s, Conformer-small + LSTM 1x512 + joint 640 + V {V}, bf16, lin_out x "
                        f"{a.out_scale:g}, blank + {a.blank_up:g}", reps=a.reps, warmup=a.warmup, limits=lim, beams={})
    with torch.no_grad():
        st = model.encode_device(speech, lens, isolate=True)
        enc_act, olens = st.enc_act, st.olens
        res["frames"] = int(enc_act.shape[1])
        for beam in [int(v) for v in a.beams.split(",")]:
            bs = M.BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, nbest=beam)

            def host_one(b):
                try:
                    return bs.default_beam_search(enc_act[b, : olens[b]], utt=b)
                except RuntimeError:
                    return None  # (a frame not left within the limit)

            def device():
                return bs.beam_device(enc_act, olens)

            def host():
                return [host_one(b) for b in range(B)]

            got = device()
            info = bs.last_beam
            states = info["status"][:, 0].tolist()
            want = host()
            for b in range(B):
                if got[b] is None:
                    continue
                if want[b] is None or [h.yseq for h in got[b]] != [h.yseq for h in want[b]] or any(
                        abs(g.score - w.score) > 1e-9 * abs(w.score) for g, w in zip(got[b], want[b])):
                    raise SystemExit(f"beam {beam}, utterance {b}: the device walk and the host route differ")
            r = dict(steps_needed=info["needed"], steps_enqueued=info["enqueued"],
                     fallbacks=sum(1 for s in states if s != 1), fallback_states=sorted(s for s in states if s != 1),
                     host_gave_up=sum(1 for w in want if w is None),
                     most_expansions_in_a_frame=int(info["status"][:, 3].max()),
                     labels_best=sum(len(g[0].yseq) - 1 for g in got if g is not None))
            print(f"[beam {beam}] {r}", file=sys.stderr, flush=True)
            r["device_ms"] = timed(device, a.reps, a.warmup, f"beam {beam} device")
            r["host_ms"] = timed(host, a.reps, a.warmup, f"beam {beam} host")
            r["host_over_device"] = round(r["host_ms"]["median"] / r["device_ms"]["median"], 2)
            res["beams"][str(beam)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
