"""Transducer default beam search with a fused language model, 32 x 10 s: the workload of tools/transducer_beam_bench.py
(Conformer-small encoder + LSTM 1 x 512 prediction network + joint 640 + V 5 000, bf16, peaked weights, beam 5 and 10)
with a SequentialRNNLM lstm 2 x 650 at lm_weight 0.3.

    python tools/transducer_beam_lm_bench.py [--batch 32] [--seconds 10] [--beams 5,10] [--reps 5] [--warmup 1] [--out FILE.json]

Reports per beam, in one process on one GPU (median and range of `--reps` runs after `--warmup`, wall clock around the
whole call with a synchronisation before and after; the host route's warm-up run is the run of the check below):
  * device_lm_ms  `beam_device` with the LM (em_transducer_beam_search_lm);
  * device_ms     `beam_device` without it, in the same process: the capability before the LM was fused;
  * host_lm_ms    `default_beam_search` with the LM utterance by utterance, under the same expansion limit per frame;
  * us_per_step_lm / us_per_step: the two device times over the steps each walk enqueued, and their difference - what
    the LM's `nlayers + 1` launches (the head streams V x d_lm weights) add to one step.
The LM changes which hypotheses are expanded, so the two walks take different numbers of steps; both counts are
reported.  Before anything is timed the walk with the LM is checked against the host route with the LM for every
utterance the walk ended.  Weights: the recipe initialisation (oracle.weights, seed 7; the LM seed 8), the transducer made
peaked as in tools/transducer_beam_bench.py.  Inputs are the BASELINE.md waveforms.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import transducer_small  # noqa: E402
from tools.transducer_beam_bench import timed  # noqa: E402


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
    ap.add_argument("--lm-unit", type=int, default=650)
    ap.add_argument("--lm-layers", type=int, default=2)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--out", default="profiles/transducer_beam_lm_bench.json")
    a = ap.parse_args()

    from espnet_amd.asr.transducer import beam_search_transducer as M
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from oracle.weights import recipe_state_dict, synth_waveform

    V, B = a.vocab, a.batch
    model, new = transducer_small(V, 0.0)
    new["joint_network.lin_out.weight"] *= a.out_scale
    new["joint_network.lin_out.bias"][0] += a.blank_up
    model.load_state_dict(new, strict=True)
    model.cuda().eval()
    lm = SequentialRNNLM(V, unit=a.lm_unit, nlayers=a.lm_layers, rnn_type="lstm", compute_dtype=model.decoder.compute_dtype)
    lm.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in lm.state_dict().items()}, 8), strict=True)
    lm.cuda().eval()
    lim = M.beam_limits()
    M.MAX_EXPANSIONS_PER_FRAME = lim["expansions"]  # the same limit on both routes
    n = int(a.seconds * 16000)
    speech = torch.stack([synth_waveform(b, n) for b in range(B)]).cuda()
    lens = [n] * B
    res = dict(workload=f"{B} x {a.seconds:g} s, Conformer-small + LSTM 1x512 + joint 640 + V {V}, bf16, lin_out x "
                        f"{a.out_scale:g}, blank + {a.blank_up:g}; LM lstm {a.lm_layers} x {a.lm_unit}, lm_weight "
                        f"{a.lm_weight:g}", reps=a.reps, warmup=a.warmup, limits=lim, beams={})
    with torch.no_grad():
        st = model.encode_device(speech, lens, isolate=True)
        enc_act, olens = st.enc_act, st.olens
        res["frames"] = int(enc_act.shape[1])
        for beam in [int(v) for v in a.beams.split(",")]:
            bs = M.BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, nbest=beam, lm=lm,
                                        lm_weight=a.lm_weight)
            bs0 = M.BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, nbest=beam)

            def host_one(b):
                try:
                    return bs.default_beam_search(enc_act[b, : olens[b]], utt=b)
                except RuntimeError:
                    return None  # (a frame not left within the limit)

            def device_lm():
                return bs.beam_device(enc_act, olens)

            def device():
                return bs0.beam_device(enc_act, olens)

            def host_lm():
                return [host_one(b) for b in range(B)]

            got = device_lm()
            info = bs.last_beam
            states = info["status"][:, 0].tolist()
            want = host_lm()
            for b in range(B):
                if got[b] is None:
                    continue
                if want[b] is None or [h.yseq for h in got[b]] != [h.yseq for h in want[b]] or any(
                        abs(g.score - w.score) > 1e-9 * abs(w.score) for g, w in zip(got[b], want[b])):
                    raise SystemExit(f"beam {beam}, utterance {b}: the device walk and the host route differ")
            got0 = device()
            info0 = bs0.last_beam
            r = dict(steps_needed_lm=info["needed"], steps_enqueued_lm=info["enqueued"],
                     steps_needed=info0["needed"], steps_enqueued=info0["enqueued"],
                     fallbacks_lm=sum(1 for s in states if s != 1),
                     fallbacks=sum(1 for s in info0["status"][:, 0].tolist() if s != 1),
                     host_gave_up=sum(1 for w in want if w is None),
                     most_expansions_in_a_frame_lm=int(info["status"][:, 3].max()),
                     best_changed_by_lm=sum(1 for g, g0 in zip(got, got0)
                                            if g is not None and g0 is not None and g[0].yseq != g0[0].yseq))
            print(f"[beam {beam}] {r}", file=sys.stderr, flush=True)
            r["device_lm_ms"] = timed(device_lm, a.reps, a.warmup, f"beam {beam} device+lm")
            r["device_ms"] = timed(device, a.reps, a.warmup, f"beam {beam} device")
            r["host_lm_ms"] = timed(host_lm, a.reps, 0,  # (the check above was its warm-up run)
                                    f"beam {beam} host+lm")
            r["us_per_step_lm"] = round(1e3 * r["device_lm_ms"]["median"] / r["steps_enqueued_lm"], 2)
            r["us_per_step"] = round(1e3 * r["device_ms"]["median"] / r["steps_enqueued"], 2)
            r["us_per_step_added"] = round(r["us_per_step_lm"] - r["us_per_step"], 2)
            r["host_lm_over_device_lm"] = round(r["host_lm_ms"]["median"] / r["device_lm_ms"]["median"], 2)
            res["beams"][str(beam)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
