"""The resumable greedy transducer walk on stream ticks: Conformer-small + LSTM 1 x 512 + joint 640 + V 5 000, bf16 (the
model of tools/transducer_bench.py), S = 32 and 128 streams x 16 new frames per tick.

    python tools/transducer_stream_bench.py [--reps 5] [--out profiles/transducer_stream_bench.json]

The encoder rows are the first 240 frames of 32 x 10 s utterances (S = 128: the same rows four times), fed as 15 ticks;
the blank bias is raised so that a stream emits 0 to 4 labels per tick.  Per S, medians over reps x 15 ticks (each timed
with device events around the enqueued region, a synchronisation after it, after one warm-up pass):
  * tick_ms      lin_enc on the tick's rows + the walk's rounds (`extend_start`), and lin_enc_ms alone
                 (`em_transducer_stream_enc_proj`); walk_ms is their difference;
  * readback_ms  host time of `extend_collect` once the tick has finished;
  * rounds       needed against enqueued, per tick;
  * dead_round_us  what an enqueued round behind the last needed one costs: a tick that brings ONE frame per stream in
                 a call of F = 16 (16 rounds enqueued, 1 needed) against the same in a call of F = 1, over 15.
The comparison, same process: `em_transducer_greedy` over the same 240 frames of the 32 utterances in one call, the only
transducer walk there was before (its lin_enc GEMM included), also divided by 15 for the share of one tick.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import transducer_small  # noqa: E402

F, TICKS = 16, 15


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--blank-bias", type=float, default=1.12)  # 0 to ~5 labels per stream and tick (mean 1.6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from oracle.weights import synth_waveform

    model, _ = transducer_small(a.vocab, a.blank_bias)
    dec, jn = model.decoder, model.joint_network
    bs = BeamSearchTransducer(dec, jn, beam_size=1)
    n = 10 * 16000
    res = dict(workload=f"Conformer-small + LSTM 1x512 + joint 640 + V {a.vocab}, bf16; {TICKS} ticks x {F} frames", reps=a.reps)
    with torch.no_grad():
        speech = torch.stack([synth_waveform(b, n) for b in range(32)]).cuda()
        enc32 = model.encode_device(speech, [n] * 32, isolate=True).enc_act[:, : F * TICKS].contiguous()
        assert enc32.shape[1] == F * TICKS
        ol = torch.full((32,), F * TICKS, dtype=torch.int32).cuda()
        for _ in range(2):
            bs.greedy_device(enc32, ol)
        one = [event_ms(lambda: bs.greedy_device(enc32, ol))[0] for _ in range(4 * a.reps)]
        res["one_shot_240_frames_32_utts_ms"] = dict(median=round(statistics.median(one), 4), min=round(min(one), 4),
                                                     max=round(max(one), 4), per_16_frames=round(statistics.median(one) / TICKS, 4))
        lib, w, pj = L.load(), dec.weights("cuda")[0], jn.packed("cuda")
        for S in (32, 128):
            enc = enc32.repeat(S // 32, 1, 1)
            tick_ms, enc_ms, rb_ms, needed, labels = [], [], [], [], []
            proj = torch.empty(S, F, w.jp, device="cuda")
            for rep in range(a.reps + 1):  # (pass 0: warm-up)
                state = bs.stream_state(S, "cuda")
                for k in range(TICKS):
                    x = enc[:, k * F : (k + 1) * F].contiguous()
                    ms, tick = event_ms(lambda: bs.extend_start(state, list(range(S)), x, [F] * S))
                    t0 = time.perf_counter()
                    hyps = bs.extend_collect(tick)
                    rb = (time.perf_counter() - t0) * 1e3
                    e_ms, _ = event_ms(lambda: L.check(lib.em_transducer_stream_enc_proj(
                        dec.em_dtype, L.ptr(x), C.c_void_p(pj.lin_enc.data_ptr()), C.c_void_p(pj.enc_b.data_ptr()), S * F,
                        int(x.shape[2]), w.jp, L.ptr(proj), L.current_stream_ptr())))
                    if rep:
                        tick_ms.append(ms), enc_ms.append(e_ms), rb_ms.append(rb), needed.append(bs.last_rounds["needed"])
                labels = [len(h.yseq) - 1 for h in hyps]
            # a dead round's cost: one frame per stream, 16 rounds enqueued against 1
            state = bs.stream_state(S, "cuda")
            x16, x1 = enc[:, :F].contiguous(), enc[:, :1].contiguous()
            wide = [event_ms(lambda: bs.extend_start(state, list(range(S)), x16, [1] * S))[0] for _ in range(12)][2:]
            slim = [event_ms(lambda: bs.extend_start(state, list(range(S)), x1, [1] * S))[0] for _ in range(12)][2:]
            med = statistics.median
            res[f"S{S}"] = dict(tick_ms=dict(median=round(med(tick_ms), 4), min=round(min(tick_ms), 4), max=round(max(tick_ms), 4)),
                                lin_enc_ms=round(med(enc_ms), 4), walk_ms=round(med(tick_ms) - med(enc_ms), 4),
                                readback_ms=round(med(rb_ms), 4), rounds_needed=dict(median=med(needed), min=min(needed), max=max(needed)),
                                rounds_enqueued=F, labels_per_stream_per_tick=round(sum(labels) / len(labels) / TICKS, 2),
                                dead_round_us=round((med(wide) - med(slim)) / (F - 1) * 1e3, 2))
        t32 = res["S32"]["tick_ms"]["median"]
        res["tick_faster_than_one_shot_share"] = bool(t32 < res["one_shot_240_frames_32_utts_ms"]["per_16_frames"])
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
