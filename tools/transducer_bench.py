"""Transducer greedy decoding, 32 x 10 s: Conformer-small encoder + LSTM 1 x 512 prediction network + joint 640 + V 5 000, bf16.

    python tools/transducer_bench.py [--batch 32] [--seconds 10] [--reps 20] [--warmup 3] [--out FILE.json]

Reports, in one process on one GPU (medians of `--reps` runs after `--warmup`, each run timed with device events around
the whole enqueued region and a synchronisation after it):
  * walk_fused_ms      em_transducer_greedy for the batch (enc_proj GEMM + the walk; the encoder is outside);
  * walk_host_loop_ms  the same walk driven from the host through em_transducer_dec_step / em_transducer_joint_logp, with
                       an arg-max read-back per frame (what a per-step scorer interface costs);
  * walk_torch_ms      a batched eager-torch restatement on the same GPU (bf16 matmuls, LSTMCell, one read-back per frame);
  * end_to_end         waveform -> hypotheses through Speech2Text-equivalent calls (encode_device + search_batch), audio-s/s;
  * launches_per_frame of the fused walk.
Weights are the recipe initialisation (oracle.weights, seed 7) with the blank bias raised so that roughly one frame in
four emits a label; inputs are the BASELINE.md waveforms.  The three walks are checked to emit the same number of
labels within 2 % (near-ties of a flat softmax may differ between them) before anything is timed.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import transducer_small  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--blank-bias", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from oracle.weights import synth_waveform

    V, B = a.vocab, a.batch
    model, new = transducer_small(V, a.blank_bias)
    dec, jn = model.decoder, model.joint_network
    bs = BeamSearchTransducer(dec, jn, beam_size=1)
    n = int(a.seconds * 16000)
    speech = torch.stack([synth_waveform(b, n) for b in range(B)]).cuda()
    lens = [n] * B
    with torch.no_grad():
        st = model.encode_device(speech, lens, isolate=True)
        enc_act, olens = st.enc_act, st.olens
        T = int(enc_act.shape[1])
        ol = torch.tensor(olens, dtype=torch.int32).cuda()

        def fused():
            return bs.greedy_device(enc_act, ol)

        def host_loop():
            enc_proj = jn.enc_proj_device(enc_act)
            tok = torch.zeros(B, dtype=torch.int32, device="cuda")
            o, q, s = dec.step_device(tok, dec.init_state(B, "cuda"))
            count = 0
            for t in range(T):
                pred = torch.argmax(jn.logp_device(dec, enc_proj[:, t].contiguous(), q), 1).to(torch.int32)
                mask = (pred != 0).to(torch.int32)
                count += int(mask.sum())  # the read-back of the frame
                o, q, s = dec.step_device(pred, s, mask=mask, out=(o, q))
            return count

        # eager torch on the same weights
        bf = torch.bfloat16
        emb = new["decoder.embed.weight"].cuda().to(bf)
        w_ih, w_hh = (new[f"decoder.decoder.0.weight_{k}_l0"].cuda().to(bf) for k in ("ih", "hh"))
        bias = (new["decoder.decoder.0.bias_ih_l0"] + new["decoder.decoder.0.bias_hh_l0"]).cuda()
        w_enc, b_enc = new["joint_network.lin_enc.weight"].cuda().to(bf), new["joint_network.lin_enc.bias"].cuda()
        w_dec = new["joint_network.lin_dec.weight"].cuda().to(bf)
        w_out, b_out = new["joint_network.lin_out.weight"].cuda().to(bf), new["joint_network.lin_out.bias"].cuda()

        def torch_cell(tok, h, c):
            g = (emb[tok] @ w_ih.T + h.to(bf) @ w_hh.T).float() + bias
            i, f, gg, o = g.chunk(4, 1)
            c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            return torch.sigmoid(o) * torch.tanh(c2), c2

        def torch_loop():
            enc_proj = (enc_act @ w_enc.T).float() + b_enc
            h = c = torch.zeros(B, 512, device="cuda")
            h, c = torch_cell(torch.zeros(B, dtype=torch.long, device="cuda"), h, c)
            dp = (h.to(bf) @ w_dec.T).float()
            count = 0
            for t in range(T):
                logits = (torch.tanh(enc_proj[:, t] + dp).to(bf) @ w_out.T).float() + b_out
                pred = torch.argmax(torch.log_softmax(logits, 1), 1)
                m = pred != 0
                count += int(m.sum())  # the read-back of the frame
                h2, c2 = torch_cell(pred, h, c)
                h, c = torch.where(m[:, None], h2, h), torch.where(m[:, None], c2, c)
                dp = (h.to(bf) @ w_dec.T).float()
            return count

        def end_to_end():
            s = model.encode_device(speech, lens, isolate=True)
            return bs.search_batch(s.enc_act, s.olens)

        n_fused = int(fused()[1].sum())
        n_host, n_torch = host_loop(), torch_loop()
        for name, v in (("host loop", n_host), ("torch", n_torch)):
            if abs(v - n_fused) > 0.02 * max(n_fused, 1):
                raise SystemExit(f"label counts differ: fused {n_fused}, {name} {v}")
        res = dict(workload=f"{B} x {a.seconds:g} s, Conformer-small + LSTM 1x512 + joint 640 + V {V}, bf16", frames=T,
                   labels_emitted=n_fused, launches_per_frame=4, reps=a.reps, warmup=a.warmup)
        for name, fn, reps in (("walk_fused_ms", fused, a.reps), ("walk_host_loop_ms", host_loop, max(3, a.reps // 4)),
                               ("walk_torch_ms", torch_loop, max(3, a.reps // 4)), ("end_to_end_ms", end_to_end, a.reps)):
            med, lo, hi = timed(fn, reps, a.warmup if reps == a.reps else 1)
            res[name] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        res["end_to_end_audio_s_per_s"] = round(B * a.seconds / (res["end_to_end_ms"]["median"] / 1e3), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
