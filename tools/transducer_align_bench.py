"""Transducer forced alignment at the shape of tools/transducer_nll_bench.py: Conformer-small + LSTM 1 x 512 prediction network
+ joint 640 + V 5 000, bf16; 64 candidates of 40-80 tokens, eight per utterance, over 8 encoder outputs of T = 249 frames.

    python tools/transducer_align_bench.py [--reps 20] [--warmup 3] [--out profiles/transducer_align_bench.json]

Reports, in one process on one GPU and on ONE lattice (medians with min and max of `--reps` runs after `--warmup`; device
legs timed with device events around the enqueued region and a synchronisation after it; the two legs of a pair are run
alternately, so both see the same clocks and neighbours):
  * align_ms / nll_ms            em_transducer_seq_align against em_transducer_seq_nll: the same loads and barriers, a max in
                                 place of expf / log1pf, plus the back-pointer stores and the back-trace (per launch, `--inner`
                                 launches enqueued back to back per run);
  * whole_align_ms / whole_nll_ms  ESPnetASRModel.transducer_align against transducer_nll: checks, copies of the ids, enc_proj,
                                 the prediction network, the lattice launch and the recursion;
  * host_route_ms                the only route before: a D2H copy of the lattice and the numpy / Python Viterbi of the
                                 restatement (tests/transducer_align_ref.py), host clock, 3 runs (`host_route_runs`);
  * long_align_ms / long_nll_ms  the long form, one candidate of T 15 000 x U 1 000 on a random lattice, the launches alone.
Before anything is timed the alignment is checked against the restatement on the device's own lattice: every total within
(T_b + U) * 2^-23 * max(1, |total|) of the float64 optimum.  Every leg is reported as measured, a losing one too.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import summary, transducer_candidates, transducer_small  # noqa: E402


def timed_pair(fa, fb, reps, warmup, inner=1):
    """fa and fb alternately, each run between its own pair of device events.  `inner`: launches enqueued back to back per
    run, the time divided by their number - for a launch of tens of microseconds, which the host cannot enqueue faster
    than the device retires it when each run holds only one."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for fn, ms in zip((fa, fb), out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / inner)
    return summary(out[0]), summary(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--per-utt", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--long-frames", type=int, default=15000)
    ap.add_argument("--long-tokens", type=int, default=1000)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed run of the align / nll pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transducer_align_bench: no GPU (a timing needs the device)")

    from espnet_amd import lib as L
    from oracle.weights import synth_waveform
    from tests.transducer_align_ref import viterbi

    V, B, N = a.vocab, a.utts, a.utts * a.per_utt
    model, _ = transducer_small(V)
    dec, jn = model.decoder, model.joint_network
    n_samples = int(a.seconds * 16000)
    speech = torch.stack([synth_waveform(b, n_samples) for b in range(B)]).cuda()
    g, ylens, ys, mem_of = transducer_candidates(N, V, a.per_utt)
    Lmax = int(ys.shape[1])
    with torch.no_grad():
        st = model.encode_device(speech, [n_samples] * B, isolate=True)
        enc_act, T = st.enc_act, int(st.enc_act.shape[1])
        olens = torch.tensor(st.olens)
        xl = olens.to(torch.int32).cuda()
        yl, mo, tg = ylens.to(torch.int32).cuda(), mem_of.to(torch.int32).cuda(), ys.to(torch.int32).cuda()
        enc_proj = jn.enc_proj_device(enc_act)
        dec_proj = dec.teacher_forced_proj(tg, yl)
        lat = jn.lattice_logp_device(dec, enc_proj, xl, dec_proj, tg, yl, mo)
        ws = torch.empty(int(L.load().em_transducer_seq_align_workspace_bytes(N, T, Lmax)), dtype=torch.uint8, device="cuda")

        def align():
            return jn.seq_align_device(lat, xl, yl, mo, ws=ws)

        def nll():
            return jn.seq_nll_device(lat, xl, yl, mo)

        def whole_align():
            return model.transducer_align(enc_act, olens, ys, ylens, mem_of=mem_of)

        def whole_nll():
            return model.transducer_nll(enc_act, olens, ys, ylens, mem_of=mem_of)

        def host_route():
            host = lat.cpu()
            return [viterbi(host[n], int(olens[int(mem_of[n])]), int(ylens[n])) for n in range(N)]

        # the check before any timing: the device against the restatement on the device's own lattice
        tok_frame, tok_logp, frame_u, total = (o.cpu() for o in align())
        whole = [o.cpu() for o in whole_align()]
        want = host_route()
        nll_host = nll().cpu()
        same_path = 0
        for n in range(N):
            tb, U = int(olens[int(mem_of[n])]), int(ylens[n])
            tot, best = float(total[n]), want[n]["total"]
            bound = (tb + U) * 2.0 ** -23 * max(1.0, abs(tot))
            if not abs(tot - best) <= bound or not tot <= -float(nll_host[n]) + bound:
                raise SystemExit(f"transducer_align_bench: candidate {n}: total {tot}, float64 optimum {best}, -nll {-float(nll_host[n])}")
            same_path += tok_frame[n, :U].tolist() == want[n]["tok_frame"]
        if not all(torch.equal(x, y) for x, y in zip(whole, (tok_frame, tok_logp, frame_u, total))):
            raise SystemExit("transducer_align_bench: the launch and the whole call disagree")
        res = dict(workload=f"{N} candidates of 40-80 tokens (Lmax {Lmax}), {a.per_utt} per utterance, over {B} x T {T}; "
                            f"Conformer-small + LSTM 1x512 + joint 640 + V {V}, bf16",
                   paths_equal_to_float64=f"{same_path} of {N}", lattice_bytes=int(lat.numel() * 4),
                   workspace_bytes=int(ws.numel()), reps=a.reps, warmup=a.warmup)
        res["align_ms"], res["nll_ms"] = timed_pair(align, nll, a.reps, a.warmup, inner=a.inner)
        res["whole_align_ms"], res["whole_nll_ms"] = timed_pair(whole_align, whole_nll, a.reps, a.warmup)
        host_ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        res["host_route_ms"] = summary(host_ms)
        res["host_route_runs"] = len(host_ms)  # (its own count, after the one run of the check above; host clock)
        res["align_over_nll"] = round(res["align_ms"]["median"] / res["nll_ms"]["median"], 3)
        res["whole_align_over_whole_nll"] = round(res["whole_align_ms"]["median"] / res["whole_nll_ms"]["median"], 3)
        res["host_route_over_whole_align"] = round(res["host_route_ms"]["median"] / res["whole_align_ms"]["median"], 1)
        # the long form: one candidate, a random lattice of honest two-way splits (log p, log(1 - p))
        LT, LU = a.long_frames, a.long_tokens
        pr = torch.rand(1, LT, LU + 1, generator=g).clamp(0.01, 0.99).cuda()
        long_lat = torch.stack([torch.log(pr), torch.log1p(-pr)], -1).contiguous()
        long_lat[:, :, LU, 1] = float("-inf")
        lxl, lyl = torch.tensor([LT], dtype=torch.int32).cuda(), torch.tensor([LU], dtype=torch.int32).cuda()
        lws = torch.empty(int(L.load().em_transducer_seq_align_workspace_bytes(1, LT, LU)), dtype=torch.uint8, device="cuda")
        long_tot = float(jn.seq_align_device(long_lat, lxl, lyl, ws=lws)[3].cpu())
        long_nll = float(jn.seq_nll_device(long_lat, lxl, lyl).cpu())
        if not (long_tot <= -long_nll and long_tot > float("-inf")):
            raise SystemExit(f"transducer_align_bench: long form total {long_tot} against -nll {-long_nll}")
        res["long_form"] = f"1 x (T {LT}, U {LU}), random lattice, {int(long_lat.numel() * 4)} bytes, workspace {int(lws.numel())} bytes"
        res["long_align_ms"], res["long_nll_ms"] = timed_pair(lambda: jn.seq_align_device(long_lat, lxl, lyl, ws=lws),
                                                              lambda: jn.seq_nll_device(long_lat, lxl, lyl),
                                                              max(3, a.reps // 4), 1)
        res["long_align_over_nll"] = round(res["long_align_ms"]["median"] / res["long_nll_ms"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
