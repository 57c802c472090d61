"""Scoring transcripts with a transducer: Conformer-small + LSTM 1 x 512 prediction network + joint 640 + V 5 000, bf16 (the
model of tools/transducer_bench.py): 64 candidates of 40-80 tokens, eight per utterance, over 8 encoder outputs of T = 249
frames (10 s of audio).

    python tools/transducer_nll_bench.py [--reps 10] [--warmup 2] [--out profiles/transducer_nll_bench.json]

Reports, in one process on one GPU (medians with min and max of `--reps` runs after `--warmup`, each run timed with device
events around the enqueued region and a synchronisation after it):
  * pred_net_ms      TransducerDecoder.teacher_forced_proj: Lmax + 1 enqueued em_transducer_dec_step calls over all candidates;
  * lattice_ms       em_transducer_lattice_logp over the ~10^6 valid lattice nodes, with the share of the bf16 MFMA peak
                     (2 500 TFLOP/s) that 2 * nodes * jp * V FLOP in that time are;
  * recursion_ms     em_transducer_seq_nll;
  * whole_call_ms    ESPnetASRModel.transducer_nll: the checks, the copies of the ids, enc_proj and the three legs;
  * joint_logp_route_ms  the route possible before: em_transducer_joint_logp over the same nodes in chunks (the [chunk][V]
                     log-softmax in memory), a gather of the two wanted columns, a per-diagonal torch recursion;
  * torch_route_ms   eager torch, candidate by candidate (the broadcast joint of the whole batch, ~19 GB in f32, does not fit
                     the habit of one call), the same recursion.
The three routes are checked to agree on nll (bf16 round-off apart) before anything is timed.  Every leg is reported as
measured, a losing one too.  Weights are the recipe initialisation (oracle.weights, seed 7); the encoder outputs come from
the encoder on the BASELINE.md waveforms.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed, transducer_candidates, transducer_small  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0


def torch_recursion(lat, tb, U):
    """The forward recursion one anti-diagonal at a time in eager torch: lat (N, T, L1, 2), tb / U (N,) long."""
    N, T, L1, _ = lat.shape
    dev = lat.device
    ninf = torch.tensor(float("-inf"), device=dev)
    u = torch.arange(L1, device=dev)
    D = T + L1 - 1
    t = torch.arange(D, device=dev)[:, None] - u  # (D, L1)
    b, e = lat[..., 0], lat[..., 1]
    bsk = torch.where(t >= 1, b[:, (t - 1).clamp(0, T - 1), u], ninf)  # (N, D, L1): b[t-1][u]
    esk = torch.where((t >= 0) & (t < T) & (u >= 1), e[:, t.clamp(0, T - 1), (u - 1).clamp(min=0)], ninf)  # e[t][u-1]
    inside = (t[None] >= 0) & (t[None] < tb[:, None, None]) & (u[None, None] <= U[:, None, None])
    alpha = torch.full((N, L1), float("-inf"), device=dev)
    for d in range(D):
        left = torch.cat([alpha.new_full((N, 1), float("-inf")), alpha[:, :-1]], 1)
        new = torch.logaddexp(alpha + bsk[:, d], left + esk[:, d])
        if d == 0:
            new[:, 0] = 0.0
        alpha = torch.where(inside[:, d], new, alpha)
    n = torch.arange(N, device=dev)
    return -(alpha[n, U] + b[n, (tb - 1).clamp(min=0), U])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--per-utt", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transducer_nll_bench: no GPU (a timing needs the device)")

    from oracle.weights import synth_waveform

    V, B, N = a.vocab, a.utts, a.utts * a.per_utt
    model, new = transducer_small(V)
    dec, jn = model.decoder, model.joint_network
    J = jn.joint_space_size
    n_samples = int(a.seconds * 16000)
    speech = torch.stack([synth_waveform(b, n_samples) for b in range(B)]).cuda()
    _, ylens, ys, mem_of = transducer_candidates(N, V, a.per_utt)
    Lmax = int(ys.shape[1])
    bf = torch.bfloat16
    with torch.no_grad():
        st = model.encode_device(speech, [n_samples] * B, isolate=True)
        enc_act, T = st.enc_act, int(st.enc_act.shape[1])
        olens = torch.tensor(st.olens)
        xl = olens.to(torch.int32).cuda()
        yl, mo, tg = ylens.to(torch.int32).cuda(), mem_of.to(torch.int32).cuda(), ys.to(torch.int32).cuda()
        tb_c, U_c = olens[mem_of].cuda(), ylens.cuda()
        nodes = int((olens[mem_of] * (ylens + 1)).sum())
        enc_proj = jn.enc_proj_device(enc_act)
        jp = int(enc_proj.shape[-1])
        dec_proj = dec.teacher_forced_proj(tg, yl)
        lat = torch.empty(N, T, Lmax + 1, 2, dtype=torch.float32, device="cuda")
        ws = torch.empty(jn.lattice_workspace_bytes(dec, "cuda", N, T, Lmax), dtype=torch.uint8, device="cuda")

        def pred_net():
            return dec.teacher_forced_proj(tg, yl)

        def lattice():
            return jn.lattice_logp_device(dec, enc_proj, xl, dec_proj, tg, yl, mo, out=lat, ws=ws)

        def recursion():
            return jn.seq_nll_device(lat, xl, yl, mo)

        def whole():
            return model.transducer_nll(enc_act, olens, ys, ylens, mem_of=mem_of)

        # the nodes of every candidate as (enc row, dec row, lattice position) lists for the routes possible before
        idx_e, idx_d, idx_lat, idx_lab = [], [], [], []
        for n in range(N):
            m, tb, U = int(mem_of[n]), int(olens[int(mem_of[n])]), int(ylens[n])
            t = torch.arange(tb).repeat_interleave(U + 1)
            u = torch.arange(U + 1).repeat(tb)
            idx_e.append(m * T + t)
            idx_d.append(u * N + n)
            idx_lat.append((n * T + t) * (Lmax + 1) + u)
            idx_lab.append(torch.where(u < U, ys[n][u.clamp(max=max(U - 1, 0))], torch.zeros_like(u)))
        idx_e, idx_d = torch.cat(idx_e).to(torch.int32).cuda(), torch.cat(idx_d).to(torch.int32).cuda()
        idx_lat, idx_lab = torch.cat(idx_lat).cuda(), torch.cat(idx_lab).cuda()
        last = torch.cat([torch.arange(int(olens[int(mem_of[n])]) * (int(ylens[n]) + 1)) % (int(ylens[n]) + 1) == int(ylens[n])
                          for n in range(N)]).cuda()
        ep_rows, dp_rows = enc_proj.view(-1, jp), dec_proj.view(-1, jp)

        def joint_logp_route():
            out = torch.empty(N * T * (Lmax + 1), 2, device="cuda")
            for s in range(0, nodes, a.chunk):
                e = min(s + a.chunk, nodes)
                logp = jn.logp_device(dec, ep_rows, dp_rows, idx_e[s:e], idx_d[s:e])
                two = torch.stack([logp[:, 0], logp.gather(1, idx_lab[s:e, None])[:, 0]], 1)
                two[:, 1] = torch.where(last[s:e], torch.full_like(two[:, 1], float("-inf")), two[:, 1])
                out[idx_lat[s:e]] = two
            return torch_recursion(out.view(N, T, Lmax + 1, 2), tb_c, U_c)

        w_out, b_out = new["joint_network.lin_out.weight"].cuda().to(bf), new["joint_network.lin_out.bias"].cuda()

        def torch_route():
            out = torch.full((N, T, Lmax + 1, 2), float("-inf"), device="cuda")
            for n in range(N):
                m, tb, U = int(mem_of[n]), int(olens[int(mem_of[n])]), int(ylens[n])
                z = torch.tanh(enc_proj[m, :tb, None, :J] + dec_proj[None, : U + 1, n, :J]).to(bf)  # (tb, U + 1, J)
                logp = torch.log_softmax((z @ w_out.T).float() + b_out, -1)
                out[n, :tb, : U + 1, 0] = logp[..., 0]
                if U:
                    out[n, :tb, :U, 1] = logp[:, :U].gather(2, ys[n, :U].cuda().view(1, U, 1).expand(tb, U, 1))[..., 0]
            return torch_recursion(out, tb_c, U_c)

        lattice()
        n_new, n_whole = recursion(), whole()
        n_joint, n_torch = joint_logp_route(), torch_route()
        if not torch.isfinite(n_new).all() or not torch.equal(n_new, n_whole):
            raise SystemExit("transducer_nll_bench: the legs and the whole call disagree")
        per = (olens[mem_of] + ylens).float().cuda()  # terms of a path
        diff = dict(new_vs_joint_logp=float(((n_new - n_joint).abs() / per).max()),
                    new_vs_torch=float(((n_new - n_torch).abs() / per).max()))
        if max(diff.values()) > 0.02:
            raise SystemExit(f"the routes disagree: {diff}")
        res = dict(workload=f"{N} candidates of 40-80 tokens (Lmax {Lmax}), {a.per_utt} per utterance, over {B} x T {T}; "
                            f"{nodes} valid lattice nodes of {N * T * (Lmax + 1)}; Conformer-small + LSTM 1x512 + joint 640 "
                            f"(jp {jp}) + V {V}, bf16",
                   mean_nll_per_term=round(float((n_new / per).mean()), 4), max_abs_diff_per_term=diff, reps=a.reps,
                   warmup=a.warmup)
        res["pred_net_ms"] = timed(pred_net, a.reps, a.warmup)
        res["lattice_ms"] = timed(lattice, a.reps, a.warmup)
        res["recursion_ms"] = timed(recursion, a.reps, a.warmup)
        res["whole_call_ms"] = timed(whole, a.reps, a.warmup)
        res["joint_logp_route_ms"] = timed(joint_logp_route, max(2, a.reps // 5), 1)
        res["torch_route_ms"] = timed(torch_route, max(2, a.reps // 5), 1)
        flop = 2.0 * nodes * jp * V
        res["lattice_tflops"] = round(flop / (res["lattice_ms"]["median"] * 1e-3) / 1e12, 1)
        res["lattice_fraction_of_bf16_mfma_peak"] = round(res["lattice_tflops"] / PEAK_BF16_TFLOPS, 4)
        res["joint_logp_route_over_whole"] = round(res["joint_logp_route_ms"]["median"] / res["whole_call_ms"]["median"], 2)
        res["torch_route_over_whole"] = round(res["torch_route_ms"]["median"] / res["whole_call_ms"]["median"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
