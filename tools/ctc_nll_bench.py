"""Scoring transcripts with CTC on the device (csrc/ctc_nll.hip): the forward trellis for a ragged batch of candidates.

    python tools/ctc_nll_bench.py [--reps 20] [--warmup 3] [--out profiles/ctc_nll_bench.json]

Two shapes, in one process on one GPU (medians with min and max of `--reps` runs after `--warmup`, each run timed with
device events around the enqueued region and a synchronisation after it; the host route by the wall clock):
  * n-best: the log-probs of 8 utterances of T = 249 frames (d 512 -> V 5 000, bf16 head), 64 candidates of 40-80 tokens,
    eight per utterance through mem_of;
  * long form: 1 x (T 15 000, L 3 000), V 5 000.
Per shape:
  * trellis_ms     em_ctc_seq_nll alone on ready lpT;
  * full_ms        CTC.nll_device: the ctc_lo GEMM, the transposed log-softmax and the trellis (n-best shape only);
  * torch_loss_ms  torch.nn.functional.ctc_loss in eager torch on the same GPU from ready (B, T, V) log-probs: it wants
                   (T, N, V), so the eight-fold replication of every utterance's log-probs is part of the route;
  * torch_full_ms  CTC.log_softmax + that (n-best shape only);
  * host_ms        the (B, T, V) log-probs copied to the host, replicated there, CPU ctc_loss.
The routes are checked to give the same nll before anything is timed.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed  # noqa: E402


def timed_wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def torch_loss(lp_btv, mem_of, tg, olens, ylens):
    """(B, T, V) log-probs -> (N,) by torch's ctc_loss, on whatever device the arguments live."""
    lp = lp_btv.transpose(0, 1)[:, mem_of]  # (T, N, V): every utterance once per candidate
    return torch.nn.functional.ctc_loss(lp, tg, olens[mem_of], ylens, blank=0, reduction="none", zero_infinity=False)


def agree(a, b, what):
    err = float(((a.double() - b.double()).abs() / b.double().abs().clamp(min=1.0)).max())
    if not err <= 1e-4 or not torch.isfinite(a).all():
        raise SystemExit(f"the routes disagree ({what}): {err}")
    return err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_nll_bench: no GPU (a timing needs the device)")

    from espnet_amd.asr.ctc import CTC

    V, D = a.vocab, 512
    g = torch.Generator().manual_seed(7)
    res = dict(reps=a.reps, warmup=a.warmup)

    with torch.no_grad():
        # ---- n-best shape
        Bm, T, per, N = 8, 249, 8, 64
        ctc = CTC(V, D, compute_dtype="bfloat16")
        ctc.ctc_lo.weight.copy_(torch.randn(V, D, generator=g) * (3.0 / D ** 0.5))
        ctc.ctc_lo.bias.copy_(0.1 * torch.randn(V, generator=g))
        ctc.cuda().eval()
        enc = torch.randn(Bm, T, D, generator=g).to(torch.bfloat16).cuda()
        olens = torch.randint(T // 2, T + 1, (Bm,), generator=g)
        olens[0] = T
        ylens = torch.randint(40, 81, (N,), generator=g)
        Lm = int(ylens.max())
        tg = torch.randint(1, V - 1, (N, Lm), generator=g)
        mem_of = torch.arange(N) // per
        olens_d, ylens_d = olens.to(torch.int32).cuda(), ylens.to(torch.int32).cuda()
        tg_d, mo_d = tg.to(torch.int32).cuda(), mem_of.to(torch.int32).cuda()
        tg_l, mo_l, olens_l, ylens_l = tg.cuda(), mem_of.cuda(), olens.cuda(), ylens.cuda()

        full = lambda: ctc.nll_device(enc, olens_d, tg_d, ylens_d, 0, mem_of=mo_d)  # noqa: E731
        lp = ctc.log_softmax(enc)  # (Bm, T, V) f32
        lpT = lp.permute(2, 0, 1).reshape(V, Bm * T).contiguous()
        trellis = lambda: CTC.nll_log_probs_t(lpT, Bm * T, olens_d, Bm, T, tg_d, Lm, ylens_d, mo_d, N, 0)  # noqa: E731
        t_loss = lambda: torch_loss(lp, mo_l, tg_l, olens_l, ylens_l)  # noqa: E731
        t_full = lambda: torch_loss(ctc.log_softmax(enc), mo_l, tg_l, olens_l, ylens_l)  # noqa: E731
        host = lambda: torch_loss(lp.cpu(), mem_of, tg, olens, ylens)  # noqa: E731
        ref = t_loss()
        diff = dict(trellis_vs_torch=agree(trellis(), ref, "trellis"), full_vs_torch=agree(full(), ref, "full"),
                    host_vs_torch=agree(host().cuda(), ref, "host"))
        r = dict(workload=f"{N} candidates of 40-80 tokens (Lmax {Lm}), {per} per utterance; {Bm} utterances of up to {T} "
                          f"frames, d {D}, V {V}, bf16 head", mean_nll=round(float(ref.mean()), 3), max_rel_diff=diff)
        r["trellis_ms"] = timed(trellis, a.reps, a.warmup)
        r["full_ms"] = timed(full, a.reps, a.warmup)
        r["torch_loss_ms"] = timed(t_loss, a.reps, a.warmup)
        r["torch_full_ms"] = timed(t_full, a.reps, a.warmup)
        r["host_ms"] = timed_wall(host, max(3, a.reps // 4), 1)
        r["log_probs_bytes"] = Bm * T * V * 4
        r["torch_loss_over_trellis"] = round(r["torch_loss_ms"]["median"] / r["trellis_ms"]["median"], 2)
        r["torch_full_over_full"] = round(r["torch_full_ms"]["median"] / r["full_ms"]["median"], 2)
        res["nbest"] = r
        del lp, lpT, enc

        # ---- long form
        T, L = 15000, 3000
        lp = torch.log_softmax(torch.randn(T, V, generator=g).cuda() * 3.0, dim=-1).unsqueeze(0)  # (1, T, V)
        lpT = lp[0].t().contiguous()
        tg = torch.randint(1, V - 1, (1, L), generator=g)
        one = torch.ones(1, dtype=torch.int32)
        olens_d, ylens_d, tg_d = (one * T).cuda(), (one * L).cuda(), tg.to(torch.int32).cuda()
        zero, olens, ylens = torch.zeros(1, dtype=torch.long), torch.tensor([T]), torch.tensor([L])
        tg_l, zero_l, olens_l, ylens_l = tg.cuda(), zero.cuda(), olens.cuda(), ylens.cuda()
        trellis = lambda: CTC.nll_log_probs_t(lpT, T, olens_d, 1, T, tg_d, L, ylens_d, None, 1, 0)  # noqa: E731
        t_loss = lambda: torch_loss(lp, zero_l, tg_l, olens_l, ylens_l)  # noqa: E731
        host = lambda: torch_loss(lp.cpu(), zero, tg, olens, ylens)  # noqa: E731
        ref = t_loss()
        diff = dict(trellis_vs_torch=agree(trellis(), ref, "long trellis"), host_vs_torch=agree(host().cuda(), ref, "long host"))
        r = dict(workload=f"1 x (T {T}, L {L}), V {V}", nll=round(float(ref[0]), 2), max_rel_diff=diff)
        r["trellis_ms"] = timed(trellis, a.reps, a.warmup)
        r["torch_loss_ms"] = timed(t_loss, max(3, a.reps // 4), 1)
        r["host_ms"] = timed_wall(host, 3, 1)
        r["log_probs_bytes"] = T * V * 4
        r["torch_loss_over_trellis"] = round(r["torch_loss_ms"]["median"] / r["trellis_ms"]["median"], 2)
        res["long_form"] = r

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
