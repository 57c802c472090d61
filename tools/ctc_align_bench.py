#!/usr/bin/env python3
"""Time CTC forced alignment on the device (csrc/ctc_align.hip): the trellis launch alone (`em_ctc_forced_align` on a
ready lpT, outputs and workspace allocated once), and log-probs + trellis (`CTC.forced_align_device`: the ctc_lo GEMM,
the transposed log-softmax and the trellis, from encoder activations), in one process, alternating, medians over rounds.

Shapes: 32 x (T = 249, L = 60) and 32 x (T = 249, L = 120) with a 256 -> 5 000 CTC head in bf16 on random activations;
1 x (T = 3 000, L = 700) and 1 x (T = 15 000, L = 3 000) on synthetic lpT (log-softmax of normal logits, V = 5 000).

With --cpu also the same alignment the way it is done without this kernel, on the same machine: (B, T, V) f32
log-probs copied to the host, then the frame loop of tests/ctc_align_ref.py per utterance (one run each: it takes
seconds); its frame labels are compared with the device's.  One JSON line per shape.

    python tools/ctc_align_bench.py [--iters 50] [--rounds 5] [--warmup 10] [--cpu] [--shapes 0,1,2,3]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed_host as timed  # noqa: E402
from espnet_amd import lib as L  # noqa: E402
from espnet_amd.asr.ctc import CTC  # noqa: E402

V, D = 5000, 256
SHAPES = [dict(B=32, T=249, L=60, head=True), dict(B=32, T=249, L=120, head=True),
          dict(B=1, T=3000, L=700, head=False), dict(B=1, T=15000, L=3000, head=False)]


def targets(B, Lmax, jitter, seed):
    g = torch.Generator().manual_seed(seed)
    ylens = (Lmax - torch.randint(0, jitter + 1, (B,), generator=g)).to(torch.int32)
    ylens[0] = Lmax
    return torch.randint(1, V - 1, (B, Lmax), generator=g).to(torch.int32), ylens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu", action="store_true", help="also the host route: log-probs D2H + the CPU frame loop")
    ap.add_argument("--shapes", default="0,1,2,3")
    a = ap.parse_args()
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    ctc = CTC(V, D, compute_dtype="bfloat16")
    with torch.no_grad():
        ctc.ctc_lo.weight.copy_(torch.randn(V, D, generator=g) * 0.2)
        ctc.ctc_lo.bias.copy_(torch.randn(V, generator=g) * 0.1)
    ctc = ctc.cuda().eval()
    for k in [int(s) for s in a.shapes.split(",")]:
        sh = SHAPES[k]
        B, T, Lm = sh["B"], sh["T"], sh["L"]
        tg, ylens = targets(B, Lm, Lm // 6 if B > 1 else 0, 10 + k)
        tg_d, ylens_d = tg.cuda(), ylens.cuda()
        olens_d = torch.full((B,), T, dtype=torch.int32).cuda()
        lpT = torch.empty(V, B * T, dtype=torch.float32, device="cuda")
        if sh["head"]:
            enc = (torch.randn(B, T, D, generator=g)).cuda().to(ctc.act_dtype)
            p = ctc.packed(enc.device)
            L.check(lib.em_ctc_log_probs_t(ctc.em_dtype, L.ptr(enc), B, T, D, L.ptr(p.weight), L.ptr(p.bias), V, L.ptr(lpT),
                                           L.current_stream_ptr()), "em_ctc_log_probs_t")
        else:
            enc = None
            lpT.copy_(torch.log_softmax(torch.randn(T, V, generator=g).cuda(), dim=-1).t())
        ws_bytes = int(lib.em_ctc_forced_align_workspace_bytes(B, T, Lm))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
        o = [torch.empty(B, T, dtype=torch.int32, device="cuda"), torch.empty(B, T, device="cuda"),
             torch.empty(B, Lm, dtype=torch.int32, device="cuda"), torch.empty(B, Lm, dtype=torch.int32, device="cuda"),
             torch.empty(B, Lm, device="cuda"), torch.empty(B, device="cuda")]

        def trellis():
            L.check(lib.em_ctc_forced_align(L.ptr(lpT), B * T, L.ptr(olens_d), L.ptr(tg_d), Lm, L.ptr(ylens_d), B, T, 0,
                                            L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.ptr(o[4]), L.ptr(o[5]),
                                            L.ptr(ws), ws_bytes, L.current_stream_ptr()), "em_ctc_forced_align")

        def with_log_probs():
            return ctc.forced_align_device(enc, olens_d, tg_d, ylens_d, 0)

        legs = [("trellis_ms", trellis)] + ([("log_probs_and_trellis_ms", with_log_probs)] if enc is not None else [])
        iters = a.iters if T <= 1000 else max(3, a.iters // 10)
        ms = {name: [] for name, _ in legs}
        for _ in range(a.rounds):  # alternating: every leg once per round
            for name, fn in legs:
                ms[name].append(timed(fn, iters, min(a.warmup, iters)))
        rec = dict(B=B, T=T, L=Lm, V=V, waves=(2 * Lm + 1 + 511) // 512, workspace_bytes=ws_bytes, iters=iters, rounds=a.rounds)
        for name, _ in legs:
            rec[name] = round(statistics.median(ms[name]), 4)
            rec[name + "_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        total = o[5].cpu()
        rec["feasible_rows"] = int(torch.isfinite(total).sum())
        if a.cpu:
            from tests.ctc_align_ref import forced_align_ref

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp_host = (ctc.log_softmax(enc.float()) if enc is not None else lpT.t().reshape(B, T, V).contiguous()).cpu()
            t1 = time.perf_counter()
            refs = [forced_align_ref(lp_host[b], tg[b, : int(ylens[b])].tolist(), 0) for b in range(B)]
            t2 = time.perf_counter()
            rec["host_route_log_probs_d2h_ms"] = round((t1 - t0) * 1e3, 2)
            rec["host_route_cpu_loop_ms"] = round((t2 - t1) * 1e3, 2)
            rec["host_route_mbytes"] = round(lp_host.numel() * 4 / 1e6, 1)
            if enc is None:  # (same lpT on both sides: the paths must be equal; with the head the log-softmax kernels differ)
                rec["labels_equal"] = all(torch.equal(o[0][b].cpu(), refs[b]["align"]) for b in range(B))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
