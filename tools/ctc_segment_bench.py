"""CTC segmentation (csrc/ctc_segment.hip) on synthetic peaked posteriors at V 5 000, two sizes: one long recording,
1 x (T 90 000, C ~ 45 000, W 8 192: an hour at 40 ms frames), and a batch of 8 x (T 7 500, C ~ 3 000: five minutes each).

    python tools/ctc_segment_bench.py [--reps 20] [--warmup 3] [--out profiles/ctc_segment_bench.json] [--shapes long,batch]

Reports per size, in one process on one GPU (medians with min and max of `--reps` runs after `--warmup`; device legs timed
with device events around the enqueued region and a synchronisation after it):
  * trellis_ms         the `em_ctc_segment` launch alone on a ready lpT, outputs and workspace allocated once;
  * logp_trellis_ms    `CTC.segment_device`: the ctc_lo GEMM + log-softmax + transpose (`em_ctc_log_probs_t`) and the trellis,
                       from a random bf16 encoder output of d = 256 (the posteriors of this leg are NOT peaked: the time of
                       neither kernel depends on the values beyond the number of band slides, and nothing of it is checked);
  * host_route_ms      the route that exists without this kernel: the D2H copy of the (T, V) log-probs (`d2h_ms`) plus the
                       vectorised NumPy restatement on the host (`numpy_ms`; tests/ctc_segment_ref.py, float32, one run,
                       host clock).  This is a NumPy loop over the frames, NOT the ctc_segmentation package's Cython loop,
                       which was not at hand.
Before anything is timed the device result is compared with that host run: paths, t_end and status equal, total and
frame_lp bit-equal.  Every leg is reported as measured, a losing one too."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import summary  # noqa: E402

SHAPES = {"long": dict(B=1, T=90000, C=45000, K=1500, pre=1500, post=2500, W=8192),
          "batch": dict(B=8, T=7500, C=3000, K=100, pre=100, post=200, W=8192)}


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
    return summary(ms)


def planted(seed, T, C, K, pre, post, V, blank=0, peak=12.0):
    """tests/ctc_segment_ref.py's planted case at scale, the (T, V) table made on the device: (lp (T, V) f32 cuda, gt)."""
    from tests.ctc_segment_ref import build_gt

    rng = np.random.default_rng(seed)
    N = C - 2 - K
    cuts = np.sort(rng.choice(np.arange(1, N), K - 1, replace=False))
    toks = rng.integers(1, V, N)
    utts = [u.tolist() for u in np.split(toks, cuts)]
    gt, begin = build_gt(utts, blank)
    assert len(gt) == C
    col_onsets = pre + np.sort(rng.choice(T - pre - post, C - 1, replace=False))
    is_tok = np.ones(C, bool)
    is_tok[[0] + begin] = False
    onsets = torch.from_numpy(col_onsets[is_tok[1:]]).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T, V, device="cuda", generator=g)
    x[pre:T - post, blank] += peak
    x[onsets, blank] -= peak
    x[onsets, torch.from_numpy(toks).cuda()] += peak
    noise = torch.cat([torch.arange(pre), torch.arange(T - post, T)]).cuda()
    x[noise, torch.from_numpy(rng.integers(1, V, noise.numel())).cuda()] += peak
    for s in range(0, T, 8192):
        x[s:s + 8192] = torch.log_softmax(x[s:s + 8192], dim=-1)
    return x, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--shapes", default="long,batch")
    ap.add_argument("--no-host", action="store_true", help="skip the host route (and with it the check)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_segment_bench: no GPU (a timing needs the device)")

    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC
    from tests.ctc_segment_ref import segment_ref

    lib, V = L.load(), a.vocab
    res = dict(bench="ctc_segment", vocab=V, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               host_route="D2H of the (T, V) log-probs + the vectorised NumPy restatement (a NumPy loop over the frames, "
                          "not the ctc_segmentation package's Cython loop)", shapes={})
    for name in a.shapes.split(","):
        s = SHAPES[name]
        B, T, C, W = s["B"], s["T"], s["C"], s["W"]
        cases = [planted(100 * b + 7, T, C, s["K"], s["pre"], s["post"], V) for b in range(B)]
        lpT = torch.empty(V, B * T, dtype=torch.float32, device="cuda")
        for b, (lp, _) in enumerate(cases):
            lpT[:, b * T:(b + 1) * T] = lp.t()
        gt_d = torch.tensor([gt for _, gt in cases], dtype=torch.int32).cuda()
        xl = torch.full((B,), T, dtype=torch.int32).cuda()
        cl = torch.full((B,), C, dtype=torch.int32).cuda()
        ws_bytes = int(lib.em_ctc_segment_workspace_bytes(B, T, C, W))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
        ff = torch.empty(B, C, dtype=torch.int32, device="cuda")
        fc, fl = torch.empty(B, T, dtype=torch.int32, device="cuda"), torch.empty(B, T, dtype=torch.float32, device="cuda")
        te, st = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        tot = torch.empty(B, dtype=torch.float32, device="cuda")

        def trellis():
            L.check(lib.em_ctc_segment(L.ptr(lpT), B * T, L.ptr(xl), L.ptr(gt_d), C, L.ptr(cl), B, T, 0, W, 1, L.ptr(ff), L.ptr(fc),
                                       L.ptr(fl), L.ptr(te), L.ptr(tot), L.ptr(st), L.ptr(ws), ws_bytes, L.current_stream_ptr()),
                    "em_ctc_segment")

        trellis()
        torch.cuda.synchronize()
        out = dict(B=B, T=T, C=C, W=min(W, C), workspace_bytes=ws_bytes, status=st.cpu().tolist(), t_end=te.cpu().tolist())
        if not a.no_host:
            d2h, npy = 0.0, 0.0
            for b, (lp, gt) in enumerate(cases):
                t0 = time.perf_counter()
                lp_h = lp.cpu().numpy()
                t1 = time.perf_counter()
                r = segment_ref(lp_h, gt, 0, W, 1, np.float32, margin=False)
                t2 = time.perf_counter()
                d2h, npy = d2h + (t1 - t0) * 1e3, npy + (t2 - t1) * 1e3
                same = (np.array_equal(ff[b].cpu().numpy(), r["first_frame"]) and np.array_equal(fc[b].cpu().numpy(), r["frame_col"])
                        and fl[b].cpu().numpy().tobytes() == r["frame_lp"].tobytes() and int(te[b]) == r["t_end"]
                        and int(st[b]) == r["status"] and np.float32(tot[b].item()).tobytes() == np.float32(r["total"]).tobytes())
                if not same:
                    raise SystemExit(f"ctc_segment_bench: {name} recording {b}: the device and the host restatement disagree")
                del lp_h
            out.update(checked_against_host=True, d2h_ms=round(d2h, 1), numpy_ms=round(npy, 1), host_route_ms=round(d2h + npy, 1),
                       host_route_runs=1)
        del cases
        out["trellis_ms"] = timed(trellis, a.reps, a.warmup)
        ctc = CTC(V, 256, compute_dtype="bfloat16").cuda()
        enc = torch.randn(B, T, 256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(torch.bfloat16)
        out["logp_trellis_ms"] = timed(lambda: ctc.segment_device(enc, xl, gt_d, cl, 0, W), a.reps, a.warmup)
        out["ms_per_1000_frames"] = round(out["trellis_ms"]["median"] / T * 1000, 4)
        res["shapes"][name] = out
        print(f"[ctc_segment_bench] {name}: {json.dumps(out)}", flush=True)
        del lpT, ws, enc
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
