"""CTC token posteriors on the device (csrc/ctc_post.hip, csrc/ctc_post_renorm.hip): forward-backward for a ragged batch
of candidates, as f32 logarithms and renormalised.

    python tools/ctc_post_bench.py [--reps 20] [--warmup 3] [--out profiles/ctc_post_bench.json]

The two shapes of tools/ctc_nll_bench.py, in one process on one GPU (medians with min and max of `--reps` runs after
`--warmup`, each run timed with device events around the enqueued region and a synchronisation after it; the host route
by the wall clock, one run):
  * n-best: 8 utterances of T = 249 frames, V 5 000, 64 candidates of 40-80 tokens, eight per utterance through mem_of;
  * long form: 1 x (T 15 000, L 3 000), V 5 000 (S above 4 096: the three-walk form of the kernel).
Per shape:
  * post_ms     em_ctc_seq_posteriors alone on ready lpT, outputs and workspace allocated once per call of the wrapper;
  * renorm_ms   em_ctc_seq_posteriors_renorm on the same inputs, timed the same way;
  * alpha_ms    em_ctc_seq_nll on the same inputs: the alpha pass alone;
  * host_ms     D2H of the utterances' (T, V) log-probs + the float64 NumPy forward-backward (tests/ctc_post_ref.py).
Beside every device leg stands what its result is worth: the largest absolute error of occ, peak and blank_post against
the float64 pass (`max_abs_err`), taken before anything is timed.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed  # noqa: E402


def shape(name, lpT, Bm, T, olens, tg, ylens, mem_of, a):
    """lpT (V, Bm*T) f32 cuda; olens / ylens / mem_of host lists, tg (N, Lmax) host int tensor."""
    from espnet_amd import lib as EL
    from espnet_amd.asr.ctc import CTC
    from tests.ctc_post_ref import ctc_post_ref

    N, Lm = len(ylens), int(tg.shape[1])
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()  # noqa: E731
    ol_d, yl_d, mo_d, tg_d = i32(olens), i32(ylens), i32(mem_of), tg.to(torch.int32).cuda()
    post = lambda **kw: CTC.posteriors_log_probs_t(lpT, Bm * T, ol_d, Bm, T, tg_d, Lm, yl_d, mo_d, N, 0, **kw)  # noqa: E731
    renorm = lambda **kw: post(renorm=True, **kw)  # noqa: E731
    alpha = lambda: CTC.nll_log_probs_t(lpT, Bm * T, ol_d, Bm, T, tg_d, Lm, yl_d, mo_d, N, 0)  # noqa: E731

    def host():
        lp = lpT.cpu().numpy()  # the D2H copy
        return [ctc_post_ref(lp[:, u * T : u * T + olens[u]].T, tg[n, : ylens[n]].tolist()) for n, u in enumerate(mem_of)]

    t0 = time.perf_counter()
    want = host()
    host_ms = (time.perf_counter() - t0) * 1e3

    def worth(route):
        """Largest absolute error of occ, peak and blank_post of a device route against float64."""
        nll, occ, peak, _, bp = [o.cpu().numpy() for o in route(blank_post=True)]
        if not np.isfinite(nll).all() or not np.isfinite(occ).all():
            raise SystemExit(f"ctc_post_bench: {name}: a value that is not finite")
        err = max(max(float(np.abs(occ[n, : ylens[n]] - w[2]).max()), float(np.abs(peak[n, : ylens[n]] - w[3]).max()),
                      float(np.abs(bp[n, : len(w[5])] - w[5]).max())) for n, w in enumerate(want))
        return float(nll.mean()), err

    # (reported, not a threshold: the plain route's alpha and beta are f32 logarithms of magnitude |nll|, and these flat
    # synthetic posteriors cost ~8 nats per frame - at |nll| ~ 1e5 it resolves gamma no longer)
    (mean_nll, err), (_, err_rn) = worth(post), worth(renorm)
    lib = EL.load()
    r = dict(candidates=N, Lmax=Lm, utterances=Bm, T=T, mean_nll=round(mean_nll, 2), max_abs_err=dict(post=err, renorm=err_rn),
             workspace_bytes=int(lib.em_ctc_seq_posteriors_workspace_bytes(N, T, Lm)),
             renorm_workspace_bytes=int(lib.em_ctc_seq_posteriors_renorm_workspace_bytes(N, T, Lm)),
             log_probs_bytes=int(lpT.numel()) * 4)
    r["post_ms"] = timed(post, a.reps, a.warmup)
    r["renorm_ms"] = timed(renorm, a.reps, a.warmup)
    r["alpha_ms"] = timed(alpha, a.reps, a.warmup)
    r["host_ms"] = round(host_ms, 1)
    r["post_over_alpha"] = round(r["post_ms"]["median"] / r["alpha_ms"]["median"], 2)
    r["renorm_over_post"] = round(r["renorm_ms"]["median"] / r["post_ms"]["median"], 2)
    print(f"[ctc_post_bench] {name}: {json.dumps(r)}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_post_bench: no GPU (a timing needs the device)")
    V = a.vocab
    g = torch.Generator().manual_seed(7)
    res = dict(bench="ctc_post", vocab=V, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0), shapes={})
    with torch.no_grad():
        Bm, T, per, N = 8, 249, 8, 64
        lp = torch.log_softmax(torch.randn(Bm * T, V, generator=g).cuda() * 3.0, dim=-1)
        olens = torch.randint(T // 2, T + 1, (Bm,), generator=g).tolist()
        olens[0] = T
        ylens = torch.randint(40, 81, (N,), generator=g).tolist()
        tg = torch.randint(1, V - 1, (N, max(ylens)), generator=g)
        res["shapes"]["nbest"] = shape("nbest", lp.t().contiguous(), Bm, T, olens, tg, ylens, [n // per for n in range(N)], a)
        del lp
        T, L = 15000, 3000
        lp = torch.log_softmax(torch.randn(T, V, generator=g).cuda() * 3.0, dim=-1)
        tg = torch.randint(1, V - 1, (1, L), generator=g)
        res["shapes"]["long_form"] = shape("long_form", lp.t().contiguous(), 1, T, [T], tg, [L], [0], a)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
