"""Per-launch time of the mixed-radix log-mel kernel (csrc/frontend_mr.hip) on 32 x 10 s at 16 kHz:

    n_fft 400 / hop 160, n_fft 1024 / hop 256                     the new sizes (80 filters; 1024 also with 23 filters,
                                                                  whose 116-tap bands take the global-memory mel path)
    n_fft 512 / hop 160 through the new kernel and through em_frontend_logmel_f32   the cost of generality
    torch.stft + matmul + log on the same GPU                     the outside comparison, per size

HIP events around `--iters` launches after `--warmup`, the legs alternating over `--rounds` rounds in one process;
the median and the spread of the per-round means are reported.  Needs an MI355X: no GPU, no number.

    python tools/frontend_nfft_bench.py [--out profiles/frontend_nfft_bench.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from espnet_amd.asr.frontend.default import DefaultFrontend  # noqa: E402
from espnet_amd.layers.stft_plan import twiddle_table  # noqa: E402
from tests.frontend_nfft_ref import logmel_nfft  # noqa: E402  (the direct call of the C entry)


def torch_logmel(fe, speech, win):
    s = torch.stft(speech, fe.n_fft, fe.hop_length, fe.win_length, win, center=True, pad_mode="reflect", onesided=True,
                   return_complex=True).transpose(1, 2)
    return torch.log(torch.clamp((s.real ** 2 + s.imag ** 2) @ fe.logmel.melmat, min=1e-10))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/frontend_nfft_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    B, N = 32, 160000
    g = torch.Generator().manual_seed(5)
    speech = (0.1 * torch.randn(B, N, generator=g)).cuda()
    legs = {}
    for n_fft, hop, win_length, n_mels in ((400, 160, 400, 80), (1024, 256, 1024, 80), (1024, 256, 1024, 23),
                                           (512, 160, 400, 80)):
        fe = DefaultFrontend(n_fft=n_fft, win_length=win_length, hop_length=hop, n_mels=n_mels).cuda()
        fl = torch.tensor(fe.feature_lengths([N] * B), dtype=torch.int32).cuda()
        win = torch.hann_window(win_length, dtype=torch.float32).cuda()
        tab = torch.from_numpy(twiddle_table(n_fft)).cuda()
        if n_mels == 23:  # bands of 116 taps: the mel weights from global memory (ML = 0)
            legs["n_fft1024_hop256_23mels_mixed_radix"] = lambda fe=fe, fl=fl, tab=tab: logmel_nfft(fe, speech, fl, tab=tab)
            continue
        legs[f"n_fft{n_fft}_hop{hop}_mixed_radix"] = lambda fe=fe, fl=fl, tab=tab: logmel_nfft(fe, speech, fl, tab=tab)
        if n_fft == 512:
            legs["n_fft512_hop160_em_frontend_logmel_f32"] = lambda fe=fe, fl=fl: fe.forward_device(speech, fl)
        legs[f"n_fft{n_fft}_hop{hop}_torch_stft_matmul_log"] = lambda fe=fe, win=win: torch_logmel(fe, speech, win)
    ref = legs["n_fft512_hop160_em_frontend_logmel_f32"]().cpu()
    diff = (legs["n_fft512_hop160_mixed_radix"]().cpu() - ref).abs().max().item()
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            per_round[k].append(timed(fn, a.iters))
    res = {"what": "us per launch, 32 x 10 s at 16 kHz, n_mels 80 unless named, f32; HIP events around `iters` launches, legs alternating "
                   "over `rounds` rounds; median (min .. max) of the round means",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
           "n_fft512_max_abs_log_diff_mixed_radix_vs_em_frontend_logmel_f32": diff,
           "legs": {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                    for k, v in per_round.items()}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
