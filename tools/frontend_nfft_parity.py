"""Where the bounds of tests/test_gpu_frontend_nfft.py come from: the linear metric (tests/frontend_ref.py) of torch's
own f32 CPU pipeline (torch.stft in float32 -> power -> matmul -> clamp -> log) against the float64 reference, on the
test's signals, per n_fft; the bound is 8x the worst value.  With a GPU present, the mixed-radix kernel's worst value
per case is added.

    python tools/frontend_nfft_parity.py [--out profiles/frontend_nfft_parity.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from espnet_amd.asr.frontend.default import DefaultFrontend  # noqa: E402
from tests import frontend_nfft_ref as nr  # noqa: E402
from tests import frontend_ref as fr  # noqa: E402


def cpu_f32(fe, x, lens, isolate):
    win = torch.hann_window(fe.win_length, dtype=torch.float32)
    T_f = 1 + x.shape[1] // fe.hop_length
    out = np.zeros((x.shape[0], T_f, fe.n_mels), dtype=np.float32)
    for b in range(x.shape[0]):
        row = torch.from_numpy(x[b, :lens[b]] if isolate else x[b])
        s = torch.stft(row, fe.n_fft, fe.hop_length, fe.win_length, win, center=True, pad_mode="reflect", onesided=True,
                       return_complex=True).T
        p = s.real ** 2 + s.imag ** 2
        nv = lens[b] // fe.hop_length + 1
        out[b, :nv] = torch.log(torch.clamp(p @ fe.logmel.melmat, min=1e-10))[:nv].numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/frontend_nfft_parity.txt")
    a = ap.parse_args()
    gpu = torch.cuda.is_available()
    lines, worst_cpu = [], {}
    for n_fft, hop, win_length, fs in nr.SIZES + [(512, 160, 400, 16000)]:
        x, lens = nr.batch(n_fft, fs)
        for n_mels in (80, 23):
            fe = DefaultFrontend(fs=fs, n_fft=n_fft, win_length=win_length, hop_length=hop, n_mels=n_mels)
            mel = fe.logmel.melmat.numpy()
            win = torch.hann_window(fe.win_length, dtype=torch.float32).numpy()
            for isolate in (True, False):
                ref = nr.logmel_f64(x, lens, mel, n_fft, hop, win, isolate)
                r_cpu = fr.linear_metric(cpu_f32(fe, x, lens, isolate), ref, mel)[0].max()
                sel, valid = fr.log_set(ref, mel)
                worst_cpu[n_fft] = max(worst_cpu.get(n_fft, 0.0), r_cpu)
                line = (f"n_fft {n_fft:4d} hop {hop:3d} win {fe.win_length:4d} n_mels {n_mels:2d} wlens {str(isolate):5s} "
                        f"band {fe.packed(torch.device('cpu')).maxlen:3d}  cpu f32 r = {r_cpu:.3e}  log-set share = "
                        f"{sel.sum() / valid.sum():.3f}")
                if gpu:
                    fe.cuda()
                    fl = torch.tensor(ref.flens, dtype=torch.int32).cuda()
                    wl = torch.tensor(lens, dtype=torch.int32).cuda() if isolate else None
                    sp = torch.from_numpy(x).cuda()
                    if n_fft == 512:  # the mixed-radix kernel's direct entry (DefaultFrontend routes 512 to its own kernel)
                        got = nr.logmel_nfft(fe, sp, fl, wl)
                    else:
                        got = fe.forward_device(sp, fl, wl)
                    line += f"  MI355X r = {fr.linear_metric(got.cpu().numpy(), ref, mel)[0].max():.3e}"
                    fe.cpu()
                lines.append(line)
    head = ["linear metric r of tests/frontend_ref.py; bound of the GPU test = 8 x the worst cpu f32 r of the size", ""]
    head += [f"n_fft {k:4d}: worst cpu f32 r = {v:.3e}   bound R = {8 * v:.3e}" for k, v in sorted(worst_cpu.items())]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(head + [""] + lines) + "\n")
    print("\n".join(head + [""] + lines))


if __name__ == "__main__":
    main()
