"""Cases and float64 reference of the mixed-radix log-mel kernel (csrc/frontend_mr.hip), numpy only; shared by
tests/test_gpu_frontend_nfft.py and tools/frontend_nfft_parity.py (which measures the bounds' CPU source).  The metric,
the log-domain set and its bound are those of tests/frontend_ref.py."""
import numpy as np
import torch

from espnet_amd import lib as L
from espnet_amd.layers.stft_plan import twiddle_table
from tests import frontend_ref as fr

# (n_fft, hop, win_length, fs): what each reaches is listed at the test
SIZES = [(256, 100, None, 8000), (400, 160, None, 16000), (400, 160, 320, 16000), (240, 80, None, 16000),
         (1024, 256, None, 16000), (972, 243, None, 16000)]

# Bound of the linear metric per n_fft: 8x the worst value of the f32 CPU pipeline (torch.stft f32 -> power -> matmul)
# against the float64 reference on these very signals, as tools/frontend_nfft_parity.py measures it without a GPU.
# Source: profiles/frontend_nfft_parity.txt.
R_CPU = {240: 7.59e-8, 256: 5.05e-8, 400: 1.90e-7, 512: 4.32e-8, 972: 4.46e-8, 1024: 4.72e-8}
R = {k: 8 * v for k, v in R_CPU.items()}


def batch(n_fft, fs):
    """(2, N) f32 and lengths: row 0 barely longer than n_fft / 2 (the reflections of both ends meet in its frames), row 1
    0.6 s of noise with an all-zero stretch of 2 n_fft samples (floor frames among valid ones)."""
    N = int(0.6 * fs) + 1
    lens = [n_fft // 2 + 7, N]
    x = np.zeros((2, N), dtype=np.float32)
    x[0, :lens[0]] = fr.signal("noise", lens[0], seed=n_fft)
    x[1] = fr.signal("noise", N, seed=n_fft + 1)
    x[1, N // 3:N // 3 + 2 * n_fft] = 0.0
    return x, lens


def logmel_f64(speech, lens, melmat, n_fft, hop, win_f32, isolate):
    """reflect pad -> frames -> window -> rfft -> power -> mel -> floor -> log -> zero the padding, as fr.LogMel."""
    x, mel = speech.astype(np.float64), np.asarray(melmat).astype(np.float64)
    w = np.zeros(n_fft)
    left = (n_fft - len(win_f32)) // 2
    w[left:left + len(win_f32)] = win_f32
    B, N = x.shape
    T_f, flens = 1 + N // hop, [n // hop + 1 for n in lens]
    out_log, out_mel = np.zeros((B, T_f, mel.shape[1])), np.zeros((B, T_f, mel.shape[1]))
    out_E, zero = np.zeros((B, T_f)), np.zeros((B, T_f), dtype=bool)
    for b in range(B):
        Nb, nv = (lens[b] if isolate else N), flens[b]
        idx = np.abs((np.arange(nv) * hop - n_fft // 2)[:, None] + np.arange(n_fft)[None, :])
        idx = np.where(idx >= Nb, 2 * (Nb - 1) - idx, idx)
        assert idx.min() >= 0 and idx.max() < N
        frames = x[b][idx]
        spec = np.fft.rfft(frames * w[None, :], axis=1)
        P = spec.real ** 2 + spec.imag ** 2
        zero[b, :nv] = ~frames.any(axis=1)
        out_mel[b, :nv], out_E[b, :nv] = P @ mel, P.sum(axis=1)
        out_log[b, :nv] = np.log(np.maximum(P @ mel, fr.FLOOR))
    return fr.LogMel(out_log, out_mel, out_E, np.asarray(flens), zero)


def logmel_nfft(fe, speech, flens_dev, wlens_dev=None, tab=None):
    """em_frontend_logmel_nfft_f32 called directly, whatever fe.n_fft is (DefaultFrontend routes 512 to its own kernel).
    tab: the twiddle table on the device, kept by the caller (a timing loop); None: built here, and the call waits."""
    pk = fe.packed(speech.device)
    own = tab is None
    if own:
        tab = torch.from_numpy(twiddle_table(fe.n_fft)).to(speech.device)
    B, N = speech.shape
    T_f = 1 + N // fe.hop_length
    feats = torch.empty(B, T_f, fe.n_mels, dtype=torch.float32, device=speech.device)
    L.check(L.load().em_frontend_logmel_nfft_f32(
        L.ptr(speech), B, N, fe.n_fft, fe.hop_length, L.ptr(pk.window), L.ptr(tab), L.ptr(pk.mel), L.ptr(pk.lo),
        pk.maxlen, fe.n_mels, L.ptr(flens_dev), L.ptr(wlens_dev), T_f, L.ptr(feats), L.current_stream_ptr()),
        "em_frontend_logmel_nfft_f32")
    if own:
        torch.cuda.current_stream().synchronize()  # (`tab` lives until the launch has run)
    return feats
