"""Host side of the mixed-radix STFT kernel (csrc/frontend_mr.hip): which sizes it takes, the radix plan of a size, and
the twiddle table the kernel reads, built in float64 and rounded to f32 once.

The packed real FFT of n_fft points is an H = n_fft / 2 point complex Stockham FFT followed by an untangling step.
Stage s (radix r, p = product of the radices before it) multiplies input q of butterfly i by W_{rp}^{kq}, k = i mod p.
Table layout, in complex entries: stage s at offset p - 1 as [q - 1][k] (r - 1 rows of p; H - 1 entries over all
stages), entry H - 1 unused, then W_{n_fft}^k for k = 0 .. H at offset H: 2 H + 1 entries.
"""
import numpy as np

N_FFT_RULE = "n_fft even, 64 <= n_fft <= 1024, n_fft / 2 with no prime factor other than 2, 3 and 5"


def radix_plan(n_fft: int):
    """The radices in stage order (4s, then one 2, then 3s, then 5s), or None for a size the kernel does not take.  At most
    six stages (972 = 2 * 2 * 3^5; every other size has five or fewer).  The launcher derives the same plan
    (em_stft_radix_plan); tests/test_cpu_frontend_nfft.py compares the two on every size."""
    if n_fft != int(n_fft) or n_fft < 64 or n_fft > 1024 or n_fft % 2:
        return None
    h, e = int(n_fft) // 2, {}
    for f in (2, 3, 5):
        e[f] = 0
        while h % f == 0:
            h, e[f] = h // f, e[f] + 1
    if h != 1:
        return None
    return [4] * (e[2] // 2) + [2] * (e[2] % 2) + [3] * e[3] + [5] * e[5]


def twiddle_table(n_fft: int, dtype=np.float32) -> np.ndarray:
    """(2 H + 1, 2) `dtype`: (re, im) of the entries described in the module docstring, computed in float64 and rounded
    once (float32 is what the kernel gets; float64 is the same table before the rounding)."""
    plan = radix_plan(n_fft)
    assert plan is not None, n_fft
    H = n_fft // 2
    tab = np.zeros(2 * H + 1, dtype=np.complex128)
    p = 1
    for r in plan:
        k = np.arange(p, dtype=np.float64)[None, :]
        q = np.arange(1, r, dtype=np.float64)[:, None]
        tab[p - 1:p - 1 + (r - 1) * p] = np.exp(-2j * np.pi * (k * q) / (r * p)).reshape(-1)
        p *= r
    assert p == H
    tab[H:] = np.exp(-2j * np.pi * np.arange(H + 1, dtype=np.float64) / n_fft)
    return np.stack([tab.real, tab.imag], axis=1).astype(dtype)
