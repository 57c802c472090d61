"""Host side of the mixed-radix STFT frontend (espnet_amd/layers/stft_plan.py, DefaultFrontend) without a GPU: which
n_fft the constructor takes, and the radix plan with its twiddle table applied in numpy float64."""
import numpy as np
import pytest
import torch

from espnet_amd.asr.frontend.default import DefaultFrontend
from espnet_amd.layers.stft_plan import radix_plan, twiddle_table


@pytest.mark.parametrize("n_fft", [1022, 401, 2048])
def test_unsupported_n_fft_is_refused(n_fft):
    with pytest.raises(NotImplementedError, match="n_fft"):
        DefaultFrontend(n_fft=n_fft, hop_length=160)


@pytest.mark.parametrize("n_fft", [400, 256, 1024, 512])
def test_supported_n_fft_constructs(n_fft):
    fe = DefaultFrontend(n_fft=n_fft, hop_length=n_fft // 4)
    assert tuple(fe.logmel.melmat.shape) == (n_fft // 2 + 1, 80)
    pk = fe.packed(torch.device("cpu"))
    assert pk.window.numel() == n_fft
    if n_fft == 512:
        assert pk.plan is None
    else:
        assert tuple(pk.plan.shape) == (n_fft + 1, 2) and pk.plan.dtype == torch.float32


def test_python_and_c_radix_rules_agree_on_every_size():
    """The constructor's rule (stft_plan.radix_plan) and the launcher's (em_stft_radix_plan): a size one takes and the
    other refuses would build a model whose first forward fails."""
    import ctypes

    from espnet_amd import lib as L

    radix = (ctypes.c_int32 * 8)()
    for n_fft in range(0, 1100):
        ns = L.load().em_stft_radix_plan(n_fft, radix)
        assert (list(radix[:ns]) if ns else None) == radix_plan(n_fft), n_fft
        assert ns <= 6


def stockham(z, plan, tab):
    """The kernel's stages (csrc/frontend_mr.hip) on an H-point complex vector, reading the twiddles from the table the
    kernel gets: butterfly i of stage (r, p) takes in[i + (H / r) q] W_{rp}^{kq}, k = i mod p, and writes DFT_r of
    them to out[(i - k) r + k + q' p]."""
    H, p = len(z), 1
    for r in plan:
        m = H // r
        i = np.arange(m)
        k = i % p
        u = np.stack([z[i + m * q] * (1.0 if q == 0 else tab[p - 1 + (q - 1) * p + k]) for q in range(r)])
        y = np.exp(-2j * np.pi * np.outer(np.arange(r), np.arange(r)) / r) @ u
        out = np.empty_like(z)
        for q in range(r):
            out[(i - k) * r + k + q * p] = y[q]
        z, p = out, p * r
    assert p == H
    return z


@pytest.mark.parametrize("n_fft,radices", [(256, [4, 4, 4, 2]), (400, [4, 2, 5, 5]), (240, [4, 2, 3, 5]),
                                           (1024, [4, 4, 4, 4, 2]), (972, [2, 3, 3, 3, 3, 3])])
def test_host_plan_reproduces_fft(n_fft, radices):
    plan = radix_plan(n_fft)
    assert plan == radices
    H = n_fft // 2
    # the table before its one rounding to f32 (the kernel's is exactly its rounding): the plan and the indexing, to 1e-12
    k = np.arange(H + 1)
    tab = twiddle_table(n_fft, np.float64)
    assert np.array_equal(twiddle_table(n_fft), tab.astype(np.float32)) and tab.shape == (n_fft + 1, 2)
    tab = tab[:, 0] + 1j * tab[:, 1]
    rng = np.random.default_rng(n_fft)
    x = rng.standard_normal(n_fft)
    z = stockham(x[0::2] + 1j * x[1::2], plan, tab)
    ref = np.fft.fft(x[0::2] + 1j * x[1::2])
    assert np.abs(z - ref).max() <= 1e-12 * np.abs(ref).max()
    # the untangling step with the table's second half: bins 0 .. H of the real transform
    zc = np.conj(z[(H - k) % H])
    zk = z[k % H]
    X = 0.5 * (zk + zc) + tab[H:] * (-0.5j) * (zk - zc)
    ref = np.fft.rfft(x)
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
