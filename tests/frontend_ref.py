"""Float64 restatement of the frontend kernels (csrc/frontend.hip), numpy only, and the case list that the CPU and the
GPU parity tests share (tests/test_cpu_frontend_ref.py, tests/test_gpu_frontend.py).

  logmel_f64        reflect pad -> frames -> window -> rfft(512) -> power -> mel -> floor -> log -> zero the padding
  utt_mvn_f64       espnet2/layers/utterance_mvn.py:45-88 (means only)
  global_mvn_f64    espnet2/layers/global_mvn.py:71-100
  frontend_variant  which kernel / template instantiation / mel tail em_frontend_logmel_f32 takes for a shape
  synthetic_melmat  banded filter matrices with chosen band positions and widths (one_hot_melmat: one unit tap each)
  signal, CASES     the test signals (built in f64, rounded to f32 once) and the shapes of the GPU test

All inputs are taken as the float32 values the device sees, widened to float64: the kernel and the reference start from
the same numbers, so what the parity tests measure is the kernel's arithmetic and nothing else.
"""
import math
from collections import namedtuple

import numpy as np

N_FFT = 512
N_BINS = 257
FLOOR = 1e-10  # log_mel.py:72 clamp(min=1e-10)
EPS32 = float(np.finfo(np.float32).eps)

# The linear-domain bound of the GPU test (metric `r`, see linear_metric).  R_CPU is the worst r of the f32 CPU
# pipeline (torch.stft in f32 -> power -> matmul -> clamp -> log) over every case below, as measured by
# tests/test_cpu_frontend_ref.py::test_tolerance_source and recorded in profiles/frontend_f64_parity.txt; the GPU
# bound is 8x that (a radix-4 Stockham FFT sums in another order, logf may differ in its last bit) and may never
# exceed 1e-5.  It is not derived from anything the kernel returns.
R_CPU = 1.74e-7
R = 8 * R_CPU
R_MAX = 1e-5
LOG_SET = 1e-2  # the log-domain check applies where e_ref >= LOG_SET * wmax * E


def stft_frame_lengths(lens, hop):
    """stft.py:108-115 with center=True: (n + 2 * 256 - 512) // hop + 1."""
    return [int(n) // hop + 1 for n in lens]


def hann_periodic(win_length):
    n = np.arange(win_length, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * math.pi * n / win_length)


def window_padded(win_length, window):
    """`window`: "hann" (periodic Hann in f64), None (all ones), or the win_length values themselves (e.g. the f32
    window the device holds).  Zero padded to 512 with left = (512 - win_length) // 2 (torch.stft)."""
    if window is None:
        w = np.ones(win_length, dtype=np.float64)
    elif isinstance(window, str):
        assert window == "hann", window
        w = hann_periodic(win_length)
    else:
        w = np.asarray(window, dtype=np.float64)
        assert w.shape == (win_length,), w.shape
    out = np.zeros(N_FFT, dtype=np.float64)
    left = (N_FFT - win_length) // 2
    out[left:left + win_length] = w
    return out


LogMel = namedtuple("LogMel", "logmel mel power_sum flens frames_zero")


def logmel_f64(speech_f32, lens, melmat_f32, win_length=None, hop=160, window="hann", isolate=False):
    """speech (B, N) f32, lens (B,) sample counts, melmat (257, n_mels) f32.  Returns LogMel with
      logmel (B, T_f, n_mels)  log(max(power @ melmat, 1e-10)), frames t >= flens[b] set to 0
      mel    (B, T_f, n_mels)  the linear mel energies before the floor (0 on the padded frames)
      power_sum (B, T_f)       E[b, t] = sum_k P[b, t, k] (0 on the padded frames)
      flens  (B,)              stft_frame_lengths
      frames_zero (B, T_f)     True where a valid frame's 512 reflected samples are all zero
    Reflection is at the padded row length N or, with `isolate`, at each utterance's own length."""
    x = np.asarray(speech_f32)
    assert x.dtype == np.float32 and x.ndim == 2, (x.dtype, x.shape)
    mel = np.asarray(melmat_f32)
    assert mel.dtype == np.float32 and mel.shape[0] == N_BINS, (mel.dtype, mel.shape)
    x, mel = x.astype(np.float64), mel.astype(np.float64)
    win_length = N_FFT if win_length is None else win_length
    w = window_padded(win_length, window)
    B, N = x.shape
    T_f = 1 + N // hop
    flens = stft_frame_lengths(lens, hop)
    n_mels = mel.shape[1]
    out_log = np.zeros((B, T_f, n_mels))
    out_mel = np.zeros((B, T_f, n_mels))
    out_E = np.zeros((B, T_f))
    zero = np.zeros((B, T_f), dtype=bool)
    for b in range(B):
        Nb = min(int(lens[b]), N) if isolate else N
        assert Nb > N_FFT // 2, "reflect padding needs more than 256 samples"
        nv = min(flens[b], T_f)
        idx = (np.arange(nv) * hop - N_FFT // 2)[:, None] + np.arange(N_FFT)[None, :]
        idx = np.abs(idx)
        idx = np.where(idx >= Nb, 2 * (Nb - 1) - idx, idx)
        assert idx.min() >= 0 and idx.max() < N
        frames = x[b][idx]
        zero[b, :nv] = ~frames.any(axis=1)
        spec = np.fft.rfft(frames * w[None, :], axis=1)
        P = spec.real ** 2 + spec.imag ** 2
        e = P @ mel
        out_mel[b, :nv] = e
        out_E[b, :nv] = P.sum(axis=1)
        out_log[b, :nv] = np.log(np.maximum(e, FLOOR))
    return LogMel(out_log, out_mel, out_E, np.asarray(flens), zero)


def valid_mask(flens, T_f):
    return np.arange(T_f)[None, :] < np.asarray(flens)[:, None]


def linear_metric(got_log, ref, melmat_f32):
    """r = |exp(got) - e_ref| / (wmax_m * E[b, t]) on the valid frames with E > 0, e_ref the floored linear mel energy
    and wmax_m the filter's largest weight (1 for an all-zero column).  An error of one tap or one bin shows here at
    the size of that tap's share of the frame's power, whatever the log does to it.  Returns (r, mask)."""
    wmax = np.asarray(melmat_f32, dtype=np.float64).max(axis=0)
    wmax = np.where(wmax > 0, wmax, 1.0)
    T_f = ref.logmel.shape[1]
    mask = valid_mask(ref.flens, T_f) & (ref.power_sum > 0)
    den = wmax[None, None, :] * np.where(mask, ref.power_sum, 1.0)[:, :, None]
    r = np.abs(np.exp(np.asarray(got_log, dtype=np.float64)) - np.maximum(ref.mel, FLOOR)) / den
    m3 = np.broadcast_to(mask[:, :, None], r.shape)
    return np.where(m3, r, 0.0), m3


def log_set(ref, melmat_f32):
    """Elements of the log-domain check: valid, and e_ref >= 1e-2 * wmax_m * E[b, t] > 0."""
    wmax = np.asarray(melmat_f32, dtype=np.float64).max(axis=0)
    wmax = np.where(wmax > 0, wmax, 1.0)
    valid = valid_mask(ref.flens, ref.logmel.shape[1])
    thr = LOG_SET * wmax[None, None, :] * ref.power_sum[:, :, None]
    sel = valid[:, :, None] & (ref.power_sum[:, :, None] > 0) & (np.maximum(ref.mel, FLOOR) >= thr)
    return sel, np.broadcast_to(valid[:, :, None], sel.shape)


def log_bound(ref_log, r_bound=None):
    r_bound = R if r_bound is None else r_bound
    return 2 * r_bound / LOG_SET + 2e-6 * np.maximum(1.0, np.abs(ref_log))


# ---------------------------------------------------------------------------------------------- MVN
def utt_mvn_f64(x_f32, flens):
    """utterance_mvn.py:45-88, norm_means only: zero the padding, mean over the valid frames, subtract it from EVERY
    frame (padded frames become -mean).  Returns (normalised, column sums, sums of |x|)."""
    x = np.asarray(x_f32, dtype=np.float64)
    pad = ~valid_mask(flens, x.shape[1])
    x = np.where(pad[:, :, None], 0.0, x)
    s = x.sum(axis=1)
    mean = s / np.asarray(flens, dtype=np.float64)[:, None]
    return x - mean[:, None, :], s, np.abs(x).sum(axis=1)


def global_mvn_f64(x_f32, flens=None, mean=None, std=None):
    """global_mvn.py:71-100: (x - mean) / std on the valid frames, padded frames 0; mean / std None: that step is off;
    flens None: every frame is valid."""
    x = np.asarray(x_f32, dtype=np.float64)
    if mean is not None:
        x = x - np.asarray(mean, dtype=np.float64)
    if flens is not None:
        x = np.where(valid_mask(flens, x.shape[1])[:, :, None], x, 0.0)
    if std is not None:
        x = x / np.asarray(std, dtype=np.float64)
    return x


# ---------------------------------------------------------------------------------------------- dispatch
def frontend_variant(B, T_f, n_mels, mel_maxlen, v1_forced=False):
    """(variant, mel tail) that em_frontend_logmel_f32 runs.  Mirrors csrc/frontend.hip:356-390, the dispatch in
    em_frontend_logmel_f32 (:361 `!v1 && mel_maxlen <= 32 && n_mels <= 80`, :371 `few = cdiv(T_f, 32) * B < 256`,
    :376 `mel_maxlen <= 20`), kernel1's mel tails (:141 `nfull = n_mels & ~63`, :149 `rest > 16`, :155 `rest > 0`) and
    kernel2's (:236 `nfull = n_mels > 64 ? 64 : 0`, :334 `if (nfull)`)."""
    if not v1_forced and mel_maxlen <= 32 and n_mels <= 80:
        few = -(-T_f // 32) * B < 256
        ml = 20 if mel_maxlen <= 20 else 32
        return f"v2/ML{ml}/FR{2 if few else 8}", ("A+B" if n_mels > 64 else "A only")
    nfull = n_mels & ~63
    rest = n_mels - nfull
    return "v1", ("rest>16" if rest > 16 else ("rest<=16" if rest > 0 else "full64"))


def band_limits(melmat):
    """(lo, hi) per column as pack_banded defines them, and the widest band."""
    m = np.asarray(melmat)
    lo = np.zeros(m.shape[1], dtype=np.int64)
    hi = np.ones(m.shape[1], dtype=np.int64)
    for j in range(m.shape[1]):
        nz = np.nonzero(m[:, j])[0]
        if len(nz):
            lo[j], hi[j] = nz[0], nz[-1] + 1
    return lo, hi, int((hi - lo).max())


def unpack_banded(packed, lo, n_bins=N_BINS):
    """Inverse of layers.log_mel.pack_banded: m[lo_j + s, j] = packed[s, j]; taps past the last bin must be zero."""
    packed, lo = np.asarray(packed), np.asarray(lo)
    out = np.zeros((n_bins, packed.shape[1]), dtype=packed.dtype)
    for j in range(packed.shape[1]):
        for s in range(packed.shape[0]):
            if lo[j] + s < n_bins:
                out[lo[j] + s, j] = packed[s, j]
            else:
                assert packed[s, j] == 0, (s, j)
    return out


# ---------------------------------------------------------------------------------------------- filter matrices
def synthetic_melmat(spec, seed=0, interior_zeros=False, zero_columns=()):
    """(257, len(spec)) f32 from a list of (lo, length) bands: seeded weights in [0.25, 1.25), so both ends of every
    band are non-zero and the packed width is exactly the largest length.  interior_zeros: every third tap strictly
    inside a band of 5 or more is zero.  zero_columns: these columns are all zero."""
    rng = np.random.default_rng(seed)
    m = np.zeros((N_BINS, len(spec)), dtype=np.float32)
    for j, (lo, n) in enumerate(spec):
        assert 0 <= lo and n >= 1 and lo + n <= N_BINS, (lo, n)
        w = (0.25 + rng.random(n)).astype(np.float32)
        if interior_zeros and n >= 5:
            w[2:n - 1:3] = 0.0
        m[lo:lo + n, j] = w
    for j in zero_columns:
        m[:, j] = 0.0
    return m


def one_hot_melmat(bins):
    """One unit tap per column: column j passes power bin bins[j] through unchanged."""
    m = synthetic_melmat([(int(k), 1) for k in bins])
    m[m != 0] = 1.0
    return m


def slaney(n_mels):
    from oracle.mel import slaney_mel_filterbank

    return np.ascontiguousarray(slaney_mel_filterbank(16000, 512, n_mels, 0, 8000).T.astype(np.float32))


def edge_bank(maxlen, n_cols=70, seed=0):
    """A synthetic bank whose widest band is exactly `maxlen`: random bands of 1 .. maxlen taps, one of exactly maxlen at
    bin 3, and the last column ending at bin 256 with min(maxlen, 32) taps ([225, 257) for maxlen 32 and 33)."""
    rng = np.random.default_rng(1000 + seed + maxlen)
    spec = []
    for j in range(n_cols - 2):
        n = int(rng.integers(1, maxlen + 1))
        spec.append((int(rng.integers(0, N_BINS - n + 1)), n))
    spec.append((3, maxlen))
    last = min(maxlen, 32)
    spec.append((N_BINS - last, last))
    return synthetic_melmat(spec, seed=seed + maxlen)


def odd_bank(n_cols, seed=5):
    """Interior zeros in every wide band, column 7 all zero, widest band 18."""
    rng = np.random.default_rng(seed)
    spec = []
    for j in range(n_cols):
        n = int(rng.integers(5, 19))
        spec.append((int(rng.integers(0, N_BINS - n + 1)), n))
    spec[0] = (100, 18)
    return synthetic_melmat(spec, seed=seed, interior_zeros=True, zero_columns=(7,))


# ---------------------------------------------------------------------------------------------- signals
def signal(kind, n, seed=0):
    """One utterance of n samples, built in f64 and rounded to f32 once."""
    rng = np.random.default_rng(77000 + seed)
    t = np.arange(n, dtype=np.float64)
    if kind == "noise":  # N(0, 0.1^2)
        x = 0.1 * rng.standard_normal(n)
    elif kind == "tone":  # exactly on bin 64 of the 512-point transform
        x = np.sin(2.0 * math.pi * 64.0 * t / 512.0)
    elif kind == "dcnyq":  # Nyquist plus DC
        x = 0.5 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + 0.2
    elif kind == "impulse":  # flat spectrum: every tap of every filter counts the same
        x = np.zeros(n)
        x[n // 2 + 3] = 1.0
    elif kind == "gap":  # noise with an all-zero stretch of 1300 samples (>= 1200) inside it: floor frames among valid ones
        assert n >= 2500, n
        x = 0.1 * rng.standard_normal(n)
        a = (n - 1300) // 2
        x[a:a + 1300] = 0.0
    elif kind == "loud":  # int16-scale audio, within +-3e4
        x = np.clip(8000.0 * rng.standard_normal(n), -3e4, 3e4)
    elif kind.startswith("multitone:"):
        # bin-centred cosines of equal amplitude on bins lo .. hi (seeded phases), overall RMS near 0.1: with the
        # rectangular 512 window every one of these bins, and no other, carries the same power.  Not in the issue's list:
        # it is what lets a one-hot bank have 10 % of its elements in the log-domain set (see CASES).
        lo, hi = (int(v) for v in kind.split(":")[1].split("-"))
        ks = np.arange(lo, hi + 1, dtype=np.float64)
        ph = rng.uniform(0.0, 2.0 * math.pi, len(ks))
        ph = np.where((ks == 0) | (ks == 256), 0.0, ph)
        x = np.cos(2.0 * math.pi * ks[None, :] * t[:, None] / 512.0 + ph[None, :]).sum(axis=1)
        x *= 0.1 * math.sqrt(2.0 / len(ks))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def build_batch(rows, N):
    """rows: list of utterances, each a list of (kind, n) segments laid end to end.  -> speech (B, N) f32, lens."""
    speech = np.zeros((len(rows), N), dtype=np.float32)
    lens = []
    for b, segs in enumerate(rows):
        pos = 0
        for i, (kind, n) in enumerate(segs):
            speech[b, pos:pos + n] = signal(kind, n, seed=31 * b + i)
            pos += n
        assert 700 <= pos <= N, pos
        lens.append(pos)
    return speech, lens


Case = namedtuple("Case", "name bank hop win_length window N rows isolate variant tail")

# rows of the Hann-400 cases: the signals of the issue, each utterance one signal
ROWS4 = [[("noise", 16000)], [("gap", 12345)], [("loud", 5000)], [("dcnyq", 700)]]
ROWS3 = [[("noise", 8000)], [("gap", 5000)], [("impulse", 700)]]
ROWS4_ODD = [[("noise", 16001)], [("gap", 12345)], [("loud", 5000)], [("impulse", 700)]]


def rows3_rect(lo, hi):
    """Rows of the one-hot (rectangular 512 window) cases.  A one-hot column sees one bin, and of white noise, an
    impulse, a tone or DC + Nyquist at most ~8 % of the (frame, bin) pairs hold 1 % of the frame's power, so the
    log-domain check's 10 % share cannot be met by the listed signals alone; row 0 is therefore the multitone that
    fills exactly the bank's bins, and the listed signals follow it in rows 1 and 2."""
    return [[(f"multitone:{lo}-{hi}", 8000)], [("tone", 2600), ("impulse", 1100), ("dcnyq", 1300)], [("noise", 700)]]


def rows32():
    """32 ragged utterances for the batch walk (FR = 8): every signal, lengths from 700 to the full row."""
    kinds = ["noise", "gap", "loud", "dcnyq", "impulse", "noise", "gap", "loud"]
    lens = [40960, 33333, 20001, 12345, 5000, 2500, 40001, 9999]
    rows = []
    for b in range(32):
        n = 700 if b in (3, 12) else lens[(b + b // 8) % 8]
        rows.append([(kinds[b % 8], n)])
    return rows


def _cases():
    H = dict(hop=160, win_length=400, window="hann")
    Rw = dict(hop=160, win_length=512, window=None)
    c = []

    def add(name, bank, N, rows, variant, tail, isolate=False, **kw):
        c.append(Case(name=name, bank=bank, N=N, rows=rows, isolate=isolate, variant=variant, tail=tail, **kw))

    add("slaney80-small", ("slaney", 80), 16000, ROWS4, "v2/ML20/FR2", "A+B", isolate=True, **H)
    add("slaney80-batch", ("slaney", 80), 40960, rows32(), "v2/ML20/FR8", "A+B", isolate=True, **H)
    add("slaney48", ("slaney", 48), 16000, ROWS4, "v2/ML32/FR2", "A only", **H)
    add("slaney64", ("slaney", 64), 16000, ROWS4, "v2/ML32/FR2", "A only", **H)
    add("slaney56-batch", ("slaney", 56), 40960, rows32(), "v2/ML32/FR8", "A only", **H)
    add("slaney72", ("slaney", 72), 16000, ROWS4, "v2/ML20/FR2", "A+B", **H)
    for ml, var in ((20, "v2/ML20/FR2"), (21, "v2/ML32/FR2"), (32, "v2/ML32/FR2"), (33, "v1")):
        add(f"edge{ml}", ("edge", ml), 8000, ROWS3, var, "rest<=16" if var == "v1" else "A+B", **H)
    for lo in (0, 80, 160, 177):
        add(f"onehot{lo}-{lo + 79}", ("onehot", lo, lo + 80), 8000, rows3_rect(lo, lo + 79), "v2/ML20/FR2", "A+B", **Rw)
    add("onehot217-256", ("onehot", 217, 257), 8000, rows3_rect(217, 256), "v2/ML20/FR2", "A only", **Rw)
    add("slaney96", ("slaney", 96), 8000, ROWS3, "v1", "rest>16", **H)
    add("slaney128", ("slaney", 128), 8000, ROWS3, "v1", "full64", **H)
    add("slaney144", ("slaney", 144), 8000, ROWS3, "v1", "rest<=16", **H)
    add("slaney23", ("slaney", 23), 8000, ROWS3, "v1", "rest>16", **H)
    add("slaney40", ("slaney", 40), 8000, ROWS3, "v1", "rest>16", **H)
    add("odd70", ("odd", 70), 8000, ROWS3, "v2/ML20/FR2", "A+B", **H)
    add("odd40", ("odd", 40), 8000, ROWS3, "v2/ML20/FR2", "A only", **H)
    H97 = dict(hop=97, win_length=400, window="hann")
    add("hop97-padded", ("slaney", 80), 16001, ROWS4_ODD, "v2/ML20/FR2", "A+B", isolate=False, **H97)
    add("hop97-isolate", ("slaney", 80), 16001, ROWS4_ODD, "v2/ML20/FR2", "A+B", isolate=True, **H97)
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case_bank(case):
    kind = case.bank[0]
    if kind == "slaney":
        return slaney(case.bank[1])
    if kind == "edge":
        return edge_bank(case.bank[1])
    if kind == "onehot":
        return one_hot_melmat(range(case.bank[1], case.bank[2]))
    if kind == "odd":
        return odd_bank(case.bank[1])
    raise ValueError(kind)


def case_inputs(case):
    """-> (speech (B, N) f32, lens, melmat (257, n_mels) f32)."""
    speech, lens = build_batch(case.rows, case.N)
    return speech, lens, case_bank(case)


def case_window_f32(case):
    """The win_length window values as the device holds them (f32): periodic Hann rounded to f32, or ones."""
    import torch

    if case.window is None:
        return np.ones(case.win_length, dtype=np.float32)
    return torch.hann_window(case.win_length, dtype=torch.float32).numpy()


_REF = {}


def case_reference(case):
    """The f64 reference of a case, computed once per process and shared (do not modify the arrays)."""
    if case.name not in _REF:
        speech, lens, melmat = case_inputs(case)
        _REF[case.name] = logmel_f64(speech, lens, melmat, case.win_length, case.hop, case_window_f32(case),
                                     case.isolate)
    return _REF[case.name]
