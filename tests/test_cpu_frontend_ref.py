"""The float64 frontend reference (tests/frontend_ref.py) without a GPU: pinned against torch.stft in float64, the
band packing round trip, the coverage table of the GPU test's case list (every kernel variant and mel tail is reached),
and the source of the GPU test's tolerance: the f32 CPU pipeline measured against the f64 reference on the same
signals."""
import numpy as np
import pytest
import torch

from espnet_amd.layers.log_mel import mel_filterbank, pack_banded
from espnet_amd.nets_utils import stft_frame_lengths
from tests import frontend_ref as fr


def _torch_logmel(speech, lens, melmat, win_length, hop, window, isolate, dtype):
    """torch.stft -> power -> matmul -> clamp -> log, padded frames 0; per utterance on its own samples with `isolate`
    (the utterance decoded alone).  `window`: the win_length values."""
    B, N = speech.shape
    T_f = 1 + N // hop
    w = torch.as_tensor(window).to(dtype)
    mel = torch.as_tensor(melmat).to(dtype)
    flens = stft_frame_lengths(lens, 512, hop)
    out = torch.zeros(B, T_f, mel.shape[1], dtype=dtype)
    lin = torch.zeros(B, T_f, mel.shape[1], dtype=dtype)
    for b in range(B):
        x = torch.as_tensor(speech[b, : lens[b] if isolate else N]).to(dtype)
        spec = torch.stft(x, n_fft=512, win_length=win_length, hop_length=hop, center=True, window=w,
                          normalized=False, onesided=True, return_complex=True)
        P = (spec.real ** 2 + spec.imag ** 2).T[: flens[b]]
        e = P @ mel
        lin[b, : flens[b]] = e
        out[b, : flens[b]] = torch.clamp(e, min=1e-10).log()
    return out.numpy(), lin.numpy()


@pytest.mark.parametrize("isolate", [False, True])
@pytest.mark.parametrize("win_length,window,hop", [(400, "hann", 160), (512, "hann", 128), (512, None, 97),
                                                   (400, "f32", 97), (512, None, 160), (400, "hann", 128)])
def test_logmel_f64_matches_torch_stft_float64(win_length, window, hop, isolate):
    speech, lens = fr.build_batch([[("noise", 4001)], [("gap", 2811)], [("dcnyq", 700)], [("tone", 1500)]], 4001)
    melmat = fr.slaney(80)
    if window == "f32":  # the f32 window values of the device, widened
        wv = torch.hann_window(win_length, dtype=torch.float32).numpy()
        arg = wv
    else:
        wv = fr.hann_periodic(win_length) if window == "hann" else np.ones(win_length)
        arg = window
    ref = fr.logmel_f64(speech, lens, melmat, win_length, hop, arg, isolate)
    want_log, want_lin = _torch_logmel(speech, lens, melmat, win_length, hop, wv, isolate, torch.float64)
    assert ref.flens.tolist() == stft_frame_lengths(lens, 512, hop) == fr.stft_frame_lengths(lens, hop)
    scale = np.abs(want_lin).max(axis=(1, 2), keepdims=True)
    # linear energies to 1e-12 of the utterance's largest; logs to 1e-12 relative wherever the energy is not a
    # cancellation residue (the f64 FFTs of numpy and torch differ by ~1e-16 of the frame's largest bin)
    assert (np.abs(ref.mel - want_lin) <= 1e-12 * scale).all()
    big = want_lin > 1e-3 * scale
    assert big.mean() > 0.3
    assert (np.abs(ref.logmel - want_log)[big] <= 1e-12 * np.maximum(1.0, np.abs(want_log[big]))).all()
    T_f = ref.logmel.shape[1]
    pad = ~fr.valid_mask(ref.flens, T_f)
    assert (ref.logmel[pad] == 0).all() and (ref.mel[pad] == 0).all() and (ref.power_sum[pad] == 0).all()


def test_logmel_f64_floor_and_zero_frames():
    speech, lens = fr.build_batch([[("gap", 5000)], [("impulse", 900)]], 5000)
    ref = fr.logmel_f64(speech, lens, fr.slaney(80), 400, 160, "hann", True)
    assert ref.frames_zero[0].sum() >= 4 and ref.frames_zero[1].sum() >= 1
    assert (ref.logmel[ref.frames_zero] == np.log(1e-10)).all()
    assert (ref.power_sum[ref.frames_zero] == 0).all()


def test_mvn_references_match_the_oracle():
    from oracle import conformer as oc

    x = torch.randn(3, 20, 7, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    flens = torch.tensor([20, 11, 1])
    got, s, sabs = fr.utt_mvn_f64(x.numpy(), flens.tolist())
    assert np.allclose(got, oc.utterance_mvn(x, flens).numpy(), rtol=0, atol=1e-13)
    assert (got[1, 11:] == -(s[1] / 11)[None, :]).all() and (sabs >= np.abs(s)).all()
    mean, std = torch.randn(7, dtype=torch.float64), torch.rand(7, dtype=torch.float64) + 0.5
    g = fr.global_mvn_f64(x.numpy(), flens.tolist(), mean.numpy(), std.numpy())
    assert np.allclose(g, oc.global_mvn(x, flens, mean, std).numpy(), rtol=0, atol=1e-13)
    assert (g[1, 11:] == 0).all()
    assert np.array_equal(fr.global_mvn_f64(x.numpy(), None, None, None), x.numpy())
    assert np.array_equal(fr.global_mvn_f64(x.numpy(), None, mean.numpy(), None), (x - mean).numpy())
    assert np.array_equal(fr.global_mvn_f64(x.numpy(), [20, 20, 20], None, std.numpy()), (x / std).numpy())


# ---------------------------------------------------------------------------------------------- packing
def _synthetic_banks():
    banks = {f"edge{ml}": fr.edge_bank(ml) for ml in (20, 21, 32, 33)}
    banks["odd70"] = fr.odd_bank(70)
    banks["odd40"] = fr.odd_bank(40)
    banks["onehot177-256"] = fr.one_hot_melmat(range(177, 257))
    banks["band225-257"] = fr.synthetic_melmat([(225, 32), (0, 1), (256, 1), (10, 7)], seed=9)
    banks["zero-first-and-last"] = fr.synthetic_melmat([(5, 3), (40, 9), (200, 57)], seed=2, interior_zeros=True,
                                                      zero_columns=(0, 2))
    return banks


def test_pack_banded_round_trips_exactly():
    for name, m in _synthetic_banks().items():
        packed, lo, maxlen = pack_banded(torch.from_numpy(m))
        back = fr.unpack_banded(packed.numpy(), lo.numpy())
        assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), m.view(np.uint32)), name
        blo, bhi, bmax = fr.band_limits(m)
        assert maxlen == bmax == packed.shape[0] and np.array_equal(lo.numpy(), blo), name
    assert fr.band_limits(fr.edge_bank(32))[2] == 32 and fr.band_limits(fr.edge_bank(33))[2] == 33
    m = fr.edge_bank(32)
    assert np.nonzero(m[:, -1])[0].tolist() == list(range(225, 257))
    m = fr.odd_bank(70)
    assert not m[:, 7].any() and ((m == 0) & (np.cumsum(m, 0) > 0) & (np.cumsum(m[::-1], 0)[::-1] > 0)).any()


def test_slaney_band_widths():
    """The widths the dispatch sees for the Slaney banks (16 kHz, n_fft 512, 0 - 8000 Hz); bin 256 has weight 0 in all."""
    want = {80: 18, 72: 20, 64: 23, 56: 26, 48: 30, 40: 36, 23: 58}
    for n, w in want.items():
        m = fr.slaney(n)
        lo, hi, maxlen = fr.band_limits(m)
        assert maxlen == w, (n, maxlen)
        assert hi.max() == 256 and not m[256].any()
        assert np.array_equal(m, mel_filterbank(16000, 512, n, 0, 8000))  # the oracle's bank is the package's


# ---------------------------------------------------------------------------------------------- coverage
def _case_shape(case):
    m = fr.case_bank(case)
    return len(case.rows), 1 + case.N // case.hop, m.shape[1], fr.band_limits(m)[2]


def test_frontend_variant_restates_the_dispatch():
    assert fr.frontend_variant(4, 101, 80, 18) == ("v2/ML20/FR2", "A+B")
    assert fr.frontend_variant(4, 101, 80, 18, v1_forced=True) == ("v1", "rest<=16")
    assert fr.frontend_variant(32, 257, 80, 20) == ("v2/ML20/FR8", "A+B")
    assert fr.frontend_variant(28, 257, 80, 20)[0] == "v2/ML20/FR2"  # 9 * 28 = 252 < 256
    assert fr.frontend_variant(8, 1001, 64, 21) == ("v2/ML32/FR8", "A only")
    assert fr.frontend_variant(1, 67, 65, 32) == ("v2/ML32/FR2", "A+B")
    assert fr.frontend_variant(1, 67, 80, 33) == ("v1", "rest<=16")
    assert fr.frontend_variant(1, 67, 81, 18) == ("v1", "rest>16")
    assert fr.frontend_variant(1, 67, 128, 18) == ("v1", "full64")
    assert fr.frontend_variant(1, 67, 40, 36) == ("v1", "rest>16")


def test_case_list_covers_every_variant_and_tail(capsys):
    seen, rows = set(), []
    for case in fr.CASES:
        B, T_f, n_mels, maxlen = _case_shape(case)
        got = fr.frontend_variant(B, T_f, n_mels, maxlen)
        assert got == (case.variant, case.tail), (case.name, got)
        seen.add(got + (n_mels,))
        forced = fr.frontend_variant(B, T_f, n_mels, maxlen, v1_forced=True)
        assert forced[0] == "v1"
        seen.add(forced + (n_mels,))
        rows.append(f"{case.name:18s} B={B:2d} T_f={T_f:3d} n_mels={n_mels:3d} maxlen={maxlen:2d} "
                    f"{got[0]:12s} {got[1]:8s} forced: {forced[1]}")
        speech, lens = fr.build_batch(case.rows, case.N)
        assert min(lens) >= 700 and speech.shape == (B, case.N)
    with capsys.disabled():
        print("\nfrontend cases:\n  " + "\n  ".join(rows))
    variants = {s[0] for s in seen}
    assert variants == {"v1", "v2/ML20/FR2", "v2/ML20/FR8", "v2/ML32/FR2", "v2/ML32/FR8"}
    natural_v1 = {(c.tail, _case_shape(c)[2]) for c in fr.CASES if c.variant == "v1"}
    assert {t for t, _ in natural_v1} == {"full64", "rest>16", "rest<=16"}
    assert all(any(t == tail and n > 80 for t, n in natural_v1) for tail in ("full64", "rest>16", "rest<=16"))
    v2 = {(s[1], s[2]) for s in seen if s[0].startswith("v2")}
    assert {t for t, _ in v2} == {"A only", "A+B"}
    assert any(t == "A+B" and 64 < n < 80 for t, n in v2)
    # both tails on both templates' batch and small walks where the issue asks for them
    for want in (("v2/ML20/FR8", "A+B"), ("v2/ML32/FR8", "A only"), ("v2/ML32/FR2", "A only"), ("v2/ML20/FR2", "A only")):
        assert any(s[:2] == want for s in seen), want
    # bin 256 carries weight in a B-lane column, in an A-lane column and in a v1 case
    def col256(c):
        m = fr.case_bank(c)
        return [j for j in range(m.shape[1]) if m[256, j] != 0]
    assert any(c.tail == "A+B" and any(j >= 64 for j in col256(c)) for c in fr.CASES if c.variant != "v1")
    assert any(c.tail == "A only" and col256(c) for c in fr.CASES if c.variant != "v1")
    assert any(col256(c) for c in fr.CASES if c.variant == "v1")
    # every signal of the issue is used, the hop-97 / odd-N rows in both reflection modes
    kinds = {k.split(":")[0] for c in fr.CASES for row in c.rows for k, _ in row}
    assert kinds == {"noise", "tone", "dcnyq", "impulse", "gap", "loud", "multitone"}
    assert {c.isolate for c in fr.CASES if c.hop == 97 and c.N % 2 == 1} == {False, True}


# ---------------------------------------------------------------------------------------------- tolerance source
@pytest.fixture(scope="module")
def f32_pipeline():
    """Per case: worst linear metric r of the f32 CPU pipeline against the f64 reference, worst log-domain excess, and
    the share of valid elements in the log-domain set."""
    out = {}
    for case in fr.CASES:
        speech, lens, melmat = fr.case_inputs(case)
        ref = fr.case_reference(case)
        got, _ = _torch_logmel(speech, lens, melmat, case.win_length, case.hop, fr.case_window_f32(case),
                               case.isolate, torch.float32)
        r, _ = fr.linear_metric(got, ref, melmat)
        sel, valid = fr.log_set(ref, melmat)
        err = np.abs(got.astype(np.float64) - ref.logmel)
        out[case.name] = (r.max(), (err / fr.log_bound(ref.logmel))[sel].max(), sel.sum() / valid.sum())
    return out


def test_tolerance_source(f32_pipeline, capsys):
    """The bound R of tests/test_gpu_frontend.py is 8x the worst r of the f32 CPU pipeline on the same signals
    (R_CPU in tests/frontend_ref.py, recorded in profiles/frontend_f64_parity.txt).  Another FFT library may differ in
    its last bits, hence the factor 2 here; R itself is fixed."""
    worst = max(v[0] for v in f32_pipeline.values())
    with capsys.disabled():
        print("\nf32 CPU pipeline vs logmel_f64 (worst r, worst log error / log bound, share in the log set):")
        for name, (r, lg, share) in f32_pipeline.items():
            print(f"  {name:18s} r = {r:.3e}  log = {lg:.3f}  share = {share:.3f}")
        print(f"  worst r = {worst:.3e}; R_CPU = {fr.R_CPU:.3e}, R = {fr.R:.3e}")
    assert fr.R == 8 * fr.R_CPU and fr.R <= fr.R_MAX
    assert worst <= 2 * fr.R_CPU, worst
    assert worst >= fr.R_CPU / 4, "R_CPU is stale: the CPU pipeline is much closer than recorded"


def test_log_domain_set_is_never_thin(f32_pipeline):
    """At least 10 % of every case's valid elements are in the log-domain set (a property of the reference alone), and
    the f32 CPU pipeline meets the log-domain bound there."""
    for name, (r, lg, share) in f32_pipeline.items():
        assert share >= 0.10, (name, share)
        assert lg <= 1.0, (name, lg)
