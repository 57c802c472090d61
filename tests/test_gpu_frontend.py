"""Float64 parity of the frontend kernels (csrc/frontend.hip): every instantiation of the log-mel kernel and every mel
tail of both kernels, the MVN kernels on each of their code paths, and the first subsampling conv with a second trip of
its channel loop, all against the numpy float64 restatement in tests/frontend_ref.py.

Tolerances.  The log-mel bound R (frontend_ref.R) is 8x the worst linear metric of the f32 CPU pipeline on the same
signals, measured without a GPU by tests/test_cpu_frontend_ref.py::test_tolerance_source; the measured CPU value, the
worst r of each case on an MI355X and R are recorded in profiles/frontend_f64_parity.txt.  The MVN bounds are derived
from the f32 format (each stated where it is used)."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from espnet_amd import lib as L
from espnet_amd.nets_utils import stft_frame_lengths
from tests import frontend_ref as fr

pytestmark = pytest.mark.gpu
EPS = fr.EPS32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


_KEEP = []


def dev(t):
    """Copy to the GPU and keep the tensor alive until the test ends (raw pointers go to the C ABI)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.contiguous().cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def sptr():
    return L.current_stream_ptr()


@contextlib.contextmanager
def frontend_v1(forced):
    """ESPNET_AMD_FRONTEND_V1 flipped in-process, as tests/test_gpu_kernels.py::test_frontend_v2_equals_v1 does."""
    if forced:
        os.environ["ESPNET_AMD_FRONTEND_V1"] = "1"
    L.load().em_dev_switches_reload()
    try:
        yield
        torch.cuda.synchronize()
    finally:
        os.environ.pop("ESPNET_AMD_FRONTEND_V1", None)
        L.load().em_dev_switches_reload()


def run_frontend(fe, sp, flens, wlens, forced):
    """One forward_device call; the block its output will most likely get from the caching allocator is filled with NaN
    first, so a frame the kernel skipped does not pass as a stale copy of an earlier run."""
    shape = (sp.shape[0], 1 + sp.shape[1] // fe.hop_length, fe.n_mels)
    junk = torch.full(shape, float("nan"), dtype=torch.float32, device=sp.device)
    del junk
    with frontend_v1(forced):
        return fe.forward_device(sp, flens, wlens).cpu().numpy()


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_logmel_f64_parity(lib, case):
    """em_frontend_logmel_f32 against logmel_f64 on the case list of tests/frontend_ref.py (shapes chosen as the
    smallest that reach each kernel variant and mel tail; tests/test_cpu_frontend_ref.py checks that the list reaches
    them all).  Bound R and its source: see the module docstring and profiles/frontend_f64_parity.txt."""
    from espnet_amd.asr.frontend.default import DefaultFrontend

    speech, lens, melmat = fr.case_inputs(case)
    ref = fr.case_reference(case)
    B, N = speech.shape
    T_f, n_mels = 1 + N // case.hop, melmat.shape[1]
    maxlen = fr.band_limits(melmat)[2]
    variant = fr.frontend_variant(B, T_f, n_mels, maxlen)
    assert variant == (case.variant, case.tail), variant  # a moved dispatch threshold must not silently un-cover a branch
    fe = DefaultFrontend(fs=16000, n_fft=512, win_length=case.win_length, hop_length=case.hop, window=case.window,
                         n_mels=n_mels)
    fe.logmel.melmat.copy_(torch.from_numpy(melmat))
    fe.cuda()
    assert np.array_equal(fe._window_padded().numpy().astype(np.float64),
                          fr.window_padded(case.win_length, fr.case_window_f32(case)))
    glens = fe.feature_lengths(lens)
    assert glens == stft_frame_lengths(lens, 512, case.hop) == ref.flens.tolist()
    sp = dev(speech)
    assert fe.packed(sp.device).maxlen == maxlen
    flens = dev(torch.tensor(glens, dtype=torch.int32))
    wlens = dev(torch.tensor(lens, dtype=torch.int32)) if case.isolate else None

    got = run_frontend(fe, sp, flens, wlens, forced=False)
    assert got.shape == (B, T_f, n_mels) and np.isfinite(got).all()
    old = run_frontend(fe, sp, flens, wlens, forced=True) if case.variant != "v1" else None

    # 1. linear metric
    r, _ = fr.linear_metric(got, ref, melmat)
    sel, valid = fr.log_set(ref, melmat)
    err = np.abs(got.astype(np.float64) - ref.logmel)
    share = sel.sum() / valid.sum()
    excess = (err / fr.log_bound(ref.logmel))[sel].max()
    print(f"\n[frontend-parity] {case.name:18s} {case.variant:12s} {case.tail:8s} worst r = {r.max():.3e} "
          f"(R = {fr.R:.3e})  log err / bound = {excess:.3f}  share = {share:.3f}")
    assert fr.R <= fr.R_MAX
    w = np.unravel_index(np.argmax(r), r.shape)
    assert r.max() <= fr.R, (case.name, r.max(), w, got[w], ref.logmel[w])
    # 2. log domain, where the filter holds at least 1 % of what it could of the frame's power
    assert share >= 0.10, share
    assert excess <= 1.0, (case.name, excess)
    # 3. floor: all-zero frames inside an utterance, and all-zero filter columns in every valid frame
    vmask = fr.valid_mask(ref.flens, T_f)
    floor_el = np.broadcast_to(ref.frames_zero[:, :, None], got.shape).copy()
    zero_cols = ~melmat.any(axis=0)
    floor_el[:, :, zero_cols] |= vmask[:, :, None]
    if any(k in ("gap", "impulse") for row in case.rows for k, _ in row) or zero_cols.any():
        assert floor_el.any()
    if floor_el.any():
        fv = got[floor_el]
        assert (np.abs(fv.astype(np.float64) - np.log(1e-10)) <= 4e-6).all(), fv.min()
        assert (fv.view(np.uint32) == fv.view(np.uint32)[0]).all()
    # 4. padding
    assert (got[~vmask] == 0.0).all()
    # the round-5 kernel's own contract, on this template and tail: the bits of the one-frame-per-wave kernel
    if old is not None:
        assert np.array_equal(got.view(np.uint32), old.view(np.uint32)), np.abs(got - old).max()
    # 5. batch transparency: an utterance decoded alone gives the row it gives in the batch, in both kernels
    if case.isolate:
        for forced in (False, True):
            for b in range(B):
                alone = run_frontend(fe, dev(sp[b:b + 1].clone()), dev(flens[b:b + 1].clone()),
                                     dev(wlens[b:b + 1].clone()), forced)
                assert np.array_equal(alone[0].view(np.uint32), got[b].view(np.uint32)), (forced, b)


# ---------------------------------------------------------------------------------------------- MVN
MVN_T = 61
MVN_FLENS = [61, 40, 9, 8, 7, 1]  # the short ones: fewer frames than the 8 parts


def _mvn_feats(D, T_f=MVN_T, B=len(MVN_FLENS), seed=0):
    """log-mel-like values; the padded frames hold large junk that no MVN kernel may use."""
    g = torch.Generator().manual_seed(100 + D + seed)
    return (torch.randn(B, T_f, D, generator=g) * 2 - 8).numpy()


def _with_junk_padding(x, flens):
    pad = ~fr.valid_mask(flens, x.shape[1])
    out = x.copy()
    out[pad] = 1.0e3
    return out


# D = 80: 16-byte path (n_mels % 4 == 0); 23 and 83: generic path; 260: wide path (n_mels > 256)
@pytest.mark.parametrize("D", [80, 23, 83, 260])
def test_utt_mvn_partial_and_apply_f64(lib, D):
    B, T_f, flens = len(MVN_FLENS), MVN_T, MVN_FLENS
    x = _with_junk_padding(_mvn_feats(D), flens)
    want, s_ref, s_abs = fr.utt_mvn_f64(x, flens)
    xd, fl = dev(x), dev(torch.tensor(flens, dtype=torch.int32))
    partial = torch.full((B, 8, D), float("nan"), device="cuda")
    L.check(lib.em_utt_mvn_partial_f32(L.ptr(xd), L.ptr(fl), B, T_f, D, L.ptr(partial), sptr()))
    p = partial.cpu().numpy().astype(np.float64)
    assert np.isfinite(p).all()
    # f32 accumulation of <= 61 terms in any order, the 8 partials summed here in f64: 4 eps sum|x| per column
    bound = 4 * EPS * s_abs
    assert (np.abs(p.sum(axis=1) - s_ref) <= bound).all(), (np.abs(p.sum(axis=1) - s_ref) / bound).max()
    # parts past the utterance's last frame are exact zeros (flens < 8: only the first flens parts hold a frame)
    for b, n in enumerate(flens):
        chunk = (n + 7) // 8
        for part in range(8):
            if part * chunk >= n:
                assert (p[b, part] == 0).all(), (b, part)
    L.check(lib.em_utt_mvn_apply_f32(L.ptr(xd), L.ptr(partial), L.ptr(fl), B, T_f, D, sptr()))
    got = xd.cpu().numpy().astype(np.float64)
    nf = np.asarray(flens, dtype=np.float64)[:, None]
    mean = s_ref / nf
    xz = np.where(fr.valid_mask(flens, T_f)[:, :, None], x.astype(np.float64), 0.0)
    # the subtraction and the division round once each, on top of the error of the sum: 2 eps (|x| + |mean|) + bound / flens
    tol = 2 * EPS * (np.abs(xz) + np.abs(mean)[:, None, :]) + (bound / nf)[:, None, :]
    assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()
    pad = ~fr.valid_mask(flens, T_f)
    assert (np.abs(got[pad] + np.broadcast_to(mean[:, None, :], got.shape)[pad]) <= tol[pad]).all()  # padded: -mean


@pytest.mark.parametrize("use_flens", [True, False])
@pytest.mark.parametrize("use_mean,use_std", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("D,T_f", [(80, 61), (80, 900), (23, 61), (23, 3000)])  # T_f * D below / above one grid sweep (65536)
def test_global_mvn_f64(lib, D, T_f, use_mean, use_std, use_flens):
    assert (T_f * D > 65536) == (T_f >= 900)
    B = 3
    flens = [T_f, T_f - 9, 7]
    x = _mvn_feats(D, T_f, B, seed=1)
    g = torch.Generator().manual_seed(7 + D)
    mean = (torch.randn(D, generator=g) * 3 - 8).numpy() if use_mean else None
    std = (torch.rand(D, generator=g) * 4 + 0.3).numpy() if use_std else None
    want = fr.global_mvn_f64(x, flens if use_flens else None, mean, std)
    xd = dev(x)
    L.check(lib.em_global_mvn_f32(L.ptr(xd), L.ptr(dev(torch.tensor(flens, dtype=torch.int32))) if use_flens else None,
                                  L.ptr(dev(mean)) if use_mean else None, L.ptr(dev(std)) if use_std else None,
                                  B, T_f, D, sptr()))
    got = xd.cpu().numpy()
    # one correctly rounded subtraction and one correctly rounded division: 2 eps |x - mean| / std
    tol = 2 * EPS * np.abs(want)
    assert (np.abs(got.astype(np.float64) - want) <= tol).all()
    if use_flens:
        assert (got[~fr.valid_mask(flens, T_f)] == 0.0).all()
    if not use_mean and not use_std:
        valid = fr.valid_mask(flens, T_f) if use_flens else np.ones((B, T_f), dtype=bool)
        assert np.array_equal(got[valid], x[valid])


# (D, d): an odd D with a second trip of the channel loop (d > 256), and the widest D the kernel takes
@pytest.mark.parametrize("with_partial", [True, False])
@pytest.mark.parametrize("D,d", [(23, 300), (128, 64)])
def test_conv2d_sub1_f64(lib, D, d, with_partial):
    B, T_f = 3, MVN_T
    flens = [T_f, T_f - 9, 7]
    x = _mvn_feats(D, T_f, B, seed=2)
    x[~fr.valid_mask(flens, T_f)] = 0.0  # (what the log-mel kernel leaves in the padded frames)
    g = torch.Generator().manual_seed(12 + d)
    w1 = (torch.randn(d, 1, 3, 3, generator=g) / 3)
    b1 = torch.randn(d, generator=g) * 0.1
    xd, fl = dev(x), dev(torch.tensor(flens, dtype=torch.int32))
    partial = None
    if with_partial:
        partial = torch.empty(B, 8, D, device="cuda")
        L.check(lib.em_utt_mvn_partial_f32(L.ptr(xd), L.ptr(fl), B, T_f, D, L.ptr(partial), sptr()))
    xin = fr.utt_mvn_f64(x, flens)[0] if with_partial else x.astype(np.float64)
    ref = F.relu(F.conv2d(torch.from_numpy(xin).unsqueeze(1), w1.double(), b1.double(), stride=2)).permute(0, 2, 3, 1)
    T1, F1 = (T_f - 3) // 2 + 1, (D - 3) // 2 + 1
    assert tuple(ref.shape) == (B, T1, F1, d)
    scale = max(ref.abs().max().item(), 1e-6)
    for dt, tdt, tol in ((L.EM_F32, torch.float32, 1e-5), (L.EM_BF16, torch.bfloat16, 1e-2)):
        out = torch.full((B, T1, F1, d), float("nan"), dtype=tdt, device="cuda")
        L.check(lib.em_conv2d_sub1(dt, L.ptr(xd), L.ptr(partial), L.ptr(fl), B, T_f, D, L.ptr(dev(w1.reshape(d, 9))),
                                   L.ptr(dev(b1)), d, L.ptr(out), sptr()))
        err = (out.cpu().double() - ref).abs().max().item()
        assert err <= tol * scale, (str(tdt), err, scale)
