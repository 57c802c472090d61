"""The mixed-radix log-mel kernel (csrc/frontend_mr.hip, n_fft other than 512) against a numpy float64 reference, through
DefaultFrontend; through ASRTask / Speech2Text at n_fft 400; and at n_fft 512 through its C entry beside the 512 kernel.

Bounds: nr.R[n_fft] = 8x the linear metric of torch's own f32 CPU pipeline on the same signals (the rule of
tests/test_gpu_frontend.py), measured without a GPU by tools/frontend_nfft_parity.py and recorded, with the worst value
of every case on an MI355X, in profiles/frontend_nfft_parity.txt."""
import numpy as np
import pytest
import torch

from espnet_amd.asr.frontend.default import DefaultFrontend
from tests import frontend_nfft_ref as nr
from tests import frontend_ref as fr

pytestmark = pytest.mark.gpu


def check(got, ref, mel, n_fft, what):
    """The linear metric within nr.R, the log domain where tests/frontend_ref.py applies it (>= 10 % of the valid elements),
    all-zero frames log(1e-10), padding exactly 0."""
    assert np.isfinite(got).all()
    r, _ = fr.linear_metric(got, ref, mel)
    sel, valid = fr.log_set(ref, mel)
    excess = (np.abs(got.astype(np.float64) - ref.logmel) / fr.log_bound(ref.logmel, nr.R[n_fft]))[sel].max()
    print(f"\n[frontend-nfft] {what}: worst r = {r.max():.3e} (R = {nr.R[n_fft]:.3e})  log err / bound = {excess:.3f}")
    assert nr.R[n_fft] <= fr.R_MAX
    assert r.max() <= nr.R[n_fft], (what, r.max(), np.unravel_index(np.argmax(r), r.shape))
    assert sel.sum() / valid.sum() >= 0.10 and excess <= 1.0, (what, excess)
    assert ref.frames_zero.any()
    assert (np.abs(got[ref.frames_zero].astype(np.float64) - np.log(1e-10)) <= 4e-6).all()
    assert (got[~fr.valid_mask(ref.flens, got.shape[1])] == 0.0).all()


def run(fe, x, lens, isolate, entry):
    mel = fe.logmel.melmat.cpu().numpy()
    win = torch.hann_window(fe.win_length, dtype=torch.float32).numpy()
    ref = nr.logmel_f64(x, lens, mel, fe.n_fft, fe.hop_length, win, isolate)
    assert fe.feature_lengths(lens) == ref.flens.tolist()
    sp, fl = torch.from_numpy(x).cuda(), torch.tensor(ref.flens, dtype=torch.int32).cuda()
    wl = torch.tensor(lens, dtype=torch.int32).cuda() if isolate else None
    junk = torch.full((x.shape[0], 1 + x.shape[1] // fe.hop_length, fe.n_mels), float("nan"), device="cuda")
    del junk  # (the block the output will most likely get: a skipped frame does not pass as a stale copy)
    got = entry(fe, sp, fl, wl).cpu().numpy()
    return got, ref, mel


# 256: H = 128, radices 4 4 4 2, hop not dividing the size, narrow bands (registers, 24 taps).  400: H = 200, radices
# 4 2 5 5, window shorter than the frame; 23 filters: 45 taps (registers, 48).  240: H = 120, radices 4 2 3 5.
# 1024: H = 512, two to four butterflies per lane and stage, 37 taps (80 filters) and 116 taps (23: the global-memory mel).
# 972: H = 486 = 2 3^5, the one size with six stages, and tiles that end inside a 32-slot block.
@pytest.mark.parametrize("isolate", [True, False], ids=["wlens", "padded"])
@pytest.mark.parametrize("n_mels", [80, 23])
@pytest.mark.parametrize("n_fft,hop,win_length,fs", nr.SIZES, ids=[f"{s[0]}-win{s[2]}" for s in nr.SIZES])
def test_logmel_nfft_f64_parity(n_fft, hop, win_length, fs, n_mels, isolate):
    fe = DefaultFrontend(fs=fs, n_fft=n_fft, win_length=win_length, hop_length=hop, n_mels=n_mels).cuda()
    x, lens = nr.batch(n_fft, fs)
    got, ref, mel = run(fe, x, lens, isolate, lambda fe, sp, fl, wl: fe.forward_device(sp, fl, wl))
    check(got, ref, mel, n_fft, f"n_fft {n_fft} win {fe.win_length} n_mels {n_mels} wlens {isolate}")


def test_nfft_entry_at_512_beside_the_512_kernel():
    """Two FFT orders of the same transform: the new kernel within the bound of the float64 reference and, in the same
    metric and under the same bound, of what em_frontend_logmel_f32 gives (no equal bits asked)."""
    fe = DefaultFrontend(n_fft=512, win_length=400, hop_length=160).cuda()
    x, lens = nr.batch(512, 16000)
    got, ref, mel = run(fe, x, lens, True, nr.logmel_nfft)
    check(got, ref, mel, 512, "n_fft 512 through em_frontend_logmel_nfft_f32")
    old = run(fe, x, lens, True, lambda fe, sp, fl, wl: fe.forward_device(sp, fl, wl))[0]
    r = fr.linear_metric(got, ref._replace(mel=np.exp(old.astype(np.float64))), mel)[0]
    print(f"[frontend-nfft] n_fft 512, new kernel against the 512 kernel: worst r = {r.max():.3e} (R = {nr.R[512]:.3e})")
    assert r.max() <= nr.R[512], (r.max(), np.unravel_index(np.argmax(r), r.shape))
    vmask = fr.valid_mask(ref.flens, got.shape[1])
    assert np.array_equal(got[~vmask], old[~vmask]) and np.array_equal(got[ref.frames_zero], old[ref.frames_zero])


def test_model_with_n_fft_400_builds_and_decodes(tmp_path):
    import yaml

    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.tasks.asr import ASRTask
    from oracle import conformer as oc
    from tests.helpers import golden_speech, golden_state_dict, hparams, load_golden

    g = load_golden("tiny_blocks")
    cfg = dict(g["config"], frontend_conf=dict(n_fft=400, win_length=400, hop_length=160), compute_dtype="float32")
    model = ASRTask.build_model(cfg)
    sd = golden_state_dict(g)
    sd["frontend.logmel.melmat"] = model.frontend.logmel.melmat.clone()  # (201, 80)
    model.load_state_dict(sd, strict=True)
    model.cuda().eval()
    speech, lens = golden_speech(g)
    feats, flens = model.frontend.forward(speech.cuda(), lens.cuda())
    want, wlens = oc.frontend_feats(speech, lens, sd["frontend.logmel.melmat"], 400, 400, 160)
    assert flens.tolist() == wlens.tolist()
    np.testing.assert_allclose(feats.cpu().numpy(), want.numpy(), atol=3e-4, rtol=0)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({k: v for k, v in cfg.items() if k != "compute_dtype"}))
    torch.save(sd, tmp_path / "model.pth")
    s2t = Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"),
                      device="cuda", dtype="float32", ctc_greedy=True, nbest=1)
    hp = hparams(g)
    n = int(lens[0])
    with torch.no_grad():
        enc, ol = oc.encode(sd, speech[:1, :n], lens[:1], hp["heads"], hp["num_blocks"], 400, 400, 160)
    assert s2t(speech[0, :n])[0][2] == oc.greedy_ctc(sd, enc, ol, blank=0, sos_eos=int(g["vocab"]) - 1)[0]
