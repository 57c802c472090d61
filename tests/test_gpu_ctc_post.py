"""CTC token posteriors on the device (csrc/ctc_post.hip) against the float64 forward-backward (tests/ctc_post_ref.py) on
the device's own f32 log-probabilities: only the recursion is under test.  nll is em_ctc_seq_nll's value bit for bit and
holds tests/test_gpu_ctc_nll.py's bounds.  occ, peak and blank_post hold E_POST; peak_t equals the reference's wherever its
two largest gamma of the token differ by more than 2 E_POST, which at most one token in ten may miss (asserted)."""
import math

import numpy as np
import pytest
import torch

from tests import scratch_fill as SF
from tests.ctc_post_ref import ctc_post_ref
from tests.helpers import golden_state_dict, load_golden
from tests.test_gpu_ctc_align import synth_y, three_cuts
from tests.test_gpu_ctc_nll import E_CTC_NLL

pytestmark = pytest.mark.gpu

# E_POST = 8 x the largest ABSOLUTE error of occ, peak and blank_post over the issue's cases and the ragged batch on the
# MI355X (the ragged batch; T 600 / L 300: 6.0e-4, every one-wave case below 2e-6).  The two cases beyond the
# issue's table (one and two frames beside a two-wave companion; S above 4 096, the three-walk form) hold the same bounds.
MEASURED = 7.611e-4
E_POST = 8 * MEASURED
A, B_ = 7, 9


def planted_lp(T, ys, seed, V=50):
    """(T, V) log-probs that favour the blank and, spread evenly over the frames, the tokens of the transcripts ys: every
    token has its frame, so the f64 reference decides the peak frames (share of undecided tokens checked on the CPU: none)."""
    x = torch.randn(T, V, generator=torch.Generator().manual_seed(seed))
    x[:, 0] += 3.0
    for y in ys:
        for i, v in enumerate(y):
            x[min(int((i + 0.5) * T / len(y)), T - 1), v] += 6.0
    return torch.log_softmax(x, dim=-1)


CASES = {
    "single frame": [(1, []), (1, [3])],
    "meeting frame is an end frame": [(2, [4]), (2, [])],
    "both parities": [(T, synth_y(L, 10 * T + L)) for T in (6, 7) for L in range(1, 6)],
    "repeated labels": [(10, [A, A, B_, B_]), (9, [A, A, A])],
    "a single path": [(6, [A, A, B_, B_]), (3, [A, B_, A])],
    "no path": [(5, [A, A, B_, B_]), (2, [4, 5, 6])],
    "one and two frames in a two-wave launch": [(1, [3]), (1, []), (2, [4]), (2, []), (300, synth_y(256, 5))],
    "two waves per direction": [(600, synth_y(300, 3))],
    "one group of waves, three walks": [(2200, synth_y(2048, 4))],
}


def device_post(utt_lps, ys, mem_of=None, T=None, ws=None):
    """Utterance rows (T_u, V) + candidates -> ((nll, occ, peak, peak_t, blank_post) on the host, lpT as the device held it)."""
    from espnet_amd.asr.ctc import CTC

    Bm, N = len(utt_lps), len(ys)
    T = T or max(lp.shape[0] for lp in utt_lps)
    Lmax = max(len(y) for y in ys)
    lpT = torch.zeros(utt_lps[0].shape[1], Bm * T)
    tg = torch.zeros(N, max(Lmax, 1), dtype=torch.int32)
    for u, lp in enumerate(utt_lps):
        lpT[:, u * T : u * T + lp.shape[0]] = lp.t()
    for n, y in enumerate(ys):
        tg[n, : len(y)] = torch.tensor(y, dtype=torch.int32)
    olens = torch.tensor([lp.shape[0] for lp in utt_lps], dtype=torch.int32).cuda()
    ylens = torch.tensor([len(y) for y in ys], dtype=torch.int32).cuda()
    mo = None if mem_of is None else torch.tensor(mem_of, dtype=torch.int32).cuda()
    lpT_d = lpT.cuda()
    out = CTC.posteriors_log_probs_t(lpT_d, Bm * T, olens, Bm, T, tg.cuda(), Lmax, ylens, mo, N, 0, blank_post=True, ws=ws)
    nll = CTC.nll_log_probs_t(lpT_d, Bm * T, olens, Bm, T, tg.cuda(), Lmax, ylens, mo, N, 0)
    torch.cuda.synchronize()
    assert SF.bytes_equal(out[0], nll)
    return [o.cpu() for o in out], lpT_d.cpu()


def check(got, lpT, rows, T, tag):
    """rows: (utterance, T_u, y) per candidate.  Returns (tokens, tokens outside the peak_t condition)."""
    nll, occ, peak, peak_t, bp = got
    worst, n_tok, n_open = 0.0, 0, 0
    for n, (u, Tu, y) in enumerate(rows):
        L = len(y)
        w_nll, gamma, w_occ, w_peak, w_pt, w_bp = ctc_post_ref(lpT[:, u * T : u * T + Tu].t().numpy(), y)
        assert not occ[n, L:].any() and not peak[n, L:].any() and not peak_t[n, L:].any() and not bp[n, Tu:].any(), (tag, n)
        if math.isinf(w_nll):
            assert nll[n] == math.inf and not occ[n].any() and not peak[n].any() and (peak_t[n, :L] == -1).all(), (tag, n)
            assert not bp[n].any(), (tag, n)
            continue
        assert abs(float(nll[n]) - w_nll) <= min(E_CTC_NLL, 4 * Tu * 2.0 ** -24) * max(abs(w_nll), 1.0), (tag, n, float(nll[n]), w_nll)
        err = max(float(np.abs(occ[n, :L].numpy() - w_occ).max(initial=0.0)),
                  float(np.abs(peak[n, :L].numpy() - w_peak).max(initial=0.0)),
                  float(np.abs(bp[n, :Tu].numpy() - w_bp).max(initial=0.0)))
        worst = max(worst, err)
        top2 = np.sort(gamma[:, 1::2], axis=0)[-2:] if Tu > 1 else np.stack([np.zeros(L), w_peak])
        sure = top2[1] - top2[0] > 2 * E_POST
        assert (peak_t[n, :L].numpy()[sure] == w_pt[sure]).all(), (tag, n)
        n_tok, n_open = n_tok + L, n_open + int((~sure).sum())
    print(f"\n[{tag}] largest error {worst:.3e} (E_POST {E_POST:.1e}); {n_open} of {n_tok} tokens without a decided peak frame")
    assert worst <= E_POST, (tag, worst)
    return n_tok, n_open


@pytest.mark.parametrize("name", list(CASES))
def test_parity(name):
    rows = CASES[name]
    lps = [planted_lp(T, [y], 31 * i + T) for i, (T, y) in enumerate(rows)]
    got, lpT = device_post(lps, [y for _, y in rows])
    Tm = max(T for T, _ in rows)
    n_tok, n_open = check(got, lpT, [(i, T, y) for i, (T, y) in enumerate(rows)], Tm, name)
    assert 10 * n_open <= n_tok
    if name == "a single path":
        assert (got[1][0, :4] - 1.0).abs().max() <= E_POST and (got[2][0, :4] - 1.0).abs().max() <= E_POST


@pytest.fixture(scope="module")
def ragged():
    """9 candidates over 3 utterances, the second shorter than T; the last candidate makes the launch a two-wave one."""
    ys = [synth_y(19, 21), [], synth_y(30, 23), synth_y(11, 20), [4, 4, 4], synth_y(5, 24), synth_y(60, 25), [], synth_y(300, 26)]
    mem_of = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    utts = [planted_lp(T, ys[3 * u : 3 * u + 3], 70 + u) for u, T in enumerate((57, 40, 330))]
    got, lpT = device_post(utts, ys, mem_of=mem_of)
    return utts, ys, mem_of, got, lpT


def test_ragged_batch_through_mem_of(ragged):
    utts, ys, mem_of, got, lpT = ragged
    n_tok, n_open = check(got, lpT, [(u, utts[u].shape[0], y) for u, y in zip(mem_of, ys)], 330, "ragged")
    assert 10 * n_open <= n_tok
    for n, (u, y) in enumerate(zip(mem_of, ys)):
        alone, _ = device_post([utts[u]], [y])
        L, Tu = len(y), utts[u].shape[0]
        # alone, the candidate gives the bits it gives inside the batch
        for a, g in zip(alone, (got[0][n : n + 1], got[1][n : n + 1, :L], got[2][n : n + 1, :L], got[3][n : n + 1, :L], got[4][n : n + 1, :Tu])):
            assert SF.bytes_equal(a[..., : g.shape[-1]].contiguous(), g.contiguous()), n


def test_workspace_contents_are_ignored():
    from espnet_amd import lib as L

    rows = CASES["both parities"][:3] + CASES["one and two frames in a two-wave launch"]  # (every barrier pairing of the meeting)
    lps = [planted_lp(T, [y], 5 * i + T) for i, (T, y) in enumerate(rows)]
    ws = torch.empty(int(L.load().em_ctc_seq_posteriors_workspace_bytes(len(rows), 300, 256)), dtype=torch.uint8, device="cuda")
    SF.assert_scratch_independent(lambda: [o.cuda() for o in device_post(lps, [y for _, y in rows], ws=ws)[0]], ws, None,
                                  names=["nll", "occ", "peak", "peak_t", "blank_post"])


@pytest.mark.parametrize("what", ["short workspace", "tokens above the cap", "mem_of out of range"])
def test_refused_arguments_touch_no_output(what):
    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC

    lib = L.load()
    cap = int(lib.em_ctc_forced_align_max_tokens())
    if what == "mem_of out of range":  # host data is checked before anything is launched
        ctc = CTC(odim=50, encoder_output_size=8)
        with pytest.raises(ValueError, match="mem_of"):
            ctc.posteriors_device(torch.zeros(1, 8, 8, device="cuda"), [8], [[3]], [1], 0, mem_of=[1])
        return
    Lmax = cap + 1 if what == "tokens above the cap" else 2
    lpT = planted_lp(8, [], 1).t().contiguous().cuda()
    need = int(lib.em_ctc_seq_posteriors_workspace_bytes(1, 8, 2))
    ws = torch.empty(need - 1 if what == "short workspace" else need, dtype=torch.uint8, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32).cuda()
    outs = [torch.full((1, Lmax), 7.0, device="cuda") for _ in range(3)] + [torch.full((1, Lmax), 7, dtype=torch.int32, device="cuda")]
    rc = lib.em_ctc_seq_posteriors(L.ptr(lpT), 8, L.ptr(i32(8)), 1, 8, L.ptr(torch.ones(1, Lmax, dtype=torch.int32).cuda()), Lmax,
                                   L.ptr(i32(2)), None, 1, 0, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(outs[3]), None,
                                   L.ptr(ws), ws.numel(), L.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.EM_ERR_UNSUPPORTED and all((o == 7).all() for o in outs)
    assert lib.em_ctc_seq_posteriors_workspace_bytes(1, 8, cap + 1) == 0


def test_batch_confidence_of_the_model(tmp_path):
    from espnet_amd.bin.asr_inference import Speech2Text

    g = load_golden("small_10s_peaked")
    (tmp_path / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), tmp_path / "model.pth")
    s2t = Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"), device="cuda",
                      dtype="float32", ctc_greedy=True)
    speech, batch, cuts = three_cuts(g)
    res = s2t.batch_confidence(batch, cuts)
    m = s2t.asr_model
    st = m.encode_device(batch.cuda(), cuts, isolate=True)
    for b, c in enumerate(cuts):
        (tokens, conf, occ, secs, nll), = res[b]
        assert tokens == s2t(speech[0, :c].numpy())[0][2] and len(tokens) > 0
        want = m.ctc.token_posteriors(st.enc_out[b : b + 1, : st.olens[b]], [st.olens[b]], [tokens], [len(tokens)], m.blank_id)
        w_nll, w_occ, w_peak, w_pt = [w.cpu()[0].tolist() for w in want]
        assert abs(nll - w_nll) <= 2 * E_CTC_NLL * max(abs(w_nll), 1.0)
        assert np.abs(np.array(conf) - w_peak).max() <= 2 * E_POST and np.abs(np.array(occ) - w_occ).max() <= 2 * E_POST * max(w_occ)
        # (em_ctc_log_probs_t rounds differently for one utterance than for three, as batch_rescore's test allows for; the
        # peaked model holds gamma at 1 over several frames, and on such a plateau that rounding moves the peak frame)
        assert 10 * sum(a != t * s2t.seconds_per_frame for a, t in zip(secs, w_pt)) <= len(tokens)
        assert all(0.0 <= x <= 1.0 + E_POST for x in conf) and all(0.0 <= a < c / 16000 for a in secs)
    # an n-best list and a transcript per utterance; a model's own tokens given back score the same
    again = s2t.batch_confidence(batch, cuts, [[res[0][0][0], res[0][0][0][:2]], res[1][0][0], res[2][0][0]])
    assert [len(r) for r in again] == [2, 1, 1] and again[0][0] == res[0][0] and again[1][0] == res[1][0]
