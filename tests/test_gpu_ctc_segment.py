"""CTC segmentation on the device (csrc/ctc_segment.hip) through the C ABI's wrapper and the host layers, against the
float32 NumPy restatement of the contract (tests/ctc_segment_ref.py).

The trellis does one f32 add per cell and compares, and so does the restatement: first_frame, frame_col, t_end and status
must be EQUAL, total and frame_lp BIT-EQUAL, no tolerance.  (tests/test_cpu_ctc_segment.py holds the float32 restatement
to the float64 one's paths on the same seeds.)  The kernel tests feed lpT directly; the shapes are GPU_CASES of the
restatement's module: one wave without and with a sliding band, slots that wrap (C > threads * 8), three waves, the cap
with the back-pointers in the workspace, a band too narrow for the planted preamble."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_segment_ref as R
from tests.scratch_fill import assert_scratch_independent

pytestmark = pytest.mark.gpu

V = R.VOCAB
NAMES = ("first_frame", "frame_col", "frame_lp", "t_end", "total", "status")


@functools.lru_cache(maxsize=None)
def case(name, blank=0):
    return R.make_case(R.GPU_CASES[name], V, blank)


@functools.lru_cache(maxsize=None)
def want_of(name, flags=R.PREAMBLE_FREE, blank=0):
    lp, gt, _ = case(name, blank)
    cfg = R.GPU_CASES[name]
    return R.segment_ref_batch([lp], [gt], cfg["T"], cfg["C"], blank, cfg["W"], flags)


def device_segment(lps, gts, T, Cmax, blank, W, flags=R.PREAMBLE_FREE, unaligned=False):
    """Rows (T_b, V) + columns -> the six outputs of one launch on the host, through CTC.segment_log_probs_t."""
    from espnet_amd.asr.ctc import CTC

    B, vocab = len(lps), lps[0].shape[1]
    ldT = B * T + (1 - (B * T) % 2 if unaligned else 0)  # odd when unaligned
    flat = torch.zeros(vocab * ldT + 1)
    lpT = flat[1:] if unaligned else flat[:-1]
    lpT = lpT.view(vocab, ldT)
    g = torch.zeros(B, Cmax, dtype=torch.int32)
    for b, (lp, gt) in enumerate(zip(lps, gts)):
        lpT[:, b * T : b * T + lp.shape[0]] = torch.from_numpy(lp).t()
        g[b, : len(gt)] = torch.tensor(gt, dtype=torch.int32)
    flat_d = flat.cuda()
    lpT_d = (flat_d[1:] if unaligned else flat_d[:-1]).view(vocab, ldT)
    assert (lpT_d.data_ptr() % 16 != 0) == unaligned
    olens = torch.tensor([lp.shape[0] for lp in lps], dtype=torch.int32).cuda()
    clens = torch.tensor([len(gt) for gt in gts], dtype=torch.int32).cuda()
    out = CTC.segment_log_probs_t(lpT_d, ldT, olens, g.cuda(), Cmax, clens, B, T, blank, W,
                                  preamble_free=bool(flags & R.PREAMBLE_FREE), from_last_frame=bool(flags & R.FROM_LAST_FRAME))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(NAMES, out)}


def assert_same(got, want, tag):
    for k in ("first_frame", "frame_col", "t_end", "status"):
        assert np.array_equal(got[k], want[k]), (tag, k, np.flatnonzero(np.ravel(got[k] != want[k]))[:8])
    for k in ("total", "frame_lp"):
        assert np.array_equal(got[k].view(np.int32), np.asarray(want[k], np.float32).view(np.int32)), (tag, k)


def run_case(name, flags=R.PREAMBLE_FREE, blank=0, unaligned=False):
    lp, gt, _ = case(name, blank)
    cfg = R.GPU_CASES[name]
    return device_segment([lp], [gt], cfg["T"], cfg["C"], blank, cfg["W"], flags, unaligned)


# ------------------------------------------------------------------ kernel against restatement
@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_kernel_equals_the_restatement(name):
    from espnet_amd import lib as L

    cfg = R.GPU_CASES[name]
    want = want_of(name)
    assert_same(run_case(name), want, name)
    assert int(want["status"][0]) == (R.CLIPPED if name.startswith("i_") else 0) and want["t_end"][0] > 0
    ws = int(L.load().em_ctc_segment_workspace_bytes(1, cfg["T"], cfg["C"], cfg["W"]))
    waves = -(-min(cfg["W"], cfg["C"]) // 512)
    assert ws == (0 if cfg["T"] * waves * 64 <= 48 * 1024 else cfg["T"] * waves * 64)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_all_flag_combinations(flags):
    name = "b_one_wave_slide"
    assert_same(run_case(name, flags), want_of(name, flags), flags)


def test_blank_is_the_last_id():
    for name in ("a_one_wave_no_slide", "b_one_wave_slide"):
        assert_same(run_case(name, blank=V - 1), want_of(name, blank=V - 1), name)


@pytest.mark.parametrize("name", ["a_one_wave_no_slide", "b2_one_wave_slots_wrap", "c2_two_waves_slots_wrap"])
def test_unaligned_log_probs_give_the_same_values(name):
    got = run_case(name, unaligned=True)
    assert_same(got, want_of(name), name)
    aligned = run_case(name)
    for k in NAMES:
        assert got[k].tobytes() == aligned[k].tobytes(), k


@pytest.mark.parametrize("W", [96, 600])
def test_ragged_batch_with_no_route_and_two_columns(W):
    """Three recordings of different T_b and C_b in one launch: one whose C_b - 1 > T_b (lengths as device tensors: the
    host check is not in the way) returns the no-route values, one has C_b = 2.  One wave (W 96) and two (W 600)."""
    cases = [R.make_case(c, V) for c in R.RAGGED]
    lps, gts = [c[0] for c in cases], [c[1] for c in cases]
    T, Cmax = 701, 652
    got = device_segment(lps, gts, T, Cmax, 0, W)
    assert_same(got, R.segment_ref_batch(lps, gts, T, Cmax, 0, W), W)
    assert got["status"][1] & R.NO_ROUTE and got["t_end"][1] == 0 and np.isneginf(got["total"][1])
    assert (got["first_frame"][1] == -1).all() and (got["frame_col"][1] == -1).all() and (got["frame_lp"][1] == 0).all()
    assert got["status"][0] & R.NO_ROUTE == 0 and got["status"][2] == 0 and got["first_frame"][2, :3].tolist()[::2] == [0, -1]
    for b in (0, 2):  # a row of the batch equals the row alone
        alone = device_segment([lps[b]], [gts[b]], lps[b].shape[0], len(gts[b]), 0, W)
        assert np.array_equal(alone["first_frame"][0], got["first_frame"][b, : len(gts[b])])
        assert alone["frame_lp"][0].tobytes() == got["frame_lp"][b, : lps[b].shape[0]].tobytes()
        assert alone["total"].tobytes() == got["total"][b : b + 1].tobytes()


@pytest.mark.parametrize("name", ["c_three_waves", "d_cap_workspace"])
def test_outputs_do_not_depend_on_workspace_or_output_contents(name):
    from espnet_amd import lib as L

    cfg = R.GPU_CASES[name]
    T, C, W = cfg["T"], cfg["C"], cfg["W"]
    lib = L.load()

    def inputs(lp, gt):
        lpT = torch.from_numpy(np.ascontiguousarray(lp.T)).cuda()
        return lpT, torch.tensor([gt], dtype=torch.int32).cuda()

    lp, gt, _ = case(name)
    lpT, g = inputs(lp, gt)
    lp2, gt2, _ = R.make_case(dict(cfg, seed=cfg["seed"] + 100), V)
    lpT2, g2 = inputs(lp2, gt2)
    xl, cl = torch.tensor([T], dtype=torch.int32).cuda(), torch.tensor([C], dtype=torch.int32).cuda()
    need = int(lib.em_ctc_segment_workspace_bytes(1, T, C, W))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pad_C = C + 3  # the pads of the outputs are defined too: the columns behind C_b, the frames behind T_b = T - 7
    xl_s = torch.tensor([T - 7], dtype=torch.int32).cuda()

    def outs():
        return [torch.empty(1, pad_C, dtype=torch.int32, device="cuda"), torch.empty(1, T, dtype=torch.int32, device="cuda"),
                torch.empty(1, T, dtype=torch.float32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
                torch.empty(1, dtype=torch.float32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")]

    def launch(lpT, g, xl, o):
        gp = torch.zeros(1, pad_C, dtype=torch.int32, device="cuda")
        gp[:, :C] = g
        L.check(lib.em_ctc_segment(L.ptr(lpT), T, L.ptr(xl), L.ptr(gp), pad_C, L.ptr(cl), 1, T, 0, W, 1, L.ptr(o[0]), L.ptr(o[1]),
                                   L.ptr(o[2]), L.ptr(o[3]), L.ptr(o[4]), L.ptr(o[5]), L.ptr(ws), need, L.current_stream_ptr()),
                "em_ctc_segment")

    o, o_stale = outs(), outs()
    ref = assert_scratch_independent(lambda: launch(lpT, g, xl_s, o), ws, o, stale=lambda: launch(lpT2, g2, xl, o_stale),
                                     names=NAMES)
    want = R.segment_ref_batch([lp[: T - 7]], [gt], T, pad_C, 0, W)
    assert_same({k: v.numpy() for k, v in zip(NAMES, ref)}, want, name)


def test_return_codes():
    from espnet_amd import lib as L

    lib = L.load()
    cap = int(lib.em_ctc_segment_max_window())
    assert cap == 8192
    T, C = 1700, 1500
    lp, gt, _ = case("c_three_waves")
    lpT = torch.from_numpy(np.ascontiguousarray(lp.T)).cuda()
    g = torch.tensor([gt], dtype=torch.int32).cuda()
    xl, cl = torch.tensor([T], dtype=torch.int32).cuda(), torch.tensor([C], dtype=torch.int32).cuda()
    ff = torch.empty(1, C, dtype=torch.int32, device="cuda")
    fc, fl = torch.empty(1, T, dtype=torch.int32, device="cuda"), torch.empty(1, T, dtype=torch.float32, device="cuda")
    te, st = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    tot = torch.empty(1, dtype=torch.float32, device="cuda")
    need = int(lib.em_ctc_segment_workspace_bytes(1, T, C, 1100))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(W=1100, lpT_=lpT, ws_=ws, ws_bytes=need, flags=1, ff_=ff):
        return lib.em_ctc_segment(L.ptr(lpT_), T, L.ptr(xl), L.ptr(g), C, L.ptr(cl), 1, T, 0, W, flags, L.ptr(ff_), L.ptr(fc),
                                  L.ptr(fl), L.ptr(te), L.ptr(tot), L.ptr(st), L.ptr(ws_), ws_bytes, L.current_stream_ptr())

    assert call() == 0
    assert call(W=cap + 1) == L.EM_ERR_UNSUPPORTED and int(lib.em_ctc_segment_workspace_bytes(1, T, C, cap + 1)) == 0
    assert call(ws_bytes=need - 1) == L.EM_ERR_WORKSPACE and call(ws_=None) == L.EM_ERR_WORKSPACE
    assert call(lpT_=None) == L.EM_ERR_BAD_ARG and call(ff_=None) == L.EM_ERR_BAD_ARG
    assert call(W=0) == L.EM_ERR_BAD_ARG and call(flags=4) == L.EM_ERR_BAD_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="window"):
        from espnet_amd.asr.ctc import CTC

        CTC.segment_log_probs_t(lpT, T, xl, g, C, cl, 1, T, 0, cap + 1)


# ------------------------------------------------------------------ end to end: CTCSegmentation on the peaked Conformer
def utterance_text(g, conv, n_utts=3, n_tok=None):
    """The fixture's own greedy tokens cut into utterances, as a kaldi-style text; returns (text, ids per utterance)."""
    n = int(g["g1_lens"][0]) if n_tok is None else n_tok
    ids = g["g1_tokens"][0, :n].tolist()
    cuts = [round(i * n / n_utts) for i in range(n_utts + 1)]
    utts = [ids[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return "".join(f"utt{k} {' '.join(conv.ids2tokens(u))}\n" for k, u in enumerate(utts)), utts


@pytest.fixture(scope="module", params=["float32", "bfloat16"])
def aligner(request, tmp_path_factory):
    from espnet_amd.bin.asr_align import CTCSegmentation
    from tests.helpers import golden_state_dict, load_golden

    g = load_golden("small_10s_peaked")
    d = tmp_path_factory.mktemp("segment_model")
    (d / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), d / "model.pth")
    return g, d, CTCSegmentation(asr_train_config=str(d / "config.yaml"), asr_model_file=str(d / "model.pth"),
                                 dtype=request.param, time_stamps="fixed")


def restated(al, speech, task, W):
    """The float32 restatement and its segments on the lpT the device produces for this recording, read back."""
    lpT = al.log_probs_t(torch.as_tensor(speech).cuda().float())
    lp = np.ascontiguousarray(lpT.cpu().numpy().T)
    flags = (R.PREAMBLE_FREE if al.preamble_transition_cost_zero else 0) | (R.FROM_LAST_FRAME if al.backtrack_from_max_t else 0)
    r = R.segment_ref(lp, task.ground_truth_mat, al.asr_model.blank_id, W, flags, margin=False)
    return r, R.segments_ref(r["first_frame"], r["frame_lp"], r["t_end"], task.utt_begin_indices, task.index_duration,
                             al.score_min_mean_over_L)


def assert_task_equals(task, r, segs):
    assert np.array_equal(task.first_frame, r["first_frame"]) and task.t_end == r["t_end"] and task.status == r["status"]
    assert task.frame_lp.view(np.int32).tolist() == r["frame_lp"].view(np.int32).tolist()
    assert np.float32(task.total).view(np.int32) == np.float32(r["total"]).view(np.int32)
    assert len(task.segments) == len(segs)
    for a, b in zip(task.segments, segs):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == pytest.approx(b[2], abs=1e-9)


def test_call_equals_the_restatement_on_the_devices_own_log_probs(aligner):
    from tests.helpers import golden_speech

    g, _, al = aligner
    speech = golden_speech(g)[0][0].numpy()
    text, utts = utterance_text(g, al.converter)
    task = al(speech, text, name="rec")
    n_fr = int(g["enc_olens"][0])
    assert task.lpz_frames == n_fr and task.index_duration == 4 * 160 / 16000 and not task.clipped
    assert task.ground_truth_mat == R.build_gt(utts, al.asr_model.blank_id, start=al.asr_model.blank_id)[0]
    r, segs = restated(al, speech, task, task.window)
    assert_task_equals(task, r, segs)
    lines = str(task).splitlines()
    assert len(lines) == 3 and lines[0].startswith("utt0 rec ")
    assert all(task.segments[k][1] <= task.segments[k + 1][0] + 1e-9 for k in range(2))
    # "auto" time stamps: the same frames, the duration from the audio's length
    al.set_config(time_stamps="auto")
    try:
        auto = al(speech, text, name="rec")
    finally:
        al.set_config(time_stamps="fixed")
    assert auto.index_duration == len(speech) / 16000 / n_fr and np.array_equal(auto.first_frame, task.first_frame)


def test_full_span_path_starts_every_token_where_the_greedy_path_shows_it(aligner):
    """The fixture's posteriors are peaked by a margin, not close to 1 (V = 5 000): with a free preamble and a free end
    the best route is a short one.  Held to the whole recording (no free preamble, back-trace from the last frame) it is
    the greedy path: every token starts in the frame the arg-max first shows it - but the first one, which the fixture
    shows in frame 0, where the separator in front of it needs a frame."""
    from tests.helpers import golden_speech

    g, _, al = aligner
    speech = golden_speech(g)[0][0].numpy()
    text, _ = utterance_text(g, al.converter)
    n_fr = int(g["enc_olens"][0])
    al.set_config(preamble_transition_cost_zero=False, backtrack_from_max_t=True)
    try:
        task = al(speech, text)
        r, segs = restated(al, speech, task, task.window)
    finally:
        al.set_config(preamble_transition_cost_zero=True, backtrack_from_max_t=False)
    assert_task_equals(task, r, segs)
    ids = g["ctc_ids"][0, :n_fr].tolist()
    onsets = [f for f in range(n_fr) if ids[f] != al.asr_model.blank_id and (f == 0 or ids[f] != ids[f - 1])]
    tok_cols = [c for c in range(1, len(task.ground_truth_mat)) if c not in task.utt_begin_indices]
    assert task.t_end == n_fr and onsets[0] == 0
    toks = [task.ground_truth_mat[c] for c in tok_cols]
    fresh = [i for i in range(1, len(toks)) if toks[i] != toks[i - 1]]  # (a repeated token may begin while its twin still peaks)
    assert len(fresh) >= len(toks) - 3 and int(task.first_frame[tok_cols[0]]) == 1
    assert [int(task.first_frame[tok_cols[i]]) for i in fresh] == [onsets[i] for i in fresh]
    assert all(s < e for s, e, _ in task.segments)


def test_batch_call_rows_equal_the_single_calls(aligner):
    from tests.helpers import golden_speech

    g, _, al = aligner
    speech = golden_speech(g)[0][0]
    n = int(speech.numel())
    text, _ = utterance_text(g, al.converter)
    short_text, _ = utterance_text(g, al.converter, n_utts=2, n_tok=8)
    cut = (n * 3) // 5
    batch = torch.zeros(2, n)
    batch[0], batch[1, :cut] = speech, speech[:cut]
    tasks = al.batch_call(batch, [n, cut], [text, short_text], ["full", "cut"])
    singles = [al(speech.numpy(), text, name="full"), al(speech[:cut].numpy(), short_text, name="cut")]
    assert tasks[0].lpz_frames > tasks[1].lpz_frames > 0
    for a, b in zip(tasks, singles):
        assert np.array_equal(a.first_frame, b.first_frame) and a.frame_lp.tobytes() == b.frame_lp.tobytes()
        assert (a.t_end, a.total, a.status, a.segments) == (b.t_end, b.total, b.status, b.segments) and str(a) == str(b)
    with pytest.raises(ValueError, match="texts"):
        al.batch_call([speech], None, [text, text])
    with pytest.raises(ValueError, match="cannot carry"):
        al(speech[:6400].numpy(), text)  # 10 frames for 30 tokens: refused on the host
    assert al(speech.numpy(), text, name="x").segments == singles[0].segments  # and nothing of the batch lingers


def test_window_doubles_while_the_path_is_clipped(aligner):
    from tests.helpers import golden_speech

    g, _, al = aligner
    speech = golden_speech(g)[0][0].numpy()
    text, _ = utterance_text(g, al.converter)
    want = al(speech, text)
    al.set_config(min_window_size=4)
    try:
        task = al(speech, text)
        first, _ = restated(al, speech, task, 4)
        assert first["status"] == R.CLIPPED  # the first run clips (and has a route)
        assert task.window > 4 and task.window & (task.window - 1) == 0 and not task.clipped
        r, segs = restated(al, speech, task, task.window)
        assert_task_equals(task, r, segs)
        assert want.window == min(8000, 8192) and not want.clipped  # (the whole table: nothing to clip)
        al.set_config(min_window_size=2, max_window_size=4)  # still clipped at the largest window allowed: kept, and said
        capped = al(speech, text)
        assert capped.window == 4 and capped.clipped
        r, segs = restated(al, speech, capped, 4)
        assert_task_equals(capped, r, segs)
    finally:
        al.set_config(min_window_size=8000, max_window_size=None)


def test_three_partitions_have_the_expected_frames(aligner):
    from espnet_amd.bin.asr_align import get_partitions
    from espnet_amd.nets_utils import conv_out_size
    from tests.helpers import golden_speech

    g, _, al = aligner
    speech = golden_speech(g)[0][0].numpy()
    text, _ = utterance_text(g, al.converter)
    whole = al(speech, text)
    keep = al.longest_audio_segments
    al.longest_audio_segments = 4.0  # F = 100 body frames of 640 samples, 30 more on each inner side
    try:
        parts = al._partitions(len(speech))
        assert parts == get_partitions(len(speech), 640, 100, 30) and len(parts) == 3
        want_T = sum(conv_out_size(1 + (s1 - s0) // 160) - head - tail for s0, s1, head, tail in parts)
        task = al(speech, text)
    finally:
        al.longest_audio_segments = keep
    assert task.lpz_frames == want_T and abs(want_T - whole.lpz_frames) <= 3
    assert len(task.segments) == 3 and task.status & R.NO_ROUTE == 0
    assert al._partitions(len(speech)) == [(0, len(speech), 0, 0)]


def test_cli_writes_the_lines_of_the_task(aligner, tmp_path, capsys):
    from espnet_amd.bin import asr_align as AA
    from espnet_amd.fileio.sound_scp import write_wav_pcm16
    from tests.helpers import golden_speech

    g, d, al = aligner
    speech = golden_speech(g)[0][0].numpy()
    write_wav_pcm16(tmp_path / "rec7.wav", speech, 16000)
    text, _ = utterance_text(g, al.converter)
    (tmp_path / "text").write_text(text)
    samples, rate = AA.read_audio(tmp_path / "rec7.wav")
    assert rate == 16000 and samples.dtype == np.float32 and len(samples) == len(speech)
    want = str(al(samples, text, name="rec7"))
    args = ["--asr_train_config", str(d / "config.yaml"), "--asr_model_file", str(d / "model.pth"), "--audio",
            str(tmp_path / "rec7.wav"), "--text", str(tmp_path / "text"), "--time_stamps", "fixed", "--dtype", al.asr_model.ctc.compute_dtype]
    AA.main(args + ["--output", str(tmp_path / "segments")])
    assert (tmp_path / "segments").read_text() == want and want.count("\n") == 3
    AA.main(args)
    assert capsys.readouterr().out == want
    AA.main(args + ["--output", str(tmp_path / "bare"), "--print_utt_text", "false", "--print_utt_score", "false"])
    assert (tmp_path / "bare").read_text().splitlines() == [" ".join(ln.split()[:4]) for ln in want.splitlines()]
