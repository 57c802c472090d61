"""CTC segmentation without a GPU: the NumPy restatement of the contract (tests/ctc_segment_ref.py) pinned by hand on
tables small enough to write out, the host arithmetic of espnet_amd/bin/asr_align.py (segments, confidence, ground truth,
partitions, the segments file), the refusals, the bindings, and the precondition of the GPU tests: on every seed and shape
they use below the cap, the float32 and the float64 restatement walk the same path."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ctc_segment_ref as R

REPO = Path(__file__).resolve().parent.parent
HI, LO = -0.25, -4.0  # exact in f32, and so is every sum of a few of them
BL, A, B_, N = 0, 1, 2, 3


def table(peaks, hi=HI):
    """(T, 4) log-'probabilities': HI on the frame's peak, LO elsewhere (the trellis does not need them normalised)."""
    lp = np.full((len(peaks), 4), LO, np.float32)
    for f, v in enumerate(peaks):
        lp[f, v] = hi
    return lp


GT = [0, A, B_, BL]  # start, a, b, the closing separator
PEAKS = [N, N, A, BL, B_, BL]


# ------------------------------------------------------------------ the restatement, by hand
def test_t6_c4_preamble_free():
    """Two noise frames are skipped for nothing: a enters at frame 2 (0 - 0.25), stays over the blank frame (its stay
    takes max(blank, a) = -0.25), b at frame 4, the separator at frame 5: four times -0.25."""
    r = R.segment_ref(table(PEAKS), GT, BL, W=4)
    assert r["first_frame"].tolist() == [0, 2, 4, 5] and r["frame_col"].tolist() == [-1, -1, 1, 1, 2, 3]
    assert r["frame_lp"].tolist() == [0, 0, HI, HI, HI, HI]
    assert r["t_end"] == 6 and r["total"] == -1.0 and r["status"] == 0  # the path ends on the TABLE's edge: not clipped


def test_t6_c4_without_preamble_free_and_the_strict_tie():
    """Column 0 now pays the blank: k[2][0] = -8.  At (3, 1) switch = -8 + a = -8.25 and stay = k[2][1] - 0.25 with
    k[2][1] = -8 (a entered at frame 0 for -4, stayed for max(-4, -4)): a tie, and stay wins.  At (2, 1) switch = k[1][0] +
    lp[1][a] = -8 = stay: stay again.  So a starts in frame 0, not in frame 2."""
    r = R.segment_ref(table(PEAKS), GT, BL, W=4, flags=0)
    assert r["first_frame"].tolist() == [0, 0, 4, 5] and r["frame_col"].tolist() == [1, 1, 1, 1, 2, 3]
    assert r["frame_lp"].tolist() == [LO, LO, HI, HI, HI, HI]
    assert r["t_end"] == 6 and r["total"] == -9.0 and r["status"] == 0
    assert r["margin"] == 3.75  # the smallest non-zero |switch - stay| on the path: (1, 1) is -inf, ties are 0
    # a quarter less for the entry in frame 0 and the tie at (2, 1) is gone: a starts in frame 1 (the tie at (3, 1) stands)
    lp = table(PEAKS)
    lp[0, A] = LO - 0.25
    assert R.segment_ref(lp, GT, BL, W=4, flags=0)["first_frame"].tolist() == [0, 1, 4, 5]


def test_lowest_t_among_equal_last_column_values_and_from_last_frame():
    """A seventh frame whose blank costs 0: k[7][3] = k[6][3] exactly.  The lowest t wins; FROM_LAST_FRAME takes 7."""
    lp = np.concatenate([table(PEAKS), table([BL], hi=0.0)])
    r = R.segment_ref(lp, GT, BL, W=4)
    assert r["t_end"] == 6 and r["total"] == -1.0 and r["frame_col"].tolist() == [-1, -1, 1, 1, 2, 3, -1]
    assert r["frame_lp"][6] == 0 and r["first_frame"].tolist() == [0, 2, 4, 5]
    r = R.segment_ref(lp, GT, BL, W=4, flags=R.PREAMBLE_FREE | R.FROM_LAST_FRAME)
    assert r["t_end"] == 7 and r["total"] == -1.0 and r["frame_col"].tolist() == [-1, -1, 1, 1, 2, 3, 3]
    # without the free frame the earlier end is strictly better, FROM_LAST_FRAME still takes the last row
    r = R.segment_ref(np.concatenate([table(PEAKS), table([N])]), GT, BL, W=4, flags=R.PREAMBLE_FREE | R.FROM_LAST_FRAME)
    assert r["t_end"] == 7 and r["total"] == -1.0 + LO and r["frame_lp"][6] == np.float32(LO)


def edges_touched(r, T, C, W):
    Wb, lower, upper = min(W, C), [], []
    for f, c in enumerate(r["frame_col"].tolist()):
        lo = R.band_lo(f + 1, T, C, Wb)
        if c > 0 and c == lo and lo > 0:
            lower.append(f + 1)
        if c > 0 and c == lo + Wb - 1 and lo + Wb < C:
            upper.append(f + 1)
    return lower, upper


def test_two_row_band_slide_and_the_clipped_flag():
    """W = 2 over C = 4, T = 6: the band holds [0, 1] in rows 1-2, [1, 2] in rows 3-4, [2, 3] in rows 5-6."""
    assert [R.band_lo(t, 6, 4, 2) for t in range(7)] == [0, 0, 0, 1, 1, 2, 2]
    r = R.segment_ref(table(PEAKS), GT, BL, W=2)
    # the same path as unbanded - column 0 leaves the band behind row 2, a enters from it in row 3 - but it sits on the
    # band's lower edge in rows 3, 4 (column 1) and 5 (column 2)
    assert r["first_frame"].tolist() == [0, 2, 4, 5] and r["total"] == -1.0 and r["status"] == R.CLIPPED
    assert edges_touched(r, 6, 4, 2) == ([3, 4, 5], [])
    # a at frame 0, b at frame 2, the separator from frame 4: upper edge in rows 1-4, rows 5-6 lie on the table's edge
    r = R.segment_ref(table([A, BL, B_, BL, BL, BL]), GT, BL, W=2)
    assert r["first_frame"].tolist() == [0, 0, 2, 4] and r["t_end"] == 5 and r["status"] == R.CLIPPED
    assert edges_touched(r, 6, 4, 2) == ([], [1, 2, 3, 4])
    # the band as wide as the table: the same cells, no flag
    assert R.segment_ref(table([A, BL, B_, BL, BL, BL]), GT, BL, W=4)["status"] == 0
    # a path the band cannot hold: b peaks in frame 0 and 1 only, a before it is impossible, so the band decides
    wide, narrow = (R.segment_ref(table([N, N, N, N, A, B_]), [0, A, B_], BL, W=w) for w in (3, 1))
    assert wide["first_frame"].tolist() == [0, 4, 5] and wide["status"] == 0
    assert narrow["status"] & R.CLIPPED and narrow["first_frame"].tolist() != wide["first_frame"].tolist()


def test_no_route():
    r = R.segment_ref(table([A, B_]), GT, BL, W=4)  # three columns behind the start, two frames
    assert r["status"] == R.NO_ROUTE and r["t_end"] == 0 and np.isneginf(r["total"])
    assert r["first_frame"].tolist() == [-1] * 4 and r["frame_col"].tolist() == [-1, -1] and r["frame_lp"].tolist() == [0, 0]
    o = R.segment_ref_batch([table(PEAKS), table([A, B_])], [GT, GT], 8, 6, BL, 4)
    assert o["status"].tolist() == [0, 1] and o["first_frame"][0].tolist() == [0, 2, 4, 5, -1, -1]
    assert o["frame_col"][0].tolist() == [-1, -1, 1, 1, 2, 3, -1, -1] and (o["frame_col"][1] == -1).all()


def test_float32_and_float64_walk_the_same_paths_on_the_gpu_tests_inputs():
    """The condition that lets tests/test_gpu_ctc_segment.py demand exact paths of a float32 kernel."""
    keys = ("first_frame", "frame_col", "t_end", "status")

    def same(lp, gt, blank, W, flags, tag):
        a, b = (R.segment_ref(lp, gt, blank, W, flags, dt, margin=False) for dt in (np.float32, np.float64))
        assert all(np.array_equal(a[k], b[k]) for k in keys), tag
        if a["status"] & R.NO_ROUTE == 0:
            assert abs(float(a["total"]) - float(b["total"])) <= 1e-3 * max(1.0, abs(float(b["total"]))), tag

    for name, cfg in R.GPU_CASES.items():
        if name in R.LARGE_CASES:
            continue
        lp, gt, _ = R.make_case(cfg)
        for flags in ((0, 1, 2, 3) if name.startswith("b_") else (1,)):
            same(lp, gt, 0, cfg["W"], flags, (name, flags))
        if name[0] in "ab" and name[1] == "_":
            lp, gt, _ = R.make_case(cfg, blank=R.VOCAB - 1)
            same(lp, gt, R.VOCAB - 1, cfg["W"], 1, (name, "blank last"))
    for cfg in R.RAGGED:
        lp, gt, _ = R.make_case(cfg)
        for W in (96, 600):
            same(lp, gt, 0, W, 1, (cfg["seed"], W))


def test_planted_cases_are_found_and_an_unclipped_band_equals_the_table():
    for name in ("a_one_wave_no_slide", "b_one_wave_slide", "b2_one_wave_slots_wrap"):
        cfg = R.GPU_CASES[name]
        lp, gt, begin = R.make_case(cfg)
        r = R.segment_ref(lp, gt, 0, cfg["W"])
        assert r["status"] == 0 and r["first_frame"][1] >= cfg["pre"] and r["t_end"] <= cfg["T"] - cfg["post"] + 1
        full = R.segment_ref(lp, gt, 0, cfg["C"])
        assert np.array_equal(full["first_frame"], r["first_frame"]) and full["total"] == r["total"]
        assert begin[0] == 1 and begin[-1] == cfg["C"] - 1 and all(gt[i] == 0 for i in begin)


# ------------------------------------------------------------------ host arithmetic of the tool
def test_segments_and_all_three_confidence_branches():
    from espnet_amd.bin.asr_align import determine_segments

    # gt: start | sep a a | sep b b b ... | sep   with utt_begin [1, 4, 8]
    first_frame = np.array([0, 10, 12, 20, 30, 40, 50, 100, 110], np.int32)
    utt_begin = [1, 4, 8]
    frame_lp = -np.arange(120, dtype=np.float32) / 64
    dur = 0.04
    segs = determine_segments(first_frame, frame_lp, 111, utt_begin, dur, n=30)
    tm = first_frame * dur
    # utterance 0: start = max(tm[2] - 0.5, (tm[1] + tm[0]) / 2) = 0.2; end = min(tm[3] + 0.5, (tm[4] + tm[3]) / 2) = 1.0
    assert segs[0][0] == (tm[1] + tm[0]) / 2 == 0.2 and segs[0][1] == (tm[4] + tm[3]) / 2 == 1.0
    # frames [5, 25): 20 <= 30 frames: the plain mean
    assert segs[0][2] == pytest.approx(float(np.mean(frame_lp[5:25].astype(np.float64))), abs=1e-12)
    # utterance 1: start = max(1.6 - 0.5, (1.2 + 0.8) / 2) = 1.1 ; end = min(4.0 + 0.5, (4.4 + 4.0) / 2) = 4.2
    assert segs[1][0] == pytest.approx(1.1, abs=1e-12) and segs[1][1] == pytest.approx(4.2, abs=1e-12)
    s, e = int(np.floor(segs[1][0] / dur)), int(np.ceil(segs[1][1] / dur))
    assert e - s > 30
    want = min(float(np.mean(frame_lp[t:t + 30].astype(np.float64))) for t in range(s, e - 30 + 1))  # last window included
    assert segs[1][2] == pytest.approx(want, abs=1e-12) and want == pytest.approx(float(np.mean(frame_lp[e - 30:e].astype(np.float64))))
    # nothing left below t_end: -1e10
    assert determine_segments(first_frame, frame_lp, 20, utt_begin, dur, n=30)[1][2] == -1e10
    # the restatement's helper says the same
    for a, b in zip(segs, R.segments_ref(first_frame, frame_lp, 111, utt_begin, dur, 30)):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == pytest.approx(b[2], abs=1e-12)


def test_ground_truth_and_utt_begin():
    from espnet_amd.bin.asr_align import build_ground_truth

    gt, begin = build_ground_truth([[5, 6], [7], [8, 9, 5]], blank=0)
    assert gt == [0, 0, 5, 6, 0, 7, 0, 8, 9, 5, 0] and begin == [1, 4, 6, 10] and begin[-1] == len(gt) - 1
    assert (gt, begin) == R.build_gt([[5, 6], [7], [8, 9, 5]], 0)
    gt, begin = build_ground_truth([[1]], blank=3)
    assert gt == [3, 3, 1, 3] and begin == [1, 3]
    with pytest.raises(ValueError, match="utt_b.*no tokens"):
        build_ground_truth([[1], []], 0, ["utt_a", "utt_b"])
    with pytest.raises(ValueError, match="utt_a.*blank"):
        build_ground_truth([[1, 0]], 0, ["utt_a"])


def _shell(kaldi=True):
    from espnet_amd.bin.asr_align import CTCSegmentation
    from espnet_amd.text.token_id_converter import TokenIDConverter, build_tokenizer

    s = CTCSegmentation.__new__(CTCSegmentation)
    s.asr_model = types.SimpleNamespace(blank_id=0)
    s.tokenizer, s.converter = build_tokenizer(token_type="word"), TokenIDConverter(token_list=["<blank>", "a", "b", "<unk>", "<sos/eos>"])
    s.kaldi_style_text, s.print_utt_text, s.print_utt_score = kaldi, True, True
    return s


def test_refusals(monkeypatch):
    from espnet_amd.bin import asr_align as AA

    with pytest.raises(NotImplementedError, match="classic"):
        AA.CTCSegmentation(text_converter="classic")
    monkeypatch.setattr(AA.ASRTask, "build_model_from_file",
                        classmethod(lambda cls, *a, **k: (types.SimpleNamespace(ctc=None), types.SimpleNamespace())))
    with pytest.raises(ValueError, match="CTC head"):
        AA.CTCSegmentation(asr_train_config="x", asr_model_file="y")
    with pytest.raises(RuntimeError, match="MI355X"):
        AA.CTCSegmentation(device="cpu")
    s = _shell()
    with pytest.raises(ValueError, match="u2.*blank"):
        s.prepare_ground_truth("u1 a b\nu2 a <blank>")
    with pytest.raises(ValueError, match="u2.*no tokens"):
        s.prepare_ground_truth("u1 a b\nu2\n")
    with pytest.raises(NotImplementedError, match="gratis_blank"):
        s.set_config(gratis_blank=True)
    with pytest.raises(TypeError, match="no_such"):
        s.set_config(no_such=1)
    task = s.prepare_ground_truth(["u1 a b", "u2 b"])
    assert task.ground_truth_mat == [0, 0, 1, 2, 0, 2, 0] and task.utt_begin_indices == [1, 4, 6] and task.utt_ids == ["u1", "u2"]
    plain = _shell(kaldi=False).prepare_ground_truth("a b\nb", name="rec")
    assert plain.utt_ids == ["rec_0000", "rec_0001"] and plain.text == ["a b", "b"] and plain.ground_truth_mat == task.ground_truth_mat


def test_host_checks_of_the_trellis_arguments():
    from espnet_amd.asr.ctc import CTC

    CTC.check_segmentable([6], [[0, 1, 2, 0]], [4], vocab=4, T=6)
    for olens, gt, clens, msg in [([6], [[0]], [1], "columns"), ([2], [[0, 1, 2, 0]], [4], "cannot carry"),
                                  ([6], [[0, 1, 4]], [3], r"\[0, 4\)"), ([6], [[0, 1]], [3], "outside"),
                                  ([7], [[0, 1]], [2], "outside")]:
        with pytest.raises(ValueError, match=msg):
            CTC.check_segmentable(olens, gt, clens, vocab=4, T=6)
    CTC.check_segmentable([6], [[-7, 1]], [2], vocab=4, T=6)  # column 0 is never read
    ol, g, cl, Cmax = CTC._segment_inputs([6, 5], [[9, 1, 2, 0], [9, 3]], [4, 2], 4, 6, torch.device("cpu"))
    assert Cmax == 4 and g.tolist() == [[0, 1, 2, 0], [0, 3, 0, 0]] and ol.tolist() == [6, 5] and cl.tolist() == [4, 2]
    assert g.dtype == torch.int32


def test_task_prints_the_segments_file():
    from espnet_amd.bin.asr_align import CTCSegmentationTask

    t = CTCSegmentationTask("rec1", ["utt_a", "utt_b"], ["hello world", "again"], [], [])
    t.segments = [(0.204, 1.0, -0.123456), (1.1, 4.256, -1e10)]
    assert str(t) == "utt_a rec1 0.20 1.00 -0.1235 hello world\nutt_b rec1 1.10 4.26 -10000000000.0000 again\n"
    t.print_utt_text = False
    assert str(t) == "utt_a rec1 0.20 1.00 -0.1235\nutt_b rec1 1.10 4.26 -10000000000.0000\n"
    t.print_utt_score = False
    assert str(t) == "utt_a rec1 0.20 1.00\nutt_b rec1 1.10 4.26\n"


def test_partitions_keep_every_frame_once():
    from espnet_amd.bin.asr_align import get_partitions

    sps = 640
    assert get_partitions(160000, sps, 250, 30) == [(0, 160000, 0, 0)]  # one partition: the identity
    assert get_partitions(160000 + 639, sps, 250, 30) == [(0, 160639, 0, 0)]
    for n, F, ov in [(160000, 100, 30), (1000000, 500, 30), (640 * 1000 + 7, 250, 0), (640 * 333, 100, 30), (640 * 305, 100, 30)]:
        parts = get_partitions(n, sps, F, ov)
        assert parts[0][0] == 0 and parts[-1][1] == n and parts[0][2] == 0 and parts[-1][3] == 0
        kept = 0
        for i, (s0, s1, head, tail) in enumerate(parts):
            assert 0 <= s0 < s1 <= n and s0 % sps == 0
            assert head == (ov if i > 0 else 0) and tail == (ov if i < len(parts) - 1 else 0)
            if i > 0:  # the bodies tile the recording: this body begins where the one before ended
                p0, p1, _, ptail = parts[i - 1]
                assert s0 + head * sps == p1 - ptail * sps
            kept += (s1 - s0) // sps - head - tail
        assert kept == n // sps
    assert len(get_partitions(160000, sps, 100, 30)) == 3 and len(get_partitions(640 * 305, sps, 100, 30)) == 3  # 5 frames: merged


# ------------------------------------------------------------------ bindings
def test_the_entry_points_are_declared_and_bound():
    from espnet_amd import lib as L

    hdr = (REPO / "include" / "espnet_amd.h").read_text()
    for name in ("em_ctc_segment", "em_ctc_segment_workspace_bytes", "em_ctc_segment_max_window"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in L._SIGNATURES, name
    assert len(L._SIGNATURES["em_ctc_segment"][1]) == 20
    assert (L.EM_SEG_PREAMBLE_FREE, L.EM_SEG_FROM_LAST_FRAME, L.EM_SEG_NO_ROUTE, L.EM_SEG_CLIPPED) == (
        R.PREAMBLE_FREE, R.FROM_LAST_FRAME, R.NO_ROUTE, R.CLIPPED)
    for macro, val in (("EM_SEG_PREAMBLE_FREE", 1), ("EM_SEG_FROM_LAST_FRAME", 2), ("EM_SEG_NO_ROUTE", 1), ("EM_SEG_CLIPPED", 2)):
        assert re.search(rf"#define {macro} {val}\b", hdr), macro
    lib = L.load()
    assert lib.em_ctc_segment_max_window() == 8192
    assert lib.em_ctc_segment_workspace_bytes(1, 400, 300, 128) == 0  # one wave, 400 x 64 bytes: LDS
    assert lib.em_ctc_segment_workspace_bytes(2, 1700, 1500, 1100) == 2 * 1700 * 192
    assert lib.em_ctc_segment_workspace_bytes(1, 9000, 8600, 8192) == 9000 * 1024
    assert lib.em_ctc_segment_workspace_bytes(1, 9000, 8600, 8193) == 0 and lib.em_ctc_segment_workspace_bytes(1, 9000, 1, 4) == 0
