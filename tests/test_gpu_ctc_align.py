"""CTC forced alignment on the device (csrc/ctc_align.hip) through the C ABI and the host layer, against the CPU
restatement of the contract (tests/ctc_align_ref.py).

The trellis does one f32 add per cell and comparisons, and so does the restatement: align, frame_lp, total and the
spans must be BIT-EQUAL; tok_lp gets 1 ulp for its one division.  Shapes are the smallest that reach every path of the
kernel: S around the 8-state lane runs and the 64-lane wave (L = 31 .. 64), around the one-wave tier (L = 255 / 256),
back-pointers in LDS and in the workspace, a back-trace of more than one chunk, frame counts that end inside a group of
four prefetched frames, unaligned utterance starts in a ragged batch."""

import numpy as np
import pytest
import torch

from tests.ctc_align_ref import forced_align_ref, forced_align_ref_batch
from tests.helpers import golden_speech, golden_state_dict, load_golden

pytestmark = pytest.mark.gpu

V = 50
KEYS = ("align", "frame_lp", "total", "tok_start", "tok_end", "tok_lp")


def synth_lp(T, seed, vocab=V):
    return torch.log_softmax(torch.randn(T, vocab, generator=torch.Generator().manual_seed(seed)), dim=-1)


def synth_y(L, seed, distinct=False, vocab=V):
    g = torch.Generator().manual_seed(1000 + seed)
    if distinct:
        return (torch.randperm(vocab - 1, generator=g)[:L] + 1).tolist()
    return torch.randint(1, vocab, (L,), generator=g).tolist()


def device_align(lps, ys, T=None, blank=0, ws_bytes=None):
    """Rows (T_b, V) + targets -> the six device outputs on the host, through CTC.align_log_probs_t."""
    from espnet_amd.asr.ctc import CTC

    B = len(lps)
    T = T or max(lp.shape[0] for lp in lps)
    Lmax = max(len(y) for y in ys)
    vocab = lps[0].shape[1]
    lpT = torch.zeros(vocab, B * T)
    tg = torch.zeros(B, max(Lmax, 1), dtype=torch.int32)
    for b, (lp, y) in enumerate(zip(lps, ys)):
        lpT[:, b * T : b * T + lp.shape[0]] = lp.t()
        tg[b, : len(y)] = torch.tensor(y, dtype=torch.int32)
    olens = torch.tensor([lp.shape[0] for lp in lps], dtype=torch.int32).cuda()
    ylens = torch.tensor([len(y) for y in ys], dtype=torch.int32).cuda()
    out = CTC.align_log_probs_t(lpT.cuda(), B * T, olens, tg[:, :Lmax].contiguous().cuda() if Lmax else tg.cuda(), Lmax,
                                ylens, B, T, blank, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in zip(("align", "frame_lp", "tok_start", "tok_end", "tok_lp", "total"), out)}


def assert_same(got, want, tag):
    for k in ("align", "tok_start", "tok_end"):
        assert torch.equal(got[k], want[k]), (tag, k)
    for k in ("frame_lp", "total"):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (tag, k)
    ulp = (got["tok_lp"].view(torch.int32) - want["tok_lp"].view(torch.int32)).abs()
    assert int(ulp.max()) <= 1 if ulp.numel() else True, (tag, "tok_lp", int(ulp.max()))


def check_batch(rows, tag, T=None):
    lps = [synth_lp(t, 31 * i + t) for i, (t, _) in enumerate(rows)]
    ys = [y for _, y in rows]
    T = T or max(t for t, _ in rows)
    got = device_align(lps, ys, T)
    assert_same(got, forced_align_ref_batch(lps, ys, T, max(len(y) for y in ys)), tag)
    return lps, ys, got


# ------------------------------------------------------------------ kernel against restatement
def test_tiny_shapes_one_ragged_batch():
    a = 7
    rows = [(1, []), (1, [3]), (5, []), (2, [4]), (7, synth_y(7, 1, distinct=True)), (5, [a, a, a]), (3, [9]),
            (17, synth_y(5, 2))]
    check_batch(rows, "tiny")


def test_lane_run_and_wave_edges():
    check_batch([(130, synth_y(L, L)) for L in (31, 32, 33, 63, 64)], "T130")


def test_one_wave_tier_edge():
    check_batch([(300, synth_y(255, 5))], "L255")  # S = 511: one wave, back-pointers in LDS
    check_batch([(300, synth_y(256, 6)), (300, synth_y(255, 5)), (41, synth_y(3, 7))], "L256")  # S = 513: two waves, workspace


def test_multi_wave_long_transcript_workspace_back_trace():
    from espnet_amd import lib as L

    assert L.load().em_ctc_forced_align_workspace_bytes(1, 3000, 700) > 0
    check_batch([(3000, synth_y(700, 8))], "T3000")


def test_ten_second_shape_and_odd_frame_counts():
    check_batch([(249, synth_y(60, 9)), (251, synth_y(20, 10)), (3, [5]), (17, synth_y(4, 11))], "T251")
    check_batch([(249, synth_y(60, 9))], "T249 alone")  # an odd row stride: the 4-byte load path


def test_ragged_batch_rows_equal_the_rows_alone():
    rows = [(40, synth_y(11, 20)), (23, []), (57, synth_y(19, 21)), (9, synth_y(4, 22)), (64, synth_y(30, 23))]
    lps, ys, got = check_batch(rows, "ragged", T=66)
    for b, (t, y) in enumerate(rows):
        assert (got["align"][b, t:] == -1).all() and (got["frame_lp"][b, t:] == 0).all()
        assert (got["tok_start"][b, len(y):] == -1).all() and (got["tok_end"][b, len(y):] == -1).all()
        assert (got["tok_lp"][b, len(y):] == 0).all()
        alone = device_align([lps[b]], [ys[b]])
        for k in KEYS:
            n = t if k in ("align", "frame_lp") else len(y)
            mine = got[k][b] if k == "total" else got[k][b, :n]
            other = alone[k][0] if k == "total" else alone[k][0, :n]
            assert torch.equal(mine, other), (b, k)


# ------------------------------------------------------------------ ties and repeatability
@pytest.mark.parametrize("kind", ["uniform", "quantised"])
def test_exact_ties_follow_the_contract(kind):
    rows = [(5, [1, 2]), (4, [1, 1]), (60, synth_y(20, 30)), (130, synth_y(64, 31))]
    if kind == "uniform":
        lps = [torch.full((t, V), float(np.log(1.0 / V))) for t, _ in rows]
    else:
        lps = [torch.round(synth_lp(t, 77 + t) * 4) / 4 for t, _ in rows]
    ys = [y for _, y in rows]
    got = device_align(lps, ys)
    assert_same(got, forced_align_ref_batch(lps, ys, 130, 64), kind)
    if kind == "uniform":
        assert got["align"][0, :5].tolist() == [1, 2, 2, 2, 2] and got["align"][1, :4].tolist() == [1, 0, 1, 1]
    again = device_align(lps, ys)
    for k in KEYS:
        assert torch.equal(got[k], again[k]), k


# ------------------------------------------------------------------ limits
def _raw_call(lpT, ldT, olens, tg, Lmax, ylens, B, T, ws=None, ws_bytes=0):
    from espnet_amd import lib as L

    dev = lpT.device
    o = dict(align=torch.zeros(B, T, dtype=torch.int32, device=dev), frame_lp=torch.ones(B, T, device=dev),
             tok_start=torch.zeros(B, max(Lmax, 1), dtype=torch.int32, device=dev),
             tok_end=torch.zeros(B, max(Lmax, 1), dtype=torch.int32, device=dev),
             tok_lp=torch.ones(B, max(Lmax, 1), device=dev), total=torch.zeros(B, device=dev))
    rc = L.load().em_ctc_forced_align(L.ptr(lpT), ldT, L.ptr(olens), L.ptr(tg), Lmax, L.ptr(ylens), B, T, 0,
                                      L.ptr(o["align"]), L.ptr(o["frame_lp"]), L.ptr(o["tok_start"]), L.ptr(o["tok_end"]),
                                      L.ptr(o["tok_lp"]), L.ptr(o["total"]), L.ptr(ws), ws_bytes, L.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in o.items()}


def test_limits_and_argument_errors():
    from espnet_amd import lib as L

    lib = L.load()
    most = int(lib.em_ctc_forced_align_max_tokens())  # the limit the library states: taken itself, refused one above
    assert most >= 2047
    one = torch.ones(1, dtype=torch.int32).cuda()
    lp8 = synth_lp(8, 1)
    lpT = lp8.t().contiguous().cuda()
    rc, o = _raw_call(lpT, 8, one * 8, torch.full((1, most), 3, dtype=torch.int32).cuda(), most, one, 1, 8)
    assert rc == 0 and torch.equal(o["align"][0], forced_align_ref(lp8, [3])["align"])
    rc, _ = _raw_call(lpT, 8, one * 8, torch.ones(1, most + 1, dtype=torch.int32).cuda(), most + 1, one, 1, 8)
    with pytest.raises(NotImplementedError):
        L.check(rc, "em_ctc_forced_align")
    # a short workspace
    T, Lm = 300, 256
    need = int(lib.em_ctc_forced_align_workspace_bytes(1, T, Lm))
    assert need > 0 and int(lib.em_ctc_forced_align_workspace_bytes(1, 249, 120)) == 0
    lp = synth_lp(T, 3).t().contiguous().cuda()
    ws = torch.empty(need, dtype=torch.uint8).cuda()
    tg = torch.tensor([synth_y(Lm, 6)], dtype=torch.int32).cuda()
    rc, _ = _raw_call(lp, T, one * T, tg, Lm, one * Lm, 1, T, ws, need - 1)
    assert rc == L.EM_ERR_WORKSPACE
    with pytest.raises(L.EspnetAmdError):
        L.check(rc, "em_ctc_forced_align")
    # null pointers, a negative Lmax, a row stride below B * T
    assert lib.em_ctc_forced_align(None, 8, None, None, 0, None, 1, 8, 0, None, None, None, None, None, None, None, 0,
                                   None) == L.EM_ERR_BAD_ARG
    rc, _ = _raw_call(lpT, 8, one * 8, one, -1, one, 1, 8)
    assert rc == L.EM_ERR_BAD_ARG
    rc, _ = _raw_call(lpT, 7, one * 8, one, 1, one, 1, 8)
    assert rc == L.EM_ERR_BAD_ARG


def test_infeasible_row_is_a_defined_result():
    """The host raises for such a row before launching; the kernel itself must still answer safely: total -inf,
    labels -1 - next to a feasible row that is aligned as usual."""
    lps = [synth_lp(2, 40), synth_lp(6, 41)]
    lpT = torch.zeros(V, 12)
    lpT[:, 0:2], lpT[:, 6:12] = lps[0].t(), lps[1].t()
    tg = torch.tensor([[3, 3], [4, 5]], dtype=torch.int32).cuda()  # [3, 3] needs 3 frames, has 2
    olens = torch.tensor([2, 6], dtype=torch.int32).cuda()
    ylens = torch.tensor([2, 2], dtype=torch.int32).cuda()
    rc, o = _raw_call(lpT.cuda(), 12, olens, tg, 2, ylens, 2, 6)
    assert rc == 0
    assert o["total"][0] == float("-inf") and (o["align"][0] == -1).all() and (o["frame_lp"][0] == 0).all()
    assert (o["tok_start"][0] == -1).all() and (o["tok_end"][0] == -1).all() and (o["tok_lp"][0] == 0).all()
    want = forced_align_ref(lps[1], [4, 5])
    assert torch.equal(o["align"][1], want["align"]) and torch.equal(o["total"][1], want["total"])


# ------------------------------------------------------------------ through the model
def build(g, dtype):
    from espnet_amd.tasks.asr import ASRTask

    cfg = dict(g["config"])
    cfg["compute_dtype"] = dtype
    model = ASRTask.build_model(cfg)
    model.load_state_dict(golden_state_dict(g), strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_peaked_model_alignment_is_the_arg_max_path(dtype):
    """Every frame of the fixture is decided by a reference margin > 1, so the arg-max path is the unique optimum of the
    trellis for its own collapsed tokens - in bf16 too."""
    g = load_golden("small_10s_peaked")
    sos_eos = int(g["vocab"]) - 1
    n_fr, n_tok = int(g["enc_olens"][0]), int(g["g1_lens"][0])
    assert not (g["ctc_ids"][0, :n_fr] == sos_eos).any()  # precondition: no <sos/eos> frame (collapse drops those)
    assert float(g["ctc_margin"][0, :n_fr].min()) > 1.0
    model = build(g, dtype)
    speech, lens = golden_speech(g)
    st = model.encode_device(speech.cuda(), lens.tolist())
    y = g["g1_tokens"][:, :n_tok].tolist()
    align, frame_lp, ts, te, tlp, total = model.ctc.forced_align_device(st.enc_act, st.olens, y, [n_tok], model.blank_id)
    assert align.dtype == torch.int32 and align.is_cuda
    assert align[0, :n_fr].cpu().tolist() == g["ctc_ids"][0, :n_fr].tolist()
    ids64 = model.ctc.forced_align(st.enc_out, torch.tensor(st.olens), torch.tensor(y), torch.tensor([n_tok]))
    assert ids64.dtype == torch.int64 and ids64[0, :n_fr].cpu().tolist() == g["ctc_ids"][0, :n_fr].tolist()
    ts, te = ts[0].cpu().tolist(), te[0].cpu().tolist()
    assert all(0 <= s < e <= n_fr for s, e in zip(ts, te)) and all(te[i] <= ts[i + 1] for i in range(n_tok - 1))
    assert abs(float(total[0]) - float(frame_lp[0, :n_fr].sum())) < 1e-2
    from espnet_amd.lib import EspnetAmdError

    with pytest.raises(EspnetAmdError):
        model.ctc.forced_align(st.enc_out.cpu(), torch.tensor(st.olens), torch.tensor(y), torch.tensor([n_tok]))
    with pytest.raises(ValueError):  # more tokens than frames: raised on the host
        model.ctc.forced_align_device(st.enc_act, [5], [list(range(1, 9))], [8], model.blank_id)


@pytest.fixture(scope="module")
def s2t_pair(tmp_path_factory):
    from espnet_amd.bin.asr_inference import Speech2Text

    g = load_golden("small_10s_peaked")
    d = tmp_path_factory.mktemp("align_model")
    (d / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), d / "model.pth")
    s2t = Speech2Text(asr_train_config=str(d / "config.yaml"), asr_model_file=str(d / "model.pth"), device="cuda",
                      dtype="bfloat16", ctc_greedy=True)
    return g, s2t


def test_speech2text_align_own_hypothesis(s2t_pair):
    g, s2t = s2t_pair
    speech, _ = golden_speech(g)
    res = s2t.align(speech[0].numpy(), None)
    text, token, token_int, _ = s2t(speech[0].numpy())[0]
    assert [t[1] for t in res["tokens"]] == token_int and [t[0] for t in res["tokens"]] == token
    n_fr = int(g["enc_olens"][0])
    spf = s2t.seconds_per_frame
    assert spf == pytest.approx(4 * 160 / 16000)
    assert res["frame_labels"].dtype == torch.int64 and res["frame_labels"].tolist() == g["ctc_ids"][0, :n_fr].tolist()
    prev_end = 0.0
    for tok, tid, s, e, lp in res["tokens"]:
        assert 0.0 <= s and prev_end <= s < e <= n_fr * spf + 1e-9 and lp <= 0.0
        prev_end = e
    assert np.isfinite(res["total"]) and res["total"] < 0
    # the same transcript given as ids (checked on the host) and as text
    again = s2t.align(speech[0].numpy(), token_int)
    assert again["tokens"] == res["tokens"] and again["total"] == res["total"]
    assert s2t.tokenizer is not None and isinstance(text, str) and s2t._target_ids(text) == token_int  # (word tokens)
    as_text = s2t.align(speech[0].numpy(), text)
    assert as_text["tokens"] == res["tokens"] and as_text["total"] == res["total"]


# Two bf16 encodings of one utterance at different launch shapes (alone / inside a ragged batch) are not bit-identical.
# The suite bounds a bf16 CTC log-prob at 4e-3 from the f32 reference's (tests/test_gpu_search.py BF16_EPS["ctc"]), so two
# bf16 runs lie within 8e-3 of each other per frame, and so do the MEAN log-probs of a span.  Everything discrete (tokens,
# ids, spans, frame labels) must be equal: the peaked fixture decides every frame by > 1.  The floats of a batch row are
# checked exactly where that is possible: against the restatement on the row's own device lpT
# (test_batch_align_rows_bit_equal_to_restatement_on_their_own_log_probs).
BF16_PAIR_EPS = 8e-3


def assert_same_alignment(a, b, tag):
    assert [t[:4] for t in a["tokens"]] == [t[:4] for t in b["tokens"]], tag
    assert torch.equal(a["frame_labels"], b["frame_labels"]), tag
    worst = max((abs(x[4] - y[4]) for x, y in zip(a["tokens"], b["tokens"])), default=0.0)
    print(f"[{tag}] largest mean-logp difference {worst:.3e}, total {a['total']:.4f} vs {b['total']:.4f}")
    assert worst <= BF16_PAIR_EPS, (tag, worst)


def three_cuts(g):
    speech, lens = golden_speech(g)
    n = int(lens[0])
    cuts = [n, (n * 3) // 5, n // 3]
    batch = torch.zeros(3, n)
    for b, c in enumerate(cuts):
        batch[b, :c] = speech[0, :c]
    return speech, batch, cuts


def test_batch_align_equals_single_calls(s2t_pair):
    g, s2t = s2t_pair
    speech, batch, cuts = three_cuts(g)
    res = s2t.batch_align(batch, cuts)
    for b, c in enumerate(cuts):
        one = s2t.align(speech[0, :c].numpy(), None)
        if b == 0:  # (the longest row: no padding, the same launch shapes as alone but for the batch size)
            assert len(one["tokens"]) == int(g["g1_lens"][0])
        assert_same_alignment(res[b], one, f"batch row {b}")


def test_batch_align_rows_bit_equal_to_restatement_on_their_own_log_probs(s2t_pair):
    """What `batch_align` returns for a ragged batch, floats included, against the restatement run on the log-probs the
    device computed for that very batch: `total` bit-equal, `mean_logp` within 1 ulp (its division), spans equal."""
    from espnet_amd import lib as L

    g, s2t = s2t_pair
    _, batch, cuts = three_cuts(g)
    res = s2t.batch_align(batch, cuts)
    m = s2t.asr_model
    st = m.encode_device(batch.cuda(), cuts, isolate=True)
    B, T, d = st.enc_act.shape
    p = m.ctc.packed(st.enc_act.device)
    lpT = torch.empty(m.ctc.odim, B * T, dtype=torch.float32, device="cuda")
    L.check(L.load().em_ctc_log_probs_t(m.ctc.em_dtype, L.ptr(st.enc_act), B, T, d, L.ptr(p.weight), L.ptr(p.bias),
                                        m.ctc.odim, L.ptr(lpT), L.current_stream_ptr()), "em_ctc_log_probs_t")
    lpT = lpT.cpu()
    spf = s2t.seconds_per_frame
    assert st.olens[0] > st.olens[1] > st.olens[2] > 0
    for b in range(B):
        y = [t[1] for t in res[b]["tokens"]]
        want = forced_align_ref(lpT[:, b * T : b * T + st.olens[b]].t().contiguous(), y, m.blank_id)
        assert res[b]["total"] == float(want["total"]), b
        assert res[b]["frame_labels"].tolist() == want["align"].tolist(), b
        for i, (_, _, s, e, lp) in enumerate(res[b]["tokens"]):
            assert s == float(want["tok_start"][i]) * spf and e == float(want["tok_end"][i]) * spf, (b, i)
            ulp = abs(int(np.float32(lp).view(np.int32)) - int(want["tok_lp"][i].view(torch.int32)))
            assert ulp <= 1, (b, i, lp, float(want["tok_lp"][i]))


def test_hypothesis_rows_cut_to_the_longest_give_the_same_result(s2t_pair):
    """texts=None beyond `align_no_sync_frames` encoder frames: the token rows are cut to the longest hypothesis before the
    launch (fewer waves, less workspace), so the kernel's Lmax and the packed host row change - the results must not."""
    g, s2t = s2t_pair
    _, batch, cuts = three_cuts(g)
    assert int(g["enc_olens"][0]) <= s2t.align_no_sync_frames  # the other tests take the uncut route
    want = s2t.batch_align(batch, cuts)
    try:
        s2t.align_no_sync_frames = 100  # (an instance attribute over the class's 255: 249 frames now count as long)
        got = s2t.batch_align(batch, cuts)
    finally:
        del s2t.align_no_sync_frames
    assert len(got) == 3 and max(len(r["tokens"]) for r in got) < 100
    for a, b in zip(got, want):
        assert a["tokens"] == b["tokens"] and a["total"] == b["total"] and torch.equal(a["frame_labels"], b["frame_labels"])


def test_beam_search_object_aligns_too(s2t_pair, tmp_path):
    """Only frontend, encoder and CTC head are used: an object built for the beam search gives the same alignment."""
    from espnet_amd.bin.asr_inference import Speech2Text

    g, greedy = s2t_pair
    (tmp_path / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), tmp_path / "model.pth")
    beam = Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"),
                       device="cuda", dtype="bfloat16", beam_size=2, ctc_weight=0.3, lm_weight=0.0)
    speech, _ = golden_speech(g)
    a, b = beam.align(speech[0].numpy(), None), greedy.align(speech[0].numpy(), None)
    assert_same_alignment(a, b, "beam object")


def test_unpeaked_bf16_model_output_bit_equal_to_restatement():
    """Nearly flat posteriors, V = 5 000, ~200 tokens in 249 frames: the path on the device's own lpT, read back, must be
    the restatement's bit for bit - rounding belongs to the encoder, the trellis is exact."""
    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC

    g = load_golden("small_10s")
    model = build(g, "bfloat16")
    speech, lens = golden_speech(g)
    st = model.encode_device(speech.cuda(), lens.tolist())
    _, tokens, tlens = model.greedy_ctc_device(st)
    B, T, d = st.enc_act.shape
    Vm = model.ctc.odim
    p = model.ctc.packed(st.enc_act.device)
    lpT = torch.empty(Vm, B * T, dtype=torch.float32, device="cuda")
    L.check(L.load().em_ctc_log_probs_t(model.ctc.em_dtype, L.ptr(st.enc_act), B, T, d, L.ptr(p.weight), L.ptr(p.bias), Vm,
                                        L.ptr(lpT), L.current_stream_ptr()), "em_ctc_log_probs_t")
    out = CTC.align_log_probs_t(lpT, B * T, st.olens_dev, tokens, T, tlens, B, T, model.blank_id)
    own = model.ctc.forced_align_device(st.enc_act, st.olens_dev, tokens, tlens, model.blank_id)
    torch.cuda.synchronize()
    n_fr, n_tok = st.olens[0], int(tlens[0])
    assert n_tok > 100
    y = tokens[0, :n_tok].cpu().tolist()
    want = forced_align_ref(lpT[:, :n_fr].t().contiguous().cpu(), y, model.blank_id)
    got = dict(zip(("align", "frame_lp", "tok_start", "tok_end", "tok_lp", "total"), [o.cpu() for o in out]))
    got = {k: (v[0] if k == "total" else v[0, : (n_fr if k in ("align", "frame_lp") else n_tok)]) for k, v in got.items()}
    assert_same(got, want, "small_10s bf16")
    assert torch.equal(own[0].cpu(), out[0].cpu()) and torch.equal(own[5].cpu(), out[5].cpu())
