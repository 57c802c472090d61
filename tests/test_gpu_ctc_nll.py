"""CTC likelihood of given transcripts on the device (csrc/ctc_nll.hip) through the C ABI and the host layer, against the
float64 restatement of the contract (tests/ctc_nll_ref.py) on the SAME f32 log-probabilities, and
Speech2Text.batch_rescore against its three scorers and against the joint search's own hypotheses.

Error rule of the kernel rows, relative to max(|nll_ref|, 1).  A hard ceiling that is derived: every cell is one
max-shifted sum and one add, a few ulp of |alpha|, and the worst case accumulates linearly over the frames, so
|err| <= 4 * T_b * 2^-24 * max(|nll_ref|, 1).  That is loose (rounding errors do not all point one way), so the tests also
hold E_CTC_NLL = 4 x the largest relative error the first GPU run printed (profiles/ctc_nll_pytest_gpu.txt; the
project's convention for E_* constants).  Every test prints what it measured.

Shapes are the smallest that reach every path of the kernel: S around the 8-state lane runs and the 64-lane wave (L = 31
.. 64), around the one-wave form (L = 255 / 256), several waves, frame counts that end inside a group of four prefetched
frames, unaligned utterance starts and the 4-byte load path in ragged batches."""
import functools
import json
import math

import pytest
import torch

from tests.ctc_nll_ref import ctc_nll_ref, ctc_nll_ref_batch
from tests.helpers import golden_speech, golden_state_dict, load_golden
from tests.test_gpu_ctc_align import synth_lp, synth_y

pytestmark = pytest.mark.gpu

V = 50
E_CTC_NLL = 4 * 2.811e-7  # the largest relative error of profiles/ctc_nll_pytest_gpu.txt (T 3 000, L 700), x 4


def device_nll(utt_lps, ys, mem_of=None, T=None, blank=0):
    """Utterance rows (T_u, V) + candidate transcripts (+ the utterance of each) -> (N,) f32 on the host, through
    CTC.nll_log_probs_t."""
    from espnet_amd.asr.ctc import CTC

    Bm, N = len(utt_lps), len(ys)
    T = T or max(max(lp.shape[0] for lp in utt_lps), 1)
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
    out = CTC.nll_log_probs_t(lpT.cuda(), Bm * T, olens, Bm, T, tg.cuda(), Lmax, ylens, mo, N, blank)
    torch.cuda.synchronize()
    return out.cpu()


def assert_close(got, lps, ys, tag):
    """Device rows against the restatement: +inf where it is +inf, else within the derived ceiling and E_CTC_NLL."""
    want = ctc_nll_ref_batch(lps, ys)
    assert not torch.isnan(got).any(), (tag, got)
    worst = 0.0
    for n, (g, w) in enumerate(zip(got.tolist(), want.tolist())):
        if math.isinf(w):
            assert g == math.inf, (tag, n, g)
            continue
        rel = abs(g - w) / max(abs(w), 1.0)
        worst = max(worst, rel)
        assert rel <= 4 * lps[n].shape[0] * 2.0 ** -24, (tag, n, g, w, rel)
    print(f"\n[{tag}] largest relative error {worst:.3e} over {len(ys)} rows (E_CTC_NLL {E_CTC_NLL:.1e})")
    assert worst <= E_CTC_NLL, (tag, worst)
    return want


def check_batch(rows, tag, T=None):
    lps = [synth_lp(t, 31 * i + t) for i, (t, _) in enumerate(rows)]
    ys = [y for _, y in rows]
    got = device_nll(lps, ys, T=T)
    assert_close(got, lps, ys, tag)
    return lps, ys, got


# ------------------------------------------------------------------ kernel against restatement
def test_tiny_shapes_one_ragged_batch():
    a = 7
    rows = [(1, []), (1, [3]), (5, []), (2, [4]), (7, synth_y(7, 1, distinct=True)), (5, [a, a, a]), (3, [9]),
            (17, synth_y(5, 2)), (2, [a, a]), (1, [3, 4])]
    _, _, got = check_batch(rows, "tiny")
    assert got[8] == math.inf and got[9] == math.inf and torch.isfinite(got[:8]).all()


def test_lane_run_and_wave_edges():
    check_batch([(130, synth_y(L, L)) for L in (31, 32, 33, 63, 64)], "T130")


def test_one_wave_tier_edge():
    check_batch([(300, synth_y(255, 5))], "L255")  # S = 511: one wave
    check_batch([(300, synth_y(256, 6)), (300, synth_y(255, 5)), (41, synth_y(3, 7))], "L256")  # S = 513: two waves


def test_multi_wave_long_transcript():
    check_batch([(3000, synth_y(700, 8))], "T3000")  # three waves; no workspace at any size


def test_ten_second_shape_and_odd_frame_counts():
    check_batch([(249, synth_y(60, 9)), (251, synth_y(20, 10)), (3, [5]), (17, synth_y(4, 11))], "T251")
    check_batch([(249, synth_y(60, 9))], "T249 alone")  # an odd row stride: the 4-byte load path


# ------------------------------------------------------------------ shared log-probabilities, independence of rows
def test_candidates_share_their_utterance_through_mem_of():
    utt = [synth_lp(57, 70), synth_lp(40, 71)]
    ys = [synth_y(19, 21), [], synth_y(30, 23), synth_y(11, 20), [4, 4, 4]]
    mem_of = [0, 0, 0, 1, 1]
    shared = device_nll(utt, ys, mem_of=mem_of)
    own = device_nll([utt[u] for u in mem_of], ys)  # the same five rows, one utterance per candidate
    assert torch.equal(shared.view(torch.int32), own.view(torch.int32)), (shared, own)
    assert_close(shared, [utt[u] for u in mem_of], ys, "mem_of")
    clamped = device_nll(utt, ys, mem_of=[-3, 0, 0, 1, 9])  # values outside [0, Bm) are clamped
    assert torch.equal(clamped, shared)


def test_every_row_of_a_batch_is_bit_equal_to_the_row_alone():
    rows = [(40, synth_y(11, 20)), (23, []), (57, synth_y(19, 21)), (9, synth_y(4, 22)), (64, synth_y(30, 23)),
            (300, synth_y(256, 6))]  # (the last row makes the batch a two-wave launch; alone, the others run as one wave)
    lps, ys, got = check_batch(rows, "ragged", T=302)
    for b in range(len(rows)):
        alone = device_nll([lps[b]], [ys[b]])
        assert torch.equal(alone.view(torch.int32), got[b : b + 1].view(torch.int32)), (b, float(alone), float(got[b]))
    again = device_nll(lps, ys, T=302)
    assert torch.equal(again, got)


# ------------------------------------------------------------------ -inf emissions
def test_minus_inf_emissions():
    lps = [synth_lp(12, 50), synth_lp(12, 51), synth_lp(12, 52), synth_lp(9, 53)]
    lps[0][:, 4] = float("-inf")        # the token's column at every frame: no path
    lps[1][[0, 3, 4, 9], 4] = float("-inf")  # at some frames only: the path goes round them
    lps[2][[2, 5], 0] = float("-inf")   # blank frames
    lps[3][:, :] = float("-inf")        # nothing anywhere
    ys = [[4, 6], [4, 6], [4, 4], []]
    got = device_nll(lps, ys)
    want = assert_close(got, lps, ys, "-inf")
    assert got[0] == math.inf and got[3] == math.inf and torch.isfinite(got[1:3]).all() and torch.isfinite(want[1:3]).all()


# ------------------------------------------------------------------ limits
def test_limits_and_argument_errors():
    from espnet_amd import lib as L

    lib = L.load()
    most = int(lib.em_ctc_forced_align_max_tokens())
    lp8 = synth_lp(8, 1)
    lpT = lp8.t().contiguous().cuda()
    one = torch.ones(1, dtype=torch.int32).cuda()
    out = torch.zeros(1, device="cuda")

    def call(Lmax, tg, ldT=8, N=1, mem_of=None):
        rc = lib.em_ctc_seq_nll(L.ptr(lpT), ldT, L.ptr(one * 8), 1, 8, L.ptr(tg), Lmax, L.ptr(one), L.ptr(mem_of), N, 0,
                                L.ptr(out), L.current_stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert call(most, torch.full((1, most), 3, dtype=torch.int32).cuda()) == 0  # the limit itself is taken (16 waves)
    want = ctc_nll_ref(lp8, [3])
    assert abs(float(out[0]) - want) <= E_CTC_NLL * max(want, 1.0)
    rc = call(most + 1, torch.ones(1, most + 1, dtype=torch.int32).cuda())
    assert rc == L.EM_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        L.check(rc, "em_ctc_seq_nll")
    # null pointers, a negative Lmax, a row stride below Bm * T, more candidates than utterances without mem_of
    assert lib.em_ctc_seq_nll(None, 8, None, 1, 8, None, 0, None, None, 1, 0, None, None) == L.EM_ERR_BAD_ARG
    assert call(-1, one) == L.EM_ERR_BAD_ARG
    assert call(1, one, ldT=7) == L.EM_ERR_BAD_ARG
    assert call(1, one, N=2) == L.EM_ERR_BAD_ARG


# ------------------------------------------------------------------ through the model: CTC.nll
def device_log_probs(m, enc_act, olens):
    """The rows (T_b, V) of em_ctc_log_probs_t for the utterances of enc_act: what the trellis itself reads."""
    from espnet_amd import lib as L

    B, T, d = enc_act.shape
    p = m.ctc.packed(enc_act.device)
    lpT = torch.empty(m.ctc.odim, B * T, dtype=torch.float32, device="cuda")
    L.check(L.load().em_ctc_log_probs_t(m.ctc.em_dtype, L.ptr(enc_act), B, T, d, L.ptr(p.weight), L.ptr(p.bias),
                                        m.ctc.odim, L.ptr(lpT), L.current_stream_ptr()), "em_ctc_log_probs_t")
    lpT = lpT.cpu()
    return [lpT[:, b * T : b * T + olens[b]].t().contiguous() for b in range(B)]


def _build_beam_s2t(d, g, **kw):
    from espnet_amd.bin.asr_inference import Speech2Text

    (d / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), d / "model.pth")
    return Speech2Text(asr_train_config=str(d / "config.yaml"), asr_model_file=str(d / "model.pth"), device="cuda",
                       dtype="float32", **kw)


@pytest.fixture(scope="module")
def rescore_case(tmp_path_factory):
    g = load_golden("small_ragged")  # 12 x 256 Conformer, 6 x 256 decoder, V 5 000; utterances of 3.0, 2.3 and 1.0 s
    # (the fixture stores no search weights: ctc_weight 0.3 as the other search goldens have it, a penalty so that
    # length_bonus is a scorer)
    s2t = _build_beam_s2t(tmp_path_factory.mktemp("rescore_model"), g, beam_size=2, ctc_weight=0.3, penalty=0.5)
    speech, lens = golden_speech(g)
    lengths = lens.tolist()[1:]
    return g, s2t, speech[1:, : max(lengths)].contiguous(), lengths


CANDS = [[5, 9, 11, 3], [5, 9], []]
OTHER = [7, 7, 30, 12, 4, 21]


def test_ctc_nll_of_the_model_and_its_argument_errors(rescore_case):
    """CTC.nll (one utterance per transcript, host arguments) against the restatement on the device's own log-probs."""
    g, s2t, speech, lengths = rescore_case
    m = s2t.asr_model
    st = m.encode_device(speech.cuda(), lengths, isolate=True)
    ys = torch.zeros(2, 6, dtype=torch.long)
    ys[0, :4], ys[1] = torch.tensor(CANDS[0]), torch.tensor(OTHER)
    got = m.ctc.nll(st.enc_out, torch.tensor(st.olens), ys, torch.tensor([4, 6]))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2,)
    assert st.enc_act.dtype == torch.float32  # (float32 mode: enc_act is what CTC.nll makes of enc_out)
    lp = device_log_probs(m, st.enc_act, st.olens)
    assert_close(got.cpu(), lp, [CANDS[0], OTHER], "CTC.nll")
    with pytest.raises(ValueError, match="blank"):
        m.ctc.nll(st.enc_out, st.olens, [[5, m.blank_id], OTHER], [2, 6], blank_idx=m.blank_id)
    with pytest.raises(ValueError, match="token ids"):
        m.ctc.nll(st.enc_out, st.olens, [[5, int(g["vocab"])], OTHER], [2, 6], blank_idx=m.blank_id)
    # more tokens than frames: no error, +inf
    long = m.ctc.nll(st.enc_out, st.olens, [list(range(1, 101)), OTHER], [100, 6], blank_idx=m.blank_id).cpu()
    assert long[0] == math.inf and long[1] == got.cpu()[1]


# ------------------------------------------------------------------ Speech2Text.batch_rescore
def test_batch_rescore_components_and_total(rescore_case):
    """Strings and ids give the same call; `ctc` and `decoder` are the NEGATED VALUES of CTC.nll_device (same mem_of) and
    of batch_nll on the same candidates, BIT-EQUAL: the same launches on the same encoder output behind both, and
    negation is exact.  CTC.nll takes one utterance per transcript, so its log-probs launch holds four utterances, not
    two: another launch shape, held to the two calls' bounds (whether it was bit-equal is printed).  `score` is the
    weighted sum, recomputed here."""
    g, s2t, speech, lengths = rescore_case
    m = s2t.asr_model
    as_text = " ".join(s2t.converter.ids2tokens(OTHER))
    assert s2t.tokenizer is not None and s2t._target_ids(as_text) == OTHER
    res = s2t.batch_rescore(speech, lengths, [CANDS, as_text])
    assert [len(r) for r in res] == [3, 1]
    assert s2t.batch_rescore(speech, lengths, [CANDS, OTHER]) == res
    flat = res[0] + res[1]
    rows, mem_of = CANDS + [OTHER], [0, 0, 0, 1]
    w = s2t.beam_search.weights
    assert w["ctc"] == 0.3 and w["length_bonus"] == 0.5
    for r, y in zip(flat, rows):
        assert r["token_int"] == y and list(r["scores"]) == ["decoder", "ctc", "length_bonus"]
        assert r["scores"]["length_bonus"] == len(y) + 1
        assert r["score"] == sum(float(w[k]) * v for k, v in r["scores"].items())
        assert abs(r["score"] - (0.7 * r["scores"]["decoder"] + 0.3 * r["scores"]["ctc"] + 0.5 * (len(y) + 1))) <= 1e-9 * abs(r["score"])
    st = m.encode_device(speech.cuda(), lengths, isolate=True)
    ylens = [len(y) for y in rows]
    shared = m.ctc.nll_device(st.enc_act, st.olens, rows, ylens, m.blank_id, mem_of=mem_of).cpu().tolist()
    ys = torch.zeros(4, 6, dtype=torch.long)
    for i, y in enumerate(rows):
        ys[i, : len(y)] = torch.tensor(y)
    own = m.ctc.nll(st.enc_out[mem_of], [st.olens[u] for u in mem_of], ys, ylens, blank_idx=m.blank_id).cpu().tolist()
    dec = s2t.batch_nll(speech, lengths, [CANDS, OTHER])
    dec = dec[0] + dec[1]
    print("\nbatch_rescore f32:", [(r["scores"]["ctc"], r["scores"]["decoder"], r["score"]) for r in flat])
    for r, a, b, d in zip(flat, shared, own, dec):
        assert r["scores"]["ctc"] == -a and r["scores"]["decoder"] == -d, (r, a, d)
        assert abs(r["scores"]["ctc"] + b) <= 2 * E_CTC_NLL * max(abs(b), 1.0), (r, b)
    print("CTC.nll (one utterance per transcript) bit-equal to the shared rows:", own == shared)
    # the restatement on the device's own log-probs
    lp = device_log_probs(m, st.enc_act, st.olens)
    assert_close(torch.tensor(shared), [lp[u] for u in mem_of], rows, "batch_rescore ctc")


def test_batch_rescore_nbest_list_equals_single_calls_and_slices(rescore_case):
    from tests import dec_seq_cases as K

    g, s2t, speech, lengths = rescore_case
    res = s2t.batch_rescore(speech, lengths, [CANDS, OTHER])

    def same(a, b, tag):
        n = len(a["token_int"]) + 1
        # ctc: a row does not depend on its companions (the contract), on the same log-probs: two f32 roundings of one value
        assert abs(a["scores"]["ctc"] - b["scores"]["ctc"]) <= 2 * E_CTC_NLL * max(abs(a["scores"]["ctc"]), 1.0), tag
        # decoder: other batch shapes of its launches, the two calls' bounds (tests/dec_seq_cases.py)
        assert abs(a["scores"]["decoder"] - b["scores"]["decoder"]) <= 2 * K.E_NLL["float32"] * n, tag
        assert abs(a["score"] - b["score"]) <= 0.3 * 2 * E_CTC_NLL * max(abs(a["scores"]["ctc"]), 1.0) + 0.7 * 2 * K.E_NLL["float32"] * n, tag

    for i, y in enumerate(CANDS):
        alone = s2t.batch_rescore(speech, lengths, [[y], OTHER])
        same(alone[0][0], res[0][i], ("alone", i))
        assert alone[0][0]["scores"]["ctc"] == res[0][i]["scores"]["ctc"]  # (the same log-probs launch: bit-equal)
    s2t.nll_rows_per_call = 2
    try:
        sliced = s2t.batch_rescore(speech, lengths, [CANDS, OTHER])
    finally:
        del s2t.nll_rows_per_call
    for i, (a, b) in enumerate(zip(sliced[0] + sliced[1], res[0] + res[1])):
        same(a, b, ("sliced", i))


def test_batch_rescore_only_enqueues_up_to_its_one_copy(rescore_case):
    """The shared driver of the batch_* calls (encode, every scorer of every slice, the concatenation) under torch's
    sync debug mode "error": nothing synchronises before the one D2H copy.  In slices of 2, so that a slice boundary lies
    inside utterance 0's list and a slice spans both utterances."""
    g, s2t, speech, lengths = rescore_case
    s2t.nll_rows_per_call = 2
    try:
        want = s2t.batch_rescore(speech, lengths, [CANDS, OTHER])  # (and the weights are packed, the lengths cached)
        keys = s2t._rescore_keys()
        cb = s2t._candidates(speech, [CANDS, OTHER], lm="lm" in keys)
        probe = torch.ones(1, device="cuda")
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                probe.item()
                honoured = False
            except RuntimeError:
                honoured = True
            if honoured:
                vals = s2t._enqueue_candidates(speech, lengths, cb, functools.partial(s2t._rescore_columns, keys))
        finally:
            torch.cuda.set_sync_debug_mode(before)
    finally:
        del s2t.nll_rows_per_call
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): .item() did not raise")
    assert vals.is_cuda and vals.cpu().tolist() == [list(r["scores"].values()) for r in want[0] + want[1]]


def test_batch_rescore_agrees_with_the_search_on_its_own_nbest(tmp_path):
    """e2e_beam5_lm (TransformerLM): the device search's n-best, rescored, carries the search's own component scores and
    total, within the tolerance the search is granted against the oracle (tests/test_gpu_search.py
    test_speech2text_with_lm_files_f32: tol_abs 2e-2, tol_rel 5e-5, combined as check_against_golden combines them); and
    the oracle's stored scores of the same sequences likewise.  Hypotheses whose <eos> the search forced at maxlen carry
    no score for it and are left out."""
    import yaml

    from espnet_amd.bin.asr_inference import Speech2Text
    from oracle.weights import recipe_state_dict, token_list

    TOL_ABS, TOL_REL = 2e-2, 5e-5
    g = load_golden("e2e_beam5_lm")
    maxlen = int(g["enc_out"].shape[0])  # maxlenratio 0: the encoder length
    lens = [int(n) for n in g["yseq_lens"]]
    assert any(n - 2 < maxlen for n in lens) and any(n - 2 >= maxlen for n in lens)  # (both kinds are in the fixture)
    Vg = int(g["vocab"])
    (tmp_path / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(golden_state_dict(g), tmp_path / "model.pth")
    (tmp_path / "lm.yaml").write_text(yaml.safe_dump(dict(lm="transformer", lm_conf=json.loads(str(g["lm_conf"])),
                                                         token_list=token_list(Vg))))
    shapes = {"lm." + k: tuple(v) for k, v in json.loads(str(g["lm_state_shapes"])).items()}
    torch.save(recipe_state_dict(shapes, int(g["wseed"]), skip=()), tmp_path / "lm.pth")
    s2t = Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"),
                      lm_train_config=str(tmp_path / "lm.yaml"), lm_file=str(tmp_path / "lm.pth"),
                      device="cuda", dtype="float32", beam_size=int(g["beam"]), ctc_weight=float(g["ctc_weight"]),
                      lm_weight=float(g["lm_weight"]), nbest=int(g["nbest"]), penalty=0.0)
    speech, slen = golden_speech(g)
    hyps = [r[3] for r in s2t(speech[0].numpy())]
    assert int(s2t.asr_model.encode_device(speech[:1].cuda(), [int(slen[0])], isolate=True).olens[0]) == maxlen
    kept = [h for h in hyps if len(h.yseq) - 2 < maxlen]
    assert len(kept) >= 1, [len(h.yseq) for h in hyps]
    res = s2t.batch_rescore(speech[:1], [int(slen[0])], [[h.yseq[1:-1].tolist() for h in kept]])[0]
    keys = json.loads(str(g["score_keys"]))
    golden = {tuple(g["yseq"][k, : g["yseq_lens"][k]].tolist()): k for k in range(len(lens))}
    n_golden = 0
    for h, r in zip(kept, res):
        assert sorted(r["scores"]) == sorted(h.scores) == sorted(keys)
        tol = TOL_ABS + TOL_REL * abs(float(h.score))
        print(f"\n[rescore vs search] len {len(h.yseq)}: score {r['score']:.4f} vs {float(h.score):.4f}; " +
              "; ".join(f"{k} {r['scores'][k]:.4f} vs {float(h.scores[k]):.4f}" for k in keys))
        assert abs(r["score"] - float(h.score)) < tol, (r["score"], float(h.score))
        for k in keys:
            assert abs(r["scores"][k] - float(h.scores[k])) < tol + TOL_REL * abs(float(h.scores[k])), (k, r, h.scores)
        k = golden.get(tuple(h.yseq.tolist()))
        if k is not None:  # the oracle's scores of the same sequence
            n_golden += 1
            tol = TOL_ABS + TOL_REL * abs(float(g["score"][k]))
            assert abs(r["score"] - float(g["score"][k])) < tol, (k, r["score"], float(g["score"][k]))
            for j, kk in enumerate(keys):
                assert abs(r["scores"][kk] - float(g["scores"][k, j])) < tol + TOL_REL * abs(float(g["scores"][k, j]))
    print(f"\n[rescore vs search] {len(kept)} of {len(hyps)} hypotheses ended on a scored <eos>, {n_golden} are the oracle's")


# ------------------------------------------------------------------ refusals
def test_refusals(rescore_case, tmp_path):
    from tests.ngram_ref import synthetic_arpa
    from tests.test_gpu_transducer import _speech2text

    g, beam, speech, lengths = rescore_case
    (tmp_path / "g").mkdir()
    greedy = _build_beam_s2t(tmp_path / "g", g, ctc_greedy=True)
    with pytest.raises(RuntimeError, match="ctc_greedy"):
        greedy.batch_rescore(speech, lengths, [CANDS, OTHER])
    (tmp_path / "t").mkdir()
    transducer, _ = _speech2text(tmp_path / "t", "float32", beam_size=2)
    with pytest.raises(RuntimeError, match="transducer"):
        transducer.batch_rescore(torch.zeros(1, 8000), [8000], [[1, 2]])
    tokens = beam.asr_model.token_list
    words = list(tokens[2:40]) + ["<unk>"]
    synthetic_arpa(tmp_path / "lm2.arpa", 0, 2, [40 * (len(words) + 2)], 17, words=words, with_unk=False)
    (tmp_path / "n").mkdir()
    with_ngram = _build_beam_s2t(tmp_path / "n", g, beam_size=2, ctc_weight=0.3, ngram_file=str(tmp_path / "lm2.arpa"))
    with pytest.raises(NotImplementedError, match="ngram_file"):
        with_ngram.batch_rescore(speech, lengths, [CANDS, OTHER])
