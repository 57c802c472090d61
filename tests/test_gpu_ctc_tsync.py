"""The time-synchronous CTC search on the MI355X (csrc/ctc_tsync.hip: em_ctc_frame_topk, em_ctc_tsync_search; the host
layer espnet_amd/nets/beam_search_timesync.py, Speech2Text(time_sync=True)) against the float64 restatement of its contract
(tests/ctc_tsync_ref.py).  Log-probs are handed to the kernels directly; the cases are chosen by the restatement alone
(margin >= 2 x the derived error ceiling, tests/test_cpu_ctc_tsync.py holds them to the seed window), so the device must
return the same n-best token lists in the same order.

Score bound.  Derived: a dp value of frame t is a max-shifted sum of at most five terms plus an add and the error grows
linearly over the frames: |delta score_ctc| <= 8 T 2^-24 max(|score|, 1) (`Result.ceiling`).  Beside it E_TSYNC, 4 x the
largest relative error the first GPU run printed (profiles/ctc_tsync_pytest_gpu.txt).  score_ngram is held to
RefNgram.path_score at the 1e-4 of tests/test_gpu_ngram.py.  Every test prints what it measured."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctc_tsync_ref as R  # noqa: E402
from tests.ctc_nll_ref import ctc_nll_ref  # noqa: E402
from tests.scratch_fill import assert_scratch_independent  # noqa: E402

E_TSYNC = 4 * 2.092e-7  # relative to max(|score|, 1): 4 x the first run's largest (k_equals_v/plain/seed0)
E_NGRAM = 1e-4


def _search(V, W, K, ngram=None, w_ng=0.0, pen=0.0):
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync

    scorers = dict(ctc=object())
    if ngram is not None:
        scorers["ngram"] = ngram
    return BeamSearchTimeSync(sos=V - 1, beam_size=W, scorers=scorers, pre_beam_ratio=K / W + 1e-9,
                              weights=dict(ctc=1.0, ngram=w_ng, length_bonus=pen))


def _run(bs, lps, xlens=None, nbest=None):
    """lps: list of (T_b, V) f32 arrays -> the host rows of one batched call: per utterance a list of (tokens, score, ctc,
    ngram, len) and the raw output tensors"""
    T = max(max(len(lp) for lp in lps), 1)
    V = lps[0].shape[1]
    batch = np.full((len(lps), T, V), np.log(1.0 / V), dtype=np.float32)
    for b, lp in enumerate(lps):
        batch[b, : len(lp)] = lp
    xlens = [len(lp) for lp in lps] if xlens is None else xlens
    outs = bs.search_log_probs(torch.from_numpy(batch).cuda(), xlens, nbest)
    tokens, lens, count, score, s_ctc, s_ng, s_len = (o.cpu() for o in outs)
    rows = []
    for b in range(len(lps)):
        rows.append([(tokens[b, r, : int(lens[b, r])].tolist(), float(score[b, r]), float(s_ctc[b, r]), float(s_ng[b, r]),
                      float(s_len[b, r])) for r in range(int(count[b]))])
    return rows, [o.cpu() for o in outs]


def _hold(rows, r, nbest, tag, ngram=None, sos=None):
    """the device n-best against the restatement's: same token lists in the same order, scores within the bounds"""
    want = r.nbest[:nbest]
    assert [h[0] for h in rows] == [h[0] for h in want], tag
    worst = 0.0
    for got, ref in zip(rows, want):
        scale = max(abs(ref[1]), abs(ref[2]), 1.0)
        for k in (1, 2):
            worst = max(worst, abs(got[k] - ref[k]) / scale)
            assert abs(got[k] - ref[k]) <= r.ceiling, (tag, k, got, ref, r.ceiling)
        assert got[4] == ref[4] == len(got[0])
        if ngram is not None:
            assert abs(got[3] - float(ngram.path_score([sos] + got[0] + [sos]))) < E_NGRAM, (tag, got)
            assert abs(got[3] - ref[3]) < E_NGRAM
        else:
            assert got[3] == 0.0
    print(f"{tag}: {len(rows)} hypotheses, worst relative score error {worst:.3e} (ceiling {r.ceiling:.3e}, margin {r.margin:.3e})")
    assert worst <= E_TSYNC, (tag, worst)
    return worst


@pytest.fixture(scope="module")
def ngrams(tmp_path_factory):
    """V -> (device scorer, RefNgram) of the seeded 3-gram of tests/ctc_tsync_ref.py::ngram_setup, built once"""
    from espnet_amd.nets.scorers.ngram import NgramFullScorer

    d = tmp_path_factory.mktemp("tsync_arpa")
    cache = {}

    def get(V):
        if V not in cache:
            path, tokens, ref = R.ngram_setup(d, V)
            cache[V] = (NgramFullScorer(str(path), tokens), ref)
        return cache[V]

    return get


# ------------------------------------------------------------------------------------------- 1. the per-frame top K
@pytest.mark.parametrize("V", [12, 65, 5000])
def test_frame_topk_equals_a_stable_sort(V):
    from espnet_amd.asr.ctc import CTC

    rng = np.random.default_rng(V)
    M = 4 * 5 + 3  # (not a multiple of the four rows of a workgroup)
    x = rng.normal(size=(M, V)).astype(np.float32)
    x[1, :] = np.round(x[1, :] * 2) / 2          # a row of exact ties
    x[2, V // 2:] = x[2, : V - V // 2]           # pairs of equal values far apart
    x[3, :] = -1.5                               # every value equal: ids 0 .. K-1
    lp = torch.from_numpy(x).cuda()
    for K in sorted({1, min(6, V), min(30, V), V}):
        blank = 0 if K != 6 else V - 2
        ids, val, bl = (t.cpu().numpy() for t in CTC.topk_log_probs(lp, K, blank))
        for m in range(M):
            want = R.topk_ref(x[m], K)
            np.testing.assert_array_equal(ids[m], want, err_msg=f"V {V} K {K} row {m}")
            np.testing.assert_array_equal(val[m], x[m][want])
        np.testing.assert_array_equal(bl, x[:, blank])
    print(f"V {V}: top-K rows equal the stable sort for K in {sorted({1, min(6, V), min(30, V), V})}")


# ------------------------------------------------------------------------------------------- 2. the walk
@pytest.mark.parametrize("with_ngram", [False, True], ids=["plain", "ngram"])
@pytest.mark.parametrize("name", sorted(R.WALK_CASES))
def test_walk_equals_the_restatement(name, with_ngram, ngrams):
    from espnet_amd.nets.beam_search_timesync import limits

    T, V, W, K, n = R.WALK_CASES[name]
    if name == "limits":
        assert (W, K) == limits()
    dev_ng, ref_ng = ngrams(V) if with_ngram else (None, None)
    got = R.walk_cases(name, ref_ng)
    bs = _search(V, W, K, dev_ng, **(R.NG_WEIGHTS if with_ngram else {}))
    assert bs.candidates_per_frame(V) == K
    rows, _ = _run(bs, [lp for _, lp, _ in got], nbest=W)
    tot = {}
    for (seed, lp, r), row in zip(got, rows):
        _hold(row, r, W, f"{name}/{'ngram' if with_ngram else 'plain'}/seed{seed}", ref_ng, V - 1)
        assert len(set(map(tuple, (h[0] for h in row)))) == len(row)
        for k, v in r.counters.items():
            tot[k] = tot.get(k, 0) + v
    if name == "branches":  # come-backs, merges into a beam entry, frames without blank among the candidates, repeats
        assert all(tot[k] > 0 for k in ("comebacks", "merges", "blank_out", "repeats")), tot
    if name == "beam_not_full":
        assert all(len(row) < W for row in rows)
    print(f"{name}: counters {tot}")


def test_prefix_that_returns_while_its_child_stays():
    """The adversarial identity case: a prefix leaves the beam and comes back while its child is still in it (the
    restatement reports the event).  No duplicate sequence, and the restatement's n-best."""
    T, V, W, K = 20, 4, 6, 3
    seed, lp, r = R.find_return_with_child(T, V, W, K)
    rows, _ = _run(_search(V, W, K), [lp], nbest=W)
    seqs = [tuple(h[0]) for h in rows[0]]
    assert len(set(seqs)) == len(seqs), seqs
    _hold(rows[0], r, W, f"return-with-child/seed{seed} ({r.counters['returns_with_child']} events)")


def test_ragged_batch_rows_equal_the_utterances_alone(ngrams):
    """Five utterances with xlens 24, 1, 0, 13, 7 in one launch: every row is bit for bit what the utterance gives alone,
    and the restatement's n-best; no frames: the empty hypothesis with score 0."""
    T, V, W, K, _ = R.WALK_CASES["branches"]
    dev_ng, ref_ng = ngrams(V)
    for ng in (None, dev_ng):
        bs = _search(V, W, K, ng, *((R.NG_WEIGHTS["w_ng"], R.NG_WEIGHTS["pen"]) if ng is not None else ()))
        lps = [R.gen_logprobs(T, V, 100 + i)[:n] for i, n in enumerate([24, 1, 0, 13, 7])]
        rows, outs = _run(bs, lps, nbest=W)
        assert rows[2] == [([], 0.0, 0.0, 0.0, 0.0)]
        for b, lp in enumerate(lps):
            if len(lp) == 0:
                continue
            alone_rows, alone = _run(bs, [lp], nbest=W)
            assert alone_rows[0] == rows[b]
            n = alone[0].shape[2]
            assert torch.equal(outs[0][b, :, :n], alone[0][0]) and (outs[0][b, :, n:] == -1).all()
            for o, a in zip(outs[1:], alone[1:]):
                assert np.array_equal(o[b].numpy().view(np.int32), a[0].numpy().view(np.int32)), b
            kw = dict(ngram=ref_ng, **R.NG_WEIGHTS) if ng is not None else {}
            r = R.tsync_ref(lp, W, K, V - 1, **kw)
            if r.margin >= 2 * r.ceiling:
                _hold(rows[b], r, W, f"ragged/{b}", ref_ng if ng is not None else None, V - 1)
            else:  # (these utterances are not chosen by margin: the best hypothesis only, tolerant of near-ties)
                assert any(h[0] == rows[b][0][0] and abs(h[1] - rows[b][0][1]) <= r.ceiling for h in r.nbest)


# ------------------------------------------------------------------------------------------- 3. invariants without a reference
def test_beam_one_equals_greedy_ctc_over_4000_frames():
    """W = K = 1 through the whole host path (CTC.log_softmax, top-K, walk) equals CTC.greedy_device's tokens."""
    from espnet_amd.asr.ctc import CTC
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync

    T, V, d = 4000, 50, 64
    lp = R.gen_logprobs(T, V, 5)
    lp[:, V - 1] -= 30.0  # (greedy CTC drops <sos/eos>; the search keeps it as a token: never the arg-max here)
    ctc = CTC(V, d, compute_dtype="float32")
    with torch.no_grad():
        ctc.ctc_lo.weight.copy_(torch.eye(V, d))
        ctc.ctc_lo.bias.zero_()
    ctc = ctc.cuda()
    act = torch.zeros(1, T, d)
    act[0, :, :V] = torch.from_numpy(lp)
    act = act.cuda()
    olens = torch.tensor([T], dtype=torch.int32, device="cuda")
    _, tokens, tlens = ctc.greedy_device(act, olens, 0, V - 1)
    want = tokens[0, : int(tlens[0])].cpu().tolist()
    bs = BeamSearchTimeSync(sos=V - 1, beam_size=1, scorers=dict(ctc=ctc), weights=dict(ctc=1.0))
    assert bs.candidates_per_frame(V) == 1
    hyp = bs.search_batch(act, [T])[0]
    assert len(hyp) == 1 and hyp[0].yseq.tolist() == [V - 1] + want + [V - 1]
    assert hyp is not None and bs.forward(act[0])[0].yseq.tolist() == hyp[0].yseq.tolist()
    print(f"beam 1 over {T} frames: {len(want)} tokens, equal to greedy CTC")


def test_unpruned_scores_are_the_ctc_likelihood():
    """T 3, V 3: 15 prefixes at most, beam 32 - nothing is pruned, so every hypothesis' ctc score is -ctc_nll_ref of its
    own tokens."""
    T, V, W = 3, 3, 32
    worst = 0.0
    for seed in range(4):
        lp = R.gen_logprobs(T, V, seed, peak=1.0)
        rows, _ = _run(_search(V, W, V), [lp], nbest=W)
        assert 1 < len(rows[0]) <= 15
        for toks, score, ctc, _, _ in rows[0]:
            want = -ctc_nll_ref(torch.from_numpy(lp), toks)
            worst = max(worst, abs(ctc - want) / max(abs(want), 1.0))
            assert score == ctc
        assert rows[0][0][1] == max(h[1] for h in rows[0])
    print(f"unpruned: worst relative error of the CTC likelihood {worst:.3e}")
    assert worst <= E_TSYNC


# ------------------------------------------------------------------------------------------- 4. scratch independence
def test_frame_topk_writes_its_outputs_whole():
    from espnet_amd import lib as L

    M, V, K = 11, 65, 30
    lp = torch.from_numpy(np.random.default_rng(1).normal(size=(M, V)).astype(np.float32)).cuda()
    outs = [torch.empty(M, K, dtype=torch.int32, device="cuda"), torch.empty(M, K, dtype=torch.float32, device="cuda"),
            torch.empty(M, dtype=torch.float32, device="cuda")]

    def call():
        L.check(L.load().em_ctc_frame_topk(L.ptr(lp), M, V, K, 0, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]),
                                           L.current_stream_ptr()), "em_ctc_frame_topk")

    assert_scratch_independent(call, [], outs, names=["cand_id", "cand_lp", "blank_lp"], synchronize=torch.cuda.synchronize)


def test_walk_does_not_depend_on_its_workspace(ngrams):
    from espnet_amd import lib as L
    from espnet_amd.asr.ctc import CTC

    lib = L.load()
    T, V, W, K = 24, 12, 4, 6
    dev_ng, _ = ngrams(V)
    model = C.byref(dev_ng.packed(torch.device("cuda", torch.cuda.current_device())).w)
    big = dict(B=4, T=40, K=8, W=7)
    ws = torch.empty(int(lib.em_ctc_tsync_search_workspace_bytes(big["B"], big["T"], big["K"], big["W"])), dtype=torch.uint8,
                     device="cuda")

    def setup(B, T, K, W, seed0):
        lp = torch.from_numpy(np.stack([R.gen_logprobs(T, V, seed0 + b) for b in range(B)])).cuda()
        tabs = CTC.topk_log_probs(lp, K, 0)
        xl = torch.tensor([T - 3 * b for b in range(B)], dtype=torch.int32, device="cuda")
        outs = [torch.empty(B, W, T, dtype=torch.int32, device="cuda"), torch.empty(B, W, dtype=torch.int32, device="cuda"),
                torch.empty(B, dtype=torch.int32, device="cuda")] + [torch.empty(B, W, dtype=torch.float32, device="cuda")
                                                                     for _ in range(4)]

        def call(ws_bytes=None):
            L.check(lib.em_ctc_tsync_search(L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), L.ptr(xl), B, T, K, W, W, V - 1, 0,
                                            1.0, 0.5, 0.3, model, *(L.ptr(o) for o in outs), L.ptr(ws),
                                            int(ws.numel()) if ws_bytes is None else ws_bytes, L.current_stream_ptr()),
                    "em_ctc_tsync_search")

        return call, outs

    call, outs = setup(3, T, K, W, 0)
    stale, _ = setup(big["B"], big["T"], big["K"], big["W"], 50)
    assert int(lib.em_ctc_tsync_search_workspace_bytes(3, T, K, W)) < ws.numel()
    assert_scratch_independent(call, ws, outs, stale=stale,
                               names=["tokens", "lens", "count", "score", "score_ctc", "score_ngram", "score_len"])
    with pytest.raises(L.EspnetAmdError, match="workspace"):  # a workspace that is too small is refused
        call(ws_bytes=int(lib.em_ctc_tsync_search_workspace_bytes(3, T, K, W)) - 8)


def test_limits_are_refused_by_name():
    from espnet_amd.nets.beam_search_timesync import limits

    W_max, K_max = limits()
    lp = torch.zeros(1, 3, 200, device="cuda").log_softmax(-1)
    with pytest.raises(NotImplementedError, match=f"beam_size <= {W_max}"):
        _search(200, W_max + 1, 8).search_log_probs(lp, [3])
    with pytest.raises(NotImplementedError, match=f"<= {K_max}"):
        _search(200, 8, K_max + 1).search_log_probs(lp, [3])


# ------------------------------------------------------------------------------------------- 5. end to end
def _s2t(tmp_path, dtype, **kw):
    from espnet_amd.bin.asr_inference import Speech2Text

    return Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"),
                       device="cuda", dtype=dtype, time_sync=True, ctc_weight=1.0, beam_size=4, nbest=2, **kw)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_speech2text_time_sync_end_to_end(tmp_path, dtype):
    """Speech2Text(time_sync=True) on the golden CLI model: the restatement runs on the device's own CTC.log_softmax
    output.  The model's log-probs cannot be chosen for margin, so near-ties are tolerated: the device's best hypothesis is
    in the restatement's n-best with a score within the bound, and no hypothesis of the restatement beats it by more."""
    import yaml

    from espnet_amd.fileio.sound_scp import read_wav
    from tests.helpers import load_golden
    from tests.test_gpu_cli import _run as cli_run, _setup, _table

    g = load_golden("cli_decode")
    _setup(tmp_path)
    tokens = yaml.safe_load(str(g["config_yaml"]))["token_list"]
    path, _, ref_ng = R.ngram_setup(tmp_path, len(tokens), tokens=tokens)
    waves = {}
    for ln in (tmp_path / "wav.scp").read_text().splitlines():
        key, wav = ln.split()
        waves[key] = read_wav(wav, dtype="float32")[0]
    keys = [k for k in waves if k != "uttC"]  # (uttC is too short for the subsampling)
    lens = [len(waves[k]) for k in keys]
    speech = torch.zeros(len(keys), max(lens))
    for b, k in enumerate(keys):
        speech[b, : lens[b]] = torch.as_tensor(waves[k])
    tol_enc = 1e-5 if dtype == "float32" else 1e-2  # (batch against alone: the encoder's rounding, not the search's)
    for with_ng in (False, True):
        kw = dict(ngram_file=str(path), ngram_weight=0.4, penalty=0.2) if with_ng else {}
        s2t = _s2t(tmp_path, dtype, **kw)
        assert s2t.beam_search is None and s2t.beam_search_timesync is not None
        if with_ng:
            assert s2t.ngram is not None and s2t.ngram._pack is not None  # packed with the other modules
        with pytest.raises(RuntimeError, match="time_sync=True"):
            s2t.batch_rescore(speech, lens, [[1]] * len(keys))
        batch = s2t.batch_decode(speech, lens)
        m = s2t.asr_model
        st = m.encode_device(speech.cuda(), lens, isolate=True)
        lp = m.ctc.log_softmax(st.enc_act).cpu().numpy()
        V = lp.shape[2]
        for b, k in enumerate(keys):
            alone = s2t(waves[k])
            assert [(r[0], r[1], r[2]) for r in alone] == [(r[0], r[1], r[2]) for r in batch[b]], k
            # (the walk is bit-identical in and out of a batch - test_ragged_batch_rows_equal_the_utterances_alone - but the
            # f32 encoder's last bits depend on the batch it ran in: 1 ulp of a score of -34 was seen)
            for ra, rb in zip(alone, batch[b]):
                assert abs(float(ra[3].score) - float(rb[3].score)) <= tol_enc * max(abs(float(rb[3].score)), 1.0), k
            assert s2t.batch_decode_async(speech[b : b + 1, : lens[b]], [lens[b]]).result()[0][0][2] == alone[0][2]
            r = R.tsync_ref(lp[b], 4, s2t.beam_search_timesync.candidates_per_frame(V), m.sos, blank=m.blank_id, T_valid=int(st.olens[b]),
                            **(dict(ngram=ref_ng, w_ng=0.4, pen=0.2) if with_ng else {}))
            hyp = batch[b][0][3]
            y, sc = hyp.yseq.tolist(), float(hyp.score)
            assert y[0] == y[-1] == m.sos and batch[b][0][2] == [t for t in y[1:-1] if t != 0]
            bound = r.ceiling
            match = [h for h in r.nbest if h[0] == y[1:-1]]
            assert match and abs(match[0][1] - sc) <= bound, (k, y, sc, r.nbest[:2])
            assert r.nbest[0][1] - sc <= bound
            assert set(hyp.scores) == ({"ctc", "ngram", "length_bonus"} if with_ng else {"ctc", "length_bonus"})
            if with_ng:
                assert abs(float(hyp.scores["ngram"]) - float(ref_ng.path_score(y))) < E_NGRAM
            print(f"{dtype} ngram={with_ng} {k}: score {sc:.5f}, restatement {match[0][1]:.5f}, bound {bound:.2e}, "
                  f"margin {r.margin:.2e}")
        # the CLI's result files agree with batch_decode
        extra = ["--ngram_file", str(path), "--ngram_weight", "0.4", "--penalty", "0.2"] if with_ng else []
        _, files = cli_run(tmp_path, f"out_{dtype}_{with_ng}", "--dtype", dtype, "--batch_size", "2", "--time_sync", "true",
                           "--ctc_weight", "1.0", "--beam_size", "4", "--nbest", "2", *extra)
        ti, tx = _table(files["1best_recog/token_int"]), _table(files["1best_recog/text"])
        sc = _table(files["1best_recog/score"])
        for b, k in enumerate(keys):
            assert ti[k].split() == [str(t) for t in batch[b][0][2]], k
            assert tx[k] == (batch[b][0][0] or ""), k
            assert abs(float(sc[k]) - float(batch[b][0][3].score)) <= 1e-3 * max(abs(float(sc[k])), 1.0), k
