"""The n-gram scorer on the MI355X (csrc/ngram.hip, the search integration in csrc/search.hip) against the restatement of
its contract (tests/ngram_ref.py) and, inside the search, against the oracle's beam search with the n-gram standing in for
its LM scorer (the oracle has no n-gram scorer of its own: its `TransformerLMOracle` name is monkeypatched with a stand-in
whose `step` returns the restatement's log10 scores for the full prefixes)."""
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import golden_speech, golden_state_dict, load_golden  # noqa: E402
from tests.ngram_ref import RefNgram, synthetic_arpa, write_arpa  # noqa: E402
from tests.test_gpu_search import _sub, build_lm, oracle_enc  # noqa: E402


def _tokens(V):
    from oracle.weights import token_list

    return token_list(V)


def _arpa_for(tmp_path, tokens, order, seed, frac=0.85, scale=1):
    """a synthetic ARPA over most of the token strings (the others, <blank> and <sos/eos> score as <unk>)"""
    rng = np.random.default_rng(seed)
    words = [t for t in tokens[2:-1] if rng.random() < frac] + ["<unk>"]
    nw = len(words) + 2
    counts = [40 * nw * scale, 25 * nw * scale, 15 * nw * scale, 10 * nw * scale, 8 * nw * scale][: order - 1]
    p = tmp_path / f"lm{order}_{seed}.arpa"
    synthetic_arpa(p, 0, order, counts, seed, words=words, with_unk=False)
    return p


def _full(path, tokens):
    from espnet_amd.nets.scorers.ngram import NgramFullScorer

    return NgramFullScorer(str(path), tokens)


# ------------------------------------------------------------------------------------------- 1. the scorer call
@pytest.mark.parametrize("V", [300, 5000])
@pytest.mark.parametrize("order", [2, 3, 4, 5, 6])
def test_em_ngram_score_equals_the_restatement(tmp_path, V, order):
    from espnet_amd.nets.scorers.ngram import NgramPartScorer

    tokens = _tokens(V)
    path = _arpa_for(tmp_path, tokens, order, seed=order * 7 + V)
    ref = RefNgram(path, tokens)
    full, part = _full(path, tokens), NgramPartScorer(str(path), tokens)
    rng = np.random.default_rng(order)
    n, steps = (12, 7) if V == 300 else (6, 6)
    # histories: mostly hub tokens (contexts with many successors), unknown tokens, dead ends, <blank> / <sos/eos>
    hub = list(range(2, 40))  # (the synthetic file gives the lowest word ids the most successors)
    Y = np.empty((n, steps + 1), dtype=np.int64)
    Y[:, 0] = V - 1
    for r in range(n):
        for j in range(1, steps + 1):
            u = rng.random()
            Y[r, j] = rng.choice(hub) if u < 0.6 else (0 if u < 0.65 else (V - 1 if u < 0.7 else rng.integers(1, V - 1)))
    xs = torch.zeros(n, 1, device="cuda")
    states, pstates = None, None
    for j in range(1, steps + 1):
        ys = torch.from_numpy(Y[:, :j])
        sc, states = full.batch_score(ys, states if j > 1 else [None] * n, xs)
        cand = torch.from_numpy(rng.integers(0, V, size=(n, 9)).astype(np.int64))
        ps, pstates = part._score(ys, pstates if j > 1 else [None] * n, xs.device, cand=cand)
        sc, ps = sc.cpu().numpy(), ps.cpu().numpy()
        for r in range(n):
            h = ref.history(Y[r, :j])
            want = ref.row(h)
            np.testing.assert_array_equal(sc[r], want, err_msg=f"row {r} step {j} history {h}")
            for c in rng.integers(0, V, size=5):  # the per-token restatement too
                assert sc[r, c] == ref.score(h, int(c))
            np.testing.assert_array_equal(ps[r], sc[r, cand[r].numpy()])  # part = full at those columns
    # the single-hypothesis calls of the reference's interface
    y = torch.from_numpy(Y[0, :3])
    s0, st0 = full.score(y[:1], None, xs[0])
    s1, st1 = full.score(y[:2], st0, xs[0])
    s2, _ = full.score(y[:3], st1, xs[0])
    np.testing.assert_array_equal(s2.cpu().numpy(), ref.row(ref.history(Y[0, :3])))
    p2, _ = part.score_partial(y[:3], torch.tensor([3, 1, V - 1]), st1, xs[0])
    np.testing.assert_array_equal(p2.cpu().numpy(), s2.cpu().numpy()[[3, 1, V - 1]])
    assert full.select_state(st1, 0) is st1


# ------------------------------------------------------------------------------------------- search helpers
def _search(g, sd, dtype="float32", ngram=None, ngram_weight=0.0, lm=None, beam=None):
    from espnet_amd.asr.ctc import CTC
    from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet_amd.nets.batch_beam_search import build_beam_search

    V = int(g["vocab"])
    d = g["config"]["encoder_conf"]["output_size"]
    dec = TransformerDecoder(V, d, compute_dtype=dtype, **g["config"]["decoder_conf"])
    dec.load_state_dict(_sub(sd, "decoder."), strict=True)
    ctc = CTC(V, d, compute_dtype=dtype)
    ctc.load_state_dict(_sub(sd, "ctc."), strict=True)
    cw = float(g["ctc_weight"])
    model = types.SimpleNamespace(decoder=dec.cuda() if cw < 1.0 else None, ctc=ctc.cuda() if cw > 0.0 else None,
                                  sos=V - 1, eos=V - 1)
    return build_beam_search(model, beam_size=beam or int(g["beam"]), ctc_weight=cw,
                             penalty=float(g["penalty"]) if "penalty" in g else 0.0,
                             lm_weight=float(g["lm_weight"]) if lm is not None else 0.0, token_list=_tokens(V), lm=lm,
                             ngram=ngram, ngram_weight=ngram_weight)


class _NgramAsOracleLM:
    """Stand-in for oracle.beam_search.TransformerLMOracle: the restatement's log10 scores of the full prefixes."""

    ref = None

    def __init__(self, *a, **k):
        pass

    def init_cache(self):
        return [(torch.zeros(1, 0), torch.zeros(1, 0))]

    def step(self, yseq, cache):
        rows = np.stack([self.ref.row(self.ref.history(y)) for y in yseq.tolist()])
        n = yseq.shape[0]
        return torch.from_numpy(rows), [(torch.zeros(n, 0), torch.zeros(n, 0))]


def _oracle_nbest(monkeypatch, g, sd, enc, ref, w):
    import oracle.beam_search as ob

    _NgramAsOracleLM.ref = ref
    monkeypatch.setattr(ob, "TransformerLMOracle", _NgramAsOracleLM)
    dc = g["config"]["decoder_conf"]
    V = int(g["vocab"])
    kw = {k: float(g[k]) for k in ("maxlenratio", "minlenratio", "penalty") if k in g}
    return ob.beam_search(sd, enc, dc["attention_heads"], dc["num_blocks"], int(g["beam"]), float(g["ctc_weight"]),
                          sos=V - 1, eos=V - 1, lm_weight=w, lm_conf={"head": 0, "layer": 0}, **kw)


def _maxlen(g, T):
    """beam_search.py:414-429 with the fixture's maxlenratio"""
    r = float(g["maxlenratio"]) if "maxlenratio" in g else 0.0
    return T if r == 0 else (-int(r) if r < 0 else max(1, int(r * T)))


def _scored(y, maxlen):
    """the tokens a hypothesis was scored on: an <eos> forced at maxlen is appended unscored (beam_search.py:393-410)"""
    return y[:-1] if len(y) == maxlen + 2 else y


def _path_and_additivity(bs, hyps, ref, maxlen, tol_ng=1e-4):
    for h in hyps:
        y = _scored(h.yseq.tolist(), maxlen)
        assert abs(float(h.scores["ngram"]) - float(ref.path_score(y))) <= tol_ng, h.yseq.tolist()
        tot = sum(bs.weights[k] * float(v) for k, v in h.scores.items())
        assert abs(tot - float(h.score)) < 1e-2 + 1e-4 * abs(tot), (tot, float(h.score))


# ------------------------------------------------------------------------------------------- 2. f32 search vs oracle
@pytest.mark.parametrize("name", ["tiny_beam5", "tiny_beam4_early_eos", "large_beam10_3s"])
@pytest.mark.parametrize("graph", [False, True])
def test_search_with_ngram_f32_matches_oracle_nbest(monkeypatch, tmp_path, name, graph):
    g = load_golden(name)
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    V = int(g["vocab"])
    tokens = _tokens(V)
    path = _arpa_for(tmp_path, tokens, 3 if V < 1000 else 4, seed=11)
    ref = RefNgram(path, tokens)
    w = 0.6
    want = _oracle_nbest(monkeypatch, g, sd, enc[0, :T], ref, w)
    bs = _search(g, sd, "float32", ngram=_full(path, tokens), ngram_weight=w)
    bs.use_hipgraph = graph
    kw = {k: float(g[k]) for k in ("maxlenratio", "minlenratio") if k in g}
    for _ in range(2 if graph else 1):  # the second call replays the captured graph
        hyps = bs.search_batch(enc[:, :T].contiguous().cuda(), [T], **kw)[0]
        mine = {tuple(h.yseq.tolist()): h for h in hyps}
        for k, r in enumerate(want):
            assert tuple(r["yseq"]) in mine, f"oracle hypothesis #{k} missing from the device n-best"
            h = mine[tuple(r["yseq"])]
            tol = 2e-3 + 2e-5 * abs(r["score"])
            assert abs(float(h.score) - r["score"]) < tol, (k, float(h.score), r["score"])
            for kk, v in r["scores"].items():
                mk = "ngram" if kk == "lm" else kk
                assert abs(float(h.scores[mk]) - v) < tol + 2e-5 * abs(v), (k, kk, float(h.scores[mk]), v)
        assert hyps[0].yseq.tolist() == want[0]["yseq"] or (len(want) > 1 and want[0]["score"] - want[1]["score"] < 1e-2)
        _path_and_additivity(bs, hyps, ref, _maxlen(g, T))


# ------------------------------------------------------------------------------------------- 3. bf16 + batching
def test_search_with_ngram_bf16_path_scores_and_batching(tmp_path):
    g = load_golden("tiny_beam4_early_eos")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    tokens = _tokens(int(g["vocab"]))
    path = _arpa_for(tmp_path, tokens, 4, seed=5)
    ref = RefNgram(path, tokens)
    ng = _full(path, tokens)
    bs = _search(g, sd, "bfloat16", ngram=ng, ngram_weight=0.8)
    hyps = bs.search_batch(enc[:, :T].contiguous().cuda(), [T])[0]
    assert len(hyps) > 0
    _path_and_additivity(bs, hyps, ref, _maxlen(g, T))
    e2 = torch.zeros(2, T, enc.shape[-1])
    e2[0], e2[1, : T - 9] = enc[0, :T], enc[0, 9:T]
    both = bs.search_batch(e2.cuda(), [T, T - 9])
    for b, (x, n) in enumerate([(enc[:, :T], T), (enc[:, 9:T], T - 9)]):
        single = bs.search_batch(x.contiguous().cuda(), [n])[0]
        assert [h.yseq.tolist() for h in single] == [h.yseq.tolist() for h in both[b]]
        for hs, hb in zip(single, both[b]):
            assert abs(float(hs.score) - float(hb.score)) < 1e-3
            assert abs(float(hs.scores["ngram"]) - float(hb.scores["ngram"])) < 1e-4
        _path_and_additivity(bs, both[b], ref, _maxlen(g, n))


# ------------------------------------------------------------------------------------------- 4. neural LM + n-gram
@pytest.mark.parametrize("graph", [False, True])
def test_search_with_lm_and_ngram(tmp_path, graph):
    g = load_golden("tiny_beam5_lm")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    tokens = _tokens(int(g["vocab"]))
    path = _arpa_for(tmp_path, tokens, 3, seed=9)
    ref = RefNgram(path, tokens)
    bs = _search(g, sd, "float32", ngram=_full(path, tokens), ngram_weight=0.5, lm=build_lm(g, "float32"))
    bs.use_hipgraph = graph
    assert list(bs.full_scorers) == ["decoder", "length_bonus", "lm", "ngram"] or list(bs.full_scorers) == [
        "decoder", "lm", "ngram"]
    for _ in range(2 if graph else 1):
        hyps = bs.search_batch(enc[:, :T].contiguous().cuda(), [T])[0]
        assert len(hyps) > 0 and all({"decoder", "ctc", "lm", "ngram"} <= set(h.scores) for h in hyps)
        _path_and_additivity(bs, hyps, ref, _maxlen(g, T))


# ------------------------------------------------------------------------------------------- 5. part mode
def test_search_with_ngram_part_scorer(tmp_path):
    """NgramPartScorer: the n-gram term is added to the pre-beam candidates only.  The one slot outside the pre-beam is the
    <eos> the reference always scores: a hypothesis that ends on an <eos> its parent's pre-beam did not hold carries no
    n-gram term for it.  The pre-beam of the last step is recomputed teacher-forced by the oracle's decoder."""
    from espnet_amd.nets.scorers.ngram import NgramPartScorer
    from oracle.beam_search import DecoderOracle

    g = load_golden("tiny_beam5")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    V = int(g["vocab"])
    tokens = _tokens(V)
    path = _arpa_for(tmp_path, tokens, 3, seed=21)
    ref = RefNgram(path, tokens)
    bs = _search(g, sd, "float32", ngram=NgramPartScorer(str(path), tokens), ngram_weight=0.7)
    assert "ngram" in bs.part_scorers and bs.do_pre_beam
    hyps = bs.search_batch(enc[:, :T].contiguous().cuda(), [T])[0]
    assert len(hyps) > 0
    dc = g["config"]["decoder_conf"]
    w_dec, w_len, S = bs.weights["decoder"], bs.weights.get("length_bonus", 0.0), bs.pre_beam_size
    outside = 0
    for h in hyps:
        y = _scored(h.yseq.tolist(), _maxlen(g, T))
        dec = DecoderOracle(sd, enc[0, :T], dc["attention_heads"], dc["num_blocks"], len(y))
        cache = dec.init_cache()
        for j in range(len(y) - 1):
            logp, cache = dec.step(torch.tensor([y[j]]), j, cache)
        full = w_dec * logp[0] + (w_len if "length_bonus" in bs.scorers else 0.0)
        pre = set(torch.topk(full, S)[1].tolist())
        want = ref.path_score(y) if y[-1] in pre else ref.path_score(y[:-1])
        outside += y[-1] not in pre
        assert abs(float(h.scores["ngram"]) - float(want)) <= 1e-4, (y, float(h.scores["ngram"]), want)
        tot = sum(bs.weights[k] * float(v) for k, v in h.scores.items())
        assert abs(tot - float(h.score)) < 1e-2 + 1e-4 * abs(tot)
    print(f"{outside} of {len(hyps)} hypotheses end on an <eos> outside their last pre-beam")


# ------------------------------------------------------------------------------------------- 5b. the three-launch tail
@pytest.mark.parametrize("part", [False, True], ids=["full", "part"])
def test_search_with_ngram_unfused_tail_equals_default(monkeypatch, tmp_path, part):
    """The n-gram records (run_sngram -> end_sngram) through update_kernel: ESPNET_AMD_NO_TAIL_FUSION=1 returns the
    hypotheses of the default one-launch tail, bit for bit."""
    from espnet_amd import lib as L
    from espnet_amd.nets.scorers.ngram import NgramPartScorer

    g = load_golden("tiny_beam5")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    tokens = _tokens(int(g["vocab"]))
    path = _arpa_for(tmp_path, tokens, 3, seed=21)
    ng = NgramPartScorer(str(path), tokens) if part else _full(path, tokens)
    bs = _search(g, sd, "float32", ngram=ng, ngram_weight=0.7)
    x = enc[:, :T].contiguous().cuda()
    default = bs.search_batch(x, [T])[0]
    monkeypatch.setenv("ESPNET_AMD_NO_TAIL_FUSION", "1")
    L.load().em_dev_switches_reload()
    try:
        unfused = bs.search_batch(x, [T])[0]
    finally:
        monkeypatch.delenv("ESPNET_AMD_NO_TAIL_FUSION")
        L.load().em_dev_switches_reload()
    assert len(default) > 0 and all("ngram" in h.scores for h in default)
    assert [h.yseq.tolist() for h in unfused] == [h.yseq.tolist() for h in default]
    for a, b in zip(default, unfused):
        assert float(a.score) == float(b.score)
        assert {k: float(v) for k, v in a.scores.items()} == {k: float(v) for k, v in b.scores.items()}


# ------------------------------------------------------------------------------------------- 6. weight 0
def test_zero_ngram_weight_is_the_plain_search(tmp_path):
    g = load_golden("tiny_beam5")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    tokens = _tokens(int(g["vocab"]))
    path = _arpa_for(tmp_path, tokens, 3, seed=2)
    x = enc[:, :T].contiguous().cuda()
    plain = _search(g, sd).search_batch(x, [T])[0]
    zero = _search(g, sd, ngram=_full(path, tokens), ngram_weight=0.0)
    assert "ngram" not in zero.scorers
    got = zero.search_batch(x, [T])[0]
    assert [h.yseq.tolist() for h in got] == [h.yseq.tolist() for h in plain]
    for a, b in zip(plain, got):
        assert float(a.score) == float(b.score)
        assert {k: float(v) for k, v in a.scores.items()} == {k: float(v) for k, v in b.scores.items()}


# ------------------------------------------------------------------------------------------- 7. it steers the search
def test_a_peaked_ngram_changes_the_best_hypothesis(tmp_path):
    g = load_golden("tiny_beam5")
    sd = golden_state_dict(g)
    enc, olens = oracle_enc(g, sd)
    T = int(olens[0])
    V = int(g["vocab"])
    tokens = _tokens(V)
    x = enc[:, :T].contiguous().cuda()
    plain = _search(g, sd).search_batch(x, [T])[0]
    best = plain[0].yseq.tolist()
    target = next(h.yseq.tolist() for h in plain[1:] if h.yseq.tolist() != best)
    tokens = list(tokens)
    tokens[1] = "u1"  # (the n-gram's strings: <sos/eos> reads as <unk>, token 1 must not, or the model would let a search end early)
    # a 6-gram model of that one sequence: every window of its history (<s> + its words) with log10 p = -0.01, every
    # other word -100, and a back-off weight of -100 on every context, so that leaving the sequence costs at least 100 per step
    words = [tokens[t] if tokens[t] != "<sos/eos>" else "<unk>" for t in target[1:]]
    hist = ["<s>"] + words
    grams = {1: [("-99" if w == "<s>" else "-100.0", w, "-100.0")
                 for w in sorted(set(tokens[1:-1]) | {"<unk>", "</s>", "<s>"})]}
    for k in range(2, 7):
        win = sorted({" ".join(hist[j - k + 1 : j + 1]) for j in range(k - 1, len(hist))})
        grams[k] = [("-0.01", w, "-100.0" if k < 6 else None) for w in win]
    write_arpa(tmp_path / "peak.arpa", grams)
    bs = _search(g, sd, ngram=_full(tmp_path / "peak.arpa", tokens), ngram_weight=3.0)
    got = bs.search_batch(x, [T])[0]
    assert got[0].yseq.tolist() == target != best


# ------------------------------------------------------------------------------------------- 8. threaded lanes
def test_threaded_lanes_share_one_ngram_pack(tmp_path):
    from espnet_amd.nets.batch_beam_search import SearchLanes

    g = load_golden("tiny_beam4_early_eos")
    sd = golden_state_dict(g)
    d = g["config"]["encoder_conf"]["output_size"]
    tokens = _tokens(int(g["vocab"]))
    path = _arpa_for(tmp_path, tokens, 4, seed=13)
    torch.manual_seed(3)
    work = []
    for lens in ([49, 31, 40], [12], [64, 64], [7, 55, 23]):
        e = torch.randn(len(lens), max(lens), d) * 0.5
        for b, n in enumerate(lens):
            e[b, n:] = 0.0
        work.append((e.cuda(), lens))
    alone_bs = _search(g, sd, ngram=_full(path, tokens), ngram_weight=0.5)
    alone = [alone_bs.search_batch(e, l) for e, l in work]
    torch.cuda.synchronize()
    ng = _full(path, tokens)
    builds = []
    orig = ng._build_pack

    def counted(pk):
        builds.append(pk.serial)
        orig(pk)

    ng._build_pack = counted
    bs = _search(g, sd, ngram=ng, ngram_weight=0.5)
    lanes = SearchLanes([bs] + [bs.clone() for _ in work[1:]], torch.device("cuda"), threaded=True)
    for k, (e, l) in enumerate(work):
        lanes.start(k, e, l, tag=k)
    for k, want in enumerate(alone):
        tag, nbest = lanes.wait(k)
        assert tag == k
        assert len(nbest) == len(want)
        for hw, hg in zip(want, nbest):
            assert len(hw) == len(hg) > 0
            for a, b in zip(hw, hg):
                assert a.yseq.tolist() == b.yseq.tolist() and float(a.score) == float(b.score)
                assert {k_: float(v) for k_, v in a.scores.items()} == {k_: float(v) for k_, v in b.scores.items()}
    lanes.close()
    assert len(builds) == 1, builds


# ------------------------------------------------------------------------------------------- 9. Speech2Text + CLI
def test_speech2text_and_cli_with_ngram_file(tmp_path):
    from espnet_amd.bin.asr_inference import Speech2Text
    from tests.test_gpu_cli import _run, _setup, _table

    g = load_golden("cli_decode")
    _setup(tmp_path)
    import yaml

    tokens = yaml.safe_load(str(g["config_yaml"]))["token_list"]
    path = _arpa_for(tmp_path, tokens, 3, seed=17)
    ref = RefNgram(path, tokens)
    for scorer in ("full", "part"):
        s2t = Speech2Text(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"),
                          device="cuda", dtype="float32", beam_size=int(g["beam"]), ctc_weight=float(g["ctc_weight"]),
                          nbest=1, lm_weight=0.0, ngram_file=str(path), ngram_weight=0.4, ngram_scorer=scorer)
        assert s2t.ngram is not None and s2t.ngram._pack is not None  # packed with the other modules
        from espnet_amd.fileio.sound_scp import read_wav

        key, wav = max((ln.split() for ln in (tmp_path / "wav.scp").read_text().splitlines()),
                       key=lambda kw: (tmp_path / kw[1]).stat().st_size)  # (the longest utterance)
        res = s2t(read_wav(wav, dtype="float32")[0])
        hyp = res[0][3]
        assert "ngram" in hyp.scores
        tot = sum(s2t.beam_search.weights[k] * float(v) for k, v in hyp.scores.items())
        assert abs(tot - float(hyp.score)) < 1e-2 + 1e-4 * abs(tot)
        if scorer == "full":
            y = hyp.yseq.tolist()  # (an <eos> forced at the encoder length is unscored)
            assert min(abs(float(hyp.scores["ngram"]) - float(ref.path_score(z))) for z in (y, y[:-1])) < 1e-4
            py_first = (key, float(hyp.score))
    _, files = _run(tmp_path, "out_ngram", "--dtype", "float32", "--batch_size", "1", "--ngram_file", str(path),
                    "--ngram_weight", "0.4")
    scores = _table(files["1best_recog/score"])
    k, sc = py_first
    assert abs(float(scores[k].replace("tensor(", "").rstrip(")")) - sc) < 1e-3, (scores[k], sc)
    _, plain = _run(tmp_path, "out_plain", "--dtype", "float32", "--batch_size", "1")
    assert _table(plain["1best_recog/score"]) != scores  # the n-gram took part
