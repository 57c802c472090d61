"""Whole-sentence n-gram scoring (em_ngram_seq_logp, csrc/ngram_seq.hip) against a float64 Katz back-off over the parsed ARPA
entries and bit for bit against the step scorer; its host layers: `NgramLM`, the perplexity tool, `batch_ngram_logp`."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from espnet_amd.bin.asr_inference import Speech2Text  # noqa: E402
from espnet_amd.bin.lm_calc_perplexity import main  # noqa: E402
from espnet_amd.lm.ngram import NgramLM  # noqa: E402
from espnet_amd.nets.scorers.ngram import NgramFullScorer  # noqa: E402
from tests.ngram_ref import RefNgram, synthetic_arpa  # noqa: E402

SENT, SENT_I = -7.25, -9  # what the raw calls fill their outputs with


def parse_arpa(path):  # -> ({words: (log10 p, back-off or None)} holding the f32 table values as floats, order)
    g, k = {}, 0
    for line in open(path, encoding="utf-8"):
        parts = line.split()
        if line.startswith("\\"):
            k = int(line[1:].split("-")[0]) if line.rstrip().endswith("-grams:") else 0
        elif k and parts:
            g[tuple(parts[1:1 + k])] = (float(np.float32(parts[0])), float(np.float32(parts[1 + k])) if len(parts) > 1 + k else None)
    return g, max(len(c) for c in g)


def katz(g, N, hist, w):
    """(log10 p(w | hist) in f64, the order that matched, sum of |terms|); hist = <s> and the words so far"""
    ctx = tuple(hist[-(N - 1):]) if N > 1 else ()
    k = next(k for k in range(len(ctx), -1, -1) if ctx[len(ctx) - k:] + (w,) in g)
    terms = [g[ctx[len(ctx) - k:] + (w,)][0]]
    terms += [g[c][1] for c in (ctx[len(ctx) - j:] for j in range(k + 1, len(ctx) + 1)) if c in g and g[c][1] is not None]
    return math.fsum(terms), k + 1, sum(abs(t) for t in terms)


@pytest.fixture(scope="module", params=[1, 2, 3, 6])
def case(request, tmp_path_factory):
    N = request.param
    path = tmp_path_factory.mktemp("arpa") / f"lm{N}.arpa"
    words = synthetic_arpa(path, 20, N, [150, 200, 200, 150, 100], seed=N)
    tokens = ["<blank>", "<unk>"] + words[:20] + ["absent_a", "absent_b", "<eos>"]  # two tokens the file does not know
    V = len(tokens)
    g, order = parse_arpa(path)
    assert order == N
    tok_of = {**{w: t for t, w in enumerate(tokens)}, "</s>": V - 1}
    word = ["</s>" if t == "<eos>" else t if (t,) in g else "<unk>" for t in tokens]
    rng, keys = np.random.default_rng(N), list(g)

    def sentence(n):  # n-grams of the file of every order strung together, single random tokens in between
        y = []
        while len(y) < n:
            y += [tok_of.get(w, V - 2) for w in keys[rng.integers(len(keys))]] if rng.random() < 0.8 else [int(rng.integers(V))]
        return y[:n]

    rows = [sentence(n) for n in (0, 1, N - 1, N, 63, 64, 65, 257, 300)]
    ref = []  # per row: (f64 value, order, sum |terms|) arrays over its tokens and <eos>
    for y in rows:
        hist = ["<s>"] + [word[t] for t in y]
        ref.append(tuple(np.array(c) for c in zip(*(katz(g, N, hist[:j + 1], word[t]) for j, t in enumerate(y + [V - 1])))))
    ids = torch.nn.utils.rnn.pad_sequence([torch.tensor(y, dtype=torch.long) for y in rows], batch_first=True)  # (9, 300)
    return types.SimpleNamespace(N=N, V=V, path=path, tokens=tokens, scorer=NgramFullScorer(str(path), tokens), rows=rows,
                                 ref=ref, ids=ids, ylens=[len(y) for y in rows])


def raw(scorer, ids, ylens, eos_id):
    """The C entry with sentinel-filled outputs -> (rc, logp, logp_tok, order_tok) on the host."""
    ids, ylens = (torch.as_tensor(np.asarray(v), dtype=torch.int32).contiguous() for v in (ids, ylens))
    n, Lp = ids.shape
    ids_d, len_d = ids.cuda(), ylens.cuda()
    logp = torch.full((n,), SENT, dtype=torch.float64, device="cuda")
    lt = torch.full((n, Lp + 1), SENT, dtype=torch.float32, device="cuda")
    ot = torch.full((n, Lp + 1), SENT_I, dtype=torch.int32, device="cuda")
    rc = L.load().em_ngram_seq_logp(C.byref(scorer.packed(ids_d.device).w), L.ptr(ids_d), L.ptr(len_d), L.ptr(ids), L.ptr(ylens),
                                    n, Lp, eos_id, L.ptr(lt), L.ptr(ot), L.ptr(logp), L.current_stream_ptr())
    return rc, logp.cpu().numpy(), lt.cpu().numpy(), ot.cpu().numpy()


@pytest.mark.parametrize("eos", [True, False])
def test_against_float64_katz(case, eos):
    logp, lt, ot = (t.cpu().numpy() for t in case.scorer.sequence_logp(case.ids, case.ylens, eos=eos))
    seen = set()
    for r, y in enumerate(case.rows):
        n = len(y) + eos
        want, order, mag = (a[:n] for a in case.ref[r])
        got = lt[r, :n].astype(np.float64)
        np.testing.assert_array_equal(ot[r, :n], order)
        bound = case.N * 2.0 ** -23 * mag  # a value is at most `order` f32 table entries added in f32
        assert (np.abs(got - want) <= bound).all(), (r, np.abs(got - want).max())
        assert not lt[r, n:].any() and not ot[r, n:].any()
        sum_bound = 2.0 ** -52 * n * np.abs(got).sum()
        assert abs(logp[r] - math.fsum(got)) <= sum_bound and abs(logp[r] - math.fsum(want)) <= sum_bound + bound.sum()
        seen |= set(order.tolist())
    assert seen == set(range(1, case.N + 1))  # every back-off depth occurred


def test_bits_equal_the_step_scorer(case):
    _, lt, _ = case.scorer.sequence_logp(case.ids, case.ylens, eos=True)
    n, V, ids, ylens = len(case.rows), case.V, case.ids.cuda(), torch.tensor(case.ylens).cuda()
    target = torch.cat([ids, ids.new_zeros(n, 1)], 1)
    target[torch.arange(n, device="cuda"), ylens] = V - 1  # the token scored at every position, <eos> behind the last
    ys = torch.cat([ids.new_full((n, 1), V - 1), ids], 1)
    states, xs = [None] * n, torch.zeros(n, 1, device="cuda")
    for j in range(ids.size(1) + 1):
        sc, states = case.scorer.batch_score(ys[:, :j + 1], states, xs)
        step, live = sc.gather(1, target[:, j:j + 1])[:, 0], ylens >= j
        assert torch.equal(step[live].view(torch.int32), lt[live, j].view(torch.int32)), j


@pytest.mark.parametrize("r", [6, 8])  # 65 and 300 tokens: alone one tile / two, in the batch three; both row-sum routes
def test_row_independence_and_padding(case, r):
    y, V, n = case.rows[r], case.V, len(case.rows[r]) + 1
    _, logp1, lt1, ot1 = raw(case.scorer, [y], [len(y)], V - 1)
    for fill in (3, V - 1):
        ids, ylens = np.full((33, 700), fill), [len(case.rows[i % 9]) for i in range(33)]
        for i in range(33):
            ids[i, :ylens[i]] = case.rows[i % 9]
        ids[17, :len(y)], ylens[17] = y, len(y)
        rc, logp, lt, ot = raw(case.scorer, ids, ylens, V - 1)
        np.testing.assert_array_equal(logp[17:18].view(np.int64), logp1.view(np.int64))
        np.testing.assert_array_equal(lt[17, :n].view(np.int32), lt1[0, :n].view(np.int32))
        np.testing.assert_array_equal(ot[17, :n], ot1[0, :n])
        assert rc == 0 and (lt[17, n:] == SENT).all() and (ot[17, n:] == SENT_I).all()


@pytest.mark.parametrize("bad", ["id_V", "id_negative", "ylen"])
def test_refusals_launch_nothing(case, bad):
    ids, ylens = np.ones((2, 5), dtype=np.int64), [5, 6 if bad == "ylen" else 3]
    ids[1, 2] = dict(id_V=case.V, id_negative=-1, ylen=1)[bad]
    rc, logp, lt, ot = raw(case.scorer, ids, ylens, case.V - 1)
    assert rc == L.EM_ERR_BAD_ARG and (logp == SENT).all() and (lt == SENT).all() and (ot == SENT_I).all()


def test_ngramlm_nll_and_the_perplexity_tool(case, tmp_path):
    pick = [1, 3, 4]  # three sentences: 1, `order` and 63 tokens
    text, lens = case.ids[pick, :63], torch.tensor([case.ylens[r] for r in pick])
    nll, xl = NgramLM(str(case.path), case.tokens).nll(text.cuda(), lens.cuda())
    assert nll.shape == (3, 64) and xl.tolist() == (lens + 1).tolist()
    nll, ln10, total, slack = nll.cpu().numpy(), math.log(10.0), 0.0, 0.0
    for i, r in enumerate(pick):
        want, _, mag = case.ref[r]
        assert (np.abs(nll[i, :len(want)] + want * ln10) <= case.N * 2.0 ** -23 * mag * ln10 + 1e-12).all()  # positive nats
        assert not nll[i, len(want):].any()  # exactly 0.0 behind
        total, slack = total - want.sum() * ln10, slack + case.N * 2.0 ** -23 * mag.sum() * ln10
    (tmp_path / "tokens.txt").write_text("\n".join(case.tokens) + "\n")
    (tmp_path / "text").write_text("".join(f"u{r} {' '.join(map(str, case.rows[r]))}\n" for r in pick))
    ppl = main(["--output_dir", str(tmp_path / "out"), "--batch_size", "2", "--ngram_file", str(case.path), "--token_list",
                str(tmp_path / "tokens.txt"), "--data_path_and_name_and_type", f"{tmp_path / 'text'},text,text_int"])
    assert abs(math.log(ppl) - total / (int(lens.sum()) + 3)) <= slack / (int(lens.sum()) + 3) + 1e-12
    assert float((tmp_path / "out" / "ppl").read_text()) == ppl
    assert (tmp_path / "out" / "utt2ntokens").read_text().split() == ["u1", "2", "u3", str(case.N + 1), "u4", "64"]


def test_batch_ngram_logp_is_the_search_column(case):
    s2t = Speech2Text.__new__(Speech2Text)
    s2t.asr_model, s2t.tokenizer, s2t.ngram = types.SimpleNamespace(blank_id=0, sos=case.V - 1, eos=case.V - 1), None, case.scorer
    s2t.device = torch.device("cuda")
    ref = RefNgram(case.path, case.tokens)  # the step scorer's contract: f32 scores accumulated in f32, as the search does
    texts = [[[t for t in case.rows[r] if 0 < t < case.V - 1] for r in (5, 2)], [2, 3], []]
    res = s2t.batch_ngram_logp(texts)
    assert [len(u) for u in res] == [2, 1, 1]
    for cands, got in zip([texts[0], [texts[1]], [texts[2]]], res):
        for y, d in zip(cands, got):
            assert d["token_int"] == y and len(d["tokens"]) == len(y) + 1
            assert np.float32(d["ngram"]) == ref.path_score([case.V - 1] + y + [case.V - 1])
