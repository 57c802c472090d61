"""The resumable time-synchronous CTC search on the MI355X (csrc/ctc_tsync.hip: em_ctc_tsync_extend, em_ctc_tsync_state_bytes;
the host layer BeamSearchTimeSync.stream_state / extend_candidates / extend; Speech2TextStreaming(search="tsync")).

The defining property (include/espnet_amd.h): after any sequence of calls that fed a slot the frames 0 .. t-1, the row's
outputs are, bit for bit in every column, what em_ctc_tsync_search returns for the same candidate tables with xlens = t -
however the frames were split into calls and whatever else the launches served.  So the reference of nearly every test here
is the one-shot search itself and no tolerance is involved; independently, the final lists are held to the float64
restatement (tests/ctc_tsync_ref.py) under the criteria of tests/test_gpu_ctc_tsync.py (`_hold`, copied from there:
Result.ceiling, E_TSYNC, E_NGRAM).  The one-shot results are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctc_tsync_ref as R  # noqa: E402
from tests.scratch_fill import BIG, ONES, bytes_equal, fill_bytes  # noqa: E402

E_TSYNC = 4 * 2.092e-7  # (tests/test_gpu_ctc_tsync.py)
E_NGRAM = 1e-4
NAMES = ["tokens", "lens", "count", "score", "score_ctc", "score_ngram", "score_len"]


def _search(V, W, K, ngram=None, w_ng=0.0, pen=0.0):
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync

    scorers = dict(ctc=object())
    if ngram is not None:
        scorers["ngram"] = ngram
    return BeamSearchTimeSync(sos=V - 1, beam_size=W, scorers=scorers, pre_beam_ratio=K / W + 1e-9,
                              weights=dict(ctc=1.0, ngram=w_ng, length_bonus=pen))


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

    d = tmp_path_factory.mktemp("tsync_stream_arpa")
    cache = {}

    def get(V):
        if V not in cache:
            path, tokens, ref = R.ngram_setup(d, V)
            cache[V] = (NgramFullScorer(str(path), tokens), ref, path, tokens)
        return cache[V][:2]

    def files(V):
        """(path of the ARPA file, its token list)"""
        get(V)
        return cache[V][2:]

    get.files = files
    return get


def _tables(lps, K):
    """list of (T, V) f32 log-prob arrays of one length -> the candidate tables (B, T, K) on the device"""
    from espnet_amd.asr.ctc import CTC

    return CTC.topk_log_probs(torch.from_numpy(np.stack(lps)).cuda(), K, 0)


class Feeder:
    """Feeds rows of whole-utterance candidate tables to slots piece by piece.  A call's tables are gathered per row from
    the row's own position; what lies behind a row's n_new frames in the call's tables is poison (NaN log-probs)."""

    def __init__(self, bs, state, tabs, slots, nbest=None):
        self.bs, self.state, self.tabs, self.slots, self.nbest = bs, state, tabs, list(slots), nbest
        self.pos = [0] * len(self.slots)
        self.started = [False] * len(self.slots)

    def call(self, rows, ns, consume=True, bs=None):
        """rows: the utterance rows this call serves, ns: their new frames -> the TsyncTick"""
        cid, clp, blp = self.tabs
        Tc = max(max(ns), 1)
        K = cid.shape[2]
        a = torch.zeros(len(rows), Tc, K, dtype=torch.int32, device="cuda")
        b = torch.full((len(rows), Tc, K), float("nan"), device="cuda")
        c = torch.full((len(rows), Tc), float("nan"), device="cuda")
        for i, (r, n) in enumerate(zip(rows, ns)):
            p = self.pos[r]
            a[i, :n], b[i, :n], c[i, :n] = cid[r, p : p + n], clp[r, p : p + n], blp[r, p : p + n]
        reset = [not self.started[r] for r in rows]
        tick = (bs or self.bs).extend_candidates(a, b, c, ns, [self.slots[r] for r in rows], reset, self.state, self.nbest)
        for r, n in zip(rows, ns):
            self.started[r] = True
            if consume:
                self.pos[r] += n
        return tick


def _assert_rows_equal(ext, i, one, b, tag):
    """row i of an extend call's outputs against row b of a one-shot call's: every column, bit for bit"""
    T = one[0].shape[2]
    n = min(T, ext[0].shape[2])
    assert torch.equal(ext[0][i, :, :n], one[0][b, :, :n]), (tag, "tokens")
    assert (ext[0][i, :, n:] == -1).all() and (one[0][b, :, n:] == -1).all(), (tag, "tokens behind the frames")
    for name, e, o in zip(NAMES[1:], ext[1:7], one[1:]):
        assert bytes_equal(e[i].contiguous(), o[b].contiguous()), (tag, name, e[i], o[b])


def _host_rows(outs, i):
    tokens, lens, count, score, s_ctc, s_ng, s_len = (o.cpu() for o in outs[:7])
    return [(tokens[i, r, : int(lens[i, r])].tolist(), float(score[i, r]), float(s_ctc[i, r]), float(s_ng[i, r]),
             float(s_len[i, r])) for r in range(int(count[i]))]


def _pieces(T, rng, zeros=True):
    """T frames in seeded random pieces, zero-frame calls among them"""
    out, left = [], T
    while left > 0:
        n = 0 if (zeros and rng.random() < 0.25) else int(rng.integers(1, min(left, 6) + 1))
        out.append(n)
        left -= n
    if zeros:
        out.insert(int(rng.integers(0, len(out) + 1)), 0)
    return out


def _poisoned_state(bs, n_slots, max_frames, K, byte=BIG):
    st = bs.stream_state(n_slots, max_frames, "cuda", K=K)
    fill_bytes(st.slab, byte)
    return st


def _case(name, with_ngram, ngrams):
    T, V, W, K, n = R.WALK_CASES[name]
    dev_ng, ref_ng = ngrams(V) if with_ngram else (None, None)
    got = R.walk_cases(name, ref_ng)
    bs = _search(V, W, K, dev_ng, **(R.NG_WEIGHTS if with_ngram else {}))
    tabs = _tables([lp for _, lp, _ in got], K)
    return T, V, W, K, got, bs, tabs, ref_ng


# ------------------------------------------------------------------------------------------- 1. any split equals one shot
@pytest.mark.parametrize("with_ngram", [False, True], ids=["plain", "ngram"])
@pytest.mark.parametrize("name", sorted(R.WALK_CASES))
def test_any_split_equals_one_shot(name, with_ngram, ngrams):
    T, V, W, K, got, bs, tabs, ref_ng = _case(name, with_ngram, ngrams)
    B = len(got)
    one = [o.cpu() for o in bs.search_candidates(*tabs, [T] * B, W)]
    rng = np.random.default_rng(7)
    splits = {"one call": [[T]] * B, "frame by frame": [[1] * T] * B, "random pieces": [_pieces(T, rng) for _ in range(B)]}
    if B > 1:
        assert len({tuple(p) for p in splits["random pieces"]}) > 1  # a different split per row
    for mode, plan in splits.items():
        state = _poisoned_state(bs, B, T + 3, K)  # (max_frames != T: other node ids, another tokens stride)
        fd = Feeder(bs, state, tabs, list(range(B)), W)
        for step in range(max(len(p) for p in plan)):
            tick = fd.call(list(range(B)), [p[step] if step < len(p) else 0 for p in plan])
        ext = [o.cpu() for o in tick.outs]
        assert ext[7].tolist() == [T] * B and ext[8].tolist() == [0] * B, (mode, ext[7], ext[8])
        for b, (seed, lp, r) in enumerate(got):
            tag = f"{name}/{'ngram' if with_ngram else 'plain'}/seed{seed}/{mode}"
            _assert_rows_equal(ext, b, one, b, tag)
            _hold(_host_rows(ext, b), r, W, tag, ref_ng, V - 1)
        hyps = bs.collect(tick)  # the host's lists are those of the one-shot outputs
        want = bs.collect(tuple(o.cuda() for o in one))
        for hb, wb in zip(hyps, want):
            assert [(h.yseq.tolist(), h.score, h.scores) for h in hb] == [(h.yseq.tolist(), h.score, h.scores) for h in wb]


# ------------------------------------------------------------------------------------------- 2. every partial result
@pytest.mark.parametrize("with_ngram", [False, True], ids=["plain", "ngram"])
@pytest.mark.parametrize("name", ["branches", "short"])
def test_every_partial_result_equals_one_shot_on_the_frames_so_far(name, with_ngram, ngrams):
    T, V, W, K, got, bs, tabs, _ = _case(name, with_ngram, ngrams)
    B = len(got)
    rng = np.random.default_rng(3)
    plan = [[0] + _pieces(T, rng) for _ in range(B)]  # the first call feeds nothing: frames = 0
    state = _poisoned_state(bs, B, T, K, ONES)
    fd = Feeder(bs, state, tabs, list(range(B)), W)
    for step in range(max(len(p) for p in plan)):
        tick = fd.call(list(range(B)), [p[step] if step < len(p) else 0 for p in plan])
        ext = [o.cpu() for o in tick.outs]
        one = [o.cpu() for o in bs.search_candidates(*tabs, fd.pos, W)]
        assert ext[7].tolist() == fd.pos and ext[8].tolist() == [0] * B
        for b in range(B):
            _assert_rows_equal(ext, b, one, b, f"{name}/step{step}/row{b}/frames{fd.pos[b]}")
        if step == 0:  # no frames: the empty hypothesis, every score 0
            for b in range(B):
                assert _host_rows(ext, b) == [([], 0.0, 0.0, 0.0, 0.0)]
    assert fd.pos == [T] * B


# ------------------------------------------------------------------------------------------- 3. the rare branch
def test_pruned_prefix_comes_back_across_the_state_round_trip():
    """A prefix leaves the beam and returns while its child stays (tests/ctc_tsync_ref.py::find_return_with_child): the
    utterance is split exactly in front of the frame where it returns and one frame either side, three rows of one launch
    sequence."""
    T, V, W, K = 20, 4, 6, 3
    seed, lp, r = R.find_return_with_child(T, V, W, K)
    events = [R.tsync_ref(lp, W, K, V - 1, T_valid=t).counters["returns_with_child"] for t in range(T + 1)]
    f = next(t for t in range(T) if events[t + 1] > events[t])  # the frame (0-based) of the first return
    cuts = [c for c in (f - 1, f, f + 1) if 0 < c < T]
    assert len(cuts) >= 2, (f, T)
    bs = _search(V, W, K)
    tabs = tuple(t.expand(len(cuts), *t.shape[1:]).contiguous() for t in _tables([lp], K))
    one = [o.cpu() for o in bs.search_candidates(*tabs, [T] * len(cuts), W)]
    state = _poisoned_state(bs, len(cuts), T, K)
    fd = Feeder(bs, state, tabs, list(range(len(cuts))), W)
    fd.call(list(range(len(cuts))), cuts)
    ext = [o.cpu() for o in fd.call(list(range(len(cuts))), [T - c for c in cuts]).outs]
    for i, c in enumerate(cuts):
        _assert_rows_equal(ext, i, one, i, f"return-with-child/seed{seed}/cut{c} (return at frame {f})")
        rows = _host_rows(ext, i)
        assert len({tuple(h[0]) for h in rows}) == len(rows)
        _hold(rows, r, W, f"return-with-child/seed{seed}/cut{c}")


# ------------------------------------------------------------------------------------------- 4. slots and neighbours
def test_slots_neighbours_reuse_and_grow(ngrams):
    """Three utterances A, B, C on a non-identity choice of slots in a poisoned slab with more slots than rows, interleaved
    over calls that serve A alone, B alone, both; A ends, its slot's bytes are overwritten with the poison patterns and C
    starts there with reset while B goes on; the slab is copied to a larger one while B and C are under way."""
    T, V, W, K, _ = R.WALK_CASES["branches"]
    dev_ng, _ = ngrams(V)
    bs = _search(V, W, K, dev_ng, **R.NG_WEIGHTS)
    lps = [R.gen_logprobs(T, V, 300 + i) for i in range(3)]
    tabs = _tables(lps, K)
    one = [o.cpu() for o in bs.search_candidates(*tabs, [T] * 3, W)]
    state = _poisoned_state(bs, 7, T, K)
    A, B_, C_ = 0, 1, 2
    fd = Feeder(bs, state, tabs, [5, 2, 5], W)  # (C takes A's slot later)
    fd.call([A], [4])
    fd.call([B_], [7])
    fd.call([B_, A], [3, 9])  # (row order != slot order)
    fd.call([A], [0])
    ext = [o.cpu() for o in fd.call([A, B_], [11, 2]).outs]
    assert fd.pos[A] == T
    _assert_rows_equal(ext, 0, one, A, "A in slot 5")
    for byte in (ONES, BIG):  # A's slot is released: whatever it holds, C starts there
        fill_bytes(state.slab[5], byte)
        fdc = Feeder(bs, state, tabs, [5, 2, 5], W)
        fdc.pos, fdc.started = list(fd.pos), [True, True, False]
        tick = fdc.call([C_, B_], [6, 0], consume=False)
        one6 = [o.cpu() for o in bs.search_candidates(*tabs, [T, fd.pos[B_], 6], W)]
        got = [o.cpu() for o in tick.outs]
        _assert_rows_equal(got, 0, one6, C_, f"C restarts slot 5 after fill {byte:#x}")
        _assert_rows_equal(got, 1, one6, B_, "B beside it")
    fd.started[C_] = True
    fd.pos[C_] = 6
    old_ptr = state.slab.data_ptr()
    state.grow()  # B (12 frames in) and C (6 frames in) move with their slab
    assert state.n_slots == 14 and state.slab.data_ptr() != old_ptr
    fill_bytes(state.slab[7:], BIG)
    fd.call([B_, C_], [5, 10])
    ext = [o.cpu() for o in fd.call([C_, B_], [8, 7]).outs]
    assert fd.pos == [T] * 3 and ext[7].tolist() == [T, T]
    _assert_rows_equal(ext, 0, one, C_, "C after reuse and grow")
    _assert_rows_equal(ext, 1, one, B_, "B after grow")


# ------------------------------------------------------------------------------------------- 5. capacity and mismatch
def test_capacity_is_all_or_nothing_and_mismatch_is_status_2():
    T, V, W, K, _ = R.WALK_CASES["branches"]
    bs, wide = _search(V, W, K), _search(V, W + 1, K)
    lp = R.gen_logprobs(T, V, 400)
    tabs = _tables([lp], K)
    state = wide.stream_state(2, 8, "cuda", K=K)  # (slots large enough for either beam)
    fill_bytes(state.slab, BIG)
    fd = Feeder(bs, state, tabs, [1], W)
    fd.call([0], [5])
    tick = fd.call([0], [4], consume=False)  # 5 + 4 > 8: nothing consumed
    ext = [o.cpu() for o in tick.outs]
    assert ext[7].tolist() == [5] and ext[8].tolist() == [1]
    _assert_rows_equal(ext, 0, [o.cpu() for o in bs.search_candidates(*tabs, [5], W)], 0, "status 1: the frames so far")
    with pytest.raises(RuntimeError, match="tsync_max_frames = 8"):
        bs.collect(tick)
    tick = fd.call([0], [0], bs=wide)  # another beam on the slot, without reset
    ext = [o.cpu() for o in tick.outs]
    assert ext[8].tolist() == [2] and ext[2].tolist() == [0]
    with pytest.raises(RuntimeError, match=rf"W \(the slot was first used with {W}, the call has {W + 1}\)"):
        wide.collect(tick)
    tick = fd.call([0], [3])  # a call that fits still works, on a slot the two refusals left alone
    ext = [o.cpu() for o in tick.outs]
    assert ext[7].tolist() == [8] and ext[8].tolist() == [0]
    _assert_rows_equal(ext, 0, [o.cpu() for o in bs.search_candidates(*tabs, [8], W)], 0, "8 frames after two refusals")
    assert len(bs.collect(tick)[0]) >= 1
    # a slot that was never reset is refused (the poisoned header is no header)
    fd2 = Feeder(bs, state, tabs, [0], W)
    fd2.started = [True]
    assert fd2.call([0], [2]).outs[8].tolist() == [2]


def test_refusals_before_any_launch():
    from espnet_amd import lib as L
    from espnet_amd.nets.beam_search_timesync import limits

    lib = L.load()
    W_max, K_max = limits()
    S, Tc, K, W, Tn = 1, 2, 6, 4, 8
    per = int(lib.em_ctc_tsync_state_bytes(Tn, K, W))
    assert per > 0 and per % 8 == 0
    assert lib.em_ctc_tsync_state_bytes(Tn, K_max + 1, W) == 0 and lib.em_ctc_tsync_state_bytes(Tn, K, W_max + 1) == 0
    assert lib.em_ctc_tsync_state_bytes(0, K, W) == 0
    assert lib.em_ctc_tsync_state_bytes(Tn, K_max, W_max) > per
    slab = torch.zeros(2, per, dtype=torch.uint8, device="cuda")
    ci = torch.zeros(S, Tc, K_max + 1, dtype=torch.int32, device="cuda")
    cl = torch.zeros(S, Tc, K_max + 1, device="cuda")
    bl = torch.zeros(S, Tc, device="cuda")
    ctl = torch.tensor([[0], [0], [1]], dtype=torch.int32, device="cuda")
    nb = W_max + 1
    outs = [torch.full((S, nb, Tn), 77, dtype=torch.int32, device="cuda"), torch.full((S, nb), 77, dtype=torch.int32, device="cuda"),
            torch.full((S,), 77, dtype=torch.int32, device="cuda")] + [torch.full((S, nb), 77.0, device="cuda") for _ in range(4)] + \
           [torch.full((S,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]

    def call(K=K, W=W, Tc=Tc, nbest=W, sos=11, slot_bytes=per, n_slots=2):
        return lib.em_ctc_tsync_extend(L.ptr(ci), L.ptr(cl), L.ptr(bl), L.ptr(ctl[0]), L.ptr(ctl[1]), L.ptr(ctl[2]), S, Tc, K, W,
                                       Tn, nbest, sos, 0, 1.0, 0.0, 0.0, None, L.ptr(slab), n_slots, slot_bytes,
                                       *(L.ptr(o) for o in outs), L.current_stream_ptr())

    assert call(slot_bytes=per - 8) == L.EM_ERR_WORKSPACE
    assert call(K=K_max + 1, slot_bytes=1 << 30) == L.EM_ERR_UNSUPPORTED
    assert call(W=W_max + 1, slot_bytes=1 << 30) == L.EM_ERR_UNSUPPORTED
    assert call(Tc=0) == L.EM_ERR_BAD_ARG and call(nbest=0) == L.EM_ERR_BAD_ARG and call(sos=0) == L.EM_ERR_BAD_ARG
    assert call(n_slots=0) == L.EM_ERR_BAD_ARG and call(slot_bytes=per + 4) == L.EM_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all((o == 77).all() for o in outs)  # nothing was launched
    with pytest.raises(NotImplementedError, match=f"beam_size <= {W_max}"):
        _search(200, W_max + 1, 8).stream_state(1, 8, "cuda", K=8)
    with pytest.raises(ValueError, match="distinct"):
        bs = _search(12, W, K)
        bs.extend_candidates(ci[:, :, :K].contiguous().expand(2, Tc, K), cl[:, :, :K].expand(2, Tc, K), bl.expand(2, Tc),
                             [0, 0], [1, 1], [1, 1], bs.stream_state(2, Tn, "cuda", K=K))
    assert call() == L.EM_OK  # (the arguments the refusals varied are otherwise good)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 6. whole writes
def test_outputs_are_written_whole_on_an_emission_only_call(ngrams):
    T, V, W, K, _ = R.WALK_CASES["short"]
    dev_ng, _ = ngrams(V)
    bs = _search(V, W, K, dev_ng, **R.NG_WEIGHTS)
    tabs = _tables([R.gen_logprobs(T, V, 500 + i) for i in range(2)], K)
    state = _poisoned_state(bs, 2, T + 5, K)
    fd = Feeder(bs, state, tabs, [1, 0], W)
    first = [o.cpu().clone() for o in fd.call([0, 1], [3, 0]).outs]  # (row 1: no frames at all)
    from espnet_amd import lib as L

    lib = L.load()
    model = C.byref(dev_ng.packed(torch.device("cuda", torch.cuda.current_device())).w)
    ci, cl, bl = (torch.zeros(2, 1, K, dtype=torch.int32, device="cuda"), torch.full((2, 1, K), float("nan"), device="cuda"),
                  torch.full((2, 1), float("nan"), device="cuda"))
    ctl = torch.tensor([[0, 0], [1, 0], [0, 0]], dtype=torch.int32, device="cuda")
    slab_before = state.slab.cpu().clone()
    runs = []
    for byte in (ONES, 0x00, BIG):
        outs = [torch.empty(2, W, T + 5, dtype=torch.int32, device="cuda"), torch.empty(2, W, dtype=torch.int32, device="cuda"),
                torch.empty(2, dtype=torch.int32, device="cuda")] + [torch.empty(2, W, device="cuda") for _ in range(4)] + \
               [torch.empty(2, dtype=torch.int32, device="cuda") for _ in range(2)]
        for o in outs:
            fill_bytes(o, byte)
        L.check(lib.em_ctc_tsync_extend(L.ptr(ci), L.ptr(cl), L.ptr(bl), L.ptr(ctl[0]), L.ptr(ctl[1]), L.ptr(ctl[2]), 2, 1, K, W,
                                        T + 5, W, V - 1, 0, 1.0, R.NG_WEIGHTS["w_ng"], R.NG_WEIGHTS["pen"], model,
                                        L.ptr(state.slab), 2, state.slot_bytes, *(L.ptr(o) for o in outs),
                                        L.current_stream_ptr()), "em_ctc_tsync_extend")
        runs.append([o.cpu() for o in outs])
    for run in runs:
        for name, o, want in zip(NAMES + ["frames", "status"], run, first):
            assert bytes_equal(o, want), name
    assert runs[0][7].tolist() == [3, 0] and runs[0][8].tolist() == [0, 0]
    assert torch.equal(state.slab.cpu(), slab_before)  # emission never changes the state


# ------------------------------------------------------------------------------------------- 7. the host layers: plumbing
# The stream's hypotheses are compared with the one-shot search on the stream's OWN candidate tables, captured tick by tick
# (`keep_tsync_tables`): bit for bit, whatever the encoder's numerics are.
CH = 10240


def _s2t(tmp_path, dtype="float32", model_ctc_weight=0.3, **kw):
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import recipe_state_dict, token_list
    from tests.helpers import load_stream_golden

    g = load_stream_golden("stream_small_6s")
    cfg = dict(token_list=token_list(50), frontend="default", frontend_conf=dict(n_fft=512, hop_length=160, win_length=400),
               normalize="utterance_mvn", normalize_conf={}, encoder="contextual_block_conformer", encoder_conf=g["conf"],
               decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
               model_conf=dict(ctc_weight=model_ctc_weight))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    args = dict(device="cuda", dtype=dtype, beam_size=4, nbest=3, ctc_weight=1.0, use_hipgraph=False, search="tsync",
                tsync_max_frames=96)
    args.update(kw)
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, **args)
    sd = s2t.asr_model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 31)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    s2t.asr_model.load_state_dict(new, strict=True)
    return s2t


def _one_shot_on_own_tables(s2t, key):
    """the one-shot search on everything the stream `key` was fed so far -> its n-best list"""
    bs = s2t.beam_search_timesync
    ticks = s2t.tsync_tables.get(key, [])
    K = bs.candidates_per_frame(50)
    n = sum(int(t[0].shape[0]) for t in ticks)
    if n == 0:
        tabs = (torch.zeros(1, 1, K, dtype=torch.int32, device="cuda"), torch.zeros(1, 1, K, device="cuda"),
                torch.zeros(1, 1, device="cuda"))
    else:
        tabs = tuple(torch.cat([t[i] for t in ticks], 0).unsqueeze(0).contiguous() for i in range(3))
    return bs.collect(bs.search_candidates(*tabs, [n], s2t.nbest))[0], n


def _same(got, want, tag):
    assert len(got) == len(want) >= 1, tag
    for a, b in zip(got, want):
        assert a.yseq.tolist() == b.yseq.tolist(), tag
        assert a.score == b.score and a.scores == b.scores, (tag, a.score, b.score, a.scores, b.scores)


def _best_ids(hyps):
    return [t for t in hyps[0].yseq[1:-1].tolist() if t != 0]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("with_ngram", [False, True], ids=["plain", "ngram"])
def test_streams_return_the_one_shot_search_on_their_own_tables(tmp_path, dtype, with_ngram, ngrams):
    from oracle.weights import synth_waveform

    kw = {}
    if with_ngram:
        path, _ = ngrams.files(50)
        kw = dict(ngram_file=str(path), ngram_weight=0.4, penalty=0.2)
    s2t = _s2t(tmp_path, dtype, **kw)
    assert s2t.beam_search is None and s2t.beam_search_timesync is not None and (s2t.ngram is not None) == with_ngram
    s2t.keep_tsync_tables = True
    keys = {"ctc", "length_bonus"} | ({"ngram"} if with_ngram else set())
    # --- __call__, chunk by chunk: the list so far after EVERY chunk
    N = 40000
    wav = synth_waveform(70, N)
    seen = 0
    for pos in range(0, N, CH):
        nxt = min(N, pos + CH)
        res = s2t(wav[pos:nxt], is_final=(nxt == N))
        want, n = _one_shot_on_own_tables(s2t, "call")
        _same([r[3] for r in res], want, f"__call__ {dtype} pos {pos} ({n} frames)")
        assert all(set(r[3].scores) == keys and r[3].yseq[0] == r[3].yseq[-1] == s2t.asr_model.sos for r in res)
        assert res[0][2] == _best_ids(want)
        seen = n
    assert seen > 20 and s2t._tsync_started is False  # the final call reset the stream
    first = s2t(wav[:CH], is_final=False)  # the next utterance starts from the empty prefix in the same slot
    s2t.tsync_tables.clear()
    s2t.reset()
    again = s2t(wav[:CH], is_final=False)
    _same([r[3] for r in again], [r[3] for r in first], "a new utterance in the reused slot")
    s2t.reset()
    s2t.tsync_tables.clear()
    # --- batch_call, S = 3: one tick in flight, per stream the one-shot result on its own tables
    S = 3
    wavs = torch.stack([synth_waveform(40 + s, N) for s in range(S)])
    prev_ids = None
    for pos in range(0, N, CH):
        nxt = min(N, pos + CH)
        tick = s2t.batch_call_async(wavs[:, pos:nxt], is_final=(nxt == N), group="g")
        ids = tick.result()
        assert len(ids) == S
        for s in range(S):
            want, n = _one_shot_on_own_tables(s2t, ("g", s))
            if tick.nbest is None:
                assert n == 0 and ids[s] == []
                continue
            _same(tick.nbest[s], want, f"batch_call {dtype} pos {pos} stream {s} ({n} frames)")
            assert ids[s] == _best_ids(want)
        prev_ids = ids
    assert not s2t._batches and prev_ids[0] != prev_ids[1]
    s2t.tsync_tables.clear()
    # --- the pool: streams join late, pause a tick, end at different ticks; five live streams grow the slab of four
    plan = [("a", 40000, 0, None), ("b", 30000, 0, 2), ("c", 45000, 1, None), ("d", 25000, 2, 3), ("e", 40000, 2, None)]
    pw = {sid: synth_waveform(60 + k, n) for k, (sid, n, _, _) in enumerate(plan)}
    pool = s2t.stream_pool()
    pos = {sid: 0 for sid, *_ in plan}
    done, t, slots_seen = set(), 0, set()
    while len(done) < len(plan):
        chunks = {}
        for sid, n, join, pause in plan:
            if sid in done or t < join or t == pause:
                continue
            nxt = min(n, pos[sid] + CH)
            chunks[sid] = (pw[sid][pos[sid]:nxt], nxt == n)
            pos[sid] = nxt
        slots_before = {sid: st["slot"] for sid, st in pool.streams.items()}
        out = pool.tick(chunks)
        for sid, (_, fin) in chunks.items():
            want, n = _one_shot_on_own_tables(s2t, sid)
            got = pool.nbest_last_tick[sid]
            if got is None:
                assert n == 0 and out[sid] == []
            else:
                _same(got, want, f"pool {dtype} tick {t} stream {sid} ({n} frames)")
                assert out[sid] == _best_ids(want)
            if fin:
                done.add(sid)
        for sid, st in pool.streams.items():  # a live stream keeps its slot, whatever joins, leaves or grows
            assert slots_before.get(sid, st["slot"]) == st["slot"]
            slots_seen.add(st["slot"])
        t += 1
        assert t < 20
    st = pool.tsync_state
    assert not pool.streams and st.n_free == st.n_slots and not st.frames  # every slot is back
    assert st.n_grown == 1 and st.n_slots == 8 and len(slots_seen) == 5


# ------------------------------------------------------------------------------------------- 8. the surface
def test_surface_refusals_and_capacity(tmp_path):
    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import synth_waveform

    cfgp = str(tmp_path / "config.yaml")
    s2t = _s2t(tmp_path, tsync_max_frames=8)
    with pytest.raises(NotImplementedError, match="ctc_weight=0.5.*pass ctc_weight=1.0"):
        Speech2TextStreaming(cfgp, None, search="tsync", ctc_weight=0.5)
    with pytest.raises(NotImplementedError, match="lm_train_config: a neural LM is not scored time-synchronously"):
        Speech2TextStreaming(cfgp, None, search="tsync", ctc_weight=1.0, lm_train_config="lm.yaml")
    for other in ("online", "greedy", "offline"):
        with pytest.raises(NotImplementedError, match=f"ngram_file with search='{other}'"):
            Speech2TextStreaming(cfgp, None, search=other, ngram_file="x.arpa")
    with pytest.raises(NotImplementedError, match="needs a model with a CTC head"):
        _s2t(tmp_path, model_ctc_weight=0.0)
    # search="online" still refuses the pool and batch_call, by the old names
    online = _s2t(tmp_path, search="online", ctc_weight=0.5, beam_size=2)
    with pytest.raises(NotImplementedError, match="the pool decodes greedily"):
        online.stream_pool()
    with pytest.raises(NotImplementedError, match="batch_call decodes greedily"):
        online.batch_call(torch.zeros(2, CH))
    # capacity: more encoder frames than tsync_max_frames = 8 raise by name, for one stream and for a pool
    wav = synth_waveform(70, 3 * CH)
    with pytest.raises(RuntimeError, match="tsync_max_frames = 8"):
        for pos in range(0, 3 * CH, CH):
            s2t(wav[pos:pos + CH], is_final=False)
    s2t.reset()
    pool = s2t.stream_pool()
    with pytest.raises(RuntimeError, match="tsync_max_frames = 8"):
        for pos in range(0, 3 * CH, CH):
            pool.tick({"a": (wav[pos:pos + CH], False)})
