"""The transducer's default beam search as a batched device walk (em_transducer_beam_search, csrc/transducer_beam.hip;
BeamSearchTransducer.beam_device / search_batch) on the MI355X.

Three references, in the order of what they prove:
  * the primitives, bit for bit: a step's log-probability rows are those of em_transducer_dec_step +
    em_transducer_joint_logp called for each row alone (`test_step_rows_equal_the_primitives`) - the premise of
  * the host-driven route, `default_beam_search` per utterance: the same label sequences in the same order and scores
    equal to 1e-9 relative (both routes sum the same float32 log-probabilities in double), with no margin;
  * the float64 restatement tests/transducer_ref.py on the peaked model, on encoder seeds whose every decision - each
    pop, top-k boundary, end test and the final order - has a float64 margin above the log-probability bound of the
    scores it compares (tests/transducer_beam_margins.py; selected on the CPU beforehand, asserted again here).

Models, encoder rows and bounds are those of tests/test_gpu_transducer.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import transducer_ref as R
from tests.scratch_fill import BIG, ONES, ZERO, fill_bytes
from tests.test_gpu_transducer import D, DTYPES, E_LOGP_PEAKED, PEAK_SCALE, PEAKED, _enc, _model, _ragged
from tests.transducer_beam_margins import beam_search_margins, terms

pytestmark = pytest.mark.gpu

CELLS = [("lstm", 1, 64, 64, 50), ("gru", 2, 320, 320, 300)]
IDS = ["-".join(map(str, c)) for c in CELLS]
RUNNING, ENDED, EXP_LIMIT, CAP_EXPANSIONS = 0, 1, 2, 3


def _bs(model, beam, **kw):
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

    return BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, **kw)


def _batch(seeds_lens, dtype):
    """Utterance b = the N(0, 1) rows of encoder seed s_b, (T_b, D), zero-padded to the longest."""
    T = max(n for _, n in seeds_lens)
    act = torch.bfloat16 if dtype == "bfloat16" else torch.float32
    dev = torch.zeros(len(seeds_lens), T, D, dtype=act, device="cuda")
    enc64 = []
    for b, (s, n) in enumerate(seeds_lens):
        d, e = _enc(s, (n, D), dtype)
        dev[b, :n] = d
        enc64.append(e)
    return dev, enc64, [n for _, n in seeds_lens]


def _same(got, want, what):
    assert [h.yseq for h in got] == [h.yseq for h in want], what
    for g, w in zip(got, want):
        assert abs(g.score - w.score) <= 1e-9 * abs(w.score), (what, g.score, w.score)


# ---------------------------------------------------------------------- 1. the bitwise premise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", CELLS, ids=IDS)
def test_step_rows_equal_the_primitives(cell, dtype):
    """Eight steps of the walk on B = 5 utterances (lengths 6, 2, 3, 4, 5; beam 2; lin_out x 40 with the blank raised by
    32 so that frames end at different steps; weights seed 51 / 11, encoder rows seed 81): after every step, the
    log-probability row of every utterance that took it equals, bit for bit, em_transducer_joint_logp for that row alone
    on the lin_dec row that em_transducer_dec_step gives, one label at a time and one row per call, for the hypothesis
    the step's trace names.  At one step at least the rows stand at different frames with different prefixes."""
    model, p, _, _ = _model(*cell, dtype, 51 if cell == PEAKED else 11, out_scale=PEAK_SCALE, out_bias=(0, 32.0))
    dec, jn = model.decoder, model.joint_network
    olens = [6, 2, 3, 4, 5]
    enc_dev, _ = _enc(81, (5, 6, D), dtype)
    bs = _bs(model, 2)
    bs.beam_device(enc_dev, olens, max_steps=8, trace=True)
    steps = bs.last_beam["steps"]
    assert len(steps) == 8
    enc_proj = [jn.enc_proj_device(enc_dev[b, : olens[b]]) for b in range(5)]
    proj = {}

    def lin_dec_row(y):
        if y not in proj:
            state = dec.init_state(1, "cuda") if len(y) == 1 else lin_dec_row(y[:-1])[1]
            _, q, st = dec.step_device(torch.tensor([y[-1]], dtype=torch.int32, device="cuda"), state)
            proj[y] = (q, st)
        return proj[y]

    spread = rows = 0
    for logp, tr in steps:
        live = [b for b in range(5) if int(tr[b, 0]) == 1]
        where = set()
        for b in live:
            t, n = int(tr[b, 1]), int(tr[b, 3])
            y = tuple(tr[b, 4 : 4 + n].tolist())
            assert y[0] == 0 and 0 <= t < olens[b]
            where.add((t, y))
            alone = jn.logp_device(dec, enc_proj[b][t : t + 1], lin_dec_row(y)[0])[0].cpu()
            assert torch.equal(alone.view(torch.int32), logp[b].view(torch.int32)), (b, t, y)
            rows += 1
        if len(live) == 5 and len({t for t, _ in where}) >= 2 and len({y for _, y in where}) >= 3:
            spread += 1
    print(f"\nstep parity {cell} {dtype}: {rows} rows equal, {spread} steps with rows at different frames and prefixes")
    assert spread >= 1


# ---------------------------------------------------------------------- 2. the device route equals the host route
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T", [(5, 7), (33, 5)])
@pytest.mark.parametrize("cell", CELLS, ids=IDS)
def test_device_route_equals_host_route(cell, B, T, dtype):
    """A ragged batch (lengths include 1 and T) at beam 2, 4 and 10 with nbest = beam: `search_batch` returns what
    `default_beam_search` returns per utterance - the same label sequences in the same order, scores equal to 1e-9
    relative.  Recipe weights seed 11 with the blank raised by 3 (a flat softmax otherwise takes hundreds of expansions
    per frame at beam 10, test 4), encoder rows seed 12: every utterance stays on the device."""
    model, _, _, _ = _model(*cell, dtype, 11, out_bias=(0, 3.0))
    olens = _ragged(B, T)
    assert 1 in olens and T in olens
    enc_dev, _ = _enc(12, (B, T, D), dtype)
    for beam in (2, 4, 10):
        bs = _bs(model, beam, nbest=beam)
        got = bs.search_batch(enc_dev, olens)
        info = bs.last_beam
        assert bs.last_routes == ["device"] * B, (beam, info["status"].tolist())
        assert (info["status"][:, 0] == ENDED).all() and info["needed"] <= info["enqueued"]
        for b in range(B):
            _same(got[b], bs.default_beam_search(enc_dev[b, : olens[b]], utt=b), (beam, b))
            assert len(got[b]) == beam and all(h.dec_state is None for h in got[b])
        print(f"\nroutes {cell} B={B} {dtype} beam {beam}: {info['needed']} steps needed, {info['enqueued']} enqueued, "
              f"most expansions in a frame {int(info['status'][:, 3].max())}")


# ---------------------------------------------------------------------- 3. against float64
# (encoder seed, frames) per utterance, from the CPU scan described in the test's docstring
F64_CASES = {"float32": {2: [(66, 7), (74, 4), (76, 7), (63, 1), (79, 4)],
                         4: [(66, 7), (74, 4), (76, 7), (63, 1), (79, 4)],
                         10: [(66, 7), (74, 4), (76, 7), (63, 1), (79, 4)]},
             "bfloat16": {2: [(343, 5), (164, 3), (201, 3), (63, 1)]}}


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_search_equals_the_float64_restatement(dtype):
    """`search_batch` on the peaked model (weights seed 51, lin_out x 40, blank raised by 32) against `R.beam_search`
    per utterance, nbest = beam: the same label sequences in the same order, scores within (labels + frames) x
    E_LOGP_PEAKED.

    The encoder seeds were chosen on the CPU with the restatement alone (tests/transducer_beam_margins.py, 64
    expansions per frame at most): seeds 61..84 at T = 7, 4, 1 and beams 2, 4, 10 in both dtypes, and seeds 61..699 at
    T = 2, 3, 5 and beams 2, 4 in bf16.  Kept are the cases whose smallest margin per log-probability term - over every
    pop, top-k boundary, end test and the final order - exceeds E_LOGP_PEAKED, so that a device within the bound decides
    as float64 does:
        float32  (bound 3.2e-5)  seed, T: margin at beam 2 / 4 / 10
                 66, 7: 2.29e-3 / 2.29e-3 / 2.27e-4    74, 4: 2.05e-1 / 4.42e-3 / 1.11e-3    76, 7: 7.63e-4 / 7.63e-4 / 4.70e-4
                 63, 1: 1.59 / 1.04e-1 / 3.93e-2       79, 4: 3.17e-3 / 3.17e-3 / 5.37e-5
        bfloat16 (bound 3.1e-1)  beam 2 only: 343, 5: 0.363   164, 3: 0.632   201, 3: 0.669   63, 1: 1.59
    In bf16 the bound is four orders above float32's and no multi-frame case of the scan passes it at beam 4 or 10 (two
    single cases at beam 4: seed 447 T = 2 at 0.312, seed 68 T = 1 at 0.33 - not a batch of three), so bf16 is held to
    float64 at beam 2 and to the host route at every beam (test 2).  The existing cell (seed 61, T = 7) does not pass
    this criterion: its smallest margin per term is 5.5e-6 (float32), and it needs more than 64 expansions in a frame.
    The margins are asserted again below; no case is skipped."""
    model, p, _, _ = _model(*PEAKED, dtype, 51, out_scale=PEAK_SCALE, out_bias=(0, 32.0))
    E = E_LOGP_PEAKED[dtype]
    for beam, cases in F64_CASES[dtype].items():
        enc_dev, enc64, olens = _batch(cases, dtype)
        assert len(cases) >= 3 and len(set(olens)) >= 3
        bs = _bs(model, beam, nbest=beam)
        got = bs.search_batch(enc_dev, olens)
        assert bs.last_routes == ["device"] * len(cases)
        for b, (seed, T) in enumerate(cases):
            want, margin, most = beam_search_margins(R.model_logits_fn(p, enc64[b]), T, p.V, beam, beam, max_expansions=64)
            assert want is not None and margin > E, (seed, T, beam, margin)
            assert [h.yseq for h in got[b]] == [y for _, y in want], (seed, T, beam)
            err = max(abs(h.score - s) / terms(y, T) for h, (s, y) in zip(got[b], want))
            print(f"\nfloat64 {dtype} beam {beam} seed {seed} T {T}: margin/term {margin:.3g}, score err/term {err:.3e}, "
                  f"most expansions {most}")
            for h, (s, y) in zip(got[b], want):
                assert abs(h.score - s) <= terms(y, T) * E, (seed, T, beam, y)


# ---------------------------------------------------------------------- 4. overflow falls back
@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_falls_back_to_the_host_route(dtype):
    """Unpeaked recipe weights (seed 200) at beam 10: the restatement, on the CPU, needs up to 320 expansions in a frame
    for encoder seed 300 at T = 12 and 156 for seed 301 at T = 3 - above the walk's capacity of expansions per frame -
    and at most 41 / 48 / 47 for seeds 304 / 308 / 310 at T = 3.  The first two stop with the capacity status, not a
    fault, and come back from `search_batch` as `default_beam_search` gives them; the other three come from the walk."""
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    model, _, _, _ = _model(*CELLS[0], dtype, 200)
    cases = [(300, 12), (304, 3), (301, 3), (308, 3), (310, 3)]
    enc_dev, _, olens = _batch(cases, dtype)
    bs = _bs(model, 10, nbest=10)
    got = bs.search_batch(enc_dev, olens)
    st = bs.last_beam["status"]
    print(f"\noverflow {dtype}: status rows {st.tolist()}, routes {bs.last_routes}")
    assert bs.last_routes == ["host", "device", "host", "device", "device"]
    assert st[:, 0].tolist() == [CAP_EXPANSIONS, ENDED, CAP_EXPANSIONS, ENDED, ENDED]
    assert int(st[0, 3]) == int(st[2, 3]) == beam_limits()["expansions"] and int(st[:, 3].max()) == beam_limits()["expansions"]
    assert 0 <= int(st[0, 1]) < 12 and 0 <= int(st[2, 1]) < 3
    for b in range(len(cases)):
        _same(got[b], bs.default_beam_search(enc_dev[b, : olens[b]], utt=b), b)


# ---------------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_one_frame_and_a_short_beside_a_long_utterance(dtype):
    """T = 1 alone; a length-1 utterance beside one of length T = 9 (it ends after its frame, the other walks on); each
    row of the batch equals the utterance decoded alone through `__call__`."""
    model, _, _, _ = _model(*CELLS[0], dtype, 11, out_bias=(0, 3.0))
    bs = _bs(model, 4, nbest=4)
    enc_dev, _ = _enc(14, (2, 9, D), dtype)
    one = bs.search_batch(enc_dev[:1, :1].contiguous(), [1])
    assert bs.last_routes == ["device"] and len(one[0]) == 4
    _same(one[0], bs.default_beam_search(enc_dev[0, :1], utt=0), "T = 1")
    got = bs.search_batch(enc_dev, [1, 9])
    st = bs.last_beam["status"]
    assert bs.last_routes == ["device", "device"] and st[:, 0].tolist() == [ENDED, ENDED]
    assert int(st[0, 2]) < int(st[1, 2]) and st[:, 1].tolist() == [0, 8]  # (expansions; the frame each ended in)
    _same(got[0], one[0], "length 1 beside length 9")
    _same(got[1], bs.default_beam_search(enc_dev[1], utt=1), "length 9 beside length 1")
    _same(bs(enc_dev[1]), got[1], "__call__")


def test_edge_beam_of_the_whole_vocabulary():
    """V = 4 and beam 3 = V - 1, beam 4 = V and beam 7 > V (beam = min(beam, V), labels per expansion min(beam, V - 1)):
    as the host route, which clamps alike."""
    model, _, _, _ = _model("lstm", 1, 64, 64, 4, "float32", 11, out_bias=(0, 1.0))
    enc_dev, _ = _enc(15, (3, 5, D), "float32")
    for beam in (3, 4, 7):
        bs = _bs(model, beam, nbest=beam)
        got = bs.search_batch(enc_dev, [5, 1, 3])
        assert bs.last_routes == ["device"] * 3
        for b, n in enumerate([5, 1, 3]):
            _same(got[b], bs.default_beam_search(enc_dev[b, :n], utt=b), (beam, b))


def test_edge_exact_ties_take_the_lowest_id():
    """The construction of test_exact_ties_take_the_lowest_id: all-zero lin_out weights and equal biases, so every
    log-probability of a row is the same number and every rank round and every pop is an exact tie.  V = 1027, beam 3:
    the labels taken are 1, 2, 3 (the lowest ids), the pops go to the earliest inserted, and the lists equal the host
    route's, order included; with the blank raised the winner is the all-blank hypothesis."""
    cell = ("lstm", 1, 64, 64, 1027)
    for shift in (0.0, 9.0):
        model, _, _, sd = _model(*cell, "float32", 43)
        sd = {k: v.clone() for k, v in sd.items()}
        sd["joint_network.lin_out.weight"].zero_()
        sd["joint_network.lin_out.bias"].fill_(0.25)
        sd["joint_network.lin_out.bias"][0] += shift
        model.load_state_dict(sd, strict=True)
        bs = _bs(model, 3, nbest=8)
        enc_dev, _ = _enc(44, (2, 2, D), "float32")
        got = bs.search_batch(enc_dev, [2, 1])
        assert bs.last_routes == ["device", "device"]
        for b, n in enumerate([2, 1]):
            _same(got[b], bs.default_beam_search(enc_dev[b, :n], utt=b), (shift, b))
            assert all(set(h.yseq) <= {0, 1, 2, 3} for h in got[b])
        if shift:
            assert got[0][0].yseq == [0] and got[1][0].yseq == [0]
    from tests import test_gpu_transducer as G

    for k in [k for k in G._cache if 43 in k]:  # (the cached model of this cell carries the test's weights)
        del G._cache[k]


def test_edge_give_up_names_the_utterance_and_the_frame(monkeypatch):
    """The give-up case of test_beam_search_gives_up_on_a_frame_it_cannot_leave through `search_batch` with B = 2 (the
    peaked model with the blank lowered by 100, limit 20): the walk stops both utterances at frame 0 with the
    expansion-limit status and the host route raises for the first.  Then a model that does leave its frames, with the
    limit set to what utterance 1 needs in its worst frame - more than the one frame of utterance 0 needs: utterance 0
    comes from the walk, utterance 1 is the one named, with its frame."""
    from espnet_amd.asr.transducer import beam_search_transducer as B

    model, _, _, _ = _model(*PEAKED, "float32", 51, out_scale=PEAK_SCALE, out_bias=(0, -100.0))
    monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", 20)
    enc_dev, _ = _enc(61, (2, 3, D), "float32")
    bs = B.BeamSearchTransducer(model.decoder, model.joint_network, beam_size=2)
    res = bs.beam_device(enc_dev, [3, 3])
    assert res == [None, None]
    assert bs.last_beam["status"][:, :2].tolist() == [[EXP_LIMIT, 0], [EXP_LIMIT, 0]]
    assert bs.last_beam["status"][:, 3].tolist() == [20, 20]
    with pytest.raises(RuntimeError, match="utterance 0, frame 0 not left after 20 expansions"):
        bs.search_batch(enc_dev, [3, 3])
    model2, _, _, _ = _model(*CELLS[0], "float32", 11, out_bias=(0, 3.0))
    bs2 = B.BeamSearchTransducer(model2.decoder, model2.joint_network, beam_size=4)
    enc2, _ = _enc(12, (2, 4, D), "float32")
    monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", 1000)
    bs2.search_batch(enc2, [1, 4])
    per_frame = bs2.last_beam["status"][:, 3].tolist()
    assert per_frame[1] > per_frame[0] >= 4, per_frame  # (utterance 1 meets a frame that needs more expansions)
    limit = per_frame[1] - 1  # (one expansion short of what utterance 1's worst frame takes)
    monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", limit)
    with pytest.raises(RuntimeError, match=f"utterance 1, frame [1-3] not left after {limit} expansions"):
        bs2.search_batch(enc2, [1, 4])
    assert bs2.last_beam["status"][:, 0].tolist() == [ENDED, EXP_LIMIT]


def _raw(model, enc_dev, olens, beam, ws_delta=0, fill=None, B=None):
    """em_transducer_beam_search called directly, every step in one call (steps behind the end return at once).
    Returns (rc, status, count, scores, lens, tokens) with host copies."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    dec, jn = model.decoder, model.joint_network
    lib = L.load()
    w, keep = dec.weights("cuda")
    nB, T = (int(enc_dev.shape[0]) if B is None else B), int(enc_dev.shape[1])
    lim = beam_limits()
    enc_proj = jn.enc_proj_device(enc_dev)
    need = int(lib.em_transducer_beam_workspace_bytes(dec.em_dtype, C.byref(w), min(nB, 64), T, min(beam, lim["beam"])))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if fill is not None:
        fill_bytes(ws, fill)
    Lmax, ncap = 2 * T + 16, lim["kept"]
    ol = torch.tensor(list(olens) + [1] * (nB - len(olens)), dtype=torch.int32).cuda()
    status = torch.zeros(nB, 4, dtype=torch.int32, device="cuda")
    tok = torch.zeros(nB, ncap, Lmax, dtype=torch.int32, device="cuda")
    lens = torch.zeros(nB, ncap, dtype=torch.int32, device="cuda")
    score = torch.zeros(nB, ncap, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(nB, dtype=torch.int32, device="cuda")
    rc = lib.em_transducer_beam_search(dec.em_dtype, C.byref(w), L.ptr(enc_proj), L.ptr(ol), nB, T, beam, 1000, Lmax, ncap, 1,
                                       T * 40, L.ptr(status), L.ptr(tok), L.ptr(lens), L.ptr(score), L.ptr(cnt), None, None,
                                       L.ptr(ws), need + ws_delta, L.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, status.cpu(), cnt.cpu(), score.cpu(), lens.cpu(), tok.cpu()


def test_edge_refused_arguments_launch_nothing():
    """A workspace one byte short, B = 65 and a beam above the limit: EM_ERR_UNSUPPORTED, and no output is touched."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    model, _, _, _ = _model(*CELLS[0], "float32", 11, out_bias=(0, 3.0))
    enc_dev, _ = _enc(12, (3, 4, D), "float32")
    assert _raw(model, enc_dev, [4, 1, 2], 4)[0] == L.EM_OK
    for kw in (dict(ws_delta=-1), dict(B=65), dict(beam=beam_limits()["beam"] + 1)):
        args = dict(beam=4)
        args.update(kw)
        big = torch.zeros(65, 4, D, device="cuda") if "B" in kw else enc_dev
        rc, status, cnt, score, lens, tok = _raw(model, big, [4, 1, 2], **args)
        assert rc == L.EM_ERR_UNSUPPORTED, kw
        assert not status.any() and not cnt.any() and not lens.any() and not tok.any()
    bs = _bs(model, beam_limits()["beam"] + 1)
    with pytest.raises(NotImplementedError, match="beam_size"):
        bs.beam_device(enc_dev, [4, 1, 2])
    got = bs.search_batch(enc_dev[:1], [2])  # (a beam above the walk's limit stays on the host route)
    assert bs.last_routes == ["host"] and len(got[0]) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_workspace_contents_are_ignored(dtype):
    """The workspace pre-filled with 0x00, 0xFF (NaN) and 0x7F (huge) bytes: the same status rows, counts, scores,
    lengths and labels, bit for bit (the gru cell with two layers, beam 4, a ragged batch of 5)."""
    model, _, _, _ = _model(*CELLS[1], dtype, 11, out_bias=(0, 3.0))
    olens = _ragged(5, 6)
    enc_dev, _ = _enc(12, (5, 6, D), dtype)
    ref = None
    for fill in (ZERO, ONES, BIG):
        rc, status, cnt, score, lens, tok = _raw(model, enc_dev, olens, 4, fill=fill)
        assert rc == 0 and (status[:, 0] == ENDED).all() and (cnt >= 4).all()
        out = [status.tolist(), cnt.tolist()]
        for b in range(5):
            for i in range(int(cnt[b])):
                n = int(lens[b, i])
                out.append((float(score[b, i]).hex(), tok[b, i, :n].tolist()))
                assert n >= 1 and int(tok[b, i, 0]) == 0 and np.isfinite(float(score[b, i]))
        if ref is None:
            ref = out
        assert out == ref, fill
