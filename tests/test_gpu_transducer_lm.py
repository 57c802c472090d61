"""Shallow fusion of a SequentialRNNLM into the transducer's default beam search on the MI355X: the row primitive
em_transducer_lm_step, the walk em_transducer_beam_search_lm (BeamSearchTransducer(lm=...).beam_device / search_batch), the
host-driven route with the LM, and Speech2Text with lm_train_config.

References, in the order of what they prove:
  * the float64 restatement tests/transducer_lm_ref.py `lm_step` for the primitive;
  * the primitive, bit for bit: a step's LM row is em_transducer_lm_step replayed one label at a time and one row per
    call for the hypothesis the step's trace names, a carried hypothesis included - the premise of
  * the host-driven route, `default_beam_search` per utterance with the LM: the same lists, scores equal to 1e-9
    relative, with no margin (both routes add the LM term in double, product and sum rounded separately);
  * the float64 restatement `beam_search_lm_margins` on the peaked model, on encoder seeds chosen on the CPU.

Transducer models are the cells of tests/test_gpu_transducer_beam.py; the LMs are oracle.weights.recipe_state_dict
weights with the seeds LM_SEEDS names.  The restatement is fed the same inputs: the matrices as the compute dtype holds
them, in float64 arithmetic.

Bounds (the convention of tests/test_gpu_transducer.py: 4 x the largest error seen on the MI355X over the cells of
`test_lm_step_primitive`; seen values in brackets; the run's printed output is profiles/transducer_lm_pytest_gpu.txt):
    LM logp          f32 5.4e-6 [1.34e-6]   bf16 3.0e-3 [7.50e-4]
    LM logp, peaked  f32 4.4e-6 [1.10e-6]   bf16 2.3e-2 [5.57e-3]   (decoder.weight x LM_PEAK_SCALE, the LM of the float64 test)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import transducer_lm_ref as LR
from tests import transducer_ref as R
from tests.scratch_fill import BIG, ONES, ZERO, fill_bytes
from tests.test_gpu_transducer import D, DTYPES, E_LOGP_PEAKED, PEAK_SCALE, PEAKED, _enc, _model, _ragged, _waves
from tests.test_gpu_transducer_beam import CELLS, ENDED, EXP_LIMIT, _batch, _same
from tests.transducer_beam_margins import beam_search_margins, terms

pytestmark = pytest.mark.gpu

# (rnn_type, nlayers, unit, nhid, tie_weights); gru 2 x 96 -> 200 pads to 128 / 256 and has unit != nhid
LMS = [("lstm", 1, 64, 64, False), ("gru", 2, 96, 200, False), ("lstm", 2, 64, 64, True)]
LM_SEEDS = {LMS[0]: 21, LMS[1]: 22, LMS[2]: 23}
# (transducer cell, LM) pairs: the LM's vocabulary is the cell's
PAIRS = [(CELLS[0], LMS[0]), (CELLS[1], LMS[1]), (CELLS[0], LMS[2])]
PAIR_IDS = ["lstm1x64-lm_lstm1x64", "gru2x320-lm_gru2x96_200", "lstm1x64-lm_lstm2x64_tied"]
LM_PEAKED = ("lstm", 1, 64, 64, False)
LM_PEAK_SCALE = 20.0  # decoder.weight scaled: LM rows that move a decision of the peaked transducer
LM_PEAKED_SEED = 31
E_LM = {"float32": 5.4e-6, "bfloat16": 3.0e-3}
E_LM_PEAKED = {"float32": 4.4e-6, "bfloat16": 2.3e-2}
_lms = {}


def _lm(cell, V, dtype, seed, out_scale=1.0):
    """(SequentialRNNLM on the GPU, restatement parameters as the compute dtype holds them); built once per argument set."""
    key = (cell, V, dtype, seed, out_scale)
    if key not in _lms:
        from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
        from oracle.weights import recipe_state_dict

        kind, nlayers, unit, nhid, tie = cell
        lm = SequentialRNNLM(V, unit=unit, nhid=nhid, nlayers=nlayers, rnn_type=kind, tie_weights=tie, compute_dtype=dtype)
        new = recipe_state_dict({k: tuple(v.shape) for k, v in lm.state_dict().items()}, seed)
        if tie:
            new["decoder.weight"] = new["encoder.weight"]
        new["decoder.weight"] = new["decoder.weight"] * out_scale
        lm.load_state_dict(new, strict=True)
        lm.cuda().eval()
        _lms[key] = (lm, LR.LmParams(new, kind, round_to=torch.bfloat16 if dtype == "bfloat16" else None), new)
    return _lms[key]


def _bs(model, beam, lm=None, **kw):
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

    return BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, lm=lm, **kw)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda()


# ---------------------------------------------------------------------- 1. the row primitive
PRIM = [(LMS[0], 50, 1.0), (LMS[1], 300, 1.0), (LMS[2], 50, 1.0), (LM_PEAKED, 50, LM_PEAK_SCALE)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell,V,scale", PRIM, ids=["lstm1x64", "gru2x96_200", "lstm2x64_tied", "lstm1x64_peaked"])
def test_lm_step_primitive(cell, V, scale, dtype):
    """em_transducer_lm_step at n = 3, 33 and 64 rows against the float64 restatement: step 1 from the zero state (row 0
    reads sos = V - 1, labels seed 13), step 2 from the returned states, step 3 masked (rows with mask == 0 copy their
    state bit for bit and leave their logp rows as they were; row 0 runs, the last row does not).  The same rows through
    SequentialRNNLM.batch_score (the tiled-GEMM route) lie within twice the bound; row r of the n = 33 call equals, bit
    for bit, the one-row call for that row; pad channels stay zero.
    Seen on the MI355X (profiles/transducer_lm_pytest_gpu.txt), largest logp error over n and the three steps:
        lstm 1 x 64          f32 7.39e-7   bf16 2.79e-4      gru 2 x 96 -> 200, V 300   f32 1.34e-6   bf16 7.50e-4
        lstm 2 x 64, tied    f32 7.68e-7   bf16 2.42e-4      lstm 1 x 64, head x 20     f32 1.10e-6   bf16 5.57e-3
    (batch_score on the same rows: 7.39e-7 / 2.21e-4, 1.34e-6 / 6.64e-4, 7.31e-7 / 2.24e-4, 8.18e-7 / 5.12e-3.)"""
    seed = LM_PEAKED_SEED if scale != 1.0 else LM_SEEDS[cell]
    lm, p, _ = _lm(cell, V, dtype, seed, scale)
    bound = (E_LM_PEAKED if scale != 1.0 else E_LM)[dtype]
    nhid = cell[3]
    worst = worst_gemm = 0.0
    for n in (3, 33, 64):
        g = torch.Generator().manual_seed(13)
        toks = [torch.randint(0, V, (n,), generator=g) for _ in range(3)]
        toks[0][0] = V - 1
        mask = (torch.rand(n, generator=g) < 0.6).to(torch.int32)
        mask[0], mask[-1] = 1, 0
        lp1, s1 = lm.step_rows(_i32(toks[0]), lm.init_rows_state(n, "cuda"))
        lp2, s2 = lm.step_rows(_i32(toks[1]), s1)
        lp3 = torch.full_like(lp2, 7.0)
        _, s3 = lm.step_rows(_i32(toks[2]), s2, mask=mask.cuda(), logp=lp3)
        torch.cuda.synchronize()
        dead = ~mask.bool().cuda()
        assert torch.equal(s3[0][:, dead], s2[0][:, dead]) and torch.equal(s3[1][:, dead], s2[1][:, dead])
        assert bool((lp3[dead] == 7.0).all()) and not bool((lp3[~dead] == 7.0).any())
        for s in (s1, s2, s3):
            assert float(s[0][:, :, nhid:].abs().max() if s[0].shape[2] > nhid else 0.0) == 0.0
            assert float(s[1][:, :, nhid:].abs().max() if s[1].shape[2] > nhid else 0.0) == 0.0
        # the tiled-GEMM route on the same rows
        xs = torch.zeros(n, 1, device="cuda")
        g1, st = lm.batch_score(toks[0].view(n, 1).cuda(), None, xs)
        g2, _ = lm.batch_score(toks[1].view(n, 1).cuda(), st, xs)
        got = [t.cpu().double() for t in (lp1, lp2, lp3)]
        gemm = [g1.cpu().double(), g2.cpu().double()]
        for r in range(n):
            state = p.init_state()
            for i in range(3):
                if i == 2 and not mask[r]:
                    break
                want, state, _ = LR.lm_step(p, int(toks[i][r]), state)
                worst = max(worst, float((got[i][r] - want).abs().max()))
                if i < 2:
                    worst_gemm = max(worst_gemm, float((gemm[i][r] - want).abs().max()))
        if n == 33:  # a row's result depends on that row's operands only
            for r in range(n):
                a1, t1 = lm.step_rows(_i32(toks[0][r : r + 1]), lm.init_rows_state(1, "cuda"))
                a2, _ = lm.step_rows(_i32(toks[1][r : r + 1]), t1)
                assert torch.equal(a1[0].view(torch.int32), lp1[r].view(torch.int32)), r
                assert torch.equal(a2[0].view(torch.int32), lp2[r].view(torch.int32)), r
                assert torch.equal(t1[0][:, 0], s1[0][:, r]) and torch.equal(t1[1][:, 0], s1[1][:, r])
    print(f"\nlm step {cell} V={V} x{scale:g} {dtype}: logp err {worst:.3e}  batch_score err {worst_gemm:.3e}")
    assert worst <= bound and worst_gemm <= 2 * bound


# ---------------------------------------------------------------------- 2. the bitwise premise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell,lmc", PAIRS, ids=PAIR_IDS)
def test_step_rows_equal_the_primitives(cell, lmc, dtype):
    """tests/test_gpu_transducer_beam.py's first test with an LM (lm_weight 0.3): eight traced steps on B = 5 utterances
    (lengths 6, 2, 3, 4, 5; beam 2; the same weights and encoder rows).  After every step the joint row of every
    utterance that took it equals the joint primitive as there, and its LM row equals, bit for bit,
    em_transducer_lm_step replayed one label at a time and one row per call - sos from the zero state, then the labels -
    for the hypothesis the trace names.  At least one traced step is a carried entry, whose LM row the head recomputes
    from the stored top h."""
    model, p, _, _ = _model(*cell, dtype, 51 if cell == PEAKED else 11, out_scale=PEAK_SCALE, out_bias=(0, 32.0))
    lm, _, _ = _lm(lmc, cell[4], dtype, LM_SEEDS[lmc])
    dec, jn = model.decoder, model.joint_network
    olens = [6, 2, 3, 4, 5]
    enc_dev, _ = _enc(81, (5, 6, D), dtype)
    bs = _bs(model, 2, lm=lm, lm_weight=0.3)
    bs.beam_device(enc_dev, olens, max_steps=8, trace=True)
    steps = bs.last_beam["steps"]
    assert len(steps) == 8 and all(len(s) == 3 for s in steps)
    enc_proj = [jn.enc_proj_device(enc_dev[b, : olens[b]]) for b in range(5)]
    proj, lmrow = {}, {}

    def lin_dec_row(y):
        if y not in proj:
            state = dec.init_state(1, "cuda") if len(y) == 1 else lin_dec_row(y[:-1])[1]
            _, q, st = dec.step_device(_i32([y[-1]]), state)
            proj[y] = (q, st)
        return proj[y]

    def lm_row(y):
        if y not in lmrow:
            if len(y) == 1:
                lmrow[y] = lm.step_rows(_i32([cell[4] - 1]), lm.init_rows_state(1, "cuda"))
            else:
                lmrow[y] = lm.step_rows(_i32([y[-1]]), lm_row(y[:-1])[1])
        return lmrow[y]

    rows = carried = 0
    for logp, tr, lm_logp in steps:
        for b in [b for b in range(5) if int(tr[b, 0]) == 1]:
            t, n = int(tr[b, 1]), int(tr[b, 3])
            y = tuple(tr[b, 4 : 4 + n].tolist())
            assert y[0] == 0 and 0 <= t < olens[b]
            alone = jn.logp_device(dec, enc_proj[b][t : t + 1], lin_dec_row(y)[0])[0].cpu()
            assert torch.equal(alone.view(torch.int32), logp[b].view(torch.int32)), (b, t, y)
            alone_lm = lm_row(y)[0][0].cpu()
            assert torch.equal(alone_lm.view(torch.int32), lm_logp[b].view(torch.int32)), (b, t, y, int(tr[b, 2]))
            rows += 1
            carried += int(tr[b, 2]) == 1
    print(f"\nlm step parity {cell} {lmc} {dtype}: {rows} rows equal, {carried} of them carried entries")
    assert carried >= 1


# ---------------------------------------------------------------------- 3. the device route equals the host route
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lm_weight", [0.3, 1.0])
@pytest.mark.parametrize("B,T", [(5, 7), (33, 5)])
@pytest.mark.parametrize("cell,lmc", PAIRS, ids=PAIR_IDS)
def test_device_route_equals_host_route(cell, lmc, B, T, lm_weight, dtype):
    """A ragged batch (lengths include 1 and T) at beam 2, 4 and 10 with nbest = beam: `search_batch` with the LM returns
    what `default_beam_search` with the LM returns per utterance - the same label sequences in the same order, scores
    equal to 1e-9 relative - and every utterance stays on the device.  Transducer weights and encoder rows as in
    tests/test_gpu_transducer_beam.py (seed 11 with the blank raised by 3, rows seed 12)."""
    model, _, _, _ = _model(*cell, dtype, 11, out_bias=(0, 3.0))
    lm, _, _ = _lm(lmc, cell[4], dtype, LM_SEEDS[lmc])
    olens = _ragged(B, T)
    assert 1 in olens and T in olens
    enc_dev, _ = _enc(12, (B, T, D), dtype)
    for beam in (2, 4, 10):
        bs = _bs(model, beam, lm=lm, lm_weight=lm_weight, nbest=beam)
        got = bs.search_batch(enc_dev, olens)
        info = bs.last_beam
        assert bs.last_routes == ["device"] * B, (beam, info["status"].tolist())
        assert (info["status"][:, 0] == ENDED).all() and info["needed"] <= info["enqueued"]
        for b in range(B):
            want = bs.default_beam_search(enc_dev[b, : olens[b]], utt=b)
            _same(got[b], want, (beam, b))
            # both routes see the same log-probability bits and add the LM term unfused, in the same order: the same
            # doubles (a contracted multiply-add on the device would differ in the last bit of some score)
            assert [float(h.score).hex() for h in got[b]] == [float(h.score).hex() for h in want], (beam, b)
            assert len(got[b]) == beam and all(h.dec_state is None and h.lm_state is None for h in got[b])
            assert all(h.lm_state is not None for h in want)
        print(f"\nlm routes {cell} {lmc} B={B} w={lm_weight} {dtype} beam {beam}: {info['needed']} steps needed, "
              f"most expansions in a frame {int(info['status'][:, 3].max())}")


# ---------------------------------------------------------------------- 4. lm_weight 0.0 is the search without an LM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell,lmc", PAIRS[:2], ids=PAIR_IDS[:2])
def test_zero_weight_is_the_search_without_an_lm(cell, lmc, dtype):
    """lm_weight = 0.0 with an LM: exactly the lists of the search without one, the scores bit for bit (beam 4, nbest 4, a
    ragged batch of 5; x + 0.0 * y == x for the finite y of a log-softmax row) - while lm_weight 1.0 changes some list."""
    model, _, _, _ = _model(*cell, dtype, 11, out_bias=(0, 3.0))
    lm, _, _ = _lm(lmc, cell[4], dtype, LM_SEEDS[lmc])
    olens = _ragged(5, 7)
    enc_dev, _ = _enc(12, (5, 7, D), dtype)
    plain = _bs(model, 4, nbest=4).search_batch(enc_dev, olens)
    bs = _bs(model, 4, lm=lm, lm_weight=0.0, nbest=4)
    zero = bs.search_batch(enc_dev, olens)
    assert bs.last_routes == ["device"] * 5
    for a, b in zip(plain, zero):
        assert [(h.yseq, float(h.score).hex()) for h in a] == [(h.yseq, float(h.score).hex()) for h in b]
    one = _bs(model, 4, lm=lm, lm_weight=1.0, nbest=4).search_batch(enc_dev, olens)
    assert any([(h.yseq, h.score) for h in a] != [(h.yseq, h.score) for h in b] for a, b in zip(plain, one))


# ---------------------------------------------------------------------- 5. against float64
LM_WEIGHT_F64 = 0.3
# (encoder seed, frames) per utterance, from the CPU scan described in the test's docstring
_F32_CASES = [(66, 7), (61, 4), (63, 1), (70, 7), (69, 4)]
F64_LM_CASES = {"float32": {2: _F32_CASES, 4: _F32_CASES, 10: _F32_CASES},
                "bfloat16": {2: [(343, 5), (164, 3), (201, 3), (63, 1)]}}
# (dtype, beam, encoder seed, frames): the 1-best with the LM differs from the 1-best without, both with margin
F64_LM_DIFFERS = [("float32", 4, 66, 7), ("float32", 10, 66, 7)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_search_with_lm_equals_the_float64_restatement(dtype):
    """`search_batch` with the peaked LM (LM_PEAKED, seed LM_PEAKED_SEED, decoder.weight x LM_PEAK_SCALE, lm_weight 0.3) on
    the peaked model of tests/test_gpu_transducer_beam.py (weights seed 51, lin_out x 40, blank raised by 32) against
    `beam_search_lm_margins` per utterance, nbest = beam: the same label sequences in the same order, scores within
    (labels + frames) x (E_LOGP_PEAKED + lm_weight x E_LM_PEAKED).

    The encoder seeds were chosen on the CPU with the restatement alone (64 expansions per frame at most), over the range
    tests/test_gpu_transducer_beam.py scanned: seeds 61..84 at T = 7, 4, 1 and beams 2, 4, 10 in both dtypes, and seeds
    61..699 at T = 2, 3, 5 and beams 2, 4 in bf16.  Kept are cases whose smallest margin per term - over every pop, top-k
    boundary, end test and the final order, the LM term counted with its weight - exceeds E_LOGP_PEAKED + 0.3 x
    E_LM_PEAKED, so that a device within the bounds decides as float64 does:
        float32  (bound 3.3e-5)  seed, T: margin at beam 2 / 4 / 10
                 66, 7: 7.91e-3 / 2.00e-3 / 1.50e-3    61, 4: 2.17e-3 / 1.73e-3 / 2.93e-4    63, 1: 1.63 / 1.04e-1 / 1.48e-3
                 70, 7: 4.81e-3 / 1.48e-3 / 3.44e-4    69, 4: 9.26e-2 / 6.36e-2 / 8.11e-4
        bfloat16 (bound 3.17e-1) beam 2 only: 343, 5: 0.437   164, 3: 0.613   201, 3: 0.693   63, 1: 1.63
    bf16 is dropped at beam 4 and 10: the scan has two single cases above the bound at beam 4 (seed 68 T = 1 at 0.33, seed
    609 T = 2 at 0.349 - not a batch of three utterances) and none at beam 10; there bf16 is held to the host route at
    every beam (test 3).  LM seed 31 and lm_weight 0.3 were kept because the LM then changes a 1-best with margin on both
    sides: for seed 66, T = 7 at beam 4 and 10 the restatement's 1-best with the LM is not its 1-best without (margin per
    term without the LM 2.29e-3 / 2.27e-4, above E_LOGP_PEAKED); the device must show both results.  No bf16 case of the
    scan differs with margin on both sides.  The margins are asserted again below; no case is skipped."""
    model, p, _, _ = _model(*PEAKED, dtype, 51, out_scale=PEAK_SCALE, out_bias=(0, 32.0))
    lm, lp, _ = _lm(LM_PEAKED, PEAKED[4], dtype, LM_PEAKED_SEED, LM_PEAK_SCALE)
    E = E_LOGP_PEAKED[dtype] + LM_WEIGHT_F64 * E_LM_PEAKED[dtype]
    lm_fn = LR.model_lm_fn(lp)
    assert F64_LM_CASES[dtype], "no case of the scan for this dtype"
    both = 0
    for beam, cases in F64_LM_CASES[dtype].items():
        enc_dev, enc64, olens = _batch(cases, dtype)
        assert len(cases) >= 3 and len(set(olens)) >= 3
        bs = _bs(model, beam, lm=lm, lm_weight=LM_WEIGHT_F64, nbest=beam)
        got = bs.search_batch(enc_dev, olens)
        assert bs.last_routes == ["device"] * len(cases)
        plain = _bs(model, beam, nbest=beam).search_batch(enc_dev, olens)
        for b, (seed, T) in enumerate(cases):
            fn = R.model_logits_fn(p, enc64[b])
            want, margin, most = LR.beam_search_lm_margins(fn, lm_fn, LM_WEIGHT_F64, T, p.V, beam, beam, max_expansions=64)
            assert want is not None and margin > E, (seed, T, beam, margin)
            assert [h.yseq for h in got[b]] == [y for _, y in want], (seed, T, beam)
            err = max(abs(h.score - s) / terms(y, T) for h, (s, y) in zip(got[b], want))
            print(f"\nfloat64 lm {dtype} beam {beam} seed {seed} T {T}: margin/term {margin:.3g}, score err/term {err:.3e}, "
                  f"most expansions {most}")
            for h, (s, y) in zip(got[b], want):
                assert abs(h.score - s) <= terms(y, T) * E, (seed, T, beam, y)
            if (dtype, beam, seed, T) in F64_LM_DIFFERS:  # the LM changes the 1-best, and the device shows both results
                want0, margin0, _ = beam_search_margins(fn, T, p.V, beam, beam, max_expansions=64)
                assert want0 is not None and margin0 > E_LOGP_PEAKED[dtype]
                assert want0[0][1] != want[0][1]
                assert plain[b][0].yseq == want0[0][1] and got[b][0].yseq == want[0][1]
                both += 1
    print(f"\nfloat64 lm {dtype}: {both} cases where the LM changes the 1-best, both results seen on the device")
    assert both >= 1 or dtype != "float32"  # (no bf16 case of the scan differs with margin on both sides)


# ---------------------------------------------------------------------- 6. stopped utterances take the host route
@pytest.mark.parametrize("dtype", DTYPES)
def test_stopped_utterances_fall_back_to_the_host_route_with_the_lm(monkeypatch, dtype):
    """Beam 4 on a batch of two (lengths 1 and 4): the walk, given one expansion per frame fewer than utterance 1 needs in
    its worst frame (MAX_EXPANSIONS_PER_FRAME lowered for the walk's call, as the give-up test of
    tests/test_gpu_transducer_beam.py lowers it), stops utterance 1 with the expansion-limit status; `search_batch`
    decodes it by the host route with the LM and returns what that route returns alone, utterance 0 comes from the walk."""
    from espnet_amd.asr.transducer import beam_search_transducer as B

    model, _, _, _ = _model(*CELLS[0], dtype, 11, out_bias=(0, 3.0))
    lm, _, _ = _lm(LMS[0], 50, dtype, LM_SEEDS[LMS[0]])
    enc_dev, _ = _enc(12, (2, 4, D), dtype)
    bs = _bs(model, 4, lm=lm, lm_weight=1.0, nbest=4)
    free = bs.search_batch(enc_dev, [1, 4])
    per_frame = bs.last_beam["status"][:, 3].tolist()
    assert bs.last_routes == ["device", "device"] and per_frame[1] > per_frame[0] >= 4, per_frame
    walk = bs.beam_device

    def lowered(*a, **kw):
        monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", per_frame[1] - 1)
        try:
            return walk(*a, **kw)
        finally:
            monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", 1000)

    monkeypatch.setattr(bs, "beam_device", lowered)
    got = bs.search_batch(enc_dev, [1, 4])
    assert bs.last_routes == ["device", "host"]
    assert bs.last_beam["status"][:, 0].tolist() == [ENDED, EXP_LIMIT]
    host = bs.default_beam_search(enc_dev[1, :4], utt=1)
    assert [(h.yseq, h.score) for h in got[1]] == [(h.yseq, h.score) for h in host]
    assert all(h.lm_state is not None for h in got[1])
    _same(got[1], free[1], "host route = the walk that was left alone")
    _same(got[0], free[0], "utterance 0")


# ---------------------------------------------------------------------- 7. workspace contents, refused arguments
def _raw(model, lm, enc_dev, olens, beam, lm_weight=0.3, ws_delta=0, fill=None, B=None, lw_edit=None, step_lm=False):
    """em_transducer_beam_search_lm called directly, every step in one call.  Returns (rc, status, count, scores, lens,
    tokens) with host copies."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    dec, jn = model.decoder, model.joint_network
    lib = L.load()
    w, keep = dec.weights("cuda")
    lw = lw_keep = None
    if lm is not None:
        src, lw_keep = lm.transducer_lm_weights("cuda")
        lw = L.EmTransducerLmWeights()
        C.memmove(C.byref(lw), C.byref(src), C.sizeof(lw))
        for k, v in (lw_edit or {}).items():
            setattr(lw, k, v)
    lw_ref = C.byref(lw) if lw is not None else None
    nB, T = (int(enc_dev.shape[0]) if B is None else B), int(enc_dev.shape[1])
    lim = beam_limits()
    enc_proj = jn.enc_proj_device(enc_dev)
    good = lm.transducer_lm_weights("cuda")[0] if lm is not None else None
    need = int(lib.em_transducer_beam_workspace_bytes_lm(dec.em_dtype, C.byref(w), C.byref(good) if good is not None else None,
                                                         min(nB, 64), T, min(beam, lim["beam"])))
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
    slm = torch.zeros(nB, dec.vocab_size, dtype=torch.float32, device="cuda") if step_lm else None
    rc = lib.em_transducer_beam_search_lm(dec.em_dtype, C.byref(w), lw_ref, lm_weight, L.ptr(enc_proj), L.ptr(ol), nB, T, beam,
                                          1000, Lmax, ncap, 1, T * 40, L.ptr(status), L.ptr(tok), L.ptr(lens), L.ptr(score),
                                          L.ptr(cnt), None, None, L.ptr(slm), L.ptr(ws), need + ws_delta,
                                          L.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, status.cpu(), cnt.cpu(), score.cpu(), lens.cpu(), tok.cpu()


def test_refused_arguments_launch_nothing():
    """A workspace one byte short (the LM's part counts), B = 65, a beam above the limit, an LM of another vocabulary, an
    LM whose hidden size is not padded, the LM trace without an LM: refused before any launch, no output is touched."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import beam_limits

    model, _, _, _ = _model(*CELLS[0], "float32", 11, out_bias=(0, 3.0))
    lm, _, _ = _lm(LMS[0], 50, "float32", LM_SEEDS[LMS[0]])
    enc_dev, _ = _enc(12, (3, 4, D), "float32")
    assert _raw(model, lm, enc_dev, [4, 1, 2], 4)[0] == L.EM_OK
    cases = [(dict(ws_delta=-1), L.EM_ERR_UNSUPPORTED), (dict(B=65), L.EM_ERR_UNSUPPORTED),
             (dict(beam=beam_limits()["beam"] + 1), L.EM_ERR_UNSUPPORTED), (dict(lw_edit=dict(vocab=51)), L.EM_ERR_BAD_ARG),
             (dict(lw_edit=dict(d=60)), L.EM_ERR_UNSUPPORTED), (dict(lw_edit=dict(out_w=None)), L.EM_ERR_BAD_ARG)]
    for kw, code in cases:
        args = dict(beam=4)
        args.update(kw)
        big = torch.zeros(65, 4, D, device="cuda") if "B" in kw else enc_dev
        rc, status, cnt, score, lens, tok = _raw(model, lm, big, [4, 1, 2], **args)
        assert rc == code, kw
        assert not status.any() and not cnt.any() and not lens.any() and not tok.any()
    rc, status, cnt, _, _, _ = _raw(model, None, enc_dev, [4, 1, 2], 4, step_lm=True)
    assert rc == L.EM_ERR_BAD_ARG and not status.any() and not cnt.any()
    # without an LM the entry is em_transducer_beam_search
    rc, status, cnt, score, lens, tok = _raw(model, None, enc_dev, [4, 1, 2], 4)
    from tests.test_gpu_transducer_beam import _raw as raw_plain

    rc0, status0, cnt0, score0, lens0, tok0 = raw_plain(model, enc_dev, [4, 1, 2], 4)
    assert rc == rc0 == 0 and torch.equal(status, status0) and torch.equal(cnt, cnt0)
    assert torch.equal(score.view(torch.int64), score0.view(torch.int64)) and torch.equal(tok, tok0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_contents_are_ignored(dtype):
    """The workspace pre-filled with 0x00, 0xFF (NaN) and 0x7F (huge) bytes: the same status rows, counts, scores, lengths
    and labels, bit for bit (the gru cell and the two-layer gru LM, beam 4, a ragged batch of 5)."""
    model, _, _, _ = _model(*CELLS[1], dtype, 11, out_bias=(0, 3.0))
    lm, _, _ = _lm(LMS[1], 300, dtype, LM_SEEDS[LMS[1]])
    olens = _ragged(5, 6)
    enc_dev, _ = _enc(12, (5, 6, D), dtype)
    ref = None
    for fill in (ZERO, ONES, BIG):
        rc, status, cnt, score, lens, tok = _raw(model, lm, enc_dev, olens, 4, fill=fill)
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


# ---------------------------------------------------------------------- 8. end to end
def test_speech2text_with_lm_train_config(tmp_path):
    """A tiny Speech2Text (the first cell's transducer, recipe weights seed 11 with the blank raised by 3, whose frames the
    default search leaves on any encoder output; config and weights written to tmp_path as tests/test_gpu_transducer.py
    `_speech2text` writes them) with lm_train_config / lm_file beside them (the peaked LM), beam 4, nbest 4, lm_weight 0.3: `batch_decode` equals BeamSearchTransducer(lm=...) called directly on the same
    encoder output, the LM is part of the search and changes a score, and the decode CLI with --lm_train_config writes the
    token_int rows of `__call__` on the same utterance at every rank of the n-best list.  (The CLI runs with batch_size 1
    and is held to the utterance decoded alone: this flat model's n-best entries lie close together, and an utterance
    padded into another batch has an encoder output that differs in its last bits, which can swap two neighbours.)"""
    import yaml

    from oracle.weights import token_list

    dtype, V = "float32", CELLS[0][4]
    lm, _, sd = _lm(LM_PEAKED, V, dtype, LM_PEAKED_SEED, LM_PEAK_SCALE)
    kind, nlayers, unit, nhid, tie = LM_PEAKED
    (tmp_path / "lm.yaml").write_text(yaml.safe_dump(dict(
        lm="seq_rnn", lm_conf=dict(unit=unit, nhid=nhid, nlayers=nlayers, rnn_type=kind, tie_weights=tie), token_list=token_list(V))))
    torch.save({"lm." + k: v for k, v in sd.items()}, tmp_path / "lm.pth")
    from espnet_amd.bin.asr_inference import Speech2Text

    _, _, cfg, asr_sd = _model(*CELLS[0], dtype, 11, out_bias=(0, 3.0))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({k: v for k, v in cfg.items() if k != "compute_dtype"}))
    torch.save(asr_sd, tmp_path / "model.pth")
    s2t = Speech2Text(str(tmp_path / "config.yaml"), str(tmp_path / "model.pth"), device="cuda", dtype=dtype, beam_size=4,
                      nbest=4, lm_train_config=str(tmp_path / "lm.yaml"), lm_file=str(tmp_path / "lm.pth"), lm_weight=0.3)
    bst = s2t.beam_search_transducer
    assert bst.lm is s2t.lm and bst.lm_weight == 0.3 and bst.lm.rnn_type == "LSTM" and bst.lm.act_dtype == torch.float32
    lens = [5000, 3000, 4000]
    speech = _waves(lens, 555)
    res = s2t.batch_decode(speech, lens)
    st = s2t.asr_model.encode_device(speech.cuda(), lens, isolate=True)
    direct = _bs(s2t.asr_model, 4, lm=lm, lm_weight=0.3, nbest=4).search_batch(st.enc_act, st.olens)
    plain = _bs(s2t.asr_model, 4, nbest=4).search_batch(st.enc_act, st.olens)
    for b in range(3):
        assert [(r[3].yseq, r[3].score) for r in res[b]] == [(h.yseq, h.score) for h in direct[b]]
        assert res[b][0][2] == [y for y in direct[b][0].yseq[1:] if y != 0]
    assert any(h.score != g.score for a, c in zip(direct, plain) for h, g in zip(a, c))
    from espnet_amd.bin.asr_inference import main
    from espnet_amd.fileio.sound_scp import write_wav_pcm16

    lines = []
    for b, n in enumerate(lens):
        write_wav_pcm16(tmp_path / f"u{b}.wav", speech[b, :n].numpy(), 16000)
        lines.append(f"u{b} {tmp_path / f'u{b}.wav'}")
    (tmp_path / "wav.scp").write_text("\n".join(lines) + "\n")
    main(["--output_dir", str(tmp_path / "out"), "--ngpu", "1", "--dtype", dtype, "--batch_size", "1",
          "--data_path_and_name_and_type", f"{tmp_path / 'wav.scp'},speech,sound", "--asr_train_config",
          str(tmp_path / "config.yaml"), "--asr_model_file", str(tmp_path / "model.pth"), "--beam_size", "4",
          "--lm_train_config", str(tmp_path / "lm.yaml"), "--lm_file", str(tmp_path / "lm.pth"), "--lm_weight", "0.3",
          "--nbest", "4"])
    alone = [s2t(speech[b, :n].numpy()) for b, n in enumerate(lens)]
    assert all(len(r) == 4 for r in alone)
    labels = 0
    for n in range(4):
        rows = dict(ln.split(maxsplit=1) if " " in ln.strip() else (ln.strip(), "")
                    for ln in (tmp_path / "out" / f"{n + 1}best_recog" / "token_int").read_text().splitlines())
        assert [rows[f"u{b}"].split() for b in range(len(lens))] == [[str(v) for v in r[n][2]] for r in alone], n
        labels += sum(len(r[n][2]) for r in alone)
    assert labels > 0
