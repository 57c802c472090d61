"""The resumable greedy transducer walk (`em_transducer_greedy_extend`, `BeamSearchTransducer.extend`) on the MI355X against
the float64 restatement tests/transducer_ref.py, teacher-forced on the device's own per-frame decisions.

Models, encoder rows and bounds are those of tests/test_gpu_transducer.py: the peaked model (weights seed 51, lin_out x
PEAK_SCALE) with the blank bias raised by BLANK_UP, at which the restatement emits a label on roughly half of the frames of
an N(0, 1) stream.  Stream 0 of every case is LABEL_ROW on every frame and stream 1 BLANK_ROW: 100 x an N(0, 1) row, which
saturates the joint network's tanh, so the first emits a label on every frame whatever its state (all F rounds of a tick
are needed) and the second none.  The row seeds and the encoder seeds were searched on the CPU with the restatement alone
(rows from 1000, encoder seeds from 200 in steps of two): the rows decide with margins above 8 x the logit bound in both
dtypes, and at most 3 of a case's 95 frames lie under the near-tie line (2 x E_LOGP_PEAKED) - the cap asserted is 10 %.
"""
import ctypes as C

import pytest
import torch

from tests import transducer_ref as R
from tests.test_gpu_transducer import D, DTYPES, E_LOGP_PEAKED, PEAK_SCALE, PEAKED, _enc, _model, _waves

pytestmark = pytest.mark.gpu

BLANK_UP = 24.0
CELLS = [PEAKED, ("gru", 2, 320, 320, 300)]
LABEL_ROW = {CELLS[0]: 1001, CELLS[1]: 1002}
BLANK_ROW = {CELLS[0]: 1002, CELLS[1]: 1010}
SHAPES = [(3, 5), (5, 16), (9, 16)]  # 15 rows; 80: over a 64-row tile's edge; 144: three tiles (V 300: two vocabulary slices)
ENC_SEED = {(CELLS[0], (3, 5)): 200, (CELLS[0], (5, 16)): 200, (CELLS[0], (9, 16)): 200,
            (CELLS[1], (3, 5)): 200, (CELLS[1], (5, 16)): 200, (CELLS[1], (9, 16)): 234}


def _search(cell, dtype, beam_size=1):
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

    model, p, _, _ = _model(*cell, dtype, 51, out_scale=PEAK_SCALE, out_bias=(0, BLANK_UP))
    return BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam_size), p


def _rows(cell, dtype, S, F, seed):
    """Encoder rows (S, F, D) on the device and in float64, streams 0 / 1 the saturating label / blank row."""
    enc_dev, enc64 = _enc(seed, (S, F, D), dtype)
    for s, row_seed in ((0, LABEL_ROW[cell]), (1, BLANK_ROW[cell])):
        row = (100.0 * torch.randn(D, generator=torch.Generator().manual_seed(row_seed))).to(enc_dev.dtype)
        enc_dev[s], enc64[s] = row.cuda(), row.to(torch.float64)
    return enc_dev, enc64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "-".join(map(str, c)))
def test_extend_teacher_forced(cell, shape, dtype):
    """One tick of S ragged streams (lengths include 0 and F) from fresh slots, with the trace: the restatement follows the
    device's decisions; where its float64 margin exceeds 2 x the logit bound the device took the float64 arg-max, every
    traced log-prob lies within the bound of the restatement's, the score within (frames + labels) x the bound of the sum
    over all frames (the stream score counts the blanks' terms too)."""
    S, F = shape
    bs, p = _search(cell, dtype)
    enc_dev, enc64 = _rows(cell, dtype, S, F, ENC_SEED[cell, shape])
    nf = [F, F] + [1 + (5 * i) % F for i in range(1, S - 2)] + [0]
    state = bs.stream_state(S + 1, "cuda")
    hyps, (tok, top, margin) = bs.extend(state, list(range(1, S + 1)), enc_dev, nf, trace=True)
    e = E_LOGP_PEAKED[dtype]
    frames = near = 0
    worst = 0.0
    for s in range(S):
        forced = tok[s, : nf[s]].tolist()
        r = R.greedy(p, enc64[s, : nf[s]], forced=forced)
        for t in range(nf[s]):
            frames += 1
            if r["margin"][t] > 2 * e:
                assert forced[t] == r["tok"][t], (s, t, forced[t], r["tok"][t], r["margin"][t])
            else:
                near += 1
            worst = max(worst, abs(float(top[s, t]) - r["lp_forced"][t]))
        labels = [t for t in forced if t != 0]
        assert hyps[s].yseq == [0] + labels == r["yseq"]
        assert abs(hyps[s].score - sum(r["lp_forced"])) <= (nf[s] + len(labels)) * e, (s, hyps[s].score, sum(r["lp_forced"]))
        assert (tok[s, nf[s]:] == -1).all() and (top[s, nf[s]:] == 0).all()  # no frame consumed: untouched
        assert state.frames[s + 1] == nf[s]
    print(f"\nextend {cell} {shape} {dtype}: {frames} frames, {near} near-ties, worst log-prob err {worst:.3e} (bound {e:g}), "
          f"rounds {bs.last_rounds}")
    assert worst <= e
    assert near <= 0.1 * frames
    assert len(hyps[0].yseq) == 1 + F and hyps[1].yseq == [0] and hyps[-1].yseq == [0] and hyps[-1].score == 0.0
    assert bs.last_rounds == dict(needed=F, enqueued=F)  # stream 0 commits one frame per round
    assert not state.slab[0].any()  # the slot no stream lives in


def _feed(bs, state, slots, enc_dev, plan):
    """Ticks after `plan`: per tick the new frames of every stream (None: the stream is not in the call)."""
    done = [0] * len(slots)
    for counts in plan:
        rows = [i for i, c in enumerate(counts) if c is not None]
        x = torch.zeros(len(rows), max(1, max(counts[i] for i in rows)), D, dtype=enc_dev.dtype, device="cuda")
        for j, i in enumerate(rows):
            x[j, : counts[i]] = enc_dev[i, done[i] : done[i] + counts[i]]
            done[i] += counts[i]
        bs.extend(state, [slots[i] for i in rows], x, [counts[i] for i in rows])
    return [(state.yseq[s], state.score[s]) for s in slots]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "-".join(map(str, c)))
def test_chunking_does_not_change_a_bit(cell, dtype):
    """The same frames of five ragged streams as one call, in chunks of one frame (every label falls on the last frame of
    its chunk: the advanced state crosses the seam) and as 3 frames + the rest with stream 1 paused in the first tick and
    stream 4 joining in the second, into a slot that served another stream and was reset; stream 0 emits on every frame,
    so its third label closes the first tick.  Same labels, same score bits, same slot bytes."""
    bs, _ = _search(cell, dtype)
    lens = [16, 16, 6, 11, 9]
    enc_dev, _ = _rows(cell, dtype, 5, 16, ENC_SEED[cell, (5, 16)])
    slots = [3, 0, 4, 1, 2]
    whole, ones, uneven = (bs.stream_state(5, "cuda") for _ in range(3))
    got_whole = _feed(bs, whole, slots, enc_dev, [lens])
    got_ones = _feed(bs, ones, slots, enc_dev, [[int(t < n) for n in lens] for t in range(16)])
    bs.extend(uneven, [2], enc_dev[:1, :7].contiguous(), [7])  # slot 2 serves another stream first
    assert len(uneven.yseq[2]) == 8
    uneven.reset([2])
    first = [3, 0, 3, 3, None]
    got_uneven = _feed(bs, uneven, slots, enc_dev, [first, [n - (c or 0) for n, c in zip(lens, first)]])
    assert sum(len(y) - 1 for y, _ in got_whole[2:]) > 0 and len(got_whole[0][0]) == 17 and got_whole[1][0] == [0]
    assert got_ones == got_whole and got_uneven == got_whole  # (label lists, and scores as Python floats: every bit)
    assert torch.equal(ones.slab, whole.slab) and torch.equal(uneven.slab, whole.slab)
    assert [whole.frames[s] for s in slots] == lens


def test_limits_raise_and_name_themselves():
    """A slot at label capacity, S or F above em_transducer_stream_limits, a workspace one byte short, beam_size > 1."""
    from espnet_amd import lib as L
    from espnet_amd.asr.transducer.beam_search_transducer import stream_limits

    cell, dtype = PEAKED, "bfloat16"
    bs, _ = _search(cell, dtype)
    lim = stream_limits()
    F = lim["frames"]
    enc_dev, _ = _rows(cell, dtype, 2, F, 200)
    state = bs.stream_state(3, "cuda")
    for _ in range(lim["labels"] // F):  # stream 0 emits on every frame: the list fills up exactly
        hyps = bs.extend(state, [1], enc_dev[:1], [F])
    assert len(hyps[0].yseq) == 1 + lim["labels"]
    with pytest.raises(RuntimeError, match="label capacity"):
        bs.extend(state, [1], enc_dev[:1], [F])
    assert len(state.yseq[1]) == 1 + lim["labels"] and state.frames[1] == lim["labels"]  # stopped in front of the frame
    assert not state.slab[0].any() and not state.slab[2].any()  # nothing written past the slot, on either side
    with pytest.raises(RuntimeError, match="label capacity"):  # and it stays stopped
        bs.extend(state, [1], enc_dev[:1], [F])
    assert state.frames[1] == lim["labels"]
    with pytest.raises(NotImplementedError, match="frames="):
        bs.extend(state, [0], torch.zeros(1, F + 1, D, dtype=enc_dev.dtype, device="cuda"), [1])
    with pytest.raises(NotImplementedError, match="streams="):
        bs.extend(state, list(range(lim["streams"] + 1)),
                  torch.zeros(lim["streams"] + 1, 1, D, dtype=enc_dev.dtype, device="cuda"), [1] * (lim["streams"] + 1))
    with pytest.raises(NotImplementedError, match="beam_size"):
        _search(cell, dtype, beam_size=2)[0].extend(state, [0], enc_dev[:1], [F])
    lib, dec = L.load(), bs.decoder
    w, keep = dec.weights("cuda")
    need = int(lib.em_transducer_greedy_extend_workspace_bytes(dec.em_dtype, C.byref(w), 1, 4))
    assert need > 0 and lib.em_transducer_greedy_extend_workspace_bytes(dec.em_dtype, C.byref(w), 1, F + 1) == 0
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(4 * w.jp, device="cuda")
    f64 = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.em_transducer_greedy_extend(dec.em_dtype, C.byref(w), L.ptr(state.slab), 3, L.ptr(i32), L.ptr(f32), L.ptr(i32[8:]),
                                         1, 4, L.ptr(f64), L.ptr(i32[16:]), L.ptr(i32[32:]), None, None, None, L.ptr(ws),
                                         need - 1, L.current_stream_ptr())
    assert rc == L.EM_ERR_WORKSPACE
    torch.cuda.synchronize()


def _streaming(tmp_path, dtype, **kw):
    """A small contextual-block Conformer + transducer model without a CTC head (recipe weights seed 31, the joint
    network peaked and the blank raised as above), built as test_gpu_ctc_tsync_stream.py builds its streaming model."""
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import recipe_state_dict, token_list
    from tests.helpers import load_stream_golden

    conf = dict(load_stream_golden("stream_small_6s")["conf"], num_blocks=2)
    rnn, layers, H, J, V = PEAKED
    cfg = dict(token_list=token_list(V), frontend="default", frontend_conf=dict(n_fft=512, hop_length=160, win_length=400),
               normalize="utterance_mvn", normalize_conf={}, encoder="contextual_block_conformer", encoder_conf=conf,
               decoder="transducer", decoder_conf=dict(rnn_type=rnn, num_layers=layers, hidden_size=H),
               joint_net_conf=dict(joint_space_size=J), model_conf=dict(ctc_weight=0.0))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, device="cuda", dtype=dtype, use_hipgraph=False, **kw)
    sd = s2t.asr_model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 31)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    new["decoder.embed.weight"][0] = 0.0
    new["joint_network.lin_out.weight"] *= PEAK_SCALE
    new["joint_network.lin_out.bias"][0] += BLANK_UP
    s2t.asr_model.load_state_dict(new, strict=True)
    return s2t


@pytest.mark.parametrize("dtype", DTYPES)
def test_speech2text_streaming_decodes_a_transducer(tmp_path, dtype):
    """`__call__` chunk by chunk: growing partials, each extending the last; the final result is `extend` on the same
    encoder frames (fed 16 at a time: the chunking does not matter).  `batch_call` and `StreamPool.tick` give every
    stream what it gets alone.  The options the walk does not serve are refused by name."""
    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming

    s2t = _streaming(tmp_path, dtype, beam_size=1)
    assert s2t.asr_model.ctc is None and s2t.transducer is not None
    N, CH = 40000, 8000
    waves = _waves([N] * 3, 70)
    encs, encode = [], s2t._encode_chunk
    s2t._encode_chunk = lambda feats, fin: (encs.append(encode(feats, fin).clone()), encs[-1])[1]
    alone = []
    for b in range(3):
        last = []
        for pos in range(0, N, CH):
            res = s2t(waves[b, pos : pos + CH], is_final=(pos + CH == N))
            assert res[0][2][: len(last)] == last and res[0][3].yseq[0] == 0  # a partial extends the one before
            last = res[0][2]
        alone.append(last)
        if b == 0:
            x = torch.cat(encs).unsqueeze(0)
            bs, st = s2t.transducer, s2t.transducer.stream_state(1, "cuda")
            for t in range(0, x.size(1), 16):
                want = bs.extend(st, [0], x[:, t : t + 16], [min(16, x.size(1) - t)])[0]
            assert res[0][3].yseq == want.yseq and res[0][3].score == want.score and x.size(1) > 20
    assert all(len(a) > 0 for a in alone) and len(set(map(tuple, alone))) > 1
    s2t._encode_chunk = encode
    for pos in range(0, N, CH):
        got = s2t.batch_call(waves[:, pos : pos + CH], is_final=(pos + CH == N))
    assert got == alone
    pool, got = s2t.stream_pool(), {}
    for k in range(N // CH + 1):  # stream "b" joins a tick after stream "a"
        chunks = {sid: (waves[i, (k - i) * CH : (k - i + 1) * CH], k - i == N // CH - 1)
                  for i, sid in enumerate("ab") if 0 <= k - i < N // CH}
        got.update(pool.tick(chunks))
    assert [got["a"], got["b"]] == alone[:2] and pool.transducer_state.n_free == pool.transducer_state.n_slots
    kw = dict(asr_train_config=str(tmp_path / "config.yaml"), device="cuda", dtype=dtype)
    for match, bad in (("beam_size=4", dict(beam_size=4)), ("search='online'", dict(search="online", beam_size=1)),
                       ("search='offline'", dict(search="offline")), ("search='tsync'", dict(search="tsync", ctc_weight=1.0)),
                       ("lm_train_config", dict(beam_size=1, lm_train_config=str(tmp_path / "lm.yaml")))):
        with pytest.raises(NotImplementedError, match=match):
            Speech2TextStreaming(**kw, **bad)
