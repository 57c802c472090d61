"""Transducer (RNN-T) decoding on the MI355X against the float64 restatement tests/transducer_ref.py.

Weights: oracle.weights.recipe_state_dict with the seed each test names, `joint_network.lin_out.bias[0]` (blank) raised by
BLANK_BIAS so that blank and label frames both occur; encoder outputs for the primitive / walk tests are N(0, 1) rows
from torch.Generator seeds named likewise, rounded to the compute dtype.  The restatement is fed the SAME inputs: the
matrices and encoder rows as the compute dtype holds them (bf16 mode: rounded to bf16), in float64 arithmetic.

Bounds (the convention of test_gpu_search_steps.py: 4 x the largest error seen on the MI355X over the cells of
`test_primitives`; seen values in brackets):
    dec_out  f32 7.0e-7 [1.74e-7]   bf16 6.8e-3 [1.70e-3]
    logp     f32 5.2e-6 [1.30e-6]   bf16 7.6e-3 [1.90e-3]
The same for the peaked model of the end-to-end and beam-search tests (lin_out x 40, which scales the logits' error
with it), over the cells of `test_primitives_peaked`:
    logp     f32 3.2e-5 [7.97e-6]   bf16 3.1e-1 [7.55e-2]
The printed output of the run that the seen values come from is profiles/r09a_transducer_pytest_gpu.txt.
A logit difference equals the difference of two log-probabilities of one row, so a top-1 / top-2 margin is known to
2 x the logp bound: where the float64 margin exceeds that, the device must take the float64 arg-max.

Recipe weights make a nearly flat softmax (logit spread ~ 0.2), so in bf16 roughly one frame in ten of an arbitrary seed
is a near-tie under that line.  The walk cells therefore carry seeds for which the restatement ALONE - on the CPU, before
any GPU run - has no frame under the line in either dtype and emits both labels and blanks (searched in steps of two
from 100; the 33-utterance cell with the blank bias at 1.0, which a flat softmax needs for blanks to win often).
"""
import numpy as np
import pytest
import torch

from tests import transducer_ref as R

pytestmark = pytest.mark.gpu

D = 64
BLANK_BIAS = 0.5
E_DEC = {"float32": 7.0e-7, "bfloat16": 6.8e-3}
E_LOGP = {"float32": 5.2e-6, "bfloat16": 7.6e-3}
E_LOGP_PEAKED = {"float32": 3.2e-5, "bfloat16": 3.1e-1}
NEAR_TIE_CAP = 0.01
DTYPES = ["float32", "bfloat16"]
_cache = {}


def _config(rnn_type, num_layers, H, J, V):
    from oracle.weights import token_list

    return dict(token_list=token_list(V), frontend="default", frontend_conf=dict(n_fft=512, hop_length=160, win_length=400),
                normalize="utterance_mvn", normalize_conf={}, encoder="conformer",
                encoder_conf=dict(output_size=D, attention_heads=1, linear_units=128, num_blocks=1, macaron_style=True,
                                  cnn_module_kernel=15),
                decoder="transducer", decoder_conf=dict(rnn_type=rnn_type, num_layers=num_layers, hidden_size=H),
                joint_net_conf=dict(joint_space_size=J), model_conf=dict(ctc_weight=0.3))


def _model(rnn_type, num_layers, H, J, V, dtype, seed, out_scale=1.0, out_bias=None):
    """(model on the GPU, restatement parameters as the compute dtype holds them); built once per argument set."""
    key = (rnn_type, num_layers, H, J, V, dtype, seed, out_scale, None if out_bias is None else tuple(out_bias))
    if key not in _cache:
        from espnet_amd.tasks.asr import ASRTask
        from oracle.weights import recipe_state_dict

        cfg = _config(rnn_type, num_layers, H, J, V)
        cfg["compute_dtype"] = dtype
        model = ASRTask.build_model(cfg)
        sd = model.state_dict()
        new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed)
        new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
        new["decoder.embed.weight"][0] = 0.0  # the padding row, as torch.nn.Embedding(padding_idx=0) initialises it
        new["joint_network.lin_out.weight"] *= out_scale
        new["joint_network.lin_out.bias"][0] += BLANK_BIAS
        if out_bias is not None:
            new["joint_network.lin_out.bias"][out_bias[0]] += out_bias[1]
        model.load_state_dict(new, strict=True)
        model.cuda().eval()
        p = R.Params(new, rnn_type, round_to=torch.bfloat16 if dtype == "bfloat16" else None)
        _cache[key] = (model, p, cfg, new)
    return _cache[key]


def _enc(seed, shape, dtype):
    g = torch.Generator().manual_seed(seed)
    act = torch.bfloat16 if dtype == "bfloat16" else torch.float32
    e = torch.randn(shape, generator=g).to(act)
    return e.cuda(), e.to(torch.float64)


def _ragged(B, T):
    """Lengths that include 1 and T."""
    return [T] + [1 + (5 * b) % T for b in range(1, B - 1)] + ([1] if B > 1 else [])


PRIM_CELLS = [("lstm", 1, 64, 64, 50, 3), ("gru", 2, 320, 320, 300, 33), ("lstm", 2, 320, 64, 1027, 70),
              ("gru", 1, 64, 320, 1027, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", PRIM_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_primitives(cell, dtype):
    """em_transducer_dec_step (two steps, the second masked) and em_transducer_joint_logp against the restatement on the
    same inputs.  Weights seed 11, encoder rows seed 12, labels / mask seed 13.  n = 70 goes through two row chunks."""
    rnn, layers, H, J, V, n = cell
    model, p, _, _ = _model(rnn, layers, H, J, V, dtype, 11)
    dec, jn = model.decoder, model.joint_network
    g = torch.Generator().manual_seed(13)
    tok1 = torch.randint(0, V, (n,), generator=g)
    tok2 = torch.randint(1, V, (n,), generator=g)
    mask = (torch.rand(n, generator=g) < 0.6).to(torch.int32)
    mask[0], mask[-1] = 1, 0
    enc_dev, enc64 = _enc(12, (n, D), dtype)
    o1, q1, s1 = dec.step_device(tok1.to(torch.int32).cuda(), dec.init_state(n, "cuda"))
    o1c, q1c = o1.clone(), q1.clone()
    o2, q2, s2 = dec.step_device(tok2.to(torch.int32).cuda(), s1, mask=mask.cuda(), out=(o1, q1))
    enc_proj = jn.enc_proj_device(enc_dev)
    logp = jn.logp_device(dec, enc_proj, q2).cpu().to(torch.float64)
    torch.cuda.synchronize()
    live = mask.bool()
    for a, b in ((s2[0], s1[0]), (s2[1], s1[1])):  # masked rows: state bit for bit (h and the master state / c)
        assert torch.equal(a[:, ~live.cuda()], b[:, ~live.cuda()])
    assert torch.equal(o2[~live.cuda()], o1c[~live.cuda()]) and torch.equal(q2[~live.cuda()], q1c[~live.cuda()])
    assert float(s2[0][:, :, H:].abs().max() if dec.dpad > H else 0.0) == 0.0  # pad channels stay zero
    e_dec = e_lp = 0.0
    for r in range(n):
        out, st = R.dec_step(p, int(tok1[r]), p.init_state())
        e_dec = max(e_dec, float((o1c[r].cpu().double() - out).abs().max()))
        if live[r]:
            out, st = R.dec_step(p, int(tok2[r]), st)
            e_dec = max(e_dec, float((o2[r].cpu().double() - out).abs().max()))
        want = R.log_softmax(R.joint_logits(p, enc64[r], out))
        e_lp = max(e_lp, float((logp[r] - want).abs().max()))
    print(f"\nprimitives {cell} {dtype}: dec_out err {e_dec:.3e}  logp err {e_lp:.3e}")
    assert e_dec <= E_DEC[dtype] and e_lp <= E_LOGP[dtype]


WALK_CELLS = [("lstm", 1, 64, 64, 50, 1, 12), ("gru", 1, 320, 64, 300, 3, 8), ("lstm", 2, 64, 320, 1027, 33, 2)]
# weights seed (encoder rows: seed + 1) and extra blank bias of each walk cell, see the module docstring
WALK_SEEDS = {WALK_CELLS[0]: (104, 0.0), WALK_CELLS[1]: (106, 0.0), WALK_CELLS[2]: (220, 0.5)}


def _walk(cell, dtype, seed=None, **kw):
    """The fused walk with its trace and the teacher-forced restatement of every utterance (shared by the tests)."""
    if seed is None:
        seed, extra = WALK_SEEDS[cell]
        if extra:
            kw = dict(kw, out_bias=(0, extra))
    key = ("walk", cell, dtype, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

        rnn, layers, H, J, V, B, T = cell
        model, p, _, _ = _model(rnn, layers, H, J, V, dtype, seed, **kw)
        bs = BeamSearchTransducer(model.decoder, model.joint_network, beam_size=1)
        olens = _ragged(B, T)
        enc_dev, enc64 = _enc(seed + 1, (B, T, D), dtype)
        ol = torch.tensor(olens, dtype=torch.int32).cuda()
        tokens, ylens, score, tr = bs.greedy_device(enc_dev, ol, trace=True)
        dev = dict(tokens=tokens.cpu(), ylens=ylens.cpu(), score=score.cpu(), tok=tr[0].cpu(), top=tr[1].cpu(), margin=tr[2].cpu())
        ref = [R.greedy(p, enc64[b, : olens[b]], forced=dev["tok"][b, : olens[b]].tolist()) for b in range(B)]
        _cache[key] = (dev, ref, olens, (model, p, bs, enc_dev, enc64, ol))
    return _cache[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", WALK_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_greedy_walk_teacher_forced(cell, dtype):
    """em_transducer_greedy frame by frame: the restatement follows the device's labels (seeds: WALK_SEEDS); where its float64 margin exceeds 2 x the logp bound the device took the float64 arg-max."""
    rnn, layers, H, J, V, B, T = cell
    dev, ref, olens, _ = _walk(cell, dtype)
    thr = 2 * E_LOGP[dtype]
    frames = near = labels = blanks = 0
    for b in range(B):
        r = ref[b]
        for t in range(olens[b]):
            frames += 1
            d_tok = int(dev["tok"][b, t])
            labels += d_tok != 0
            blanks += d_tok == 0
            if r["margin"][t] > thr:
                assert d_tok == r["tok"][t], (b, t, d_tok, r["tok"][t], r["margin"][t])
            else:
                near += 1
            assert abs(float(dev["top"][b, t]) - r["lp_forced"][t]) <= E_LOGP[dtype], (b, t)
        n = int(dev["ylens"][b])
        assert dev["tokens"][b, :n].tolist() == r["yseq"][1:] and n == len(r["yseq"]) - 1
        assert abs(float(dev["score"][b]) - r["score"]) <= max(n, 1) * E_LOGP[dtype]
        assert (dev["tok"][b, olens[b]:] == -1).all() and (dev["top"][b, olens[b]:] == 0).all()  # frames past the end: untouched
        assert (dev["tokens"][b, n:] == -1).all()
    print(f"\nwalk {cell} {dtype}: {frames} frames, {labels} labels, {blanks} blanks, {near} near-ties (margin <= {thr:g})")
    assert labels > 0 and (blanks > 0 or frames < 4)
    assert near <= NEAR_TIE_CAP * frames


@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_emit_always_and_never(dtype):
    """lin_out.bias decides: blank lowered by 50 - a label on every frame (ylen == olens, at most one per frame); blank
    raised by 50 - nothing is emitted.  B = 33 with ragged lengths, one of them 1 (weights seed 31, encoder seed 32)."""
    cell = ("lstm", 1, 64, 64, 300, 33, 9)
    dev, ref, olens, _ = _walk(cell, dtype, seed=31, out_bias=(0, -50.0))
    assert 1 in olens and 9 in olens
    assert dev["ylens"].tolist() == olens
    for b in range(33):
        assert (dev["tokens"][b, : olens[b]] > 0).all() and (dev["tokens"][b, olens[b]:] == -1).all()
    dev, ref, olens, _ = _walk(cell, dtype, seed=31, out_bias=(0, 50.0))
    assert dev["ylens"].tolist() == [0] * 33 and (dev["tokens"] == -1).all() and (dev["score"] == 0).all()
    assert all((dev["tok"][b, : olens[b]] == 0).all() for b in range(33))


def test_exact_ties_take_the_lowest_id():
    """All-zero lin_out weights and equal biases: every logit of a frame is the same number, in both the tile partials
    and their reduction; the arg-max must be label 0 (blank) - and label 1 when only blank is lowered."""
    cell = ("lstm", 1, 64, 64, 1027, 3, 4)
    for shift, want in ((0.0, 0), (-1.0, 1)):
        model, p, _, sd = _model(*cell[:5], "float32", 41)
        sd = {k: v.clone() for k, v in sd.items()}
        sd["joint_network.lin_out.weight"].zero_()
        sd["joint_network.lin_out.bias"].fill_(0.25)
        sd["joint_network.lin_out.bias"][0] += shift
        model.load_state_dict(sd, strict=True)
        from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

        bs = BeamSearchTransducer(model.decoder, model.joint_network, beam_size=1)
        enc_dev, _ = _enc(42, (3, 4, D), "float32")
        _, _, _, tr = bs.greedy_device(enc_dev, torch.tensor([4, 2, 1], dtype=torch.int32).cuda(), trace=True)
        tok, margin = tr[0].cpu(), tr[2].cpu()
        assert (tok[0] == want).all() and (tok[1, :2] == want).all() and int(tok[2, 0]) == want
        assert float(margin.abs().max()) == 0.0
    for k in [k for k in _cache if 41 in k]:  # (the cached model of this cell carries the test's weights)
        del _cache[k]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", WALK_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_fused_walk_equals_host_driven_loop(cell, dtype):
    """The per-frame loop over em_transducer_dec_step / em_transducer_joint_logp (one read-back per frame) on the cells
    of the walk test: the same labels as em_transducer_greedy wherever the float64 margin is above the near-tie line."""
    rnn, layers, H, J, V, B, T = cell
    dev, ref, olens, (model, p, bs, enc_dev, enc64, ol) = _walk(cell, dtype)
    dec, jn = model.decoder, model.joint_network
    enc_proj = jn.enc_proj_device(enc_dev)
    tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    o, q, st = dec.step_device(tok, dec.init_state(B, "cuda"))
    thr = 2 * E_LOGP[dtype]
    for t in range(T):
        logp = jn.logp_device(dec, enc_proj[:, t].contiguous(), q)
        pred = torch.argmax(logp, 1).cpu()  # the read-back of this frame
        for b in range(B):
            if t < olens[b] and ref[b]["margin"][t] > thr:
                assert int(pred[b]) == int(dev["tok"][b, t]), (b, t)
        # follow the fused walk's own decisions, so that both sides stay on one path through near-ties as well
        forced = torch.tensor([int(dev["tok"][b, t]) if t < olens[b] else 0 for b in range(B)], dtype=torch.int32)
        mask = (forced != 0).to(torch.int32).cuda()
        o, q, st = dec.step_device(forced.cuda(), st, mask=mask, out=(o, q))


# ---------------------------------------------------------------------- through the public interface, peaked
PEAKED = ("lstm", 1, 64, 64, 50)
PEAK_SCALE = 40.0  # lin_out scaled: margins of several units, above twice E_LOGP_PEAKED
# first waveform seed of the end-to-end test's three utterances: of the sets 0, 3, 6 .. the one whose restatement - on the
# CPU reference encoder's output, before any GPU run - has the widest smallest margin (1.79)
PEAKED_WAVES = 555


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blank_up", [0.0, 32.0])
def test_primitives_peaked(blank_up, dtype):
    """em_transducer_joint_logp on the peaked model of the tests below (weights seed 51, lin_out x 40; with the blank
    raised by 32 it is the beam-search test's) against the restatement on the same inputs: 33 rows, encoder rows seed
    62, labels seed 63.  The error of a whole log-softmax row, which E_LOGP_PEAKED bounds."""
    n, V = 33, PEAKED[4]
    model, p, _, _ = _model(*PEAKED, dtype, 51, out_scale=PEAK_SCALE, out_bias=(0, blank_up) if blank_up else None)
    dec, jn = model.decoder, model.joint_network
    tok = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(63))
    enc_dev, enc64 = _enc(62, (n, D), dtype)
    _, q, _ = dec.step_device(tok.to(torch.int32).cuda(), dec.init_state(n, "cuda"))
    logp = jn.logp_device(dec, jn.enc_proj_device(enc_dev), q).cpu().to(torch.float64)
    err = 0.0
    for r in range(n):
        out, _ = R.dec_step(p, int(tok[r]), p.init_state())
        err = max(err, float((logp[r] - R.log_softmax(R.joint_logits(p, enc64[r], out))).abs().max()))
    print(f"\nprimitives peaked blank+{blank_up:g} {dtype}: logp err {err:.3e}")
    assert err <= E_LOGP_PEAKED[dtype]


def _speech2text(tmp_path, dtype, beam_size=1, **kw):
    import yaml

    from espnet_amd.bin.asr_inference import Speech2Text

    model, p, cfg, sd = _model(*PEAKED, dtype, 51, out_scale=PEAK_SCALE)
    cfg = {k: v for k, v in cfg.items() if k != "compute_dtype"}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / "model.pth")
    return Speech2Text(str(tmp_path / "config.yaml"), str(tmp_path / "model.pth"), device="cuda", dtype=dtype,
                       beam_size=beam_size, **kw), p


def _waves(lens, first=60):
    from oracle.weights import synth_waveform

    speech = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        speech[b, :n] = synth_waveform(first + b, n)
    return torch.round(speech * 32768.0).clamp(-32768, 32767) / 32768.0  # (exactly what a 16-bit wav file holds)


@pytest.mark.parametrize("dtype", DTYPES)
def test_peaked_end_to_end_greedy(tmp_path, dtype):
    """Speech2Text on a tiny Conformer transducer (weights seed 51, lin_out x 40, waveforms PEAKED_WAVES ..): batch_decode,
    __call__ and batch_decode_async give the restatement's greedy labels on the device's own encoder output; row b of
    the batch is the utterance decoded alone."""
    s2t, p = _speech2text(tmp_path, dtype)
    lens = [5000, 3000, 4000]
    speech = _waves(lens, PEAKED_WAVES)
    res = s2t.batch_decode(speech, lens)
    st = s2t.asr_model.encode_device(speech.cuda(), lens, isolate=True)
    enc64 = st.enc_act.cpu().to(torch.float64)
    for b, n in enumerate(lens):
        want = R.greedy(p, enc64[b, : st.olens[b]])
        # peaked indeed: every frame of the restatement lies above twice the peaked model's logp bound
        assert min(want["margin"]) > 2 * E_LOGP_PEAKED[dtype]
        text, token, token_int, hyp = res[b][0]
        assert hyp.yseq == want["yseq"] and hyp.yseq[0] == 0
        assert token_int == [y for y in want["yseq"][1:] if y != 0] and len(token) == len(token_int)
        print(f"\nend to end {dtype} utt {b}: {len(token_int)} labels, score err {abs(hyp.score - want['score']):.3e}")
        assert abs(hyp.score - want["score"]) <= max(len(token_int), 1) * E_LOGP_PEAKED[dtype]
        alone = s2t(speech[b, :n].numpy())
        assert alone[0][2] == token_int
    again = s2t.batch_decode_async(speech, lens).result()
    assert [r[0][2] for r in again] == [r[0][2] for r in res]
    # the decode CLI on the same utterances as 16-bit wav files
    from espnet_amd.bin.asr_inference import main
    from espnet_amd.fileio.sound_scp import write_wav_pcm16

    lines = []
    for b, n in enumerate(lens):
        write_wav_pcm16(tmp_path / f"u{b}.wav", speech[b, :n].numpy(), 16000)
        lines.append(f"u{b} {tmp_path / f'u{b}.wav'}")
    (tmp_path / "wav.scp").write_text("\n".join(lines) + "\n")
    main(["--output_dir", str(tmp_path / "out"), "--ngpu", "1", "--dtype", dtype, "--batch_size", "2",
          "--data_path_and_name_and_type", f"{tmp_path / 'wav.scp'},speech,sound", "--asr_train_config",
          str(tmp_path / "config.yaml"), "--asr_model_file", str(tmp_path / "model.pth"), "--beam_size", "1",
          "--transducer_conf", "{score_norm: true}"])
    rows = dict(ln.split(maxsplit=1) if " " in ln.strip() else (ln.strip(), "")
                for ln in (tmp_path / "out" / "1best_recog" / "token_int").read_text().splitlines())
    assert [rows[f"u{b}"].split() for b in range(len(lens))] == [[str(v) for v in r[0][2]] for r in res]


def test_speech2text_refusals(tmp_path):
    import yaml

    from espnet_amd.bin.asr_inference import Speech2Text

    _speech2text(tmp_path, "float32")
    kw = dict(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"), device="cuda")
    with pytest.raises(NotImplementedError, match="lm_train_config"):
        Speech2Text(lm_train_config=str(tmp_path / "lm.yaml"), **kw)
    with pytest.raises(NotImplementedError, match="ngram_file"):
        Speech2Text(ngram_file=str(tmp_path / "x.arpa"), **kw)
    with pytest.raises(NotImplementedError, match="alsd"):
        Speech2Text(transducer_conf=dict(search_type="alsd"), beam_size=2, **kw)
    with pytest.raises(NotImplementedError, match="streaming"):
        Speech2Text(streaming=True, **kw)
    assert Speech2Text(ctc_greedy=True, **kw)(_waves([8000])[0].numpy())[0][3] is not None  # the CTC head still decodes
    cfg = yaml.safe_load((tmp_path / "config.yaml").read_text())
    cfg.update(decoder="transformer", decoder_conf=dict(attention_heads=1, linear_units=64, num_blocks=1))
    cfg.pop("joint_net_conf")
    (tmp_path / "att.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="transducer_conf"):
        Speech2Text(str(tmp_path / "att.yaml"), None, device="cuda", transducer_conf={})


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_beam_search(tmp_path, dtype):
    """Beam 2 and 4 on the peaked model: the n-best label sequences of the restatement, scores within the peaked model's
    logp bound x the number of terms of a score (one per label and one blank per frame)."""
    # (blank raised by 32 on top: in a peaked model without it every context prefers some label, and the default search -
    # the reference's as much as the restatement's - keeps extending within one frame; checked on the CPU beforehand)
    model, p, _, _ = _model(*PEAKED, dtype, 51, out_scale=PEAK_SCALE, out_bias=(0, 32.0))
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

    enc_dev, enc64 = _enc(61, (7, D), dtype)
    for beam in (2, 4):
        bs = BeamSearchTransducer(model.decoder, model.joint_network, beam_size=beam, nbest=beam)
        got = bs(enc_dev)
        want = R.beam_search(p, enc64, beam, nbest=beam)
        assert [h.yseq for h in got] == [y for _, y in want]
        for h, (s, y) in zip(got, want):
            print(f"\nbeam {beam} {dtype} {y}: score err {abs(h.score - s):.3e}")
            assert abs(h.score - s) <= (len(y) - 1 + 7) * E_LOGP_PEAKED[dtype]


def test_beam_search_gives_up_on_a_frame_it_cannot_leave(monkeypatch):
    """The peaked model without the raised blank: every context prefers some label, so the default search - the
    reference's too - extends within frame 0 for ever.  Here it raises, naming the utterance and the frame (blank lowered
    by 100 on top; limit lowered to 20 expansions for the test)."""
    from espnet_amd.asr.transducer import beam_search_transducer as B

    model, p, _, _ = _model(*PEAKED, "float32", 51, out_scale=PEAK_SCALE, out_bias=(0, -100.0))
    monkeypatch.setattr(B, "MAX_EXPANSIONS_PER_FRAME", 20)
    enc_dev, _ = _enc(61, (1, 3, D), "float32")
    bs = B.BeamSearchTransducer(model.decoder, model.joint_network, beam_size=2)
    with pytest.raises(RuntimeError, match="utterance 0, frame 0 not left after 20 expansions"):
        bs.search_batch(enc_dev, [3])


def test_beam_search_leaves_the_greedy_path():
    """A cell (f32, recipe weights seed 71 unscaled, encoder rows seed 72) where the restatement's beam-4 winner is not
    its greedy sequence: the device's default beam search finds the same winner."""
    model, p, _, _ = _model("lstm", 1, 64, 64, 50, "float32", 71)
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer

    enc_dev, enc64 = _enc(72, (6, D), "float32")
    greedy = R.greedy(p, enc64)["yseq"]
    (s, y), = R.beam_search(p, enc64, 4, nbest=1)
    assert y != greedy
    got = BeamSearchTransducer(model.decoder, model.joint_network, beam_size=4)(enc_dev)[0]
    assert got.yseq == y and abs(got.score - s) <= (len(y) + 6) * E_LOGP["float32"]
