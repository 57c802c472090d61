"""GPU parity of the Transformer encoder (encoder: transformer) through the C-ABI: the attention kernels
(em_abs_attention_bf16 / em_abs_attention, csrc/abs_attn.hip) against torch, em_transformer_encode against the f32 CPU
restatement (tests/transformer_ref.py), the 512-wide row-block ReLU FFN, and Speech2Text / the decode CLI end to end."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import conformer as oc  # noqa: E402
from oracle.weights import recipe_tensor  # noqa: E402
from tests import transformer_ref as tr  # noqa: E402
from tests.helpers import golden_state_dict, load_golden  # noqa: E402


# ------------------------------------------------------------------------------------------- 1. the attention kernels
def _torch_attention(q, k, v, klens):
    """q / k / v (B, H, T, 64) f32 -> ctx (B, T, H * 64): softmax(q k^T / 8) over keys j < klens[b]."""
    B, H, T, _ = q.shape
    s = torch.matmul(q, k.transpose(-2, -1)) / 8.0
    valid = torch.arange(T, device=q.device)[None, :] < klens[:, None]
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(s, -1), v).transpose(1, 2).reshape(B, T, H * 64)


@pytest.mark.parametrize("T", [1, 17, 249, 256, 257, 600, 1100, 3000])
@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_abs_attention_matches_torch(T, H, prec):
    from espnet_amd import lib as L

    lib = L.load()
    g = torch.Generator().manual_seed(T * 10 + H)
    B = 3
    klens = torch.tensor([T, max(1, T // 2 + 1), 1], dtype=torch.int32)
    q, k, v = (torch.randn(B, H, T, 64, generator=g) for _ in range(3))
    k = k * 2.0  # (peakier softmax)
    dev = torch.device("cuda")
    kl = klens.to(dev)
    st = L.current_stream_ptr()
    dt = torch.float32 if prec == "f32" else torch.bfloat16
    qd, kd, vd = (t.to(dt).to(dev) for t in (q, k, v))
    want = _torch_attention(qd.float(), kd.float(), vd.float(), kl)
    # row layout q | k | v [B*T][3d]
    qkv = torch.cat([t.transpose(1, 2).reshape(B, T, H * 64) for t in (qd, kd, vd)], -1).contiguous()
    ctx = torch.full((B, T, H * 64), float("nan"), dtype=dt, device=dev)
    L.check(lib.em_abs_attention(L.DTYPES[{"f32": "float32", "bf16": "bfloat16"}[prec]], L.ptr(qkv), L.ptr(kl), B, T, H,
                                 64, L.ptr(ctx), st), "em_abs_attention")
    outs = [("rows", ctx)]
    if prec == "bf16":
        # per-head operands as EM_EPI_QK_HEADS / EM_EPI_VT_HEADS write them; the padding frames hold NaN: never read as keys
        Tpad = (T + 255) // 256 * 256
        qh = torch.full((B, H, Tpad, 64), float("nan"), dtype=dt, device=dev)
        kh, vt = qh.clone(), torch.full((B, H, 64, Tpad), float("nan"), dtype=dt, device=dev)
        qh[:, :, :T], kh[:, :, :T], vt[:, :, :, :T] = qd, kd, vd.transpose(-2, -1)
        c2 = torch.full((B, T, H * 64), float("nan"), dtype=dt, device=dev)
        L.check(lib.em_abs_attention_bf16(L.ptr(qh), L.ptr(kh), L.ptr(vt), L.ptr(kl), B, T, Tpad, H, L.ptr(c2), st),
                "em_abs_attention_bf16")
        outs.append(("mfma", c2))
    torch.cuda.synchronize()
    for name, got in outs:
        err = (got.float() - want).abs().max().item()
        tol = 2e-5 if prec == "f32" else 3e-2  # bf16: the probabilities enter P . V as bf16, the output is stored in bf16
        assert err < tol, (name, err)


# ------------------------------------------------------------------------------------------- 2. encoder parity
def _cfg(d, heads, ff, blocks, layer="conv2d", dtype="float32", vocab=40):
    return dict(token_list=["<blank>", "<unk>"] + [f"t{i}" for i in range(vocab - 3)] + ["<sos/eos>"], frontend="default",
                frontend_conf=dict(n_fft=512, win_length=400, hop_length=160), normalize="utterance_mvn", normalize_conf={},
                encoder="transformer",
                encoder_conf=dict(output_size=d, attention_heads=heads, linear_units=ff, num_blocks=blocks, input_layer=layer,
                                  normalize_before=True, concat_after=False, positionwise_layer_type="linear",
                                  dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.0),
                decoder="transformer", decoder_conf=dict(attention_heads=heads, linear_units=256, num_blocks=1),
                model_conf=dict(ctc_weight=0.3), compute_dtype=dtype)


def _model(cfg, seed=3):
    """ASRTask model with recipe weights (oracle.weights.recipe_tensor) for every parameter but the mel matrix."""
    from espnet_amd.tasks.asr import ASRTask

    model = ASRTask.build_model(cfg)
    sd = {k: (v.detach().float().cpu() if k == "frontend.logmel.melmat" else recipe_tensor(k, v.shape, seed))
          for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd


def _speech(lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    wav = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        wav[b, :n] = 0.1 * torch.randn(n, generator=g)
    return wav


@pytest.mark.parametrize("d,heads,ff,blocks,layer", [(256, 4, 2048, 12, "conv2d"), (256, 4, 1024, 2, "conv2d6"),
                                                     (256, 4, 1024, 2, "conv2d8"), (512, 8, 2048, 3, "conv2d")])
def test_encode_matches_the_restatement(d, heads, ff, blocks, layer):
    lens = [16000 * 4, 16000 * 3 - 555]  # a padded ragged batch: reference semantics (keys masked by olens)
    speech = _speech(lens)
    cfg = _cfg(d, heads, ff, blocks, layer)
    m32, sd = _model(cfg)
    with torch.no_grad():
        ref, rol = tr.encode(sd, speech, torch.tensor(lens), heads, blocks, 512, 400, 160)
    st = m32.encode_device(speech.cuda(), lens)
    assert st.olens == rol.tolist()
    for b, n in enumerate(st.olens):
        err = (st.enc_out[b, :n].cpu() - ref[b, :n]).abs().max().item()
        assert err < 2e-3, ("f32", b, err)
    m16, _ = _model(dict(cfg, compute_dtype="bfloat16"))
    st16 = m16.encode_device(speech.cuda(), lens)
    for b, n in enumerate(st16.olens):
        rel = ((st16.enc_out[b, :n].cpu() - ref[b, :n]).norm() / ref[b, :n].norm()).item()
        assert rel < 3e-2, ("bf16", b, rel)
    # ESPnetASRModel.encode (the reference's entry) is the same computation
    enc, olens = m32.encode(speech.cuda(), torch.tensor(lens))
    assert olens.tolist() == st.olens
    assert torch.equal(enc.cpu(), st.enc_out.cpu())


def test_isolated_rows_equal_each_utterance_alone():
    lens = [16000 * 3, 16000 * 2 - 321, 9000]
    speech = _speech(lens, seed=11)
    m32, sd = _model(_cfg(256, 4, 1024, 3))
    st = m32.encode_device(speech.cuda(), lens, isolate=True)
    for b, n in enumerate(lens):
        with torch.no_grad():
            r, ol = tr.encode(sd, speech[b : b + 1, :n], torch.tensor([n]), 4, 3, 512, 400, 160)
        T = int(ol[0])
        assert st.olens[b] == T
        assert (st.enc_out[b, :T].cpu() - r[0]).abs().max().item() < 2e-3, b


def test_too_short_input_raises():
    from espnet_amd import lib as L

    m32, _ = _model(_cfg(256, 4, 1024, 1))
    with pytest.raises(L.TooShortUttError):
        m32.encode_device(torch.zeros(1, 900).cuda(), [900])  # 6 feature frames < 7
    with pytest.raises(oc.TooShortUttError):
        tr.transformer_encoder(dict(m32.state_dict()), torch.zeros(1, 6, 80), torch.tensor([6]), 4, 1)


def test_transformer_512_row_block_relu_ffn_matches_per_operator():
    """At d = 512 (bf16) the FFN + residual + the next LayerNorm is one row-block launch of csrc/ffn_rows.hip with ReLU when
    a round of 64-row workgroups fills its share of the chip.  Forced on (fill rule lowered) against forced off
    (ESPNET_AMD_NO_FFN_ROWS): equal to bf16 round-off, both against the f32 restatement under the bf16 bound."""
    from espnet_amd import lib as L

    cfg = _cfg(512, 8, 2048, 3, dtype="bfloat16")
    model, sd = _model(cfg, seed=5)
    n, B = 16000 * 3, 6
    one = _speech([n], seed=9)
    wav = one.repeat(B, 1).cuda()
    lens = [n] * B
    lib = L.load()

    def run(env):
        for k, v in env.items():
            os.environ[k] = v
        lib.em_dev_switches_reload()
        try:
            model.encoder.invalidate()
            st = model.encode_device(wav, lens)
            return st.enc_out.float().cpu(), st.olens
        finally:
            for k in env:
                del os.environ[k]
            lib.em_dev_switches_reload()

    rows, olens = run({"ESPNET_AMD_FFN_ROWS_MIN_FILL": "1"})
    plain, _ = run({"ESPNET_AMD_NO_FFN_ROWS": "1"})
    T = int(olens[0])
    for k in (1, B - 1):
        assert torch.equal(rows[0], rows[k]), k
    dd = (rows[0, :T] - plain[0, :T]).abs()
    print(f"[transformer 512, row-block vs per-operator] max {dd.max():.3e} mean {dd.mean():.3e}")
    assert dd.max() < 0.08 and dd.mean() < 6e-3 and dd.max() > 0.0  # (> 0: the two paths really are different launches)
    with torch.no_grad():
        ref, ol = tr.encode(sd, one, torch.tensor([n]), 8, 3, 512, 400, 160)
    assert int(ol[0]) == T
    for name, enc in (("row-block", rows), ("per-operator", plain)):
        rel = (enc[0, :T] - ref[0]).norm() / ref[0].norm()
        assert rel < 3e-2, (name, float(rel))


# ------------------------------------------------------------------------------------------- 3. end to end
def _write_model(tmp_path, dtype_seed=13):
    """A Transformer-encoder yaml + .pth: the decode fixture's frontend / decoder / CTC with a transformer encoder_conf,
    recipe weights for the encoder."""
    import yaml

    from espnet_amd.fileio.sound_scp import write_wav_pcm16
    from oracle.weights import synth_waveform
    from espnet_amd.tasks.asr import ASRTask

    g = load_golden("cli_decode")
    conf = yaml.safe_load(str(g["config_yaml"]))
    conf["encoder"] = "transformer"
    conf["encoder_conf"] = dict(output_size=128, attention_heads=2, linear_units=256, num_blocks=3, input_layer="conv2d",
                                dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.1,
                                normalize_before=True)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    sd = {k: v for k, v in golden_state_dict(g).items() if not k.startswith("encoder.")}
    shapes = ASRTask.build_model(dict(conf, compute_dtype="float32")).state_dict()
    for k, v in shapes.items():
        if k.startswith("encoder."):
            sd[k] = recipe_tensor(k, v.shape, dtype_seed)
    torch.save(sd, tmp_path / "model.pth")
    lines = []
    for key, u, n in json.loads(str(g["utts"])):
        write_wav_pcm16(tmp_path / f"{key}.wav", synth_waveform(u, n).numpy(), 16000)
        lines.append(f"{key} {tmp_path / (key + '.wav')}")
    (tmp_path / "wav.scp").write_text("\n".join(lines) + "\n")
    return g, conf, sd


def test_speech2text_greedy_beam_and_batch_decode(tmp_path):
    import oracle.beam_search as ob
    from espnet_amd.bin.asr_inference import Speech2Text
    from espnet_amd.fileio.sound_scp import read_wav

    g, conf, sd = _write_model(tmp_path)
    ec, dc = conf["encoder_conf"], conf["decoder_conf"]
    V = len(conf["token_list"])
    fc = conf["frontend_conf"]
    wavs = []
    for ln in (tmp_path / "wav.scp").read_text().splitlines():
        x = read_wav(ln.split()[1], dtype="float32")[0]
        if len(x) >= 16000:
            wavs.append(torch.as_tensor(x))
    wavs = wavs[:3]
    beam, cw = int(g["beam"]), float(g["ctc_weight"])
    kw = dict(asr_train_config=str(tmp_path / "config.yaml"), asr_model_file=str(tmp_path / "model.pth"), device="cuda",
              dtype="float32", lm_weight=0.0)
    greedy = Speech2Text(**kw, ctc_greedy=True, nbest=1)
    s2t = Speech2Text(**kw, beam_size=beam, ctc_weight=cw, nbest=1)
    for x in wavs:
        with torch.no_grad():
            enc, ol = tr.encode(sd, x[None], torch.tensor([len(x)]), ec["attention_heads"], ec["num_blocks"],
                                fc["n_fft"], fc["win_length"], fc["hop_length"])
        T = int(ol[0])
        want = oc.greedy_ctc(sd, enc, ol, blank=0, sos_eos=V - 1)[0]
        assert greedy(x)[0][2] == want
        ref = ob.beam_search(sd, enc[0, :T], dc["attention_heads"], dc["num_blocks"], beam, cw, sos=V - 1, eos=V - 1)
        hyp = s2t(x)[0][3]
        assert hyp.yseq.tolist() == ref[0]["yseq"], (hyp.yseq.tolist(), ref[0]["yseq"])
        assert abs(float(hyp.score) - ref[0]["score"]) < 2e-3, (float(hyp.score), ref[0]["score"])
    # utterance-batched decoding equals one call per utterance
    lens = [len(x) for x in wavs]
    pad = torch.zeros(len(wavs), max(lens))
    for b, x in enumerate(wavs):
        pad[b, : len(x)] = x
    for obj in (greedy, s2t):
        batched = obj.batch_decode(pad, lens)
        for b, x in enumerate(wavs):
            one = obj(x)
            assert batched[b][0][2] == one[0][2], b
            if obj is s2t:
                assert abs(float(batched[b][0][3].score) - float(one[0][3].score)) < 1e-3


def test_decode_cli_writes_1best(tmp_path):
    from espnet_amd.bin.asr_inference import main

    g, conf, _ = _write_model(tmp_path)
    out = tmp_path / "out"
    main(["--output_dir", str(out), "--ngpu", "1", "--data_path_and_name_and_type", f"{tmp_path / 'wav.scp'},speech,sound",
          "--asr_train_config", str(tmp_path / "config.yaml"), "--asr_model_file", str(tmp_path / "model.pth"),
          "--beam_size", str(int(g["beam"])), "--ctc_weight", str(float(g["ctc_weight"])), "--nbest", "1",
          "--lm_weight", "0.0", "--dtype", "float32", "--batch_size", "2"])
    keys = [ln.split()[0] for ln in (tmp_path / "wav.scp").read_text().splitlines()]
    for name in ("token_int", "text", "score"):
        lines = (out / "1best_recog" / name).read_text().splitlines()
        assert {ln.split(maxsplit=1)[0] for ln in lines} <= set(keys) and len(lines) >= len(keys) - 1, name
