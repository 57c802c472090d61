"""GPU parity of the streaming (contextual block) Conformer encoder step (SURVEY.md §8(a) A16,
BASELINE config 5) against fixtures produced by the reference class fed chunk by chunk."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import load_stream_golden, stream_feats  # noqa: E402


def build(g, dtype):
    from espnet_amd.asr.encoder.contextual_block_conformer_encoder import ContextualBlockConformerEncoder

    enc = ContextualBlockConformerEncoder(input_size=80, compute_dtype=dtype, **g["conf"])
    enc.load_state_dict(g["sd"], strict=True)
    return enc.cuda().eval()


def run_chunks(enc, feats, cf):
    outs, lens, state, pos = [], [], None, 0
    while pos < feats.size(0):
        nxt = min(feats.size(0), pos + cf)
        y, _, state = enc(feats[None, pos:nxt].cuda(), torch.tensor([nxt - pos]), state,
                          is_final=(nxt == feats.size(0)), infer_mode=True)
        outs.append(y[0])
        lens.append(int(y.size(1)))
        pos = nxt
    return torch.cat(outs, 0), lens


@pytest.mark.parametrize("name", ["stream_tiny_4s", "stream_tiny_short", "stream_small_6s"])
def test_streaming_encoder_f32_matches_reference(name):
    g = load_stream_golden(name)
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"]))
    enc = build(g, "float32")
    ys, lens = run_chunks(enc, feats, int(g["chunk_frames"]))
    assert lens == g["out_lens"].tolist()  # same frames emitted by every call
    ke = int(g["keep_every"])
    # f32 MFMA vs CPU fp32: summation-order round-off through 12 layers of O(1) activations
    np.testing.assert_allclose(ys.cpu()[::ke].numpy(), g["ys"], atol=2e-3, rtol=0)
    y1, _, _ = enc(feats[None].cuda(), torch.tensor([feats.size(0)]), None, is_final=True, infer_mode=True)
    np.testing.assert_allclose(y1[0].cpu()[::ke].numpy(), g["ys_oneshot"], atol=2e-3, rtol=0)


def test_streaming_encoder_bf16_within_tolerance():
    g = load_stream_golden("stream_small_6s")
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"]))
    enc = build(g, "bfloat16")
    ys, lens = run_chunks(enc, feats, int(g["chunk_frames"]))
    assert lens == g["out_lens"].tolist()
    err = np.abs(ys.cpu()[:: int(g["keep_every"])].numpy() - g["ys"])
    # LayerNorm'ed outputs are O(1); bf16 operands through 12 layers
    assert err.max() < 0.2 and err.mean() < 0.02, (err.max(), err.mean())


def test_streaming_fused_layers_match_per_operator_sequence():
    """Round 4: the contextual-block layer as five launches on the row-block kernels (csrc/block.hip with EM_BLOCK_RELU,
    conv width 15, ff 2048; csrc/streaming.hip `cb_fusable`) against the thirteen-launch sequence of the same bf16
    weights: same frames per call, outputs equal to bf16 round-off of differently ordered sums; both within the bf16
    tolerance of the reference fixture; also the one-shot (many blocks at once) and short-utterance paths."""
    import os

    from espnet_amd import lib as _L

    os.environ.pop("ESPNET_AMD_STREAM_FUSED_MIN", None)  # (rounds 4 - 5: calls of fewer than 8 blocks kept the per-operator sequence)
    _L.load().em_dev_switches_reload()
    g = load_stream_golden("stream_small_6s")
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"]))
    enc = build(g, "bfloat16")
    assert enc._fusable()
    ys_f, lens_f = run_chunks(enc, feats, int(g["chunk_frames"]))
    one_f, _, _ = enc(feats[None].cuda(), torch.tensor([feats.size(0)]), None, is_final=True, infer_mode=True)
    short_f, _, _ = enc(feats[None, :100].cuda(), torch.tensor([100]), None, is_final=True, infer_mode=True)
    enc.fused = False
    enc.invalidate()
    ys_u, lens_u = run_chunks(enc, feats, int(g["chunk_frames"]))
    one_u, _, _ = enc(feats[None].cuda(), torch.tensor([feats.size(0)]), None, is_final=True, infer_mode=True)
    short_u, _, _ = enc(feats[None, :100].cuda(), torch.tensor([100]), None, is_final=True, infer_mode=True)
    assert lens_f == lens_u == g["out_lens"].tolist()
    for name, a, b in (("chunked", ys_f, ys_u), ("one-shot", one_f, one_u), ("short", short_f, short_u)):
        d = (a.float() - b.float()).abs()
        print(f"[stream fused vs per-operator, {name}] max {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert d.max().item() < 8e-2 and d.mean().item() < 8e-3, name
    err = np.abs(ys_f.cpu()[:: int(g["keep_every"])].numpy() - g["ys"])
    assert err.max() < 0.2 and err.mean() < 0.02, (err.max(), err.mean())


def test_streaming_chunking_invariance():
    """Size-independent property: the frames a streaming run emits do not depend on how the audio
    is cut into calls once a block is complete -- chunked == one-shot (f32, same kernels)."""
    g = load_stream_golden("stream_tiny_4s")
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"]))
    enc = build(g, "float32")
    a, _ = run_chunks(enc, feats, 37)
    b, _ = run_chunks(enc, feats, 64)
    c, _ = run_chunks(enc, feats, 10 ** 6)
    assert a.shape == b.shape == c.shape
    assert (a - b).abs().max().item() < 1e-4
    assert (a - c).abs().max().item() < 1e-4


def test_block_mha_kernel():
    from espnet_amd import lib as L

    lib = L.load()
    torch.manual_seed(0)
    n_blk, Lb, d, h = 3, 42, 256, 4
    dk = d // h
    qkv = torch.randn(n_blk * Lb, 3 * d)
    for dt, tdt, tol in ((L.EM_F32, torch.float32, 1e-5), (L.EM_BF16, torch.bfloat16, 2e-2)):
        qd = qkv.to(tdt).cuda()
        ctx = torch.empty(n_blk * Lb, d, dtype=tdt, device="cuda")
        for mode in (0, 1):
            L.check(lib.em_block_mha(dt, L.ptr(qd), n_blk, Lb, d, h, mode, L.ptr(ctx), None), "mha")
            torch.cuda.synchronize()
            q, k, v = qd.float().cpu().view(n_blk, Lb, 3, h, dk).permute(2, 0, 3, 1, 4)
            sc = q @ k.transpose(-1, -2) / dk ** 0.5
            if mode:
                m = torch.zeros(Lb, Lb, dtype=torch.bool)
                m[1:, : Lb - 1] = True
                sc = sc.masked_fill(~m, torch.finfo(torch.float32).min)
                ref = (torch.softmax(sc, -1).masked_fill(~m, 0.0) @ v)
            else:
                ref = torch.softmax(sc, -1) @ v
            ref = ref.permute(0, 2, 1, 3).reshape(n_blk * Lb, d)
            assert (ctx.float().cpu() - ref).abs().max().item() < tol, (dt, mode)


def test_streaming_step_hipgraph_replay_equals_eager():
    """BASELINE config 5: the steady-state chunk step replayed from a hipGraph gives exactly the
    eager results (same kernels, same data), including across the eager -> graph -> final hand-over."""
    from espnet_amd.asr.encoder._contextual_block_base import StreamingStepGraph

    g = load_stream_golden("stream_small_6s")
    feats = stream_feats(int(g["utt_id"]), int(g["n_samples"])).cuda()
    enc = build(g, "bfloat16")
    cf = 64  # 640 ms of 10 ms frames -> 16 encoder frames = one block per call
    eager, state, pos = [], None, 0
    while pos < feats.size(0):
        nxt = min(feats.size(0), pos + cf)
        y, _, state = enc.forward_infer(feats[None, pos:nxt], torch.tensor([nxt - pos]), state,
                                        nxt == feats.size(0))
        eager.append(y[0].clone())
        pos = nxt
    runner = StreamingStepGraph(enc, cf)
    for rep in range(2):  # second utterance reuses the captured graph
        got, pos = [], 0
        runner.reset()
        while pos < feats.size(0):
            nxt = min(feats.size(0), pos + cf)
            got.append(runner(feats[pos:nxt], is_final=(nxt == feats.size(0))).clone())
            pos = nxt
        assert runner.n_replays > 0
        assert [t.size(0) for t in got] == [t.size(0) for t in eager]
        for a, b in zip(got, eager):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["stream_frontend_gmvn", "stream_frontend_umvn"])
def test_streaming_apply_frontend_matches_reference(name, tmp_path):
    """Speech2TextStreaming.apply_frontend: waveform overlap buffer + edge trimming on the host,
    features from the HIP frontend; per-call feature counts and values vs the reference."""
    import json
    import types

    from espnet_amd.asr.frontend.default import DefaultFrontend
    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from espnet_amd.layers.global_mvn import GlobalMVN
    from espnet_amd.layers.utterance_mvn import UtteranceMVN
    from oracle.weights import synth_waveform
    from tests.helpers import GOLDEN

    z = np.load(GOLDEN / f"{name}.npz")
    fc = json.loads(str(z["frontend_conf"]))
    fe = DefaultFrontend(**fc)
    fe.logmel.melmat.copy_(torch.from_numpy(z["melmat"]))
    if bool(z["use_global_mvn"]):
        np.savez(tmp_path / "stats.npz", count=np.array(1.0), sum=z["gmvn_mean"],
                 sum_square=z["gmvn_std"] ** 2 + z["gmvn_mean"] ** 2)
        norm = GlobalMVN(str(tmp_path / "stats.npz"))
        norm.mean.copy_(torch.from_numpy(z["gmvn_mean"]))
        norm.std.copy_(torch.from_numpy(z["gmvn_std"]))
    else:
        norm = UtteranceMVN()
    s2t = object.__new__(Speech2TextStreaming)
    s2t.asr_model = types.SimpleNamespace(frontend=fe.cuda(), normalize=norm.cuda())
    s2t.device, s2t.n_fft, s2t.hop_length, s2t.win_length = "cuda", fc["n_fft"], fc["hop_length"], fc["win_length"]
    n, cs = int(z["n_samples"]), int(z["chunk_samples"])
    wav = synth_waveform(int(z["utt_id"]), n)
    feats, lens, state, pos = [], [], None, 0
    while pos < n:
        nxt = min(n, pos + cs)
        f, fl, state = s2t.apply_frontend(wav[pos:nxt], state, is_final=(nxt == n))
        lens.append(-1 if f is None else int(f.size(1)))
        if f is not None:
            assert int(fl[0]) == f.size(1)
            feats.append(f[0].cpu())
        pos = nxt
    assert lens == z["feat_lens"].tolist()
    np.testing.assert_allclose(torch.cat(feats, 0).numpy(), z["feats"], atol=3e-4, rtol=0)


def test_speech2text_streaming_end_to_end(tmp_path):
    """Chunked Speech2TextStreaming (HIP frontend + hipGraph encoder step + incremental greedy CTC)
    == the same model run in one final call: identical token ids (f32), and the hipGraph path
    was actually taken."""
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import recipe_state_dict, synth_waveform, token_list

    g = load_stream_golden("stream_small_6s")
    V = 50
    cfg = dict(token_list=token_list(V), frontend="default",
               frontend_conf=dict(n_fft=512, hop_length=160, win_length=400), normalize="utterance_mvn",
               normalize_conf={}, encoder="contextual_block_conformer", encoder_conf=g["conf"],
               decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
               model_conf=dict(ctc_weight=0.3))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, device="cuda", dtype="float32",
                               beam_size=1)  # the per-chunk greedy step (the class default is the reference's 20)
    sd = s2t.asr_model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 31)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    s2t.asr_model.load_state_dict(new, strict=True)
    wav = synth_waveform(30, 80000)
    res = []
    for pos in range(0, 80000, 10240):
        nxt = min(80000, pos + 10240)
        res = s2t(wav[pos:nxt], is_final=(nxt == 80000))
    assert s2t._runner is not None and s2t._runner.n_replays > 0
    chunked = res[0][2]
    s2t.use_hipgraph = False
    oneshot = s2t(wav, is_final=True)[0][2]
    assert len(chunked) > 0 and all(isinstance(t, int) for t in chunked)
    # chunked streaming sees per-chunk utterance-MVN statistics, so only the eager-vs-graph and
    # API contract are compared here (same chunking, graph vs eager):
    s2t.reset()
    eager = []
    for pos in range(0, 80000, 10240):
        nxt = min(80000, pos + 10240)
        eager = s2t(wav[pos:nxt], is_final=(nxt == 80000))
    assert eager[0][2] == chunked
    assert isinstance(oneshot, list)


@pytest.mark.parametrize("name,dtype,atol", [("stream_tiny_4s", "float32", 2e-4), ("stream_small_6s", "float32", 2e-4),
                                             ("stream_small_6s", "bfloat16", 0.12)])
def test_batch_of_streams(name, dtype, atol):
    """Lock-step batch of streams (forward_infer_batch: one launch sequence for S streams) == every stream encoded
    alone, call by call: same frames emitted per call, same values (f32: the GEMMs pick other tiles at other row
    counts, so summation order only; bf16: operand rounding of intermediate activations differs with it)."""
    g = load_stream_golden(name)
    n, cf = int(g["n_samples"]), int(g["chunk_frames"])
    feats = torch.stack([stream_feats(int(g["utt_id"]) + s, n) for s in range(3)])  # (S, T, 80): three utterances
    enc = build(g, dtype)
    singles, lens_single = [], None
    for s in range(feats.size(0)):
        ys, lens = run_chunks(enc, feats[s], cf)
        singles.append(ys)
        lens_single = lens
    outs, lens, state, pos = [], [], None, 0
    T = feats.size(1)
    while pos < T:
        nxt = min(T, pos + cf)
        y, y_len, state = enc.forward_infer_batch(feats[:, pos:nxt].cuda(), state, is_final=(nxt == T))
        assert y.shape[:2] == (3, y_len)
        outs.append(y)
        lens.append(y_len)
        pos = nxt
    assert lens == lens_single
    got = torch.cat(outs, 1).cpu()
    for s in range(3):
        err = (got[s] - singles[s].cpu()).abs().max().item()
        assert err < atol, (s, err)
    # the three streams are different utterances: rows must not be copies of each other
    assert (got[0] - got[1]).abs().max().item() > 0.1


def test_batch_tick_context_hand_over_in_the_block_launches_equals_its_own_launch():
    """Round 5: with one block per stream and call, the fused streaming layer takes the context hand-over between layers
    (contextual_block_encoder_layer.py:292-304) into the launches either side of it - block<A> reads slot 0 from the
    previous call's context vectors, block<D> writes the last slot to this call's (csrc/enc_host.h `stream_fold_ctx`,
    EmBlockArgs.row0_src / last_dst) - instead of a launch per layer that copies them.  Only WHERE rows are read and
    written changes: eight lock-step streams (8 blocks per call: the fused layers), chunk by chunk, bit for bit against
    the hand-over launches (ESPNET_AMD_STREAM_NO_CTX_FOLD, read per call); stream 0 against the reference fixture."""
    import os

    g = load_stream_golden("stream_small_6s")
    n, cf = int(g["n_samples"]), int(g["chunk_frames"])
    feats = torch.stack([stream_feats(int(g["utt_id"]) + s, n) for s in range(8)])
    enc = build(g, "bfloat16")
    assert enc._fusable()

    def run():
        outs, state, pos, T = [], None, 0, feats.size(1)
        while pos < T:
            nxt = min(T, pos + cf)
            y, y_len, state = enc.forward_infer_batch(feats[:, pos:nxt].cuda(), state, is_final=(nxt == T))
            outs.append(y)
            pos = nxt
        return torch.cat(outs, 1).cpu()

    from espnet_amd import lib as _L

    os.environ.pop("ESPNET_AMD_STREAM_NO_CTX_FOLD", None)
    _L.load().em_dev_switches_reload()
    folded = run()
    os.environ["ESPNET_AMD_STREAM_NO_CTX_FOLD"] = "1"
    _L.load().em_dev_switches_reload()
    try:
        launched = run()
    finally:
        os.environ.pop("ESPNET_AMD_STREAM_NO_CTX_FOLD", None)
        _L.load().em_dev_switches_reload()
    assert folded.shape == launched.shape and torch.equal(folded, launched)
    assert (folded[0] - folded[1]).abs().max().item() > 0.1  # (different utterances)
    err = np.abs(folded[0][:: int(g["keep_every"])].numpy() - g["ys"])
    assert err.max() < 0.2 and err.mean() < 0.02, (err.max(), err.mean())


@pytest.mark.parametrize("n_streams", [1, 8, 24])
def test_split_ffn_of_the_block_launches(n_streams):
    """Round 6: a tick that leaves CUs idle deals each FFN's hidden dimension to S workgroups per 32-row block (grid z of
    block<A | RELU> / block<D | RELU>, EmBlockArgs.ffn_split; csrc/enc_host.h `stream_ffn_split`: 4 shares up to 32 row blocks,
    2 up to 64): each leaves the partial sum of its share in the workspace and the LAST to arrive adds them in split order.
    Only the order of an f32 sum changes (contextual_block_encoder_layer.py:218-222, 280-284 are the FFNs): against the
    unsplit launches (ESPNET_AMD_STREAM_FFN_SPLIT=1) within bf16 round-off of the layers behind it, the same bits on a second
    run whatever the arrival order, also at 8 and 16 shares (2 chunks of 64 each: the shortest stream the ring runs), and
    stream 0 within the bf16 tolerance of the reference fixture."""
    import os

    from espnet_amd import lib as _L

    g = load_stream_golden("stream_small_6s")
    n, cf = int(g["n_samples"]), int(g["chunk_frames"])
    feats = torch.stack([stream_feats(int(g["utt_id"]) + s, n) for s in range(n_streams)])
    enc = build(g, "bfloat16")
    assert enc._fusable()

    def run(split):
        if split is None:
            os.environ.pop("ESPNET_AMD_STREAM_FFN_SPLIT", None)
        else:
            os.environ["ESPNET_AMD_STREAM_FFN_SPLIT"] = str(split)
        _L.load().em_dev_switches_reload()
        outs, state, pos, T = [], None, 0, feats.size(1)
        while pos < T:
            nxt = min(T, pos + cf)
            y, y_len, state = enc.forward_infer_batch(feats[:, pos:nxt].cuda(), state, is_final=(nxt == T))
            outs.append(y)
            pos = nxt
        return torch.cat(outs, 1).cpu()

    try:
        whole = run(1)
        for split in (None, 8, 16):
            a, b = run(split), run(split)
            assert torch.equal(a, b), f"split {split}: not repeatable"
            d = (a - whole).abs()
            print(f"[split FFN {split or 'automatic'}, {n_streams} streams] max {d.max().item():.3e} mean {d.mean().item():.3e}")
            assert d.max().item() < 8e-2 and d.mean().item() < 4e-3, split
            err = np.abs(a[0][:: int(g["keep_every"])].numpy() - g["ys"])
            assert err.max() < 0.2 and err.mean() < 0.02, (split, err.max(), err.mean())
    finally:
        os.environ.pop("ESPNET_AMD_STREAM_FFN_SPLIT", None)
        _L.load().em_dev_switches_reload()


@pytest.mark.parametrize("n_streams", [1, 8])
def test_block_attention_in_the_c_launch_equals_its_own_launch(n_streams):
    """Round 6: the plain multi-head attention over a block's slots (contextual_block_encoder_layer.py:236-262) runs in front
    of the C part IN its launch (csrc/block.hip, EM_BLOCK_ATT | EM_BLOCK_C | EM_BLOCK_RELU) instead of a launch of its own
    (csrc/streaming.hip cb_mha_heads_mfma_kernel, kept behind ESPNET_AMD_STREAM_SPLIT_ATT): the same MFMAs on the same
    operands, the context rounded to bf16 at the same point - bit for bit, chunk by chunk (contextual mask, 42 slots), one-shot
    (many blocks per call) and on the short-utterance path (no mask, a block of as many slots as there are frames)."""
    import os

    from espnet_amd import lib as _L

    g = load_stream_golden("stream_small_6s")
    n, cf = int(g["n_samples"]), int(g["chunk_frames"])
    feats = torch.stack([stream_feats(int(g["utt_id"]) + s, n) for s in range(n_streams)])
    enc = build(g, "bfloat16")
    assert enc._fusable()

    def run(split):
        if split:
            os.environ["ESPNET_AMD_STREAM_SPLIT_ATT"] = "1"
        else:
            os.environ.pop("ESPNET_AMD_STREAM_SPLIT_ATT", None)
        _L.load().em_dev_switches_reload()
        outs, state, pos, T = [], None, 0, feats.size(1)
        while pos < T:
            nxt = min(T, pos + cf)
            y, y_len, state = enc.forward_infer_batch(feats[:, pos:nxt].cuda(), state, is_final=(nxt == T))
            outs.append(y)
            pos = nxt
        one, _, _ = enc(feats[:1].cuda(), torch.tensor([feats.size(1)]), None, is_final=True, infer_mode=True)
        shorts = [enc(feats[:1, :k].cuda(), torch.tensor([k]), None, is_final=True, infer_mode=True)[0].cpu() for k in (100, 131, 163)]
        return torch.cat(outs, 1).cpu(), one.cpu(), shorts

    try:
        fused, one_f, short_f = run(False)
        split, one_s, short_s = run(True)
    finally:
        os.environ.pop("ESPNET_AMD_STREAM_SPLIT_ATT", None)
        _L.load().em_dev_switches_reload()
    assert torch.equal(fused, split) and torch.equal(one_f, one_s)
    for a, b in zip(short_f, short_s):
        assert a.shape == b.shape and a.numel() > 0 and torch.equal(a, b)
    err = np.abs(fused[0][:: int(g["keep_every"])].numpy() - g["ys"])
    assert err.max() < 0.2 and err.mean() < 0.02, (err.max(), err.mean())


def test_batch_call_equals_single_streams(tmp_path):
    """Speech2TextStreaming.batch_call (S lock-step streams, one launch sequence per tick: batched HIP frontend ->
    forward_infer_batch -> incremental greedy CTC) returns for every stream the tokens `__call__` returns for it alone
    (f32, eager single-stream runs)."""
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import recipe_state_dict, synth_waveform, token_list

    g = load_stream_golden("stream_small_6s")
    V = 50
    cfg = dict(token_list=token_list(V), frontend="default",
               frontend_conf=dict(n_fft=512, hop_length=160, win_length=400), normalize="utterance_mvn",
               normalize_conf={}, encoder="contextual_block_conformer", encoder_conf=g["conf"],
               decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
               model_conf=dict(ctc_weight=0.3))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, device="cuda", dtype="float32", beam_size=1,
                               use_hipgraph=False)
    sd = s2t.asr_model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 31)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    s2t.asr_model.load_state_dict(new, strict=True)
    N, CH, S = 80000, 10240, 3
    wavs = torch.stack([synth_waveform(40 + s, N) for s in range(S)])
    singles = []
    for s in range(S):
        res = []
        for pos in range(0, N, CH):
            nxt = min(N, pos + CH)
            res = s2t(wavs[s, pos:nxt], is_final=(nxt == N))
        singles.append(res[0][2])
    got = []
    for pos in range(0, N, CH):
        nxt = min(N, pos + CH)
        got = s2t.batch_call(wavs[:, pos:nxt], is_final=(nxt == N))
    assert len(got) == S
    # token_int of __call__ drops id 0 (= blank, already dropped here); compare the id lists
    for s in range(S):
        assert got[s] == singles[s], (s, got[s][:10], singles[s][:10])
    assert got[0] != got[1]
    # round 6: two groups of streams, a tick of each in flight on its own HIP stream (batch_call_async; the second group is the
    # first one's streams in another order): per tick what batch_call gives, results taken one tick late
    perm = [2, 0, 1]
    sts = [torch.cuda.Stream(), torch.cuda.Stream()]
    per_tick = [[], []]
    pend = [None, None]
    for pos in range(0, N, CH):
        nxt = min(N, pos + CH)
        for gi, w in enumerate((wavs, wavs[perm])):
            if pend[gi] is not None:
                per_tick[gi].append(pend[gi].result())
            pend[gi] = s2t.batch_call_async(w[:, pos:nxt].contiguous().pin_memory(), is_final=(nxt == N), group=gi, stream=sts[gi])
    for gi in range(2):
        per_tick[gi].append(pend[gi].result())
    assert per_tick[0][-1] == got and per_tick[1][-1] == [got[j] for j in perm]
    assert all(len(a[0]) <= len(b[0]) for a, b in zip(per_tick[0], per_tick[0][1:]))  # (ids only ever grow)
    assert not s2t._batches
    # ... and with the steady-state tick of a group replayed as one hipGraph (BatchTickGraph: eager until two ticks in a row have
    # the same shapes, the next one captured, the rest replayed; the final - shorter - tick eager again): the same ids, tick by
    # tick, for two utterances in a row (the second one replays the first one's graph)
    s2t.use_hipgraph = True
    for rep in range(2):
        ticks = []
        for pos in range(0, N, CH):
            nxt = min(N, pos + CH)
            ticks.append(s2t.batch_call(wavs[:, pos:nxt].contiguous().pin_memory(), is_final=(nxt == N)))
        assert ticks == per_tick[0], rep
    tgs = list(s2t._tick_graphs.values())
    assert len(tgs) == 1 and tgs[0].n_replays >= 6, [t.n_replays for t in tgs]
    s2t.use_hipgraph = False


def test_stream_pool_ragged(tmp_path):
    """Speech2TextStreaming.stream_pool(): streams that JOIN at different ticks, have different lengths, pause for a
    tick and finish at different times (per-row position offset / final flag / active set instead of
    lock step) get, each, exactly the tokens `__call__` returns for that stream alone; the live streams of a tick are
    served by a handful of batched launch sequences (groups of equal state shapes), not one per stream."""
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming
    from oracle.weights import recipe_state_dict, synth_waveform, token_list

    g = load_stream_golden("stream_small_6s")
    V = 50
    cfg = dict(token_list=token_list(V), frontend="default",
               frontend_conf=dict(n_fft=512, hop_length=160, win_length=400), normalize="utterance_mvn",
               normalize_conf={}, encoder="contextual_block_conformer", encoder_conf=g["conf"],
               decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
               model_conf=dict(ctc_weight=0.3))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, device="cuda", dtype="float32", beam_size=1,
                               use_hipgraph=False)
    sd = s2t.asr_model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 31)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    s2t.asr_model.load_state_dict(new, strict=True)
    CH = 10240
    # (stream id, samples, tick it joins at, tick it sits out)
    plan = [("a", 80000, 0, None), ("b", 64000, 0, 3), ("c", 93000, 2, None), ("d", 52000, 5, 7), ("e", 80000, 5, None),
            ("f", 30000, 6, None)]
    wavs = {sid: synth_waveform(60 + k, n) for k, (sid, n, _, _) in enumerate(plan)}
    singles = {}
    for sid, n, _, _ in plan:
        res = []
        for pos in range(0, n, CH):
            nxt = min(n, pos + CH)
            res = s2t(wavs[sid][pos:nxt], is_final=(nxt == n))
        singles[sid] = res[0][2]
    pool = s2t.stream_pool()
    pos = {sid: 0 for sid, *_ in plan}
    done, got, tick, max_groups, max_active = set(), {}, 0, 0, 0
    while len(done) < len(plan):
        chunks = {}
        for sid, n, join, pause in plan:
            if sid in done or tick < join or tick == pause:
                continue
            nxt = min(n, pos[sid] + CH)
            chunks[sid] = (wavs[sid][pos[sid]:nxt], nxt == n)
            pos[sid] = nxt
        out = pool.tick(chunks)
        max_groups, max_active = max(max_groups, pool.groups_last_tick), max(max_active, len(chunks))
        for sid, (_, fin) in chunks.items():
            if fin:
                done.add(sid)
                got[sid] = out[sid]
        tick += 1
        assert tick < 40
    for sid, *_ in plan:
        assert got[sid] == singles[sid], (sid, got[sid][:10], singles[sid][:10])
    assert not pool.streams  # every finished stream left the pool
    assert max_active >= 4 and max_groups < max_active  # batching happened: fewer launch sequences than live streams
    print(f"[stream pool] {len(plan)} ragged streams, up to {max_active} live per tick in at most {max_groups} groups")
