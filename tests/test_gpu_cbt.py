"""GPU parity of the streaming Transformer encoder (`encoder: contextual_block_transformer`) against tests/cbt_reference.py
(oracle/streaming.py's golden-pinned state machine around the Transformer layer), in two configurations: tiny (2 layers,
d 128, 2 heads, ff 256: the per-operator launches) and the streaming recipe (12 x 256d, 4 heads, ff 2048, block 40 / hop 16
/ look-ahead 16: the row-block launches of csrc/block.hip, EM_BLOCK_Q / EM_BLOCK_T).  Tolerances are those of
tests/test_gpu_streaming.py."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.cbt_reference import RECIPE, TINY, CBTEncoderOracle, seeded_state_dict  # noqa: E402
from tests.cbt_reference import run_chunks as ref_chunks  # noqa: E402

CONFS = {"tiny": TINY, "recipe": RECIPE}
N_SAMPLES = 96000  # 6 s


def _config(conf, vocab=50):
    from oracle.weights import token_list

    return dict(token_list=token_list(vocab), frontend="default",
                frontend_conf=dict(n_fft=512, hop_length=160, win_length=400), normalize="utterance_mvn",
                normalize_conf={}, encoder="contextual_block_transformer", encoder_conf=dict(conf),
                decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
                model_conf=dict(ctc_weight=0.3))


def _feats(utt, n=N_SAMPLES):
    from tests.helpers import stream_feats

    return stream_feats(utt, n)


_CACHE = {}


def build(name, dtype):
    """(encoder on the GPU, its state dict on the CPU): seeded random-init, built through ASRTask.build_model."""
    from espnet_amd.tasks.asr import ASRTask

    torch.manual_seed(11)
    model = ASRTask.build_model(dict(_config(CONFS[name]), compute_dtype=dtype))
    enc = model.encoder
    if name not in _CACHE:
        _CACHE[name] = seeded_state_dict(enc, 21)
    enc.load_state_dict(_CACHE[name], strict=True)
    return enc.cuda().eval(), _CACHE[name]


def oracle(name, sd):
    c = CONFS[name]
    return CBTEncoderOracle(sd, c["attention_heads"], c["num_blocks"], c["block_size"], c["hop_size"], c["look_ahead"])


_REF = {}


def reference(name, sd, utt=0, chunk=64, n=N_SAMPLES):
    key = (name, utt, chunk, n)
    if key not in _REF:
        _REF[key] = ref_chunks(oracle(name, sd), _feats(utt, n), chunk)
    return _REF[key]


def run_chunks(enc, feats, cf):
    outs, lens, state, pos = [], [], None, 0
    while pos < feats.size(0):
        nxt = min(feats.size(0), pos + cf)
        y, _, state = enc(feats[None, pos:nxt].cuda(), torch.tensor([nxt - pos]), state, is_final=(nxt == feats.size(0)),
                          infer_mode=True)
        outs.append(y[0])
        lens.append(int(y.size(1)))
        pos = nxt
    return torch.cat(outs, 0).cpu(), lens


def run_batch(enc, feats, cf):
    outs, lens, state, pos, T = [], [], None, 0, feats.size(1)
    while pos < T:
        nxt = min(T, pos + cf)
        y, y_len, state = enc.forward_infer_batch(feats[:, pos:nxt].cuda(), state, is_final=(nxt == T))
        outs.append(y)
        lens.append(y_len)
        pos = nxt
    return torch.cat(outs, 1).cpu(), lens


def switches(**env):
    from espnet_amd import lib as L

    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    L.load().em_dev_switches_reload()


@pytest.fixture(autouse=True)
def _clean_switches():
    yield
    switches(ESPNET_AMD_STREAM_NO_FUSED=None, ESPNET_AMD_STREAM_NO_CTX_FOLD=None, ESPNET_AMD_STREAM_TF_MERGE=None)


@pytest.mark.parametrize("name", ["tiny", "recipe"])
def test_f32_matches_reference(name):
    """f32: chunk by chunk (64-frame chunks, last call final), one shot, and the short-utterance path; atol 2e-3 (f32 MFMA vs
    CPU fp32: summation-order round-off through the layers), identical frame counts per call."""
    enc, sd = build(name, "float32")
    feats = _feats(0)
    want, want_lens = reference(name, sd)
    ys, lens = run_chunks(enc, feats, 64)
    assert lens == want_lens
    e = (ys - want).abs().max().item()
    one, one_lens = run_chunks(enc, feats, 10 ** 6)
    want1, want1_lens = reference(name, sd, chunk=10 ** 6)
    e1 = (one - want1).abs().max().item()
    short, short_lens = run_chunks(enc, feats[:100], 10 ** 6)
    wants, wants_lens = ref_chunks(oracle(name, sd), feats[:100], 10 ** 6)
    es = (short - wants).abs().max().item()
    print(f"[cbt f32 {name}] chunked {e:.2e} one-shot {e1:.2e} short {es:.2e}")
    assert one_lens == want1_lens and short_lens == wants_lens and short.size(0) == 24
    assert e < 2e-3 and e1 < 2e-3 and es < 2e-3


def test_f32_chunking_invariance():
    enc, _ = build("tiny", "float32")
    feats = _feats(1)
    a, _ = run_chunks(enc, feats, 37)
    b, _ = run_chunks(enc, feats, 64)
    c, _ = run_chunks(enc, feats, 10 ** 6)
    assert a.shape == b.shape == c.shape
    assert (a - b).abs().max().item() < 1e-4 and (a - c).abs().max().item() < 1e-4


def _bound(a, b, what):
    err = (a.float() - b.float()).abs()
    print(f"[cbt bf16 {what}] max {err.max().item():.3e} mean {err.mean().item():.3e}")
    assert err.max().item() < 0.2 and err.mean().item() < 0.02, what


def test_bf16_fused_and_per_operator_within_tolerance():
    """bf16, the recipe shape: the row-block launches AND the per-operator sequence (ESPNET_AMD_STREAM_NO_FUSED=1) against the
    reference, and against each other, chunk by chunk (the steady tick: one block per call), one shot (several blocks per
    call) and on the short-utterance path; the recipe shape really takes the fused launches."""
    enc, sd = build("recipe", "bfloat16")
    feats = _feats(0)
    want, want_lens = reference("recipe", sd)
    want1, _ = reference("recipe", sd, chunk=10 ** 6)
    wants, _ = ref_chunks(oracle("recipe", sd), feats[:100], 10 ** 6)
    switches(ESPNET_AMD_STREAM_NO_FUSED=None)
    assert enc._fusable() and enc.plan(1, 1, True) in (2, 3) and enc.plan(1, 8, True) == 1
    ys_f, lens_f = run_chunks(enc, feats, 64)
    one_f, _ = run_chunks(enc, feats, 10 ** 6)
    short_f, _ = run_chunks(enc, feats[:100], 10 ** 6)
    switches(ESPNET_AMD_STREAM_NO_FUSED=1)
    assert enc.plan(1, 1, True) == 0
    ys_u, lens_u = run_chunks(enc, feats, 64)
    one_u, _ = run_chunks(enc, feats, 10 ** 6)
    short_u, _ = run_chunks(enc, feats[:100], 10 ** 6)
    switches(ESPNET_AMD_STREAM_NO_FUSED=None)
    assert lens_f == lens_u == want_lens
    _bound(ys_f, want, "fused vs reference, chunked")
    _bound(ys_u, want, "per-operator vs reference, chunked")
    _bound(ys_f, ys_u, "fused vs per-operator, chunked")
    _bound(one_f, want1, "fused vs reference, one-shot")
    _bound(one_u, want1, "per-operator vs reference, one-shot")
    _bound(one_f, one_u, "fused vs per-operator, one-shot")
    _bound(short_f, wants, "fused vs reference, short")
    _bound(short_u, wants, "per-operator vs reference, short")
    _bound(short_f, short_u, "fused vs per-operator, short")


def test_bf16_tiny_per_operator_within_tolerance():
    enc, sd = build("tiny", "bfloat16")
    assert not enc._fusable() and enc.plan(1, 1, True) == 0
    want, want_lens = reference("tiny", sd)
    ys, lens = run_chunks(enc, _feats(0), 64)
    assert lens == want_lens
    _bound(ys, want, "tiny per-operator vs reference")


def test_hand_over_in_the_launches_equals_its_own_launch():
    """One block per stream and call: the context hand-over folded into the launches (row0_src / last_dst) - as two launches
    per layer and with a layer's second launch carrying the next layer's first (ESPNET_AMD_STREAM_TF_MERGE) - moves rows
    only: bit for bit the hand-over as its own launch (ESPNET_AMD_STREAM_NO_CTX_FOLD), 8 lock-step streams, chunk by chunk."""
    enc, sd = build("recipe", "bfloat16")
    feats = torch.stack([_feats(s) for s in range(8)])
    runs = {}
    for tag, env in (("launch", dict(ESPNET_AMD_STREAM_NO_CTX_FOLD=1, ESPNET_AMD_STREAM_TF_MERGE=None)),
                     ("fold2", dict(ESPNET_AMD_STREAM_NO_CTX_FOLD=None, ESPNET_AMD_STREAM_TF_MERGE=0)),
                     ("merged", dict(ESPNET_AMD_STREAM_NO_CTX_FOLD=None, ESPNET_AMD_STREAM_TF_MERGE=1))):
        switches(**env)
        assert enc.plan(8, 1, True) == {"launch": 1, "fold2": 2, "merged": 3}[tag]
        runs[tag], _ = run_batch(enc, feats, 64)
    assert torch.equal(runs["fold2"], runs["launch"]) and torch.equal(runs["merged"], runs["launch"])
    assert (runs["launch"][0] - runs["launch"][1]).abs().max().item() > 0.1  # (different utterances)
    want, _ = reference("recipe", sd)
    _bound(runs["merged"][0], want, "stream 0 of 8 vs reference")


@pytest.mark.parametrize("name,dtype", [("recipe", "bfloat16"), ("tiny", "float32")])
def test_step_graph_replay_equals_eager(name, dtype):
    from espnet_amd.asr.encoder._contextual_block_base import StreamingStepGraph

    enc, _ = build(name, dtype)
    feats = _feats(2).cuda()
    cf = 64
    eager, state, pos = [], None, 0
    while pos < feats.size(0):
        nxt = min(feats.size(0), pos + cf)
        y, _, state = enc.forward_infer(feats[None, pos:nxt], torch.tensor([nxt - pos]), state, nxt == feats.size(0))
        eager.append(y[0].clone())
        pos = nxt
    runner = StreamingStepGraph(enc, cf)
    for rep in range(2):
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


@pytest.mark.parametrize("name,dtype", [("tiny", "float32"), ("recipe", "float32"), ("recipe", "bfloat16")])
def test_batch_of_five_streams_equals_single_streams(name, dtype):
    enc, sd = build(name, dtype)
    feats = torch.stack([_feats(10 + s) for s in range(5)])
    singles = [run_chunks(enc, feats[s], 64) for s in range(5)]
    got, lens = run_batch(enc, feats, 64)
    assert lens == singles[0][1]
    for s in range(5):
        if dtype == "float32":
            err = (got[s] - singles[s][0]).abs().max().item()
            assert err < 2e-4, (s, err)
        else:
            _bound(got[s], singles[s][0], f"batch row {s} vs single")
    assert (got[0] - got[1]).abs().max().item() > 0.1
    if dtype == "float32":
        want, _ = ref_chunks(oracle(name, sd), feats[0], 64)
        assert (got[0] - want).abs().max().item() < 2e-3


def _s2t(tmp_path, name, beam, **kw):
    import yaml

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming

    (tmp_path / "config.yaml").write_text(yaml.safe_dump(_config(CONFS[name])))
    torch.manual_seed(31)
    s2t = Speech2TextStreaming(str(tmp_path / "config.yaml"), None, device="cuda", dtype="float32", beam_size=beam, **kw)
    sd = s2t.asr_model.state_dict()
    new = dict(seeded_state_dict(s2t.asr_model, 41))
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    # a peaked CTC / output head: clear top-1 gaps, so that f32 round-off cannot reorder hypotheses
    for k in ("ctc.ctc_lo.weight", "decoder.output_layer.weight"):
        new[k] = new[k] * 6.0
    s2t.asr_model.load_state_dict(new, strict=True)
    return s2t, {k: v.detach().cpu().float() for k, v in s2t.asr_model.state_dict().items()}


@pytest.mark.parametrize("name", ["tiny", "recipe"])
def test_speech2text_streaming_beam3_end_to_end_f32(name, tmp_path):
    """Speech2TextStreaming over this encoder + the Transformer decoder + CTC, beam 3, fed in chunks: the frames handed to the
    search per call equal the reference encoder's in count and within 2e-3; the final n-best equals that of
    oracle.beam_search_online.OnlineBeamSearchOracle run on the reference encoder's frames (scores within the project's f32
    search bound, 2e-3 + 2e-5 |score|)."""
    from oracle.beam_search_online import OnlineBeamSearchOracle
    from oracle.weights import synth_waveform

    s2t, sd = _s2t(tmp_path, name, 3, ctc_weight=0.3, nbest=3, use_hipgraph=False)
    assert s2t.search == "online"
    s2t.beam_search.max_frames = 256
    m = s2t.asr_model
    esd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    orc = oracle(name, esd)
    search = OnlineBeamSearchOracle(sd, 4, 1, 3, 0.3, m.sos, m.eos)
    handed = []
    inner = s2t._encode_chunk

    def spy(feats, is_final):
        y = inner(feats, is_final)
        handed.append((feats.detach().cpu().clone(), y.detach().cpu().clone(), is_final))
        return y

    s2t._encode_chunk = spy
    n, chunk = 80000, 10240
    wav = synth_waveform(30, n)
    res = []
    for pos in range(0, n, chunk):
        nxt = min(n, pos + chunk)
        res = s2t(wav[pos:nxt], is_final=(nxt == n))
    state, ref, worst = None, [], 0.0
    for feats, y, fin in handed:
        want, state = orc.forward_infer(feats, state, fin)
        assert y.shape == want.shape
        if y.numel():
            worst = max(worst, (y - want).abs().max().item())
        ref = search.forward(want, is_final=fin)
    print(f"[cbt e2e {name}] {len(handed)} calls, frames handed to the search within {worst:.2e}")
    assert worst < 2e-3
    ref = ref[:3]
    assert len(res) == len(ref) and len(res) >= 1
    for (text, token, token_int, hyp), r in zip(res, ref):
        assert hyp.yseq.tolist() == [int(t) for t in r["yseq"]]
        assert abs(float(hyp.score) - float(r["score"])) < 2e-3 + 2e-5 * abs(float(r["score"]))


def test_batch_call_and_stream_pool_equal_single_streams(tmp_path):
    """Greedy through batch_call for 4 streams equals the 4 streams alone; a StreamPool with streams joining and finishing
    at different ticks returns what the single streams return."""
    from oracle.weights import synth_waveform

    s2t, _ = _s2t(tmp_path, "recipe", 1, use_hipgraph=False)
    N, CH, S = 80000, 10240, 4
    wavs = torch.stack([synth_waveform(40 + s, N) for s in range(S)])

    def single(w):
        res = []
        for pos in range(0, w.numel(), CH):
            nxt = min(w.numel(), pos + CH)
            res = s2t(w[pos:nxt], is_final=(nxt == w.numel()))
        return res[0][2]

    singles = [single(wavs[s]) for s in range(S)]
    got = []
    for pos in range(0, N, CH):
        nxt = min(N, pos + CH)
        got = s2t.batch_call(wavs[:, pos:nxt], is_final=(nxt == N))
    assert len(got) == S and all(got[s] == singles[s] for s in range(S))
    assert len(singles[0]) > 0 and got[0] != got[1]
    plan = [("a", 80000, 0), ("b", 64000, 0), ("c", 93000, 2), ("d", 52000, 5), ("e", 30000, 6)]
    pw = {sid: synth_waveform(60 + k, n) for k, (sid, n, _) in enumerate(plan)}
    alone = {sid: single(pw[sid]) for sid, _, _ in plan}
    pool = s2t.stream_pool()
    pos = {sid: 0 for sid, *_ in plan}
    done, out_of, tick = set(), {}, 0
    while len(done) < len(plan):
        chunks = {}
        for sid, n, join in plan:
            if sid in done or tick < join:
                continue
            nxt = min(n, pos[sid] + CH)
            chunks[sid] = (pw[sid][pos[sid]:nxt], nxt == n)
            pos[sid] = nxt
        out = pool.tick(chunks)
        for sid, (_, fin) in chunks.items():
            if fin:
                done.add(sid)
                out_of[sid] = out[sid]
        tick += 1
        assert tick < 40
    for sid, *_ in plan:
        assert out_of[sid] == alone[sid], sid
    assert not pool.streams
