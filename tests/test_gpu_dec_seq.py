"""Whole-transcript scoring with the attention decoder on the device (csrc/dec_seq.hip, the head: csrc/vocab_head.hip): the source-attention kernel alone,
the chain `em_dec_seq_nll` through TransformerDecoder.sequence_nll / ESPnetASRModel.nll / batchify_nll /
Speech2Text.batch_nll, against the float64 restatement (tests/dec_seq_ref.py) on the weights and memories as the device
holds them.

Bounds (tests/dec_seq_cases.py) are 4 x the largest error of the first run (profiles/dec_seq_first_run.txt); every test
prints what it measured.  tests/test_cpu_dec_seq.py::test_defects_are_visible shows that a forgotten memory mask, a causal
mask one key too wide, a wrong position and a missing sqrt(d) each move some nll by more than four times these bounds."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from tests import dec_seq_cases as K  # noqa: E402
from tests import dec_seq_ref as R  # noqa: E402

DTYPES = ["float32", "bfloat16"]
ACT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
ROUND = {"float32": None, "bfloat16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _model(name, dtype):
    return K.build_model(name, dtype).to("cuda")


@functools.lru_cache(maxsize=None)
def _params(name, dtype):
    return R.Params(K.state_dict(name), K.MODELS[name][1], round_to=ROUND[dtype])


@functools.lru_cache(maxsize=None)
def _want(name, dtype, Lp):
    """(memory, hlens, text, lens, float64 per-token nll, ys_in_lens) of the shared case of width Lp: computed once, never
    changed."""
    V = K.MODELS[name][0]
    mem, hl = K.make_memory(1000 + Lp, round_to=ROUND[dtype])
    text, lens = K.make_text(Lp, V)
    nll, in_lens = R.nll(_params(name, dtype), mem.double(), hl, text, lens, V - 1, V - 1)
    return mem, hl, text, lens, nll, in_lens


def _tokens(model, text, lens):
    """Per-token nll through the public pieces: the host pair builder and TransformerDecoder.sequence_nll."""
    from espnet_amd.asr.espnet_model import build_dec_nll_batch

    return build_dec_nll_batch(text, lens, model.sos, model.eos, model.vocab_size)


# ---------------------------------------------------------------------- em_dec_seq_src_attention
SRC_SHAPES = [(1, 1), (31, 15), (32, 16), (33, 17), (65, 40), (200, 17)]  # (T, Lp)


def _src_case(T, Lp, heads, dtype, shared, B=5, d=K.D):
    """Random operands in the layout em_decoder_memory leaves: kv [Bm*T][2d] (k | v), V^T [Bm][d][Tpad] zero padded behind
    T.  Behind a memory's klens both hold NaN: a masked frame must contribute an exact zero whatever lies there."""
    g = torch.Generator().manual_seed(97 * T + Lp + heads)
    Bm = 2 if shared else B
    Tpad = (T + 31) // 32 * 32
    klens = torch.tensor([T, 1] if shared else [T, 1, T // 2 + 1, max(T - 1, 1), min(T, 17)], dtype=torch.int32)
    mem_of = torch.tensor([0, 1, 1, 0, 1], dtype=torch.int32) if shared else None
    qs = (torch.randn(B * Lp, d, generator=g) * 1.5).to(ACT[dtype])
    kv = torch.randn(Bm, T, 2 * d, generator=g)
    kv[..., :d] *= 1.5  # scores a few units apart
    kv = kv.to(ACT[dtype])
    valid = (torch.arange(T).unsqueeze(0) < klens.unsqueeze(1)).unsqueeze(2)
    clean = torch.where(valid, kv.double(), torch.zeros((), dtype=torch.float64))
    kv = torch.where(valid, kv, torch.full((), float("nan"), dtype=kv.dtype))
    vT = torch.zeros(Bm, d, Tpad, dtype=ACT[dtype])
    vT[:, :, :T] = kv[..., d:].transpose(1, 2)
    idx = mem_of.long() if shared else torch.arange(B)
    want = R.src_attention(qs.double().view(B, Lp, d), clean[idx][..., :d], clean[idx][..., d:], klens.long()[idx], heads)
    return qs, kv.reshape(Bm * T, 2 * d).contiguous(), vT, klens, mem_of, Bm, Tpad, want


def _run_src(dtype, qs, kv, vT, klens, mem_of, B, Bm, Lp, d, heads, T, Tpad):
    ctx = torch.full((B * Lp, d), float("nan"), dtype=ACT[dtype], device="cuda")
    dev = [t.cuda() if t is not None else None for t in (qs, kv, vT, klens, mem_of)]
    L.check(L.load().em_dec_seq_src_attention(L.DTYPES[dtype], L.ptr(dev[0]), L.ptr(dev[1]), 2 * d, L.ptr(dev[2]),
                                              L.ptr(dev[3]), L.ptr(dev[4]), B, Bm, Lp, d, heads, T, Tpad, L.ptr(ctx),
                                              L.current_stream_ptr()), "em_dec_seq_src_attention")
    return ctx.cpu().to(torch.float64).view(B, Lp, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("T,Lp", SRC_SHAPES)
def test_src_attention(T, Lp, heads, shared, dtype):
    """Five sentences of Lp queries against ragged memories (klens include 1 and T), one memory each or - `shared` - two
    memories under mem_of = [0, 1, 1, 0, 1]; ctx pre-filled with NaN: every row comes back finite and within the bound."""
    qs, kv, vT, klens, mem_of, Bm, Tpad, want = _src_case(T, Lp, heads, dtype, shared)
    got = _run_src(dtype, qs, kv, vT, klens, mem_of, 5, Bm, Lp, K.D, heads, T, Tpad)
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"\nsrc attention T {T} Lp {Lp} heads {heads} shared {shared} {dtype}: err {err:.3e}")
    assert err <= K.E_SRC[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_src_attention_long_memory(dtype):
    """T = 3 000 frames, which the label step's kernel refuses (its score rows live in LDS); Lp = 3."""
    T, Lp, heads, B, d = 3000, 3, 2, 2, K.D
    g = torch.Generator().manual_seed(3000)
    klens = torch.tensor([T, 1777], dtype=torch.int32)
    qs = (torch.randn(B * Lp, d, generator=g) * 1.5).to(ACT[dtype])
    kv = torch.randn(B, T, 2 * d, generator=g)
    kv[..., :d] *= 1.5
    kv = kv.to(ACT[dtype])
    Tpad = (T + 31) // 32 * 32
    vT = torch.zeros(B, d, Tpad, dtype=ACT[dtype])
    vT[:, :, :T] = kv[..., d:].transpose(1, 2)
    want = R.src_attention(qs.double().view(B, Lp, d), kv.double()[..., :d], kv.double()[..., d:], klens.long(), heads)
    got = _run_src(dtype, qs, kv.reshape(B * T, 2 * d).contiguous(), vT, klens, None, B, B, Lp, d, heads, T, Tpad)
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"\nsrc attention T {T} Lp {Lp} {dtype}: err {err:.3e}")
    assert err <= K.E_SRC[dtype]
    if dtype == "bfloat16":  # (the premise: the label-step kernel does refuse this memory)
        ctx = torch.empty(B, d, dtype=torch.bfloat16, device="cuda")
        dev = [t.cuda() for t in (qs[:B].contiguous(), kv.reshape(B * T, 2 * d).contiguous(), vT, klens)]
        rc = L.load().em_dec_src_attention(L.EM_BF16, L.ptr(dev[0]), L.ptr(dev[1]), 2 * d, L.ptr(dev[2]), L.ptr(dev[3]), B, 1, d,
                                           heads, T, Tpad, L.ptr(ctx), L.current_stream_ptr())
        assert rc == L.EM_ERR_UNSUPPORTED


def test_src_attention_refuses_other_head_widths():
    z = torch.zeros(4, 2 * 192, device="cuda")
    kl = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        L.check(L.load().em_dec_seq_src_attention(L.EM_F32, L.ptr(z), L.ptr(z), 2 * 192, L.ptr(z), L.ptr(kl), None, 1, 1, 1,
                                                  192, 2, 1, 32, L.ptr(z), L.current_stream_ptr()))


@pytest.mark.parametrize("Lp", [1, 5])
def test_row_position_embedding(Lp):
    """x[r] = embed[tok[r]] * sqrt(d) + pe[r % Lp] for all rows in one launch: f32 products and sums, to the last bit but
    for the fused multiply-add (2 ulp of the result's size)."""
    V, d, B = 37, K.D, 3
    g = torch.Generator().manual_seed(Lp)
    embed = torch.randn(V, d, generator=g)
    pe = R.pos_table(8, d).float()
    tok = torch.randint(0, V, (B * Lp,), generator=g, dtype=torch.int32)
    x = torch.full((B * Lp, d), float("nan"), device="cuda")
    dev = [t.cuda() for t in (embed, pe, tok)]
    args = [L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), B * Lp, V, d, Lp, 8, L.ptr(x), L.current_stream_ptr()]
    L.check(L.load().em_dec_seq_embed_f32(*args), "em_dec_seq_embed_f32")
    want = embed.double()[tok.long()] * float(torch.tensor(float(d)).sqrt()) + pe.double()[torch.arange(B * Lp) % Lp]
    err = float((x.cpu().double() - want).abs().max())
    print(f"\nrow-position embedding Lp {Lp}: err {err:.3e}")
    assert err <= 2 * 2.0 ** -23 * float(want.abs().max())
    args[6], args[7] = 9, 8  # more positions than the table holds
    with pytest.raises(ValueError):
        L.check(L.load().em_dec_seq_embed_f32(*args))


# ---------------------------------------------------------------------- the chain and the public interface
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(K.MODELS))
@pytest.mark.parametrize("Lp", K.WIDTHS)
def test_nll_against_restatement(Lp, name, dtype):
    """Per scored token (TransformerDecoder.sequence_nll) and per transcript (ESPnetASRModel.nll, their sums); where
    nothing is scored the value is exactly 0.0.  Memories of 45, 1 and 23 valid frames with N(0, 5^2) behind them."""
    mem, hl, text, lens, want, in_lens = _want(name, dtype, Lp)
    m = _model(name, dtype)
    x, km, t = _tokens(m, text, lens)
    got = m.decoder.sequence_nll(mem.cuda(), hl, x, km, t).cpu().double()
    assert got.shape == want.shape == (3, Lp)
    scored = torch.arange(Lp).unsqueeze(0) < in_lens.unsqueeze(1)
    assert (got[~scored] == 0).all() and torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"\nnll {name} Lp {Lp} {dtype}: err {err:.3e} (largest nll {float(want.max()):.2f})")
    assert err <= K.E_NLL[dtype]
    total = m.nll(mem.cuda(), hl.cuda(), text.cuda(), lens.cuda())
    assert total.shape == (3,) and total.dtype == torch.float32
    assert float((total.cpu().double() - want.sum(1)).abs().max()) <= K.E_NLL[dtype] * Lp


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_depend_on_their_own_inputs_only(dtype):
    """Bit for bit, for one (B, Lp, T): a sentence's nll does not change with the other sentences of the batch, with the
    tokens behind its own end, or with what the memory holds at and behind hlens (N(0, 5^2) against zeros)."""
    name, Lp = "h4", 17
    V = K.MODELS[name][0]
    mem, hl, text, lens, _, in_lens = _want(name, dtype, Lp)
    m = _model(name, dtype)
    x, km, t = _tokens(m, text, lens)
    run = lambda mem_, x_, km_, t_: m.decoder.sequence_nll(mem_.cuda(), hl, x_, km_, t_).cpu()  # noqa: E731
    base = run(mem, x, km, t)
    g = torch.Generator().manual_seed(5)
    # tokens behind a sentence's end (x only: the key mask and the targets say where the sentence ends)
    x2 = torch.where(km.bool(), x, torch.randint(0, V, x.shape, generator=g, dtype=torch.int32))
    assert not torch.equal(x2, x)
    assert torch.equal(run(mem, x2, km, t), base)
    # the memory behind hlens: zeros instead of noise
    valid = (torch.arange(K.T_MEM).unsqueeze(0) < hl.unsqueeze(1)).unsqueeze(2)
    mem0 = torch.where(valid, mem, torch.zeros(()))
    assert not torch.equal(mem0, mem)
    assert torch.equal(run(mem0, x, km, t), base)
    # other sentences beside sentence 0 (and other memories beside memory 0), same shapes
    text3 = torch.randint(1, V - 1, text.shape, generator=g)
    text3[0] = text[0]
    lens3 = torch.tensor([int(lens[0]), Lp - 1, 1])
    x3, km3, t3 = _tokens(m, text3, lens3)
    mem3 = torch.randn(mem.shape, generator=g).to(ACT[dtype]).float()
    mem3[0] = mem[0]
    got = run(mem3, x3, km3, t3)
    assert torch.equal(got[0], base[0]) and not torch.equal(got[1], base[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_batchify_nll(dtype):
    """Five utterances in chunks of two (a chunk size that does not divide B) and in one call."""
    name = "h2"
    V = K.MODELS[name][0]
    g = torch.Generator().manual_seed(21)
    hlens = (30, 7, 45, 1, 19)
    mem, hl = K.make_memory(77, Bm=5, hlens=hlens, round_to=ROUND[dtype])
    lens = torch.tensor([9, 33, 0, 20, 17])
    text = torch.randint(1, V - 1, (5, 33), generator=g)
    m = _model(name, dtype)
    whole = m.batchify_nll(mem.cuda(), hl.cuda(), text.cuda(), lens.cuda(), batch_size=100)
    parts = m.batchify_nll(mem.cuda(), hl.cuda(), text.cuda(), lens.cuda(), batch_size=2)
    assert parts.shape == whole.shape == (5,)
    want, _ = R.nll(_params(name, dtype), mem.double(), hl, text, lens, V - 1, V - 1)
    for got in (whole, parts):
        err = (got.cpu().double() - want.sum(1)).abs()
        print(f"\nbatchify_nll {dtype}: per-token share of the error {float((err / (lens + 1)).max()):.3e}")
        assert bool((err <= K.E_NLL[dtype] * (lens + 1)).all())


@pytest.mark.parametrize("name", sorted(K.MODELS))
def test_agrees_with_the_step_path(name):
    """`TransformerDecoder.forward` (position by position through em_decoder_step) + log-softmax + gather, f32: within
    twice the f32 bound."""
    mem, hl, text, lens, _, in_lens = _want(name, "float32", 17)
    m = _model(name, "float32")
    x, km, t = _tokens(m, text, lens)
    got = m.decoder.sequence_nll(mem.cuda(), hl, x, km, t).cpu().double()
    logits, _ = m.decoder(mem.cuda(), hl, x.long(), in_lens)
    scored = t >= 0
    step = -torch.log_softmax(logits.double(), -1).cpu().gather(2, t.long().clamp(min=0).unsqueeze(2)).squeeze(2)
    err = float(((got - step) * scored).abs().max())
    print(f"\nsequence path vs step path {name} f32: {err:.3e}")
    assert err <= 2 * K.E_NLL["float32"]


def test_workspace_and_shape_checks():
    m = _model("h2", "float32")
    dev = torch.device("cuda", torch.cuda.current_device())
    pk = m.decoder.packed(dev, 8)
    lib = L.load()
    B, Lp, T, Tpad, d = 2, 5, 4, 32, K.D
    need = lib.em_dec_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
    assert need > 0
    kv = torch.zeros(K.LAYERS, B * T, 2 * d, device="cuda")
    vT = torch.zeros(K.LAYERS, B, d, Tpad, device="cuda")
    kl = torch.full((B,), T, dtype=torch.int32, device="cuda")
    x = torch.ones(B, Lp, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, Lp, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda w, n, lp=Lp: lib.em_dec_seq_nll(pk.dtype, C.byref(w), L.ptr(kv), L.ptr(vT), L.ptr(kl), None, L.ptr(x),  # noqa: E731
                                                  L.ptr(x), L.ptr(x), B, B, lp, T, Tpad, L.ptr(out), L.ptr(ws), n,
                                                  L.current_stream_ptr())
    assert call(pk.w, need) == L.EM_OK
    assert call(pk.w, need - 1) == L.EM_ERR_WORKSPACE
    assert call(pk.w, need, pk.w.pe_len + 1) == L.EM_ERR_BAD_ARG  # more positions than the pack's table
    # d_k = 96: refused by the workspace query, by the entry point and - before any launch - by the Python wrapper
    from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder

    wide = TransformerDecoder(20, 192, attention_heads=2, linear_units=64, num_blocks=1, compute_dtype="float32").to("cuda")
    wk = wide.packed(dev, 8)
    assert lib.em_dec_seq_nll_workspace_bytes(wk.dtype, C.byref(wk.w), B, Lp) == 0
    assert call(wk.w, need) == L.EM_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="96"):
        wide.sequence_nll(torch.zeros(B, T, 192, device="cuda"), kl, x, x, x)
    # host-side refusals of the wrapper
    dec = m.decoder
    mem = torch.zeros(B, T, d, device="cuda")
    with pytest.raises(ValueError):
        dec.sequence_nll(mem, kl, x * 300, x, x)  # token id == V
    with pytest.raises(ValueError):
        dec.sequence_nll(mem, kl * 2, x, x, x)  # hlens beyond T
    with pytest.raises(ValueError):
        dec.sequence_nll(mem, kl, x, x, x, mem_of=torch.tensor([0, 2]))
    with pytest.raises(ValueError):
        dec.sequence_nll(mem[:1], kl[:1], x, x, x)  # two transcripts, one memory, no mem_of
    with pytest.raises(L.EspnetAmdError):
        dec.sequence_nll(mem.cpu(), kl, x, x, x)
    # more sentences than a grid dimension holds: the workspace query says 0, the wrapper names the sizes
    assert lib.em_dec_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), 70000, Lp) == 0
    many = torch.ones(70000, Lp, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="70000 x 5"):
        dec.sequence_nll(mem[:1], kl[:1], many, many, many, mem_of=torch.zeros(70000, dtype=torch.int32))


# ---------------------------------------------------------------------- Speech2Text.batch_nll
@pytest.fixture(scope="module")
def s2t_case(tmp_path_factory):
    from espnet_amd.bin.asr_inference import Speech2Text
    from tests.helpers import golden_speech, golden_state_dict, load_golden

    g = load_golden("small_ragged")  # 12 x 256 Conformer, 6 x 256 decoder (4 heads), V 5 000; utterances of 3.0, 2.3 and 1.0 s
    sd = golden_state_dict(g)
    d = tmp_path_factory.mktemp("nll_model")
    (d / "config.yaml").write_text(str(g["config_yaml"]))
    torch.save(sd, d / "model.pth")
    # (greedy CTC: no search is built - scoring transcripts needs the decoder alone)
    s2t = Speech2Text(asr_train_config=str(d / "config.yaml"), asr_model_file=str(d / "model.pth"), device="cuda",
                      dtype="float32", ctc_greedy=True)
    speech, lens = golden_speech(g)
    lengths = lens.tolist()[1:]
    return g, sd, s2t, speech[1:, : max(lengths)].contiguous(), lengths


def test_speech2text_batch_nll(s2t_case):
    """Transcripts as strings and as ids, an n-best list of three candidates that share one memory: the values are those
    of three separate calls, and those of the restatement on the device's own encoder output."""
    g, sd, s2t, speech, lengths = s2t_case
    heads = g["config"]["decoder_conf"]["attention_heads"]
    V = int(g["vocab"])
    cands = [[5, 9, 11, 3], [5, 9], []]
    other = [7, 7, 30, 12, 4, 21]
    as_text = " ".join(s2t.converter.ids2tokens(other))
    assert s2t.tokenizer is not None and s2t._target_ids(as_text) == other  # (word tokens)
    res = s2t.batch_nll(speech, lengths, [cands, as_text])
    assert [len(r) for r in res] == [3, 1] and all(isinstance(v, float) for r in res for v in r)
    assert s2t.batch_nll(speech, lengths, [cands, other]) == res  # ids instead of the string: the same call
    # against the restatement on the encoder output of the same isolated encoding
    st = s2t.asr_model.encode_device(speech.cuda(), lengths, isolate=True)
    mem, hl = st.enc_act.float().cpu().double(), torch.tensor(st.olens)
    p = R.Params(sd, heads)
    rows = cands + [other]
    ys = torch.zeros(4, 6, dtype=torch.long)
    for i, y in enumerate(rows):
        ys[i, : len(y)] = torch.tensor(y, dtype=torch.long)
    ylens = torch.tensor([len(y) for y in rows])
    want, _ = R.nll(p, mem, hl, ys, ylens, V - 1, V - 1, mem_of=torch.tensor([0, 0, 0, 1]))
    got = torch.tensor(res[0] + res[1], dtype=torch.float64)
    err = (got - want.sum(1)).abs()
    print(f"\nbatch_nll f32: {got.tolist()}  per-token share of the error {float((err / (ylens + 1)).max()):.3e}")
    assert bool((err <= K.E_NLL["float32"] * (ylens + 1)).all())
    # one candidate per call (the same encoding, other batch shapes of the decoder): equal within the two calls' bounds
    for i, y in enumerate(cands):
        alone = s2t.batch_nll(speech, lengths, [[y], other])[0][0]
        assert abs(alone - res[0][i]) <= 2 * K.E_NLL["float32"] * (len(y) + 1), (i, alone, res[0][i])
    # the slices of a long candidate list give the values of the single call
    s2t.nll_rows_per_call = 2
    try:
        sliced = s2t.batch_nll(speech, lengths, [cands, other])
    finally:
        del s2t.nll_rows_per_call
    for a, b, n in zip(sliced[0] + sliced[1], res[0] + res[1], (ylens + 1).tolist()):
        assert abs(a - b) <= 2 * K.E_NLL["float32"] * n
    with pytest.raises(ValueError):
        s2t.batch_nll(speech, lengths, [cands])  # two utterances, one entry
    with pytest.raises(ValueError):
        s2t.batch_nll(speech, lengths, [[[5, V - 1]], other])  # <sos/eos> inside a transcript
