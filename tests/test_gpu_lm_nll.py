"""Whole-sentence scoring with the language model on the device (csrc/lm_seq.hip, the head: csrc/vocab_head.hip): the two kernels alone, the chain
`em_lm_seq_nll` through TransformerLM.sequence_nll / ESPnetLanguageModel.nll / batchify_nll, the recurrent LM's route and
the perplexity tool, against the float64 restatement (tests/lm_seq_ref.py) on the weights as the device holds them.

Bounds (tests/lm_nll_cases.py) are 4 x the largest error of the first run (profiles/lm_nll_first_run.txt); every test
prints what it measured.  tests/test_cpu_lm_nll.py::test_defects_are_visible shows that a wrong causal mask, a missing
id-0 mask and a wrong position each move some nll by more than four times these bounds."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from tests import lm_nll_cases as K  # noqa: E402
from tests import lm_seq_ref as R  # noqa: E402

DTYPES = ["float32", "bfloat16"]
ACT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
ROUND = {"float32": None, "bfloat16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _model(name, dtype):
    return K.build_model(name, dtype).to("cuda")


@functools.lru_cache(maxsize=None)
def _params(name, dtype):
    V, heads, pos_enc, _ = K.MODELS[name]
    return R.Params(K.build_model(name).state_dict(), heads, pos_enc is not None, round_to=ROUND[dtype])


@functools.lru_cache(maxsize=None)
def _want(name, dtype, Lp):
    """(text, lens, float64 nll, x_lengths) of the shared sentences of width Lp: computed once, never changed."""
    text, lens = K.make_text(Lp, K.MODELS[name][0])
    nll, xl = R.nll(_params(name, dtype), text, lens)
    return text, lens, nll, xl


# ---------------------------------------------------------------------- em_lm_causal_attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("Lp", K.WIDTHS)
def test_causal_attention(Lp, heads, dtype):
    """B = 3 ragged sentences (tokens 0 behind the end, one id 0 in the middle of the first), random q | k | v: every row,
    the rows behind a sentence's end included, against the restatement on the same rounded operands."""
    B, d = 3, K.ATT
    g = torch.Generator().manual_seed(7 * Lp + heads)
    qkv = torch.randn(B * Lp, 3 * d, generator=g)
    qkv[:, : 2 * d] *= 1.5  # scores a few units apart
    qkv = qkv.to(ACT[dtype])
    lens = [Lp, max(Lp // 2, 1), max(Lp - 3, 1)]
    x = torch.randint(1, 50, (B, Lp), generator=g, dtype=torch.int32)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    if Lp >= 3:
        x[0, Lp // 2] = 0
    q64 = qkv.to(torch.float64).view(B, Lp, 3 * d)
    want = R.attention(q64[..., :d], q64[..., d : 2 * d], q64[..., 2 * d :], x.long(), heads)
    ctx = torch.full((B * Lp, d), float("nan"), dtype=ACT[dtype], device="cuda")
    qkv_d, x_d = qkv.cuda(), x.cuda()
    L.check(L.load().em_lm_causal_attention(L.DTYPES[dtype], L.ptr(qkv_d), L.ptr(x_d), B, Lp, d, heads, L.ptr(ctx),
                                            L.current_stream_ptr()), "em_lm_causal_attention")
    got = ctx.cpu().to(torch.float64).view(B, Lp, d)
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"\nattention Lp {Lp} heads {heads} {dtype}: err {err:.3e}")
    assert err <= K.E_ATT[dtype]


def test_causal_attention_refuses_other_head_widths():
    z = torch.zeros(4, 3 * 96, device="cuda")
    x = torch.ones(1, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        L.check(L.load().em_lm_causal_attention(L.EM_F32, L.ptr(z), L.ptr(x), 1, 4, 96, 2, L.ptr(z), L.current_stream_ptr()))


# ---------------------------------------------------------------------- em_lm_head_nll
def _head_case(M, V, d=128):
    g = torch.Generator().manual_seed(1000 * M + V)
    xr = torch.randn(M, d, generator=g) * 3 + 0.5
    gn, bn = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w = torch.randn(V, d, generator=g) * (2.0 / d ** 0.5)
    bias = 0.5 * torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    tgt[0] = V - 1
    peaked = torch.zeros(M, dtype=torch.bool)
    if M >= 8:
        tgt[1], tgt[2], tgt[M - 1] = 0, -1, -1
        # rows 3 and 4 are one row whose logit of column c is 40 above the rest: scored at c (nll ~ 0) and elsewhere (~ 40)
        c = V // 2
        xr[4] = xr[3]
        xn = torch.nn.functional.layer_norm(xr[3], (d,), gn, bn, 1e-12)
        w[c] = xn * (40.0 / float(xn @ xn))
        bias[c] = 0.0
        tgt[3], tgt[4] = c, (c + 1) % V
        peaked[3] = peaked[4] = True
    return xr, gn, bn, w, bias, tgt, peaked


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,V", [(1, 50), (77, 1027), (130, 300)])
def test_head_nll(M, V, dtype):
    d = 128
    xr, gn, bn, w, bias, tgt, peaked = _head_case(M, V)
    w = w.to(ACT[dtype])
    want = R.rows_nll(xr.double(), gn.double(), bn.double(), w.double(), bias.double(), tgt.long())
    if M >= 8:
        y3 = (torch.nn.functional.layer_norm(xr[3].double(), (d,), gn.double(), bn.double(), 1e-12) @ w.double().t() + bias.double())
        top2 = y3.topk(2).values
        assert float(top2[0] - top2[1]) > 30 and int(y3.argmax()) == V // 2  # peaked indeed
    lib = L.load()
    dt = L.DTYPES[dtype]
    need = lib.em_lm_head_nll_workspace_bytes(dt, M, V)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((M,), float("nan"), device="cuda")
    dev = [t.cuda() for t in (xr, gn, bn, w, bias, tgt)]
    args = [dt] + [L.ptr(t) for t in dev] + [M, V, d, L.ptr(out), L.ptr(ws), need, L.current_stream_ptr()]
    L.check(lib.em_lm_head_nll(*args), "em_lm_head_nll")
    got = out.cpu().double()
    assert (got[tgt < 0] == 0).all()  # exactly
    err = (got - want).abs()
    e_plain = float(err[~peaked].max())
    e_peak = float(err[peaked].max()) if peaked.any() else 0.0
    print(f"\nhead M {M} V {V} {dtype}: err {e_plain:.3e}  peaked rows {e_peak:.3e} (nll {want[peaked].tolist()})")
    assert e_plain <= K.E_HEAD[dtype] and e_peak <= K.E_HEAD_PEAKED[dtype]
    if need:
        args[-2] = need - 1
        assert lib.em_lm_head_nll(*args) == L.EM_ERR_WORKSPACE


# ---------------------------------------------------------------------- the chain and the public interface
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(K.MODELS))
@pytest.mark.parametrize("Lp", K.WIDTHS)
def test_nll_against_restatement(Lp, name, dtype):
    """ESPnetLanguageModel.nll (-> TransformerLM.sequence_nll -> em_lm_seq_nll) per scored token; behind x_lengths the
    value is exactly 0.0 although the caller's padding there is random."""
    text, lens, want, xl = _want(name, dtype, Lp)
    got, gxl = _model(name, dtype).nll(text.cuda(), lens.cuda())
    got = got.cpu().double()
    assert got.shape == want.shape == (3, Lp) and torch.equal(gxl.cpu(), xl)
    scored = torch.arange(Lp).unsqueeze(0) < xl.unsqueeze(1)
    assert (got[~scored] == 0).all()
    err = float((got - want).abs().max())
    print(f"\nnll {name} Lp {Lp} {dtype}: err {err:.3e} (largest nll {float(want.max()):.2f})")
    assert err <= K.E_NLL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_depend_on_their_own_past_only(dtype):
    """Bit for bit: other tokens behind position j of a sentence's text (nll[j] scores text[j] given text[:j]), and other
    sentences beside it in a batch of the same shape, leave nll[:, : j + 1] of that sentence as it was."""
    name, Lp = "h4pe", 65
    V = K.MODELS[name][0]
    text, lens, _, _ = _want(name, dtype, Lp)
    m = _model(name, dtype)
    base, _ = m.nll(text.cuda(), lens.cuda())
    g = torch.Generator().manual_seed(5)
    for j in (0, 15, 16, 31, 40):
        t2 = text.clone()
        t2[0, j + 1:] = torch.randint(0, V - 1, (Lp - 2 - j,), generator=g)  # zeros among them
        got, _ = m.nll(t2.cuda(), lens.cuda())
        assert torch.equal(got[0, : j + 1], base[0, : j + 1]), j
        assert torch.equal(got[1:], base[1:])
    t3 = torch.randint(0, V - 1, text.shape, generator=g)
    t3[0] = text[0]
    l3 = torch.tensor([int(lens[0]), Lp - 1, 1])
    got, _ = m.nll(t3.cuda(), l3.cuda())
    assert torch.equal(got[0], base[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_batchify_nll(dtype):
    name = "h2pe"
    V = K.MODELS[name][0]
    g = torch.Generator().manual_seed(21)
    lens = torch.tensor([9, 33, 4, 20, 17])
    text = torch.randint(1, V - 1, (5, 33), generator=g)
    m = _model(name, dtype)
    whole, xl = m.batchify_nll(text.cuda(), lens.cuda(), batch_size=100)
    parts, xl2 = m.batchify_nll(text.cuda(), lens.cuda(), batch_size=2)
    assert parts.shape == whole.shape == (5, 34) and torch.equal(xl, xl2) and xl.tolist() == [10, 34, 5, 21, 18]
    want, _ = R.nll(_params(name, dtype), text, lens)
    for got in (whole, parts):
        assert float((got.cpu().double() - want).abs().max()) <= K.E_NLL[dtype]
    with pytest.raises(ValueError):
        m.nll(text.cuda(), lens.cuda(), max_length=20)


@pytest.mark.parametrize("name", ["h2pe", "h4"])
def test_agrees_with_the_step_path(name):
    """`forward` (position by position through em_lm_step) + log-softmax + gather, f32: within twice the f32 bound."""
    text, lens, _, xl = _want(name, "float32", 65)
    m = _model(name, "float32")
    got, _ = m.nll(text.cuda(), lens.cuda())
    x, t, _ = R.sentence_pair(text, lens, m.sos, m.eos)
    scored = torch.arange(x.size(1)).unsqueeze(0) < xl.unsqueeze(1)
    x = torch.where(scored, x, torch.zeros_like(x))
    logits, _ = m.lm(x.cuda(), None)
    step = -torch.log_softmax(logits.double(), -1).cpu().gather(2, t.unsqueeze(2)).squeeze(2)
    err = float(((got.cpu().double() - step) * scored).abs().max())
    print(f"\nsequence path vs step path {name} f32: {err:.3e}")
    assert err <= 2 * K.E_NLL["float32"]


def test_workspace_and_kind_checks():
    m = _model("h2", "float32")
    pk = m.lm.packed(torch.device("cuda", torch.cuda.current_device()), 8)
    lib = L.load()
    need = lib.em_lm_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), 2, 5)
    assert need > 0
    x = torch.ones(2, 5, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 5, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda w, n: lib.em_lm_seq_nll(pk.dtype, C.byref(w), L.ptr(x), L.ptr(x), 2, 5, L.ptr(out), L.ptr(ws), n,  # noqa: E731
                                          L.current_stream_ptr())
    assert call(pk.w, need) == L.EM_OK
    assert call(pk.w, need - 1) == L.EM_ERR_WORKSPACE
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    rnn = SequentialRNNLM(20, unit=64, nlayers=1, compute_dtype="float32").to("cuda")
    rk = rnn.packed(torch.device("cuda", torch.cuda.current_device()))
    assert call(rk.w, need) == L.EM_ERR_BAD_ARG
    assert lib.em_lm_seq_nll_workspace_bytes(rk.dtype, C.byref(rk.w), 2, 5) == 0


E_RNN = 3.9e-6  # f32 LSTM LM against the f32 step oracle: 4 x the first run's 9.537e-7 (profiles/lm_nll_first_run.txt)


def test_seq_rnn_lm_nll():
    """ESPnetLanguageModel.nll with a SequentialRNNLM (LSTM): through its `forward`, em_log_softmax_rows_f32 and a gather,
    against SeqRnnLMOracle fed token by token."""
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel
    from oracle.beam_search import SeqRnnLMOracle

    V = 40
    torch.manual_seed(31)
    model = ESPnetLanguageModel(SequentialRNNLM(V, unit=64, nhid=64, nlayers=2, compute_dtype="float32"), V).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    text, lens = K.make_text(12, V)
    got, xl = model.to("cuda").nll(text.cuda(), lens.cuda())
    got = got.cpu()
    x, t, _ = R.sentence_pair(text, lens, V - 1, V - 1)
    orc = SeqRnnLMOracle(sd, 2)
    err = 0.0
    for b in range(3):
        cache = orc.init_cache()
        for j in range(int(xl[b])):
            logp, cache = orc.step(x[b : b + 1, : j + 1], cache)
            err = max(err, abs(float(-logp[0, t[b, j]]) - float(got[b, j])))
        assert (got[b, int(xl[b]):] == 0).all()
    print(f"\nseq_rnn nll err {err:.3e}")
    assert xl.tolist() == (lens + 1).tolist() and err <= E_RNN


# ---------------------------------------------------------------------- the perplexity tool
@pytest.mark.parametrize("dtype", DTYPES)
def test_calc_perplexity_cli(tmp_path, dtype):
    import yaml

    from espnet_amd.bin.lm_calc_perplexity import calc_perplexity

    name = "h2pe"
    V, heads, pos_enc, _ = K.MODELS[name]
    torch.save(K.build_model(name).state_dict(), tmp_path / "lm.pth")
    conf = dict(lm="transformer", token_list=[f"t{i}" for i in range(V)],
                lm_conf=dict(pos_enc=pos_enc, embed_unit=K.EMBED, att_unit=K.ATT, head=heads, unit=K.UNIT, layer=K.LAYERS))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    g = torch.Generator().manual_seed(41)
    sents = {f"utt{i}": torch.randint(1, V - 1, (n,), generator=g).tolist() for i, n in enumerate([5, 17, 1, 33, 8, 12])}
    (tmp_path / "text").write_text("".join(f"{k} {' '.join(map(str, v))}\n" for k, v in sents.items()))
    p = _params(name, dtype)
    nll = {}
    for k, v in sents.items():
        nll[k] = float(R.nll(p, torch.tensor([v]), torch.tensor([len(v)]))[0].sum())
    ntok = {k: len(v) + 1 for k, v in sents.items()}
    E = K.E_NLL[dtype]  # per token, so of a mean too: |ppl - want| <= want * (exp(E) - 1)
    for base in (None, 2.0):
        out = tmp_path / f"out_{base}"
        calc_perplexity(str(out), 4, dtype, 1, 0, 1, "INFO", [(str(tmp_path / "text"), "text", "text_int")], None,
                        str(tmp_path / "config.yaml"), str(tmp_path / "lm.pth"), base, False)
        assert (out / "utt2ntokens").read_text() == "".join(f"{k} {ntok[k]}\n" for k in sents)
        lines = [l.split() for l in (out / "utt2ppl").read_text().splitlines()]
        assert [l[0] for l in lines] == list(sents)
        for k, v in lines:
            want = math.exp(nll[k] / ntok[k])  # log_base ** (x / ln(log_base)) = exp(x)
            assert abs(float(v) - want) <= want * (math.exp(E) - 1), (k, v, want)
        want = math.exp(sum(nll.values()) / sum(ntok.values()))
        got = float((out / "ppl").read_text())
        print(f"\nppl {dtype} log_base {base}: {got:.6f} (float64 {want:.6f})")
        assert abs(got - want) <= want * (math.exp(E) - 1)
