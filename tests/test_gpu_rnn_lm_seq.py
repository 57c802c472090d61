"""Whole-sentence scoring with the recurrent LM (`em_rnn_lm_seq_nll`, csrc/rnn_lm_seq.hip) through its public routes, against
the float64 restatement (tests/rnn_lm_seq_ref.py) on the weights as the device holds them.  The bound is not a constant:
every case measures the route before (`forward` + em_log_softmax_rows_f32 + gather) on the same inputs against the same
float64 values, and the new path's largest error must stay within 4 x that: both round the same quantities at the same
places and differ in summation order only.  First run: profiles/rnn_lm_seq_first_run.txt."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from tests import rnn_lm_seq_ref as R  # noqa: E402
from tests import scratch_fill as sf  # noqa: E402
from tests.lm_nll_cases import make_text  # noqa: E402

DTYPES = ["float32", "bfloat16"]
ROUND = {"float32": None, "bfloat16": torch.bfloat16}

# name: (rnn_type, nlayers, nhid, unit, tie_weights, V, B, Lp, ragged)
CASES = {
    "plain": ("lstm", 1, 64, 64, False, 40, 3, 12, True),
    "ragged": ("lstm", 2, 72, 40, False, 90, 5, 34, True),  # a partial channel group, K padding, one empty sentence
    "gru": ("gru", 2, 96, 64, False, 60, 5, 34, True),
    "deep": ("lstm", 3, 64, 64, False, 40, 2, 1, True),  # a wavefront shorter than its depth
    "tied": ("lstm", 2, 64, 64, True, 200, 3, 12, True),
    "tanh": ("rnn_tanh", 2, 72, 40, False, 50, 3, 12, True),
    "relu": ("rnn_relu", 2, 72, 40, False, 50, 3, 12, True),
    "tile2": ("lstm", 2, 64, 64, False, 40, 65, 9, True),  # a second row tile
    "default": ("lstm", 2, 650, 650, False, 120, 4, 10, False),  # the class default: 40 full groups + 10 channels, pad 704
}


def _cpu_model(name, dtype="float32"):
    """The case's model with seeded weights: matrices N(0, s^2 / fan_in), s = 1.5 in the cells (relu: 0.7), 2 in the head."""
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel

    rnn, nl, nhid, unit, tie, V = CASES[name][:6]
    model = ESPnetLanguageModel(SequentialRNNLM(V, unit=unit, nhid=nhid, nlayers=nl, tie_weights=tie, rnn_type=rnn,
                                                compute_dtype=dtype), V)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k == "lm.encoder.weight":
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / unit ** 0.5 if tie else 1.0))
            elif p.dim() == 2:
                s = 2.0 if "decoder" in k else 0.7 if rnn == "rnn_relu" else 1.5  # (a relu cell has no bound of its own)
                p.copy_(torch.randn(p.shape, generator=g) * (s / p.shape[1] ** 0.5))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model.lm.invalidate()
    return model.eval()


@functools.lru_cache(maxsize=None)
def _model(name, dtype):
    return _cpu_model(name, dtype).to("cuda")


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(text, lens, float64 nll, x_lengths), computed once: make_text's triples side by side; `ragged` keeps their lengths
    (from five sentences on the second is emptied), otherwise every sentence is full."""
    rnn, V, B, Lp, ragged = CASES[name][0], *CASES[name][5:]
    parts = [make_text(Lp, V, seed=300 + i) for i in range((B + 2) // 3)]
    text, lens = torch.cat([p[0] for p in parts])[:B], torch.cat([p[1] for p in parts])[:B]
    if not ragged:
        lens = torch.full_like(lens, Lp - 1)
    elif B >= 5:
        lens[1] = 0
    sd = {k[3:]: v for k, v in _cpu_model(name).state_dict().items()}
    want, xl = R.nll(R.LmParams(sd, rnn, round_to=ROUND[dtype]), text, lens)
    return text, lens, want, xl


def _route_before(model, text, lens):
    """ESPnetLanguageModel.nll before `sequence_nll`: `forward` (64 rows a call, its limit), row log-softmax, gather."""
    x, t, _, scored = model._masked_pair(text, lens)
    logits = torch.cat([model.lm(x[i:i + 64], None)[0] for i in range(0, x.size(0), 64)])
    B, Lp, V = logits.shape
    rows = logits.reshape(B * Lp, V)
    L.check(L.load().em_log_softmax_rows_f32(L.ptr(rows), B * Lp, V, L.current_stream_ptr()), "em_log_softmax_rows_f32")
    nll = -rows.gather(1, t.reshape(-1, 1).long()).reshape(B, Lp)
    return torch.where(scored, nll, torch.zeros_like(nll))


def _pair(name, dtype):
    """(model, x, target with -1 where nothing is scored, x_lengths, scored) on the device."""
    text, lens, _, _ = _case(name, dtype)
    m = _model(name, dtype)
    x, t, xl, scored = m._masked_pair(text.cuda(), lens.cuda())
    return m, x, torch.where(scored, t, torch.full_like(t, -1)), xl, scored


@functools.lru_cache(maxsize=None)
def _bound(name, dtype):
    text, lens, want, _ = _case(name, dtype)
    old = float((_route_before(_model(name, dtype), text.cuda(), lens.cuda()).cpu().double() - want).abs().max())
    return 4 * old, old


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_nll_against_float64(name, dtype):
    text, lens, want, xl = _case(name, dtype)
    m, x, tm, x_lengths, scored = _pair(name, dtype)
    got, gxl = m.nll(text.cuda(), lens.cuda())
    assert torch.equal(m.lm.sequence_nll(x, tm, x_lengths), got) and torch.equal(gxl.cpu(), xl) and got.shape == want.shape
    got = got.cpu().double()
    assert (got[~scored.cpu()] == 0).all()  # exactly
    bound, old = _bound(name, dtype)
    err = float((got - want).abs().max())
    print(f"\nrnn seq nll {name} {dtype}: err {err:.3e}  route before {old:.3e}  (largest nll {float(want.max()):.2f})")
    assert err <= bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_depend_on_their_own_past_only(dtype):
    """Other tokens in the other sentences and behind every end, same (B, Lp): the untouched sentence keeps its bits."""
    V = CASES["ragged"][5]
    m, x, tm, xl, scored = _pair("ragged", dtype)
    base = m.lm.sequence_nll(x, tm, xl)
    g = torch.Generator().manual_seed(9)
    for keep in (0, 2):
        noise = torch.randint(0, V, x.shape, generator=g).cuda()
        own = scored.clone()
        own[torch.arange(x.size(0), device="cuda") != keep] = False
        x2 = torch.where(own, x, noise)
        t2 = torch.where(own | ~scored, tm, noise)
        got = m.lm.sequence_nll(x2, t2, xl)
        assert torch.equal(got[keep], base[keep]) and not torch.equal(got, base)


def test_c_abi_checks():
    from tests.lm_nll_cases import build_model

    dtype = "bfloat16"
    m, x, tm, xl, _ = _pair("ragged", dtype)
    xi, ti = x.to(torch.int32).contiguous(), tm.to(torch.int32).contiguous()
    B, Lp = xi.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    pk = m.lm.packed(dev)
    lib = L.load()
    need = lib.em_rnn_lm_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(w, lens_i, n=need, fill=0x00):
        sf.fill_bytes(ws, fill)
        out = torch.full((B, Lp), 7.0, device="cuda")
        rc = lib.em_rnn_lm_seq_nll(pk.dtype, C.byref(w), L.ptr(xi), L.ptr(ti), L.ptr(lens_i), B, Lp, L.ptr(out), L.ptr(ws), n,
                                   L.current_stream_ptr())
        return rc, out

    tk = build_model("h2", dtype).to("cuda").lm.packed(dev, Lp + 1)
    rc, out = call(tk.w, None)
    assert rc == L.EM_ERR_BAD_ARG and (out == 7.0).all()  # nothing was launched
    assert lib.em_rnn_lm_seq_nll_workspace_bytes(tk.dtype, C.byref(tk.w), B, Lp) == 0
    assert call(pk.w, None, need - 1)[0] == L.EM_ERR_WORKSPACE
    li = xl.to(torch.int32)
    (rc0, a), (rc1, b) = call(pk.w, li, fill=0x00), call(pk.w, li, fill=0xFF)
    assert rc0 == rc1 == L.EM_OK and sf.bytes_equal(a, b) and torch.isfinite(a).all()
    # without lengths: every sentence Lp long, the targets as they are
    full = torch.full((B,), Lp, dtype=torch.int32, device="cuda")
    (_, c), (_, d) = call(pk.w, None), call(pk.w, full, fill=0xFF)
    assert sf.bytes_equal(c, d) and sf.bytes_equal(c, a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_routes(tmp_path, dtype):
    """batchify_nll in slices of 2 against nll whole, and the perplexity tool on a seq_rnn config: both within the case's
    bound per token (so is a mean of nll; |ppl - want| <= want * (exp(bound) - 1))."""
    import yaml

    from espnet_amd.bin.lm_calc_perplexity import calc_perplexity

    name = "ragged"
    rnn, nl, nhid, unit, tie, V = CASES[name][:6]
    text, lens, want, xl = _case(name, dtype)
    bound, _ = _bound(name, dtype)
    m = _model(name, dtype)
    whole, xl1 = m.nll(text.cuda(), lens.cuda())
    parts, xl2 = m.batchify_nll(text.cuda(), lens.cuda(), batch_size=2)
    assert parts.shape == whole.shape and torch.equal(xl1, xl2) and torch.equal(xl1.cpu(), xl)
    errs = [float((v.cpu().double() - want).abs().max()) for v in (whole, parts)]
    print(f"\nbatchify {dtype}: whole {errs[0]:.3e} slices of 2 {errs[1]:.3e} same bits {torch.equal(whole, parts)}")
    assert max(errs) <= bound
    torch.save(_cpu_model(name).state_dict(), tmp_path / "lm.pth")
    conf = dict(lm="seq_rnn", token_list=[f"t{i}" for i in range(V)],
                lm_conf=dict(unit=unit, nhid=nhid, nlayers=nl, rnn_type=rnn, tie_weights=tie))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    rows = [i for i in range(text.size(0)) if int(lens[i]) > 0]  # (a line of the text file holds at least one token)
    (tmp_path / "text").write_text("".join(f"utt{i} {' '.join(map(str, text[i, : int(lens[i])].tolist()))}\n" for i in rows))
    want_ppl = math.exp(float(want[rows].sum()) / int(xl[rows].sum()))
    calc_perplexity(str(tmp_path / "out"), 2, dtype, 1, 0, 1, "INFO", [(str(tmp_path / "text"), "text", "text_int")], None,
                    str(tmp_path / "config.yaml"), str(tmp_path / "lm.pth"), None, False)
    got = float((tmp_path / "out" / "ppl").read_text())
    print(f"ppl seq_rnn {dtype}: {got:.6f} (float64 {want_ppl:.6f})")
    assert abs(got - want_ppl) <= want_ppl * (math.exp(bound) - 1)
