"""Mask-CTC decoding on the device (csrc/maskctc.hip, em_dec_full_attention in csrc/lm_seq.hip, both heads in
csrc/vocab_head.hip, the decoder pass csrc/dec_seq.hip's chain): the primitives, the
integer logic of collapse and fill, the refinement chain pass by pass, independence of the batch and of the workspace,
and MaskCTCModel / Speech2Text / the command line, against the float64 restatement (tests/maskctc_ref.py) on the weights
and inputs as the device holds them.

Bounds (tests/maskctc_cases.py) are 4 x the largest error of the first run (profiles/maskctc_first_run.txt); every test
prints what it measured.  A logit difference is known to 2 x the bound of a logit: where a float64 margin (top-1 minus
top-2 logit, |confidence - threshold|, the score gap across a selection's boundary) exceeds that, the device must have
made the float64 decision; the rest are counted as near-ties and capped (tests/maskctc_cases.py NEAR_TIE_CAP: none in
f32, one decision in ten in bf16; CHAIN_SEEDS were chosen on the CPU so that the restatement alone stays below it).
The restatement is teacher-forced: every pass starts from the y_in the device had."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from tests import maskctc_cases as K  # noqa: E402
from tests import maskctc_ref as R  # noqa: E402
from tests import scratch_fill as S  # noqa: E402

DTYPES = ["float32", "bfloat16"]
ACT = K.ACT


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


# ---------------------------------------------------------------------- em_ctc_frame_top
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [19, 33, 1027])
def test_ctc_frame_top(V, dtype):
    """150 rows (two full 64-row blocks and a partial one) against a CTC head of V labels (19, 33: no multiple of the
    16-column tile; 1027: three 512-column slices): the ids of CTC.argmax on the same input, the probabilities of the
    float64 softmax."""
    from espnet_amd.asr.ctc import CTC

    sd = K.state_dict(40 + V, V=V)
    ctc = CTC(V, K.D, compute_dtype=dtype)
    ctc.load_state_dict({"ctc_lo.weight": sd["ctc.ctc_lo.weight"], "ctc_lo.bias": sd["ctc.ctc_lo.bias"]})
    ctc.cuda()
    mem = K.memory(7, dtype, B=3, T=50)
    dev = mem.to(ACT[dtype]).cuda()
    ids, prob = ctc.frame_top_device(dev)
    assert torch.equal(ids, ctc.argmax(dev, as_int32=True))
    w, b = K.ctc_params(sd, dtype)
    lp = R.ctc_log_probs(mem.reshape(-1, K.D).to(torch.float64), w, b).numpy()
    ids64, p64 = R.ctc_frames(lp)
    err = float(np.abs(prob.cpu().numpy().reshape(-1) - p64).max())
    top2 = np.sort(lp, axis=1)
    clear = (top2[:, -1] - top2[:, -2]) > 1e-3
    print(f"\nframe top V {V} {dtype}: prob err {err:.3e}, p in [{p64.min():.3f}, {p64.max():.3f}], "
          f"{int((~clear).sum())} rows with a float64 margin <= 1e-3")
    assert np.array_equal(ids.cpu().numpy().reshape(-1)[clear], ids64[clear])
    assert err <= K.E_PROB[dtype]


# ---------------------------------------------------------------------- em_dec_full_attention
ATT_LENS = [1, 31, 32, 33, 80, 0, 17]  # the key tile is 32: one key, tile - 1, tile, tile + 1, 2.5 tiles; an empty sentence


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [2, 1])
def test_full_attention(heads, dtype):
    """Seven sentences of Lp = 80 rows, d 64; the k and v rows at and behind a sentence's length hold NaN: the rows below
    it come back finite and within the bound, the empty sentence's rows are zeros."""
    d, Lp, B = K.D, 80, len(ATT_LENS)
    g = torch.Generator().manual_seed(500 + heads)
    qkv = torch.randn(B, Lp, 3 * d, generator=g)
    qkv[..., : 2 * d] *= 1.5  # scores a few units apart
    qkv = qkv.to(ACT[dtype])
    lens = torch.tensor(ATT_LENS)
    valid = (torch.arange(Lp).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(2)
    q64 = qkv.double()
    want = R.full_attention(q64[..., :d], torch.where(valid, q64[..., d : 2 * d], 0.0), torch.where(valid, q64[..., 2 * d :], 0.0),
                            lens, heads)
    poisoned = qkv.clone()
    poisoned[..., d:] = torch.where(valid, qkv[..., d:], torch.full((), float("nan"), dtype=qkv.dtype))
    ctx = torch.full((B * Lp, d), float("nan"), dtype=ACT[dtype], device="cuda")
    q_dev, lens_dev = poisoned.reshape(B * Lp, 3 * d).cuda(), _i32(ATT_LENS)
    L.check(L.load().em_dec_full_attention(L.DTYPES[dtype], L.ptr(q_dev), L.ptr(lens_dev), B, Lp, d, heads, L.ptr(ctx),
                                           L.current_stream_ptr()), "em_dec_full_attention")
    got = ctx.cpu().double().view(B, Lp, d)
    err = 0.0
    for b, n in enumerate(ATT_LENS):
        assert torch.isfinite(got[b, :n]).all()
        err = max(err, float((got[b, :n] - want[b, :n]).abs().max()) if n else 0.0)
    assert float(got[ATT_LENS.index(0)].abs().max()) == 0.0
    print(f"\nfull attention heads {heads} {dtype}: err {err:.3e}")
    assert err <= K.E_CTX[dtype]


def test_full_attention_refuses_other_head_widths():
    z = torch.zeros(4, 3 * 192, device="cuda")
    with pytest.raises(NotImplementedError):
        L.check(L.load().em_dec_full_attention(L.EM_F32, L.ptr(z), L.ptr(_i32([1])), 1, 1, 192, 2, L.ptr(z),
                                               L.current_stream_ptr()))


# ---------------------------------------------------------------------- em_lm_head_top1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V1", [20, 34, 1030])
def test_head_top1(V1, dtype):
    """70 rows through LayerNorm and a head of V + 1 columns.  Column V1 - 3 repeats column 3 (weights and bias, raised so
    that the pair wins in a good share of the rows): an exact tie, which goes to column 3."""
    d, M = K.D, 70
    g = torch.Generator().manual_seed(600 + V1)
    x = torch.randn(M, d, generator=g) * 2.0 + 0.3
    gam, bet = 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w = torch.randn(V1, d, generator=g) * 0.4
    bias = torch.randn(V1, generator=g) * 0.5
    bias[3] += 4.0 if V1 < 100 else 9.0  # (the largest of 1 030 logits of spread 3.2 lies near 10)
    w[V1 - 3], bias[V1 - 3] = w[3], bias[3]
    w = w.to(ACT[dtype])
    y = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-12) @ w.double().t() + bias.double()
    s64, a64 = y.max(dim=1).values.numpy(), y.numpy().argmax(axis=1)
    top2 = np.sort(y.numpy(), axis=1)
    margin = np.where(a64 == 3, top2[:, -1] - top2[:, -3], top2[:, -1] - top2[:, -2])  # (the pair apart)
    lib = L.load()
    need = lib.em_lm_head_top1_workspace_bytes(L.DTYPES[dtype], M, V1)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    smax = torch.empty(M, dtype=torch.float32, device="cuda")
    amax = torch.empty(M, dtype=torch.int32, device="cuda")
    dev = [t.cuda() for t in (x, gam, bet, w, bias)]
    args = [L.DTYPES[dtype]] + [L.ptr(t) for t in dev] + [M, V1, d, L.ptr(smax), L.ptr(amax)]
    L.check(lib.em_lm_head_top1(*args, L.ptr(ws), need, L.current_stream_ptr()), "em_lm_head_top1")
    err = float(np.abs(smax.cpu().numpy() - s64).max())
    a = amax.cpu().numpy()
    print(f"\nhead top1 V+1 {V1} {dtype}: smax err {err:.3e}, {int((a64 == 3).sum())} of {M} rows won by the tied pair")
    assert (a64 == 3).sum() >= 5 and not (a == V1 - 3).any()
    clear = margin > 2 * K.E_TOP[dtype]
    assert np.array_equal(a[clear], a64[clear]) and err <= K.E_TOP[dtype]
    if need:
        assert lib.em_lm_head_top1(*args, L.ptr(ws), need - 1, L.current_stream_ptr()) == L.EM_ERR_WORKSPACE


# ---------------------------------------------------------------------- collapse and fill: integer logic, exact
def _fill_numpy(y, s, a, M0, Kp, p, mask_token):
    y = y.copy()
    n_iter = Kp if M0 >= Kp else M0
    if M0 <= 0 or p >= n_iter:
        return y
    pos = np.flatnonzero(y == mask_token)
    if p < n_iter - 1:
        pos = np.array(sorted(pos, key=lambda j: (-s[j], j))[: M0 // n_iter], dtype=np.int64)
    y[pos] = a[pos]
    return y


@pytest.mark.parametrize("Lcap", [300, 40])
def test_collapse_exact(Lcap):
    """B = 5 ragged utterances of up to 300 frames (runs cross the kernel's 256-frame chunk), one all blank, one without a
    masked token; ids with runs, f32 probabilities: tokens, confidences, y_in, counts and everything behind them equal
    the restatement on the same f32 numbers exactly.  Lcap 40 clips the token sequences."""
    B, T, V, mask_token, thres = 5, 300, 6, 6, 0.5
    g = torch.Generator().manual_seed(71)
    ids = torch.randint(0, V, (B, T), generator=g).repeat_interleave(3, dim=1)[:, :T].contiguous()
    ids[:, 250:262] = 4  # one run across the chunk boundary
    prob = torch.rand(B, T, generator=g)
    ids[3] = 0
    ids[4, :3] = 2  # (its one valid frame is a label)
    prob[4] = 0.5 + 0.5 * torch.rand(T, generator=g)  # nothing below the threshold
    olens = [300, 157, 256, 300, 1]
    out = [torch.full((B, Lcap), 77, dtype=torch.int32, device="cuda"), torch.full((B, Lcap), 7.0, device="cuda"),
           torch.full((B, Lcap), 77, dtype=torch.int32, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"),
           torch.full((B,), 77, dtype=torch.int32, device="cuda")]
    dev = [ids.to(torch.int32).cuda(), prob.cuda(), _i32(olens)]
    L.check(L.load().em_maskctc_collapse(*[L.ptr(t) for t in dev], B, T, Lcap, 0, mask_token, thres, *[L.ptr(t) for t in out],
                                         L.current_stream_ptr()), "em_maskctc_collapse")
    tokens, conf, y_in, ylens, nmask = (t.cpu().numpy() for t in out)
    for b, n in enumerate(olens):
        tk, cf = R.collapse(ids[b, :n].numpy(), prob[b, :n].numpy())
        tk, cf = tk[:Lcap], np.asarray(cf[:Lcap], dtype=np.float32)
        yi = [mask_token if c < np.float32(thres) else t for t, c in zip(tk, cf)]
        Lb = len(tk)
        assert ylens[b] == Lb and nmask[b] == sum(1 for v in yi if v == mask_token)
        assert tokens[b, :Lb].tolist() == tk and y_in[b, :Lb].tolist() == yi and np.array_equal(conf[b, :Lb], cf)
        assert (tokens[b, Lb:] == -1).all() and (y_in[b, Lb:] == -1).all() and (conf[b, Lb:] == 0.0).all()
    assert ylens[3] == 0 and nmask[4] == 0 and ylens[4] == 1
    print(f"\ncollapse Lcap {Lcap}: lengths {ylens.tolist()} masked {nmask.tolist()}")


@pytest.mark.parametrize("Kp", [1, 3, 10])
def test_fill_exact(Kp):
    """B = 5 sentences of Lp = 300 positions (more than one round of the workgroup's 256 threads), scores on a grid of 0.5
    (many exact ties), predictions that include <mask>; one sentence without a mask: Kp passes on fresh scores each equal
    the restatement on the same numbers exactly."""
    B, Lp, mask_token = 5, 300, 9
    g = torch.Generator().manual_seed(80 + Kp)
    y = torch.randint(0, 9, (B, Lp), generator=g)
    y[torch.rand(B, Lp, generator=g) < 0.4] = mask_token
    y[2][y[2] == mask_token] = 1
    y[0, 200:] = -1
    y[4, 5:] = -1
    M0 = (y == mask_token).sum(dim=1)
    y_dev, want = y.to(torch.int32).cuda(), y.numpy().copy()
    for p in range(Kp):
        s = torch.round(torch.randn(B, Lp, generator=g) * 4) / 2
        a = torch.randint(0, 10, (B, Lp), generator=g)
        tr = torch.full((B, Lp), 77, dtype=torch.int32, device="cuda")
        dev = [s.cuda(), a.to(torch.int32).cuda(), _i32(M0)]
        L.check(L.load().em_maskctc_fill(L.ptr(y_dev), *[L.ptr(t) for t in dev], B, Lp, Kp, p, mask_token, L.ptr(tr),
                                         L.current_stream_ptr()), "em_maskctc_fill")
        for b in range(B):
            want[b] = _fill_numpy(want[b], s[b].numpy(), a[b].numpy(), int(M0[b]), Kp, p, mask_token)
        assert np.array_equal(y_dev.cpu().numpy(), want) and np.array_equal(tr.cpu().numpy(), want), p
    left = (want == mask_token).sum(axis=1)
    print(f"\nfill K {Kp}: masked at first {M0.tolist()}, left (predicted as <mask>) {left.tolist()}")
    assert (want[2] == y[2].numpy()).all()
    assert L.load().em_maskctc_fill(L.ptr(y_dev), L.ptr(y_dev), L.ptr(y_dev), L.ptr(y_dev), B, Lp, 0, 0, mask_token, None,
                                    L.current_stream_ptr()) == L.EM_ERR_BAD_ARG  # K < 1


# ---------------------------------------------------------------------- the chain
@functools.lru_cache(maxsize=None)
def _chain(dtype):
    """The chain case decoded once on the device, with its trace (shared, never changed)."""
    sd, mem, ctc, p_thres, share = K.chain_case(dtype)
    model = K.build_model(sd, dtype).cuda()
    dev = mem.cuda()
    olens = _i32(K.OLENS)
    ids, prob = model.ctc.frame_top_device(dev)
    y, ylens, tokens, conf, tr = model._decode_maskctc(dev, olens, K.K, p_thres, trace=True)
    torch.cuda.synchronize()
    host = dict(ids=ids.cpu().numpy(), prob=prob.cpu().numpy(), y=y.cpu().numpy(), ylens=ylens.cpu().numpy(),
                tokens=tokens.cpu().numpy(), conf=conf.cpu().numpy(), tr=[t.cpu().numpy() for t in tr])
    return sd, mem, ctc, p_thres, share, model, host


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_teacher_forced(dtype):
    """em_ctc_frame_top, em_maskctc_collapse and em_maskctc_refine on the chain case (tests/maskctc_cases.py: B = 4 ragged,
    T 40, d 64, 2 blocks, V 19, K = 3): collapse and fill exactly as the restatement on the device's own numbers; every
    threshold, arg-max and selection as the float64 restatement on the device's y_in wherever its margin is clear."""
    sd, mem, ctc, p_thres, share, model, h = _chain(dtype)
    assert 0.25 <= share <= 0.75
    mask_token, B = K.V, len(K.OLENS)
    y0, yt, st, at = h["tr"]
    Lp = y0.shape[1]
    e_p, e_s = K.E_PROB[dtype], K.E_CHAIN[dtype]
    n_dec = near = 0
    err_p = err_s = 0.0
    M0 = []
    for b, n in enumerate(K.OLENS):
        ids64, p64 = ctc[b][0], ctc[b][1]
        assert np.array_equal(h["ids"][b, :n], ids64)  # (CHAIN_SEEDS: no frame of the restatement is a near-tie)
        tk, cf = R.collapse(h["ids"][b, :n], h["prob"][b, :n])  # integer logic on the device's own numbers: exact
        Lb = len(tk)
        yi = [mask_token if c < np.float32(p_thres) else t for t, c in zip(tk, cf)]
        assert h["ylens"][b] == Lb and h["tokens"][b, :Lb].tolist() == tk and y0[b, :Lb].tolist() == yi
        assert np.array_equal(h["conf"][b, :Lb], np.asarray(cf, dtype=np.float32)) and (y0[b, Lb:] == -1).all()
        M0.append(sum(1 for v in yi if v == mask_token))
        c64 = np.asarray(ctc[b][3])
        assert tk == ctc[b][2]
        err_p = max(err_p, float(np.abs(h["conf"][b, :Lb] - c64).max()) if Lb else 0.0)
        for j in range(Lb):
            n_dec += 1
            if abs(c64[j] - p_thres) > 2 * e_p:
                assert (yi[j] == mask_token) == (c64[j] < p_thres), (b, j)
            else:
                near += 1
    p = R.Params(sd, K.HEADS, round_to=K.ROUND[dtype])
    m64, hl, yl = mem.to(torch.float64), torch.tensor(K.OLENS), torch.tensor(h["ylens"].astype(np.int64))
    for ps in range(K.K):
        before = y0 if ps == 0 else yt[ps - 1]
        logits = R.mlm_forward(p, m64, hl, torch.tensor(before.astype(np.int64)), yl).numpy()
        for b in range(B):
            Lb = int(h["ylens"][b])
            r = R.pass_step(before[b, :Lb].tolist(), logits[b, :Lb], mask_token, M0[b], K.K, ps)
            want = _fill_numpy(before[b], st[ps][b], at[ps][b], M0[b], K.K, ps, mask_token)
            assert np.array_equal(yt[ps][b], want), (ps, b)  # the fill on the device's own scores: exact
            if r["mode"] == "idle":
                continue
            taken_dev = sorted(set(r["pos"]) - set(np.flatnonzero(_fill_numpy(before[b], st[ps][b], np.full(Lp, -7), M0[b], K.K,
                                                                              ps, mask_token) == mask_token).tolist()))
            for i, j in enumerate(r["pos"]):
                n_dec += 1
                err_s = max(err_s, abs(float(st[ps][b, j]) - r["s"][i]))
                if r["margin"][i] > 2 * e_s:
                    assert at[ps][b, j] == r["a"][i], (ps, b, j)
                else:
                    near += 1
            if r["mode"] == "partial":
                n_dec += 1
                if r["sel_gap"] > 2 * e_s:
                    assert taken_dev == r["taken"], (ps, b)
                else:
                    near += 1
    print(f"\nchain {dtype}: p_thres {p_thres:.4f} masked share {share:.2f} lengths {h['ylens'].tolist()} masked {M0}; "
          f"conf err {err_p:.3e}, score err {err_s:.3e}; {n_dec} decisions, {near} near-ties skipped")
    assert err_p <= e_p and err_s <= e_s
    assert near <= K.NEAR_TIE_CAP[dtype] * n_dec


@pytest.mark.parametrize("dtype", DTYPES)
def test_utterances_do_not_depend_on_their_batch(dtype):
    sd, mem, ctc, p_thres, share, model, h = _chain(dtype)
    for b, n in enumerate(K.OLENS):
        y, ylens, tokens, conf = model._decode_maskctc(mem[b : b + 1, :n].cuda(), _i32([n]), K.K, p_thres)
        Lb = int(h["ylens"][b])
        assert int(ylens[0]) == Lb and y.cpu().numpy()[0, :Lb].tolist() == h["y"][b, :Lb].tolist()
        assert np.array_equal(conf.cpu().numpy()[0, :Lb], h["conf"][b, :Lb])


@pytest.mark.parametrize("dtype", DTYPES)
def test_refine_does_not_depend_on_its_workspace(dtype):
    """em_maskctc_refine under the fills of tests/scratch_fill.py, and after a larger batch of other tokens ran in the same
    workspace: y_in and the traces bit for bit."""
    sd, mem, ctc, p_thres, share, model, h = _chain(dtype)
    dec, dev, olens = model.decoder, mem.cuda(), _i32(K.OLENS)
    y0 = torch.as_tensor(h["tr"][0]).cuda()
    B, Lp = y0.shape
    ylens, nmask = _i32(h["ylens"]), _i32((h["tr"][0] == K.V).sum(axis=1))
    big = torch.full((B + 2, Lp + 9), K.V, dtype=torch.int32, device="cuda")
    pk = dec.packed(dev.device, Lp + 9)
    need = L.load().em_maskctc_refine_workspace_bytes(pk.dtype, C.byref(pk.w), B + 2, Lp + 9)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y = y0.clone()
    outs = [y] + [torch.empty(K.K, B, Lp, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.int32)]

    def call():
        y.copy_(y0)
        tr = dec.refine_device(dev, olens, y, ylens, nmask, K.K, trace=True, ws=ws)
        for o, t in zip(outs[1:], tr):
            o.copy_(t)

    def stale():
        mem2 = torch.randn(B + 2, K.T, K.D, generator=torch.Generator().manual_seed(9)).cuda()
        dec.refine_device(mem2, _i32([K.T] * (B + 2)), big.clone(), _i32([Lp + 9] * (B + 2)), _i32([Lp + 9] * (B + 2)), K.K, ws=ws)

    ref = S.assert_scratch_independent(call, ws, outs, stale=stale, names=["y_in", "y_trace", "s_trace", "a_trace"])
    assert np.array_equal(ref[0].numpy(), h["y"])


# ---------------------------------------------------------------------- limits
def test_workspace_one_byte_short_and_unsupported_heads():
    sd, mem, ctc, p_thres, share, model, h = _chain("float32")
    dec, lib = model.decoder, L.load()
    y = torch.as_tensor(h["tr"][0]).cuda()
    B, Lp = y.shape
    pk = dec.packed(y.device, Lp)
    need = lib.em_maskctc_refine_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    args = [pk.dtype, C.byref(pk.w), L.ptr(ws), L.ptr(ws), L.ptr(z), L.ptr(y), L.ptr(z), L.ptr(z), B, Lp, K.T, 64, K.K, K.V, None,
            None, None, L.ptr(ws)]
    assert need > 0 and lib.em_maskctc_refine(*args, need - 1, L.current_stream_ptr()) == L.EM_ERR_WORKSPACE
    from espnet_amd.asr.decoder.mlm_decoder import MLMDecoder

    wide = MLMDecoder(K.V, 192, attention_heads=2, linear_units=64, num_blocks=1, compute_dtype="float32").cuda()
    pw = wide.packed(y.device, Lp)
    assert lib.em_maskctc_refine_workspace_bytes(pw.dtype, C.byref(pw.w), B, Lp) == 0
    args[1] = C.byref(pw.w)
    assert lib.em_maskctc_refine(*args, need, L.current_stream_ptr()) == L.EM_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="heads of 96"):
        wide.refine_device(torch.zeros(B, K.T, 192, device="cuda"), z[:B], y, z[:B], z[:B], K.K)
    with pytest.raises(NotImplementedError, match="heads of 96"):
        wide(torch.zeros(B, K.T, 192, device="cuda"), z[:B], y, z[:B])


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_and_a_sentence_longer_than_the_positional_table(dtype):
    """MLMDecoder.forward against the restatement, and one sentence of 1 030 masked tokens - more than the 1 024 rows a
    pack's positional table starts with - refined in one pass (K = 1): the pack grows its table, as for sequence_nll."""
    sd, mem, ctc, p_thres, share, model, h = _chain(dtype)
    dec = model.decoder
    p = R.Params(sd, K.HEADS, round_to=K.ROUND[dtype])
    y0 = torch.as_tensor(h["tr"][0].astype(np.int64))
    yl = torch.as_tensor(h["ylens"].astype(np.int64))
    got, _ = dec(mem.cuda(), torch.tensor(K.OLENS), y0.clamp(min=0), yl)
    want = R.mlm_forward(p, mem.double(), torch.tensor(K.OLENS), y0, yl)
    err = max(float((got[b, :n].cpu().double() - want[b, :n]).abs().max()) for b, n in enumerate(yl.tolist()) if n)
    print(f"\nforward {dtype}: logits err {err:.3e}")
    assert err <= K.E_FWD[dtype]
    Lp = 1030
    y = torch.full((1, Lp), K.V, dtype=torch.int32, device="cuda")
    tr = dec.refine_device(mem[:1].cuda(), _i32([K.T]), y, _i32([Lp]), _i32([Lp]), 1, trace=True)
    assert dec.packed(y.device).pe_len >= Lp
    logits = R.mlm_forward(p, mem[:1].double(), torch.tensor([K.T]), torch.full((1, Lp), K.V), torch.tensor([Lp]))[0].numpy()
    r = R.pass_step([K.V] * Lp, logits, K.V, Lp, 1, 0)
    clear = np.asarray(r["margin"]) > 2 * K.E_LONG[dtype]
    err = float(np.abs(tr[1][0, 0].cpu().numpy() - np.asarray(r["s"])).max())
    print(f"long sentence {dtype}: score err {err:.3e}, {int((~clear).sum())} of {Lp} near-ties")
    assert r["mode"] == "final" and err <= K.E_LONG[dtype]
    assert np.array_equal(y.cpu().numpy()[0][clear], np.asarray(r["a"])[clear])
    assert np.array_equal(y.cpu().numpy()[0], tr[2][0, 0].cpu().numpy())  # K = 1: every position takes its arg-max


# ---------------------------------------------------------------------- through the public interface, peaked
PEAK_V, PEAK_SCALE, PEAK_SEED, PEAK_LENS = 30, 40.0, 51, [5000, 3000, 4000]
# first waveform seed of the three utterances: of the sets 555, 558, 561 .. the one whose restatement (on the device's
# encoder output, K = 10 and K = 1) has the widest smallest margin - profiles/maskctc_first_run.txt lists them
PEAK_WAVES = {"float32": 579, "bfloat16": 555}


def _peaked_config():
    from oracle.weights import token_list

    return dict(token_list=token_list(PEAK_V), frontend="default", frontend_conf=dict(n_fft=512, hop_length=160, win_length=400),
                normalize="utterance_mvn", normalize_conf={}, encoder="conformer",
                encoder_conf=dict(output_size=K.D, attention_heads=1, linear_units=128, num_blocks=1, macaron_style=True,
                                  cnn_module_kernel=15),
                decoder="mlm", decoder_conf=dict(attention_heads=2, linear_units=128, num_blocks=1),
                model="maskctc", model_conf=dict(ctc_weight=0.3))


@functools.lru_cache(maxsize=None)
def _peaked_state():
    """Recipe weights (seed 51) with both output layers x 40: margins of several units (tests/test_gpu_transducer.py)."""
    from espnet_amd.tasks.asr import ASRTask
    from oracle.weights import recipe_state_dict

    sd = ASRTask.build_model(_peaked_config()).state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, PEAK_SEED)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    new["decoder.output_layer.weight"] *= PEAK_SCALE
    new["ctc.ctc_lo.weight"] *= K.CTC_SCALE  # (x 40 would put every confidence at 1.0: nothing to mask)
    return new


def _speech2text(tmp_path, dtype, **kw):
    import yaml

    from espnet_amd.bin.asr_inference_maskctc import Speech2Text

    (tmp_path / "config.yaml").write_text(yaml.safe_dump(_peaked_config()))
    torch.save(_peaked_state(), tmp_path / "model.pth")
    return Speech2Text(str(tmp_path / "config.yaml"), str(tmp_path / "model.pth"), device="cuda", dtype=dtype, **kw)


def _waves(lens, first):
    from oracle.weights import synth_waveform

    speech = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        speech[b, :n] = synth_waveform(first + b, n)
    return torch.round(speech * 32768.0).clamp(-32768, 32767) / 32768.0  # (exactly what a 16-bit wav file holds)


def peaked_case(s2t, dtype, first):
    """The utterances of waveform seeds first, first + 1, first + 2 encoded on the device and restated: (speech, st, ctc,
    p_thres, masked share, half the threshold's gap, {(K, p_thres): restatement}, the smallest margin of all of them)."""
    sd = _peaked_state()
    speech = _waves(PEAK_LENS, first)
    st = s2t.asr_model.encode_device(speech.cuda(), PEAK_LENS, isolate=True)
    mem = st.enc_act.float().cpu()
    ctc = K.restate_ctc(sd, mem, st.olens, dtype)
    p_thres, share, half_gap = K.widest_gap_threshold([c for r in ctc for c in r[3]])
    want = {(Kp, th): K.restate_decode(sd, mem, st.olens, dtype, th, Kp, ctc=ctc) for Kp, th in ((10, p_thres), (1, p_thres), (10, 0.0))}
    margins = [m for w in want.values() for _, tr in w for r in tr
               for m in r["margin"] + ([r["sel_gap"]] if r["mode"] == "partial" else [])]
    return speech, st, ctc, p_thres, share, half_gap, want, min(margins) if margins else float("inf")


@pytest.mark.parametrize("dtype", DTYPES)
def test_peaked_end_to_end(tmp_path, dtype):
    """Speech2Text on a tiny Conformer Mask-CTC model: `batch_decode`, `__call__` and the command line give the token lists
    of the restatement on the device's own encoder output, with K = 10, K = 1 (one pass fills everything) and p_thres 0
    (the greedy CTC tokens).  The threshold lies in the widest gap of the restatement's confidences."""
    s2t = _speech2text(tmp_path, dtype)
    model = s2t.asr_model
    assert model.mask_token == PEAK_V and s2t.converter.ids2tokens([PEAK_V]) == ["<mask>"]
    speech, st, ctc, p_thres, share, half_gap, wants, margin = peaked_case(s2t, dtype, PEAK_WAVES[dtype])
    ids, prob = model.ctc.frame_top_device(st.enc_act)
    err_p = max(float(np.abs(prob[b, :n].cpu().numpy() - ctc[b][1]).max()) for b, n in enumerate(st.olens))
    # the scores of the masked positions, pass by pass (the device's passes start from the restatement's y_in as long as
    # the decisions agree, which the token lists below show)
    tr = model.decode_maskctc_device(st, 10, p_thres, trace=True)[4]
    err_s = max([abs(float(tr[2][ps, b, j]) - s) for b, (_, t) in enumerate(wants[(10, p_thres)])
                 for ps, r in enumerate(t) for j, s in zip(r["pos"], r["s"])] + [0.0])
    masked = sum(sum(1 for c in r[3] if c < p_thres) for r in ctc)
    print(f"\nend to end {dtype}: waves {PEAK_WAVES[dtype]}, p_thres {p_thres:.4f}, lengths {[len(r[2]) for r in ctc]}, masked "
          f"{masked}, smallest margin {margin:.3f}, half gap {half_gap:.3g}, prob err {err_p:.3e}, score err {err_s:.3e}")
    # peaked indeed: every decision of the restatement lies above twice the bounds
    assert half_gap > 2 * K.E_PEAK_PROB[dtype] and margin > 2 * K.E_PEAK[dtype] and 0.25 <= share <= 0.75
    assert err_p <= K.E_PEAK_PROB[dtype] and err_s <= K.E_PEAK[dtype]
    results = {}
    for (Kp, thres), want in wants.items():
        s2t.s2t.n_iterations, s2t.s2t.threshold_probability = Kp, thres
        res = s2t.batch_decode(speech, PEAK_LENS)
        for b, (yseq, t) in enumerate(want):
            text, token, token_int, hyp = res[b][0]
            assert hyp.yseq.tolist() == yseq and token_int == R.token_int(yseq) and len(token) == len(token_int)
            if thres == 0.0:
                assert yseq[1:-1] == ctc[b][2] and t == []
            if Kp == 1:
                assert [r["mode"] for r in t] in ([], ["final"])
        alone = s2t(speech[1, : PEAK_LENS[1]].numpy())
        assert alone[0][2] == res[1][0][2]
        results[(Kp, thres)] = [r[0][2] for r in res]
    # the command line on the same utterances as 16-bit wav files
    from espnet_amd.bin.asr_inference_maskctc import main
    from espnet_amd.fileio.sound_scp import write_wav_pcm16

    lines = []
    for b, n in enumerate(PEAK_LENS):
        write_wav_pcm16(tmp_path / f"u{b}.wav", speech[b, :n].numpy(), 16000)
        lines.append(f"u{b} {tmp_path / f'u{b}.wav'}")
    (tmp_path / "wav.scp").write_text("\n".join(lines) + "\n")
    main(["--output_dir", str(tmp_path / "out"), "--ngpu", "1", "--dtype", dtype, "--batch_size", "2",
          "--data_path_and_name_and_type", f"{tmp_path / 'wav.scp'},speech,sound", "--asr_train_config",
          str(tmp_path / "config.yaml"), "--asr_model_file", str(tmp_path / "model.pth"), "--maskctc_n_iterations", "10",
          "--maskctc_threshold_probability", repr(p_thres)])
    rows = dict(ln.split(maxsplit=1) if " " in ln.strip() else (ln.strip(), "")
                for ln in (tmp_path / "out" / "1best_recog" / "token_int").read_text().splitlines())
    assert [rows[f"u{b}"].split() for b in range(len(PEAK_LENS))] == [[str(v) for v in r] for r in results[(10, p_thres)]]
    assert (tmp_path / "out" / "1best_recog" / "token").exists()


def test_speech2text_refuses_a_model_that_is_not_maskctc(tmp_path):
    import yaml

    from espnet_amd.bin.asr_inference_maskctc import Speech2Text
    from espnet_amd.tasks.asr import ASRTask

    cfg = dict(_peaked_config(), decoder="transformer", model="espnet")
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save(ASRTask.build_model(cfg).state_dict(), tmp_path / "model.pth")
    with pytest.raises(ValueError, match="MaskCTCModel"):
        Speech2Text(str(tmp_path / "config.yaml"), str(tmp_path / "model.pth"), device="cuda")
