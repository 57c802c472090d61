"""GPU parity of the E-Branchformer encoder through the C-ABI
(em_ebranchformer_encode; kernel-level: em_gemm GELU epilogue, em_layernorm_act, em_dwconv modes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import conformer as oc  # noqa: E402
from oracle import ebranchformer as oe  # noqa: E402
from tests.helpers import golden_speech, golden_state_dict, hparams, load_golden  # noqa: E402


def build(g, dtype):
    from espnet_amd.tasks.asr import ASRTask

    cfg = dict(g["config"])
    cfg["compute_dtype"] = dtype
    model = ASRTask.build_model(cfg)
    model.load_state_dict(golden_state_dict(g), strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("gname", ["ebf_tiny_blocks", "bf_tiny_blocks", "bf_learned_ave_4s", "bf_fixed_ave_4s"])
def test_state_dict_keys_equal_reference(gname):
    g = load_golden(gname)
    model = build(g, "float32")
    import json

    ref = {k: tuple(v) for k, v in json.loads(str(g["state_shapes"])).items()}
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert {k: v for k, v in mine.items() if k.startswith("encoder.")} == \
           {k: v for k, v in ref.items() if k.startswith("encoder.")}


@pytest.mark.parametrize("name", ["ebf_small_5s", "bf_small_4s", "ebf_sub6_4s", "ebf_legacy_4s", "bf_learned_ave_4s",
                                  "bf_fixed_ave_4s"])
def test_encode_float32_matches_reference(name):
    g = load_golden(name)
    model = build(g, "float32")
    speech, lens = golden_speech(g)
    enc, olens = model.encode(speech.cuda(), lens)
    assert olens.tolist() == g["enc_olens"].tolist()
    ke = int(g["enc_keep_every"])
    ref = torch.from_numpy(g["enc_out"])
    for b in range(enc.size(0)):  # padded rows beyond olens are not defined by the reference either
        n = (int(olens[b]) + ke - 1) // ke
        err = (enc[b, ::ke].cpu()[:n] - ref[b, :n]).abs().max().item()
        assert err < 2e-3, (b, err)
    _, tokens, tlens = model.greedy_ctc_device(model._last_state)
    ids = model.ctc.argmax(enc).cpu().numpy()
    diff = ids != g["ctc_ids"]
    for b in range(ids.shape[0]):
        n = int(olens[b])
        assert (g["ctc_margin"][b, :n][diff[b, :n]] < 1e-4).all()
        if not diff[b, :n].any():
            assert tokens[b, : int(tlens[b])].tolist() == g["g1_tokens"][b, : g["g1_lens"][b]].tolist()


@pytest.mark.parametrize("gname", ["ebf_small_5s", "bf_small_4s"])
def test_encode_bfloat16_within_tolerance_and_isolated_rows(gname):
    g = load_golden(gname)
    sd = golden_state_dict(g)
    hp = hparams(g)
    speech, lens = golden_speech(g)
    model = build(g, "bfloat16")
    enc, olens = model.encode(speech.cuda(), lens)
    ke = int(g["enc_keep_every"])
    ref = torch.from_numpy(g["enc_out"])
    for b in range(enc.size(0)):
        n = (int(olens[b]) + ke - 1) // ke
        rel = (enc[b, ::ke].cpu()[:n] - ref[b, :n]).norm() / ref[b, :n].norm()
        assert rel < 3e-2, (b, float(rel))  # bf16 operands, f32 accumulation / residual stream
    # isolated-utterance batching (decode CLI semantics): row b == the ORACLE on utterance b alone
    m32 = build(g, "float32")
    st = m32.encode_device(speech.cuda(), [int(v) for v in lens], isolate=True)
    for b, n in enumerate(int(v) for v in lens):
        with torch.no_grad():
            r, ol = oe.encode(sd, speech[b : b + 1, :n], torch.tensor([n]), hp["heads"], hp["num_blocks"],
                              hp["n_fft"], hp["win_length"], hp["hop"])
        T = int(ol[0])
        assert st.olens[b] == T
        assert (st.enc_out[b, :T].cpu() - r[0]).abs().max().item() < 2e-3


@pytest.mark.parametrize("gname", ["bf_learned_ave_4s", "bf_fixed_ave_4s"])
def test_branchformer_merge_methods_bfloat16(gname):
    """merge_method learned_ave / fixed_ave in bf16: relative error of the encoder output vs the fp32 reference."""
    g = load_golden(gname)
    speech, lens = golden_speech(g)
    model = build(g, "bfloat16")
    enc, olens = model.encode(speech.cuda(), lens)
    assert olens.tolist() == g["enc_olens"].tolist()
    ke = int(g["enc_keep_every"])
    ref = torch.from_numpy(g["enc_out"])
    for b in range(enc.size(0)):
        n = (int(olens[b]) + ke - 1) // ke
        rel = (enc[b, ::ke].cpu()[:n] - ref[b, :n]).norm() / ref[b, :n].norm()
        assert rel < 3e-2, (b, float(rel))


def _dev(t):
    return t.cuda().contiguous()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_branch_learned_ave_against_torch(prec):
    """em_branch_learned_ave (masked attention pooling of both branches -> softmax of the two scalars ->
    weighted sum) against the reference's formulation in plain torch fp32 (branchformer_encoder.py:212-270);
    ragged lengths incl. fewer valid frames than the 4 waves of the pooling workgroup."""
    from espnet_amd import lib as L

    lib = L.load()
    dt, tdt, tol = (L.EM_F32, torch.float32, 2e-5) if prec == "f32" else (L.EM_BF16, torch.bfloat16, 2e-2)
    gen = torch.Generator().manual_seed(11)
    B, T, d = 3, 50, 192
    lens = [50, 3, 21]
    cat = (torch.randn(B, T, 2 * d, generator=gen)).to(tdt)
    pw, pb = torch.randn(2, d, generator=gen) * 0.3, torch.randn(2, generator=gen)
    ww, wb = torch.randn(2, d, generator=gen) * 0.3, torch.randn(2, generator=gen)
    x = cat.float()
    ws = []
    for k in range(2):
        xb = x[..., k * d:(k + 1) * d]
        score = (F.linear(xb, pw[k:k + 1], pb[k:k + 1]).transpose(1, 2)) / d ** 0.5
        m = torch.arange(T)[None, None, :] >= torch.tensor(lens)[:, None, None]
        score = torch.softmax(score.masked_fill(m, torch.finfo(torch.float32).min), -1).masked_fill(m, 0.0)
        ws.append(F.linear(torch.matmul(score, xb).squeeze(1), ww[k:k + 1], wb[k:k + 1]))
    raw = torch.cat(ws, -1)
    mwr = torch.softmax(raw, -1)
    ref = mwr[:, 0, None, None] * x[..., :d] + mwr[:, 1, None, None] * x[..., d:]
    catd, ld = _dev(cat), torch.tensor(lens, dtype=torch.int32, device="cuda")
    mw = torch.empty(B, 2, device="cuda")
    out = torch.empty(B, T, d, dtype=tdt, device="cuda")
    args = [_dev(t) for t in (pw, pb, ww, wb)]
    L.check(lib.em_branch_learned_ave(dt, catd.data_ptr(), ld.data_ptr(), B, T, d, *[a.data_ptr() for a in args],
                                      mw.data_ptr(), out.data_ptr(), L.current_stream_ptr()), "learned_ave")
    assert (mw.cpu() - raw).abs().max().item() < 1e-4 * (1 + raw.abs().max().item())
    assert (out.float().cpu() - ref).abs().max().item() < tol * (1 + ref.abs().max().item())


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_cgmlp_kernels_against_torch(prec):
    """GELU epilogue, strided LayerNorm and the gated / self-residual depthwise conv, each against plain
    torch fp32 on the same (rounded) inputs."""
    from espnet_amd import lib as L

    lib = L.load()
    dt, tdt, tol = (L.EM_F32, torch.float32, 3e-5) if prec == "f32" else (L.EM_BF16, torch.bfloat16, 2e-2)
    g = torch.Generator().manual_seed(3)
    M, d, cg, B, T, k = 2 * 37, 128, 256, 2, 37, 15
    ch = cg // 2
    sp = L.current_stream_ptr()
    # GEMM + exact GELU
    a = (torch.randn(M, d, generator=g) * 0.5).to(tdt)
    w = (torch.randn(cg, d, generator=g) * d ** -0.5).to(tdt)
    bias = torch.randn(cg, generator=g) * 0.1
    ref = F.gelu(F.linear(a.float(), w.float(), bias))
    h = torch.empty(M, cg, dtype=tdt, device="cuda")
    ad, wd, bd = _dev(a), _dev(w), _dev(bias)
    args = L.EmGemmArgs(A=ad.data_ptr(), W=wd.data_ptr(), C=h.data_ptr(), bias=bd.data_ptr(), M=M, N=cg, K=d,
                        lda=d, ldc=cg, scale=1.0)
    L.check(lib.em_gemm(dt, L.EM_EPI_GELU, L.EM_A_PLAIN, args, sp), "gelu gemm")
    assert (h.float().cpu() - ref).abs().max().item() < tol * 4
    # LayerNorm of the gate half, in place in the wide matrix
    hq = h.float().cpu()
    gam, bet = 1 + 0.1 * torch.randn(ch, generator=g), 0.1 * torch.randn(ch, generator=g)
    ref_gn = F.layer_norm(hq[:, ch:], (ch,), gam, bet, 1e-12)
    gn = torch.empty(M, ch, dtype=tdt, device="cuda")
    gd, bd2 = _dev(gam), _dev(bet)
    L.check(lib.em_layernorm_act(dt, h.data_ptr() + ch * h.element_size(), cg, gd.data_ptr(), bd2.data_ptr(), M, ch,
                                 1e-12, gn.data_ptr(), ch, sp), "ln act")
    assert (gn.float().cpu() - ref_gn).abs().max().item() < tol * 8
    # gated depthwise conv: r * (conv(gn) + b), with and without length masking
    cw = torch.randn(ch, 1, k, generator=g) * k ** -0.5
    cb = torch.randn(ch, generator=g) * 0.1
    gq = gn.float().cpu().view(B, T, ch)
    rq = hq[:, :ch].view(B, T, ch)
    cwd, cbd = _dev(cw.reshape(ch, k).t()), _dev(cb)
    for tl in (None, [T, T // 2]):
        gm = gq.clone()
        if tl is not None:
            for bi, n in enumerate(tl):
                gm[bi, n:] = 0
        ref_gate = rq * F.conv1d(gm.transpose(1, 2), cw, cb, padding=(k - 1) // 2, groups=ch).transpose(1, 2)
        out = torch.empty(B, T, ch, dtype=tdt, device="cuda")
        tld = torch.tensor(tl, dtype=torch.int32, device="cuda") if tl is not None else None
        L.check(lib.em_dwconv(dt, L.EM_DW_GATE, gn.data_ptr(), ch, cwd.data_ptr(), cbd.data_ptr(), L.ptr(tld), B, T, ch,
                              k, h.data_ptr(), cg, out.data_ptr(), ch, sp), "dw gate")
        for bi in range(B):
            n = T if tl is None else tl[bi]
            assert (out[bi, :n].float().cpu() - ref_gate[bi, :n]).abs().max().item() < tol * 8
    # LayerNorm folded into the conv's input stage: bit-identical to layernorm_act + gated conv
    stats = torch.empty(M, 2, device="cuda")
    L.check(lib.em_row_stats(dt, h.data_ptr() + ch * h.element_size(), cg, M, ch, 1e-12, stats.data_ptr(), sp), "stats")
    ref_mean = hq[:, ch:].mean(1)
    assert (stats[:, 0].cpu() - ref_mean).abs().max().item() < 1e-5
    for tl in (None, [T, T // 2]):
        tld = torch.tensor(tl, dtype=torch.int32, device="cuda") if tl is not None else None
        unfused = torch.empty(B, T, ch, dtype=tdt, device="cuda")
        fused = torch.empty(B, T, ch, dtype=tdt, device="cuda")
        L.check(lib.em_dwconv(dt, L.EM_DW_GATE, gn.data_ptr(), ch, cwd.data_ptr(), cbd.data_ptr(), L.ptr(tld), B, T, ch,
                              k, h.data_ptr(), cg, unfused.data_ptr(), ch, sp), "dw gate")
        L.check(lib.em_dwconv_ln_gate(dt, h.data_ptr() + ch * h.element_size(), cg, stats.data_ptr(), gd.data_ptr(),
                                      bd2.data_ptr(), cwd.data_ptr(), cbd.data_ptr(), L.ptr(tld), B, T, ch, k,
                                      h.data_ptr(), cg, fused.data_ptr(), ch, sp), "dw ln gate")
        for bi in range(B):
            n = T if tl is None else tl[bi]
            assert torch.equal(fused[bi, :n], unfused[bi, :n])
    # self-residual depthwise conv over a [.., 2d] matrix
    cat = (torch.randn(B, T, 2 * d, generator=g) * 0.5).to(tdt)
    mw = torch.randn(2 * d, 1, 7, generator=g) * 7 ** -0.5
    mb = torch.randn(2 * d, generator=g) * 0.1
    ref_m = cat.float() + F.conv1d(cat.float().transpose(1, 2), mw, mb, padding=3, groups=2 * d).transpose(1, 2)
    outm = torch.empty(B, T, 2 * d, dtype=tdt, device="cuda")
    catd, mwd, mbd = _dev(cat), _dev(mw.reshape(2 * d, 7).t()), _dev(mb)
    L.check(lib.em_dwconv(dt, L.EM_DW_SELFRES, catd.data_ptr(), 2 * d, mwd.data_ptr(), mbd.data_ptr(), None, B, T,
                          2 * d, 7, None, 0, outm.data_ptr(), 2 * d, sp), "dw selfres")
    assert (outm.float().cpu() - ref_m).abs().max().item() < tol * 8


def test_ebranchformer_512_row_block_ffn_matches_per_operator_and_oracle():
    """Round 6: at d = 512 (bf16) the two feed-forward modules of an E-Branchformer block run as row-block launches of
    csrc/ffn_rows.hip ([macaron FFN + residual + norm_mha], [FFN + residual + norm_final + the next LayerNorm / after_norm])
    when a round of 64-row workgroups fills its share of the chip.  No reference fixture has d = 512: a seeded 3-block model
    (512d, 8 heads, linear_units 1024, cgMLP 3072, merge kernel 31) is encoded (a) through the row-block launches (fill rule
    lowered by the developer switch), (b) through the per-operator sequence (ESPNET_AMD_NO_FFN_ROWS), (c) by the f32 CPU oracle
    (oracle/ebranchformer.py, which restates e_branchformer_encoder.py:110-183): (a) against (b) to bf16 round-off, both
    against (c) under the bound of the other bf16 encoder tests; rows of equal utterances bit-identical."""
    import os

    from espnet_amd import lib as L
    from espnet_amd.tasks.asr import ASRTask

    torch.manual_seed(5)
    vocab = 40
    conf = dict(output_size=512, attention_heads=8, linear_units=1024, num_blocks=3, input_layer="conv2d", rel_pos_type="latest",
                pos_enc_layer_type="rel_pos", attention_layer_type="rel_selfattn", cgmlp_linear_units=3072, cgmlp_conv_kernel=31,
                use_linear_after_conv=False, gate_activation="identity", use_ffn=True, macaron_ffn=True,
                ffn_activation_type="swish", merge_conv_kernel=31)
    cfg = dict(token_list=["<blank>", "<unk>"] + [f"t{i}" for i in range(vocab - 3)] + ["<sos/eos>"], frontend="default",
               frontend_conf=dict(n_fft=512, hop_length=160), normalize="utterance_mvn", normalize_conf={},
               encoder="e_branchformer", encoder_conf=conf, decoder="transformer",
               decoder_conf=dict(attention_heads=8, linear_units=256, num_blocks=1), model_conf=dict(ctc_weight=0.3),
               compute_dtype="bfloat16")
    model = ASRTask.build_model(cfg).cuda().eval()
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    n = 16000 * 3
    g = torch.Generator().manual_seed(9)
    one = 0.1 * torch.randn(1, n, generator=g)
    B = 6
    wav = one.repeat(B, 1).cuda()
    lens = [n] * B
    lib = L.load()

    def run(env):
        for k, v in env.items():
            os.environ[k] = v
        lib.em_dev_switches_reload()
        try:
            model.encoder.invalidate()  # (pack again: nothing is cached across the switch)
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
    d = (rows[0, :T] - plain[0, :T]).abs()
    print(f"[ebf 512, row-block vs per-operator] max {d.max():.3e} mean {d.mean():.3e}")
    assert d.max() < 0.08 and d.mean() < 6e-3 and d.max() > 0.0  # (> 0: the two paths really are different launches)
    with torch.no_grad():
        ref, ol = oe.encode(sd, one, torch.tensor([n]), 8, 3, 512, 512, 160)
    assert int(ol[0]) == T
    for name, enc in (("row-block", rows), ("per-operator", plain)):
        rel = (enc[0, :T] - ref[0]).norm() / ref[0].norm()
        print(f"[ebf 512, {name} vs oracle] relative error {float(rel):.3e}")
        assert rel < 3e-2, (name, float(rel))
