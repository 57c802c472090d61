"""No output bit of an entry point may depend on what its scratch held on entry (include/espnet_amd.h, "Scratch memory").

Every cell runs one entry point on scratch filled with zeros (twice: the repeatability premise), with 0xFF bytes (NaN in
f32 and bf16, -1 in int32), with 0x7F bytes (+3.39e38, finite: fmax drops NaN, a huge finite value is not dropped) and on
the leftovers of a larger call of the same entry point with other inputs, and compares the outputs bit for bit
(tests/scratch_fill.py).  The reference of every cell is the same call on zero-filled scratch: no tolerance anywhere.

The models are the smallest the suite builds, with seeded random weights: the reference is the call itself, so trained
weights add nothing.  The host layers allocate their outputs inside the call; `_AllocShim` stands in for the `torch` name
of those modules so that every `torch.empty` of a run starts from the run's pre-fill pattern (an element the call never
writes then differs between the runs)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from espnet_amd import lib as L  # noqa: E402
from tests import scratch_fill as sf  # noqa: E402

DEV = torch.device("cuda")


class _AllocShim:
    """`torch` for a host-layer module: `empty` on the device comes back filled with `byte` (None: as allocated)."""

    byte = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        t = torch.empty(*args, **kw)
        if self.byte is not None and t.is_cuda:
            sf.fill_bytes(t, self.byte)
        return t

    def set(self, byte):
        self.byte = byte


def _shim(monkeypatch, *modules):
    shim = _AllocShim()
    for m in modules:
        monkeypatch.setattr(m, "torch", shim)
    return shim


def _seeded(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m.to(DEV).eval()


# ======================================================================================= batch encoders (forward_device)
def _feats(flens, seed, n_mels=80):
    """(B, max flens, n_mels) f32 log-mel-like noise, zero behind every utterance's end (as a collate pads)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(flens), max(flens), n_mels, generator=g)
    for b, n in enumerate(flens):
        x[b, n:] = 0
    return x.to(DEV), torch.tensor(flens, dtype=torch.int32).to(DEV)


def _frames_for(T):
    """Feature frames that Conv2dSubsampling (conv2d) turns into T encoder frames: ((T_f - 1) // 2 - 1) // 2 = T."""
    return 4 * T + 3


@functools.lru_cache(maxsize=None)
def _encoder(kind, dtype="bfloat16", blocks=2):
    from espnet_amd.asr.ctc import CTC
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_amd.asr.encoder.e_branchformer_encoder import BranchformerEncoder, EBranchformerEncoder
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder

    if kind in ("conformer", "conformer_ctc"):
        enc = ConformerEncoder(80, 256, 4, 512, blocks, macaron_style=True, rel_pos_type="latest", compute_dtype=dtype)
    elif kind == "conformer512":
        enc = ConformerEncoder(80, 512, 8, 2048, blocks, macaron_style=True, rel_pos_type="latest", compute_dtype=dtype)
    elif kind == "legacy":
        enc = ConformerEncoder(80, 256, 4, 512, blocks, macaron_style=True, rel_pos_type="legacy", compute_dtype=dtype)
    elif kind == "e_branchformer":
        enc = EBranchformerEncoder(80, 256, attention_heads=4, linear_units=512, cgmlp_linear_units=512, num_blocks=blocks,
                                   use_ffn=True, macaron_ffn=True, compute_dtype=dtype)
    elif kind == "branchformer":
        enc = BranchformerEncoder(80, 256, attention_heads=4, cgmlp_linear_units=512, num_blocks=blocks,
                                  merge_method="learned_ave", compute_dtype=dtype)
    elif kind == "transformer":
        enc = TransformerEncoder(80, 256, 4, 512, blocks, compute_dtype=dtype)
    else:
        raise KeyError(kind)
    enc = _seeded(enc, 11)
    if kind == "conformer_ctc":  # the head whose per-frame arg-max the last block kernel hands back (EM_BLOCK_CTC)
        object.__setattr__(enc, "fused_ctc", _seeded(CTC(100, 256, compute_dtype=dtype), 12))
    return enc


def _encoder_cell(monkeypatch, enc, T, *, isolate=False, attrs=None, ctc_ids=False, B_stale=4, T_stale=300):
    """B = 3 ragged utterances (T frames, about T / 2, the fewest the subsampling allows) through `forward_device` with
    the stream's workspace (`encoder._ws`) pre-seeded: ZERO, ONES, BIG, and STALE = the leftovers of B = 4, T = 300."""
    from espnet_amd.asr.encoder import _subsampled_base, conformer_encoder

    shim = _shim(monkeypatch, _subsampled_base, conformer_encoder)
    for k, v in (attrs or {}).items():
        monkeypatch.setattr(enc, k, v, raising=False)
    T_f = _frames_for(T)
    assert enc.output_frames(T_f) == T
    flens = [T_f, _frames_for(max(1, T // 2)) + 1, 7]
    feats, flens_dev = _feats(flens, 100 + T)
    big_T_f = _frames_for(T_stale)
    big_lens = [big_T_f, big_T_f - 90, 500, 33][:B_stale]
    big, big_dev = _feats(big_lens, 7)
    big = big * 3.0 + 1.0  # (other features, another scale)
    skey = torch.cuda.current_stream().cuda_stream
    enc._ws.pop(skey, None)

    def stale():
        shim.set(None)
        enc.forward_device(big, big_lens, big_dev, None, isolate)

    stale()  # allocates the workspace every run below reuses: the host layer's reuse rule is part of what is tested
    torch.cuda.synchronize()
    ws = enc._ws[skey]

    def call():
        enc_out, enc_act, olens, _ = enc.forward_device(feats, flens, flens_dev, None, isolate)
        assert enc._ws[skey] is ws and olens[0] == T and olens[2] <= 3
        outs = [enc_out, enc_act]
        if ctc_ids:
            assert enc.last_ctc_ids is not None, "the fused CTC arg-max plan was not taken"
            outs.append(enc.last_ctc_ids)
        return outs

    ref = sf.assert_scratch_independent(call, ws, None, None, stale=stale, prefill=shim.set,
                                        names=["enc_out", "enc_act", "last_ctc_ids"])
    assert tuple(ref[0].shape) == (3, T, enc.output_size())
    return ref


# The clear of V^T (csrc/encoder.hip, em_conformer_encode) is taken when 32 * ceil(T / 32) < Tpad: T = 40 (Tpad 256: taken),
# 225 and 256 (the 32-frame row blocks write every column; 256 is the exact tile), 257 (Tpad 512: taken).
@pytest.mark.parametrize("T", [40, 225, 256, 257])
def test_conformer256_fused(monkeypatch, T):
    enc = _encoder("conformer")
    pk = enc.packed(DEV)  # (the premise: these weights take the fused block kernels)
    assert L.load().em_conformer_encode_plan(enc.em_dtype, C.byref(pk.w), 0) & L.EM_ENC_PLAN_FUSED
    _encoder_cell(monkeypatch, enc, T)


VARIANTS = {
    "split_att": dict(attrs=dict(split_att=True)),              # EM_ENC_SPLIT_ATT: em_relpos_attention2_bf16 + block<C>
    "fold_c_2": dict(attrs=dict(fold_c=True), blocks=2),        # EM_ENC_FOLD_C: the x / `big` ping-pong ends in either slot
    "fold_c_3": dict(attrs=dict(fold_c=True), blocks=3),
    "no_fused": dict(attrs=dict(fused=False)),                  # EM_ENC_NO_FUSED: one operator per launch
    "f32": dict(dtype="float32"),
    "isolate": dict(isolate=True),                              # EM_ENC_ISOLATE_UTTS
    "ctc_ids": dict(kind="conformer_ctc", ctc_ids=True),        # the fused CTC arg-max plan: last_ctc_ids is an output
}


@pytest.mark.parametrize("T", [40, 256])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_conformer256_variants(monkeypatch, variant, T):
    v = dict(VARIANTS[variant])
    enc = _encoder(v.pop("kind", "conformer"), v.pop("dtype", "bfloat16"), v.pop("blocks", 2))
    _encoder_cell(monkeypatch, enc, T, **v)


def test_conformer512(monkeypatch):
    """The 512-wide model: q / k / V^T head slabs cleared per call (csrc/encoder.hip, `attn2`), em_relpos_attention2_bf16,
    once with the per-operator launches a small batch takes by default and once - the fill rule lowered - with the
    row-block launches and their q | k | v walk (csrc/ffn_rows.hip) at B * T = 210 rows, no multiple of their 64-row
    block.  The two are different launch sequences: their outputs differ in some bit."""
    lib = L.load()
    enc = _encoder("conformer512")
    lib.em_dev_switches_reload()
    plain = _encoder_cell(monkeypatch, enc, 70)
    monkeypatch.setenv("ESPNET_AMD_FFN_ROWS_MIN_FILL", "1")
    lib.em_dev_switches_reload()
    try:
        rows = _encoder_cell(monkeypatch, enc, 70)
    finally:
        monkeypatch.delenv("ESPNET_AMD_FFN_ROWS_MIN_FILL", raising=False)
        lib.em_dev_switches_reload()
    assert not sf.bytes_equal(rows[0], plain[0]), "the row-block launches were not taken"


@pytest.mark.parametrize("T", [40, 257])
def test_legacy_relpos(monkeypatch, T):
    _encoder_cell(monkeypatch, _encoder("legacy"), T)


@pytest.mark.parametrize("T", [70, 270])
@pytest.mark.parametrize("kind", ["e_branchformer", "branchformer"])
def test_branchformers(monkeypatch, kind, T):
    _encoder_cell(monkeypatch, _encoder(kind), T)


@pytest.mark.parametrize("T", [17, 256, 257])
def test_transformer_encoder(monkeypatch, T):
    _encoder_cell(monkeypatch, _encoder("transformer"), T)


# ======================================================================================= streaming encoders (forward_infer_batch)
@functools.lru_cache(maxsize=None)
def _stream_encoder(kind, dtype):
    from espnet_amd.asr.encoder.contextual_block_conformer_encoder import ContextualBlockConformerEncoder
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder

    if kind == "cb":
        enc = ContextualBlockConformerEncoder(80, 256, 4, 512, 2, macaron_style=True, cnn_module_kernel=15, compute_dtype=dtype)
    else:
        enc = ContextualBlockTransformerEncoder(80, 256, 4, 512, 2, compute_dtype=dtype)
    return _seeded(enc, 21)


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("kind", ["cb", "cbt"])
def test_streaming_encoders(monkeypatch, kind, S, dtype):
    """em_cb_encode_blocks_batch / em_cbt_encode_blocks_batch through `forward_infer_batch` and the encoder's `_ws` dict:
    three consecutive ticks of S lock-step streams (360, 128, 128 feature frames: 4, 2 and 2 blocks per stream, so the third
    tick runs in the workspace the second left behind) and a final one.  Outputs: the frames of every tick, and the
    carried context (`next_ctx`) and `prev_addin` behind the third.  STALE: the same ticks with other features first."""
    from espnet_amd.asr.encoder import _contextual_block_base

    enc = _stream_encoder(kind, dtype)
    shim = _shim(monkeypatch, _contextual_block_base)
    g = torch.Generator().manual_seed(31 + S)
    ticks = [torch.randn(S, n, 80, generator=g).to(DEV) for n in (360, 128, 128, 100)]
    other = [(t * 2.0 - 1.0).flip(0).contiguous() for t in ticks]

    def run(chunks):
        outs, st = [], None
        for i, x in enumerate(chunks):
            if i == 3:
                ctx, addin = st["past_encoder_ctx"], st["prev_addin"]
            ys, y_len, st = enc.forward_infer_batch(x, st, is_final=(i == 3))
            assert y_len > 0
            outs.append(ys)
        return outs + [ctx, addin]

    shim.set(None)
    enc._ws.clear()
    run(ticks)  # allocates the workspaces of the shapes below
    torch.cuda.synchronize()
    held = dict(enc._ws)
    assert len(held) >= 2

    def call():
        outs = run(ticks)
        assert all(enc._ws[k] is v for k, v in held.items()) and len(enc._ws) == len(held)
        return outs

    def stale():
        shim.set(None)
        run(other)

    sf.assert_scratch_independent(call, list(held.values()), None, None, stale=stale, prefill=shim.set,
                                  names=["ys tick 1", "ys tick 2", "ys tick 3", "ys final", "next_ctx", "prev_addin"])


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("kind", ["cb", "cbt"])
def test_streaming_short_utterance(monkeypatch, kind, S):
    """em_cb_encode_blocks / em_cbt_encode_blocks (the entry without context slots): S utterances that end inside their
    first block, 100 feature frames -> 24 encoder frames <= block_size.  STALE: other utterances of the same shape."""
    from espnet_amd.asr.encoder import _contextual_block_base

    enc = _stream_encoder(kind, "bfloat16")
    shim = _shim(monkeypatch, _contextual_block_base)
    g = torch.Generator().manual_seed(37 + S)
    x = torch.randn(S, 100, 80, generator=g).to(DEV)
    other = (x * 2.0 - 1.0).flip(1).contiguous()

    def run(feats):
        ys, y_len, st = enc.forward_infer_batch(feats, None, is_final=True)
        assert st is None and 0 < y_len <= enc.block_size
        return [ys]

    shim.set(None)
    enc._ws.clear()
    run(x)
    torch.cuda.synchronize()
    held = dict(enc._ws)
    assert len(held) == 1

    def call():
        outs = run(x)
        assert all(enc._ws[k] is v for k, v in held.items()) and len(enc._ws) == 1
        return outs

    def stale():
        shim.set(None)
        run(other)

    sf.assert_scratch_independent(call, list(held.values()), None, None, stale=stale, prefill=shim.set, names=["ys"])


# ======================================================================================= scorers and walkers (C ABI)
class _Abi:
    """One C-ABI call on a workspace the test owns: `need` bytes, `run(ws)` enqueues it, `outputs` it writes, `defined`
    per output None or the mask of the region the header defines as written."""

    def __init__(self, need, run, outputs, defined=None, names=None, finite=None):
        self.need, self.run, self.outputs, self.defined, self.names, self.finite = int(need), run, outputs, defined, names, finite


def _abi_cell(small: _Abi, big: _Abi):
    """`small` on ZERO / ONES / BIG scratch and on what `big` (a larger shape, other inputs) left in the same workspace."""
    assert big.need >= small.need > 0, (small.need, big.need)
    ws = torch.empty(big.need, dtype=torch.uint8, device=DEV)
    return sf.assert_scratch_independent(lambda: small.run(ws), ws, small.outputs, small.defined,
                                         stale=lambda: big.run(ws), names=small.names, finite=small.finite)


def _i32(v):
    return torch.as_tensor(v).to(torch.int32).contiguous().to(DEV)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_dec_seq_nll(dtype):
    """em_dec_seq_nll: the h4 decoder of tests/dec_seq_cases.py (V = 1 027), three ragged transcripts at Lp = 17 (51 rows,
    no whole 16-query tile) on memories of 45, 1 and 23 frames; STALE: five transcripts at Lp = 41 on five other memories."""
    from espnet_amd.asr.espnet_model import build_dec_nll_batch
    from tests import dec_seq_cases as K

    name = "h4"
    V = K.MODELS[name][0]
    m = K.build_model(name, dtype).to(DEV)
    dec, lib = m.decoder, L.load()
    rt = torch.bfloat16 if dtype == "bfloat16" else None
    pk = dec.packed(DEV, 64)

    def case(mem, hl, text, lens):
        xi, ki, ti = (_i32(t) for t in build_dec_nll_batch(text, lens, m.sos, m.eos, V))
        dec._mem = None
        mm = dec._memory(mem.to(DEV), pk)
        dec._mem = None
        B, Lp = xi.shape
        kl = _i32(hl)
        nll = torch.empty(B, Lp, dtype=torch.float32, device=DEV)
        need = lib.em_dec_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)

        def run(ws):
            L.check(lib.em_dec_seq_nll(pk.dtype, C.byref(pk.w), L.ptr(mm["mem_kv"]), L.ptr(mm["mem_vT"]), L.ptr(kl), None,
                                       L.ptr(xi), L.ptr(ki), L.ptr(ti), B, mem.size(0), Lp, mem.size(1), mm["Tpad"],
                                       L.ptr(nll), L.ptr(ws), ws.numel(), L.current_stream_ptr()), "em_dec_seq_nll")

        return _Abi(need, run, [nll], names=["nll"])

    mem, hl = K.make_memory(1017, round_to=rt)
    text, lens = K.make_text(17, V)
    g = torch.Generator().manual_seed(41)
    mem2, hl2 = K.make_memory(77, Bm=5, hlens=(30, 7, 45, 1, 19), round_to=rt)
    text2, lens2 = torch.randint(1, V - 1, (5, 40), generator=g), torch.tensor([40, 13, 0, 27, 39])
    ref = _abi_cell(case(mem, hl, text, lens), case(mem2, hl2, text2, lens2))
    assert tuple(ref[0].shape) == (3, 17)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_lm_seq_nll(dtype):
    """em_lm_seq_nll: the h4pe TransformerLM of tests/lm_nll_cases.py, three ragged sentences at Lp = 65 (195 rows);
    STALE: five sentences at Lp = 130."""
    from tests import lm_nll_cases as K

    name = "h4pe"
    V = K.MODELS[name][0]
    m = K.build_model(name, dtype).to(DEV)
    lm, lib = m.lm, L.load()
    pk = lm.packed(DEV, 140)

    def case(text, lens):
        x, t, _, scored = m._masked_pair(text, lens)
        xi, ti = _i32(x), _i32(torch.where(scored, t, torch.full_like(t, -1)))
        B, Lp = xi.shape
        nll = torch.empty(B, Lp, dtype=torch.float32, device=DEV)
        need = lib.em_lm_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)

        def run(ws):
            L.check(lib.em_lm_seq_nll(pk.dtype, C.byref(pk.w), L.ptr(xi), L.ptr(ti), B, Lp, L.ptr(nll), L.ptr(ws), ws.numel(),
                                      L.current_stream_ptr()), "em_lm_seq_nll")

        return _Abi(need, run, [nll], names=["nll"])

    g = torch.Generator().manual_seed(43)
    text2, lens2 = torch.randint(1, V - 1, (5, 129), generator=g), torch.tensor([129, 64, 1, 100, 77])
    ref = _abi_cell(case(*K.make_text(65, V)), case(text2, lens2))
    assert tuple(ref[0].shape) == (3, 65)


def test_lm_head_nll_bf16():
    """em_lm_head_nll (bf16: per-tile running statistics in the workspace): M = 77 rows, V = 1 027 (a partial last tile of
    both); STALE: M = 130, V = 1 500."""
    lib, d = L.load(), 128

    def case(M, V):
        g = torch.Generator().manual_seed(1000 * M + V)
        xr = (torch.randn(M, d, generator=g) * 3 + 0.5).to(DEV)
        gn, bn = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
        w = (torch.randn(V, d, generator=g) * (2.0 / d ** 0.5)).to(torch.bfloat16).to(DEV)
        bias = (0.5 * torch.randn(V, generator=g)).to(DEV)
        tgt = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
        tgt[1::7] = -1  # rows where nothing is scored: exactly 0.0
        tgt = tgt.to(DEV)
        out = torch.empty(M, dtype=torch.float32, device=DEV)
        need = lib.em_lm_head_nll_workspace_bytes(L.EM_BF16, M, V)

        def run(ws):
            L.check(lib.em_lm_head_nll(L.EM_BF16, L.ptr(xr), L.ptr(gn), L.ptr(bn), L.ptr(w), L.ptr(bias), L.ptr(tgt), M, V, d,
                                       L.ptr(out), L.ptr(ws), ws.numel(), L.current_stream_ptr()), "em_lm_head_nll")

        return _Abi(need, run, [out], names=["nll"])

    _abi_cell(case(77, 1027), case(130, 1500))


def test_ctc_forced_align():
    """em_ctc_forced_align with the back-pointers in the workspace (T = 400 frames x 64 threads x 2 bytes > 48 KiB of LDS):
    B = 3 ragged (400, 201, 1 frames; 20, 7, 0 tokens); STALE: B = 4, T = 450, other posteriors.  Every output is written
    whole (labels -1, spans -1, scores 0 behind the lengths)."""
    lib = L.load()
    V, blank = 50, 0

    def case(xlens, ylens, T, seed):
        g = torch.Generator().manual_seed(seed)
        B, Lmax = len(xlens), max(ylens)
        lpT = torch.log_softmax(torch.randn(B * T, V, generator=g) * 2, -1).t().contiguous().to(DEV)
        tg = _i32(torch.randint(1, V, (B, Lmax), generator=g))
        xl, yl = _i32(xlens), _i32(ylens)
        outs = [torch.empty(B, T, dtype=torch.int32, device=DEV), torch.empty(B, T, dtype=torch.float32, device=DEV),
                torch.empty(B, Lmax, dtype=torch.int32, device=DEV), torch.empty(B, Lmax, dtype=torch.int32, device=DEV),
                torch.empty(B, Lmax, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.float32, device=DEV)]
        need = lib.em_ctc_forced_align_workspace_bytes(B, T, Lmax)

        def run(ws):
            L.check(lib.em_ctc_forced_align(L.ptr(lpT), B * T, L.ptr(xl), L.ptr(tg), Lmax, L.ptr(yl), B, T, blank,
                                            *(L.ptr(o) for o in outs), L.ptr(ws), ws.numel(), L.current_stream_ptr()),
                    "em_ctc_forced_align")

        return _Abi(need, run, outs, names=["align", "frame_lp", "tok_start", "tok_end", "tok_lp", "total"])

    ref = _abi_cell(case([400, 201, 1], [20, 7, 0], 400, 51), case([450, 300, 77, 450], [30, 5, 11, 2], 450, 52))
    assert bool((ref[0][0] >= 0).all()) and bool((ref[0][2, 1:] == -1).all())


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("cell", [("gru", 1, 320, 64, 300, 3, 8), ("lstm", 2, 64, 320, 1027, 33, 2)],
                         ids=lambda c: "-".join(map(str, c)))
def test_transducer_greedy(cell, dtype):
    """em_transducer_greedy with its frame traces, on the walk cells of tests/test_gpu_transducer.py that have ragged
    lengths (B = 3, T = 8 and B = 33, T = 2: rows that fill no 16-row tile).  Defined: tokens[b][< ylens[b]], the traces
    [b][< olens[b]], ylens and score whole; everything else keeps its pre-fill.  STALE: B = 40, T = 12."""
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from tests import test_gpu_transducer as TG

    rnn, layers, H, J, V, B, T = cell
    seed, extra = TG.WALK_SEEDS[cell]
    model, _, _, _ = TG._model(rnn, layers, H, J, V, dtype, seed, **(dict(out_bias=(0, extra)) if extra else {}))
    dec, jn = model.decoder, model.joint_network
    BeamSearchTransducer(dec, jn, beam_size=1)  # (attaches the joint network to the decoder's weights)
    w, keep = dec.weights(DEV)
    lib = L.load()

    def case(B, T, olens, seed):
        enc_dev, _ = TG._enc(seed, (B, T, TG.D), dtype)
        enc_proj = jn.enc_proj_device(enc_dev)
        ol = _i32(olens)
        outs = [torch.empty(B, T, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV),
                torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, T, dtype=torch.int32, device=DEV),
                torch.empty(B, T, dtype=torch.float32, device=DEV), torch.empty(B, T, dtype=torch.float32, device=DEV)]
        need = lib.em_transducer_greedy_workspace_bytes(dec.em_dtype, C.byref(w), B, T)

        def run(ws):
            L.check(lib.em_transducer_greedy(dec.em_dtype, C.byref(w), L.ptr(enc_proj), L.ptr(ol), B, T,
                                             *(L.ptr(o) for o in outs), L.ptr(ws), ws.numel(), L.current_stream_ptr()),
                    "em_transducer_greedy")

        return _Abi(need, run, outs, names=["tokens", "ylens", "score", "frame_tok", "frame_top", "frame_margin"]), enc_proj

    olens = TG._ragged(B, T)
    small, _ = case(B, T, olens, seed + 1)
    big, _ = case(40, 12, TG._ragged(40, 12), seed + 2)
    # the written region of `tokens` is known only from the walk itself: ylens of a first run (tokens[b][y], y < ylens[b])
    ws0 = torch.zeros(big.need, dtype=torch.uint8, device=DEV)
    small.run(ws0)
    torch.cuda.synchronize()
    ylens = small.outputs[1].cpu()
    assert int(ylens.max()) > 0 and bool((ylens <= torch.tensor(olens)).all())
    frames = torch.arange(T).unsqueeze(0)
    in_olens = frames < torch.tensor(olens).unsqueeze(1)
    small.defined = [frames < ylens.unsqueeze(1), None, None, in_olens, in_olens, in_olens]
    ref = _abi_cell(small, big)
    assert torch.equal(ref[1], ylens)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_transducer_lattice_logp(dtype):
    """em_transducer_lattice_logp (the compacted row list lives in the workspace) on the ragged case of
    tests/test_gpu_transducer_nll.py: 7 candidates of 3 utterances, 1 002 nodes = 15 full 64-row tiles + 42 rows.  Defined:
    the nodes t < xlens[mem_of[n]], u <= ylens[n]; the others keep their pre-fill.  STALE: 69 candidates of 4 other utterances."""
    from tests import test_gpu_transducer as TG
    from tests import test_gpu_transducer_nll as TN

    V, J = 1027, 64
    model, _, _, _ = TG._model("lstm", 1, 64, J, V, dtype, 81)
    dec, jn = model.decoder, model.joint_network
    w, keep = dec.weights(DEV)
    lib = L.load()

    def case(xlens, cands, seed):
        N, T, Lmax = len(cands), max(xlens), max(u for _, u in cands)
        g = torch.Generator().manual_seed(seed)
        targets = torch.randint(1, V, (N, Lmax), generator=g)
        ylens, mem_of = [u for _, u in cands], [m for m, _ in cands]
        enc_dev, _ = TG._enc(seed + 1, (len(xlens), T, TG.D), dtype)
        enc_proj = jn.enc_proj_device(enc_dev)
        dec_proj = dec.teacher_forced_proj(targets, torch.tensor(ylens))
        tg, xl, yl, mo = _i32(targets), _i32(xlens), _i32(ylens), _i32(mem_of)
        lat = torch.empty(N, T, Lmax + 1, 2, dtype=torch.float32, device=DEV)
        need = lib.em_transducer_lattice_logp_workspace_bytes(jn.em_dtype, C.byref(w), N, T, Lmax)

        def run(ws):
            jn.lattice_logp_device(dec, enc_proj, xl, dec_proj, tg, yl, mo, out=lat, ws=ws)

        t_ok = torch.arange(T).view(1, T, 1, 1) < torch.tensor([xlens[m] for m in mem_of]).view(N, 1, 1, 1)
        u_ok = torch.arange(Lmax + 1).view(1, 1, Lmax + 1, 1) <= torch.tensor(ylens).view(N, 1, 1, 1)
        # (the label slot of a candidate's last node, u == ylens[n], is -inf by definition)
        last = (torch.arange(Lmax + 1).view(1, 1, Lmax + 1, 1) == torch.tensor(ylens).view(N, 1, 1, 1)) & \
            (torch.arange(2).view(1, 1, 1, 2) == 1)
        return _Abi(need, run, [lat], [(t_ok & u_ok).expand(N, T, Lmax + 1, 2)], names=["lat"],
                    finite=[~last.expand(N, T, Lmax + 1, 2)])

    small = case(TN.LAT_XLENS, TN.LAT_CANDS, 82)
    big = case([40, 9, 2, 33], [(0, 25), (3, 25), (1, 0), (2, 2), (0, 1), (3, 7), (1, 9), (2, 0), (0, 13)] + [(3, 3)] * 60, 90)
    _abi_cell(small, big)


# ======================================================================================= beam search
# Every index the search loads from its buffers is written earlier in the same search or clamped where it is used:
# em_search_init writes tok[0], parent[0], all of anc_a / anc_b, alive, end_count, done (csrc/search.hip); a label step writes
# cand_tok / cand_total of every row (dead rows and done utterances: -inf totals) and sel_idx (-1 for a -inf pick) before
# update_kernel reads them; the embeddings clamp the token ids of rows that never lived (csrc/decoder.hip) and the
# recurrent LM their parents (rnn_gather_kernel); the n-gram scorer walks live rows only; the host reads the ended lists
# up to end_count.
HOST_WRITTEN = ("xlens", "maxlens", "minlens")


def _beam_search(kind, dtype, d=64, heads=2, V=50, beam=5, tmp_path=None):
    """Decoder + CTC (+ a language model / an n-gram scorer) with seeded weights around BatchBeamSearch."""
    import types

    from espnet_amd.asr.ctc import CTC
    from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from espnet_amd.lm.transformer_lm import TransformerLM
    from espnet_amd.nets.batch_beam_search import build_beam_search
    from oracle.weights import token_list

    dec = _seeded(TransformerDecoder(V, d, attention_heads=heads, linear_units=2 * d, num_blocks=2, compute_dtype=dtype), 61)
    ctc = _seeded(CTC(V, d, compute_dtype=dtype), 62)
    with torch.no_grad():  # (logits a few units apart, so that hypotheses end before the forced <eos>)
        dec.output_layer.weight.mul_(20.0)
        ctc.ctc_lo.weight.mul_(20.0)
    lm = ngram = None
    if kind == "transformer_lm":
        lm = _seeded(TransformerLM(V, pos_enc=None, embed_unit=64, att_unit=64, head=2, unit=128, layer=2,
                                   compute_dtype=dtype), 63)
    elif kind in ("lstm", "gru"):  # nhid = 96 -> padded to 128: the state rows have a 32-channel tail that must read as zero
        lm = _seeded(SequentialRNNLM(V, unit=64, nhid=96, nlayers=2, rnn_type=kind, compute_dtype=dtype), 64)
    elif kind == "ngram":
        from tests import test_gpu_ngram as TNG

        tokens = token_list(V)
        ngram = TNG._full(TNG._arpa_for(tmp_path, tokens, 3, seed=65), tokens)
    model = types.SimpleNamespace(decoder=dec, ctc=ctc, sos=V - 1, eos=V - 1)
    return build_beam_search(model, beam_size=beam, ctc_weight=0.3, penalty=0.0, lm_weight=0.6 if lm is not None else 0.0,
                             token_list=token_list(V), lm=lm, ngram=ngram, ngram_weight=0.5 if ngram is not None else 0.0)


def _memories(lens, d, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(len(lens), max(lens), d, generator=g) * 0.5
    for b, n in enumerate(lens):
        enc[b, n:] = 0.0
    return enc.to(torch.bfloat16 if dtype == "bfloat16" else torch.float32).to(DEV)


def _nbest_bits(res):
    """The n-best of every utterance as comparable data: token sequences, and scores / per-scorer scores as f32 bits."""
    bits = lambda v: sf.raw_bytes(torch.as_tensor(float(v), dtype=torch.float32)).tobytes()  # noqa: E731
    out = []
    for hyps in res:
        assert len(hyps) > 0
        out.append([(h.yseq.tolist(), bits(h.score), {k: bits(v) for k, v in h.scores.items()}) for h in hyps])
        for h in hyps:
            assert all(torch.isfinite(torch.as_tensor(float(v))) for v in [h.score, *h.scores.values()])
    return out


def _zero_regions(bs):
    """The regions of the buffers the caller zeroes once (`_ZERO`) that the kernels rely on reading zero: channels
    nhid .. d of every recurrent-LM state row (rnn_cell_kernel writes channels < nhid, rnn_gather_kernel and the w_hh GEMM
    read all d).  mem_vT has no pad column offline: the search pads the memory itself to Tpad = T frames."""
    lm = bs.scorers.get("lm")
    out = []
    for bufs in bs._bufs.values():
        for name in ("rnn_hs", "rnn_cs", "rnn_hin"):
            if name in bufs:
                out.append((name, bufs[name][..., lm.nhid:]))
    return out


BEAM_CELLS = [("dec_ctc", "float32", False), ("dec_ctc", "bfloat16", False), ("dec_ctc", "float32", True),
              ("transformer_lm", "float32", False), ("transformer_lm", "bfloat16", False), ("lstm", "float32", False),
              ("lstm", "bfloat16", False), ("gru", "float32", False), ("gru", "bfloat16", False), ("ngram", "float32", False),
              ("frag", "bfloat16", False)]
_beam_ids = [f"{k}-{d}{'-hipgraph' if g else ''}" for k, d, g in BEAM_CELLS]


def _beam_cell(kind, dtype, graph, tmp_path):
    if kind == "frag":  # bf16, B * W = 100 >= 96 rows: the fragment-major memory (mem_kf / mem_vf) and weights are taken
        bs = _beam_search("dec_ctc", dtype, d=256, heads=4, V=100, beam=10)
        lens_a, lens_b = [37, 20, 5, 33, 1, 40, 17, 29, 36, 8], [40, 9, 31, 2, 38, 16, 25, 7, 33, 12]
    else:
        bs = _beam_search(kind, dtype, tmp_path=tmp_path)
        lens_a, lens_b = [37, 20, 1], [40, 9, 26]
    bs.use_hipgraph = graph
    d = 256 if kind == "frag" else 64
    return bs, (_memories(lens_a, d, 71, dtype), lens_a), (_memories(lens_b, d, 72, dtype), lens_b)


@pytest.mark.parametrize("kind,dtype,graph", BEAM_CELLS, ids=_beam_ids)
def test_beam_search_poisoned_buffers(kind, dtype, graph, tmp_path):
    """`step_hook` hands over the buffer set before em_search_init: every buffer but the three the host writes and the
    four the caller zeroes once is filled with ZERO (twice), BIG and ONES; the n-best must be the same token sequences
    with bit-equal scores and per-scorer scores."""
    from espnet_amd.nets.batch_beam_search import _ZERO

    bs, _, (enc, lens) = _beam_cell(kind, dtype, graph, tmp_path)
    fill = [sf.ZERO]
    seen = {}

    def hook(bufs, **_):
        for name, t in bufs.items():
            if name not in HOST_WRITTEN and name not in _ZERO:
                sf.fill_bytes(t, fill[0])
        seen.update(bufs)

    bs.step_hook = hook
    runs = {}
    for tag, byte in (("ZERO", sf.ZERO), ("ZERO again", sf.ZERO), ("BIG", sf.BIG), ("ONES", sf.ONES)):
        fill[0] = byte
        runs[tag] = _nbest_bits(bs.search_batch(enc, lens))
    if kind == "frag":
        assert "mem_kf" in seen and "mem_vf" in seen, "the fragment-major memory was not allocated"
    assert runs["ZERO again"] == runs["ZERO"], "the search is not bit-repeatable on zero-filled buffers"
    for tag in ("BIG", "ONES"):
        assert runs[tag] == runs["ZERO"], f"the n-best depends on what the buffers held ({tag} against ZERO)"
    for name, tail in _zero_regions(bs):
        assert not bool(tail.any()), f"{name}: the library wrote into the region the caller zeroed"


@pytest.mark.parametrize("kind,dtype,graph", BEAM_CELLS, ids=_beam_ids)
def test_beam_search_dirty_reuse(monkeypatch, kind, dtype, graph, tmp_path):
    """Utterances A, then B of the same shape bucket on the same object: B must equal B searched on a fresh `clone()`, bit
    for bit, and afterwards the zero regions of the `_ZERO` buffers are still zero.  Whatever `_alloc` takes from
    `torch.empty` starts as BIG bytes here (a fresh allocation may hold anything), so a buffer missing from `_ZERO` shows
    in its zero region - as a finite value: 0 x 3.39e38 is still 0, where NaN there would reach every logit."""
    from espnet_amd.nets import batch_beam_search

    shim = _shim(monkeypatch, batch_beam_search)
    shim.set(sf.BIG)
    bs, (enc_a, lens_a), (enc_b, lens_b) = _beam_cell(kind, dtype, graph, tmp_path)
    bs.search_batch(enc_a, lens_a)
    assert len(bs._bufs) == 1
    dirty = _nbest_bits(bs.search_batch(enc_b, lens_b))
    assert len(bs._bufs) == 1, "A and B were meant to share one buffer set"
    fresh_bs = bs.clone()
    fresh = _nbest_bits(fresh_bs.search_batch(enc_b, lens_b))
    assert dirty == fresh, "utterance B's n-best depends on the search that used the buffers before"
    for name, tail in _zero_regions(bs) + _zero_regions(fresh_bs):
        assert not bool(tail.any()), f"{name}: its zero region does not read as zero after a search"
    if kind in ("lstm", "gru"):
        assert len(_zero_regions(bs)) == 3 and all(t.numel() > 0 for _, t in _zero_regions(bs))


def test_online_search_dirty_restart():
    """batch_beam_search_online across a restart: utterance A block by block, reset(), then utterance B on the same object
    equals B on a freshly built search, bit for bit at every call."""
    from tests.helpers import golden_state_dict, load_golden
    from tests.test_gpu_online_search import build_online

    g = load_golden("stream_search_b")
    sd = golden_state_dict(g)
    enc_b = torch.from_numpy(g["enc_all"]).to(DEV)
    enc_a = (enc_b.flip(0) * 1.5).contiguous()
    lens = g["enc_lens"].tolist()

    def run(bs, enc):
        pos, outs = 0, []
        for k, n in enumerate(lens):
            res = bs(enc[pos : pos + n], is_final=(k == len(lens) - 1))
            outs.append([(h.yseq.tolist(), sf.raw_bytes(torch.as_tensor(float(h.score), dtype=torch.float32)).tobytes(),
                          {kk: sf.raw_bytes(torch.as_tensor(float(v), dtype=torch.float32)).tobytes()
                           for kk, v in h.scores.items()}) for h in res])
            pos += n
        bs.reset()
        return outs

    bs = build_online(g, sd, "float32")
    run(bs, enc_a)
    dirty = run(bs, enc_b)
    fresh = run(build_online(g, sd, "float32"), enc_b)
    assert any(len(o) > 0 for o in fresh)
    assert dirty == fresh
