"""MLMDecoder (the masked-language-model decoder of Mask-CTC) on the MI355X.

Mirrors espnet2/asr/decoder/mlm_decoder.py: a TransformerDecoder's parameters and state-dict keys with one more embedding
row and output column for `<mask>`, and a self-attention WITHOUT the causal mask - query j of a sentence sees every key
below the sentence's length.  Packing and `EmDecoderWeights` are the base class's (built with `vocab_size + 1`).

`refine_device` is the decoding path: the K mask-predict passes of a ragged batch as one enqueued chain
(`em_maskctc_refine`, csrc/maskctc.hip: K times the layer chain `em_dec_seq_nll` runs, csrc/dec_seq.hip, and the arg-max
head of csrc/vocab_head.hip).  `forward` keeps the reference's signature and returns the (B, L, V + 1) scores: the same
layers driven launch by launch from here - on purpose not through that chain, so that it stays the independent route the
chain is checked against - for parity tests and for callers that want the logits themselves.
"""
import ctypes as C

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder

LN_EPS = 1e-12  # transformer/layer_norm.py


def _vp(v):
    return C.c_void_p(v)


class MLMDecoder(TransformerDecoder):
    def __init__(self, vocab_size: int, encoder_output_size: int, **kw):
        for k, want in (("input_layer", "embed"), ("normalize_before", True), ("concat_after", False),
                        ("use_output_layer", True)):
            if kw.get(k, want) != want:
                raise NotImplementedError(f"MLMDecoder({k}={kw[k]!r}) is outside the MI355X hot path (supported: {want!r})")
        super().__init__(vocab_size + 1, encoder_output_size, **kw)  # mlm_decoder.py: vocab_size += 1 for <mask>

    def _check_heads(self, what):
        if self.d % self.heads or self.d // self.heads not in (32, 64):
            raise NotImplementedError(f"{what}: heads of {self.d // self.heads} channels (d {self.d}, {self.heads} heads); "
                                      "the device path covers 32 and 64")

    def _memory_of(self, hs_pad, pk):
        self._mem = None
        mem = self._memory(hs_pad if hs_pad.size(0) > 1 else hs_pad[0:1], pk)
        self._mem = None
        return mem

    # ------------------------------------------------------------------ the reference's forward: scores of every position
    @torch.no_grad()
    def forward(self, hs_pad: torch.Tensor, hlens: torch.Tensor, ys_in_pad: torch.Tensor, ys_in_lens: torch.Tensor):
        """mlm_decoder.py MLMDecoder.forward (inference only): hs_pad (B, T, d) on the GPU, hlens (B,), ys_in_pad (B, L)
        token ids (`<mask>` = vocab_size - 1 where a token is hidden), ys_in_lens (B,) -> (scores before the softmax
        (B, L, V + 1) f32, ys_in_lens).  Rows at and behind a sentence's length are don't-care."""
        L.require_gpu(hs_pad, "hs_pad")
        self._check_heads("MLMDecoder.forward")
        hs_pad = hs_pad.contiguous()
        dev = hs_pad.device
        B, T, d = hs_pad.shape
        Lp = ys_in_pad.size(1)
        V, ff, act, dt = self.vocab_size, self.linear_units, self.act_dtype, self.em_dtype
        pk = self.packed(dev, Lp)
        mem = self._memory_of(hs_pad, pk)
        kl = torch.as_tensor(hlens).to(device=dev, dtype=torch.int32).contiguous()
        yl = torch.as_tensor(ys_in_lens).to(device=dev, dtype=torch.int32).contiguous()
        tok = ys_in_pad.to(device=dev, dtype=torch.int32).clamp_(0, V - 1).contiguous()
        M, w, lib, st = B * Lp, pk.w, L.load(), L.current_stream_ptr()
        x = torch.empty(M, d, dtype=torch.float32, device=dev)
        xn, ctx = (torch.empty(M, d, dtype=act, device=dev) for _ in range(2))
        qkv = torch.empty(M, 3 * d, dtype=act, device=dev)
        hb = torch.empty(M, ff, dtype=act, device=dev)
        out = torch.empty(B, Lp, V, dtype=torch.float32, device=dev)
        es = xn.element_size()

        def ln(g, b):
            L.check(lib.em_layernorm(dt, L.ptr(x), _vp(g), _vp(b), M, d, LN_EPS, L.ptr(xn), None, st), "em_layernorm")

        def gemm(epi, a, wt, c, bias, N, K):
            args = L.EmGemmArgs(A=a.data_ptr(), W=wt, C=c.data_ptr(), bias=bias, M=M, N=N, K=K, lda=K, ldc=N, scale=1.0)
            L.check(lib.em_gemm(dt, epi, L.EM_A_PLAIN, args, st), "em_gemm")

        L.check(lib.em_dec_seq_embed_f32(_vp(w.embed), _vp(w.pe), L.ptr(tok), M, V, d, Lp, w.pe_len, L.ptr(x), st),
                "em_dec_seq_embed_f32")
        for l in range(self.num_blocks):
            q = w.layers[l]
            kv = mem["mem_kv"].data_ptr() + l * B * T * 2 * d * es
            vT = mem["mem_vT"].data_ptr() + l * B * d * mem["Tpad"] * es
            ln(q.norm1_g, q.norm1_b)
            gemm(L.EM_EPI_STORE, xn, q.self_wqkv, qkv, q.self_bqkv, 3 * d, d)
            L.check(lib.em_dec_full_attention(dt, L.ptr(qkv), L.ptr(yl), B, Lp, d, self.heads, L.ptr(ctx), st),
                    "em_dec_full_attention")
            gemm(L.EM_EPI_RESID_F32, ctx, q.self_wout, x, q.self_bout, d, d)
            ln(q.norm2_g, q.norm2_b)
            gemm(L.EM_EPI_STORE, xn, q.src_wq, qkv, q.src_bq, d, d)
            L.check(lib.em_dec_seq_src_attention(dt, L.ptr(qkv), _vp(kv), 2 * d, _vp(vT), L.ptr(kl), None, B, B, Lp, d,
                                                 self.heads, T, mem["Tpad"], L.ptr(ctx), st), "em_dec_seq_src_attention")
            gemm(L.EM_EPI_RESID_F32, ctx, q.src_wout, x, q.src_bout, d, d)
            ln(q.norm3_g, q.norm3_b)
            gemm(L.EM_EPI_RELU, xn, q.w1, hb, q.b1, ff, d)
            gemm(L.EM_EPI_RESID_F32, hb, q.w2, x, q.b2, d, ff)
        ln(w.after_norm_g, w.after_norm_b)
        gemm(L.EM_EPI_STORE_F32, xn, w.out_w, out, w.out_b, V, d)
        return out, ys_in_lens

    # ------------------------------------------------------------------ the K mask-predict passes, one enqueued chain
    @torch.no_grad()
    def refine_workspace_bytes(self, device, B: int, Lp: int) -> int:
        """The workspace of `refine_device` for B sentences of Lp positions; 0: the shape is outside the device path."""
        pk = self.packed(torch.device(device), Lp)
        return int(L.load().em_maskctc_refine_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp))

    @torch.no_grad()
    def refine_device(self, hs_pad: torch.Tensor, hlens_dev: torch.Tensor, y_in: torch.Tensor, ylens: torch.Tensor,
                      nmask: torch.Tensor, n_iterations: int, trace: bool = False, ws: torch.Tensor = None, mem=None):
        """`em_maskctc_refine`: hs_pad (B, T, d) encoder memories on the GPU, hlens_dev (B,) int32 their valid frames;
        y_in (B, Lp) int32 contiguous, ylens / nmask (B,) int32 as `em_maskctc_collapse` leaves them (all on the device).
        y_in is refined IN PLACE through n_iterations passes; nothing is read back.  `trace`: also returns
        (y after each pass (K, B, Lp) int32, max logits (K, B, Lp) f32, arg-max (K, B, Lp) int32).  `ws`: a uint8 device
        tensor to use as the workspace (its contents do not matter), None: a fresh one.  `mem`: what `_memory_of(hs_pad, pk)`
        returned for these memories and this pack, when the caller holds it already (the projection is then not repeated)."""
        L.require_gpu(hs_pad, "hs_pad")
        K = int(n_iterations)
        if K < 1:
            raise NotImplementedError(f"maskctc_n_iterations={K}: the reference then fills one token per pass without a "
                                      "bound; the device chain has a fixed length (>= 1)")
        self._check_heads("MLMDecoder.refine_device")
        hs_pad = hs_pad.contiguous()
        dev = hs_pad.device
        B, T, _ = hs_pad.shape
        if y_in.dtype != torch.int32 or not y_in.is_contiguous() or y_in.dim() != 2 or y_in.size(0) != B:
            raise ValueError(f"y_in must be a contiguous int32 (B = {B}, Lp) device tensor")
        Lp = int(y_in.size(1))
        pk = self.packed(dev, Lp)
        lib = L.load()
        need = lib.em_maskctc_refine_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
        if need == 0:
            raise NotImplementedError(f"refine_device: a batch of {B} x {Lp} tokens is outside the device path's shapes; "
                                      "decode it in smaller batches")
        if mem is None:
            mem = self._memory_of(hs_pad, pk)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        yt = st_ = at = None
        if trace:
            yt = torch.empty(K, B, Lp, dtype=torch.int32, device=dev)
            st_ = torch.empty(K, B, Lp, dtype=torch.float32, device=dev)
            at = torch.empty(K, B, Lp, dtype=torch.int32, device=dev)
        L.check(lib.em_maskctc_refine(pk.dtype, C.byref(pk.w), L.ptr(mem["mem_kv"]), L.ptr(mem["mem_vT"]), L.ptr(hlens_dev),
                                      L.ptr(y_in), L.ptr(ylens), L.ptr(nmask), B, Lp, T, mem["Tpad"], K, self.vocab_size - 1,
                                      L.ptr(yt), L.ptr(st_), L.ptr(at), L.ptr(ws), ws.numel(), L.current_stream_ptr()),
                "em_maskctc_refine")
        return (yt, st_, at) if trace else None
