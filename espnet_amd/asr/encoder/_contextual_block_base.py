"""The host state machine the two contextual-block streaming encoders share (ContextualBlockConformerEncoder,
ContextualBlockTransformerEncoder): in the reference, `forward_infer` of espnet2/asr/encoder/contextual_block_conformer_encoder.py
:386-600 and of contextual_block_transformer_encoder.py are the same code - the buffers before / after the 4x subsampling, block
counting, block assembly with StreamPositionalEncoding and the two context slots, the short-utterance path, output stitching
and the carried state dictionary - around layer stacks that differ.  A subclass supplies its parameter containers,
`_build_pack` (a pack whose `w` has conv1_w / conv1_b / conv2_w / conv2_b / embed_w / embed_b / after_norm_g / after_norm_b,
plus `pe`), and the names of its three C entries.  One stream is a batch of one: `forward_infer_batch` is the state machine,
`forward_infer` its adapter to the reference's interface.  `StreamingStepGraph` replays a single stream's steady-state call
as a hipGraph, for either encoder.
"""
import ctypes as C
import math
from typing import Optional, Tuple

import torch

from espnet_amd import lib as L
from espnet_amd.packing import PackedModule

LN_EPS = 1e-12


class ContextualBlockEncoderBase(PackedModule):
    # C entries of the layer stack (include/espnet_amd.h): workspace size, one stream, a batch of lock-step streams
    _WS_FN, _ENC_FN, _ENC_BATCH_FN = None, None, None

    def output_size(self) -> int:
        return self._output_size

    @property
    def em_dtype(self) -> int:
        return L.DTYPES[self.compute_dtype]

    # ------------------------------------------------------------------ device pieces
    def _embed_device_batch(self, pk, xs: torch.Tensor) -> torch.Tensor:
        """Conv2dSubsamplingWOPosEnc.forward for S streams at once: xs (S, t, idim) f32 on the GPU -> (S, t', d)."""
        lib, w = L.load(), pk.w
        S, t, nm = xs.shape
        d = self._output_size
        T1, F1 = (t - 3) // 2 + 1, (nm - 3) // 2 + 1
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        dev, act, st = xs.device, self.act_dtype, L.current_stream_ptr()
        # (a batch's ticks repeat their shapes: filled once, not per tick.  The launch below reads `flen` only together with
        # the utterance-MVN partial sums, which this path never passes - so a captured graph that holds an entry's
        # address stays valid after the entry is evicted)
        flen = self._flen_cache.get((S, t, dev))
        if flen is None:
            if len(self._flen_cache) > 64:
                self._flen_cache.clear()
            flen = self._flen_cache[(S, t, dev)] = torch.full((S,), t, dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()  # (filled before another stream's tick may read it)
        c1 = torch.empty(S * T1 * F1 * d, dtype=act, device=dev)
        L.check(lib.em_conv2d_sub1(self.em_dtype, L.ptr(xs), None, L.ptr(flen), S, t, nm, w.conv1_w,
                                   w.conv1_b, d, L.ptr(c1), st), "em_conv2d_sub1")
        c2 = torch.empty(S * T2 * F2 * d, dtype=act, device=dev)
        a = L.EmGemmArgs(A=c1.data_ptr(), W=w.conv2_w, C=c2.data_ptr(), bias=w.conv2_b, M=S * T2 * F2, N=d,
                         K=9 * d, lda=0, ldc=d, scale=1.0, T1=T1, F1=F1, T2=T2, F2=F2, d=d)
        L.check(lib.em_gemm(self.em_dtype, L.EM_EPI_RELU, L.EM_A_CONV2, a, st), "em_gemm(conv2)")
        out = torch.empty(S, T2, d, dtype=torch.float32, device=dev)
        a = L.EmGemmArgs(A=c2.data_ptr(), W=w.embed_w, C=out.data_ptr(), bias=w.embed_b, M=S * T2, N=d,
                         K=F2 * d, lda=F2 * d, ldc=d, scale=1.0)
        L.check(lib.em_gemm(self.em_dtype, L.EM_EPI_SCALE_F32, L.EM_A_PLAIN, a, st), "em_gemm(embed.out)")
        return out

    def _workspace(self, pk, dev, n_blk, Lb):
        need = getattr(L.load(), self._WS_FN)(self.em_dtype, C.byref(pk.w), n_blk, Lb)
        key = (torch.cuda.current_stream().cuda_stream, n_blk, Lb)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._ws[key] = ws
        return ws

    def _after_norm(self, pk, ys: torch.Tensor) -> torch.Tensor:
        w = pk.w
        L.check(L.load().em_layernorm_inplace_f32(L.ptr(ys), w.after_norm_g, w.after_norm_b,
                                                  ys.size(0), ys.size(1), LN_EPS,
                                                  L.current_stream_ptr()), "after_norm")
        return ys

    # ------------------------------------------------------------------ reference entry points
    def forward(self, xs_pad, ilens, prev_states=None, is_final=True, infer_mode=False):
        if not infer_mode:
            raise NotImplementedError("forward_train (full-utterance block processing used in "
                                      "training) is outside the inference hot path")
        return self.forward_infer(xs_pad, ilens, prev_states, is_final)

    def _empty_out(self, dev):
        e = self.__dict__.get("_empty_cache")
        if e is None or e[0].device != dev:
            e = self._empty_cache = (torch.zeros(1, 0, self._output_size, device=dev), torch.zeros(1, device=dev))
        return e

    def _olen_out(self, dev, n):
        c = self.__dict__.setdefault("_olen_cache", {})
        t = c.get((dev, n))
        if t is None:
            if len(c) > 256:
                c.clear()
            t = c[(dev, n)] = torch.full((1,), float(n), device=dev)
            torch.cuda.current_stream().synchronize()  # (filled before any stream may read it)
        return t

    def forward_infer(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None,
                      is_final: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[dict]]:
        """contextual_block_conformer_encoder.py:386-600.  xs_pad (1, t, idim) f32 ON THE GPU.  One stream is a batch of
        one: the state machine below, with the stream dimension put on the carried buffers on the way in and taken off
        what the call made on the way out (views, no launch).  The state dictionary is the reference's - tensors without
        a stream dimension, `ilens_buffer` - and the lengths come back as the reference returns them, f32 (1,) on the
        device."""
        assert xs_pad.size(0) == 1
        dev = xs_pad.device
        carried = ("prev_addin", "buffer_before_downsampling", "buffer_after_downsampling", "past_encoder_ctx")
        st = dict(prev_states) if prev_states else None
        if st is not None:
            st.update((k, st[k].unsqueeze(0)) for k in carried if st.get(k) is not None)
        ys, y_len, nst, short = self._infer_batch(xs_pad, st, is_final)
        if nst is None:  # (a short utterance (:496-505) reports length 0, as it always has)
            return ys, self._olen_out(dev, 0 if short else y_len), None
        nst["ilens_buffer"] = torch.tensor([nst["buffer_before_downsampling"].size(1)])
        nst.update((k, nst[k][0]) for k in carried if nst[k] is not None)
        if ys is None:  # (the call only buffered; cached: two fills per call otherwise)
            return (*self._empty_out(dev), nst)
        return ys, self._olen_out(dev, y_len), nst

    # ------------------------------------------------------------------ a batch of lock-step streams
    @torch.no_grad()
    def forward_infer_batch(self, xs_pad: torch.Tensor, prev_states=None, is_final: bool = False):
        """`forward_infer` (contextual_block_conformer_encoder.py:386-600) for S streams whose carried buffers have the
        same SHAPES: every stream is fed a chunk of the same length at this call (a server batching its live
        connections) and they agree on the buffer lengths and on whether they have processed a block yet; the NUMBER
        of blocks a stream has processed may differ per stream (`n_processed_blocks` a list of S ints: streams that
        joined at different times - it only moves the positional-encoding offsets, em_cb_build_blocks_rows_f32).
        Streams in different phases are grouped by `espnet_amd.bin.asr_inference_streaming.StreamPool`.
        xs_pad (S, t, idim) f32 ON THE GPU.  Returns (ys (S, t_out, d), t_out, state); row s equals what
        `forward_infer` - the same state machine with S = 1 - returns for stream s alone (tests/test_gpu_streaming.py::
        test_batch_of_streams).  The dense operators of a call see S * n_blk independent blocks - one launch sequence
        for all streams."""
        ys, y_len, nst, _ = self._infer_batch(xs_pad, prev_states, is_final)
        if ys is None:
            ys = torch.zeros(xs_pad.size(0), 0, self._output_size, device=xs_pad.device)
        return ys, y_len, nst

    def _infer_batch(self, xs_pad: torch.Tensor, prev_states, is_final: bool):
        """The state machine: (ys, y_len, state, short utterance).  A call that only buffers returns (None, 0, state,
        False); the state dictionary is a new one."""
        L.require_gpu(xs_pad, "xs_pad")
        dev = xs_pad.device
        pk = self.packed(dev)
        lib = L.load()
        S = xs_pad.size(0)
        d, bs, hs, la, sub = self._output_size, self.block_size, self.hop_size, self.look_ahead, self.subsample
        st = prev_states or dict(prev_addin=None, buffer_before_downsampling=None, buffer_after_downsampling=None,
                                 n_processed_blocks=0, past_encoder_ctx=None)
        prev_addin, buf_after = st["prev_addin"], st["buffer_after_downsampling"]
        n_proc, past_ctx = st["n_processed_blocks"], st["past_encoder_ctx"]
        n_rows = None  # per-stream block counts (all zero or all positive: the callers group streams that way)
        if isinstance(n_proc, (list, tuple)):
            n_rows = [int(v) for v in n_proc]
            if len(n_rows) != S or (min(n_rows) == 0) != (max(n_rows) == 0):
                raise ValueError("n_processed_blocks: one count per stream, all zero or all positive")
            n_proc = n_rows[0] if len(set(n_rows)) == 1 else (1 if n_rows[0] > 0 else 0)
            if len(set(n_rows)) == 1:
                n_rows = None
        xs = xs_pad.to(torch.float32)
        if st["buffer_before_downsampling"] is not None:
            xs = torch.cat([st["buffer_before_downsampling"], xs], dim=1)
        if is_final:
            buf_before = None
        else:
            n_samples = xs.size(1) // sub - 1
            if n_samples < 2:  # :424-438
                return None, 0, dict(st, buffer_before_downsampling=xs), False
            n_res = xs.size(1) % sub + sub * 2
            buf_before = xs[:, xs.size(1) - n_res:].contiguous()
            xs = xs[:, : n_samples * sub]
        x = self._embed_device_batch(pk, xs.contiguous())
        if buf_after is not None:
            x = torch.cat([buf_after, x], dim=1)
        total = x.size(1)
        if is_final:
            block_num = math.ceil(float(total - (bs - hs - la) - la) / float(hs))
            buf_after = None
        else:
            if total <= bs:  # :474-487
                return None, 0, dict(prev_addin=prev_addin, buffer_before_downsampling=buf_before,
                                     buffer_after_downsampling=x, n_processed_blocks=st["n_processed_blocks"],
                                     past_encoder_ctx=past_ctx), False
            overlap = bs - hs
            block_num = max(0, total - overlap) // hs
            res = total - hs * block_num
            buf_after = x[:, total - res:].contiguous()
            x = x[:, : block_num * hs + overlap]
        x = x.contiguous()
        stream = L.current_stream_ptr()
        if n_proc == 0 and total <= bs and is_final:  # short utterances (:496-505): no context slots
            xc = torch.empty(S, total, d, dtype=torch.float32, device=dev)
            for s_ in range(S):  # (rare path: one launch per stream)
                L.check(lib.em_stream_pos_enc_f32(L.ptr(x[s_]), L.ptr(pk.pe), 0, total, d, L.ptr(xc[s_]), stream),
                        "em_stream_pos_enc_f32")
            ws = self._workspace(pk, dev, S, total)
            L.check(getattr(lib, self._ENC_FN)(self.em_dtype, C.byref(pk.w), L.ptr(xc), S, total, 0, None, None,
                                            L.ptr(ws), ws.numel(), stream), self._ENC_FN)
            return self._after_norm(pk, xc.view(S * total, d)).view(S, total, d), total, None, True
        Lb = bs + 2
        chunks = torch.empty(S, block_num, Lb, d, dtype=torch.float32, device=dev)
        addin = torch.empty(S, d, dtype=torch.float32, device=dev)
        rows_static = st.get("n_processed_blocks_dev")  # (S,) int32 on the device: set by a captured call only (StreamingStepGraph, BatchTickGraph)
        if rows_static is not None:
            L.check(lib.em_cb_build_blocks_rows_f32(L.ptr(x), L.ptr(pk.pe), L.ptr(prev_addin), L.ptr(rows_static), S,
                                                    block_num, x.size(1), bs, hs, d, L.ptr(chunks), L.ptr(addin), stream),
                    "em_cb_build_blocks_rows_f32")
        elif n_rows is None:
            L.check(lib.em_cb_build_blocks_batch_f32(L.ptr(x), L.ptr(pk.pe), L.ptr(prev_addin), n_proc, S, block_num,
                                                     x.size(1), bs, hs, d, L.ptr(chunks), L.ptr(addin), stream),
                    "em_cb_build_blocks_batch_f32")
        else:
            rows_dev = torch.tensor(n_rows, dtype=torch.int32).to(dev, non_blocking=True)
            L.check(lib.em_cb_build_blocks_rows_f32(L.ptr(x), L.ptr(pk.pe), L.ptr(prev_addin), L.ptr(rows_dev), S,
                                                    block_num, x.size(1), bs, hs, d, L.ptr(chunks), L.ptr(addin), stream),
                    "em_cb_build_blocks_rows_f32")
        next_ctx = torch.empty(S, self.num_blocks, d, dtype=torch.float32, device=dev)
        ws = self._workspace(pk, dev, S * block_num, Lb)
        L.check(getattr(lib, self._ENC_BATCH_FN)(self.em_dtype, C.byref(pk.w), L.ptr(chunks), S, block_num, Lb, 1,
                                              L.ptr(past_ctx), L.ptr(next_ctx), L.ptr(ws), ws.numel(), stream),
                self._ENC_BATCH_FN)
        ys_chunk = chunks[:, :, 1 : bs + 1]
        offset = bs - la - hs
        if is_final:
            y_len = x.size(1) if n_proc == 0 else x.size(1) - offset
        else:
            y_len = block_num * hs + (offset if n_proc == 0 else 0)
        # (not final: the head piece and the blocks' hops below tile [0, y_len) exactly - nothing to clear)
        ys = (torch.zeros if is_final else torch.empty)(S, y_len, d, dtype=torch.float32, device=dev)
        if n_proc == 0:
            ys[:, :offset] = ys_chunk[:, 0, :offset]
        for i in range(block_num):  # :565-576 (slicing only)
            cur = i * hs + (offset if n_proc == 0 else 0)
            clen = min(bs - offset, y_len - cur) if (i == block_num - 1 and is_final) else hs
            ys[:, cur : cur + clen] = ys_chunk[:, i, offset : offset + clen]
        ys = self._after_norm(pk, ys.view(S * y_len, d)).view(S, y_len, d)
        if is_final:
            return ys, y_len, None, False
        n_next = n_proc + block_num if n_rows is None else [v + block_num for v in n_rows]
        return ys, y_len, dict(prev_addin=addin, buffer_before_downsampling=buf_before,
                               buffer_after_downsampling=buf_after, n_processed_blocks=n_next,
                               past_encoder_ctx=next_ctx), False


class StreamingStepGraph:
    """hipGraph replay of the steady-state streaming step (BASELINE config 5).

    Feeding fixed-size chunks, `forward_infer` reaches a steady state after a few calls: the carried
    buffers keep their shapes and every call processes the same number of blocks, so the ~200
    kernel launches of a call are identical except for the positional-encoding offset (read from
    device memory).  This wrapper runs the encoder eagerly until two consecutive calls have the same
    signature, captures the next call into a hipGraph (torch.cuda.CUDAGraph = hipGraph on ROCm)
    over static input / state buffers, and from then on replays it: one graph launch per chunk.
    `is_final` calls and any call whose chunk size differs fall back to the eager path.
    """

    def __init__(self, encoder: ContextualBlockEncoderBase, chunk_frames: int = 0):
        # chunk_frames is only a hint: the graph is captured for whatever chunk size repeats
        self.enc, self.chunk, self.last_size = encoder, chunk_frames, -1
        self.state, self.graph, self.graph_sig = None, None, None
        self.in_graph_state = False
        self.n_replays = 0

    @staticmethod
    def _signature(st):
        return (tuple(st["buffer_before_downsampling"].shape), tuple(st["buffer_after_downsampling"].shape),
                st["prev_addin"] is not None, st["past_encoder_ctx"] is not None)

    def reset(self):
        self.state = None  # the captured graph stays valid for the next utterance
        self.in_graph_state = False

    def _capture(self, feats):
        st = self.state
        dev = feats.device
        self.s_in = feats.clone()
        self.s_state = dict(
            prev_addin=st["prev_addin"].clone(),
            buffer_before_downsampling=st["buffer_before_downsampling"].clone(),
            ilens_buffer=st["ilens_buffer"],
            buffer_after_downsampling=st["buffer_after_downsampling"].clone(),
            n_processed_blocks=1,  # > 0: steady state; the real count lives on the device
            n_processed_blocks_dev=torch.tensor([st["n_processed_blocks"]], dtype=torch.int32, device=dev),
            past_encoder_ctx=st["past_encoder_ctx"].clone())
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream (allocator, workspaces)
            self.enc.forward_infer(self.s_in[None], torch.tensor([self.chunk]), dict(self.s_state), False)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ys, _, nst = self.enc.forward_infer(self.s_in[None], torch.tensor([self.chunk]),
                                                dict(self.s_state), False)
            # carry the state forward inside the graph (static buffers, same shapes)
            self.s_state["prev_addin"].copy_(nst["prev_addin"])
            self.s_state["buffer_before_downsampling"].copy_(nst["buffer_before_downsampling"])
            self.s_state["buffer_after_downsampling"].copy_(nst["buffer_after_downsampling"])
            self.s_state["past_encoder_ctx"].copy_(nst["past_encoder_ctx"])
            self.s_state["n_processed_blocks_dev"].add_(nst["n_processed_blocks"] - 1)
        self.graph, self.s_out = g, ys
        self.blocks_per_call = nst["n_processed_blocks"] - 1

    def _load_static_state(self):
        st = self.state
        for k in ("prev_addin", "buffer_before_downsampling", "buffer_after_downsampling", "past_encoder_ctx"):
            self.s_state[k].copy_(st[k])
        self.s_state["n_processed_blocks_dev"].fill_(st["n_processed_blocks"])

    @torch.no_grad()
    def __call__(self, feats: torch.Tensor, is_final: bool = False):
        """feats (t, idim) f32 on the GPU.  Returns ys (t_out, d) f32 (a view of a static buffer
        when replayed: consume or clone it before the next call)."""
        if self.graph is None and feats.size(0) == self.last_size:
            self.chunk = feats.size(0)  # a repeating chunk size: this is the one worth capturing
        self.last_size = feats.size(0)
        steady = (not is_final and feats.size(0) == self.chunk and self.state is not None
                  and self.state["past_encoder_ctx"] is not None
                  and self.state["buffer_after_downsampling"] is not None)
        if steady and self.graph is not None and self._signature(self.state) == self.graph_sig:
            if not self.in_graph_state:
                self._load_static_state()
                self.in_graph_state = True
            self.s_in.copy_(feats)
            self.graph.replay()
            self.n_replays += 1
            self.state["n_processed_blocks"] += self.blocks_per_call
            return self.s_out[0]
        if self.in_graph_state:  # leave graph mode: pull the state back out
            for k in ("prev_addin", "buffer_before_downsampling", "buffer_after_downsampling", "past_encoder_ctx"):
                self.state[k] = self.s_state[k].clone()
            self.in_graph_state = False
        prev_sig = self._signature(self.state) if steady else None
        ys, _, nst = self.enc.forward_infer(feats[None], torch.tensor([feats.size(0)]), self.state, is_final)
        self.state = nst
        if (steady and self.graph is None and nst is not None and prev_sig == self._signature(nst)):
            self.graph_sig = prev_sig
            self._capture(feats)
            self.in_graph_state = False
        return ys[0]
