"""CTC head on the MI355X.  Mirrors espnet2/asr/ctc.py:9-215 for inference (`ctc_lo`,
`softmax`/`log_softmax`/`argmax`, `forced_align`); state-dict keys `ctc_lo.{weight,bias}`.  Of the loss only the
per-utterance value exists (`nll`: scoring given transcripts); gradients and the reduced training loss are out of scope."""
import os

import torch

from espnet_amd import lib as L
from espnet_amd.packing import PackedModule


class CTC(PackedModule):
    def __init__(self, odim: int, encoder_output_size: int, dropout_rate: float = 0.0,
                 ctc_type: str = "builtin", reduce: bool = True, ignore_nan_grad: bool = None,
                 zero_infinity: bool = True, brctc_risk_strategy: str = "exp",
                 brctc_group_strategy: str = "end", brctc_risk_factor: float = 0.0,
                 compute_dtype: str = "bfloat16"):
        super().__init__()
        self.odim, self.eprojs = odim, encoder_output_size
        self.dropout_rate = dropout_rate
        self.ctc_lo = torch.nn.Linear(encoder_output_size, odim)  # parameter container
        self.ctc_type = ctc_type
        self.compute_dtype = compute_dtype

    @property
    def em_dtype(self):
        return L.DTYPES[self.compute_dtype]

    def _build_pack(self, pk):
        pk.weight, pk.bias = pk.A(self.ctc_lo.weight), pk.F(self.ctc_lo.bias)

    def _to_act(self, hs_pad: torch.Tensor) -> torch.Tensor:
        L.require_gpu(hs_pad, "hs_pad")
        if hs_pad.dtype == self.act_dtype:
            return hs_pad.contiguous()
        src = hs_pad.to(torch.float32).contiguous()
        dst = torch.empty(src.shape, dtype=self.act_dtype, device=src.device)
        L.check(L.load().em_cast_f32(self.em_dtype, L.ptr(src), src.numel(), L.ptr(dst),
                                     L.current_stream_ptr()), "em_cast_f32")
        return dst

    def logits_device(self, enc_act: torch.Tensor) -> torch.Tensor:
        """enc_act (B,T,d) in the compute dtype -> logits (B,T,V) f32."""
        p = self.packed(enc_act.device)
        B, T, d = enc_act.shape
        out = torch.empty(B, T, self.odim, dtype=torch.float32, device=enc_act.device)
        a = L.EmGemmArgs(A=enc_act.data_ptr(), W=p.weight.data_ptr(), C=out.data_ptr(),
                         bias=p.bias.data_ptr(), M=B * T, N=self.odim, K=d, lda=d, ldc=self.odim,
                         scale=1.0)
        L.check(L.load().em_gemm(self.em_dtype, L.EM_EPI_STORE_F32, L.EM_A_PLAIN, a,
                                 L.current_stream_ptr()), "em_gemm(ctc_lo)")
        return out

    def log_softmax(self, hs_pad: torch.Tensor) -> torch.Tensor:
        """asr/ctc.py:197-205."""
        logits = self.logits_device(self._to_act(hs_pad))
        B, T, V = logits.shape
        L.check(L.load().em_log_softmax_rows_f32(L.ptr(logits), B * T, V, L.current_stream_ptr()),
                "em_log_softmax_rows_f32")
        return logits

    def argmax(self, hs_pad: torch.Tensor, as_int32: bool = False) -> torch.Tensor:
        """asr/ctc.py:207-215.  Returns (B, T) int64 like the reference (`as_int32`: the kernel's own int32 ids, for
        callers that read them back to the host anyway - one conversion launch less per streaming tick)."""
        act = self._to_act(hs_pad)
        B, T, d = act.shape
        V, dev, st = self.odim, act.device, L.current_stream_ptr()
        ids = torch.empty(B, T, dtype=torch.int32, device=dev)
        if d % 64 != 0 or os.environ.get("ESPNET_AMD_CTC_ARGMAX_LOGITS"):
            # the (B, T, V) f32 logits written and read back (rounds 1-4; developer A/B switch; widths the arg-max
            # epilogue's GEMM does not take)
            logits = self.logits_device(act)
            L.check(L.load().em_argmax_rows_f32(L.ptr(logits), B * T, V, L.ptr(ids), st), "em_argmax_rows_f32")
            return ids if as_int32 else ids.to(torch.int64)
        # round 5: arg-max in the epilogue of the ctc_lo GEMM, as em_ctc_greedy has it - the logits never exist (10 MB per
        # tick of a 32-stream batch, 26.5 + 26.1 us of its 1.25 ms: profiles/r05x_stream_batch32_kernel_stats.csv); only
        # (value, column) pairs per 64 columns are written and reduced.  Same values compared, ties to the lowest column.
        p = self.packed(dev)
        G = 2 * ((V + 127) // 128)
        part = torch.empty(B * T * G * 2, dtype=torch.float32, device=dev)
        a = L.EmGemmArgs(A=act.data_ptr(), W=p.weight.data_ptr(), C=part.data_ptr(), bias=p.bias.data_ptr(), M=B * T, N=V,
                         K=d, lda=d, ldc=G, scale=1.0)
        L.check(L.load().em_gemm(self.em_dtype, L.EM_EPI_ARGMAX_PART, L.EM_A_PLAIN, a, st), "em_gemm(ctc_lo, arg-max)")
        L.check(L.load().em_argmax_partials(L.ptr(part), B * T, G, L.ptr(ids), st), "em_argmax_partials")
        return ids if as_int32 else ids.to(torch.int64)

    def frame_top_device(self, hs_pad: torch.Tensor):
        """Per frame the arg-max id and its probability, exp(max_v log_softmax) (`em_ctc_frame_top`, csrc/vocab_head.hip: the
        logits never exist): hs_pad (B, T, d) on the GPU -> (ids (B, T) int32, prob (B, T) f32).  Only enqueues."""
        act = self._to_act(hs_pad)
        B, T, d = act.shape
        p, dev, lib = self.packed(act.device), act.device, L.load()
        ids = torch.empty(B, T, dtype=torch.int32, device=dev)
        prob = torch.empty(B, T, dtype=torch.float32, device=dev)
        need = lib.em_ctc_frame_top_workspace_bytes(self.em_dtype, B * T, self.odim)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        L.check(lib.em_ctc_frame_top(self.em_dtype, L.ptr(act), L.ptr(p.weight), L.ptr(p.bias), B * T, self.odim, d,
                                     L.ptr(ids), L.ptr(prob), L.ptr(ws), need, L.current_stream_ptr()), "em_ctc_frame_top")
        return ids, prob

    def frame_topk_device(self, hs_pad: torch.Tensor, K: int, blank: int = 0):
        """Per frame the K most probable tokens of `log_softmax(hs_pad)` (`em_ctc_frame_topk`, csrc/ctc_tsync.hip): hs_pad
        (B, T, d) on the GPU -> (cand_id (B, T, K) int32, cand_lp (B, T, K) f32 descending, ties to the lower id, blank_lp
        (B, T) f32).  What the time-synchronous search reads (espnet_amd/nets/beam_search_timesync.py).  Only enqueues."""
        return self.topk_log_probs(self.log_softmax(hs_pad), K, blank)

    @staticmethod
    def topk_log_probs(lp: torch.Tensor, K: int, blank: int = 0):
        """`em_ctc_frame_topk` on given log-probabilities lp (..., V) f32 on the device."""
        L.require_gpu(lp, "lp")
        if lp.dtype != torch.float32:
            raise ValueError("lp must be float32")
        lp = lp.contiguous()
        V = int(lp.shape[-1])
        lead = tuple(lp.shape[:-1])
        M = lp.numel() // V if V else 0
        if not 1 <= int(K) <= V:
            raise ValueError(f"K must lie in [1, {V}], not {K}")
        cand_id = torch.empty(lead + (int(K),), dtype=torch.int32, device=lp.device)
        cand_lp = torch.empty(lead + (int(K),), dtype=torch.float32, device=lp.device)
        blank_lp = torch.empty(lead, dtype=torch.float32, device=lp.device)
        L.check(L.load().em_ctc_frame_topk(L.ptr(lp), M, V, int(K), int(blank), L.ptr(cand_id), L.ptr(cand_lp), L.ptr(blank_lp),
                                           L.current_stream_ptr()), "em_ctc_frame_topk")
        return cand_id, cand_lp, blank_lp

    # ------------------------------------------------------------------ forced alignment (csrc/ctc_align.hip)
    @staticmethod
    def check_alignable(olens, targets, blank, vocab):
        """The host-side checks of a forced alignment, before anything is launched: every id in [0, vocab) and not the
        blank, and enough frames for the tokens (T_b >= L_b + number of adjacent equal tokens).  `targets`: one list
        of ids per utterance.  Raises ValueError."""
        for b, (T_b, y) in enumerate(zip(olens, targets)):
            y = [int(v) for v in y]
            if any(v == blank for v in y):
                raise ValueError(f"utterance {b}: the blank id {blank} cannot be aligned")
            if any(v < 0 or v >= vocab for v in y):
                raise ValueError(f"utterance {b}: token ids must lie in [0, {vocab})")
            need = len(y) + sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])
            if int(T_b) < max(need, 1):
                raise ValueError(f"utterance {b}: {int(T_b)} encoder frames cannot carry {len(y)} tokens "
                                 f"({need} frames needed)")

    def _trellis_inputs(self, enc_act, olens, targets, ylens, blank, mem_of, align: bool):
        """The arguments of `forced_align_device` (align: one transcript per utterance, enough frames for it) and
        `nll_device` (N transcripts, mem_of or None) as device tensors: all HOST data is checked and copied over, all
        int32 DEVICE tensors are taken as they are, a mixture is refused.  Returns (olens_d, tg_d, ylens_d, mem_of_d or
        None, N, Lmax); tg_d's row stride is max(Lmax, 1)."""
        Bm, T, _ = enc_act.shape
        dev = enc_act.device
        given = (olens, targets, ylens) + (() if mem_of is None else (mem_of,))
        names = ["olens", "targets", "ylens"] + ([] if align else ["mem_of"])
        on_dev = [torch.is_tensor(x) and x.is_cuda for x in given]
        if all(on_dev):
            if any(x.dtype != torch.int32 for x in given) or targets.dim() != 2:
                raise ValueError(f"device-side {' / '.join(names)} must be int32, targets ({'B' if align else 'N'}, Lmax)")
            olens_d, tg_d, ylens_d = olens.contiguous(), targets.contiguous(), ylens.contiguous()
            mo_d = None if mem_of is None else mem_of.contiguous()
            N, Lmax = int(targets.shape[0]), int(targets.shape[1])
            if not align and (int(olens_d.numel()) != Bm or int(ylens_d.numel()) != N
                              or (mo_d is not None and int(mo_d.numel()) != N)):
                raise ValueError(f"olens must have {Bm} entries, ylens and mem_of {N}")
            return olens_d, tg_d, ylens_d, mo_d, N, Lmax
        if any(on_dev):
            raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} must be all host data or all device tensors")
        ol, rows, yl, mo = [x.tolist() if torch.is_tensor(x) else list(x) for x in given] + ([None] if mem_of is None else [])
        N = len(rows)
        if align:
            if len(ol) != Bm or len(yl) != Bm or N != Bm:
                raise ValueError(f"olens, targets and ylens must have {Bm} rows")
        elif len(ol) != Bm or len(yl) != N or (mo is not None and len(mo) != N):
            raise ValueError(f"olens must have {Bm} entries, ylens and mem_of as many as targets ({N})")
        if any(n < 0 or n > len(r) for n, r in zip(yl, rows)) or any(n < 0 or n > T for n in ol):
            raise ValueError("a length lies outside its row")
        if mo is not None and any(u < 0 or u >= Bm for u in mo):
            raise ValueError(f"mem_of must lie in [0, {Bm})")
        rows = [[int(v) for v in r[:n]] for r, n in zip(rows, yl)]
        # (the likelihood checks the ids only: too few frames give +inf there, not an error)
        self.check_alignable(ol if align else [2 ** 31] * N, rows, blank, self.odim)
        Lmax = max(yl) if yl else 0
        tg = torch.zeros(max(N, 1), max(Lmax, 1), dtype=torch.int32)
        for n, r in enumerate(rows):
            tg[n, : len(r)] = torch.tensor(r, dtype=torch.int32)
        olens_d, ylens_d, tg_d = (torch.as_tensor(v, dtype=torch.int32).to(dev, non_blocking=True) for v in (ol, yl, tg))
        mo_d = None if mo is None else torch.tensor(mo, dtype=torch.int32).to(dev, non_blocking=True)
        return olens_d, tg_d, ylens_d, mo_d, N, Lmax

    def forced_align_device(self, enc_act: torch.Tensor, olens, targets, ylens, blank: int):
        """Viterbi alignment of `targets` to the CTC posteriors of enc_act (B,T,d) (compute dtype, on the device) for a
        ragged batch, by `em_ctc_log_probs_t` -> `em_ctc_forced_align` (include/espnet_amd.h states the recursion and
        the tie rule).  Returns (align (B,T) i32, frame_lp (B,T) f32, tok_start, tok_end (B,Lmax) i32, tok_lp (B,Lmax)
        f32, total (B,) f32) as device tensors, no host sync.

        olens / ylens: per-utterance lengths, targets (B, Lmax) ids padded with anything.  Given as HOST data (lists or
        CPU tensors) they are checked first (`check_alignable`: ValueError before any launch) and copied over; given as
        int32 DEVICE tensors they are taken as they are - for ids the device produced itself (the greedy CTC tokens),
        which are valid by construction."""
        L.require_gpu(enc_act, "enc_act")
        B, T, _ = enc_act.shape
        olens_d, tg_d, ylens_d, _, _, Lmax = self._trellis_inputs(enc_act, olens, targets, ylens, blank, None, align=True)
        return self.align_log_probs_t(self.log_probs_t_device(enc_act), B * T, olens_d, tg_d, Lmax, ylens_d, B, T, blank)

    @staticmethod
    def align_log_probs_t(lpT, ldT, olens_d, tg_d, Lmax, ylens_d, B, T, blank, ws_bytes=None):
        """`em_ctc_forced_align` on given transposed log-posteriors lpT [V][ldT] (device tensors throughout)."""
        lib, dev = L.load(), lpT.device
        if ws_bytes is None:
            ws_bytes = int(lib.em_ctc_forced_align_workspace_bytes(B, T, Lmax))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        Lp = max(Lmax, 1)
        align = torch.empty(B, T, dtype=torch.int32, device=dev)
        frame_lp = torch.empty(B, T, dtype=torch.float32, device=dev)
        tok_start = torch.empty(B, Lp, dtype=torch.int32, device=dev)
        tok_end = torch.empty(B, Lp, dtype=torch.int32, device=dev)
        tok_lp = torch.empty(B, Lp, dtype=torch.float32, device=dev)
        total = torch.empty(B, dtype=torch.float32, device=dev)
        L.check(lib.em_ctc_forced_align(L.ptr(lpT), ldT, L.ptr(olens_d), L.ptr(tg_d), Lmax, L.ptr(ylens_d), B, T, blank,
                                        L.ptr(align), L.ptr(frame_lp), L.ptr(tok_start), L.ptr(tok_end), L.ptr(tok_lp),
                                        L.ptr(total), L.ptr(ws), ws_bytes, L.current_stream_ptr()), "em_ctc_forced_align")
        return align, frame_lp, tok_start[:, :Lmax], tok_end[:, :Lmax], tok_lp[:, :Lmax], total

    def forced_align(self, hs_pad: torch.Tensor, hlens, ys_pad, ylens, blank_idx: int = 0) -> torch.Tensor:
        """CTC.forced_align of the reference (espnet2/asr/ctc.py; there a wrapper of
        torchaudio.functional.forced_align for ONE utterance): hs_pad (B,T,d) encoder output on the device, hlens (B,),
        ys_pad (B,Lmax) target ids, ylens (B,).  Returns the (B,T) int64 frame labels of the best path, -1 beyond
        hlens[b].  Any B is taken.  Where two moves tie exactly the smaller one is kept (include/espnet_amd.h;
        torchaudio's CPU loop takes neither move when both beat staying and are equal): identical on inputs without
        exact ties."""
        act = self._to_act(hs_pad)
        host = [x.cpu() if torch.is_tensor(x) else x for x in (hlens, ys_pad, ylens)]
        return self.forced_align_device(act, host[0], host[1], host[2], int(blank_idx))[0].to(torch.int64)

    # ------------------------------------------------------------------ segmentation (csrc/ctc_segment.hip)
    @staticmethod
    def check_segmentable(olens, gt, clens, vocab, T=None):
        """The host-side checks of a segmentation, before anything is launched: lengths inside their rows, C_b >= 2,
        C_b - 1 <= T_b, every id of the columns 1 .. C_b - 1 in [0, vocab) (the blank is allowed: separators).  `gt`: one
        list of columns per recording.  Raises ValueError."""
        for b, (T_b, row, C_b) in enumerate(zip(olens, gt, clens)):
            T_b, C_b = int(T_b), int(C_b)
            if C_b > len(row) or T_b < 0 or (T is not None and T_b > T):
                raise ValueError(f"recording {b}: a length lies outside its row")
            if C_b < 2:
                raise ValueError(f"recording {b}: {C_b} ground-truth columns (the start symbol and at least one more are needed)")
            if C_b - 1 > T_b:
                raise ValueError(f"recording {b}: {T_b} encoder frames cannot carry {C_b - 1} ground-truth columns")
            if any(int(v) < 0 or int(v) >= vocab for v in row[1:C_b]):
                raise ValueError(f"recording {b}: token ids must lie in [0, {vocab})")

    @staticmethod
    def _segment_inputs(olens, gt, clens, vocab, T, dev):
        """(olens_d, gt_d, clens_d, Cmax): HOST data is checked (`check_segmentable`) and copied over, int32 DEVICE
        tensors are taken as they are, a mixture is refused."""
        given = (olens, gt, clens)
        on_dev = [torch.is_tensor(x) and x.is_cuda for x in given]
        if all(on_dev):
            if any(x.dtype != torch.int32 for x in given) or gt.dim() != 2 or gt.shape[1] < 2:
                raise ValueError("device-side olens / gt / clens must be int32, gt (B, Cmax) with Cmax >= 2")
            if int(olens.numel()) != int(gt.shape[0]) or int(clens.numel()) != int(gt.shape[0]):
                raise ValueError(f"olens and clens must have {int(gt.shape[0])} entries")
            return olens.contiguous(), gt.contiguous(), clens.contiguous(), int(gt.shape[1])
        if any(on_dev):
            raise ValueError("olens, gt and clens must be all host data or all device tensors")
        ol, rows, cl = [x.tolist() if torch.is_tensor(x) else list(x) for x in given]
        if not (len(ol) == len(rows) == len(cl)) or not rows:
            raise ValueError("olens, gt and clens must have one entry per recording")
        rows = [list(r) for r in rows]
        CTC.check_segmentable(ol, rows, cl, vocab, T)
        Cmax = max(cl)
        g = torch.zeros(len(rows), Cmax, dtype=torch.int32)
        for b, (r, n) in enumerate(zip(rows, cl)):
            g[b, 1:n] = torch.tensor([int(v) for v in r[1:n]], dtype=torch.int32)
        olens_d, clens_d, gt_d = (torch.as_tensor(v, dtype=torch.int32).to(dev, non_blocking=True) for v in (ol, cl, g))
        return olens_d, gt_d, clens_d, Cmax

    def segment_device(self, enc_act: torch.Tensor, olens, gt, clens, blank: int, window: int,
                       preamble_free: bool = True, from_last_frame: bool = False):
        """CTC segmentation of the recordings enc_act (B,T,d) (compute dtype, on the device) against their ground-truth
        columns, by `em_ctc_log_probs_t` -> `em_ctc_segment` (include/espnet_amd.h states the band, the recursion and
        the tie rule).  Returns (first_frame (B,Cmax) i32, frame_col (B,T) i32, frame_lp (B,T) f32, t_end (B,) i32,
        total (B,) f32, status (B,) i32) as device tensors, no host sync.

        olens / clens: per-recording lengths, gt (B, Cmax) columns (column 0 is the start symbol, never read).  Given as
        HOST data they are checked first (`check_segmentable`: ValueError before any launch) and copied over; given as
        int32 DEVICE tensors they are taken as they are."""
        L.require_gpu(enc_act, "enc_act")
        B, T, d = enc_act.shape
        dev, V = enc_act.device, self.odim
        olens_d, gt_d, clens_d, Cmax = self._segment_inputs(olens, gt, clens, V, T, dev)
        if int(gt_d.shape[0]) != B:
            raise ValueError(f"gt must have {B} rows")
        return self.segment_log_probs_t(self.log_probs_t_device(enc_act), B * T, olens_d, gt_d, Cmax, clens_d, B, T, blank,
                                        window, preamble_free=preamble_free, from_last_frame=from_last_frame)

    def log_probs_t_device(self, enc_act: torch.Tensor) -> torch.Tensor:
        """enc_act (B,T,d) in the compute dtype -> the transposed log-posteriors lpT (V, B*T) f32 the trellis kernels
        read (`em_ctc_log_probs_t`: frame-contiguous rows); only enqueues work."""
        B, T, d = enc_act.shape
        p = self.packed(enc_act.device)
        lpT = torch.empty(self.odim, B * T, dtype=torch.float32, device=enc_act.device)
        L.check(L.load().em_ctc_log_probs_t(self.em_dtype, L.ptr(enc_act), B, T, d, L.ptr(p.weight), L.ptr(p.bias),
                                            self.odim, L.ptr(lpT), L.current_stream_ptr()), "em_ctc_log_probs_t")
        return lpT

    @staticmethod
    def segment_log_probs_t(lpT, ldT, olens_d, gt_d, Cmax, clens_d, B, T, blank, window, preamble_free=True,
                            from_last_frame=False, ws_bytes=None):
        """`em_ctc_segment` on given transposed log-posteriors lpT [V][ldT] (device tensors throughout)."""
        lib, dev = L.load(), lpT.device
        window = int(window)
        if window < 1 or window > int(lib.em_ctc_segment_max_window()):
            raise ValueError(f"window must lie in [1, {int(lib.em_ctc_segment_max_window())}], not {window}")
        flags = (L.EM_SEG_PREAMBLE_FREE if preamble_free else 0) | (L.EM_SEG_FROM_LAST_FRAME if from_last_frame else 0)
        if ws_bytes is None:
            ws_bytes = int(lib.em_ctc_segment_workspace_bytes(B, T, Cmax, window))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        first_frame = torch.empty(B, Cmax, dtype=torch.int32, device=dev)
        frame_col = torch.empty(B, T, dtype=torch.int32, device=dev)
        frame_lp = torch.empty(B, T, dtype=torch.float32, device=dev)
        t_end = torch.empty(B, dtype=torch.int32, device=dev)
        total = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(lib.em_ctc_segment(L.ptr(lpT), ldT, L.ptr(olens_d), L.ptr(gt_d), Cmax, L.ptr(clens_d), B, T, blank, window,
                                   flags, L.ptr(first_frame), L.ptr(frame_col), L.ptr(frame_lp), L.ptr(t_end), L.ptr(total),
                                   L.ptr(status), L.ptr(ws), ws_bytes, L.current_stream_ptr()), "em_ctc_segment")
        return first_frame, frame_col, frame_lp, t_end, total, status

    # ------------------------------------------------------------------ likelihood of given transcripts (csrc/ctc_nll.hip)
    def nll_device(self, enc_act: torch.Tensor, olens, targets, ylens, blank: int, mem_of=None) -> torch.Tensor:
        """-log p_ctc(targets[n] | utterance mem_of[n]) for N candidate transcripts, (N,) f32 on the device, by
        `em_ctc_log_probs_t` -> `em_ctc_seq_nll` (include/espnet_amd.h states the recursion); only enqueues work.

        enc_act (Bm,T,d) in the compute dtype; olens (Bm,); targets (N, Lmax) ids padded with anything, ylens (N,);
        mem_of (N,) the utterance of each candidate, None: candidate n belongs to utterance n (N == Bm).  The argument
        forms are `forced_align_device`'s: HOST data (lists or CPU tensors) is checked first - ids in [0, V) and not the
        blank, lengths inside their rows, mem_of in [0, Bm): ValueError before any launch - and copied over; int32
        DEVICE tensors are taken as they are.  A transcript its utterance has too few frames for is no error here: its
        value is +inf, as the reference's ctc_loss has it."""
        L.require_gpu(enc_act, "enc_act")
        Bm, T, _ = enc_act.shape
        olens_d, tg_d, ylens_d, mo_d, N, Lmax = self._trellis_inputs(enc_act, olens, targets, ylens, blank, mem_of, align=False)
        if N == 0:
            return torch.empty(0, dtype=torch.float32, device=enc_act.device)
        if mo_d is None and N != Bm:
            raise ValueError(f"{N} transcripts for {Bm} utterances need mem_of")
        return self.nll_log_probs_t(self.log_probs_t_device(enc_act), Bm * T, olens_d, Bm, T, tg_d, Lmax, ylens_d, mo_d, N, blank)

    @staticmethod
    def nll_log_probs_t(lpT, ldT, olens_d, Bm, T, tg_d, Lmax, ylens_d, mem_of_d, N, blank) -> torch.Tensor:
        """`em_ctc_seq_nll` on given transposed log-posteriors lpT [V][ldT] (device tensors throughout; tg_d's row stride
        is Lmax, or 1 when Lmax == 0)."""
        nll = torch.empty(N, dtype=torch.float32, device=lpT.device)
        L.check(L.load().em_ctc_seq_nll(L.ptr(lpT), ldT, L.ptr(olens_d), Bm, T, L.ptr(tg_d), Lmax, L.ptr(ylens_d),
                                        L.ptr(mem_of_d), N, blank, L.ptr(nll), L.current_stream_ptr()), "em_ctc_seq_nll")
        return nll

    def nll(self, hs_pad: torch.Tensor, hlens, ys_pad, ys_lens, blank_idx: int = 0) -> torch.Tensor:
        """The per-utterance value of the reference's CTC.forward with reduce=False under the builtin ctc_loss
        (espnet2/asr/ctc.py; there the values are summed and divided by the batch size): hs_pad (B,T,d) encoder output
        on the device, hlens (B,), ys_pad (B,Lmax) target ids, ys_lens (B,) -> (B,) f32 on the device, +inf where the
        frames cannot carry the transcript (ctc_loss with zero_infinity=False).  Ids equal to the blank or outside
        [0, V) raise ValueError."""
        act = self._to_act(hs_pad)
        host = [x.cpu() if torch.is_tensor(x) else x for x in (hlens, ys_pad, ys_lens)]
        return self.nll_device(act, host[0], host[1], host[2], int(blank_idx))

    @staticmethod
    def _token_outputs(B, T, dev, out):
        """(tokens (B,T) i32, token_lens (B,) i32): fresh tensors, or the caller's (`out`: e.g. the current slot of an
        `espnet_amd.distributed.RecordRing`, so the records are written where the collation reads them)."""
        if out is None:
            return torch.empty(B, T, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        tokens, tlens = out
        if (tuple(tokens.shape) != (B, T) or tuple(tlens.shape) != (B,) or tokens.dtype != torch.int32
                or tlens.dtype != torch.int32 or not tokens.is_contiguous() or not tlens.is_contiguous()):
            raise ValueError(f"out must be contiguous int32 ({B}, {T}) and ({B},) tensors")
        L.require_gpu(tokens, "out tokens")
        return tokens, tlens

    def greedy_device(self, enc_act: torch.Tensor, olens_dev: torch.Tensor, blank: int, sos_eos: int, out=None):
        """Fused G1 path (bin/asr_inference.py:574-575): returns (ids (B,T) i32, tokens (B,T) i32
        padded with -1, token_lens (B,) i32), all on the device, no host sync."""
        p = self.packed(enc_act.device)
        B, T, d = enc_act.shape
        dev = enc_act.device
        logits = torch.empty(B * T, self.odim, dtype=torch.float32, device=dev)
        ids = torch.empty(B, T, dtype=torch.int32, device=dev)
        tokens, tlens = self._token_outputs(B, T, dev, out)
        L.check(L.load().em_ctc_greedy(self.em_dtype, L.ptr(enc_act), L.ptr(p.weight), L.ptr(p.bias),
                                       B, T, d, self.odim, L.ptr(olens_dev), blank, sos_eos,
                                       L.ptr(logits), L.ptr(ids), L.ptr(tokens), L.ptr(tlens),
                                       L.current_stream_ptr()), "em_ctc_greedy")
        return ids, tokens, tlens

    def collapse_device(self, ids: torch.Tensor, olens_dev: torch.Tensor, blank: int, sos_eos: int, out=None):
        """groupby + drop blank / <sos/eos> (bin/asr_inference.py:574-575) over given per-frame ids (B, T) i32:
        returns (ids, tokens padded with -1, token_lens), no host sync."""
        B, T = ids.shape
        tokens, tlens = self._token_outputs(B, T, ids.device, out)
        L.check(L.load().em_ctc_collapse(L.ptr(ids), L.ptr(olens_dev), B, T, blank, sos_eos, L.ptr(tokens),
                                         L.ptr(tlens), L.current_stream_ptr()), "em_ctc_collapse")
        return ids, tokens, tlens
