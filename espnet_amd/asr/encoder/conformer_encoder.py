"""ConformerEncoder on the MI355X: parameter tree + weight packing + one C-ABI call per batch.

Mirrors espnet2/asr/encoder/conformer_encoder.py:53-429 (constructor keywords, `output_size()`,
`forward(xs_pad, ilens, prev_states=None) -> (ys, olens, None)`) and exposes the SAME state-dict
keys as the reference (`embed.conv.{0,2}`, `embed.out`, `encoders.N.{self_attn,feed_forward,
feed_forward_macaron,conv_module,norm_*}`, `after_norm`), so reference checkpoints load unchanged.

Only the BASELINE combination is accelerated (input_layer=conv2d, rel_pos / rel_selfattn with
rel_pos_type=latest, macaron_style, use_cnn_module, normalize_before, swish, d_k = 64); any other
combination raises NotImplementedError at construction (a maintainer integrating this class into
the reference registry keeps the stock `conformer` entry for those).

The torch.nn layers below are parameter CONTAINERS: their forward() is never called.  The
arithmetic is csrc/{frontend,gemm,norm,attention,conv,encoder}.hip.
"""
import contextlib
import ctypes as C
import os
import threading
import weakref
from typing import List, Optional

import torch

from espnet_amd import lib as L
from espnet_amd.asr.encoder._subsampled_base import (LN_EPS, LayerNorm, SubsampledEncoderBase,  # noqa: F401
                                                     _Conv2dSubsampling, _fused_enabled, pack_conv1_frags,
                                                     pack_conv2_frags, rel_pos_table, resolve_rel_pos,
                                                     rows_ffn_packable)
from espnet_amd.nets_utils import SUBSAMPLING_CONVS

_POS_PROJ_LOCK = threading.Lock()
# the packed weights struct carries the per-call `ctc_ids` pointer: setting it and launching the encoder is one critical
# section for host threads that encode concurrently; the ids a call produced are kept per THREAD
_ENC_CALL_LOCK = threading.Lock()
_TLS = threading.local()

class _RelPositionMultiHeadedAttention(torch.nn.Module):
    """Parameters of transformer/attention.py:362-389 (+ MultiHeadedAttention :24-75)."""

    def __init__(self, n_head, n_feat):
        super().__init__()
        self.d_k, self.h = n_feat // n_head, n_head
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)
        self.linear_pos = torch.nn.Linear(n_feat, n_feat, bias=False)
        self.pos_bias_u = torch.nn.Parameter(torch.Tensor(self.h, self.d_k))
        self.pos_bias_v = torch.nn.Parameter(torch.Tensor(self.h, self.d_k))
        torch.nn.init.xavier_uniform_(self.pos_bias_u)
        torch.nn.init.xavier_uniform_(self.pos_bias_v)


class _PositionwiseFeedForward(torch.nn.Module):
    def __init__(self, idim, hidden):
        super().__init__()
        self.w_1 = torch.nn.Linear(idim, hidden)
        self.w_2 = torch.nn.Linear(hidden, idim)


class _ConvolutionModule(torch.nn.Module):
    """Parameters of conformer/convolution.py:22-54."""

    def __init__(self, channels, kernel_size):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0
        self.pointwise_conv1 = torch.nn.Conv1d(channels, 2 * channels, 1)
        self.depthwise_conv = torch.nn.Conv1d(channels, channels, kernel_size,
                                              padding=(kernel_size - 1) // 2, groups=channels)
        self.norm = torch.nn.BatchNorm1d(channels)
        self.pointwise_conv2 = torch.nn.Conv1d(channels, channels, 1)


class _EncoderLayer(torch.nn.Module):
    """Parameters of conformer/encoder_layer.py:43-77."""

    def __init__(self, size, heads, ff, kernel):
        super().__init__()
        self.self_attn = _RelPositionMultiHeadedAttention(heads, size)
        self.feed_forward = _PositionwiseFeedForward(size, ff)
        self.feed_forward_macaron = _PositionwiseFeedForward(size, ff)
        self.conv_module = _ConvolutionModule(size, kernel)
        self.norm_ff = LayerNorm(size)
        self.norm_mha = LayerNorm(size)
        self.norm_ff_macaron = LayerNorm(size)
        self.norm_conv = LayerNorm(size)
        self.norm_final = LayerNorm(size)


def pack_k_units(w: torch.Tensor) -> torch.Tensor:
    """[N][256] -> the fragment-major "K units" of the fused block kernel (include/espnet_amd.h, EmBlockArgs): per
    64 rows one 32 KiB unit [nf][ks][lg][lr][e] = w[64 u + 16 nf + lr][32 ks + 8 lg + e], so that each MFMA weight
    operand of a wave is one contiguous 1 KiB line."""
    n, k = w.shape
    assert k == 256 and n % 64 == 0, (n, k)
    return w.detach().reshape(n // 64, 4, 16, 8, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous().reshape(n, k)


def _pad_chunks(ff: int) -> int:
    """FFN width as the fused kernel walks it: whole PAIRS of 64-wide chunks."""
    assert ff % 64 == 0, ff
    return (ff + 127) // 128 * 128


def pack_w1(w: torch.Tensor) -> torch.Tensor:
    """First matrix of an FFN, [ff][256] -> K units, zero-padded to an even number of 64-row chunks (the padded
    chunk's hidden activation is swish(0 + 0) = 0 and meets zero columns of w_2)."""
    ff = w.shape[0]
    return pack_k_units(torch.nn.functional.pad(w.detach(), (0, 0, 0, _pad_chunks(ff) - ff)))


def pack_w2(w: torch.Tensor) -> torch.Tensor:
    """Second matrix of an FFN, [256][ff] -> 64 KiB per pair of hidden chunks in the order the kernel's waves hold the
    hidden activation (include/espnet_amd.h, EmBlockArgs):
    pair[p][w][f][lg][lr][e] = W[16 f + lr][64 (2 p + (e >> 2)) + 16 w + 4 lg + (e & 3)]."""
    d, ff = w.shape
    assert d == 256 and ff % 64 == 0, (d, ff)
    ffp = _pad_chunks(ff)
    wp = torch.nn.functional.pad(w.detach(), (0, ffp - ff))
    # [o = 16 f + lr][hidden = 128 p + 64 ci + 16 wv + 4 lg + r] -> [p][wv][f][lg][lr][ci][r]
    u = wp.reshape(16, 16, ffp // 128, 2, 4, 4, 4).permute(2, 4, 0, 5, 1, 3, 6).contiguous()
    return u.reshape(ffp // 128, 4 * 16 * 64 * 8)


def pack_ffn_rows_w1(w: torch.Tensor) -> torch.Tensor:
    """First matrix of an FFN of the 512-wide model, [ff][512] -> the operand stream of csrc/ffn_rows.hip
    (include/espnet_amd.h, EmFfnRowsArgs): [c][ks][wv][lg][lr][e] = W1[128 c + 16 wv + lr][32 ks + 8 lg + e]."""
    ff, k = w.shape
    assert k == 512 and ff % 128 == 0, (ff, k)
    # [row = 128 c + 16 wv + lr][col = 32 ks + 8 lg + e] -> [c][ks][wv][lg][lr][e]
    u = w.detach().reshape(ff // 128, 8, 16, 16, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous()
    return u.reshape(ff, k)


def pack_ffn_rows_w2(w: torch.Tensor) -> torch.Tensor:
    """Second matrix, [512][ff] -> [c][s][cf][wv][lg][lr][e] = W2[64 wv + 16 cf + lr][128 c + 32 s + 16 (e >> 2) + 4 lg + (e & 3)]:
    the contraction index in the order the kernel's waves hold the hidden activation."""
    d, ff = w.shape
    assert d == 512 and ff % 128 == 0, (d, ff)
    # [o = 64 wv + 16 cf + lr][hidden = 128 c + 32 s + 16 eh + 4 lg + el] -> [c][s][cf][wv][lg][lr][eh][el]
    u = w.detach().reshape(8, 4, 16, ff // 128, 4, 2, 4, 4).permute(3, 4, 1, 0, 6, 2, 5, 7).contiguous()
    return u.reshape(ff // 128, 4 * 4 * 8 * 64 * 8)


def pack_rows_proj(w: torch.Tensor) -> torch.Tensor:
    """A [512][512] projection in front of a row-block feed-forward launch (EmFfnRowsArgs.pre_w):
    [ks][cf][wv][lg][lr][e] = W[64 wv + 16 cf + lr][32 ks + 8 lg + e]."""
    n, k = w.shape
    assert n == 512 and k == 512, (n, k)
    return w.detach().reshape(8, 4, 16, 16, 4, 8).permute(3, 1, 0, 4, 2, 5).contiguous().reshape(n, k)


def glu_chunk_order(d: int = 512) -> torch.Tensor:
    """Row order of pointwise_conv1 ([value rows 0 .. d) | gate rows d .. 2 d), F.glu(dim=1), convolution.py:66) for the
    row-block GLU launch: chunk 2 j = the value rows of output columns 128 j .. 128 j + 127, chunk 2 j + 1 their gate rows."""
    idx = torch.arange(2 * d).reshape(2, d // 128, 128)  # [value | gate][j][128]
    return idx.permute(1, 0, 2).reshape(-1)


def pack_rows_glu(w: torch.Tensor) -> torch.Tensor:
    """pointwise_conv1 [2 * 512][512] -> the w1p layout of EmFfnRowsArgs in value / gate chunk pairs (EM_ROWS_GLU)."""
    return pack_ffn_rows_w1(w.detach()[glu_chunk_order(w.shape[1])])


class ConformerEncoder(SubsampledEncoderBase):
    _WS_FN, _ENC_FN = "em_conformer_workspace_bytes", "em_conformer_encode"  # C-ABI entry points of forward_device

    @staticmethod
    def _option_check(*, input_layer, normalize_before, concat_after, positionwise_layer_type, macaron_style,
                      rel_pos_type, pos_enc_layer_type, selfattention_layer_type, activation_type, use_cnn_module,
                      zero_triu, interctc_layer_idx, interctc_use_conditioning, ctc_trim, qk_norm, output_size,
                      attention_heads, linear_units, cnn_module_kernel):
        """Options of espnet2/asr/encoder/conformer_encoder.py:89-121 that the MI355X kernels do not cover ->
        (list of "name=value" strings, legacy rel-pos flag).  An empty list = the fast path applies."""
        bad = []
        if input_layer not in SUBSAMPLING_CONVS: bad.append(f"input_layer={input_layer}")
        if not normalize_before: bad.append("normalize_before=False")
        if concat_after: bad.append("concat_after=True")
        if positionwise_layer_type != "linear": bad.append(f"positionwise_layer_type={positionwise_layer_type}")
        if not macaron_style: bad.append("macaron_style=False")
        pos_enc_layer_type, selfattention_layer_type, legacy = resolve_rel_pos(rel_pos_type, pos_enc_layer_type,
                                                                               selfattention_layer_type)
        if not legacy:
            if pos_enc_layer_type != "rel_pos": bad.append(f"pos_enc_layer_type={pos_enc_layer_type}")
            if selfattention_layer_type != "rel_selfattn": bad.append(f"selfattention_layer_type={selfattention_layer_type}")
        if activation_type != "swish": bad.append(f"activation_type={activation_type}")
        if not use_cnn_module: bad.append("use_cnn_module=False")
        if zero_triu: bad.append("zero_triu=True")
        if len(interctc_layer_idx) > 0 or interctc_use_conditioning or ctc_trim: bad.append("interctc/ctc_trim")
        if qk_norm: bad.append("qk_norm=True")
        if output_size % 64 or output_size // attention_heads != 64: bad.append("d_k != 64")
        if linear_units % 64: bad.append("linear_units % 64 != 0")
        if cnn_module_kernel not in (3, 7, 15, 31): bad.append(f"cnn_module_kernel={cnn_module_kernel}")
        return bad, legacy

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4,
                 linear_units: int = 2048, num_blocks: int = 6, dropout_rate: float = 0.1,
                 positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: Optional[str] = "conv2d", normalize_before: bool = True,
                 concat_after: bool = False, positionwise_layer_type: str = "linear",
                 positionwise_conv_kernel_size: int = 3, macaron_style: bool = False,
                 rel_pos_type: str = "legacy", pos_enc_layer_type: str = "rel_pos",
                 selfattention_layer_type: str = "rel_selfattn", activation_type: str = "swish",
                 use_cnn_module: bool = True, zero_triu: bool = False, cnn_module_kernel: int = 31,
                 padding_idx: int = -1, interctc_layer_idx: List[int] = [],
                 interctc_use_conditioning: bool = False, ctc_trim: bool = False,
                 stochastic_depth_rate=0.0, layer_drop_rate: float = 0.0,
                 max_pos_emb_len: int = 5000, qk_norm: bool = False, use_flash_attn: bool = True,
                 compute_dtype: str = "bfloat16"):
        bad, legacy = self._unsupported(locals())
        if bad:
            raise NotImplementedError("outside the MI355X Conformer fast path: " + ", ".join(bad))
        super().__init__(input_size, output_size, attention_heads, linear_units, num_blocks, input_layer, compute_dtype,
                         lambda: _EncoderLayer(output_size, attention_heads, linear_units, cnn_module_kernel),
                         legacy_relpos=legacy, max_pos_emb_len=max_pos_emb_len)
        self.cnn_module_kernel = cnn_module_kernel
        self.normalize_before = normalize_before
        self.last_ctc_ids = None
        object.__setattr__(self, "fused_ctc", None)  # set by the model: a CTC head to fuse (not a submodule of the encoder)

    # ------------------------------------------------------------------ packing (load time)
    def _build_pack(self, pk):
        """The reference-layout parameters in the layouts the kernels consume."""
        A, F = pk.A, pk.F
        d, ff, Lb = self._output_size, self.linear_units, self.num_blocks
        w = L.EmConformerWeights()
        w.d, w.heads, w.ff, w.num_blocks = d, self.heads, ff, Lb
        w.kernel, w.n_mels = self.cnn_module_kernel, self._input_size
        t = self._pack_embed(pk, w)
        t["wpos_all"] = A(torch.cat([l.self_attn.linear_pos.weight for l in self.encoders], dim=0))
        pk.fill(w, t)
        layers = (L.EmConformerLayer * Lb)()
        glu_perm = torch.arange(2 * d).reshape(2, d // 16, 16).permute(1, 0, 2).reshape(-1)
        for i, l in enumerate(self.encoders):
            sa, cm = l.self_attn, l.conv_module
            bn = cm.norm
            scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
            dw_w = cm.depthwise_conv.weight.double().reshape(d, -1) * scale[:, None]
            dw_b = (cm.depthwise_conv.bias.double() - bn.running_mean.double()) * scale + bn.bias.double()
            lt = dict(
                norm_ff_mac_g=F(l.norm_ff_macaron.weight), norm_ff_mac_b=F(l.norm_ff_macaron.bias),
                norm_mha_g=F(l.norm_mha.weight), norm_mha_b=F(l.norm_mha.bias),
                norm_conv_g=F(l.norm_conv.weight), norm_conv_b=F(l.norm_conv.bias),
                norm_ff_g=F(l.norm_ff.weight), norm_ff_b=F(l.norm_ff.bias),
                norm_final_g=F(l.norm_final.weight), norm_final_b=F(l.norm_final.bias),
                ffm_w1=A(l.feed_forward_macaron.w_1.weight), ffm_b1=F(l.feed_forward_macaron.w_1.bias),
                ffm_w2=A(l.feed_forward_macaron.w_2.weight), ffm_b2=F(l.feed_forward_macaron.w_2.bias),
                wqkv=A(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)),
                bqkv=F(torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0)),
                pos_u=F(sa.pos_bias_u), pos_v=F(sa.pos_bias_v),
                wout=A(sa.linear_out.weight), bout=F(sa.linear_out.bias),
                pw1=A(cm.pointwise_conv1.weight.reshape(2 * d, d)[glu_perm]),
                pw1_b=F(cm.pointwise_conv1.bias[glu_perm]),
                dw_w=F(dw_w.t()), dw_b=F(dw_b),  # [k][d]: tap-major, coalesced over channels
                pw2=A(cm.pointwise_conv2.weight.reshape(d, d)), pw2_b=F(cm.pointwise_conv2.bias),
                ff_w1=A(l.feed_forward.w_1.weight), ff_b1=F(l.feed_forward.w_1.bias),
                ff_w2=A(l.feed_forward.w_2.weight), ff_b2=F(l.feed_forward.w_2.bias),
            )
            pk.fill(layers[i], lt)
        if self._fusable():
            self._pack_fused(pk, layers)
            self._pack_fused_ctc(pk, w)
        elif rows_ffn_packable(pk.act, d, ff) and _fused_enabled(self):
            # the 512-wide model: each feed-forward module as one row-block launch (csrc/ffn_rows.hip)
            for i, l in enumerate(self.encoders):
                lt = dict(ffm_w1p=A(pack_ffn_rows_w1(l.feed_forward_macaron.w_1.weight)),
                          ffm_w2p=A(pack_ffn_rows_w2(l.feed_forward_macaron.w_2.weight)),
                          ff_w1p=A(pack_ffn_rows_w1(l.feed_forward.w_1.weight)),
                          ff_w2p=A(pack_ffn_rows_w2(l.feed_forward.w_2.weight)),
                          pw2p=A(pack_rows_proj(l.conv_module.pointwise_conv2.weight.reshape(d, d))),
                          woutp=A(pack_rows_proj(l.self_attn.linear_out.weight)),
                          pw1f=A(pack_rows_glu(l.conv_module.pointwise_conv1.weight.reshape(2 * d, d))),
                          fp_c=F(l.conv_module.pointwise_conv1.bias[glu_chunk_order(d)]))
                if self.heads * 64 == d:  # round 6: q | k | v walked behind the macaron launch (EmFfnRowsArgs.post_q)
                    sa = l.self_attn
                    lt["wqkvp"] = A(pack_ffn_rows_w1(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)))
                pk.fill(layers[i], lt)
            self._pack_rows_ctc(pk, w)
        w.layers = C.cast(layers, C.POINTER(L.EmConformerLayer))
        pk.w, pk.layers = w, layers

    def _fusable(self) -> bool:
        """Shapes the row-block fused kernels cover (csrc/block.hip); everything else keeps the per-operator launches."""
        return (self.em_dtype == L.EM_BF16 and self._output_size == 256 and self.heads == 4
                and self.linear_units <= 1024 and self.cnn_module_kernel == 31
                and not self.legacy_relpos)

    def _pack_fused(self, pk, layers):
        """Operands of em_conformer_block_fused (include/espnet_amd.h): pointwise_conv1 in 64-row value / gate
        granules and the bias / LayerNorm vectors of every kernel as groups of EM_BLOCK_PARAM_GROUP floats in the
        order the kernel consumes them."""
        A, F = pk.A, pk.F
        d, G = self._output_size, L.EM_BLOCK_PARAM_GROUP

        def group(*vecs):
            v = torch.cat([t.detach().to(torch.float32).reshape(-1).cpu() for t in vecs])
            assert v.numel() <= G
            return torch.nn.functional.pad(v, (0, G - v.numel()))

        def pad_ff(b):
            return torch.nn.functional.pad(b.detach().to(torch.float32).cpu(), (0, 1024 - b.numel()))

        perm = torch.cat([torch.cat([torch.arange(64 * j, 64 * j + 64), torch.arange(d + 64 * j, d + 64 * j + 64)])
                          for j in range(d // 64)])

        def a_groups(l):
            sa = l.self_attn
            return [group(l.norm_ff_macaron.weight, l.norm_ff_macaron.bias, pad_ff(l.feed_forward_macaron.w_1.bias),
                          l.feed_forward_macaron.w_2.bias),
                    group(l.norm_mha.weight, l.norm_mha.bias, sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias)]

        n = len(self.encoders)
        for i, l in enumerate(self.encoders):
            cm = l.conv_module
            pw1 = cm.pointwise_conv1.weight.reshape(2 * d, d)
            d_groups = [group(cm.pointwise_conv2.bias, l.norm_ff.weight, l.norm_ff.bias),
                        group(pad_ff(l.feed_forward.w_1.bias), l.feed_forward.w_2.bias, l.norm_final.weight,
                              l.norm_final.bias)]
            tail = a_groups(self.encoders[i + 1]) if i + 1 < n else [group(self.after_norm.weight,
                                                                           self.after_norm.bias)]
            sa = l.self_attn
            lt = dict(pw1f=A(pack_k_units(pw1[perm])), ffm_w2p=A(pack_w2(l.feed_forward_macaron.w_2.weight)),
                      ff_w2p=A(pack_w2(l.feed_forward.w_2.weight)),
                      woutp=A(pack_k_units(sa.linear_out.weight)),
                      pw2p=A(pack_k_units(cm.pointwise_conv2.weight.reshape(d, d))),
                      ff_w1p=A(pack_w1(l.feed_forward.w_1.weight)),
                      ffm_w1p=A(pack_w1(l.feed_forward_macaron.w_1.weight)),
                      wqkvp=A(pack_k_units(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0))),
                      fp_c=F(group(l.self_attn.linear_out.bias, l.norm_conv.weight, l.norm_conv.bias,
                                   cm.pointwise_conv1.bias[perm])),
                      fp_da=F(torch.cat(d_groups + tail)))
            if i == 0:
                lt["fp_a"] = F(torch.cat(a_groups(l)))
            pk.fill(layers[i], lt)

    def _pack_fused_ctc(self, pk, w):
        """The CTC head the model attached (`fused_ctc`, a espnet_amd.asr.ctc.CTC): its weight zero-padded to 64-row
        units and its bias padded with -3e38, for the arg-max stage of the last block kernel (EM_BLOCK_CTC)."""
        ctc = getattr(self, "fused_ctc", None)
        if ctc is None or ctc.eprojs != self._output_size:
            return
        V = ctc.odim
        units = (V + 63) // 64
        if units > L.EM_BLOCK_CTC_MAX_UNITS:
            return
        wt = torch.zeros(units * 64, self._output_size, dtype=torch.float32)
        wt[:V] = ctc.ctc_lo.weight.detach().to(torch.float32).cpu()
        bt = torch.full((units * 64,), -3.0e38, dtype=torch.float32)
        bt[:V] = ctc.ctc_lo.bias.detach().to(torch.float32).cpu()
        pk.fill(w, dict(ctc_w=pk.A(pack_k_units(wt)), ctc_b=pk.F(bt)))
        w.ctc_units, pk.ctc_stamp = units, self._ctc_version(ctc)

    def _pack_rows_ctc(self, pk, w):
        """512-wide model: the attached CTC head for the arg-max walk behind the last row-block launch (EmFfnRowsArgs.post_*):
        weight zero-padded to whole 128-row chunks in the w1p layout, bias padded with -3e38."""
        ctc = getattr(self, "fused_ctc", None)
        if ctc is None or ctc.eprojs != self._output_size:
            return
        V = ctc.odim
        chunks = (V + 127) // 128
        wt = torch.zeros(chunks * 128, self._output_size, dtype=torch.float32)
        wt[:V] = ctc.ctc_lo.weight.detach().to(torch.float32).cpu()
        bt = torch.full((chunks * 128,), -3.0e38, dtype=torch.float32)
        bt[:V] = ctc.ctc_lo.bias.detach().to(torch.float32).cpu()
        pk.fill(w, dict(ctc_w=pk.A(pack_ffn_rows_w1(wt)), ctc_b=pk.F(bt)))
        w.ctc_units, pk.ctc_stamp = chunks, self._ctc_version(ctc)

    @staticmethod
    def _ctc_version(ctc):
        lo = ctc.ctc_lo
        return (lo.weight.data_ptr(), lo.weight._version, lo.bias.data_ptr(), lo.bias._version)

    def _pack_current(self, pk) -> bool:
        """A pack that carries the attached CTC head is current while the head's parameters are the ones it copied."""
        stamp = getattr(pk, "ctc_stamp", None)
        return stamp is None or self.fused_ctc is None or stamp == self._ctc_version(self.fused_ctc)

    def _pos_projected(self, T: int, device, pk, pos: torch.Tensor) -> torch.Tensor:
        """pos (2T-1 | T, d) x wpos_all^T -> (rows, num_blocks * d) in the activation dtype, through the same em_gemm
        call the encoder entry point makes without EM_ENC_POS_PROJECTED (bit-identical); kept for the last few lengths
        of the current packing."""
        cache = self.__dict__.setdefault("_pos_proj_cache", {})
        lock = _POS_PROJ_LOCK  # (concurrent batches on host threads; module-level: a lock in __dict__ is not picklable)
        key = (T, str(device), pk.serial)
        cur = torch.cuda.current_stream()
        with lock:
            ent = cache.get(key)
            if ent is not None:
                out, ev, sid, _ = ent
                if sid != cur.cuda_stream:  # produced on another stream (concurrent batches): order this one behind
                    cur.wait_event(ev)      # it, and keep the block from being recycled under this stream's readers
                    out.record_stream(cur)  # when the entry is evicted (a same-stream free is ordered anyway)
                return out
        out = None
        if out is None:
            pos = pos.contiguous()
            rows, d = pos.shape
            n = self.num_blocks * d
            # the fused 256-wide bf16 path also wants the rows fragment-major (block<ATT|C>): packed here, once per length,
            # behind the table (EM_ENC_POS_PACKED)
            packed = (self.em_dtype == L.EM_BF16 and d == 256 and rows == 2 * T - 1 and not getattr(pk.w, "legacy_relpos", 0))
            es = 2 if self.em_dtype == L.EM_BF16 else 4
            tbytes = (rows * n * es + 255) // 256 * 256
            npg = L.load().em_relpos_pos_fragments(T) if packed else 0
            flat = torch.empty(tbytes + self.num_blocks * 4 * npg * 2048, dtype=torch.uint8, device=device)
            out = flat[:rows * n * es].view(self.act_dtype).view(rows, n)
            out._em_flat, out._em_packed = flat, packed  # (keeps the block alive; read back in forward_device)
            args = L.EmGemmArgs(A=pos.data_ptr(), W=pk.w.wpos_all, C=out.data_ptr(), bias=None, M=rows, N=n, K=d,
                                lda=d, ldc=n, scale=1.0)
            L.check(L.load().em_gemm(self.em_dtype, L.EM_EPI_STORE, L.EM_A_PLAIN, C.byref(args),
                                     L.current_stream_ptr()), "em_gemm(linear_pos)")
            if packed:
                L.check(L.load().em_relpos_pack_pos_bf16(out.data_ptr(), n, T, self.num_blocks, flat.data_ptr() + tbytes,
                                                         L.current_stream_ptr()), "em_relpos_pack_pos_bf16")
            ev = torch.cuda.Event()
            ev.record(cur)
            with lock:
                while len(cache) >= 8:
                    cache.pop(next(iter(cache)))
                cache[key] = (out, ev, cur.cuda_stream, pk)  # (the pack is kept alive with its projection)
        return out

    # ------------------------------------------------------------------ forward (the hooks of SubsampledEncoderBase)
    def _call_operands(self, T: int, dev, pk):
        flags = 0
        if self.fold_c if getattr(self, "fold_c", None) is not None else os.environ.get("ESPNET_AMD_FOLD") == "1":
            flags |= L.EM_ENC_FOLD_C  # block<C|D|...>: two launches per block (opt-in: measured no faster)
        if self.split_att if getattr(self, "split_att", None) is not None else os.environ.get("ESPNET_AMD_SPLIT_ATT") == "1":
            flags |= L.EM_ENC_SPLIT_ATT  # attention and block<C> as two launches (rounds 2-5) instead of block<ATT|C>: A/B switch
        pos = self._pos_emb(T, dev)
        if pk.w.wpos_all:
            # linear_pos of every block depends on T and the weights only: projected once per length, handed over ready
            pos = self._pos_projected(T, dev, pk, pos)
            flags |= L.EM_ENC_POS_PROJECTED | (L.EM_ENC_POS_PACKED if getattr(pos, "_em_packed", False) else 0)
        return pos, flags

    @contextlib.contextmanager
    def _ctc_ids_plan(self, w, enc_flags, B, T, T_f, dev):
        """The fused path also hands back the CTC head's per-frame arg-max (EM_BLOCK_CTC): no logits, no second pass.
        Whether they WILL be written is the library's decision, asked through em_conformer_encode_plan_for: the host does
        not re-derive the kernel's shape conditions."""
        self.last_ctc_ids = None
        with _ENC_CALL_LOCK:
            w.ctc_ids = None
            if w.ctc_units > 0:
                ids = torch.empty(B, T, dtype=torch.int32, device=dev)
                w.ctc_ids = ids.data_ptr()
                plan = L.load().em_conformer_encode_plan_for(self.em_dtype, C.byref(w), enc_flags, B, T_f)
                if plan < 0:
                    L.check(plan, "em_conformer_encode_plan")
                if plan & L.EM_ENC_PLAN_CTC_IDS:
                    self.last_ctc_ids = ids
                else:
                    w.ctc_ids = None
            yield

    @property
    def last_ctc_ids(self):
        """Per-frame CTC arg-max ids of the calling thread's last `forward_device` (None when the launch sequence taken
        does not produce them)."""
        ids = getattr(_TLS, "ids", None)
        return ids.get(self) if ids is not None else None

    @last_ctc_ids.setter
    def last_ctc_ids(self, v):
        if not hasattr(_TLS, "ids"):
            _TLS.ids = weakref.WeakKeyDictionary()  # (keyed by the encoder itself: an entry dies with it, ids are never reused)
        _TLS.ids[self] = v
