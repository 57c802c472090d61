"""ContextualBlockConformerEncoder (streaming, BASELINE config 5) on the MI355X.

Mirrors espnet2/asr/encoder/contextual_block_conformer_encoder.py:39-600 for streaming inference:
the constructor keywords, `output_size()`, `forward(xs_pad, ilens, prev_states, is_final=...,
infer_mode=True)` and `forward_infer(xs_pad, ilens, prev_states, is_final)` with the reference's
state dictionary (`prev_addin`, `buffer_before_downsampling`, `ilens_buffer`,
`buffer_after_downsampling`, `n_processed_blocks`, `past_encoder_ctx`), and the reference's
state-dict keys (`embed.conv.{0,2}`, `embed.out`, `encoders.N.{self_attn,feed_forward,
feed_forward_macaron,conv_module,norm1,norm2,norm_ff_macaron,norm_conv,norm_final}`, `after_norm`).

Split of work:
  * host (`_contextual_block_base.py`, shared with the streaming Transformer encoder; integers + tensor slicing only): the buffering before / after the 4x
    subsampling, block counting, output stitching — exactly the reference's control flow
    (:386-600), because it decides WHICH frames a call processes;
  * device (csrc/streaming.hip, gemm.hip, norm.hip, conv.hip, frontend.hip): every arithmetic op —
    subsampling convs, block assembly with stream positional encoding and block means, all
    encoder layers, context hand-over, after_norm.

`StreamingStepGraph` (`_contextual_block_base.py`) captures one steady-state call (fixed chunk -> fixed block count) into a
hipGraph (torch.cuda.CUDAGraph on ROCm) so a chunk costs one graph launch instead of ~200 kernel launches.
The torch.nn layers are parameter containers only.
"""
import ctypes as C
from typing import Optional

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table
from espnet_amd.asr.encoder._contextual_block_base import LN_EPS, ContextualBlockEncoderBase  # noqa: F401
from espnet_amd.asr.encoder.conformer_encoder import (LayerNorm, _ConvolutionModule,
                                                      _PositionwiseFeedForward)


class _Conv2dSubsamplingWOPosEnc(torch.nn.Module):
    """Parameters of transformer/subsampling_without_posenc.py:11-42 (kernels [3,3], strides [2,2])."""

    def __init__(self, idim, odim):
        super().__init__()
        self.conv = torch.nn.Sequential(torch.nn.Conv2d(1, odim, 3, 2), torch.nn.ReLU(),
                                        torch.nn.Conv2d(odim, odim, 3, 2), torch.nn.ReLU())
        self.out = torch.nn.Linear(odim * (((idim - 3) // 2 + 1 - 3) // 2 + 1), odim)


class _MultiHeadedAttention(torch.nn.Module):
    def __init__(self, n_head, n_feat):
        super().__init__()
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)


class _ContextualBlockEncoderLayer(torch.nn.Module):
    """Parameters of conformer/contextual_block_encoder_layer.py:46-77."""

    def __init__(self, size, heads, ff, kernel):
        super().__init__()
        self.self_attn = _MultiHeadedAttention(heads, size)
        self.feed_forward = _PositionwiseFeedForward(size, ff)
        self.feed_forward_macaron = _PositionwiseFeedForward(size, ff)
        self.conv_module = _ConvolutionModule(size, kernel)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)
        self.norm_ff_macaron = LayerNorm(size)
        self.norm_conv = LayerNorm(size)
        self.norm_final = LayerNorm(size)


class ContextualBlockConformerEncoder(ContextualBlockEncoderBase):
    _WS_FN, _ENC_FN, _ENC_BATCH_FN = "em_cb_workspace_bytes", "em_cb_encode_blocks", "em_cb_encode_blocks_batch"

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4,
                 linear_units: int = 2048, num_blocks: int = 6, dropout_rate: float = 0.1,
                 positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: Optional[str] = "conv2d", normalize_before: bool = True,
                 concat_after: bool = False, positionwise_layer_type: str = "linear",
                 positionwise_conv_kernel_size: int = 3, macaron_style: bool = False,
                 pos_enc_class=None, selfattention_layer_type: str = "rel_selfattn",
                 activation_type: str = "swish", use_cnn_module: bool = True,
                 cnn_module_kernel: int = 31, padding_idx: int = -1, block_size: int = 40,
                 hop_size: int = 16, look_ahead: int = 16, init_average: bool = True,
                 ctx_pos_enc: bool = True, compute_dtype: str = "bfloat16"):
        super().__init__()
        bad = []
        if input_layer != "conv2d": bad.append(f"input_layer={input_layer}")
        if not normalize_before: bad.append("normalize_before=False")
        if concat_after: bad.append("concat_after=True")
        if positionwise_layer_type != "linear": bad.append(f"positionwise_layer_type={positionwise_layer_type}")
        if not macaron_style: bad.append("macaron_style=False")
        if pos_enc_class is not None: bad.append("pos_enc_class")
        if activation_type != "swish": bad.append(f"activation_type={activation_type}")
        if not use_cnn_module: bad.append("use_cnn_module=False")
        if not init_average: bad.append("init_average=False")
        if not ctx_pos_enc: bad.append("ctx_pos_enc=False")
        if output_size % 64 or output_size // attention_heads not in (32, 64): bad.append("d_k not in {32,64}")
        if linear_units % 64: bad.append("linear_units % 64 != 0")
        if cnn_module_kernel not in (3, 7, 15, 31): bad.append(f"cnn_module_kernel={cnn_module_kernel}")
        if block_size <= 0 or block_size + 2 > 64: bad.append(f"block_size={block_size}")
        if bad:
            raise NotImplementedError("outside the MI355X streaming-Conformer fast path: " + ", ".join(bad))
        self._output_size, self._input_size = output_size, input_size
        self.heads, self.linear_units, self.num_blocks = attention_heads, linear_units, num_blocks
        self.cnn_module_kernel = cnn_module_kernel
        self.normalize_before = normalize_before
        self.block_size, self.hop_size, self.look_ahead = block_size, hop_size, look_ahead
        self.init_average, self.ctx_pos_enc = init_average, ctx_pos_enc
        self.subsample = 4
        self.compute_dtype = compute_dtype
        self.embed = _Conv2dSubsamplingWOPosEnc(input_size, output_size)
        self.encoders = torch.nn.ModuleList(
            [_ContextualBlockEncoderLayer(output_size, attention_heads, linear_units, cnn_module_kernel)
             for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self._ws = {}
        self._flen_cache = {}  # (streams, frames, device) -> per-stream frame counts on the device (_embed_device_batch)

    # ------------------------------------------------------------------ packing (load time)
    def _build_pack(self, pk):
        A, F = pk.A, pk.F
        d, ff, NL = self._output_size, self.linear_units, self.num_blocks
        e = self.embed
        F2 = e.out.in_features // d
        w = L.EmConformerWeights()
        w.d, w.heads, w.ff, w.num_blocks = d, self.heads, ff, NL
        w.kernel, w.n_mels = self.cnn_module_kernel, self._input_size
        top = dict(conv1_w=F(e.conv[0].weight.reshape(d, 9)), conv1_b=F(e.conv[0].bias),
                   conv2_w=A(e.conv[2].weight.permute(0, 2, 3, 1).reshape(d, 9 * d)),
                   conv2_b=F(e.conv[2].bias),
                   embed_w=A(e.out.weight.reshape(d, d, F2).permute(0, 2, 1).reshape(d, F2 * d)),
                   embed_b=F(e.out.bias), after_norm_g=F(self.after_norm.weight),
                   after_norm_b=F(self.after_norm.bias))
        pk.fill(w, top)
        layers = (L.EmConformerLayer * NL)()
        glu_perm = torch.arange(2 * d).reshape(2, d // 16, 16).permute(1, 0, 2).reshape(-1)
        for i, l in enumerate(self.encoders):
            sa, cm = l.self_attn, l.conv_module
            bn = cm.norm
            scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            dw_w = cm.depthwise_conv.weight.double().reshape(d, -1) * scale[:, None]
            dw_b = (cm.depthwise_conv.bias.double() - bn.running_mean.double()) * scale + bn.bias.double()
            lt = dict(
                norm_ff_mac_g=F(l.norm_ff_macaron.weight), norm_ff_mac_b=F(l.norm_ff_macaron.bias),
                norm_mha_g=F(l.norm1.weight), norm_mha_b=F(l.norm1.bias),
                norm_conv_g=F(l.norm_conv.weight), norm_conv_b=F(l.norm_conv.bias),
                norm_ff_g=F(l.norm2.weight), norm_ff_b=F(l.norm2.bias),
                norm_final_g=F(l.norm_final.weight), norm_final_b=F(l.norm_final.bias),
                ffm_w1=A(l.feed_forward_macaron.w_1.weight), ffm_b1=F(l.feed_forward_macaron.w_1.bias),
                ffm_w2=A(l.feed_forward_macaron.w_2.weight), ffm_b2=F(l.feed_forward_macaron.w_2.bias),
                wqkv=A(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)),
                bqkv=F(torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0)),
                wout=A(sa.linear_out.weight), bout=F(sa.linear_out.bias),
                pw1=A(cm.pointwise_conv1.weight.reshape(2 * d, d)[glu_perm]),
                pw1_b=F(cm.pointwise_conv1.bias[glu_perm]),
                dw_w=F(dw_w.t()), dw_b=F(dw_b),
                pw2=A(cm.pointwise_conv2.weight.reshape(d, d)), pw2_b=F(cm.pointwise_conv2.bias),
                ff_w1=A(l.feed_forward.w_1.weight), ff_b1=F(l.feed_forward.w_1.bias),
                ff_w2=A(l.feed_forward.w_2.weight), ff_b2=F(l.feed_forward.w_2.bias))
            if self._fusable():
                lt.update(self._fused_layer(l, A, F))
            pk.fill(layers[i], lt)
        w.layers = C.cast(layers, C.POINTER(L.EmConformerLayer))
        pk.w, pk.layers = w, layers
        pk.pe = F(abs_pos_table(5000, d))  # StreamPositionalEncoding.extend_pe (embedding.py:357-374)

    def _fusable(self) -> bool:
        """Shapes the fused streaming layer covers (csrc/streaming.hip `cb_fusable`, csrc/block.hip with EM_BLOCK_RELU):
        bf16, 256 wide, 4 heads, depthwise conv width 15, feed-forward width a multiple of 128 up to 4096 - the
        aishell streaming recipe.  Everything else keeps the thirteen launches per layer."""
        return (bool(getattr(self, "fused", True))  # (`enc.fused = False` + `invalidate()`: A/B and bisecting)
                and self.em_dtype == L.EM_BF16 and self._output_size == 256 and self.heads == 4
                and self.cnn_module_kernel == 15 and self.linear_units % 128 == 0 and self.linear_units <= 4096)

    def _fused_layer(self, l, A, F):
        """Operands of the row-block kernels for one contextual-block layer (include/espnet_amd.h, EmBlockArgs): weights
        in fragment-major units (`pack_k_units` / `pack_w1` / `pack_w2` of the Conformer encoder), bias / LayerNorm
        vectors as groups of EM_BLOCK_PARAM_GROUP floats in the order the kernels consume them.  The first FFN bias
        does not fit a group at ff = 2048: the kernels read it from the row-major `ffm_b1` / `ff_b1` (EmBlockArgs.ffm_b1g /
        ff_b1g) and its slot in the group stays zero."""
        from espnet_amd.asr.encoder.conformer_encoder import pack_k_units, pack_w1, pack_w2

        d, G = self._output_size, L.EM_BLOCK_PARAM_GROUP
        sa, cm = l.self_attn, l.conv_module

        def group(*vecs):
            v = torch.cat([t.detach().to(torch.float32).reshape(-1).cpu() for t in vecs])
            assert v.numel() <= G
            return torch.nn.functional.pad(v, (0, G - v.numel()))

        b1_slot = torch.zeros(1024)
        perm = torch.cat([torch.cat([torch.arange(64 * j, 64 * j + 64), torch.arange(d + 64 * j, d + 64 * j + 64)])
                          for j in range(d // 64)])
        pw1 = cm.pointwise_conv1.weight.reshape(2 * d, d)
        fp_a = torch.cat([group(l.norm_ff_macaron.weight, l.norm_ff_macaron.bias, b1_slot, l.feed_forward_macaron.w_2.bias),
                          group(l.norm1.weight, l.norm1.bias, sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias)])
        fp_d = torch.cat([group(cm.pointwise_conv2.bias, l.norm2.weight, l.norm2.bias),
                          group(b1_slot, l.feed_forward.w_2.bias, l.norm_final.weight, l.norm_final.bias),
                          torch.zeros(G)])
        return dict(
            pw1f=A(pack_k_units(pw1[perm])), ffm_w2p=A(pack_w2(l.feed_forward_macaron.w_2.weight)),
            ff_w2p=A(pack_w2(l.feed_forward.w_2.weight)), woutp=A(pack_k_units(sa.linear_out.weight)),
            pw2p=A(pack_k_units(cm.pointwise_conv2.weight.reshape(d, d))),
            ff_w1p=A(pack_w1(l.feed_forward.w_1.weight)), ffm_w1p=A(pack_w1(l.feed_forward_macaron.w_1.weight)),
            wqkvp=A(pack_k_units(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0))),
            fp_c=F(group(sa.linear_out.bias, l.norm_conv.weight, l.norm_conv.bias, cm.pointwise_conv1.bias[perm])),
            fp_da=F(fp_d), fp_a=F(fp_a))
