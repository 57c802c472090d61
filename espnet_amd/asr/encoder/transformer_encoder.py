"""TransformerEncoder on the MI355X: parameter tree + weight packing + one C-ABI call per batch
(`em_transformer_encode`, csrc/transformer.hip).

Mirrors espnet2/asr/encoder/transformer_encoder.py (TransformerEncoder: constructor keywords, `output_size()`,
`forward(xs_pad, ilens, prev_states=None) -> (ys, olens, None)`) and exposes the SAME state-dict keys as the
reference (`embed.conv.{0,2[,4]}`, `embed.out`, `encoders.N.{self_attn.linear_{q,k,v,out}, feed_forward.w_{1,2},
norm1, norm2}`, `after_norm`), so reference checkpoints load unchanged.

Accelerated combination: input_layer conv2d / conv2d6 / conv2d8 with PositionalEncoding, normalize_before=True,
concat_after=False, linear position-wise FFN (ReLU), no intermediate CTC, qk_norm=False, d_k = 64; anything else - and
any keyword the reference class does not take - raises NotImplementedError at construction.  The subsampling, GEMMs and
LayerNorms are the Conformer's kernels; the attention is csrc/abs_attn.hip.  The torch.nn layers below are parameter
CONTAINERS: their forward() is never called.
"""
import ctypes as C
from typing import List, Optional

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table
from espnet_amd.asr.encoder._subsampled_base import LayerNorm, SubsampledEncoderBase, rows_ffn_packable
from espnet_amd.asr.encoder.conformer_encoder import _PositionwiseFeedForward, pack_ffn_rows_w1, pack_ffn_rows_w2
from espnet_amd.nets_utils import SUBSAMPLING_CONVS


class _MultiHeadedAttention(torch.nn.Module):
    """Parameters of transformer/attention.py MultiHeadedAttention: `linear_{q,k,v,out}`."""

    def __init__(self, n_head, n_feat):
        super().__init__()
        self.d_k, self.h = n_feat // n_head, n_head
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)


class _EncoderLayer(torch.nn.Module):
    """Parameters of transformer/encoder_layer.py EncoderLayer: `self_attn`, `feed_forward`, `norm1`, `norm2`."""

    def __init__(self, size, heads, ff):
        super().__init__()
        self.self_attn = _MultiHeadedAttention(heads, size)
        self.feed_forward = _PositionwiseFeedForward(size, ff)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)


class TransformerEncoder(SubsampledEncoderBase):
    _WS_FN, _ENC_FN = "em_transformer_workspace_bytes", "em_transformer_encode"

    @staticmethod
    def _option_check(*, input_layer, pos_enc_class, normalize_before, concat_after, positionwise_layer_type,
                      interctc_layer_idx, interctc_use_conditioning, qk_norm, output_size, attention_heads, linear_units):
        """Options of TransformerEncoder.__init__ that the MI355X kernels do not cover -> (list of "name=value"
        strings, None).  An empty list = the fast path applies."""
        bad = []
        if input_layer not in SUBSAMPLING_CONVS: bad.append(f"input_layer={input_layer}")
        if pos_enc_class is not None and getattr(pos_enc_class, "__name__", str(pos_enc_class)) != "PositionalEncoding":
            bad.append(f"pos_enc_class={getattr(pos_enc_class, '__name__', pos_enc_class)}")
        if not normalize_before: bad.append("normalize_before=False")
        if concat_after: bad.append("concat_after=True")
        if positionwise_layer_type != "linear": bad.append(f"positionwise_layer_type={positionwise_layer_type}")
        if len(interctc_layer_idx or []) > 0 or interctc_use_conditioning: bad.append("interctc")
        if qk_norm: bad.append("qk_norm=True")
        if output_size % 64 or output_size // attention_heads != 64 or output_size % attention_heads:
            bad.append("d_k != 64")
        if linear_units % 64: bad.append("linear_units % 64 != 0")
        return bad, None

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 attention_dropout_rate: float = 0.0, input_layer: Optional[str] = "conv2d", pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False, positionwise_layer_type: str = "linear",
                 positionwise_conv_kernel_size: int = 1, padding_idx: int = -1, interctc_layer_idx: List[int] = [],
                 interctc_use_conditioning: bool = False, layer_drop_rate: float = 0.0, qk_norm: bool = False,
                 use_flash_attn: bool = True, compute_dtype: str = "bfloat16", **unsupported):
        # (the reference takes no other keyword: a Conformer / E-Branchformer option in a transformer encoder_conf is a
        # configuration this class cannot reproduce, reported like Speech2Text's **unsupported)
        bad, _ = self._unsupported(locals())
        if bad:
            raise NotImplementedError("outside the MI355X Transformer-encoder fast path: " + ", ".join(bad))
        super().__init__(input_size, output_size, attention_heads, linear_units, num_blocks, input_layer, compute_dtype,
                         lambda: _EncoderLayer(output_size, attention_heads, linear_units))
        self.normalize_before = normalize_before

    def _build_pack(self, pk):
        A, F, act = pk.A, pk.F, pk.act
        d, ff, Lb = self._output_size, self.linear_units, self.num_blocks
        w = L.EmTransformerWeights()
        w.d, w.heads, w.ff, w.num_blocks, w.n_mels = d, self.heads, ff, Lb, self._input_size
        pk.fill(w, self._pack_embed(pk, w))
        layers = (L.EmTransformerLayer * max(Lb, 1))()
        rows = rows_ffn_packable(act, d, ff)
        for i, l in enumerate(self.encoders):
            sa, fw = l.self_attn, l.feed_forward
            lt = dict(norm1_g=F(l.norm1.weight), norm1_b=F(l.norm1.bias), norm2_g=F(l.norm2.weight),
                      norm2_b=F(l.norm2.bias),
                      wqkv=A(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)),
                      bqkv=F(torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0)),
                      wout=A(sa.linear_out.weight), bout=F(sa.linear_out.bias),
                      ff_w1=A(fw.w_1.weight), ff_b1=F(fw.w_1.bias), ff_w2=A(fw.w_2.weight), ff_b2=F(fw.w_2.bias))
            if rows:  # operand streams of the row-block feed-forward launch (csrc/ffn_rows.hip, ReLU)
                lt.update(ff_w1p=A(pack_ffn_rows_w1(fw.w_1.weight)), ff_w2p=A(pack_ffn_rows_w2(fw.w_2.weight)))
            pk.fill(layers[i], lt)
        w.layers = C.cast(layers, C.POINTER(L.EmTransformerLayer))
        pk.w, pk.layers = w, layers

    def _call_operands(self, T: int, device, pk):
        """pe[:T] (T, d) f32: PositionalEncoding's table (embedding.py extend_pe, the same fp32 torch ops) sliced as the
        reference slices it; one table per device, rebuilt longer (doubling) when an input outgrows it.  Row t depends on
        t alone, so a slice of a longer table is bit-identical to a table built for T."""
        key = (str(device), "abs")
        tab = self._pos_cache.get(key)
        if tab is None or tab.size(0) < T:
            n = max(5000, 2 * tab.size(0) if tab is not None else 0)
            while n < T:
                n *= 2
            tab = abs_pos_table(n, self._output_size).to(torch.float32).to(device)
            self._pos_cache[key] = tab
        return tab[:T], 0
