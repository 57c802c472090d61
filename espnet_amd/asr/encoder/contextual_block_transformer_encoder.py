"""ContextualBlockTransformerEncoder (streaming) on the MI355X.

Mirrors espnet2/asr/encoder/contextual_block_transformer_encoder.py for streaming inference: the constructor keywords,
`output_size()`, `forward(xs_pad, ilens, prev_states, is_final=..., infer_mode=True)` and `forward_infer` with the
reference's state dictionary, and the reference's state-dict keys (`embed.conv.{0,2}`, `embed.out`,
`encoders.N.{self_attn.linear_{q,k,v,out}, feed_forward.w_{1,2}, norm1, norm2}`, `after_norm`), so reference checkpoints
load unchanged.

The class is the contextual-block Conformer encoder with a plainer layer
(transformer/contextual_block_encoder_layer.py forward_infer, normalize_before, no concat_after):
    x = x + self_attn(norm1(x), mask);  x = x + w_2(relu(w_1(norm2(x))))
Everything around the layer stack - Conv2dSubsamplingWOPosEnc, StreamPositionalEncoding, the whole of `forward_infer` - is
the reference's same code and here the same host code: `_contextual_block_base.ContextualBlockEncoderBase`.  This file has
the parameter containers, the weight pack and the names of the C entries (csrc/streaming_tf.hip; the fused layer's launches
are csrc/block.hip EM_BLOCK_Q / EM_BLOCK_T).  The torch.nn layers are parameter containers only.
"""
import ctypes as C
import inspect
from typing import List, Optional

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table
from espnet_amd.asr.encoder._contextual_block_base import ContextualBlockEncoderBase
from espnet_amd.asr.encoder.conformer_encoder import LayerNorm, _PositionwiseFeedForward
from espnet_amd.asr.encoder.contextual_block_conformer_encoder import _Conv2dSubsamplingWOPosEnc, _MultiHeadedAttention


class _ContextualBlockEncoderLayer(torch.nn.Module):
    """Parameters of transformer/contextual_block_encoder_layer.py ContextualBlockEncoderLayer (concat_after=False)."""

    def __init__(self, size, heads, ff):
        super().__init__()
        self.self_attn = _MultiHeadedAttention(heads, size)
        self.feed_forward = _PositionwiseFeedForward(size, ff)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)


class ContextualBlockTransformerEncoder(ContextualBlockEncoderBase):
    _WS_FN, _ENC_FN, _ENC_BATCH_FN = "em_cbt_workspace_bytes", "em_cbt_encode_blocks", "em_cbt_encode_blocks_batch"

    @staticmethod
    def _option_check(*, input_layer, pos_enc_class, normalize_before, concat_after, positionwise_layer_type,
                      init_average, ctx_pos_enc, output_size, attention_heads, linear_units, block_size):
        """Options of ContextualBlockTransformerEncoder.__init__ outside the MI355X path -> list of "name=value" strings
        (empty: the fast path applies)."""
        bad = []
        if input_layer != "conv2d": bad.append(f"input_layer={input_layer}")
        if not normalize_before: bad.append("normalize_before=False")
        if concat_after: bad.append("concat_after=True")
        if positionwise_layer_type != "linear": bad.append(f"positionwise_layer_type={positionwise_layer_type}")
        # (the reference's default is the StreamPositionalEncoding class itself: that one is what the kernels compute)
        if pos_enc_class is not None and getattr(pos_enc_class, "__name__", "") != "StreamPositionalEncoding":
            bad.append(f"pos_enc_class={getattr(pos_enc_class, '__name__', pos_enc_class)}")
        if not init_average: bad.append("init_average=False")
        if not ctx_pos_enc: bad.append("ctx_pos_enc=False")
        if attention_heads <= 0 or output_size % 64 or output_size % attention_heads or \
                output_size // attention_heads not in (32, 64):
            bad.append("d_k not in {32,64}")
        if linear_units % 64: bad.append("linear_units % 64 != 0")
        if block_size <= 0 or block_size + 2 > 64: bad.append(f"block_size={block_size}")
        return bad

    @classmethod
    def unsupported_options(cls, *args, **kwargs) -> List[str]:
        """The constructor arguments outside the fast path (reference defaults applied; keywords the reference class does
        not take included), without building anything."""
        ba = inspect.signature(cls.__init__).bind(None, *args, **kwargs)
        ba.apply_defaults()
        foreign = [f"{k}={v!r} (not a ContextualBlockTransformerEncoder keyword)"
                   for k, v in ba.arguments.get("unsupported", {}).items()]
        names = inspect.signature(cls._option_check).parameters
        return foreign + cls._option_check(**{k: ba.arguments[k] for k in names})

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048,
                 num_blocks: int = 6, dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1,
                 attention_dropout_rate: float = 0.0, input_layer: Optional[str] = "conv2d", pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False, positionwise_layer_type: str = "linear",
                 positionwise_conv_kernel_size: int = 1, padding_idx: int = -1, block_size: int = 40, hop_size: int = 16,
                 look_ahead: int = 16, init_average: bool = True, ctx_pos_enc: bool = True,
                 compute_dtype: str = "bfloat16", **unsupported):
        # (pos_enc_class=None stands for the reference's default, StreamPositionalEncoding: this package has no such class
        # to name - the table is built by the pack and applied by the block-assembly kernel)
        super().__init__()
        bad = [f"{k}={v!r} (not a ContextualBlockTransformerEncoder keyword)" for k, v in unsupported.items()]
        bad += self._option_check(
            input_layer=input_layer, pos_enc_class=pos_enc_class, normalize_before=normalize_before,
            concat_after=concat_after, positionwise_layer_type=positionwise_layer_type, init_average=init_average,
            ctx_pos_enc=ctx_pos_enc, output_size=output_size, attention_heads=attention_heads, linear_units=linear_units,
            block_size=block_size)
        if bad:
            raise NotImplementedError("outside the MI355X streaming-Transformer fast path: " + ", ".join(bad))
        self._output_size, self._input_size = output_size, input_size
        self.heads, self.linear_units, self.num_blocks = attention_heads, linear_units, num_blocks
        self.normalize_before = normalize_before
        self.block_size, self.hop_size, self.look_ahead = block_size, hop_size, look_ahead
        self.init_average, self.ctx_pos_enc = init_average, ctx_pos_enc
        self.subsample = 4
        self.compute_dtype = compute_dtype
        self.embed = _Conv2dSubsamplingWOPosEnc(input_size, output_size)
        self.encoders = torch.nn.ModuleList(
            [_ContextualBlockEncoderLayer(output_size, attention_heads, linear_units) for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self._ws = {}
        self._flen_cache = {}  # (streams, frames, device) -> per-stream frame counts on the device (_embed_device_batch)

    # ------------------------------------------------------------------ packing (load time)
    def _build_pack(self, pk):
        A, F = pk.A, pk.F
        d, ff, NL = self._output_size, self.linear_units, self.num_blocks
        e = self.embed
        F2 = e.out.in_features // d
        w = L.EmTransformerWeights()
        w.d, w.heads, w.ff, w.num_blocks, w.n_mels, w.subsample = d, self.heads, ff, NL, self._input_size, 4
        top = dict(conv1_w=F(e.conv[0].weight.reshape(d, 9)), conv1_b=F(e.conv[0].bias),
                   conv2_w=A(e.conv[2].weight.permute(0, 2, 3, 1).reshape(d, 9 * d)),
                   conv2_b=F(e.conv[2].bias),
                   embed_w=A(e.out.weight.reshape(d, d, F2).permute(0, 2, 1).reshape(d, F2 * d)),
                   embed_b=F(e.out.bias), after_norm_g=F(self.after_norm.weight),
                   after_norm_b=F(self.after_norm.bias))
        pk.fill(w, top)
        layers = (L.EmTransformerLayer * max(NL, 1))()
        fusable = self._fusable()
        for i, l in enumerate(self.encoders):
            sa, fw = l.self_attn, l.feed_forward
            lt = dict(norm1_g=F(l.norm1.weight), norm1_b=F(l.norm1.bias), norm2_g=F(l.norm2.weight),
                      norm2_b=F(l.norm2.bias),
                      wqkv=A(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0)),
                      bqkv=F(torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0)),
                      wout=A(sa.linear_out.weight), bout=F(sa.linear_out.bias),
                      ff_w1=A(fw.w_1.weight), ff_b1=F(fw.w_1.bias), ff_w2=A(fw.w_2.weight), ff_b2=F(fw.w_2.bias))
            if fusable:
                nxt = self.encoders[i + 1] if i + 1 < NL else None
                lt.update(self._fused_layer(l, nxt, A, F))
            pk.fill(layers[i], lt)
        w.layers = C.cast(layers, C.POINTER(L.EmTransformerLayer))
        pk.w, pk.layers = w, layers
        pk.pe = F(abs_pos_table(5000, d))  # StreamPositionalEncoding.extend_pe (embedding.py:357-374)

    def _fusable(self) -> bool:
        """Shapes the fused streaming layer covers (csrc/streaming_tf.hip `fusable`, csrc/block.hip EM_BLOCK_Q / EM_BLOCK_T):
        bf16, 256 wide, 4 heads, feed-forward width a multiple of 128 up to 4096 - the streaming-Transformer recipe.
        Everything else keeps the six launches per layer."""
        return (bool(getattr(self, "fused", True))  # (`enc.fused = False` + `invalidate()`: A/B and bisecting)
                and self.em_dtype == L.EM_BF16 and self._output_size == 256 and self.heads == 4
                and self.linear_units % 128 == 0 and self.linear_units <= 4096)

    def plan(self, n_streams: int = 1, n_blk: int = 1, has_ctx: bool = True, device="cuda") -> int:
        """Which launch sequence a call of `n_streams` streams x `n_blk` blocks takes (include/espnet_amd.h
        em_cbt_encode_plan): 0 per-operator, 1 row-block launches + hand-over launch, 2 hand-over folded in (two launches
        per layer), 3 a layer's second launch merged with the next layer's first."""
        pk = self.packed(torch.device(device))
        return int(L.load().em_cbt_encode_plan(self.em_dtype, C.byref(pk.w), n_streams, n_blk, self.block_size + 2, 1,
                                               int(has_ctx)))

    def _fused_layer(self, l, nxt, A, F):
        """Operands of the row-block launches for one layer (include/espnet_amd.h, EmTransformerLayer.cb_* / fp_t): weights
        in fragment-major units (`pack_k_units` / `pack_w1` / `pack_w2` of the Conformer encoder), and three groups of
        EM_BLOCK_PARAM_GROUP floats: this layer's [norm1 g | b | bq bk bv], [bout | norm2 g | b | ff b2], and the next
        layer's first group (what the merged launch normalises with; zeros behind the last layer).  The first FFN bias is
        read from the row-major `ff_b1`."""
        from espnet_amd.asr.encoder.conformer_encoder import pack_k_units, pack_w1, pack_w2

        G = L.EM_BLOCK_PARAM_GROUP

        def group(*vecs):
            v = torch.cat([t.detach().to(torch.float32).reshape(-1).cpu() for t in vecs])
            assert v.numel() <= G
            return torch.nn.functional.pad(v, (0, G - v.numel()))

        def q_group(m):
            sa = m.self_attn
            return group(m.norm1.weight, m.norm1.bias, sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias)

        sa, fw = l.self_attn, l.feed_forward
        fp = torch.cat([q_group(l), group(sa.linear_out.bias, l.norm2.weight, l.norm2.bias, fw.w_2.bias),
                        q_group(nxt) if nxt is not None else torch.zeros(G)])
        return dict(
            cb_wqkvp=A(pack_k_units(torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0))),
            cb_woutp=A(pack_k_units(sa.linear_out.weight)), cb_ff_w1p=A(pack_w1(fw.w_1.weight)),
            cb_ff_w2p=A(pack_w2(fw.w_2.weight)), fp_t=F(fp))
