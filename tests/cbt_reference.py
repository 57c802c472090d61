"""CPU fp32 restatement of the reference's streaming (contextual block) TRANSFORMER encoder, for the tests of
espnet_amd.asr.encoder.contextual_block_transformer_encoder (test infrastructure: never on the product path).

Restates
  * ContextualBlockTransformerEncoder.forward_infer  (espnet2/asr/encoder/contextual_block_transformer_encoder.py)
  * ContextualBlockEncoderLayer.forward_infer        (espnet2/legacy/nets/pytorch_backend/transformer/
                                                      contextual_block_encoder_layer.py; normalize_before=True,
                                                      concat_after=False)
over the reference's flat state dict.  In the reference the encoder is the contextual-block Conformer encoder with a plainer
layer: the buffering, block assembly, mask, short-utterance path, stitching and carried state are the same code.  So this is
`oracle.streaming.CBEncoderOracle` - pinned against the reference class by tests/golden/stream_*.npz - with `_layers`
overridden and nothing else: the state machine it runs is the golden-pinned one.
"""
import torch

from oracle.streaming import CBEncoderOracle, _lin, _ln, plain_mha


def cbt_layer_infer(sd, x, mask, pre, h):
    """x = x + self_attn(norm1(x), mask); x = x + w_2(relu(w_1(norm2(x)))): residual scale 1, no macaron module, no
    convolution module, no norm_final.  x (n_blk, L, d); the context hand-over is the caller's."""
    x = x + plain_mha(sd, _ln(x, sd, pre + "norm1."), mask, pre + "self_attn.", h)
    t = _ln(x, sd, pre + "norm2.")
    return x + _lin(torch.relu(_lin(t, sd, pre + "feed_forward.w_1.")), sd, pre + "feed_forward.w_2.")


class CBTEncoderOracle(CBEncoderOracle):
    def _layers(self, x, mask, past_ctx, short):
        """CBEncoderOracle._layers with the Transformer layer in place of the Conformer layer (the hand-over unchanged)."""
        next_ctx = None if short else torch.zeros(self.nl, self.d)
        for l in range(self.nl):
            x = cbt_layer_infer(self.sd, x, mask, f"encoders.{l}.", self.h)
            if not short:
                x = x.clone()
                x[0, 0] = x[0, -1] if past_ctx is None else past_ctx[l]
                if x.size(0) > 1:
                    x[1:, 0] = x[:-1, -1]
                next_ctx[l] = x[-1, -1]
        return x, next_ctx


def run_chunks(oracle, feats, chunk):
    """Feed feats (t, idim) `chunk` frames at a time (last call final) -> (ys (t_out, d), frames emitted per call)."""
    outs, lens, state, pos = [], [], None, 0
    while pos < feats.size(0):
        nxt = min(feats.size(0), pos + chunk)
        y, state = oracle.forward_infer(feats[pos:nxt], state, nxt == feats.size(0))
        outs.append(y)
        lens.append(int(y.size(0)))
        pos = nxt
    return torch.cat(outs, 0), lens


# The two configurations of tests/test_gpu_cbt.py: tiny (per-operator launches) and the streaming recipe (fused launches)
TINY = dict(output_size=128, attention_heads=2, linear_units=256, num_blocks=2, block_size=40, hop_size=16, look_ahead=16)
RECIPE = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, block_size=40, hop_size=16, look_ahead=16)


def seeded_state_dict(module, seed):
    """A seeded random state dict for `module` with weights of a trained model's scale: matrices N(0, 1 / fan_in), LayerNorm
    gains around 1, small biases - so that activations stay O(1) through the stack."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in module.state_dict().items():
        if v.dim() >= 2:
            fan_in = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) / fan_in ** 0.5
        elif k.endswith("weight"):  # LayerNorm gain
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
    return sd
