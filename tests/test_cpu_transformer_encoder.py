"""Transformer encoder (encoder: transformer) without a GPU: the parameter tree against the reference naming, the options
outside the fast path, and the CPU restatement (tests/transformer_ref.py) against the oracle pieces it is built from."""
import math
import types

import pytest
import torch

from oracle import conformer as oc
from oracle.beam_search import DecoderOracle, abs_pos_table
from tests import transformer_ref as tr


def _enc(**kw):
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder

    return TransformerEncoder(**{"input_size": 80, **kw})


def test_state_dict_keys_follow_the_reference_naming():
    d, ff, n, F2 = 256, 1024, 2, 19  # conv2d over 80 mel bins: ((80 - 1) // 2 - 1) // 2 = 19
    want = {"embed.conv.0.weight": (d, 1, 3, 3), "embed.conv.0.bias": (d,), "embed.conv.2.weight": (d, d, 3, 3),
            "embed.conv.2.bias": (d,), "embed.out.weight": (d, d * F2), "embed.out.bias": (d,),
            "after_norm.weight": (d,), "after_norm.bias": (d,)}
    for i in range(n):
        p = f"encoders.{i}."
        for name in ("linear_q", "linear_k", "linear_v", "linear_out"):
            want[p + f"self_attn.{name}.weight"], want[p + f"self_attn.{name}.bias"] = (d, d), (d,)
        want[p + "feed_forward.w_1.weight"], want[p + "feed_forward.w_1.bias"] = (ff, d), (ff,)
        want[p + "feed_forward.w_2.weight"], want[p + "feed_forward.w_2.bias"] = (d, ff), (d,)
        for name in ("norm1", "norm2"):
            want[p + f"{name}.weight"], want[p + f"{name}.bias"] = (d,), (d,)
    enc = _enc(output_size=d, attention_heads=4, linear_units=ff, num_blocks=n)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want
    assert enc.output_size() == d
    e8 = _enc(output_size=d, num_blocks=1, input_layer="conv2d8")
    assert "embed.conv.4.weight" in e8.state_dict()


@pytest.mark.parametrize("kw", [dict(input_layer="linear"), dict(input_layer="embed"), dict(normalize_before=False),
                                dict(concat_after=True), dict(positionwise_layer_type="conv1d"),
                                dict(interctc_layer_idx=[1]), dict(interctc_use_conditioning=True), dict(qk_norm=True),
                                dict(output_size=256, attention_heads=8), dict(output_size=200, attention_heads=4),
                                dict(linear_units=1000),
                                dict(pos_enc_class=types.SimpleNamespace(__name__="ScaledPositionalEncoding"))])
def test_options_outside_the_fast_path_raise_and_are_reported(kw):
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder

    with pytest.raises(NotImplementedError):
        _enc(**kw)
    assert TransformerEncoder.unsupported_options(80, **kw)


@pytest.mark.parametrize("kw", [dict(macaron_style=True), dict(use_cnn_module=True), dict(rel_pos_type="latest"),
                                dict(pos_enc_layer_type="rel_pos"), dict(selfattention_layer_type="rel_selfattn"),
                                dict(cnn_module_kernel=31)])
def test_foreign_keywords_raise_and_are_reported(kw):
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder

    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        _enc(**kw)
    assert any(next(iter(kw)) in s for s in TransformerEncoder.unsupported_options(80, **kw))


def test_fast_path_options_build_and_report_nothing():
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder

    for kw in (dict(), dict(input_layer="conv2d6"), dict(input_layer="conv2d8"),
               dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=1),
               dict(dropout_rate=0.2, positional_dropout_rate=0.2, attention_dropout_rate=0.1, layer_drop_rate=0.0,
                    positionwise_conv_kernel_size=1, padding_idx=-1, use_flash_attn=False),
               dict(pos_enc_class=types.SimpleNamespace(__name__="PositionalEncoding"))):
        _enc(**kw)
        assert TransformerEncoder.unsupported_options(80, **kw) == []


def test_registry_builds_a_transformer_model():
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder
    from espnet_amd.tasks.asr import ASRTask

    cfg = dict(token_list=["<blank>", "a", "b", "<sos/eos>"], frontend="default", frontend_conf=dict(n_fft=512, hop_length=160),
               normalize="utterance_mvn", encoder="transformer",
               encoder_conf=dict(output_size=256, attention_heads=4, linear_units=512, num_blocks=2),
               decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
               compute_dtype="float32")
    model = ASRTask.build_model(cfg)
    assert isinstance(model.encoder, TransformerEncoder)


def _sd(d=128, ff=256, n=2, heads=2, seed=0, kind="conv2d", D=20):
    from espnet_amd.nets_utils import SUBSAMPLING_CONVS, conv_out_size

    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 1
    for i, (k, s) in enumerate(SUBSAMPLING_CONVS[kind]):
        sd[f"encoder.embed.conv.{2 * i}.weight"] = torch.randn(d, cin, k, k, generator=g) / math.sqrt(cin * k * k)
        sd[f"encoder.embed.conv.{2 * i}.bias"] = 0.1 * torch.randn(d, generator=g)
        cin = d
    fin = d * conv_out_size(D, kind)
    sd["encoder.embed.out.weight"] = torch.randn(d, fin, generator=g) / math.sqrt(fin)
    sd["encoder.embed.out.bias"] = 0.1 * torch.randn(d, generator=g)
    for name, shape in [("after_norm.weight", (d,)), ("after_norm.bias", (d,))]:
        sd["encoder." + name] = 1.0 + 0.1 * torch.randn(shape, generator=g) if name.endswith("weight") else 0.1 * torch.randn(shape, generator=g)
    for i in range(n):
        p = f"encoder.encoders.{i}."
        for nm in ("linear_q", "linear_k", "linear_v", "linear_out"):
            sd[p + f"self_attn.{nm}.weight"] = torch.randn(d, d, generator=g) / math.sqrt(d)
            sd[p + f"self_attn.{nm}.bias"] = 0.05 * torch.randn(d, generator=g)
        sd[p + "feed_forward.w_1.weight"] = torch.randn(ff, d, generator=g) / math.sqrt(d)
        sd[p + "feed_forward.w_1.bias"] = 0.05 * torch.randn(ff, generator=g)
        sd[p + "feed_forward.w_2.weight"] = torch.randn(d, ff, generator=g) / math.sqrt(ff)
        sd[p + "feed_forward.w_2.bias"] = 0.05 * torch.randn(d, generator=g)
        for nm in ("norm1", "norm2"):
            sd[p + f"{nm}.weight"] = 1.0 + 0.1 * torch.randn(d, generator=g)
            sd[p + f"{nm}.bias"] = 0.1 * torch.randn(d, generator=g)
    return sd


@pytest.mark.parametrize("kind", ["conv2d", "conv2d6", "conv2d8"])
def test_restatement_without_layers_is_the_embedding(kind):
    sd = _sd(kind=kind)
    feats = torch.randn(2, 60, 20, generator=torch.Generator().manual_seed(1))
    flens = torch.tensor([60, 41])
    out, olens = tr.transformer_encoder(sd, feats, flens, heads=2, num_blocks=0)
    x = oc.conv2d_subsampling(sd, feats)
    T, d = x.size(1), x.size(2)
    want = oc.layer_norm(x * math.sqrt(d) + abs_pos_table(T, d)[None], sd, "encoder.after_norm.")
    assert torch.equal(out, want)
    assert olens.tolist() == oc.subsampled_lengths(flens, 60, kind).tolist()
    with pytest.raises(oc.TooShortUttError):
        tr.transformer_encoder(sd, feats[:, : oc.SHORT_LIMIT[kind] - 1], flens.clamp(max=3), heads=2, num_blocks=0)


def test_restatement_attention_without_padding_is_the_decoder_oracles():
    g = torch.Generator().manual_seed(3)
    B, T, h, d = 3, 11, 4, 256
    q, k, v = (torch.randn(B, T, d, generator=g) for _ in range(3))
    mine = tr.attend(q, k, v, torch.ones(B, T, dtype=torch.bool), h)
    me = types.SimpleNamespace(h=h, dk=d // h, d=d)
    for t in range(T):
        ref = DecoderOracle._mha(me, q[:, t : t + 1], k, v)
        assert torch.allclose(mine[:, t : t + 1], ref, atol=1e-6, rtol=1e-5), t
    assert torch.equal(tr.attend(q, k, v, None, h), mine)
    # a padded key changes nothing when it is masked
    valid = torch.ones(B, T + 2, dtype=torch.bool)
    valid[:, T:] = False
    pad = torch.cat([k, 100 * torch.randn(B, 2, d, generator=g)], 1), torch.cat([v, torch.randn(B, 2, d, generator=g)], 1)
    assert torch.allclose(tr.attend(q, pad[0], pad[1], valid, h), mine, atol=1e-6)
