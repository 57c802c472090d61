"""The streaming Transformer encoder (`encoder: contextual_block_transformer`) on the CPU: the model builds through the
task table, its parameter tree is the reference's, options outside the path are named, tests/cbt_reference.py is
self-consistent, and its weight pack builds through espnet_amd/packing.py like the siblings'."""
import ctypes as C
import inspect

import pytest
import torch

from tests.cbt_reference import RECIPE, TINY, CBTEncoderOracle, run_chunks, seeded_state_dict

CPU = torch.device("cpu")


def _config(enc_conf, vocab=30):
    from oracle.weights import token_list

    return dict(token_list=token_list(vocab), frontend="default",
                frontend_conf=dict(n_fft=512, hop_length=160, win_length=400), normalize="utterance_mvn",
                normalize_conf={}, encoder="contextual_block_transformer", encoder_conf=dict(enc_conf),
                decoder="transformer", decoder_conf=dict(attention_heads=4, linear_units=256, num_blocks=1),
                model_conf=dict(ctc_weight=0.3))


def _expected_keys(n_layers):
    keys = [f"embed.conv.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")] + ["embed.out.weight", "embed.out.bias"]
    for n in range(n_layers):
        keys += [f"encoders.{n}.self_attn.linear_{x}.{p}" for x in ("q", "k", "v", "out") for p in ("weight", "bias")]
        keys += [f"encoders.{n}.feed_forward.w_{x}.{p}" for x in (1, 2) for p in ("weight", "bias")]
        keys += [f"encoders.{n}.norm{x}.{p}" for x in (1, 2) for p in ("weight", "bias")]
    return sorted(keys + ["after_norm.weight", "after_norm.bias"])


def test_build_model_and_state_dict_keys():
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder
    from espnet_amd.tasks.asr import ASRTask

    torch.manual_seed(0)
    model = ASRTask.build_model(_config(TINY))
    enc = model.encoder
    assert type(enc) is ContextualBlockTransformerEncoder and enc.output_size() == 128
    assert sorted(enc.state_dict()) == _expected_keys(2)
    sd = seeded_state_dict(enc, 3)
    enc.load_state_dict(sd, strict=True)
    back = enc.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)


def test_constructor_signature_is_the_reference_one():
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder

    ps = inspect.signature(ContextualBlockTransformerEncoder.__init__).parameters
    want = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=6, dropout_rate=0.1,
                positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d", normalize_before=True,
                concat_after=False, positionwise_layer_type="linear", positionwise_conv_kernel_size=1, padding_idx=-1,
                block_size=40, hop_size=16, look_ahead=16, init_average=True, ctx_pos_enc=True, compute_dtype="bfloat16")
    names = [n for n, p in ps.items() if p.kind is p.POSITIONAL_OR_KEYWORD and n != "self"]
    assert names == ["input_size", "output_size", "attention_heads", "linear_units", "num_blocks", "dropout_rate",
                     "positional_dropout_rate", "attention_dropout_rate", "input_layer", "pos_enc_class",
                     "normalize_before", "concat_after", "positionwise_layer_type", "positionwise_conv_kernel_size",
                     "padding_idx", "block_size", "hop_size", "look_ahead", "init_average", "ctx_pos_enc", "compute_dtype"]
    assert ps["input_size"].default is inspect.Parameter.empty
    for k, v in want.items():
        assert ps[k].default == v, k
    # the reference's default is its StreamPositionalEncoding class, which this package does not define: None stands for it
    assert ps["pos_enc_class"].default is None


@pytest.mark.parametrize("kw,named", [
    (dict(input_layer="linear"), "input_layer"), (dict(normalize_before=False), "normalize_before"),
    (dict(concat_after=True), "concat_after"), (dict(positionwise_layer_type="conv1d"), "positionwise_layer_type"),
    (dict(pos_enc_class=torch.nn.Identity), "pos_enc_class"), (dict(init_average=False), "init_average"),
    (dict(ctx_pos_enc=False), "ctx_pos_enc"), (dict(output_size=256, attention_heads=2), "d_k"),
    (dict(linear_units=1000), "linear_units"), (dict(block_size=63), "block_size"),
    (dict(macaron_style=True), "macaron_style")])
def test_unsupported_options_are_named(kw, named):
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder as E

    with pytest.raises(NotImplementedError, match=named):
        E(80, **kw)
    assert any(named in s for s in E.unsupported_options(80, **kw))
    assert E.unsupported_options(80) == []


def test_streaming_inference_names_both_encoders():
    import types

    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming

    src = inspect.getsource(Speech2TextStreaming.__init__)
    assert "contextual_block_conformer" in src and "contextual_block_transformer" in src
    assert types  # (the class needs a GPU to construct: tests/test_gpu_cbt.py drives it)


def test_cbt_reference_chunking_invariance():
    """As the streaming chunking-invariance test does for the Conformer: 37- and 64-frame chunks and one shot agree."""
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder as E

    enc = E(80, compute_dtype="float32", **TINY)
    sd = seeded_state_dict(enc, 5)
    orc = CBTEncoderOracle(sd, TINY["attention_heads"], TINY["num_blocks"])
    feats = torch.randn(601, 80, generator=torch.Generator().manual_seed(6))
    a, la = run_chunks(orc, feats, 37)
    b, lb = run_chunks(orc, feats, 64)
    c, lc = run_chunks(orc, feats, 10 ** 6)
    assert a.shape == b.shape == c.shape == (149, 128) and sum(la) == sum(lb) == lc[0]
    print(f"[cbt reference] chunked vs one-shot {(a - c).abs().max().item():.2e} {(b - c).abs().max().item():.2e}")
    assert (a - b).abs().max().item() < 1e-4 and (a - c).abs().max().item() < 1e-4
    short, _ = run_chunks(orc, feats[:100], 10 ** 6)  # the short-utterance path: no context slots
    assert short.shape == (24, 128)
    # the subclass overrides the layer stack only
    from oracle.streaming import CBEncoderOracle

    own = {k for k, v in vars(CBTEncoderOracle).items() if callable(v)}
    assert own == {"_layers"} and CBTEncoderOracle.forward_infer is CBEncoderOracle.forward_infer


def _pointers(pk):
    out = []
    for tag, s in [("w", pk.w)] + [(f"layers[{i}]", s) for i, s in enumerate(pk.layers)]:
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ is C.c_void_p and v:
                out.append((f"{tag}.{name}", v))
    return out


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_pack_builds_on_cpu_and_is_not_the_conformers(dtype):
    from espnet_amd.asr.encoder.contextual_block_conformer_encoder import ContextualBlockConformerEncoder
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder

    tf = ContextualBlockTransformerEncoder(80, 256, 4, 512, 2, compute_dtype=dtype)
    cf = ContextualBlockConformerEncoder(80, 256, 4, 512, 2, macaron_style=True, cnn_module_kernel=15, compute_dtype=dtype)
    pk, pc = tf.packed(CPU), cf.packed(CPU)
    held = {t.data_ptr() for t in pk.keep}
    ptrs = _pointers(pk)
    assert len(ptrs) >= 9
    for field, addr in ptrs:
        assert addr in held, field
    with pytest.raises(AttributeError):
        pk.w = None
    # equal sizes, never one pack: each module owns its build (a serial of its own, structs of its own type)
    assert pk is not pc and pk.serial != pc.serial and type(pk.w) is not type(pc.w)
    assert tf.packed(CPU) is pk and cf.packed(CPU) is pc
    fused = dtype == "bfloat16"
    assert tf._fusable() == fused
    lay = pk.layers[0]
    assert all(bool(getattr(lay, n)) == fused for n in ("cb_wqkvp", "cb_woutp", "cb_ff_w1p", "cb_ff_w2p", "fp_t"))
    tf.load_state_dict(tf.state_dict())
    assert tf.packed(CPU) is not pk  # a reload gives a new pack


def test_recipe_shape_parameter_groups():
    """fp_t: [norm1 g | b | bq bk bv] [bout | norm2 g | b | ff b2] [the next layer's first group], 1792 floats each."""
    from espnet_amd import lib as L
    from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder

    conf = dict(RECIPE, num_blocks=2, linear_units=256)
    enc = ContextualBlockTransformerEncoder(80, compute_dtype="bfloat16", **conf)
    enc.load_state_dict(seeded_state_dict(enc, 9))
    pk = enc.packed(CPU)
    G = L.EM_BLOCK_PARAM_GROUP
    fps = [t for t in pk.keep if t.dtype == torch.float32 and t.numel() == 3 * G]
    assert len(fps) == 2
    l0, l1 = enc.encoders[0], enc.encoders[1]
    g = fps[0].view(3, G)
    assert torch.equal(g[0, :256], l0.norm1.weight.detach()) and torch.equal(g[0, 512:768], l0.self_attn.linear_q.bias.detach())
    assert torch.equal(g[1, :256], l0.self_attn.linear_out.bias.detach()) and torch.equal(g[1, 768:1024], l0.feed_forward.w_2.bias.detach())
    assert torch.equal(g[2, 256:512], l1.norm1.bias.detach()) and torch.equal(g[2, 1024:1280], l1.self_attn.linear_v.bias.detach())
    assert fps[1].view(3, G)[2].abs().max().item() == 0.0


def test_espnet2_adapter_registers_and_falls_back():
    """The reference-side binding: `mi355x_contextual_block_transformer` is an AbsEncoder, registers in the reference's encoder
    table, and options outside the path build the stock class.  Needs espnet2."""
    pytest.importorskip("espnet2")
    from espnet2.asr.encoder.abs_encoder import AbsEncoder
    from espnet2.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder as Stock

    from espnet_amd.integration import espnet2_adapters as A

    cls = A.ADAPTERS["encoder"]["mi355x_contextual_block_transformer"]
    enc = cls(80, output_size=128, attention_heads=2, linear_units=256, num_blocks=1)
    assert isinstance(enc, cls) and isinstance(enc, AbsEncoder)
    stock = cls(80, output_size=128, attention_heads=2, linear_units=256, num_blocks=1, concat_after=True)
    assert type(stock) is Stock
    tables = A.register()
    assert tables["encoder"].classes["mi355x_contextual_block_transformer"] is cls
