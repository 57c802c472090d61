"""The models, inputs and error bounds that tests/test_cpu_dec_seq.py and tests/test_gpu_dec_seq.py share: the CPU test
shows that each defect a bound is meant to catch (tests/dec_seq_ref.py DEFECTS) moves some scored nll of every model by
more than four times the largest bf16 bound, the GPU tests hold the device to the bounds.

Bounds follow the repository's rule (tests/lm_nll_cases.py): measured against the float64 restatement
(tests/dec_seq_ref.py) on the same rounded weights and memories, constant = 4 x the largest value of the first run, which
is kept in profiles/dec_seq_first_run.txt.
"""
import torch

from oracle.weights import recipe_state_dict, token_list

# (vocabulary, heads, weight seed): d = 128 (d_k 64 with 2 heads, 32 with 4), 2 layers, 256 units; V = 1027 spans three
# 512-column slices of the vocabulary head with a partial last tile.
MODELS = {"h2": (300, 2, 21), "h4": (1027, 4, 22)}
D, UNITS, LAYERS = 128, 256, 2
WIDTHS = (1, 2, 17, 65)  # Lp = longest transcript + 1: one position, two, just over a 16-query tile, several 32-key tiles
T_MEM = 45  # frames of the chain tests' memories: a full 32-frame tile and a partial one
HLENS = (45, 1, 23)
PAD_NOISE = 5.0  # the frames at and behind hlens hold N(0, 5^2): a forgotten memory mask is loud

# Largest errors of the first run (profiles/dec_seq_first_run.txt) x 4:
#   |nll - float64 restatement| per scored token of the tiny models (nll values up to 13.8): f32 7.608e-6, bf16 9.371e-2;
#   |ctx - restatement| of the stand-alone source attention (contexts of order 1): f32 2.246e-6, bf16 8.794e-3.
# The models' scales (state_dict) were fixed before that run, from the restatement's defects alone.
E_NLL = {"float32": 3.0e-5, "bfloat16": 3.7e-1}
E_SRC = {"float32": 9.0e-6, "bfloat16": 3.5e-2}


def decoder_shapes(V, d=D, ff=UNITS, layers=LAYERS):
    s = {"decoder.embed.0.weight": (V, d), "decoder.after_norm.weight": (d,), "decoder.after_norm.bias": (d,),
         "decoder.output_layer.weight": (V, d), "decoder.output_layer.bias": (V,)}
    for l in range(layers):
        p = f"decoder.decoders.{l}."
        for a in ("self_attn", "src_attn"):
            for lin in ("linear_q", "linear_k", "linear_v", "linear_out"):
                s[f"{p}{a}.{lin}.weight"], s[f"{p}{a}.{lin}.bias"] = (d, d), (d,)
        s[p + "feed_forward.w_1.weight"], s[p + "feed_forward.w_1.bias"] = (ff, d), (ff,)
        s[p + "feed_forward.w_2.weight"], s[p + "feed_forward.w_2.bias"] = (d, ff), (d,)
        for n in ("norm1", "norm2", "norm3"):
            s[f"{p}{n}.weight"], s[f"{p}{n}.bias"] = (d,), (d,)
    return s


def state_dict(name):
    """Recipe weights (oracle.weights) of decoder `name`, rescaled so that the defects of tests/dec_seq_ref.py are loud.
    The recipe's matrices are torch's default initialisation: every attention is close to uniform, its output small
    beside the embedding (N(0, 1) * sqrt(d)), and no mask or position matters (a forgotten memory mask moved no nll by
    more than 0.79, a wrong causal mask by 0.14).  So, as tests/lm_nll_cases.py does: the query and key projections x 4
    (attention that prefers some keys), the value and output projections x 2, the vocabulary head x 3 (logits a few
    units apart), the embedding table x 0.1 (x * sqrt(d) and pe[j] of one size).  Every defect then moves some nll by
    2.4 and more (tests/test_cpu_dec_seq.py::test_defects_are_visible prints them)."""
    V, heads, seed = MODELS[name]
    sd = recipe_state_dict(decoder_shapes(V), seed, skip=())
    for k in sd:
        if k.endswith("linear_q.weight") or k.endswith("linear_k.weight"):
            sd[k] = sd[k] * 4.0
        elif k.endswith("linear_v.weight") or k.endswith("linear_out.weight"):
            sd[k] = sd[k] * 2.0
    sd["decoder.output_layer.weight"] = sd["decoder.output_layer.weight"] * 3.0
    sd["decoder.embed.0.weight"] = sd["decoder.embed.0.weight"] * 0.1
    return sd


def build_model(name, compute_dtype="float32"):
    """ESPnetASRModel around TransformerDecoder `name` alone (no frontend, encoder or CTC head: `nll` needs none)."""
    from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet_amd.asr.espnet_model import ESPnetASRModel

    V, heads, _ = MODELS[name]
    dec = TransformerDecoder(V, D, attention_heads=heads, linear_units=UNITS, num_blocks=LAYERS, compute_dtype=compute_dtype)
    model = ESPnetASRModel(V, token_list(V), frontend=None, specaug=None, normalize=None, preencoder=None, encoder=None,
                           postencoder=None, decoder=dec, ctc=None, ctc_weight=0.0)
    model.load_state_dict(state_dict(name), strict=True)
    return model.eval()


def make_memory(seed, Bm=len(HLENS), T=T_MEM, hlens=HLENS, pad=PAD_NOISE, round_to=None):
    """(memory (Bm, T, D) float32, hlens): valid frames N(0, 1), the padded ones N(0, pad^2); rounded through `round_to`
    where the device holds the memory in bf16."""
    g = torch.Generator().manual_seed(seed)
    mem = torch.randn(Bm, T, D, generator=g)
    noise = torch.randn(Bm, T, D, generator=g) * pad
    hl = torch.tensor(hlens, dtype=torch.long)
    mem = torch.where((torch.arange(T).unsqueeze(0) < hl.unsqueeze(1)).unsqueeze(2), mem, noise)
    if round_to is not None:
        mem = mem.to(round_to).to(torch.float32)
    return mem, hl


def make_text(Lp, V, seed=300):
    """Three ragged transcripts whose longest has Lp - 1 tokens: ids in [1, V - 2]; random ids behind every end."""
    L = Lp - 1
    g = torch.Generator().manual_seed(seed + Lp)
    lens = torch.tensor([L, L // 2, max(L - 3, 0)], dtype=torch.long)
    return torch.randint(1, V - 1, (3, max(L, 1)), generator=g), lens
