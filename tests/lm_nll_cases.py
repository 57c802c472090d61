"""The models, sentences and error bounds that tests/test_cpu_lm_nll.py and tests/test_gpu_lm_nll.py share: the CPU test
shows that the defects a bound is meant to catch move some scored nll by more than four times that bound, the GPU tests
hold the device to the bounds.

Bounds follow the repository's rule (tests/test_gpu_transducer.py E_DEC / E_LOGP): measured against the float64
restatement (tests/lm_seq_ref.py) on the same rounded weights, constant = 4 x the largest value of the first run, which is
kept in profiles/lm_nll_first_run.txt.
"""
import torch

# (vocabulary, heads, pos_enc, weight seed).  2 layers, att_unit 128 (d_k 64 with 2 heads, 32 with 4), unit 128, embed_unit 64;
# V = 1027 spans three 512-column slices of the vocabulary head with a partial last tile.
MODELS = {"h2": (300, 2, None, 11), "h2pe": (300, 2, "sinusoidal", 12), "h4": (1027, 4, None, 13),
          "h4pe": (1027, 4, "sinusoidal", 14)}
LAYERS, ATT, UNIT, EMBED = 2, 128, 128, 64
WIDTHS = (1, 2, 63, 64, 65, 130)  # Lp = longest sentence + 1: one position, a partial / full / just-over 32-key and 16-query tile, many tiles
TEXT_SEED = 100

# Largest errors of the first run (profiles/lm_nll_first_run.txt) x 4:
#   |nll - float64 restatement| per scored token of the tiny models: f32 7.473e-6, bf16 6.438e-2;
#   per row of the stand-alone head: 2.391e-6 / 8.999e-3; its rows with one logit 40 above the rest (nll up to 41): 1.455e-5 / 1.691e-2;
#   |ctx - restatement| of the stand-alone attention (values of order 1): 2.529e-6 / 8.917e-3.
# That run scored sentences with a single id 0 per batch; a missing id-0 mask then moved no nll by more than 0.38, less
# than four times the bf16 bound, so make_text now zeroes every fourth token of two sentences (1.5 and more).  The bounds
# were not changed for it.
E_NLL = {"float32": 3.0e-5, "bfloat16": 2.6e-1}
E_HEAD = {"float32": 9.6e-6, "bfloat16": 3.6e-2}
E_HEAD_PEAKED = {"float32": 5.9e-5, "bfloat16": 6.8e-2}
E_ATT = {"float32": 1.1e-5, "bfloat16": 3.6e-2}


def build_model(name, compute_dtype="float32"):
    """ESPnetLanguageModel(TransformerLM) `name` on the CPU with seeded weights.  Scales: matrices N(0, s^2 / fan_in) with
    s = 2 for the query / key projections (attention that prefers some keys), 2 for the vocabulary head (logits a few
    units apart) and 1 elsewhere; the input LayerNorm's gain around 0.1, so that x * sqrt(d) and pe[j] are of one size;
    other gains 1 +- 0.1, biases 0.1."""
    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel, TransformerLM

    V, heads, pos_enc, seed = MODELS[name]
    lm = TransformerLM(V, pos_enc=pos_enc, embed_unit=EMBED, att_unit=ATT, head=heads, unit=UNIT, layer=LAYERS,
                       compute_dtype=compute_dtype)
    model = ESPnetLanguageModel(lm, V)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.dim() == 2:
                s = 2.0 if ("linear_q" in k or "linear_k" in k or k == "lm.decoder.weight") else 1.0
                if k == "lm.embed.weight":
                    p.copy_(torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * (s / p.shape[1] ** 0.5))
            elif k.endswith("weight"):  # LayerNorm gains
                base = 0.1 if k == "lm.encoder.embed.1.weight" else 1.0
                p.copy_(base * (1.0 + 0.1 * torch.randn(p.shape, generator=g)))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model.lm.invalidate()
    return model.eval()


def make_text(Lp, V, seed=TEXT_SEED):
    """Three ragged sentences whose longest has Lp - 1 tokens: ids in [1, V - 2] with an id 0 in the middle of the first
    sentence (three tokens or more); from nine tokens on, one in the third sentence too and every fourth token of both
    (a missing id-0 mask then moves some nll by 1.5 and more: with a single id 0 per batch it was 0.38, too close to
    the bf16 bound).  The second sentence has none.  Random ids (never scored, never a key) behind every end."""
    L = Lp - 1
    g = torch.Generator().manual_seed(seed + Lp)
    lens = torch.tensor([L, L // 2, max(L - 3, 0)], dtype=torch.long)
    text = torch.randint(1, V - 1, (3, L), generator=g)
    if L >= 3:
        text[0, L // 2] = 0
    if L >= 9:
        text[2, L // 3] = 0
        text[0, 3::4] = 0
        text[2, 3::4] = 0
    return text, lens
