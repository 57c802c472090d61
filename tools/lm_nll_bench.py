"""Scoring sentences with the LibriSpeech-recipe TransformerLM (16 x 512, 8 heads, 2048 units, embed 128, V 5 000), bf16:
64 ragged sentences of 40-80 tokens.

    python tools/lm_nll_bench.py [--batch 64] [--reps 20] [--warmup 3] [--out FILE.json]

Reports, in one process on one GPU (medians with min and max of `--reps` runs after `--warmup`, each run timed with device
events around the whole call and a synchronisation after it):
  * seq_nll_ms    ESPnetLanguageModel.nll: all B * Lp rows in one enqueue (em_lm_seq_nll, csrc/lm_seq.hip;
                  head: csrc/vocab_head.hip);
  * step_route_ms TransformerLM.forward position by position through the search's step kernels, then log-softmax and a
                  gather (the only whole-sequence route before em_lm_seq_nll);
  * torch_ms      an eager-torch restatement on the same GPU and the same bf16 weights (batched matmuls, masked softmax).
The three are checked to give the same nll (bf16 round-off apart) before anything is timed; `launches_seq` is counted
from the chain (3 + 7 per layer + 2).  Weights are seeded random values (tests/lm_nll_cases.py scales).
"""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_nll_bench: no GPU (a timing needs the device)")

    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel, TransformerLM, build_nll_batch

    V, B, d, H, NL = a.vocab, a.batch, 512, 8, a.layers
    g = torch.Generator().manual_seed(7)
    lm = TransformerLM(V, pos_enc=None, embed_unit=128, att_unit=d, head=H, unit=2048, layer=NL, compute_dtype="bfloat16")
    model = ESPnetLanguageModel(lm, V)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.dim() == 2 and k != "lm.embed.weight":
                s = 2.0 if ("linear_q" in k or "linear_k" in k or k == "lm.decoder.weight") else 1.0
                p.copy_(torch.randn(p.shape, generator=g) * (s / p.shape[1] ** 0.5))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g))
            elif not k.endswith("weight"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model.lm.invalidate()
    model.cuda().eval()
    lens = torch.randint(40, 81, (B,), generator=g)
    text = torch.randint(1, V - 1, (B, int(lens.max())), generator=g)
    text_d, lens_d = text.cuda(), lens.cuda()
    x, t, xl = build_nll_batch(text_d, lens_d, V - 1, V - 1)
    scored = torch.arange(x.size(1), device="cuda").unsqueeze(0) < xl.unsqueeze(1)
    x = torch.where(scored, x, torch.zeros_like(x))
    Lp = x.size(1)

    def seq():
        return model.nll(text_d, lens_d)[0]

    def step():
        logits, _ = model.lm(x, None)
        nll = -torch.log_softmax(logits, -1).gather(2, t.unsqueeze(2)).squeeze(2)
        return torch.where(scored, nll, torch.zeros_like(nll))

    bf = torch.bfloat16
    sd = {k: (v.detach().to(bf) if v.dim() == 2 else v.detach().float()) for k, v in model.state_dict().items()}
    causal = torch.tril(torch.ones(Lp, Lp, dtype=torch.bool, device="cuda"))

    def lin(h, pre):
        return (h.to(bf) @ sd[pre + "weight"].T).float() + sd[pre + "bias"]

    def ln(h, pre, eps):
        return torch.nn.functional.layer_norm(h, (h.size(-1),), sd[pre + "weight"], sd[pre + "bias"], eps)

    def eager():
        h = torch.relu(ln(lin(sd["lm.embed.weight"][x], "lm.encoder.embed.0."), "lm.encoder.embed.1.", 1e-5))
        ok = (causal.unsqueeze(0) & (x != 0).unsqueeze(1)).unsqueeze(1)
        for l in range(NL):
            pre = f"lm.encoder.encoders.{l}."
            n1 = ln(h, pre + "norm1.", 1e-12)
            q, k, v = (lin(n1, pre + f"self_attn.linear_{c}.").to(bf).view(B, Lp, H, d // H).transpose(1, 2) for c in "qkv")
            sc = (q @ k.transpose(-2, -1)).float() / math.sqrt(d // H)
            att = torch.softmax(sc.masked_fill(~ok, torch.finfo(torch.float32).min), -1).masked_fill(~ok, 0.0)
            ctx = (att.to(bf) @ v).transpose(1, 2).reshape(B, Lp, d)
            h = h + lin(ctx, pre + "self_attn.linear_out.")
            n2 = ln(h, pre + "norm2.", 1e-12)
            h = h + lin(torch.relu(lin(n2, pre + "feed_forward.w_1.")), pre + "feed_forward.w_2.")
        logits = lin(ln(h, "lm.encoder.after_norm.", 1e-12), "lm.decoder.")
        nll = -torch.log_softmax(logits, -1).gather(2, t.unsqueeze(2)).squeeze(2)
        return torch.where(scored, nll, torch.zeros_like(nll))

    with torch.no_grad():
        n_seq, n_step, n_torch = seq(), step(), eager()
        diff = dict(seq_vs_step=float((n_seq - n_step).abs().max()), seq_vs_torch=float((n_seq - n_torch).abs().max()))
        if max(diff.values()) > 0.25 or not torch.isfinite(n_seq).all():
            raise SystemExit(f"the routes disagree: {diff}")
        res = dict(workload=f"{B} sentences of 40-80 tokens (Lp {Lp}, {int(xl.sum())} scored tokens), TransformerLM {NL} x {d}, "
                            f"{H} heads, 2048 units, embed 128, V {V}, bf16",
                   mean_nll=round(float(n_seq.sum() / xl.sum()), 4), max_abs_diff=diff, launches_seq=3 + 7 * NL + 2,
                   launches_step_route=f"~{Lp * (3 + 6 * NL + 2)}", reps=a.reps, warmup=a.warmup)
        res["seq_nll_ms"] = timed(seq, a.reps, a.warmup)
        res["step_route_ms"] = timed(step, max(3, a.reps // 5), 1)
        res["torch_ms"] = timed(eager, a.reps, a.warmup)
        res["step_over_seq"] = round(res["step_route_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["step_min_over_seq_max"] = round(res["step_route_ms"]["min"] / res["seq_nll_ms"]["max"], 2)
        res["torch_over_seq"] = round(res["torch_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["scored_tokens_per_s_seq"] = round(float(xl.sum()) / (res["seq_nll_ms"]["median"] / 1e3))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
