"""Scoring transcripts with the attention decoder of the Conformer-large recipe (6 x 512, 8 heads, 2048 units, V 5 000),
bf16: 64 ragged transcripts of 40-80 tokens against 64 encoder memories of T = 249 frames (10 s of audio), ragged too.

    python tools/dec_nll_bench.py [--batch 64] [--reps 20] [--warmup 3] [--out profiles/dec_nll_bench.json]

Reports, in one process on one GPU (medians with min and max of `--reps` runs after `--warmup`, each run timed with device
events around the whole call and a synchronisation after it):
  * seq_nll_ms    ESPnetASRModel.nll: memory projection + all B * Lp rows in one enqueue (em_dec_seq_nll, csrc/dec_seq.hip;
                  head: csrc/vocab_head.hip);
  * step_route_ms TransformerDecoder.forward position by position through the label step's kernels, then log-softmax, a
                  gather and the sum (the only whole-sequence route before em_dec_seq_nll);
  * torch_ms      an eager-torch restatement on the same GPU and the same bf16 weights (batched matmuls, masked softmax).
The three are checked to give the same nll (bf16 round-off apart) before anything is timed; `launches_seq` is counted from
the chain (2 per layer for the memory, 1 + 11 per layer + 2).  Weights are the recipe's seeded values with the scales of
tests/dec_seq_cases.py.
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
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dec_nll_bench: no GPU (a timing needs the device)")

    from espnet_amd.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet_amd.asr.espnet_model import ESPnetASRModel, build_dec_nll_batch
    from oracle.weights import recipe_state_dict, token_list

    V, B, T, d, H, FF, NL = a.vocab, a.batch, a.frames, 512, 8, 2048, 6
    dec = TransformerDecoder(V, d, attention_heads=H, linear_units=FF, num_blocks=NL, compute_dtype="bfloat16")
    model = ESPnetASRModel(V, token_list(V), frontend=None, specaug=None, normalize=None, preencoder=None, encoder=None,
                           postencoder=None, decoder=dec, ctc=None, ctc_weight=0.0)
    sd = recipe_state_dict({"decoder." + k: tuple(v.shape) for k, v in dec.state_dict().items()}, 5, skip=())
    for k in sd:
        if k.endswith("linear_q.weight") or k.endswith("linear_k.weight"):
            sd[k] = sd[k] * 4.0
        elif k.endswith("linear_v.weight") or k.endswith("linear_out.weight"):
            sd[k] = sd[k] * 2.0
    sd["decoder.output_layer.weight"] = sd["decoder.output_layer.weight"] * 3.0
    sd["decoder.embed.0.weight"] = sd["decoder.embed.0.weight"] * 0.1
    model.load_state_dict(sd, strict=True)
    model.cuda().eval()
    sos = eos = V - 1

    g = torch.Generator().manual_seed(7)
    lens = torch.randint(40, 81, (B,), generator=g)
    text = torch.randint(1, V - 1, (B, int(lens.max())), generator=g)
    hlens = torch.randint(T // 2, T + 1, (B,), generator=g)
    hlens[0] = T
    bf = torch.bfloat16
    mem = torch.randn(B, T, d, generator=g).to(bf).float().cuda()
    text_d, lens_d, hlens_d = text.cuda(), lens.cuda(), hlens.cuda()
    x, keymask, target = build_dec_nll_batch(text_d, lens_d, sos, eos, V)
    x, scored, tgt = x.long(), target >= 0, target.long().clamp(min=0)
    Lp = x.size(1)
    in_lens = lens_d + 1

    def seq():
        return model.nll(mem, hlens_d, text_d, lens_d)

    def step():
        logits, _ = dec(mem, hlens_d, x, in_lens)
        nll = -torch.log_softmax(logits, -1).gather(2, tgt.unsqueeze(2)).squeeze(2)
        return torch.where(scored, nll, torch.zeros_like(nll)).sum(1)

    w = {k: (v.detach().to(bf) if v.dim() == 2 and k != "decoder.embed.0.weight" else v.detach().float()).cuda()
         for k, v in model.state_dict().items()}
    pe = torch.zeros(Lp, d)
    position = torch.arange(0, Lp, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2], pe[:, 1::2] = torch.sin(position * div_term), torch.cos(position * div_term)
    pe = pe.cuda()
    causal = torch.tril(torch.ones(Lp, Lp, dtype=torch.bool, device="cuda"))
    self_ok = (causal.unsqueeze(0) & keymask.bool().unsqueeze(1)).unsqueeze(1)
    src_ok = (torch.arange(T, device="cuda").unsqueeze(0) < hlens_d.unsqueeze(1)).view(B, 1, 1, T)

    def lin(h, pre):
        return (h.to(bf) @ w[pre + "weight"].T).float() + w[pre + "bias"]

    def ln(h, pre):
        return torch.nn.functional.layer_norm(h, (h.size(-1),), w[pre + "weight"], w[pre + "bias"], 1e-12)

    def heads(t):
        return t.to(bf).view(B, t.size(1), H, d // H).transpose(1, 2)

    def mha(q, k, v, ok):
        sc = (heads(q) @ heads(k).transpose(-2, -1)).float() / math.sqrt(d // H)
        att = torch.softmax(sc.masked_fill(~ok, torch.finfo(torch.float32).min), -1).masked_fill(~ok, 0.0)
        return (att.to(bf) @ heads(v)).transpose(1, 2).reshape(B, q.size(1), d)

    def eager():
        h = w["decoder.embed.0.weight"][x] * math.sqrt(d) + pe
        for l in range(NL):
            pre = f"decoder.decoders.{l}."
            n1 = ln(h, pre + "norm1.")
            ctx = mha(*(lin(n1, pre + f"self_attn.linear_{c}.") for c in "qkv"), self_ok)
            h = h + lin(ctx, pre + "self_attn.linear_out.")
            n2 = ln(h, pre + "norm2.")
            ctx = mha(lin(n2, pre + "src_attn.linear_q."), lin(mem, pre + "src_attn.linear_k."),
                      lin(mem, pre + "src_attn.linear_v."), src_ok)
            h = h + lin(ctx, pre + "src_attn.linear_out.")
            n3 = ln(h, pre + "norm3.")
            h = h + lin(torch.relu(lin(n3, pre + "feed_forward.w_1.")), pre + "feed_forward.w_2.")
        logits = lin(ln(h, "decoder.after_norm."), "decoder.output_layer.")
        nll = -torch.log_softmax(logits, -1).gather(2, tgt.unsqueeze(2)).squeeze(2)
        return torch.where(scored, nll, torch.zeros_like(nll)).sum(1)

    with torch.no_grad():
        n_seq, n_step, n_torch = seq(), step(), eager()
        ntok = in_lens.float()
        diff = dict(seq_vs_step=float(((n_seq - n_step).abs() / ntok).max()),
                    seq_vs_torch=float(((n_seq - n_torch).abs() / ntok).max()))
        if max(diff.values()) > 0.25 or not torch.isfinite(n_seq).all():  # (per scored token of a transcript)
            raise SystemExit(f"the routes disagree: {diff}")
        res = dict(workload=f"{B} transcripts of 40-80 tokens (Lp {Lp}, {int(in_lens.sum())} scored tokens) against {B} memories "
                            f"of T {T} ({int(hlens.min())}-{int(hlens.max())} valid frames), TransformerDecoder {NL} x {d}, {H} "
                            f"heads, {FF} units, V {V}, bf16",
                   mean_nll=round(float(n_seq.sum() / in_lens.sum()), 4), max_abs_diff_per_token=diff,
                   launches_seq=2 * NL + 1 + 11 * NL + 2, launches_step_route=f"~{Lp * (1 + 8 * NL + 1)}", reps=a.reps,
                   warmup=a.warmup)
        res["seq_nll_ms"] = timed(seq, a.reps, a.warmup)
        res["step_route_ms"] = timed(step, a.reps, a.warmup)
        res["torch_ms"] = timed(eager, a.reps, a.warmup)
        res["step_over_seq"] = round(res["step_route_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["step_min_over_seq_max"] = round(res["step_route_ms"]["min"] / res["seq_nll_ms"]["max"], 2)
        res["torch_over_seq"] = round(res["torch_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["scored_tokens_per_s_seq"] = round(float(in_lens.sum()) / (res["seq_nll_ms"]["median"] / 1e3))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    if res["seq_nll_ms"]["max"] >= res["step_route_ms"]["min"]:
        raise SystemExit("dec_nll_bench: the sequence route's slowest run is not below the step route's fastest")


if __name__ == "__main__":
    main()
