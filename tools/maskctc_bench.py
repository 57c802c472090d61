"""Mask-CTC decoding: 32 encoder memories of T = 249 frames, d 512 (10 s of audio each) through a CTC head and an MLM
decoder of 6 blocks x 512 / 2048 units / 8 heads / V 5 000, bf16, K = 10 passes.

    python tools/maskctc_bench.py [--reps 20] [--warmup 3] [--out profiles/maskctc_bench.json]

The memories are synthetic, built so that the greedy CTC pass yields 40-80 tokens per utterance of which roughly a third
fall below the threshold 0.99 (frame t of a token's run is alpha_t times the unit-norm CTC row of its label: alpha 20 gives
a probability of 1 - 1e-5, alpha 9 one of about 0.6; the achieved share is reported).  Reports, in one process on one GPU
(medians with min and max of `--reps` runs after `--warmup`, each run between device events around the enqueued region):
  * ctc_stage_ms     em_ctc_frame_top (csrc/vocab_head.hip) + em_maskctc_collapse;
  * memory_ms        em_decoder_memory: the source attention's K | V and V^T of all blocks, once per batch;
  * refine_ms        em_maskctc_refine: the K passes and fills as one enqueued chain (memory projected beforehand);
  * whole_call_ms    MaskCTCModel.decode_maskctc_device: the three above with the one read-back of the counts;
  * host_driven_ms   the same passes driven from the host: MLMDecoder.forward (this library's kernels, the (B, L, V + 1)
                     logits in memory), max / arg-max and the fill in torch with a read-back per pass;
  * torch_ms         eager torch on the same GPU: the decoder in bf16 torch ops, the fill on the device, no read-back.
The three routes are checked to agree on the tokens (bf16 near-ties apart) before anything is timed.  Every leg is reported
as measured, a losing one too.  Weights are the recipe initialisation (oracle.weights, seed 7).
"""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed  # noqa: E402

D, HEADS, FF, LAYERS = 512, 8, 2048, 6


def build(V):
    from espnet_amd.asr.ctc import CTC
    from espnet_amd.asr.decoder.mlm_decoder import MLMDecoder
    from espnet_amd.asr.maskctc_model import MaskCTCModel
    from oracle.weights import recipe_state_dict, token_list

    dec = MLMDecoder(V, D, attention_heads=HEADS, linear_units=FF, num_blocks=LAYERS, compute_dtype="bfloat16")
    model = MaskCTCModel(V, token_list(V), frontend=None, specaug=None, normalize=None, preencoder=None, encoder=None,
                         postencoder=None, decoder=dec, ctc=CTC(V, D, compute_dtype="bfloat16"), ctc_weight=0.3)
    sd = recipe_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 7, skip=())
    w = torch.randn(V, D, generator=torch.Generator().manual_seed(8))
    sd["ctc.ctc_lo.weight"] = w / w.norm(dim=1, keepdim=True)
    sd["ctc.ctc_lo.bias"] = torch.zeros(V)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd


def memories(sd, B, T, V):
    """(enc (B, T, D), the planted token counts): runs of two frames per token, blanks between and behind them."""
    g = torch.Generator().manual_seed(9)
    w = sd["ctc.ctc_lo.weight"]
    enc = torch.zeros(B, T, D)
    counts = torch.randint(40, 81, (B,), generator=g).tolist()
    for b, n in enumerate(counts):
        ids = torch.zeros(T, dtype=torch.long)
        alpha = torch.full((T,), 20.0)
        lab = torch.randint(1, V - 1, (n,), generator=g)
        unsure = torch.rand(n, generator=g) < 1.0 / 3.0
        for j in range(n):
            ids[3 * j : 3 * j + 2] = lab[j]
            if unsure[j]:
                alpha[3 * j : 3 * j + 2] = 9.0
        enc[b] = w[ids] * alpha.unsqueeze(1)
    return enc, counts


def torch_decoder(sd, bf=torch.bfloat16):
    """The MLM decoder in eager torch: bf16 matrices, f32 residual stream and norms (what the device path computes)."""
    from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table

    F = torch.nn.functional
    p = {k[len("decoder."):]: (v.cuda().to(bf) if v.dim() == 2 and "embed" not in k else v.cuda().float()) for k, v in sd.items()
         if k.startswith("decoder.")}
    pe = abs_pos_table(1024, D).cuda()

    def lin(x, pre):
        return F.linear(x.to(bf), p[pre + "weight"]).float() + p[pre + "bias"]

    def ln(x, pre):
        return F.layer_norm(x, (D,), p[pre + "weight"], p[pre + "bias"], 1e-12)

    def mha(q, k, v, ok):  # q (B, Lq, D), k / v (B, Lk, D), ok (B, 1, 1, Lk)
        B, Lq, _ = q.shape
        q, k, v = (t.to(bf).view(B, t.size(1), HEADS, D // HEADS).transpose(1, 2) for t in (q, k, v))
        return F.scaled_dot_product_attention(q, k, v, attn_mask=ok).transpose(1, 2).reshape(B, Lq, D).float()

    def memory(enc):
        return [(lin(enc, f"decoders.{l}.src_attn.linear_k."), lin(enc, f"decoders.{l}.src_attn.linear_v.")) for l in range(LAYERS)]

    def forward(mem, hlens, ys, ylens):
        B, Lp = ys.shape
        x = p["embed.0.weight"][ys.clamp(min=0)] * math.sqrt(D) + pe[:Lp]
        ok_self = (torch.arange(Lp, device=ys.device)[None] < ylens[:, None])[:, None, None, :]
        ok_src = (torch.arange(mem[0][0].size(1), device=ys.device)[None] < hlens[:, None])[:, None, None, :]
        for l in range(LAYERS):
            pre = f"decoders.{l}."
            t = ln(x, pre + "norm1.")
            x = x + lin(mha(lin(t, pre + "self_attn.linear_q."), lin(t, pre + "self_attn.linear_k."),
                            lin(t, pre + "self_attn.linear_v."), ok_self), pre + "self_attn.linear_out.")
            t = ln(x, pre + "norm2.")
            x = x + lin(mha(lin(t, pre + "src_attn.linear_q."), mem[l][0], mem[l][1], ok_src), pre + "src_attn.linear_out.")
            t = ln(x, pre + "norm3.")
            x = x + lin(torch.relu(lin(t, pre + "feed_forward.w_1.")), pre + "feed_forward.w_2.")
        return lin(ln(x, "after_norm."), "output_layer.")

    return memory, forward


def torch_fill(y, logits, M0, K, p, mask_token):
    """One pass of the fill for the whole batch on the device (score descending, position ascending)."""
    s, a = logits.max(dim=-1)
    masked = y == mask_token
    n_iter = torch.where(M0 >= K, torch.full_like(M0, K), M0).clamp(min=1)
    n = M0 // n_iter
    order = torch.argsort(torch.where(masked, s, torch.full_like(s, float("-inf"))), dim=1, descending=True, stable=True)
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(y.size(1), device=y.device).expand_as(order))
    active = (M0 > 0) & (p < n_iter)
    last = p == n_iter - 1
    take = masked & active[:, None] & (last[:, None] | (rank < n[:, None]))
    return torch.where(take, a.to(y.dtype), y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.99)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("maskctc_bench: no GPU (a timing needs the device)")
    B, T, V, K = a.utts, a.frames, a.vocab, a.iterations
    model, sd = build(V)
    dec, mask_token = model.decoder, model.mask_token
    enc_host, planted = memories(sd, B, T, V)
    with torch.no_grad():
        enc = enc_host.cuda()
        olens = torch.full((B,), T, dtype=torch.int32, device="cuda")
        y_dev, ylens, tokens, conf = model._decode_maskctc(enc, olens, K, a.threshold)
        y_in = torch.where(conf < a.threshold, torch.full_like(tokens, mask_token), tokens)
        y_in = torch.where(tokens < 0, tokens, y_in).contiguous()
        nmask = (y_in == mask_token).sum(dim=1).to(torch.int32)
        Lp = int(y_in.shape[1])
        share = float(nmask.sum()) / float(ylens.sum())
        if ylens.cpu().tolist() != planted:
            raise SystemExit(f"the CTC pass found {ylens.cpu().tolist()} tokens, planted {planted}")
        pk = dec.packed(enc.device, Lp)
        ws = torch.empty(dec.refine_workspace_bytes(enc.device, B, Lp), dtype=torch.uint8, device="cuda")

        def ctc_stage():
            ids, prob = model.ctc.frame_top_device(enc)
            return model.collapse_device(ids, prob, olens, a.threshold)

        def memory():
            return dec._memory_of(enc, pk)

        def refine():
            y = y_in.clone()
            dec.refine_device(enc, olens, y, ylens, nmask, K, ws=ws, mem=mem_dev)
            return y

        def whole():
            return model._decode_maskctc(enc, olens, K, a.threshold)[0]

        def host_driven():
            y = y_in.clone()
            M0 = nmask.to(torch.long)
            for p in range(K):
                logits, _ = dec(enc, olens, y.clamp(min=0), ylens)
                y = torch_fill(y, logits, M0, K, p, mask_token)
                if not bool((y == mask_token).any().cpu()):  # the read-back of a host-driven loop
                    break
            return y

        t_memory, t_forward = torch_decoder(sd)
        hl, yl = olens.long(), ylens.long()

        def torch_route():
            y = y_in.clone()
            M0 = nmask.to(torch.long)
            mem = t_memory(enc)
            for p in range(K):
                y = torch_fill(y, t_forward(mem, hl, y, yl), M0, K, p, mask_token)
            return y

        mem_dev = memory()
        r_new, r_whole, r_host, r_torch = refine(), whole(), host_driven(), torch_route()
        valid = (tokens >= 0)
        agree = dict(refine_vs_whole=float((r_new == r_whole)[valid].float().mean()),
                     refine_vs_host_driven=float((r_new == r_host)[valid].float().mean()),
                     refine_vs_torch=float((r_new == r_torch)[valid].float().mean()))
        if agree["refine_vs_whole"] != 1.0 or min(agree.values()) < 0.9:
            raise SystemExit(f"the routes disagree: {agree}")
        res = dict(workload=f"{B} memories of T {T}, d {D}; MLM decoder {LAYERS} x {D} / {FF} / {HEADS} heads / V {V}, bf16; token "
                            f"sequences of {int(ylens.min())}-{int(ylens.max())} (Lp {Lp}), {int(nmask.sum())} of {int(ylens.sum())} "
                            f"tokens masked at p_thres {a.threshold}; K = {K}",
                   masked_share=round(share, 4), token_agreement=agree, reps=a.reps, warmup=a.warmup)
        res["ctc_stage_ms"] = timed(ctc_stage, a.reps, a.warmup)
        res["memory_ms"] = timed(memory, a.reps, a.warmup)
        res["refine_ms"] = timed(refine, a.reps, a.warmup)
        res["whole_call_ms"] = timed(whole, a.reps, a.warmup)
        res["host_driven_ms"] = timed(host_driven, a.reps, a.warmup)
        res["torch_ms"] = timed(torch_route, a.reps, a.warmup)
        res["host_driven_over_refine"] = round(res["host_driven_ms"]["median"] / res["refine_ms"]["median"], 2)
        res["torch_over_refine"] = round(res["torch_ms"]["median"] / (res["refine_ms"]["median"] + res["memory_ms"]["median"]), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
