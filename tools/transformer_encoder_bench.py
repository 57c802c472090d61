#!/usr/bin/env python3
"""Time the Transformer encoder (encoder: transformer) in bf16: the device path (TransformerEncoder.forward_device ->
em_transformer_encode) against the same forward as eager torch on the same GPU (the f32 restatement of
tests/transformer_ref.py in bf16, with scaled_dot_product_attention), both from the same features, for 32 x 10 s at
256 d / 12 blocks / 2048 units and 512 d / 18 blocks / 2048 units.  Prints one JSON line per shape: ms per batch,
audio-s/s, and the relative (Frobenius-norm) difference of the two outputs.

    python tools/transformer_encoder_bench.py [--batch 32] [--seconds 10] [--iters 20] [--warmup 5] [--only 256|512]
                                              [--no-eager]"""
import argparse
import json
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from espnet_amd.asr.decoder.transformer_decoder import abs_pos_table  # noqa: E402
from espnet_amd.nets_utils import conv2d_subsampled_lengths  # noqa: E402
from espnet_amd.tasks.asr import ASRTask  # noqa: E402
from oracle.weights import recipe_tensor  # noqa: E402

SHAPES = {256: dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12),
          512: dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=18)}


def eager_encoder(sd, feats, olens, heads, blocks):
    """The restatement's forward in the activation dtype of `sd`, attention by scaled_dot_product_attention."""
    dt = sd["encoder.embed.out.weight"].dtype
    x = feats.to(dt).unsqueeze(1)
    x = F.relu(F.conv2d(x, sd["encoder.embed.conv.0.weight"], sd["encoder.embed.conv.0.bias"], stride=2))
    x = F.relu(F.conv2d(x, sd["encoder.embed.conv.2.weight"], sd["encoder.embed.conv.2.bias"], stride=2))
    b, c, t, f = x.shape
    x = F.linear(x.transpose(1, 2).reshape(b, t, c * f), sd["encoder.embed.out.weight"], sd["encoder.embed.out.bias"])
    d = x.size(-1)
    x = x * math.sqrt(d) + sd["_pe"][:t].to(dt)
    mask = (torch.arange(t, device=x.device)[None, :] < olens[:, None])[:, None, None, :]
    dk = d // heads

    def ln(v, p):
        return F.layer_norm(v, (d,), sd[p + "weight"], sd[p + "bias"], 1e-12)

    def lin(v, p):
        return F.linear(v, sd[p + "weight"], sd[p + "bias"])

    for i in range(blocks):
        p = f"encoder.encoders.{i}."
        h = ln(x, p + "norm1.")
        q, k, v = (lin(h, p + f"self_attn.linear_{n}.").view(b, t, heads, dk).transpose(1, 2) for n in "qkv")
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(b, t, d)
        x = x + lin(a, p + "self_attn.linear_out.")
        x = x + lin(F.relu(lin(ln(x, p + "norm2."), p + "feed_forward.w_1.")), p + "feed_forward.w_2.")
    return ln(x, "encoder.after_norm.")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", type=int, choices=sorted(SHAPES), default=None)
    ap.add_argument("--no-eager", action="store_true", help="time the device path only (a kernel trace of it alone)")
    args = ap.parse_args()
    B, n = args.batch, int(16000 * args.seconds)
    for d, conf in SHAPES.items():
        if args.only and d != args.only:
            continue
        cfg = dict(token_list=["<blank>", "<unk>"] + [f"t{i}" for i in range(5000 - 3)] + ["<sos/eos>"],
                   frontend="default", frontend_conf=dict(n_fft=512, win_length=400, hop_length=160),
                   normalize="utterance_mvn", encoder="transformer", encoder_conf=dict(conf, input_layer="conv2d"),
                   decoder=None, compute_dtype="bfloat16")
        model = ASRTask.build_model(cfg)
        sd = {k: (v if k == "frontend.logmel.melmat" else recipe_tensor(k, v.shape, 1)) for k, v in model.state_dict().items()}
        model.load_state_dict(sd)
        model = model.cuda().eval()
        enc = model.encoder
        g = torch.Generator().manual_seed(0)
        speech = (0.1 * torch.randn(B, n, generator=g)).cuda()
        lens = [n] * B
        st = model.encode_device(speech, lens)  # (features for both legs: frontend + MVN applied)
        feats, flens = st.feats, st.flens
        if model.normalize is not None:  # the eager leg needs normalised features; the device leg folds MVN into conv1
            m = feats.sum(1, keepdim=True) / torch.tensor(flens, device=feats.device, dtype=torch.float32).view(-1, 1, 1)
            nfeats = feats - m
        flens_dev = torch.tensor(flens, dtype=torch.int32, device="cuda")
        partial = model.normalize.partial_sums(feats, flens_dev) if model.normalize is not None else None
        esd = {k: v.detach().to(torch.bfloat16).cuda() for k, v in enc.state_dict().items()}
        esd = {"encoder." + k: v for k, v in esd.items()}
        esd["_pe"] = abs_pos_table(4096, d).cuda()
        olens = torch.tensor(conv2d_subsampled_lengths(flens, feats.size(1), "conv2d"), device="cuda")
        with torch.no_grad():
            dev_out = enc.forward_device(feats, flens, flens_dev, partial)[0]
            t_dev = timed(lambda: enc.forward_device(feats, flens, flens_dev, partial), args.iters, args.warmup)
            rel, t_eager = float("nan"), float("nan")
            if not args.no_eager:
                eager_out = eager_encoder(esd, nfeats, olens, conf["attention_heads"], conf["num_blocks"]).float()
                rel = ((dev_out - eager_out).norm() / eager_out.norm()).item()
                t_eager = timed(lambda: eager_encoder(esd, nfeats, olens, conf["attention_heads"], conf["num_blocks"]),
                                args.iters, args.warmup)
        audio = B * args.seconds
        res = dict(shape=f"{d}d_{conf['num_blocks']}blocks_{conf['linear_units']}units", batch=B, seconds=args.seconds,
                   T=int(dev_out.size(1)), device_ms=round(t_dev, 3), device_audio_s_per_s=round(audio / (t_dev / 1e3), 1))
        if not args.no_eager:
            res.update(eager_torch_ms=round(t_eager, 3), eager_audio_s_per_s=round(audio / (t_eager / 1e3), 1),
                       speedup=round(t_eager / t_dev, 2), rel_diff_vs_eager=round(rel, 5))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
