#!/usr/bin/env python3
"""Time the streaming Transformer encoder (encoder: contextual_block_transformer) against the contextual-block Conformer
encoder of the same sizes (12 x 256 d, 4 heads, 2048 units, block 40 / hop 16 / look-ahead 16, bf16), in one process,
alternating runs: one stream fed 640 ms chunks (`forward_infer`, the steady call of one block) and a 32-stream tick
(`forward_infer_batch`), each as a replayed hipGraph of the steady call and eagerly.  Also the new encoder's per-operator
sequence (ESPNET_AMD_STREAM_NO_FUSED=1) and its two fused forms (ESPNET_AMD_STREAM_TF_MERGE=0 / 1).  Prints one JSON line per
(encoder, variant, streams): ms per call (median of `--rounds` rounds of `--iters` calls), and the launches per layer the
plan announces; the launch count that counts is the one of a kernel trace:

    rocprofv3 --kernel-trace --stats -- python tools/stream_transformer_bench.py --trace-one transformer

runs 10 steady calls of one stream of that encoder and nothing else.

    python tools/stream_transformer_bench.py [--streams 1,32] [--iters 200] [--rounds 5] [--warmup 20] [--eager]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed_host as timed  # noqa: E402
from espnet_amd import lib as L  # noqa: E402
from espnet_amd.asr.encoder.contextual_block_conformer_encoder import ContextualBlockConformerEncoder  # noqa: E402
from espnet_amd.asr.encoder.contextual_block_transformer_encoder import ContextualBlockTransformerEncoder  # noqa: E402

SIZES = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, block_size=40, hop_size=16, look_ahead=16)
CHUNK = 64  # 640 ms of 10 ms frames -> 16 encoder frames: one block per call


def seeded(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.1))
    return m.cuda().eval()


def encoders():
    tf = seeded(ContextualBlockTransformerEncoder(80, compute_dtype="bfloat16", **SIZES), 1)
    cf = seeded(ContextualBlockConformerEncoder(80, compute_dtype="bfloat16", macaron_style=True, cnn_module_kernel=15,
                                                **SIZES), 2)
    return {"transformer": tf, "conformer": cf}


def steady_state(enc, S):
    """Feed chunks until the call's shapes repeat; returns the state in front of a steady call."""
    g = torch.Generator().manual_seed(7)
    state, sig = None, None
    for k in range(12):
        x = torch.randn(S, CHUNK, 80, generator=g).cuda()
        if S == 1:
            _, _, state = enc.forward_infer(x, torch.tensor([CHUNK]), state, False)
        else:
            _, _, state = enc.forward_infer_batch(x, state, False)
        s = (tuple(state["buffer_before_downsampling"].shape), tuple(state["buffer_after_downsampling"].shape),
             state["past_encoder_ctx"] is not None)
        if s == sig and k >= 4:
            return state
        sig = s
    raise RuntimeError("no steady state")


def make_call(enc, S, graph):
    state = steady_state(enc, S)
    x = torch.randn(S, CHUNK, 80, generator=torch.Generator().manual_seed(9)).cuda()
    ilens = torch.tensor([CHUNK])

    def call():  # (the same state every time: what is timed is the call, not the stream's progress)
        if S == 1:
            return enc.forward_infer(x, ilens, dict(state), False)[0]
        return enc.forward_infer_batch(x, dict(state), False)[0]

    if not graph:
        return call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return g.replay


def set_env(env):
    for k in ("ESPNET_AMD_STREAM_NO_FUSED", "ESPNET_AMD_STREAM_TF_MERGE"):
        os.environ.pop(k, None)
    os.environ.update(env)
    L.load().em_dev_switches_reload()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,32")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--eager", action="store_true", help="also time the calls without a hipGraph")
    ap.add_argument("--trace-one", choices=["transformer", "conformer"], help="10 steady eager calls of one stream, for a kernel trace")
    a = ap.parse_args()
    encs = encoders()
    if a.trace_one:
        call = make_call(encs[a.trace_one], 1, False)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        return
    variants = [("conformer", "fused", {}), ("transformer", "fused", {}),
                ("transformer", "fused, two launches per layer", {"ESPNET_AMD_STREAM_TF_MERGE": "0"}),
                ("transformer", "fused, layer seam merged", {"ESPNET_AMD_STREAM_TF_MERGE": "1"}),
                ("transformer", "per-operator", {"ESPNET_AMD_STREAM_NO_FUSED": "1"}),
                ("conformer", "per-operator", {"ESPNET_AMD_STREAM_NO_FUSED": "1"})]
    for S in [int(s) for s in a.streams.split(",")]:
        for graph in ([True, False] if a.eager else [True]):
            calls = []
            for name, tag, env in variants:
                set_env(env)
                enc = encs[name]
                plan = enc.plan(S, 1, True) if name == "transformer" else None
                calls.append((name, tag, env, plan, make_call(enc, S, graph)))  # (a graph keeps the launches it was captured with)
            ms = {i: [] for i in range(len(calls))}
            for _ in range(a.rounds):  # alternating: every variant once per round
                for i, (name, tag, env, plan, fn) in enumerate(calls):
                    set_env(env)
                    ms[i].append(timed(fn, a.iters, a.warmup))
            for i, (name, tag, env, plan, fn) in enumerate(calls):
                rec = dict(encoder=name, variant=tag, streams=S, hipgraph=graph, ms_per_call=round(statistics.median(ms[i]), 4),
                           ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4), rounds=a.rounds, iters=a.iters)
                if plan is not None:
                    rec["plan"] = plan
                    rec["launches_per_layer"] = {0: 6, 1: 3, 2: 2, 3: "1 (+1 per call)"}[plan]
                print(json.dumps(rec), flush=True)
    set_env({})


if __name__ == "__main__":
    main()
