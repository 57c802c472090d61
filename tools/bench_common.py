"""What several of the bench tools share: the timers whose bodies were the same in every tool that had them, and the model
and the candidates of the transducer benches.  A tool whose timer differs keeps its own."""
import statistics
import time

import torch


def summary(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def timed(fn, reps, warmup):
    """Each of `reps` runs after `warmup` between its own pair of device events, a synchronisation after it."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def timed_host(fn, iters, warmup):
    """The mean of `iters` runs enqueued back to back, host clock, one synchronisation behind them."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def transducer_small(vocab, blank_bias=1.0):
    """Conformer-small + LSTM 1 x 512 prediction network + joint 640 + V `vocab`, bf16, on the GPU: the recipe initialisation
    (oracle.weights, seed 7) with the blank's embedding zeroed and its bias raised.  Returns (model, its state dict)."""
    from espnet_amd.tasks.asr import ASRTask
    from oracle.weights import recipe_state_dict, token_list

    cfg = dict(token_list=token_list(vocab), frontend="default", frontend_conf=dict(n_fft=512, hop_length=160, win_length=400),
               normalize="utterance_mvn", normalize_conf={}, encoder="conformer",
               encoder_conf=dict(output_size=256, attention_heads=4, linear_units=1024, num_blocks=12, macaron_style=True,
                                 cnn_module_kernel=31),
               decoder="transducer", decoder_conf=dict(rnn_type="lstm", num_layers=1, hidden_size=512),
               joint_net_conf=dict(joint_space_size=640), model_conf=dict(ctc_weight=0.0), compute_dtype="bfloat16")
    model = ASRTask.build_model(cfg)
    sd = model.state_dict()
    new = recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 7)
    new["frontend.logmel.melmat"] = sd["frontend.logmel.melmat"].clone()
    new["decoder.embed.weight"][0] = 0.0
    new["joint_network.lin_out.bias"][0] += blank_bias
    model.load_state_dict(new, strict=True)
    model.cuda().eval()
    return model, new


def transducer_candidates(N, vocab, per_utt):
    """N candidates of 40-80 tokens, `per_utt` per utterance (seed 7): (the generator, ylens (N,), ys (N, Lmax), mem_of)."""
    g = torch.Generator().manual_seed(7)
    ylens = torch.randint(40, 81, (N,), generator=g)
    ys = torch.randint(1, vocab - 1, (N, int(ylens.max())), generator=g)
    return g, ylens, ys, torch.arange(N) // per_utt
