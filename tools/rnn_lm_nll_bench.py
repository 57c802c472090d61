"""Scoring sentences with the default recurrent LM (lm: seq_rnn, lstm 2 x 650, V 5 000), bf16, on two workloads: 64 ragged
sentences of 40-80 tokens, and one sentence of 3 000 tokens.

    python tools/rnn_lm_nll_bench.py [--reps 20] [--warmup 3] [--out profiles/rnn_lm_nll_bench.json]

Reports per workload, in one process on one GPU (medians with min and max, each run between its own pair of device events
with a synchronisation after it):
  * seq_nll_ms     ESPnetLanguageModel.nll: the whole call (em_rnn_lm_seq_nll, csrc/rnn_lm_seq.hip);
  * hoist_ms, chain_ms, head_ms   its three parts alone on the workspace of a whole call (em_rnn_lm_seq_nll_parts): the
                   embedding + layer 0's input product, the Lp + nlayers - 1 step launches, the vocabulary head;
  * step_route_ms  the route before: SequentialRNNLM.forward position by position through the search's step kernels, then
                   em_log_softmax_rows_f32 and a gather (what ESPnetLanguageModel.nll ran for a recurrent LM);
  * torch_ms       eager torch.nn.LSTM + Linear + log_softmax + gather on the same GPU and the same weights (`torch_dtype`:
                   bfloat16 where torch runs the LSTM in it, else float32).
The whole call, its parts and the route before are checked to give the same nll (bf16 round-off apart) before anything is
timed; eager torch's distance is reported.  The criterion of the
route's adoption: seq_nll_ms' slowest run below step_route_ms' fastest (`criterion_met`).  Weights are seeded random values.
"""
import argparse
import copy
import ctypes as C
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_common import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_lm_nll_bench: no GPU (a timing needs the device)")

    from espnet_amd import lib as L
    from espnet_amd.lm.seq_rnn_lm import SequentialRNNLM
    from espnet_amd.lm.transformer_lm import ESPnetLanguageModel

    V, NL, H = a.vocab, 2, 650
    g = torch.Generator().manual_seed(7)
    model = ESPnetLanguageModel(SequentialRNNLM(V, unit=H, nhid=H, nlayers=NL, rnn_type="lstm", compute_dtype="bfloat16"), V)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k == "lm.encoder.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * ((2.0 if "decoder" in k else 1.5) / p.shape[1] ** 0.5))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model.lm.invalidate()
    model.cuda().eval()
    lm, lib = model.lm, L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    pk = lm.packed(dev)

    tdt = torch.bfloat16
    rnn_t = copy.deepcopy(lm.rnn).to(tdt)
    try:
        with torch.no_grad():
            rnn_t(torch.zeros(1, 2, H, dtype=tdt, device="cuda"))
    except RuntimeError:
        tdt = torch.float32
        rnn_t = copy.deepcopy(lm.rnn)
    emb_t, dec_w, dec_b = lm.encoder.weight.detach().to(tdt), lm.decoder.weight.detach().to(tdt), lm.decoder.bias.detach().float()

    def workload(name, lens):
        B = lens.numel()
        text = torch.randint(1, V - 1, (B, int(lens.max())), generator=g)
        text_d, lens_d = text.cuda(), lens.cuda()
        x, t, xl, scored = model._masked_pair(text_d, lens_d)
        Lp = x.size(1)
        xi = x.to(torch.int32).contiguous()
        ti = torch.where(scored, t, torch.full_like(t, -1)).to(torch.int32).contiguous()
        li = xl.to(torch.int32).contiguous()
        need = lib.em_rnn_lm_seq_nll_workspace_bytes(pk.dtype, C.byref(pk.w), B, Lp)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.empty(B, Lp, device="cuda")

        def part(mask):
            return lambda: L.check(lib.em_rnn_lm_seq_nll_parts(pk.dtype, C.byref(pk.w), L.ptr(xi), L.ptr(ti), L.ptr(li), B, Lp,
                                                               L.ptr(out), L.ptr(ws), need, mask, L.current_stream_ptr()))

        def seq():
            return model.nll(text_d, lens_d)[0]

        def step():
            logits = torch.cat([lm(x[i:i + 64], None)[0] for i in range(0, B, 64)])
            rows = logits.reshape(B * Lp, V)
            L.check(lib.em_log_softmax_rows_f32(L.ptr(rows), B * Lp, V, L.current_stream_ptr()))
            nll = -rows.gather(1, t.reshape(-1, 1)).reshape(B, Lp)
            return torch.where(scored, nll, torch.zeros_like(nll))

        def eager():
            h, _ = rnn_t(emb_t[x])
            logp = torch.log_softmax((h @ dec_w.T).float() + dec_b, -1)
            nll = -logp.gather(2, t.unsqueeze(2)).squeeze(2)
            return torch.where(scored, nll, torch.zeros_like(nll))

        with torch.no_grad():
            n_seq, n_step, n_torch = seq(), step(), eager()
            part(7)()
            diff = dict(seq_vs_step=float((n_seq - n_step).abs().max()), seq_vs_torch=float((n_seq - n_torch).abs().max()),
                        parts_vs_seq=float((out - n_seq).abs().max()))
            # (eager torch keeps c and the gates in its own dtype: its distance is reported, not judged)
            if max(diff["seq_vs_step"], diff["parts_vs_seq"]) > 0.25 or not torch.isfinite(n_seq).all():
                raise SystemExit(f"{name}: the routes disagree: {diff}")
            few = max(3, a.reps // 5)
            res = dict(workload=f"{name}: B {B}, Lp {Lp}, {int(xl.sum())} scored tokens; lstm {NL} x {H}, V {V}, bf16",
                       mean_nll=round(float(n_seq.sum() / xl.sum()), 4), max_abs_diff=diff,
                       launches_seq=2 + (Lp + NL - 1) + 2, step_launches=Lp + NL - 1, torch_dtype=str(tdt).split(".")[1],
                       seq_nll_ms=timed(seq, a.reps, a.warmup), hoist_ms=timed(part(L.EM_RNN_SEQ_HOIST), a.reps, a.warmup),
                       chain_ms=timed(part(L.EM_RNN_SEQ_CHAIN), a.reps, a.warmup),
                       head_ms=timed(part(L.EM_RNN_SEQ_HEAD), a.reps, a.warmup), step_route_ms=timed(step, few, 1),
                       torch_ms=timed(eager, few, 1))
        res["step_over_seq"] = round(res["step_route_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["torch_over_seq"] = round(res["torch_ms"]["median"] / res["seq_nll_ms"]["median"], 2)
        res["criterion_met"] = res["seq_nll_ms"]["max"] < res["step_route_ms"]["min"]
        res["scored_tokens_per_s_seq"] = round(float(xl.sum()) / (res["seq_nll_ms"]["median"] / 1e3))
        return res

    res = dict(reps=a.reps, warmup=a.warmup, batch=workload("64 ragged sentences of 40-80 tokens", torch.randint(40, 81, (64,), generator=g)),
               long=workload("one sentence of 3 000 tokens", torch.tensor([3000])))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
