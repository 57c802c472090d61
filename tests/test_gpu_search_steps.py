"""Step-level checks of the device beam search's pruning kernels (espnet_amd/csrc/search.hip) against the float64
restatement of ONE label step, tests/search_step_ref.py (pinned to the oracle's whole search on the CPU by
tests/test_cpu_search_step_ref.py).

The search is walked one label step at a time through `BatchBeamSearch.step_hook` (eager launches, one step per call);
after every step the buffers are copied to the host.  The state after step i is the pre-state of step i + 1, the state
after em_search_init is held against the restatement's initial state.  Per step, from the DEVICE's own pre-state:
log-softmax rows, the pre-beam (order, values, nothing better left outside), log psi and the total of every candidate
slot (the extra <eos> slot and its `dup` rule included), the selection (EXACT: a pure function of the device's totals:
value descending, flat index ascending) and the complete new state (integers exact; floats recomputed in float64 for the
device's selection).  Where the selection ran as the global-memory loop (W*NC > 1024) the winners' totals were knocked
out of cand_total by the kernel; they are put back from sel_total, which the update leaves holding them.

Float bounds: |device - float64 restatement| per label step and quantity, 4x the largest value seen on MI355X (f32 and
bf16 cells alike: the restatement reads the log-prob rows the device wrote, so the scorers' dtype does not enter).  The CTC
quantities are log-probabilities of whole frame sequences, about 4 nats per frame, so their magnitude and with it one f32
ulp grows with the memory: three groups of cells by frame stride T.  Largest values seen (bound):
                          lse               weighted          log psi           total             r                 running sums
  T = 32 (all others)     1.9e-6 (8e-6)     4.5e-7 (2e-6)     1.5e-5 (6e-5)     1.4e-5 (5.7e-5)   4.5e-5 (1.8e-4)   6.7e-6 (2.7e-5)
  T 192..768 (tail tiers) 6.0e-7            1.2e-7            1.2e-4 (4.9e-4)   8.9e-5 (3.6e-4)   1.2e-3 (4.9e-3)   1.3e-6
  T 1248..2048 (capacity) 4.2e-7            1.1e-7            2.2e-4 (8.8e-4)   2.2e-4 (8.8e-4)   5.4e-3 (2.2e-2)   3.8e-7
(lse, weighted and the running sums do not depend on T and keep the first row's bounds.)  r above 2e-3 in the capacity
cells is not a defect of the step: the forward variables there are -4 000 .. -8 000, one f32 ulp is 4.9e-4, and the
values come out of a recurrence over up to 2 048 frames: 5.4e-3 (11 ulp) is the sequential blank cumsum of em_search_init
at T = 2048 and 1248, 3.6e-3 (7 ulp) the winners' chains; log psi and the totals, which decide the search, stay at 2.2e-4.

Near-ties: a pre-beam boundary decision whose float64 margin (worst token kept - best token left out) is below the
weighted-score bound cannot be judged; they are counted and printed per cell and at most 1% of a cell's (row, step)
decisions may be such.  Exact ties (equal float64 scores, i.e. equal device log-probs) ARE judged: lowest id stays.
The seeds named in the cells' docstrings were checked on the device: every cell printed 0 near-ties with them.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import search_step_ref as ref  # noqa: E402
from tests.helpers import golden_state_dict, load_golden  # noqa: E402

# quantity -> bound, by frame stride (module docstring)
BOUNDS = dict(lse=8e-6, weighted=2e-6, psi=6e-5, total=5.7e-5, r=1.8e-4, run=2.7e-5)
BOUNDS_LONG = dict(BOUNDS, psi=4.9e-4, total=3.6e-4, r=4.9e-3)
BOUNDS_CAPACITY = dict(BOUNDS, psi=8.8e-4, total=8.8e-4, r=2.2e-2)

SNAP = ["xlens", "maxlens", "minlens", "tok", "parent", "anc_a", "anc_b", "alive", "run_score", "run_sdec", "run_sctc",
        "run_slen", "run_slm", "s_prev", "r_a", "r_b", "cand_tok", "cand_full", "cand_psi", "cand_total", "sel_idx",
        "sel_total", "end_count", "end_pos", "end_slot", "end_forced", "end_score", "end_sdec", "end_sctc", "end_slen",
        "end_slm", "best_all", "best_by_len", "done", "dec_logp", "lm_logp"]


# ------------------------------------------------------------------------------------------------ models and cells
def tiny_case(V=50, beam=5, ctc_weight=None, penalty=0.0, base="tiny_beam5"):
    """The goldens' tiny decoder (d 64, 2 heads, ff 128, one block) and CTC head with recipe weights at vocabulary V."""
    from oracle.weights import recipe_state_dict

    g = dict(load_golden(base))
    V0 = int(g["vocab"])
    shapes = {k: tuple(V if (s == V0 and ("output_layer" in k or "embed.0" in k or "ctc_lo" in k)) else s for s in shp)
              for k, shp in g["shapes"].items() if k.startswith(("decoder.", "ctc."))}
    sd = golden_state_dict(g) if V == V0 else recipe_state_dict(shapes, int(g["wseed"]))
    sd = {k: v for k, v in sd.items() if k.startswith(("decoder.", "ctc.", "lm."))}
    g.update(vocab=np.int64(V), beam=np.int64(beam), penalty=np.float64(penalty))
    if ctc_weight is not None:
        g["ctc_weight"] = np.float64(ctc_weight)
    return g, sd


def memory(g, lens, seed, dtype):
    d = g["config"]["encoder_conf"]["output_size"]
    gen = torch.Generator().manual_seed(seed)
    enc = torch.randn(len(lens), max(lens), d, generator=gen) * 0.7
    for b, n in enumerate(lens):
        enc[b, n:] = 0.0
    return enc.to(torch.bfloat16 if dtype == "bfloat16" else torch.float32)


def build(g, sd, dtype, lm=False):
    from tests.test_gpu_search import build_lm, build_search

    bs = build_search(g, sd, dtype, lm=build_lm(g, dtype) if lm else None)
    bs.use_hipgraph = False
    return bs


# ------------------------------------------------------------------------------------------------ walking the steps
def snapshot(bufs):
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy().copy() for k in SNAP if k in bufs}


def walk(bs, enc, olens, maxlenratio):
    """Runs the search with the step hook: every label step on its own, a host copy of the buffers after each, then the
    search itself (from its own init).  Returns (params dict, snapshots [after init, after step 0, ...], ctc_lpT, hyps)."""
    rec = {}

    def hook(p, bufs, init, steps, maxlens, em_dtype):
        rec["p"] = {f: getattr(p, f) for f, _ in p._fields_}
        init()
        snaps = [snapshot(bufs)]
        for i in range(max(maxlens)):
            steps(i, i + 1)
            snaps.append(snapshot(bufs))
            if snaps[-1]["done"].all():
                break
        rec["snaps"] = snaps
        if "ctc_lpT" in bufs:
            rec["lpT"] = bufs["ctc_lpT"].cpu().numpy().astype(np.float64).reshape(p.V, p.B, p.T)

    assert not bs.use_hipgraph
    bs.step_hook = hook
    try:
        hyps = bs.search_batch(enc.cuda(), olens, maxlenratio)
    finally:
        bs.step_hook = None
    return rec["p"], rec["snaps"], rec.get("lpT"), hyps


def to_state(s, i, p):
    """Device snapshot -> the restatement's state at step i (float64 / int64; r and anc of parity i)."""
    n = p["B"] * p["W"]
    st = {}
    for k in ("alive", "done", "tok", "parent", "xlens", "maxlens", "minlens", "end_count", "end_pos", "end_slot",
              "end_forced"):
        st[k] = s[k].astype(np.int64)
    for k in ("run_score", "run_sdec", "run_sctc", "run_slen", "s_prev", "end_score", "end_sdec", "end_sctc", "end_slen",
              "best_all", "best_by_len"):
        st[k] = s[k].astype(np.float64)
    st["run_slm"] = s["run_slm"].astype(np.float64) if "run_slm" in s else np.zeros(n)
    st["end_slm"] = s["end_slm"].astype(np.float64) if "end_slm" in s else np.zeros(s["end_score"].shape)
    st["r"] = s["r_b" if i & 1 else "r_a"].astype(np.float64)
    st["anc"] = s["anc_b" if i & 1 else "anc_a"].astype(np.int64)
    return st


class Tally:
    def __init__(self):
        self.err = dict(lse=0.0, weighted=0.0, psi=0.0, total=0.0, r=0.0, run=0.0)
        self.decisions = self.near = self.exact_ties = self.dups = self.sel_ties = 0

    def see(self, q, dev, want):
        """Largest |dev - want| of quantity q.  Entries that are log-zero markers (magnitude 1e10, where one f32 ulp is
        1024: LOGZERO plus a log-prob) are held to 1e-6 relative instead; equal infinities count as equal."""
        dev, want = np.asarray(dev, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
        assert not np.isnan(dev).any() and not np.isnan(want).any(), (q, dev, want)
        zero = np.isfinite(want) & (np.abs(want) > 1e8)
        same = zero | (np.isinf(want) & (dev == want))
        with np.errstate(invalid="ignore"):
            assert (np.abs(dev[zero] - want[zero]) <= 1e-6 * np.abs(want[zero])).all(), (q, dev[zero], want[zero])
            e = np.where(same, 0.0, np.abs(dev - want))
        self.err[q] = max(self.err[q], float(e.max()) if e.size else 0.0)


def check_init(p, s0, lpT):
    n, W = p["B"] * p["W"], p["W"]
    want = ref.initial_state(p, s0["xlens"], s0["maxlens"], s0["minlens"], lpT)
    assert s0["alive"].tolist() == want["alive"].tolist()
    assert (s0["tok"][0] == p["sos"]).all() and (s0["parent"][0] == -1).all()
    for a in ("anc_a", "anc_b"):
        assert (s0[a] == np.arange(n)[:, None]).all()
    assert (s0["run_score"] == want["run_score"]).all()
    for k in ("run_sdec", "run_sctc", "run_slen", "s_prev") + (("run_slm",) if "run_slm" in s0 else ()):
        assert (s0[k] == 0).all(), k
    assert (s0["end_count"] == 0).all() and (s0["done"] == 0).all()
    assert (s0["best_all"] == -np.inf).all() and (s0["best_by_len"] == -np.inf).all()
    worst = 0.0
    if p["w_ctc"] != 0:
        for b in range(p["B"]):
            x = int(s0["xlens"][b])
            assert (s0["r_a"][b * W, :x, 0] == np.float32(ref.LOGZERO)).all()
            worst = max(worst, float(np.abs(s0["r_a"][b * W, :x, 1] - want["r"][b * W, :x, 1]).max()))
    return worst


def check_step(p, pre_s, post_s, i, lpT, bounds, tl):
    """One device label step (pre_s -> post_s) against the restatement."""
    B, W, V, S, NC = p["B"], p["W"], p["V"], p["S"], p["NC"]
    n = B * W
    pre = to_state(pre_s, i, p)
    dec_logp = post_s["dec_logp"].astype(np.float64) if p["w_dec"] != 0 else None
    lm_logp = post_s["lm_logp"].astype(np.float64) if p["w_lm"] != 0 else None
    ctc = p["w_ctc"] != 0
    cand_tok = post_s["cand_tok"].astype(np.int64)
    cand_total = post_s["cand_total"].astype(np.float64)
    sel_idx = post_s["sel_idx"].astype(np.int64)
    # the global-memory selection loop knocks its winners out of cand_total: put them back (module docstring)
    if W * NC > 64 * 16:
        for rnew in range(n):
            b = rnew // W
            if sel_idx[rnew] >= 0 and not pre["done"][b]:
                flat = cand_total[b * W:(b + 1) * W].reshape(-1)
                assert flat[sel_idx[rnew]] == -np.inf
                cand_total[b * W + sel_idx[rnew] // NC, sel_idx[rnew] % NC] = float(post_s["sel_total"][rnew])
    for r in range(n):
        b = r // W
        if not pre["alive"][r] or pre["done"][b]:
            assert (post_s["cand_total"][r] == -np.inf).all(), ("a dead / done row carries candidates", i, r)
            continue
        # ---- log-softmax rows
        for lp in (dec_logp, lm_logp):
            if lp is not None:
                m = lp[r].max()
                tl.see("lse", m + math.log(np.exp(lp[r] - m).sum()), 0.0)
        w = ref.weighted_full(p, dec_logp, lm_logp, r)
        # ---- pre-beam
        if S < V:
            ids, full = cand_tok[r, :S], post_s["cand_full"][r, :S].astype(np.float64)
            assert len(set(ids.tolist())) == S and ids.min() >= 0 and ids.max() < V, (i, r, ids)
            for k in range(S - 1):
                assert full[k] > full[k + 1] or (full[k] == full[k + 1] and ids[k] < ids[k + 1]), (i, r, k, full, ids)
            tl.see("weighted", full, w[ids])
            out = np.ones(V, bool)
            out[ids] = False
            outside = np.nonzero(out)[0]
            best_out = outside[np.argmax(w[outside])]  # (argmax: lowest id among equals)
            assert w[best_out] <= full[S - 1] + bounds["weighted"], (i, r, best_out, w[best_out], full[S - 1])
            tl.decisions += 1
            worst_in = w[ids].min()
            if w[best_out] == worst_in:  # an exact tie across the boundary: the lowest ids stay
                tl.exact_ties += 1
                assert best_out > ids[w[ids] == worst_in].max(), ("tie order at the pre-beam boundary", i, r, best_out, ids)
            elif worst_in - w[best_out] < bounds["weighted"]:
                tl.near += 1
            assert cand_tok[r, S] == p["eos"]
        else:
            assert (cand_tok[r] == np.arange(V)).all()
        # ---- candidates: log psi and total of every slot
        for s in range(NC):
            tk = int(cand_tok[r, s])
            if S < V and s == S and p["eos"] in cand_tok[r, :S].tolist():
                tl.dups += 1
                assert cand_total[r, s] == -np.inf, ("dup <eos> slot", i, r)
                continue
            psi, tot = ref.total_of(p, pre, i, lpT, r, tk, w[tk])
            if ctc:
                tl.see("psi", post_s["cand_psi"][r, s], psi)
            if abs(tot) > 1e8:  # a LOGZERO term (blank): one f32 ulp there is 256
                assert abs(cand_total[r, s] - tot) <= 1e-6 * abs(tot)
            else:
                tl.see("total", cand_total[r, s], tot)
    # ---- selection: exact
    want_sel = ref.select(p, cand_total)
    assert sel_idx.tolist() == want_sel.tolist(), ("selection", i, sel_idx.tolist(), want_sel.tolist())
    for b in range(B):
        flat = cand_total[b * W:(b + 1) * W].reshape(-1)
        v = [flat[j] for j in sel_idx[b * W:(b + 1) * W] if j >= 0]
        tl.sel_ties += sum(1 for a, c in zip(v, v[1:]) if a == c)
    # ---- the new state, for the device's own selection
    new, written = ref.apply_selection(p, pre, i, lpT, dec_logp, lm_logp, sel_idx, cand_tok)
    post = to_state(post_s, i + 1, p)
    assert post["alive"].tolist() == new["alive"].tolist(), ("alive", i)
    assert post["done"].tolist() == new["done"].tolist(), ("done", i)
    assert post["end_count"].tolist() == new["end_count"].tolist(), ("end_count", i)
    for r in range(n):
        b = r // W
        if sel_idx[r] >= 0 and not pre["done"][b]:
            assert post["tok"][i + 1, r] == new["tok"][i + 1, r] and post["parent"][i + 1, r] == new["parent"][i + 1, r]
            assert post["anc"][r, :i + 2].tolist() == new["anc"][r, :i + 2].tolist(), ("anc", i, r)
    assert (post["tok"][:i + 1] == pre["tok"][:i + 1]).all() and (post["parent"][:i + 1] == pre["parent"][:i + 1]).all()
    for k in ("s_prev", "run_score", "run_sdec", "run_sctc", "run_slen", "run_slm"):
        tl.see("run", post[k], new[k])
    for b in range(B):
        c = int(new["end_count"][b])
        for k in ("end_pos", "end_slot", "end_forced"):
            assert post[k][b, :c].tolist() == new[k][b, :c].tolist(), (k, i, b)
        for k in ("end_score", "end_sdec", "end_sctc", "end_slen", "end_slm"):
            tl.see("run", post[k][b, :c], new[k][b, :c])
        tl.see("run", post["best_all"][b], new["best_all"][b])
        tl.see("run", post["best_by_len"][b], new["best_by_len"][b])
    for r, frames in written.items():
        if frames:
            tl.see("r", post["r"][r, frames[0]:frames[-1] + 1], new["r"][r, frames[0]:frames[-1] + 1])


def same_hyps(a, b):
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert x.yseq.tolist() == y.yseq.tolist()
            assert float(x.score) == float(y.score)
            assert {k: float(v) for k, v in x.scores.items()} == {k: float(v) for k, v in y.scores.items()}


def run_cell(tag, bs, enc, olens, maxlenratio, monkeypatch, bounds=BOUNDS, equalities=True, min_steps=1):
    """Walks the cell's steps against the restatement, asserts the bounds and the near-tie share, then the whole-search
    equalities: unfused tail == default, hipGraph replay == eager (bit for bit)."""
    from espnet_amd import lib as L

    p, snaps, lpT, hyps = walk(bs, enc, olens, maxlenratio)
    tl = Tally()
    init_err = check_init(p, snaps[0], lpT)
    for i in range(len(snaps) - 1):
        check_step(p, snaps[i], snaps[i + 1], i, lpT, bounds, tl)
    assert len(snaps) - 1 >= min_steps
    print(f"[{tag}] V {p['V']} W {p['W']} S {p['S']} NC {p['NC']} T {p['T']} steps {len(snaps) - 1}: init r {init_err:.1e} " +
          " ".join(f"{k} {v:.2e}" for k, v in tl.err.items()) +
          f" | pre-beam decisions {tl.decisions} near-ties {tl.near} exact ties {tl.exact_ties} dup slots {tl.dups}"
          f" selection ties {tl.sel_ties}")
    assert init_err <= bounds["r"]
    for k, v in tl.err.items():
        assert v <= bounds[k], (tag, k, v, bounds[k])
    assert tl.near <= 0.01 * tl.decisions, (tag, tl.near, tl.decisions)
    if equalities:
        monkeypatch.setenv("ESPNET_AMD_NO_TAIL_FUSION", "1")
        L.load().em_dev_switches_reload()
        try:
            unfused = bs.search_batch(enc.cuda(), olens, maxlenratio)
        finally:
            monkeypatch.delenv("ESPNET_AMD_NO_TAIL_FUSION")
            L.load().em_dev_switches_reload()
        same_hyps(hyps, unfused)
        bs.use_hipgraph = True
        try:
            replay = bs.search_batch(enc.cuda(), olens, maxlenratio)
        finally:
            bs.use_hipgraph = False
        same_hyps(hyps, replay)
    return p, snaps, hyps, tl


def contains_oracle_nbest(g, sd, enc, olens, hyps, maxlenratio):
    from oracle import beam_search as ob

    V, dc = int(g["vocab"]), g["config"]["decoder_conf"]
    for b, T in enumerate(olens):
        with torch.no_grad():
            want = ob.beam_search(sd, enc[b, :T].float(), dc["attention_heads"], dc["num_blocks"], int(g["beam"]),
                                  float(g["ctc_weight"]), sos=V - 1, eos=V - 1, penalty=float(g["penalty"]),
                                  maxlenratio=maxlenratio)
        mine = {tuple(h.yseq.tolist()): float(h.score) for h in hyps[b]}
        assert len(want) > 0
        for r in want:
            assert tuple(r["yseq"]) in mine, (b, r["yseq"])
            assert abs(mine[tuple(r["yseq"])] - r["score"]) < 2e-3 + 2e-5 * abs(r["score"])


# ------------------------------------------------------------------------------------------------ the cells
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_baseline_searched_to_the_end(dtype, monkeypatch):
    """V 50, beam 5, three ragged memories, one of a single frame, searched to the end: ended list, forced <eos>,
    end detection, a done utterance beside running ones (seed 1)."""
    g, sd = tiny_case()
    lens = [26, 1, 17]
    p, snaps, hyps, tl = run_cell(f"baseline {dtype}", build(g, sd, dtype), memory(g, lens, 1, dtype), lens, 0.0,
                                  monkeypatch, min_steps=2)
    assert snaps[1]["done"][1] == 1 and not snaps[1]["done"].all()  # the 1-frame utterance is done after step 0
    assert snaps[1]["end_forced"][1, 0] == 1
    assert all(len(h) > 0 for h in hyps)


@pytest.mark.parametrize("V,dtype", [(2048, "float32"), (2049, "float32"), (5120, "float32"), (5121, "float32"),
                                     (5121, "bfloat16"), (10240, "float32"), (10241, "float32")])
def test_row_kernel_vocabulary_edges(V, dtype, monkeypatch):
    """logsoftmax_prebeam_kernel<8> / <20> / <40> and the generic prebeam_kernel + candidate_kernel path, on both sides of
    every switch; beam 10, two ragged memories, four steps (seed 2)."""
    g, sd = tiny_case(V=V, beam=10)
    lens = [29, 24]
    run_cell(f"V {V} {dtype}", build(g, sd, dtype), memory(g, lens, 2, dtype), lens, -4.0, monkeypatch, min_steps=4)


@pytest.mark.parametrize("beam", [11, 12, 16, 17, 43, 64])
def test_prebeam_width_and_selection_tiers(beam, monkeypatch):
    """Lane merge (S 16) / register merge (S 18); fused tail up to W 16; selection W*NC <= 256 / <= 1024 / loop.  V 300,
    three steps: the third has all W rows alive (seed 3)."""
    g, sd = tiny_case(V=300, beam=beam)
    lens = [24, 19] if beam <= 17 else [24]
    run_cell(f"beam {beam}", build(g, sd, "float32"), memory(g, lens, 3, "float32"), lens, -3.0, monkeypatch, min_steps=3)


def test_prebeam_wider_than_the_row_kernel(monkeypatch):
    """pre_beam_ratio 3.0 at beam 43: S = 129 > PREBEAM_SMAX, the generic path by width (seed 4)."""
    g, sd = tiny_case(V=300, beam=43)
    bs = build(g, sd, "float32")
    bs.pre_beam_size = int(3.0 * 43)
    p, *_ = run_cell("S 129", bs, memory(g, [24], 4, "float32"), [24], -3.0, monkeypatch, min_steps=3)
    assert p["S"] == 129 and p["NC"] == 130


@pytest.mark.parametrize("V", [50, 300])
@pytest.mark.parametrize("penalty", [0.0, 0.5])
def test_all_vocabulary_mode(V, penalty, monkeypatch):
    """ctc_weight 1.0: no decoder, no pre-beam, candidate_kernel over NC == V slots (seed 5)."""
    g, sd = tiny_case(V=V, beam=5, ctc_weight=1.0, penalty=penalty)
    lens = [27, 22]
    enc = memory(g, lens, 5, "float32")
    p, snaps, hyps, tl = run_cell(f"all-vocabulary V {V} penalty {penalty}", build(g, sd, "float32"), enc, lens, -5.0,
                                  monkeypatch, min_steps=5)
    assert p["S"] == V and p["NC"] == V and p["w_dec"] == 0
    contains_oracle_nbest(g, sd, enc, lens, hyps, -5.0)


def test_attention_only(monkeypatch):
    """ctc_weight 0.0: no CTC state at all; V 300, beam 5 (seed 6)."""
    g, sd = tiny_case(V=300, beam=5, ctc_weight=0.0)
    lens = [27, 22]
    enc = memory(g, lens, 6, "float32")
    p, snaps, hyps, tl = run_cell("attention only", build(g, sd, "float32"), enc, lens, -5.0, monkeypatch, min_steps=5)
    assert p["w_ctc"] == 0 and p["NC"] == 300
    contains_oracle_nbest(g, sd, enc, lens, hyps, -5.0)


@pytest.mark.parametrize("name,dtype", [("tiny_beam5_lm", "float32"), ("tiny_beam60_lm_v300", "float32"),
                                        ("tiny_beam4_lm_posenc", "bfloat16"), ("tiny_beam60_lm_v300", "bfloat16")])
def test_with_lm_scorer(name, dtype, monkeypatch):
    """The w_lm term and the scorer order (decoder, length_bonus, lm); beam 60 (seed 7).  tiny_beam5_lm has no bf16 cell: its
    LM's embed_unit is 32 and the bf16 pack refuses it before any launch (NotImplementedError "embed_unit must be a multiple
    of 64 in bfloat16 mode"); tiny_beam4_lm_posenc, the LM model the suite's other bf16 tests use, stands in."""
    g = load_golden(name)
    sd = golden_state_dict(g)
    lens = [25, 20] if int(g["beam"]) < 60 else [25]
    steps = 4 if int(g["beam"]) < 60 else 3
    p, *_ = run_cell(f"{name} {dtype}", build(g, sd, dtype, lm=True), memory(g, lens, 7, dtype), lens, -float(steps),
                     monkeypatch, min_steps=steps)
    assert p["w_lm"] != 0


@pytest.mark.parametrize("beam,T", [(10, 320), (10, 352), (10, 736), (10, 768), (16, 192), (16, 224), (16, 448), (16, 480)])
def test_tail_lds_tiers(beam, T, monkeypatch):
    """tail_lds = W*5*ldT*4 bytes: default (<= 64 KiB), raised cap (<= 144 KiB), unfused above, on both sides of each edge;
    three steps, two memories, the longer one of exactly the frame stride (seed 8)."""
    g, sd = tiny_case(V=50, beam=beam)
    lens = [T, T - 37]
    p, *_ = run_cell(f"tail W {beam} T {T}", build(g, sd, "float32"), memory(g, lens, 8, "float32"), lens, -3.0, monkeypatch,
                     bounds=BOUNDS_LONG, min_steps=3)
    assert p["T"] == T


@pytest.mark.parametrize("dtype,T", [("float32", 1248), ("bfloat16", 1696), ("ctc_only", 2048)])
def test_ctc_frame_capacity(dtype, T, monkeypatch):
    """CTC_TMAX = 2048 sizes the row kernel's phi arrays and the chain kernels' LDS.  The tiny decoder does not accept a
    2048-frame memory: em_search_steps returns EM_ERR_UNSUPPORTED (-1) there, the source attention's score rows (16 rows x
    Tpad, LDS) end at Tpad 1248 in f32 and 1696 in bf16 - the largest memories the fused row kernel can meet, run here.
    T = 2048 itself is reached by the CTC-only search (no decoder: candidate_kernel and the chain in the fused tail under
    the raised LDS cap); one frame more is refused by em_search_init.  Beam 2, two steps (seed 9)."""
    g, sd = tiny_case(V=50, beam=2, ctc_weight=1.0 if dtype == "ctc_only" else None)
    bs = build(g, sd, "float32" if dtype == "ctc_only" else dtype)
    lens = [T, T - 37]
    p, *_ = run_cell(f"capacity {dtype} T {T}", bs, memory(g, lens, 9, dtype), lens, -2.0, monkeypatch,
                     bounds=BOUNDS_CAPACITY, min_steps=2)
    assert p["T"] == T
    if T == 2048:
        with pytest.raises(NotImplementedError):
            bs.search_batch(memory(g, [2049], 9, dtype).cuda(), [2049], -2.0)


def test_tie_order(monkeypatch):
    """Identical rows (weight and bias) in the decoder's output layer AND the CTC head: tokens 40 == 41 and 100 == 101.
    Six tokens (40, 41 among them) carry an output bias of +30 and fill the pre-beam's first six places on every row; 100
    and 101 carry +15 and tie for the seventh and last place (S = 7): the pair straddles the boundary by construction and
    100 must stay.  40 and 41 tie inside the pre-beam with equal CTC scores, so their totals tie in the selection:
    lowest flat index first (seed 10)."""
    g, sd = tiny_case(V=300, beam=5)
    top = [17, 40, 41, 77, 150, 222]
    for a, b in ((40, 41), (100, 101)):
        for k in ("decoder.output_layer", "ctc.ctc_lo"):
            sd[k + ".weight"][b] = sd[k + ".weight"][a]
            sd[k + ".bias"][b] = sd[k + ".bias"][a]
    sd["decoder.output_layer.bias"][top] += 30.0
    sd["decoder.output_layer.bias"][[100, 101]] += 15.0
    lens = [27, 22]
    p, snaps, hyps, tl = run_cell("ties", build(g, sd, "float32"), memory(g, lens, 10, "float32"), lens, -4.0, monkeypatch,
                                  min_steps=4)
    assert p["S"] == 7
    assert tl.exact_ties == tl.decisions > 0, (tl.exact_ties, tl.decisions)
    for s in snaps[1:]:
        for r in np.nonzero(s["cand_total"][:, 0] > -np.inf)[0]:
            ids = s["cand_tok"][r, :7].tolist()
            assert sorted(ids) == sorted(top + [100]) and ids.index(40) + 1 == ids.index(41), (r, ids)
    assert tl.sel_ties > 0


@pytest.mark.parametrize("V", [100, 300])
def test_selection_tie_order_inside_one_lane(V, monkeypatch):
    """The selection keeps its candidates in registers, flat index = lane + 64 k: two equal totals 64 apart sit in ONE
    lane, where only the strict comparison of the scan keeps the lower index.  CTC-only search (slot = token), tokens 10
    and 74 with identical, favoured CTC head rows: equal totals in every row, among the winners.  V 100: the register form
    (W*NC = 500); V 300: the global-memory loop (1500) (seed 12)."""
    g, sd = tiny_case(V=V, beam=5, ctc_weight=1.0)
    for k in ("weight", "bias"):
        sd["ctc.ctc_lo." + k][74] = sd["ctc.ctc_lo." + k][10]
    sd["ctc.ctc_lo.bias"][[10, 74]] += 4.0
    lens = [27, 22]
    p, snaps, hyps, tl = run_cell(f"lane ties V {V}", build(g, sd, "float32"), memory(g, lens, 12, "float32"), lens, -4.0,
                                  monkeypatch, min_steps=4)
    assert tl.sel_ties > 0


def test_one_threads_values_take_the_exact_rounds(monkeypatch):
    """V 2049, beam 10 (S 15): an output bias of +20 on tokens 5, 261, 517, 773 - four of a wave's top S in ONE thread's
    strided values, so its three-deep list runs empty and the wave redoes its rounds the exact way (seed 11)."""
    g, sd = tiny_case(V=2049, beam=10)
    four = [5, 261, 517, 773]
    sd["decoder.output_layer.bias"][four] += 20.0
    lens = [29, 24]
    p, snaps, hyps, tl = run_cell("one thread's values", build(g, sd, "float32"), memory(g, lens, 11, "float32"), lens, -4.0,
                                  monkeypatch, min_steps=4)
    for s in snaps[1:]:
        for r in np.nonzero(s["cand_total"][:, 0] > -np.inf)[0]:
            assert sorted(s["cand_tok"][r, :4].tolist()) == four, (r, s["cand_tok"][r, :15])
