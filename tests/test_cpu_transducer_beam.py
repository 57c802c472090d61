"""The transducer's device beam search without a GPU: its C-ABI entries, its limits as the host names them, and a NumPy
restatement of the walk's bookkeeping (csrc/transducer_beam.hip: open and kept arrays with dead marks instead of list
pops, one node per expanded hypothesis, state slots freed at a frame's end, label sequences from back-pointers) held
against the list-based restatement tests/transducer_ref.py `beam_search_from_logits`."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import transducer_ref as R

REPO = Path(__file__).resolve().parent.parent
NEW = ("em_transducer_beam_limits", "em_transducer_beam_workspace_bytes", "em_transducer_beam_search")
TOK_DEAD, TOK_CARRIED = -1, -2


def test_new_symbols_are_declared_bound_and_exported():
    from espnet_amd import lib as L

    hdr = (REPO / "include" / "espnet_amd.h").read_text()
    declared = set(re.findall(r"\b(em_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    table = subprocess.run(["nm", "-D", "--defined-only", str(L.library_path())], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in table.splitlines() if ln.strip()}
    for name in NEW:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name) and name in exported, name
    res, args = L._SIGNATURES["em_transducer_beam_search"]
    assert res is C.c_int and len(args) == 22 and args[-2] is C.c_size_t
    assert L._SIGNATURES["em_transducer_beam_workspace_bytes"][0] is C.c_size_t


def test_limits_are_what_the_host_names():
    """em_transducer_beam_limits runs without a GPU; `beam_device` names every one of its values when it refuses a beam,
    and the workspace query refuses (0) what the search entry refuses."""
    from espnet_amd import lib as L
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.transducer import beam_search_transducer as B
    from espnet_amd.asr.transducer.joint_network import JointNetwork

    lim = B.beam_limits()
    assert set(lim) == {"beam", "open", "kept", "expansions", "labels"} and all(v > 0 for v in lim.values())
    assert lim["open"] == lim["kept"] + lim["expansions"] * lim["beam"]  # carried entries + beam children per expansion
    assert lim["beam"] >= 10 and B.MAX_WALK_ROWS == 64
    dec, jn = TransducerDecoder(10, hidden_size=16), JointNetwork(10, 64, 16, joint_space_size=16)
    bs = B.BeamSearchTransducer(dec, jn, beam_size=lim["beam"] + 1)
    enc = torch.zeros(1, 2, 64)
    with pytest.raises(L.EspnetAmdError):  # (a CPU tensor: refused before the limits are looked at)
        bs.beam_device(enc, [2])
    # the message, taken where it is raised without a device: patch the device check away
    real = L.require_gpu
    L.require_gpu = lambda *a, **k: None
    try:
        with pytest.raises(NotImplementedError) as ei:
            bs.beam_device(enc, [2])
    finally:
        L.require_gpu = real
    named = [int(v) for v in re.findall(r"\d+", str(ei.value))]
    assert named == [lim["beam"] + 1, lim["beam"], lim["open"], lim["kept"], lim["expansions"], lim["labels"]]
    w = L.EmTransducerWeights()
    w.kind, w.vocab, w.nhid, w.d, w.num_layers, w.joint, w.jp, w.blank = L.EM_LM_LSTM, 50, 64, 64, 1, 64, 64, 0
    w.embed = w.lin_dec = w.lin_out = w.out_b = 64  # (non-NULL; the query reads the shape only)
    w.rnn = C.cast(C.pointer(L.EmRnnLayer()), C.POINTER(L.EmRnnLayer))
    q = L.load().em_transducer_beam_workspace_bytes
    assert int(q(L.EM_F32, C.byref(w), 5, 16, 4)) > 0
    assert int(q(L.EM_F32, C.byref(w), 64, 16, lim["beam"])) > 0
    assert int(q(L.EM_F32, C.byref(w), 65, 16, 4)) == 0
    assert int(q(L.EM_F32, C.byref(w), 5, 16, lim["beam"] + 1)) == 0
    assert int(q(L.EM_F32, C.byref(w), 5, 0, 4)) == 0


# ---------------------------------------------------------------------- the walk's bookkeeping, restated on arrays
def array_walk(logits_fn, T, V, beam_size, exp_cap=128, blank=0, trace=None, max_steps=None):
    """The device walk of one utterance, step by step as select / expand do it.  Returns ([(score, yseq)] in kept order,
    stats) or (None, stats) when a frame reaches exp_cap expansions (or the walk max_steps).  trace: a list that takes
    (frame, label sequence) of every step's expanded hypothesis."""
    beam = min(beam_size, V)
    beam_k = min(beam, V - 1)
    nslot = 2 * exp_cap
    ocap = exp_cap + exp_cap * beam_k
    open_score, open_node, open_tok = np.zeros(ocap), np.zeros(ocap, np.int64), np.full(ocap, TOK_DEAD, np.int64)
    kept_score, kept_node = np.zeros(exp_cap), np.zeros(exp_cap, np.int64)
    nodes = []  # (parent, token, length, slot)
    slot_used = np.zeros(nslot, bool)
    slot_seq = [None] * nslot  # stands for the state a slot holds: the label sequence that produced it
    open_score[0], open_node[0], open_tok[0] = 0.0, -1, blank
    n_open, n_kept, n_exp, t = 1, 0, 0, 0
    stats = dict(steps=0, max_exp=0, max_open=1, max_slots=0)

    def yseq(n):
        out = []
        while n >= 0:
            out.append(nodes[n][1])
            n = nodes[n][0]
        return out[::-1]

    while True:
        # select: the best open entry, the lowest index of equal scores
        alive = np.flatnonzero(open_tok[:n_open] != TOK_DEAD)
        i = alive[np.argmax(open_score[alive])]  # (argmax: the first of equal maxima)
        node, tk, score = int(open_node[i]), int(open_tok[i]), float(open_score[i])
        open_tok[i] = TOK_DEAD
        if tk == TOK_CARRIED:
            e = node
            assert slot_used[nodes[e][3]] and slot_seq[nodes[e][3]] == yseq(e)  # its lin_dec row is still stored
        else:
            if node >= 0:  # the pre-state: the parent's slot, still held
                assert slot_used[nodes[node][3]] and slot_seq[nodes[node][3]] == yseq(node)
            slot = int(np.flatnonzero(~slot_used)[0])
            nodes.append((node, tk, (nodes[node][2] if node >= 0 else 0) + 1, slot))
            e = len(nodes) - 1
            slot_used[slot], slot_seq[slot] = True, yseq(e)
        if trace is not None:
            trace.append((t, yseq(e)))
        # expand
        logp = R.log_softmax(torch.as_tensor(np.asarray(logits_fn(t, tuple(yseq(e))), dtype=np.float64))).numpy()
        kept_score[n_kept], kept_node[n_kept] = score + float(logp[0]), e
        n_kept += 1
        pv, pi = np.inf, -1
        for j in range(beam_k):  # rank rounds: the best label below the last pick, the lowest id of equal ones
            cand = [c for c in range(1, V) if logp[c] < pv or (logp[c] == pv and c > pi)]
            c = max(cand, key=lambda c: (logp[c], -c))
            open_score[n_open], open_node[n_open], open_tok[n_open] = score + float(logp[c]), e, c
            n_open += 1
            pv, pi = logp[c], c
        n_exp += 1
        stats["steps"] += 1
        stats["max_exp"], stats["max_open"] = max(stats["max_exp"], n_exp), max(stats["max_open"], n_open)
        stats["max_slots"] = max(stats["max_slots"], int(slot_used.sum()))
        alive = np.flatnonzero(open_tok[:n_open] != TOK_DEAD)
        best_left = open_score[alive].max()
        above = np.flatnonzero(kept_score[:n_kept] > best_left)
        if max_steps is not None and stats["steps"] >= max_steps:
            return None, stats
        if len(above) < beam:
            if n_exp >= exp_cap:
                return None, stats
            continue
        if t + 1 == T:
            return [(float(kept_score[k]), yseq(int(kept_node[k]))) for k in above], stats
        for pos, k in enumerate(above):  # the next frame's open set, in kept order; every other slot is free
            open_score[pos], open_node[pos], open_tok[pos] = kept_score[k], kept_node[k], TOK_CARRIED
        slot_used[:] = False
        for k in above:
            slot_used[nodes[int(kept_node[k])][3]] = True
        n_open, n_kept, n_exp, t = len(above), 0, 0, t + 1


def finish(entries, nbest, score_norm):
    most = sorted(entries, key=lambda h: h[0])
    key = (lambda h: h[0] / len(h[1])) if score_norm else (lambda h: h[0])
    return sorted(most, key=key, reverse=True)[:nbest]


def random_logits(seed, V, levels=None, blank_up=1.5):
    """logits_fn(t, yseq): N(0, 1) drawn per (seed, t, yseq), the blank raised so that frames end; `levels`: quantised to
    that many values, so that exact ties abound (equal log-probabilities, equal scores)."""
    def fn(t, y):
        g = np.random.default_rng([seed, t, len(y)] + list(y))
        x = g.standard_normal(V)
        if levels:
            x = np.round(x * (levels / 4.0)) * (4.0 / levels)
        x[0] += blank_up
        return x
    return fn


@pytest.mark.parametrize("levels", [None, 3, 2])
@pytest.mark.parametrize("V,T,beam", [(2, 3, 2), (3, 6, 2), (4, 5, 4), (5, 4, 3), (8, 6, 4), (8, 4, 10), (6, 1, 3)])
def test_array_walk_equals_the_list_restatement(V, T, beam, levels):
    slots = 0
    for seed in range(4):
        fn = random_logits(seed, V, levels)
        got, stats = array_walk(fn, T, V, beam)
        assert got is not None, stats
        slots = max(slots, stats["max_slots"])
        for score_norm in (True, False):
            want = R.beam_search_from_logits(fn, T, V, beam, nbest=64, score_norm=score_norm)
            mine = finish(got, 64, score_norm)
            assert [y for _, y in mine] == [y for _, y in want], (seed, score_norm)
            assert [s for s, _ in mine] == [s for s, _ in want]  # the same sums in the same order: equal, not close
    assert slots <= 2 * 128


def test_array_walk_pinned_by_hand():
    """The garden-path case of tests/test_cpu_transducer.py, and all-equal logits (V = 4, beam 3 = V - 1): every rank
    round and every pop is an exact tie."""
    from tests.test_cpu_transducer import _garden_path

    got, _ = array_walk(_garden_path, 2, 3, 2)
    assert [y for _, y in finish(got, 2, True)] == [[0, 2], [0, 1]]
    flat = lambda t, y: np.zeros(4)  # noqa: E731
    got, stats = array_walk(flat, 3, 4, 3)
    assert got is not None and finish(got, 16, True) == R.beam_search_from_logits(flat, 3, 4, 3, nbest=16)


def test_array_walk_stops_at_the_expansion_capacity():
    """Labels beat blank in every context: the frame is never left, the walk reports it instead of running on."""
    fn = random_logits(0, 4, blank_up=-50.0)
    got, stats = array_walk(fn, 3, 4, 2, exp_cap=16)
    assert got is None and stats["max_exp"] == 16 and stats["max_open"] <= 16 + 16 * 2
