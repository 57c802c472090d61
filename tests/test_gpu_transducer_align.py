"""Transducer forced alignment on the MI355X (csrc/transducer_align.hip) through the C ABI's wrappers and the host layers,
against the float64 restatement of the contract (tests/transducer_align_ref.py) on the SAME lattices.

  * the kernel alone on synthetic lattices whose values are multiples of 2^-6 in [-8, 0] drawn from a few distinct values:
    every f32 sum along a path is exact (at most 2 100 + 300 terms of at most 8: below 2^15, 21 bits with the 6 fractional
    ones), so every output must EQUAL the restatement's, exact ties included;
  * the entry point under poisoned workspace and outputs (tests/scratch_fill.py);
  * the device chain on model lattices: the device's path re-scored in float64 on the device's own lattice against the
    float64 optimum on that lattice, within the f32 rounding of a sum of T_b + U terms;
  * the public interface on the peaked tiny Conformer transducer of tests/test_gpu_transducer.py (its `_model`, `_enc`,
    `_speech2text`, `_waves` are imported, as tests/test_gpu_transducer_nll.py imports them).
"""
import math

import numpy as np
import pytest
import torch

from tests import scratch_fill as sf
from tests import test_gpu_transducer as TG
from tests import transducer_align_ref as R

pytestmark = pytest.mark.gpu

DTYPES = TG.DTYPES
NAMES = ("tok_frame", "tok_logp", "frame_u", "total")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _jn():
    from espnet_amd.asr.transducer.joint_network import JointNetwork

    return JointNetwork(8, 64, 64, 64)


def _exact_lattice(g, Tb, U, T, Lmax, k=3):
    """(T, Lmax + 1, 2) f32: NaN outside (T_b, U), inside k distinct multiples of 2^-6 in [-8, 0] - few values, so a good
    share of the nodes see an exact tie - and -inf for the label of u == U."""
    lat = torch.full((T, Lmax + 1, 2), float("nan"))
    if Tb:
        vals = -torch.randint(0, 8 * 64 + 1, (k,), generator=g).to(torch.float32) / 64.0
        lat[:Tb, : U + 1] = vals[torch.randint(0, k, (Tb, U + 1, 2), generator=g)]
        lat[:Tb, U, 1] = -math.inf
    return lat


def _assert_row_equals(got, n, want, Tb, U, tag):
    """Row n of the device outputs (host tensors) against the restatement's dict: equal, and padding behind the lengths."""
    tok_frame, tok_logp, frame_u, total = got
    assert tok_frame[n, :U].tolist() == want["tok_frame"], tag
    assert tok_logp[n, :U].to(torch.float64).tolist() == want["tok_logp"], tag
    assert frame_u[n, :Tb].tolist() == want["frame_u"], tag
    assert float(total[n]) == want["total"], (tag, float(total[n]), want["total"])
    assert bool((tok_frame[n, U:] == -1).all()) and bool((tok_logp[n, U:] == 0).all()) and bool((frame_u[n, Tb:] == -1).all()), tag
    assert not bool(torch.isnan(tok_logp[n]).any()) and not math.isnan(float(total[n])), tag


def _count_ties(lat, Tb, U):
    """Nodes whose two moves carry exactly the same finite value: the recursion in float64 on the exact inputs, one
    anti-diagonal at a time (cell (t, u) of diagonal d = t + u sits at index u)."""
    lat = lat[:Tb, : U + 1].to(torch.float64).numpy()
    b, e = lat[..., 0], lat[..., 1]
    u = np.arange(U + 1)
    prev = np.full(U + 1, -np.inf)  # v of diagonal d - 1, by column
    ties = 0
    for d in range(Tb + U):
        t = d - u
        on = (t >= 0) & (t < Tb)
        tc = np.clip(t, 0, Tb - 1)
        stay = np.where(on & (t >= 1), prev + b[np.clip(t - 1, 0, Tb - 1), u], -np.inf)
        left = np.concatenate(([-np.inf], prev[:-1]))
        emit = np.where(on & (u >= 1), left + e[tc, np.clip(u - 1, 0, U)], -np.inf)
        ties += int((on & (stay == emit) & (stay > -np.inf)).sum())
        cur = np.maximum(stay, emit)
        if d == 0:
            cur[0] = 0.0
        prev = np.where(on, cur, -np.inf)
    return ties


# ---------------------------------------------------------------------- the kernel alone, exact
# one frame; no tokens; the token cap; the 32-bit word edges of the back-pointer store; a column longer than 64 words
SHAPES = [(1, 0), (1, 5), (7, 0), (3, 1023), (31, 4), (32, 4), (33, 40), (64, 9), (65, 300), (2100, 300)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_on_exact_lattices(shape):
    Tb, U = shape
    T, Lmax = Tb + 3, min(U + 2, 1023)  # padding frames and columns, NaN there
    g = torch.Generator().manual_seed(1000 * Tb + U)
    lat = _exact_lattice(g, Tb, U, T, Lmax)
    got = [o.cpu() for o in _jn().seq_align_device(lat[None].cuda(), _i32([Tb]), _i32([U]))]
    assert [tuple(o.shape) for o in got] == [(1, Lmax), (1, Lmax), (1, T), (1,)]
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    want = R.viterbi(lat, Tb, U)
    assert math.isfinite(want["total"])
    _assert_row_equals(got, 0, want, Tb, U, shape)
    if Tb > 1 and U > 0:  # (one frame or no token: one path, nothing to tie)
        ties, inner = _count_ties(lat, Tb, U), (Tb - 1) * U  # nodes with two predecessors
        print(f"\nexact lattice {Tb} x {U}: {ties} of {inner} two-way nodes with an exact tie")
        assert ties * 50 >= inner  # a good share: at least one node in fifty decides by the tie rule


def test_all_equal_lattice_takes_every_tie_as_a_blank_move():
    """-1 everywhere: every path scores the same and every node ties; the blank move is kept, so seen from the end the
    path runs back over blanks: every token is emitted on frame 0."""
    Tb, U = 40, 7
    lat = torch.full((1, Tb, U + 1, 2), -1.0)
    lat[:, :, U, 1] = -math.inf
    got = [o.cpu() for o in _jn().seq_align_device(lat.cuda(), _i32([Tb]), _i32([U]))]
    assert got[0][0].tolist() == [0] * U and got[2][0].tolist() == [U] * Tb and float(got[3][0]) == -(Tb + U)
    _assert_row_equals(got, 0, R.viterbi(lat[0], Tb, U), Tb, U, "all equal")


# ---------------------------------------------------------------------- one finite path: the two recursions agree
# the smallest case; one frame, several tokens; the back-pointer word edge, with two waves of columns; five waves
ONE_PATH_XLENS = [65, 33, 32, 1]
ONE_PATH_CANDS = [(3, 0), (3, 5), (2, 4), (1, 64), (0, 300)]  # (utterance, U): (T_b, U) = (1, 0) (1, 5) (32, 4) (33, 64) (65, 300)
ONE_PATH_T, ONE_PATH_LMAX = 68, 302  # padding frames and padding columns, NaN there


def _one_path_lattice(g, Tb, U, T, Lmax):
    """(T, Lmax + 1, 2) f32 with exactly one finite path from (0, 0) to (T_b - 1, U): the planted path's own moves and the
    closing blank are multiples of 2^-6 in [-8, 0] (as `_exact_lattice` draws them), everything else inside (T_b, U) is
    -inf, everything outside NaN.  Returns (lat, tok_frame [U], the path's sum in float64)."""
    lat = torch.full((T, Lmax + 1, 2), float("nan"))
    lat[:Tb, : U + 1] = -math.inf
    tok_frame = sorted(torch.randint(0, Tb, (U,), generator=g).tolist())
    draw = iter((-torch.randint(0, 8 * 64 + 1, (Tb + U,), generator=g).to(torch.float64) / 64.0).tolist())
    total, u = 0.0, 0
    for t in range(Tb):
        while u < U and tok_frame[u] == t:
            lat[t, u, 1] = next(draw)
            total += float(lat[t, u, 1])
            u += 1
        lat[t, u, 0] = next(draw)  # the move to frame t + 1; at t == T_b - 1 the closing blank
        total += float(lat[t, u, 0])
    return lat, tok_frame, total


def test_one_finite_path_sum_and_max_agree_bit_for_bit():
    """On a lattice with ONE finite path the sum over paths and the maximum over paths are the same number: at most 65 + 300
    terms of at most 8 in multiples of 2^-6 - below 2^12, 18 bits - so every partial sum is exact in f32, and
    logaddexp(x, -inf) is x exactly (expf(-inf) = 0, log1pf(0) = 0).  So `total` of seq_align_device EQUALS the planted sum,
    seq_nll_device is its negation bit for bit, and the path is the planted one.  One ragged batch over mem_of, with
    padding frames and columns."""
    g = torch.Generator().manual_seed(4242)
    made = [_one_path_lattice(g, ONE_PATH_XLENS[m], U, ONE_PATH_T, ONE_PATH_LMAX) for m, U in ONE_PATH_CANDS]
    # the restatements first, on the CPU: the planted path and sum, and the sum's negation
    for (m, U), (lat, frames, want) in zip(ONE_PATH_CANDS, made):
        Tb = ONE_PATH_XLENS[m]
        ref = R.viterbi(lat, Tb, U)
        assert ref["tok_frame"] == frames and ref["total"] == want and math.isfinite(want), (Tb, U)
        assert R.forward_nll(lat, Tb, U) == -want, (Tb, U)
    jn = _jn()
    lat_dev = torch.stack([lat for lat, _, _ in made]).cuda()
    xl, yl, mo = _i32(ONE_PATH_XLENS), _i32([u for _, u in ONE_PATH_CANDS]), _i32([m for m, _ in ONE_PATH_CANDS])
    tok_frame, tok_logp, frame_u, total = (o.cpu() for o in jn.seq_align_device(lat_dev, xl, yl, mo))
    nll = jn.seq_nll_device(lat_dev, xl, yl, mo).cpu()
    for n, ((m, U), (lat, frames, want)) in enumerate(zip(ONE_PATH_CANDS, made)):
        Tb = ONE_PATH_XLENS[m]
        print(f"\none path {Tb} x {U}: planted {want!r}, total {float(total[n])!r}, nll {float(nll[n])!r}")
        assert float(total[n]) == want, (Tb, U)
        assert sf.bytes_equal(nll[n], -total[n]), (Tb, U)
        assert tok_frame[n, :U].tolist() == frames, (Tb, U)
        assert frame_u[n, :Tb].tolist() == [sum(1 for f in frames if f <= t) for t in range(Tb)], (Tb, U)
        assert tok_logp[n, :U].tolist() == [float(lat[f, u, 1]) for u, f in enumerate(frames)], (Tb, U)
        assert bool((tok_frame[n, U:] == -1).all()) and bool((tok_logp[n, U:] == 0).all()) and bool((frame_u[n, Tb:] == -1).all())


# ---------------------------------------------------------------------- a ragged batch
RAG_XLENS = [13, 0, 40]
RAG_CANDS = [(0, 5), (2, 12), (1, 3), (0, 0), (2, 0), (2, 7), (0, 12), (1, 0), (2, 1)]  # (utterance, U); utterance 1: no frame
RAG_T, RAG_LMAX = 41, 12
RAG_BLOCKED, RAG_SCATTER, RAG_DEAD_FRAME = 5, 1, 6


def _ragged():
    g = torch.Generator().manual_seed(77)
    lats = []
    for n, (m, U) in enumerate(RAG_CANDS):
        Tb = RAG_XLENS[m]
        lat = _exact_lattice(g, Tb, U, RAG_T, RAG_LMAX, k=4)
        if n == RAG_BLOCKED:
            lat[:Tb, 3, 1] = -math.inf  # label 3 can never be emitted: no path
        if n == RAG_DEAD_FRAME:
            lat[6, : U + 1] = -math.inf  # frame 6 neither emits nor moves on: no path
        if n == RAG_SCATTER:
            hit = torch.rand(Tb, U + 1, 2, generator=g) < 0.05
            hit[:, U, 0] = False  # (the closing blanks stay: a path remains)
            hit[:, :, 0] &= torch.arange(U + 1)[None, :] == U // 2  # blocked blanks in one column only
            lat[:Tb, : U + 1][hit] = -math.inf
        lats.append(lat)
    return torch.stack(lats)


def test_ragged_batch_and_rows_alone():
    jn = _jn()
    lat = _ragged()
    lat_dev = lat.cuda()
    xl, yl, mo = _i32(RAG_XLENS), _i32([u for _, u in RAG_CANDS]), _i32([m for m, _ in RAG_CANDS])
    got = [o.cpu() for o in jn.seq_align_device(lat_dev, xl, yl, mo)]
    n_inf = 0
    for n, (m, U) in enumerate(RAG_CANDS):
        Tb = RAG_XLENS[m]
        want = R.viterbi(lat[n], Tb, U)
        _assert_row_equals(got, n, want, Tb, U, n)
        if want["total"] == -math.inf:
            n_inf += 1
            assert bool((got[0][n] == -1).all()) and bool((got[1][n] == 0).all()) and bool((got[2][n] == -1).all())
    assert n_inf == 4 and math.isfinite(float(got[3][RAG_SCATTER]))  # utterance 1's two, the blocked label, the dead frame
    assert float(got[3][RAG_BLOCKED]) == -math.inf and float(got[3][RAG_DEAD_FRAME]) == -math.inf
    # every candidate alone: N = 1, its utterance its own, the same bytes - and in a narrower lattice (another Lmax,
    # another number of waves and another back-pointer stride) the same values
    for n, (m, U) in enumerate(RAG_CANDS):
        alone = [o.cpu() for o in jn.seq_align_device(lat_dev[n : n + 1], _i32([RAG_XLENS[m]]), _i32([U]))]
        for name, a, b in zip(NAMES, alone, got):
            assert sf.bytes_equal(a[0], b[n]), (n, name)
        narrow = lat_dev[n : n + 1, :, : U + 1].contiguous()
        alone = [o.cpu() for o in jn.seq_align_device(narrow, _i32([7, RAG_XLENS[m]]), _i32([U]), _i32([1]))]
        assert sf.bytes_equal(alone[0][0], got[0][n, :U]) and sf.bytes_equal(alone[1][0], got[1][n, :U]), n
        assert sf.bytes_equal(alone[2][0], got[2][n]) and sf.bytes_equal(alone[3][0], got[3][n]), n


# ---------------------------------------------------------------------- scratch independence
def test_outputs_do_not_depend_on_the_workspace_or_the_outputs_contents():
    """The workspace under ZERO / ONES / BIG / STALE, the outputs pre-filled: every output element is written and none
    depends on what the back-pointer store held.  STALE: the same entry point at a larger shape with other lattices."""
    import ctypes as C  # noqa: F401

    from espnet_amd import lib as L

    lib = L.load()
    lat = _ragged().cuda()
    N, T, Lmax = len(RAG_CANDS), RAG_T, RAG_LMAX
    xl, yl, mo = _i32(RAG_XLENS), _i32([u for _, u in RAG_CANDS]), _i32([m for m, _ in RAG_CANDS])
    # the larger call: 12 candidates of 70 frames x 45 tokens, all of them in use
    N2, T2, L2 = 12, 70, 45
    g = torch.Generator().manual_seed(78)
    big = torch.stack([_exact_lattice(g, T2, L2, T2, L2, k=5) for _ in range(N2)]).cuda()
    xl2, yl2 = _i32([T2] * N2), _i32([L2] * N2)
    need, need2 = (int(lib.em_transducer_seq_align_workspace_bytes(*s)) for s in ((N, T, Lmax), (N2, T2, L2)))
    assert 0 < need < need2
    ws = torch.empty(need2, dtype=torch.uint8, device="cuda")

    def launch(lat, xl, yl, mo, outs):
        n, t, lm = int(lat.shape[0]), int(lat.shape[1]), int(lat.shape[2]) - 1
        L.check(lib.em_transducer_seq_align(L.ptr(lat), L.ptr(xl), int(xl.numel()), t, lm, L.ptr(yl), L.ptr(mo), n,
                                            *(L.ptr(o) for o in outs), L.ptr(ws), int(ws.numel()), L.current_stream_ptr()),
                "em_transducer_seq_align")

    def make_outs(n, t, lm):
        return [torch.empty(n, lm, dtype=torch.int32, device="cuda"), torch.empty(n, lm, dtype=torch.float32, device="cuda"),
                torch.empty(n, t, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")]

    outs, outs2 = make_outs(N, T, Lmax), make_outs(N2, T2, L2)
    want_total = torch.tensor([R.viterbi(lat[n].cpu(), RAG_XLENS[m], U)["total"] for n, (m, U) in enumerate(RAG_CANDS)])
    ref = sf.assert_scratch_independent(lambda: launch(lat, xl, yl, mo, outs), ws, outs, None,
                                        stale=lambda: launch(big, xl2, yl2, None, outs2),
                                        finite=[None, None, None, torch.isfinite(want_total)], names=NAMES)
    assert torch.equal(ref[3], want_total.to(torch.float32))
    # a workspace one byte short, and a transcript above the cap
    with pytest.raises(L.EspnetAmdError, match="em_transducer_seq_align"):
        _jn().seq_align_device(lat, xl, yl, mo, ws=torch.empty(need - 256, dtype=torch.uint8, device="cuda"))
    cap = int(lib.em_transducer_seq_nll_max_tokens())
    assert int(lib.em_transducer_seq_align_workspace_bytes(1, 1, cap)) > 0
    assert int(lib.em_transducer_seq_align_workspace_bytes(1, 1, cap + 1)) == 0
    with pytest.raises(NotImplementedError):
        _jn().seq_align_device(torch.zeros(1, 1, cap + 2, 2, device="cuda"), _i32([1]), _i32([cap + 1]))


# ---------------------------------------------------------------------- model lattices
UNSCALED = TG.WALK_CELLS[0][:5]  # ("lstm", 1, 64, 64, 50): the first walk cell of tests/test_gpu_transducer.py, unscaled
MODEL_XLENS = [33, 20]
MODEL_CANDS = [(0, 0), (0, 1), (0, 9), (1, 4), (1, 19), (0, 40)]  # (utterance, U): N = 6 over 2 utterances


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", ["peaked", "unscaled"])
def test_device_path_is_the_optimum_of_the_device_lattice(cell, dtype):
    """The chain teacher_forced_proj -> lattice_logp_device -> seq_align_device.  On the device's own lattice, read back:
    the device's path re-scored in float64 lies within (T_b + U) * 2^-23 * max(1, |total|) of the float64 optimum - the
    f32 rounding of a sum of T_b + U terms, each add within 2^-24 relative to a partial sum that |total| bounds, twice
    for the two paths compared (derived, not measured) - `total` lies within the same bound of that re-score, and
    total <= log p(y | x) + bound with the likelihood from seq_nll_device on the same lattice."""
    if cell == "peaked":
        model, p, _, _ = TG._model(*TG.PEAKED, dtype, 51, out_scale=TG.PEAK_SCALE)
    else:
        model, p, _, _ = TG._model(*UNSCALED, dtype, TG.WALK_SEEDS[TG.WALK_CELLS[0]][0])
    dec, jn = model.decoder, model.joint_network
    V = p.out_w.shape[0]
    N, T, Lmax = len(MODEL_CANDS), max(MODEL_XLENS), max(u for _, u in MODEL_CANDS)
    targets = torch.randint(1, V, (N, Lmax), generator=torch.Generator().manual_seed(85))
    ylens, mem_of = [u for _, u in MODEL_CANDS], [m for m, _ in MODEL_CANDS]
    enc_dev, _ = TG._enc(86, (len(MODEL_XLENS), T, TG.D), dtype)
    enc_proj = jn.enc_proj_device(enc_dev)
    dec_proj = dec.teacher_forced_proj(targets, torch.tensor(ylens))
    xl, yl, mo = _i32(MODEL_XLENS), _i32(ylens), _i32(mem_of)
    lat = jn.lattice_logp_device(dec, enc_proj, xl, dec_proj, targets.to(torch.int32).cuda(), yl, mo)
    tok_frame, tok_logp, frame_u, total = (o.cpu() for o in jn.seq_align_device(lat, xl, yl, mo))
    nll = jn.seq_nll_device(lat, xl, yl, mo).cpu()
    lat64 = lat.cpu().to(torch.float64)
    worst = 0.0
    for n, (m, U) in enumerate(MODEL_CANDS):
        Tb = MODEL_XLENS[m]
        frames = tok_frame[n, :U].tolist()
        assert frames == sorted(frames) and all(0 <= f < Tb for f in frames), n
        assert frame_u[n, :Tb].tolist() == [sum(1 for f in frames if f <= t) for t in range(Tb)], n
        assert torch.equal(tok_logp[n, :U], lat[n].cpu()[frames, list(range(U)), 1]) if U else True
        assert bool((tok_frame[n, U:] == -1).all()) and bool((tok_logp[n, U:] == 0).all()) and bool((frame_u[n, Tb:] == -1).all())
        rescored = R.path_value(lat64[n], Tb, U, frames)
        best = R.viterbi(lat64[n], Tb, U)["total"]
        tot = float(total[n])
        bound = (Tb + U) * 2.0 ** -23 * max(1.0, abs(tot))
        print(f"\n{cell} {dtype} candidate {n} ({Tb} x {U}): total {tot:.6f}, re-scored {rescored:.6f}, optimum {best:.6f}, "
              f"-nll {-float(nll[n]):.6f}, bound {bound:.3e}")
        assert math.isfinite(tot) and rescored <= best + 1e-12
        assert best - rescored <= bound, n
        assert abs(tot - rescored) <= bound, n
        assert tot <= -float(nll[n]) + bound, n
        worst = max(worst, (best - rescored) / bound, abs(tot - rescored) / bound)
    print(f"\n{cell} {dtype}: largest share of the bound used {worst:.3f}")
    # the model's method on the same candidates: the same bytes
    ys = targets.clone()
    outs = model.transducer_align(enc_dev, torch.tensor(MODEL_XLENS), ys, torch.tensor(ylens), mem_of=mem_of)
    for name, a, b in zip(NAMES, outs, (tok_frame, tok_logp, frame_u, total)):
        assert a.is_cuda and sf.bytes_equal(a.cpu(), b), name


# ---------------------------------------------------------------------- the public interface
def _assert_floats_on_own_encoding(p, enc_act, r, spf, dtype, tag):
    """The floats of one result of `batch_transducer_align` against the float64 restatement of the whole chain (lin_enc,
    the teacher-forced prediction network, the joint network's log-softmax; tests/transducer_nll_ref.py) on the encoder
    output enc_act (T_b, D) that the device made for that call: every token's logp within E of the restatement's
    log-probability at its node, and `total` within (T_b + U) * (E + 2^-23 * max(1, |total|)) of the restatement's value of
    the same path.  E = E_LOGP_PEAKED of tests/test_gpu_transducer.py: the suite's bound of a log-softmax row of this
    model against float64 on the same inputs, the prediction network's and lin_enc's rounding included; a path has
    T_b + U such terms, added in f32 (each add within 2^-24 of a partial sum that |total| bounds; twice that is taken).
    Returns the restatement's value of the path and the bound on `total`."""
    y = r["token_int"]
    enc64 = enc_act.cpu().to(torch.float64)
    Tb, U = int(enc64.shape[0]), len(y)
    frames = [int(round(t[2] / spf)) for t in r["tokens"]]
    lat = R.lattice(p, enc64 @ p.enc_w.T + p.enc_b, R.teacher_forced_dec_out(p, y) @ p.dec_w.T, y,
                    round_z=dtype == "bfloat16")
    E = TG.E_LOGP_PEAKED[dtype]
    d_tok = max([abs(t[4] - float(lat[f, u, 1])) for u, (f, t) in enumerate(zip(frames, r["tokens"]))], default=0.0)
    want = R.path_value(lat, Tb, U, frames)
    bound = (Tb + U) * (E + 2.0 ** -23 * max(1.0, abs(r["total"])))
    print(f"\n[{tag}] against float64 on its own encoder output: a token's logp off by up to {d_tok:.3e} (bound {E:.3e}), "
          f"total {r['total']:.6f} against {want:.6f} (bound {bound:.3e})")
    assert d_tok <= E, (tag, d_tok)
    assert abs(r["total"] - want) <= bound, (tag, r["total"], want)
    return want, bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_interface_on_the_peaked_model(tmp_path, dtype):
    """Speech2Text.batch_transducer_align / transducer_align on the peaked tiny Conformer transducer (weights seed 51,
    waveforms PEAKED_WAVES ..): texts=None aligns the greedy hypothesis of batch_decode."""
    s2t, p = TG._speech2text(tmp_path, dtype)
    lens = [5000, 3000, 4000]
    speech = TG._waves(lens, TG.PEAKED_WAVES)
    greedy = [r[0][2] for r in s2t.batch_decode(speech, lens)]
    res = s2t.batch_transducer_align(speech, lens)
    st = s2t.asr_model.encode_device(speech.cuda(), lens, isolate=True)
    spf = s2t.seconds_per_frame
    assert spf == 4 * 160 / 16000
    for b, r in enumerate(res):
        assert r["token_int"] == greedy[b] and [t[1] for t in r["tokens"]] == greedy[b]
        assert [t[0] for t in r["tokens"]] == s2t.converter.ids2tokens(greedy[b])
        Tb, U = st.olens[b], len(greedy[b])
        assert r["frame_u"].dtype == torch.int64 and tuple(r["frame_u"].shape) == (Tb,)
        frames = [int(round(t[2] / spf)) for t in r["tokens"]]
        assert len(frames) == U and frames == sorted(frames) and all(0 <= f < Tb for f in frames)
        for f, (_, _, start, end, lp) in zip(frames, r["tokens"]):
            assert start == f * spf and end == (f + 1) * spf and abs((end - start) - spf) <= 1e-12
            assert lp <= 0.0 and math.isfinite(lp)
        assert r["frame_u"].tolist() == [sum(1 for f in frames if f <= t) for t in range(Tb)]
        assert math.isfinite(r["total"]) and r["total"] < 0.0
        print(f"\npublic {dtype} utt {b}: {U} tokens over {Tb} frames at {frames}, total {r['total']:.4f}")
    assert sum(len(g) for g in greedy) > 0
    # the same ids as given transcripts: another Lmax (the longest transcript, not T), bit for bit the same result
    given = s2t.batch_transducer_align(speech, lens, texts=greedy)
    for a, b in zip(given, res):
        assert a["tokens"] == b["tokens"] and a["token_int"] == b["token_int"] and a["total"] == b["total"]
        assert torch.equal(a["frame_u"], b["frame_u"])
    # one utterance alone against its batch row.  Everything discrete is equal: tokens, ids, times, frame_u.  The floats
    # are held to what the two calls were given: each result - the batch row's and the lone call's - against the float64
    # restatement of the whole chain on the encoder output the device made for THAT call (`_assert_floats_on_own_encoding`),
    # and where the two encoder outputs are the same bits (the longest row: the same launch shapes but for the batch
    # size) the two results are equal bit for bit.  They are not compared with each other beyond that: on this fixture
    # the encoder outputs of a short row alone and inside the ragged batch differ by up to 6.7e-2 (f32 and bf16 alike;
    # the features are bit-identical, and in f32 either encoding lies 0.06-0.12 from the CPU oracle's at |enc| <= 3.3: the
    # one-block fixture's encoder amplifies the summation order of the launch shape), lin_out x 40 turns that into tenths
    # of a unit on the blanks (total 0.44 apart at -105.6), and no test of the suite bounds two encodings against each
    # other for this model.  With both results inside their bounds the difference of the totals is at most the
    # difference of the two restatements plus both bounds, which is asserted as well.
    same_bits = 0
    for b, n in enumerate(lens):
        one = s2t.transducer_align(speech[b, :n].numpy())
        assert one["token_int"] == res[b]["token_int"] and torch.equal(one["frame_u"], res[b]["frame_u"])
        assert [t[:4] for t in one["tokens"]] == [t[:4] for t in res[b]["tokens"]]
        st1 = s2t.asr_model.encode_device(speech[b : b + 1, :n].cuda(), [n], isolate=True)
        enc_row, enc_one = st.enc_act[b, : st.olens[b]], st1.enc_act[0, : st1.olens[0]]
        ref_row, bound_row = _assert_floats_on_own_encoding(p, enc_row, res[b], spf, dtype, f"{dtype} batch row {b}")
        ref_one, bound_one = _assert_floats_on_own_encoding(p, enc_one, one, spf, dtype, f"{dtype} utt {b} alone")
        d_tot = abs(one["total"] - res[b]["total"])
        assert d_tot <= abs(ref_one - ref_row) + bound_one + bound_row
        if torch.equal(enc_row, enc_one):
            same_bits += 1
            assert one["tokens"] == res[b]["tokens"] and one["total"] == res[b]["total"]
        d_enc = float((enc_one.float() - enc_row.float()).abs().max())
        d_tok = max([abs(x[4] - y[4]) for x, y in zip(one["tokens"], res[b]["tokens"])], default=0.0)
        print(f"\npublic {dtype} utt {b} alone against its batch row: encoder output differs by up to {d_enc:.3e}, a token's "
              f"logp by up to {d_tok:.3e}, total by {d_tot:.3e} (the restatements by {abs(ref_one - ref_row):.3e})")
    assert same_bits >= 1  # (the longest row)
    # an object built with a beam still aligns the greedy walk's hypothesis
    s2t_beam, _ = TG._speech2text(tmp_path, dtype, beam_size=3)
    assert [r["token_int"] for r in s2t_beam.batch_transducer_align(speech, lens)] == greedy


def test_refusals_of_the_public_interface(tmp_path):
    import yaml

    from espnet_amd.bin.asr_inference import Speech2Text

    s2t, _ = TG._speech2text(tmp_path, "float32")
    speech = TG._waves([3000])
    with pytest.raises(ValueError, match="<blank>"):
        s2t.batch_transducer_align(speech, [3000], [[1, 0]])
    with pytest.raises(ValueError, match="transcripts"):
        s2t.batch_transducer_align(speech, [3000], [[1], [2]])
    cfg = yaml.safe_load((tmp_path / "config.yaml").read_text())
    # ctc_weight: 0, the usual setting of a transducer recipe: the CTC route still refuses, this one aligns
    cfg0 = dict(cfg, model_conf=dict(ctc_weight=0.0))
    (tmp_path / "noctc.yaml").write_text(yaml.safe_dump(cfg0))
    noctc = Speech2Text(str(tmp_path / "noctc.yaml"), None, device="cuda")
    with pytest.raises(ValueError, match="forced alignment needs a CTC head"):
        noctc.batch_align(speech, [3000], [[1]])
    r = noctc.batch_transducer_align(speech, [3000], [[1, 2]])[0]
    assert r["token_int"] == [1, 2] and len(r["tokens"]) == 2 and math.isfinite(r["total"])
    # a model with a CTC head and no joint network
    cfg.update(decoder="transformer", decoder_conf=dict(attention_heads=1, linear_units=64, num_blocks=1))
    cfg.pop("joint_net_conf")
    (tmp_path / "att.yaml").write_text(yaml.safe_dump(cfg))
    att = Speech2Text(str(tmp_path / "att.yaml"), None, device="cuda")
    with pytest.raises(RuntimeError, match="batch_align"):
        att.batch_transducer_align(speech, [3000], [[1]])
    with pytest.raises(RuntimeError, match="joint network"):
        att.asr_model.transducer_align(torch.zeros(1, 2, TG.D, device="cuda"), torch.tensor([2]), torch.ones(1, 1), torch.tensor([1]))
