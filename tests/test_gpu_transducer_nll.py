"""Transducer likelihood of given transcripts on the MI355X (csrc/transducer_nll.hip) through the C ABI's wrappers and the
host layer, against the float64 restatement of the contract (tests/transducer_nll_ref.py) on the SAME inputs: the
recursion on synthetic f32 lattices, the lattice launch on the device's own enc_proj / dec_proj read back (so that only
the new kernel is under test), the whole chain from the device's own encoder output.

Models, encoder rows and waveforms are those of tests/test_gpu_transducer.py (`_model`, `_enc`, `_speech2text`, `_waves`),
the seeds named in each test.  Bounds follow that file's convention: 4 x the largest error the first MI355X run printed
(profiles/transducer_nll_pytest_gpu_first.txt, seen values in brackets; the final tree's run is
profiles/transducer_nll_pytest_gpu.txt - the bf16 lattice figures moved in the third digit with the kernel's column order):
    recursion  relative to max(1, |nll|)           f32 lattice in, f32 out    E_SEQ    4 x [2.314e-07]
    lattice    absolute, a node's log-probability  f32 4 x [1.477e-06]   bf16 4 x [1.398e-06]     E_LAT
    chain      relative to max(1, |nll|), peaked   f32 4 x [1.615e-07]   bf16 4 x [2.495e-04]     E_CHAIN
    chain      the same, the V = 5 recipe model    f32 4 x [1.513e-07]   bf16 4 x [5.949e-05]     E_CHAIN_FLAT
f32 stays at accumulation-order noise on the lattice and the recursion's error is that of ~T_b + U rounded additions.
bf16 on the lattice came out at the same noise: the restatement rounds z as the device does, and in none of the cells
did a z element's f32 tanh fall on the other side of a bf16 rounding boundary than the float64 tanh (such a flip would
show as ~1e-4); in the chain the bf16 error is the prediction network's output and lin_enc / lin_dec, rounded on the device
and exact in the restatement.
"""
import math

import numpy as np
import pytest
import torch

from tests import test_gpu_transducer as TG
from tests import transducer_nll_ref as R

pytestmark = pytest.mark.gpu

DTYPES = TG.DTYPES
E_SEQ = 4 * 2.314e-07
E_LAT = {"float32": 4 * 1.477e-06, "bfloat16": 4 * 1.398e-06}
E_CHAIN = {"float32": 4 * 1.615e-07, "bfloat16": 4 * 2.495e-04}
E_CHAIN_FLAT = {"float32": 4 * 1.513e-07, "bfloat16": 4 * 5.949e-05}
SENTINEL = 12345.0


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


# ---------------------------------------------------------------------- the recursion alone
SEQ_CASES = [(1, 0), (1, 3), (7, 0), (5, 1), (33, 63), (33, 64), (9, 70), (40, 130), (0, 2)]  # (T_b, U); T_b = 0: +inf


def _synthetic(T, Lmax):
    """One lattice per case, f32 log-probabilities in (-5, 0], NaN outside (T_b, U); -inf entries: a blocked column in
    the (33, 63) case, an all -inf frame in the (9, 70) case, scattered ones in (33, 64) and (40, 130)."""
    g = torch.Generator().manual_seed(91)
    lats = []
    for Tb, U in SEQ_CASES:
        lat = torch.full((T, Lmax + 1, 2), float("nan"))
        lat[:Tb, : U + 1] = -5.0 * torch.rand(Tb, U + 1, 2, generator=g)
        if Tb:
            lat[:Tb, U, 1] = -math.inf
        if (Tb, U) == (33, 63):
            lat[:Tb, 10, 1] = -math.inf
        if (Tb, U) == (9, 70):
            lat[4, : U + 1] = -math.inf
        if (Tb, U) in ((33, 64), (40, 130)):
            hit = torch.rand(Tb, U + 1, 2, generator=g) < 0.05
            lat[:Tb, : U + 1][hit] = -math.inf
        lats.append(lat)
    return lats


def test_recursion_on_synthetic_lattices():
    from espnet_amd.asr.transducer.joint_network import JointNetwork

    jn = JointNetwork(8, 64, 64, 64)
    T, Lmax = 41, 130  # xlens shorter than T everywhere
    lats = _synthetic(T, Lmax)
    xl, yl = [c[0] for c in SEQ_CASES], [c[1] for c in SEQ_CASES]
    got = jn.seq_nll_device(torch.stack(lats).cuda(), _i32(xl), _i32(yl)).cpu()
    want = [R.forward_nll(lat, Tb, U) for lat, (Tb, U) in zip(lats, SEQ_CASES)]
    err, n_inf = 0.0, 0
    for g, w, c in zip(got.tolist(), want, SEQ_CASES):
        if math.isinf(w):
            assert g == math.inf, (c, g)
            n_inf += 1
        else:
            assert math.isfinite(g), (c, g)
            err = max(err, _rel(g, w))
    print(f"\nrecursion: {len(SEQ_CASES)} lattices, {n_inf} without a path, largest relative error {err:.3e}")
    assert n_inf == 3 and math.isinf(want[4]) and math.isinf(want[6]) and math.isinf(want[8])
    assert err <= E_SEQ
    # the same candidates in another order, in a wider array (another Lmax, so another number of waves), with the
    # lengths shared through mem_of: bit for bit the same values
    order = [7, 2, 5, 0, 8, 4, 1, 6, 3]
    Lmax2 = 200
    wide = torch.full((len(order), T, Lmax2 + 1, 2), float("nan"))
    for i, k in enumerate(order):
        wide[i, :, : Lmax + 1] = lats[k]
    uniq = sorted(set(xl))
    got2 = jn.seq_nll_device(wide.cuda(), _i32(uniq), _i32([yl[k] for k in order]),
                             mem_of=_i32([uniq.index(xl[k]) for k in order])).cpu()
    assert torch.equal(got2, got[order])


# ---------------------------------------------------------------------- the lattice launch alone
LAT_CELLS = [(37, 40), (530, 128), (1027, 64)]  # (V, J): V not a multiple of 16, several vocabulary tiles per wave, jp padding
LAT_XLENS = [33, 7, 1]
LAT_CANDS = [(0, 20), (0, 0), (1, 5), (1, 1), (2, 20), (2, 0), (0, 5)]  # (utterance, U): 1 002 nodes, 15 full tiles + 42 rows
_lat_cache = {}


def _lattice_case(cell, dtype):
    """The launch and its float64 restatement, computed once per (cell, dtype) and shared."""
    key = (cell, dtype)
    if key not in _lat_cache:
        V, J = cell
        model, p, _, _ = TG._model("lstm", 1, 64, J, V, dtype, 81)
        dec, jn = model.decoder, model.joint_network
        N, T, Lmax = len(LAT_CANDS), max(LAT_XLENS), max(u for _, u in LAT_CANDS)
        g = torch.Generator().manual_seed(82)
        targets = torch.randint(1, V, (N, Lmax), generator=g)
        ylens = [u for _, u in LAT_CANDS]
        mem_of = [m for m, _ in LAT_CANDS]
        enc_dev, _ = TG._enc(83, (len(LAT_XLENS), T, TG.D), dtype)
        enc_proj = jn.enc_proj_device(enc_dev)
        dec_proj = dec.teacher_forced_proj(targets, torch.tensor(ylens))
        tg_dev = targets.to(torch.int32).cuda()
        lat = torch.full((N, T, Lmax + 1, 2), SENTINEL, device="cuda")
        jn.lattice_logp_device(dec, enc_proj, _i32(LAT_XLENS), dec_proj, tg_dev, _i32(ylens), _i32(mem_of), out=lat)
        ep, dp = enc_proj.cpu(), dec_proj.cpu()
        want = [R.lattice(p, ep[m], dp[:, n], targets[n, :U].tolist(), LAT_XLENS[m], U, round_z=dtype == "bfloat16")
                for n, (m, U) in enumerate(LAT_CANDS)]
        _lat_cache[key] = dict(model=model, p=p, enc_proj=enc_proj, dec_proj=dec_proj, targets=targets, tg_dev=tg_dev,
                               ylens=ylens, mem_of=mem_of, lat=lat, want=want, N=N, T=T, Lmax=Lmax)
    return _lat_cache[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", LAT_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_lattice_against_float64(cell, dtype):
    c = _lattice_case(cell, dtype)
    assert sum(LAT_XLENS[m] * (U + 1) for m, U in LAT_CANDS) % 64 != 0
    lat = c["lat"].cpu().to(torch.float64).numpy()
    err = 0.0
    for n, (m, U) in enumerate(LAT_CANDS):
        Tb, w = LAT_XLENS[m], c["want"][n]
        got = lat[n, :Tb, : U + 1]
        assert np.all(np.isneginf(got[:, U, 1]))  # no label beyond the transcript
        fin = np.isfinite(w)
        assert np.all(np.isfinite(got[fin])) and np.all(got[fin] <= 0.0)
        err = max(err, float(np.abs(got[fin] - w[fin]).max()))
        # nodes outside (T_b, U) keep what the test wrote there
        assert np.all(lat[n, Tb:] == SENTINEL) and np.all(lat[n, :, U + 1:] == SENTINEL)
    print(f"\nlattice V {cell[0]} J {cell[1]} {dtype}: largest error of a node's log-probability {err:.3e}")
    assert err <= E_LAT[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", LAT_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_lattice_agrees_with_joint_logp(cell, dtype):
    """em_transducer_joint_logp on the same (t, u) pairs: the two values of a node within the sum of both bounds."""
    c = _lattice_case(cell, dtype)
    model, N, T, Lmax = c["model"], c["N"], c["T"], c["Lmax"]
    nodes = [(n, t, u) for n, (m, U) in enumerate(LAT_CANDS) for t in range(LAT_XLENS[m]) for u in range(U + 1)]
    pick = torch.randperm(len(nodes), generator=torch.Generator().manual_seed(84))[:100].tolist()
    nodes = [nodes[i] for i in pick]
    jp = c["enc_proj"].shape[-1]
    logp = model.joint_network.logp_device(model.decoder, c["enc_proj"].view(-1, jp), c["dec_proj"].view(-1, jp),
                                           _i32([c["mem_of"][n] * T + t for n, t, u in nodes]),
                                           _i32([u * N + n for n, t, u in nodes])).cpu()
    lat = c["lat"].cpu()
    bound = E_LAT[dtype] + TG.E_LOGP[dtype]
    worst = 0.0
    for i, (n, t, u) in enumerate(nodes):
        worst = max(worst, abs(float(lat[n, t, u, 0]) - float(logp[i, 0])))
        if u < c["ylens"][n]:
            worst = max(worst, abs(float(lat[n, t, u, 1]) - float(logp[i, int(c["targets"][n, u])])))
    print(f"\nlattice vs joint_logp V {cell[0]} J {cell[1]} {dtype}: largest difference {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", LAT_CELLS, ids=lambda c: "-".join(map(str, c)))
def test_lattice_values_do_not_depend_on_the_batch(cell, dtype):
    """Fewer candidates in another order (other tiles, other row slots), a larger Lmax, and replicated utterances in
    place of mem_of: every node bit for bit."""
    c = _lattice_case(cell, dtype)
    model, T, Lmax = c["model"], c["T"], c["Lmax"]
    order = [4, 0, 6, 3, 1]
    Lmax2 = Lmax + 5
    N2 = len(order)
    dec_proj2 = torch.zeros(Lmax2 + 1, N2, c["dec_proj"].shape[-1], device="cuda")
    dec_proj2[: Lmax + 1] = c["dec_proj"][:, order]
    targets2 = torch.ones(N2, Lmax2, dtype=torch.int32)
    targets2[:, :Lmax] = c["targets"][order].to(torch.int32)
    enc_rep = c["enc_proj"][[c["mem_of"][k] for k in order]].contiguous()  # candidate n owns utterance n
    lat2 = torch.full((N2, T, Lmax2 + 1, 2), SENTINEL, device="cuda")
    model.joint_network.lattice_logp_device(model.decoder, enc_rep, _i32([LAT_XLENS[c["mem_of"][k]] for k in order]),
                                            dec_proj2, targets2.cuda(), _i32([c["ylens"][k] for k in order]), None, out=lat2)
    for i, k in enumerate(order):
        Tb, U = LAT_XLENS[c["mem_of"][k]], c["ylens"][k]
        assert torch.equal(lat2[i, :Tb, : U + 1], c["lat"][k, :Tb, : U + 1]), (i, k)
        assert bool((lat2[i, Tb:] == SENTINEL).all()) and bool((lat2[i, :, U + 1:] == SENTINEL).all())


# ---------------------------------------------------------------------- the whole chain
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_chain_through_the_public_interface(tmp_path, dtype):
    """Speech2Text.batch_transducer_nll and ESPnetASRModel.transducer_nll on the peaked tiny model (weights seed 51,
    waveforms PEAKED_WAVES ..) against the restatement run from the device's own encoder output.  Candidates per
    utterance: empty, one token, the model's own greedy hypothesis, a random one."""
    s2t, p = TG._speech2text(tmp_path, dtype)
    m = s2t.asr_model
    lens = [5000, 3000, 4000]
    speech = TG._waves(lens, TG.PEAKED_WAVES)
    greedy = [r[0][2] for r in s2t.batch_decode(speech, lens)]
    g = torch.Generator().manual_seed(92)
    texts = [[[], [int(torch.randint(1, 49, (1,), generator=g))], greedy[b],
              torch.randint(1, 49, (4,), generator=g).tolist()] for b in range(len(lens))]
    got = s2t.batch_transducer_nll(speech, lens, texts)
    st = m.encode_device(speech.cuda(), lens, isolate=True)
    enc64 = st.enc_act.cpu().to(torch.float64)
    err = 0.0
    for b in range(len(lens)):
        assert len(got[b]) == 4
        for y, v in zip(texts[b], got[b]):
            want = R.model_nll(p, enc64[b, : st.olens[b]], y, round_z=dtype == "bfloat16")
            assert math.isfinite(v) and v > 0.0
            err = max(err, _rel(v, want))
    print(f"\nchain {dtype}: 12 candidates, largest relative error of nll {err:.3e}")
    assert err <= E_CHAIN[dtype]
    # the slicing path: three candidates per call, bit for bit the unsliced values
    s2t.nll_rows_per_call = 3
    assert s2t.batch_transducer_nll(speech, lens, texts) == got
    # the model's method on the same candidates, and one transcript per utterance without mem_of
    flat = [y for group in texts for y in group]
    ys = torch.zeros(len(flat), max(len(y) for y in flat), dtype=torch.long)
    for i, y in enumerate(flat):
        ys[i, : len(y)] = torch.tensor(y, dtype=torch.long)
    ylens = torch.tensor([len(y) for y in flat])
    olens = torch.tensor(st.olens)
    vals = m.transducer_nll(st.enc_act, olens, ys, ylens, mem_of=[b for b in range(len(lens)) for _ in range(4)])
    assert vals.is_cuda and vals.dtype == torch.float32 and vals.cpu().tolist() == [v for group in got for v in group]
    own = m.batchify_transducer_nll(st.enc_act, olens, ys[2::4], ylens[2::4], batch_size=2).cpu().tolist()
    assert own == [got[b][2] for b in range(len(lens))]
    with pytest.raises(ValueError, match="<blank>"):
        s2t.batch_transducer_nll(speech, lens, [[1, 0], [1], [1]])
    # the other scorers keep refusing a transducer model
    with pytest.raises(RuntimeError, match="transducer"):
        s2t.batch_nll(speech, lens, [[1], [1], [1]])
    with pytest.raises(RuntimeError, match="transducer"):
        s2t.batch_rescore(speech, lens, [[1], [1], [1]])
    with pytest.raises(NotImplementedError):
        m.joint_network(st.enc_out, st.enc_out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_probabilities_of_all_short_transcripts_stay_below_one(dtype):
    """V = 5 (recipe weights seed 95, encoder rows seed 96, 3 frames): the 1 + 4 + 16 transcripts of at most two labels
    are disjoint events, so their probabilities sum to at most 1 - on the device and in the restatement."""
    model, p, _, _ = TG._model("lstm", 1, 64, 64, 5, dtype, 95)
    enc_dev, enc64 = TG._enc(96, (1, 3, TG.D), dtype)
    cands = [[]] + [[a] for a in range(1, 5)] + [[a, b] for a in range(1, 5) for b in range(1, 5)]
    ys = torch.zeros(len(cands), 2, dtype=torch.long)
    for i, y in enumerate(cands):
        ys[i, : len(y)] = torch.tensor(y, dtype=torch.long)
    got = model.transducer_nll(enc_dev, torch.tensor([3]), ys, torch.tensor([len(y) for y in cands]),
                               mem_of=[0] * len(cands)).cpu().tolist()
    want = [R.model_nll(p, enc64[0], y, round_z=dtype == "bfloat16") for y in cands]
    err = max(_rel(g, w) for g, w in zip(got, want))
    tot_dev, tot_ref = sum(math.exp(-v) for v in got), sum(math.exp(-v) for v in want)
    print(f"\nshort transcripts {dtype}: sum of probabilities device {tot_dev:.6f} restatement {tot_ref:.6f}, "
          f"largest relative error of nll {err:.3e}")
    assert 0.0 < tot_dev <= 1.0 and 0.0 < tot_ref <= 1.0
    assert err <= E_CHAIN_FLAT[dtype]


# ---------------------------------------------------------------------- limits
def test_limits(tmp_path):
    import yaml

    from espnet_amd import lib as L
    from espnet_amd.bin.asr_inference import Speech2Text

    cap = int(L.load().em_transducer_seq_nll_max_tokens())
    assert cap >= 1023
    model, p, _, _ = TG._model("lstm", 1, 64, 64, 37, "float32", 81)
    dec, jn = model.decoder, model.joint_network
    # one token above the cap: the recursion, the lattice and the model's method all say so
    with pytest.raises(NotImplementedError):
        jn.seq_nll_device(torch.zeros(1, 1, cap + 2, 2, device="cuda"), _i32([1]), _i32([cap + 1]))
    assert jn.lattice_workspace_bytes(dec, "cuda", 1, 1, cap) > 0 and jn.lattice_workspace_bytes(dec, "cuda", 1, 1, cap + 1) == 0
    enc_dev, _ = TG._enc(83, (1, 2, TG.D), "float32")
    with pytest.raises(NotImplementedError, match=str(cap)):
        model.transducer_nll(enc_dev, torch.tensor([2]), torch.ones(1, cap + 1, dtype=torch.long), torch.tensor([cap + 1]))
    # exactly at the cap the recursion runs (a lattice of log(1/2) everywhere: 2 frames, cap labels)
    lat = torch.full((1, 2, cap + 1, 2), math.log(0.5), device="cuda")
    lat[:, :, cap, 1] = -math.inf
    v = float(jn.seq_nll_device(lat, _i32([2]), _i32([cap])).cpu())
    want = R.forward_nll(lat[0].cpu(), 2, cap)
    # (per diagonal two rounded additions and one log1p(exp()) of a few ulp, each relative to |alpha| <= |nll|: at most
    # 4 x 2^-24 per diagonal along the cap + 2 diagonals - from the number format, not from a run)
    assert _rel(v, want) <= (cap + 2) * 4 * 2.0 ** -24
    # a workspace that is too small
    enc_proj = jn.enc_proj_device(enc_dev)
    dec_proj = dec.teacher_forced_proj(torch.ones(1, 1, dtype=torch.long), torch.tensor([1]))
    with pytest.raises(L.EspnetAmdError, match="em_transducer_lattice_logp"):
        jn.lattice_logp_device(dec, enc_proj, _i32([2]), dec_proj, _i32([[1]]), _i32([1]),
                               ws=torch.empty(4, dtype=torch.uint8, device="cuda"))
    # a model without a joint network
    TG._speech2text(tmp_path, "float32")
    cfg = yaml.safe_load((tmp_path / "config.yaml").read_text())
    cfg.update(decoder="transformer", decoder_conf=dict(attention_heads=1, linear_units=64, num_blocks=1))
    cfg.pop("joint_net_conf")
    (tmp_path / "att.yaml").write_text(yaml.safe_dump(cfg))
    att = Speech2Text(str(tmp_path / "att.yaml"), None, device="cuda")
    with pytest.raises(RuntimeError, match="joint network"):
        att.batch_transducer_nll(torch.zeros(1, 3000), [3000], [[1]])
    with pytest.raises(RuntimeError, match="joint network"):
        att.asr_model.transducer_nll(torch.zeros(1, 2, TG.D, device="cuda"), torch.tensor([2]), torch.ones(1, 1), torch.tensor([1]))
