"""Per-element float64 parity of the decoder step kernels (csrc/decoder.hip), through the C ABI:

  em_dec_self_attention        f32, bf16   dec_self_attn_kernel: d_k 64 / 32, ESPNET_AMD_SA_SPLIT automatic / 1 / 2 / 4, a
                                           partial last row group, tok_tab (id-0 keys masked), pos_dev + anc_odd
  em_dec_self_attention_beam   bf16        dec_self_attn_tree_kernel<5 | 10 | 16>, and the per-row kernel on the same cases
                                           (ESPNET_AMD_NO_SA_TREE=1); em_dec_self_attention_beam_route says which one ran
  em_dec_src_attention         f32, bf16   dec_src_attn_kernel, d_k 64 / 32; em_dec_transpose_v exact, padding included
  em_dec_src_attention_lnq, _lnq_frag      bit-equal to em_ln_gemm + em_dec_src_attention, which is inside the budget
  em_dec_embed_f32, em_lm_embed, em_lm_input_norm_f32

Reference, inputs, case lists and the one tolerance are tests/dec_step_ref.py (the budget is tests/attention_ref.py's):
|got - ref| <= 3 u A + f (1 + S) A per element for bf16, f (1 + S) A for f32, exactly zero where no visible key reaches the
channel.  Everything a kernel must not read (cache positions from pos on, cache rows no ancestor names, the ancestor table
of the other step parity, memory frames behind klens[b]) holds +-8 in every channel.  tests/test_cpu_dec_step_ref.py shows
that a dropped key, a key from another slot, klens off by one, an unmasked id-0 key and the wrong table each break the budget
in every case.  Every self-attention case also checks the caches bit for bit: kc[pos] / vc[pos] are the new K / V and every
other element, on both sides of pos, is unchanged.

The worst err / budget per route is printed when the module ends (`PARITY SUMMARY`).  Measured on an MI355X (the CPU
simulations reach 0.34 for the per-row form and 0.68 for rounded probabilities, dec_step_ref.SIM_*_BF16_MAX; no route needed
a rounding point added to the reference and no kernel was found wrong):
  em_dec_self_attention              f32 0.072 (d_k 32, pos 1, split 4, sharp)    bf16 0.326 (d_k 64, pos 31, split 4, sharp)
    tok_tab                          f32 0.071 (d_k 64, pos 65, sharp)            bf16 0.328 (d_k 64, pos 65, sharp)
    pos_dev                          f32 0.050 (d_k 32, position 129, sharp)      bf16 0.326 (d_k 64, position 129, flat)
  em_dec_self_attention_beam         tree 0.651, per-row 0.330 (both W = 5, one shared path, pos 61, sharp)
  em_dec_src_attention               f32 0.190, bf16 0.672 (both d_k 64, T = 31, W = 20, sharp)
  em_ln_gemm + em_dec_src_attention  0.636 (d = 512, T = 16, W = 33); lnq and lnq_frag bit-equal to it in every case
  em_dec_embed_f32                   0.74 of 2^-24 (2 |e| sqrt(d) + |x|);  em_lm_embed exact
  em_lm_input_norm_f32               0.11 of the operation-count bound (d = 200)
"""
import contextlib
import os

import pytest
import torch

from espnet_amd import lib as L
from tests import dec_step_ref as dr

pytestmark = pytest.mark.gpu
DT = {"f32": (L.EM_F32, torch.float32), "bf16": (L.EM_BF16, torch.bfloat16)}
SHAPE_IDS = ["dk64", "dk32"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


_KEEP = []
_WORST = {}


def dev(t):
    """Copy to the GPU and keep the tensor alive until the test ends (raw pointers go to the C ABI)."""
    t = t.contiguous().cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


@pytest.fixture(scope="module", autouse=True)
def _print_summary():
    yield
    for route in sorted(_WORST):
        r, what = _WORST[route]
        print(f"PARITY SUMMARY {route}: worst err / budget {r:.3f} ({what})")


@contextlib.contextmanager
def switches(lib, **env):
    """developer switches of the library for the block: os.environ + em_dev_switches_reload, restored afterwards"""
    names = {f"ESPNET_AMD_{k}": str(v) for k, v in env.items() if v is not None}
    try:
        os.environ.update(names)
        lib.em_dev_switches_reload()
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
        lib.em_dev_switches_reload()


def hold(route, got, ref, dtype, dk, what):
    torch.cuda.synchronize()
    r = dr.assert_in_budget(got, ref, dtype, f"{route} {what}", dk)
    if r >= _WORST.get(route, (-1.0, ""))[0]:
        _WORST[route] = (r, what)
    return r


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def check_caches(case, pos, step, kc, vc, tdt, what):
    """kc[pos] / vc[pos] hold the new K / V bit for bit; every other element of both caches is unchanged"""
    torch.cuda.synchronize()
    qkv, kc0, vc0 = step
    d = case.d
    for name, got, before, new in (("kc", kc, kc0, qkv[:, d:2 * d]), ("vc", vc, vc0, qkv[:, 2 * d:])):
        want = before.clone()
        want[pos] = new
        assert same_bits(got, want.to(tdt)), f"{what}: {name} differs at " \
            f"{torch.nonzero(bits(got.cpu()) != bits(want.to(tdt))).tolist()[:4]} ([position][row][channel])"


def upload_step(step, tdt):
    qkv, kc, vc = step
    return dev(qkv.to(tdt)), dev(kc.to(tdt)), dev(vc.to(tdt))


def out_rows(n, d, tdt):
    return torch.full((n, d), float("nan"), dtype=tdt, device="cuda")


# ------------------------------------------------------------------------------------------ per-row self-attention
@pytest.mark.parametrize("regime", dr.REGIMES)
@pytest.mark.parametrize("split", ["auto-ungrouped"] + dr.SELF_SPLITS, ids=lambda s: f"split-{s}")
@pytest.mark.parametrize("h,d", dr.SELF_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_attention_parity(lib, prec, h, d, split, regime):
    """seven rows in groups of three (ESPNET_AMD_SA_GROUP=3: without it a launch this small runs one row per workgroup, the
    `auto-ungrouped` variant): the last workgroup holds one live row and two clamped ones."""
    dt, tdt = DT[prec]
    case = dr.self_case(dr.SELF_N, dr.SELF_N, h, d, dr.SELF_LMAX, regime, tdt)
    env = {} if split == "auto-ungrouped" else {"SA_GROUP": dr.SELF_GROUP, "SA_SPLIT": split}
    top = 0.0
    with switches(lib, **env):
        for pos in dr.SELF_POS:
            step = dr.at_position(case, pos)
            qkv, kc, vc = upload_step(step, tdt)
            ctx = out_rows(case.n, d, tdt)
            L.check(lib.em_dec_self_attention(dt, L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(dev(case.anc)), L.ptr(dev(case.other)),
                                              case.n, d, h, case.Lmax, pos, None, dr.SELF_GROUP, None, L.ptr(ctx),
                                              L.current_stream_ptr()), "self_attn")
            what = f"d_k={case.dk} pos={pos} split={split} {regime}"
            top = max(top, hold(f"em_dec_self_attention[{prec}]", ctx, dr.ref_self(case, pos, step), tdt, case.dk, what))
            check_caches(case, pos, step, kc, vc, tdt, what)
    print(f"PARITY em_dec_self_attention[{prec}] d_k={case.dk} split={split} {regime}: err / budget {top:.3f}")


@pytest.mark.parametrize("regime", dr.REGIMES)
@pytest.mark.parametrize("h,d", dr.SELF_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_attention_token_mask_parity(lib, prec, h, d, regime):
    """tok_tab: ids 0 scattered over the prefix, row 2's current token id 0, the last row with every key masked (zeros)."""
    dt, tdt = DT[prec]
    case = dr.self_case(dr.SELF_N, dr.SELF_N, h, d, dr.SELF_LMAX, regime, tdt, tok=True)
    top = 0.0
    with switches(lib, SA_GROUP=dr.SELF_GROUP):
        for pos in dr.TOK_POS:
            step = dr.at_position(case, pos)
            qkv, kc, vc = upload_step(step, tdt)
            ctx = out_rows(case.n, d, tdt)
            L.check(lib.em_dec_self_attention(dt, L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(dev(case.anc)), L.ptr(dev(case.other)),
                                              case.n, d, h, case.Lmax, pos, None, dr.SELF_GROUP, L.ptr(dev(case.tok)), L.ptr(ctx),
                                              L.current_stream_ptr()), "self_attn tok_tab")
            what = f"tok_tab d_k={case.dk} pos={pos} {regime}"
            top = max(top, hold(f"em_dec_self_attention[{prec}] tok_tab", ctx, dr.ref_self(case, pos, step), tdt, case.dk, what))
            assert bool((ctx[case.n - 1] == 0).all()), what  # every key masked
            check_caches(case, pos, step, kc, vc, tdt, what)
    print(f"PARITY em_dec_self_attention[{prec}] tok_tab d_k={case.dk} {regime}: err / budget {top:.3f}")


@pytest.mark.parametrize("regime", dr.REGIMES)
@pytest.mark.parametrize("h,d", dr.SELF_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_attention_device_position_parity(lib, prec, h, d, regime):
    """pos_dev as every replayed step passes it: host pos = 0, the table chosen by step parity (the other one names the
    poisoned rows), and *pos_dev = Lmax, where the launch must leave ctx and both caches alone."""
    dt, tdt = DT[prec]
    case = dr.self_case(dr.SELF_N, dr.SELF_N, h, d, dr.SELF_LMAX, regime, tdt)
    top = 0.0
    with switches(lib, SA_GROUP=dr.SELF_GROUP):
        for pos in dr.POSDEV_POS + [case.Lmax]:
            step = dr.at_position(case, min(pos, case.Lmax - 1))
            qkv, kc, vc = upload_step(step, tdt)
            ctx = out_rows(case.n, d, tdt)
            even, odd = (case.anc, case.other) if pos % 2 == 0 else (case.other, case.anc)
            pd = dev(torch.tensor([pos], dtype=torch.int32))
            L.check(lib.em_dec_self_attention(dt, L.ptr(qkv), L.ptr(kc), L.ptr(vc), L.ptr(dev(even)), L.ptr(dev(odd)), case.n, d, h,
                                              case.Lmax, 0, L.ptr(pd), dr.SELF_GROUP, None, L.ptr(ctx), L.current_stream_ptr()),
                    "self_attn pos_dev")
            what = f"pos_dev d_k={case.dk} *pos_dev={pos} {regime}"
            if pos == case.Lmax:
                torch.cuda.synchronize()
                assert bool(torch.isnan(ctx).all()), what
                assert same_bits(kc, step[1].to(tdt)) and same_bits(vc, step[2].to(tdt)), what
                continue
            top = max(top, hold(f"em_dec_self_attention[{prec}] pos_dev", ctx, dr.ref_self(case, pos, step), tdt, case.dk, what))
            check_caches(case, pos, step, kc, vc, tdt, what)
    print(f"PARITY em_dec_self_attention[{prec}] pos_dev d_k={case.dk} {regime}: err / budget {top:.3f}")


# ------------------------------------------------------------------------------------------ beam tree
@pytest.mark.parametrize("regime", dr.REGIMES)
@pytest.mark.parametrize("route", ["tree", "row"])
@pytest.mark.parametrize("kind", dr.TREE_KINDS)
@pytest.mark.parametrize("W,Lmax", dr.TREE_W_LMAX, ids=[f"W{W}" for W, _ in dr.TREE_W_LMAX])
def test_self_attention_beam_parity(lib, W, Lmax, kind, route, regime):
    """em_dec_self_attention_beam on the tree kernel and, with ESPNET_AMD_NO_SA_TREE=1, on the per-row kernel: each against
    the reference, and em_dec_self_attention_beam_route names the kernel that ran.  The last step of the list passes the
    (odd) position through pos_dev with the tables swapped."""
    tdt = torch.bfloat16
    h, d, n = dr.TREE_HEADS, dr.TREE_D, dr.TREE_B * W
    case = dr.self_case(n, W, h, d, Lmax, regime, tdt, kind)
    env = {"SA_TREE_MIN_ROWS": 0, "NO_SA_TREE": 1 if route == "row" else None}
    name = f"em_dec_self_attention_beam[{route}]"
    top = 0.0
    with switches(lib, **env):
        assert lib.em_dec_self_attention_beam_route(L.EM_BF16, n, d, h, Lmax, W) == (1 if route == "tree" else 0)
        for pos, by_dev in [(p, False) for p in dr.tree_positions(kind, W, Lmax)] + [(dr.TREE_POSDEV, True)]:
            step = dr.at_position(case, pos)
            qkv, kc, vc = upload_step(step, tdt)
            ctx = out_rows(n, d, tdt)
            if by_dev:
                pd = dev(torch.tensor([pos], dtype=torch.int32))
                args = (L.ptr(dev(case.other)), L.ptr(dev(case.anc)), n, d, h, Lmax, 0, L.ptr(pd))
            else:
                args = (L.ptr(dev(case.anc)), L.ptr(dev(case.other)), n, d, h, Lmax, pos, None)
            L.check(lib.em_dec_self_attention_beam(L.EM_BF16, L.ptr(qkv), L.ptr(kc), L.ptr(vc), *args, W, L.ptr(ctx),
                                                   L.current_stream_ptr()), name)
            what = f"W={W} Lmax={Lmax} {kind} pos={pos}{' (pos_dev)' if by_dev else ''} {regime}"
            top = max(top, hold(name, ctx, dr.ref_self(case, pos, step, "tree"), tdt, case.dk, what))
            check_caches(case, pos, step, kc, vc, tdt, what)
    print(f"PARITY {name} W={W} {kind} {regime}: err / budget {top:.3f}")


def test_beam_route_follows_the_acceptance_condition(lib):
    """the route function is the launcher's own condition: dtype, d_k, W, Lmax, the LDS bound, the row minimum, the switch"""
    route = lib.em_dec_self_attention_beam_route
    with switches(lib, SA_TREE_MIN_ROWS=0):
        assert route(L.EM_BF16, 20, 128, 2, 400, 10) == 1
        assert route(L.EM_F32, 20, 128, 2, 400, 10) == 0
        assert route(L.EM_BF16, 20, 64, 2, 400, 10) == 0    # d_k = 32
        assert route(L.EM_BF16, 20, 128, 2, 513, 2) == 0    # Lmax > 512
        assert route(L.EM_BF16, 34, 128, 2, 100, 17) == 0   # W > 16
        assert route(L.EM_BF16, 7, 128, 2, 100, 1) == 0     # W = 1
        assert route(L.EM_BF16, 32, 128, 2, 332, 16) == 1 and route(L.EM_BF16, 32, 128, 2, 333, 16) == 0  # 64 KiB of LDS
    assert route(L.EM_BF16, 190, 128, 2, 258, 10) == 0 and route(L.EM_BF16, 200, 128, 2, 258, 10) == 1    # 200 rows
    with switches(lib, NO_SA_TREE=1):
        assert route(L.EM_BF16, 200, 128, 2, 258, 10) == 0


# ------------------------------------------------------------------------------------------ source attention
def run_transpose(lib, dt, tdt, case, Tpad, what):
    kv = dev(case.kv.to(tdt))
    vT = dev(torch.zeros(case.B, case.d, Tpad, dtype=tdt))
    L.check(lib.em_dec_transpose_v(dt, L.ptr(kv), case.B, case.T, case.d, Tpad, L.ptr(vT), L.current_stream_ptr()), "transpose_v")
    torch.cuda.synchronize()
    assert same_bits(vT, dr.want_vt(case, Tpad).to(tdt)), f"em_dec_transpose_v {what}"
    return kv, vT


@pytest.mark.parametrize("regime", dr.REGIMES)
@pytest.mark.parametrize("h,d", dr.SRC_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_src_attention_parity(lib, prec, h, d, regime):
    dt, tdt = DT[prec]
    top = 0.0
    for T, W, Tpad in dr.src_cases():
        case = dr.src_case(T, W, h, d, regime, tdt)
        what = f"d_k={case.dk} T={T} klens={case.klens} W={W} Tpad={Tpad} {regime}"
        kv, vT = run_transpose(lib, dt, tdt, case, Tpad, what)
        ctx = out_rows(case.B * W, d, tdt)
        L.check(lib.em_dec_src_attention(dt, L.ptr(dev(case.qs.to(tdt))), L.ptr(kv), 2 * d, L.ptr(vT),
                                         L.ptr(dev(torch.tensor(case.klens, dtype=torch.int32))), case.B, W, d, h, T, Tpad, L.ptr(ctx),
                                         L.current_stream_ptr()), "src_attn")
        top = max(top, hold(f"em_dec_src_attention[{prec}]", ctx, dr.ref_src(case), tdt, case.dk, what))
    print(f"PARITY em_dec_src_attention[{prec}] d_k={case.dk} {regime}: err / budget {top:.3f}")


@pytest.mark.parametrize("d", [256, 512])
def test_src_attention_lnq_parity(lib, d):
    """em_dec_src_attention_lnq and _lnq_frag stay bit-equal to em_ln_gemm + em_dec_src_attention (W = 17: a second row group
    of one row), and that two-launch result, from the q the device rounded, is inside the budget."""
    dt, tdt = DT["bf16"]
    h = d // 64
    top = 0.0
    for T, W in dr.LNQ_CASES:
        case = dr.src_case(T, W, h, d, "flat", tdt)
        n, Tpad = case.B * W, (T + 31) // 32 * 32
        what = f"d={d} T={T} klens={case.klens} W={W}"
        g = torch.Generator().manual_seed(7 * T + W + d)
        x = dev(torch.randn(n, d, generator=g) * 2 + 0.3)
        ln_g, ln_b = dev(1 + 0.1 * torch.randn(d, generator=g)), dev(0.1 * torch.randn(d, generator=g))
        wq = dev((torch.randn(d, d, generator=g) * d ** -0.5).to(tdt))  # (q of unit scale: scores as in the flat regime)
        bq = dev(0.1 * torch.randn(d, generator=g))
        kv, vT = run_transpose(lib, dt, tdt, case, Tpad, what)
        kl = dev(torch.tensor(case.klens, dtype=torch.int32))
        qs = out_rows(n, d, tdt)
        L.check(lib.em_ln_gemm(dt, L.EM_EPI_STORE, L.ptr(x), L.ptr(ln_g), L.ptr(ln_b), 1e-12, L.ptr(wq), L.ptr(bq), L.ptr(qs),
                               n, d, d, d, L.current_stream_ptr()), "em_ln_gemm")
        two = out_rows(n, d, tdt)
        L.check(lib.em_dec_src_attention(dt, L.ptr(qs), L.ptr(kv), 2 * d, L.ptr(vT), L.ptr(kl), case.B, W, d, h, T, Tpad, L.ptr(two),
                                         L.current_stream_ptr()), "src_attn")
        tail = (L.ptr(bq), L.ptr(kv), 2 * d, L.ptr(vT), L.ptr(kl), case.B, W, d, h, T, Tpad)
        one = out_rows(n, d, tdt)
        L.check(lib.em_dec_src_attention_lnq(dt, L.ptr(x), L.ptr(ln_g), L.ptr(ln_b), 1e-12, L.ptr(wq), *tail, L.ptr(one),
                                             L.current_stream_ptr()), "src_attn_lnq")
        frag = out_rows(n, d, tdt)
        wqf = dev(L.pack_frag16(wq))
        L.check(lib.em_dec_src_attention_lnq_frag(dt, L.ptr(x), L.ptr(ln_g), L.ptr(ln_b), 1e-12, L.ptr(wqf), *tail, L.ptr(frag),
                                                  L.current_stream_ptr()), "src_attn_lnq_frag")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(qs.float()).all()), what
        top = max(top, hold("em_ln_gemm + em_dec_src_attention[bf16]", two, dr.ref_src(case, qs.float().cpu()), tdt, 64, what))
        assert same_bits(one, two), f"lnq {what}: {(one.float() - two.float()).abs().max().item()}"
        assert same_bits(frag, two), f"lnq_frag {what}: {(frag.float() - two.float()).abs().max().item()}"
    print(f"PARITY em_dec_src_attention_lnq d={d}: err / budget {top:.3f}")


# ------------------------------------------------------------------------------------------ embeddings, LM input norm
EMB_V, EMB_N, EMB_LMAX = 11, 9, 6
EMB_IDS = [0, 10, -1, -7, 11, 400, 5, 3, 10]  # below 0 and at or above V: clamped


def in_bound(got, ref, bound, what):
    torch.cuda.synchronize()
    err = (got.cpu().to(torch.float64) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    flat = int(ratio.argmax())
    assert float(ratio.reshape(-1)[flat]) <= 1.0, (f"{what}: err / bound = {float(ratio.reshape(-1)[flat]):.3g} at row {flat // ref.shape[1]}, "
                                                   f"channel {flat % ref.shape[1]}: got {float(got.reshape(-1)[flat])!r}, reference {float(ref.reshape(-1)[flat])!r}")
    return float(ratio.max())


def token_table(g):
    """[Lmax][n] ids; row `pos` of it is what a step reads"""
    tab = torch.randint(-3, EMB_V + 3, (EMB_LMAX, EMB_N), generator=g, dtype=torch.int32)
    tab[3] = torch.tensor(EMB_IDS, dtype=torch.int32)
    return tab


@pytest.mark.parametrize("d", [64, 200])
def test_dec_embed_parity(lib, d):
    """em_dec_embed_f32: x = embed[clamp(tok)] * sqrt(d) + pe[pos]; host position and pos_dev; untouched at the limit."""
    g = torch.Generator().manual_seed(d)
    embed, pe, tab = torch.randn(EMB_V, d, generator=g), torch.randn(EMB_LMAX, d, generator=g), token_table(g)
    top = 0.0
    for pos, by_dev in [(3, False), (3, True), (5, True), (0, False), (EMB_LMAX, True)]:
        x = out_rows(EMB_N, d, torch.float32)
        pd = dev(torch.tensor([pos], dtype=torch.int32)) if by_dev else None
        tok = dev(tab) if by_dev else dev(tab[pos])
        L.check(lib.em_dec_embed_f32(L.ptr(dev(embed)), L.ptr(dev(pe)), L.ptr(tok), EMB_N, EMB_V, d, 0 if by_dev else pos, L.ptr(pd),
                                     EMB_LMAX, L.ptr(x), L.current_stream_ptr()), "dec_embed")
        torch.cuda.synchronize()
        if pos == EMB_LMAX:
            assert bool(torch.isnan(x).all())
            continue
        ref, bound = dr.ref_dec_embed(embed, pe, tab[pos], pos)
        top = max(top, in_bound(x, ref, bound, f"em_dec_embed_f32 d={d} pos={pos} pos_dev={by_dev}"))
    _WORST[f"em_dec_embed_f32 d={d}"] = (top, "of 2^-24 (2 |e| sqrt(d) + |x|)")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_lm_embed_is_exact(lib, prec):
    """em_lm_embed only copies (f32) or rounds to nearest even (bf16): exact; ids clamped; untouched at the limit."""
    dt, tdt = DT[prec]
    eu = 130
    g = torch.Generator().manual_seed(eu)
    embed, tab = torch.randn(EMB_V, eu, generator=g), token_table(g)
    for pos, by_dev in [(3, False), (3, True), (4, True), (EMB_LMAX, True)]:
        e = out_rows(EMB_N, eu, tdt)
        pd = dev(torch.tensor([pos], dtype=torch.int32)) if by_dev else None
        tok = dev(tab) if by_dev else dev(tab[pos])
        L.check(lib.em_lm_embed(dt, L.ptr(dev(embed)), L.ptr(tok), EMB_N, EMB_V, eu, L.ptr(pd), EMB_LMAX, L.ptr(e),
                                L.current_stream_ptr()), "lm_embed")
        torch.cuda.synchronize()
        if pos == EMB_LMAX:
            assert bool(torch.isnan(e).all())
            continue
        assert same_bits(e, embed[dr.clamp_ids(tab[pos], EMB_V)].to(tdt)), (prec, pos, by_dev)


@pytest.mark.parametrize("d", [64, 200, 512])
def test_lm_input_norm_parity(lib, d):
    """em_lm_input_norm_f32: LayerNorm(1e-5) -> ReLU -> optional x sqrt(d) + pe[pos], in place; five rows (a partial last
    workgroup of four waves); with and without pe, host position and pos_dev; untouched at the limit."""
    n = 5
    g = torch.Generator().manual_seed(d + 1)
    x0 = torch.randn(n, d, generator=g) * 2 + 0.3
    ln_g, ln_b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    pe = torch.randn(EMB_LMAX, d, generator=g)
    top = 0.0
    for with_pe, pos, by_dev in [(False, 0, False), (True, 4, False), (True, 3, True), (False, 3, True), (True, EMB_LMAX, True)]:
        x = dev(x0.clone())
        pd = dev(torch.tensor([pos], dtype=torch.int32)) if by_dev else None
        L.check(lib.em_lm_input_norm_f32(L.ptr(x), L.ptr(dev(ln_g)), L.ptr(dev(ln_b)), L.ptr(dev(pe)) if with_pe else None, n, d,
                                         0 if by_dev else pos, L.ptr(pd), EMB_LMAX, L.current_stream_ptr()), "lm_input_norm")
        torch.cuda.synchronize()
        if pos == EMB_LMAX:
            assert same_bits(x, x0)
            continue
        ref, bound = dr.ref_lm_input_norm(x0, ln_g, ln_b, pe if with_pe else None, pos)
        top = max(top, in_bound(x, ref, bound, f"em_lm_input_norm_f32 d={d} pe={with_pe} pos={pos} pos_dev={by_dev}"))
    _WORST[f"em_lm_input_norm_f32 d={d}"] = (top, "of the operation-count bound")
