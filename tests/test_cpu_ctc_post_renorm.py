"""The renormalised CTC token posteriors without a GPU: the C ABI's symbols, workspace size and argument checks (which
return before anything is launched)."""
import ctypes as C
from pathlib import Path

import pytest

from espnet_amd import lib as L

REPO = Path(__file__).resolve().parent.parent
NAMES = ("em_ctc_seq_posteriors_renorm", "em_ctc_seq_posteriors_renorm_workspace_bytes")


def test_symbols_are_declared_and_bound():
    hdr = (REPO / "include" / "espnet_amd.h").read_text()
    for name in NAMES:
        assert name + "(" in hdr and name in L._SIGNATURES, name
    assert L._SIGNATURES[NAMES[0]] == L._SIGNATURES["em_ctc_seq_posteriors"]
    assert L._SIGNATURES[NAMES[1]] == (C.c_size_t, [C.c_int32] * 3)


def test_workspace_covers_rows_and_offsets():
    lib = L.load()
    cap = int(lib.em_ctc_forced_align_max_tokens())
    for N, T, Lmax in ((1, 1, 0), (3, 249, 80), (1, 600, 300), (1, 15000, 3000), (2, 7, cap)):
        plain, mine = int(lib.em_ctc_seq_posteriors_workspace_bytes(N, T, Lmax)), int(lib.em_ctc_seq_posteriors_renorm_workspace_bytes(N, T, Lmax))
        rows = 2 * ((T + 1) // 2 + 1)  # of both directions: one int32 offset each
        assert mine % 16 == 0 and plain + 4 * N * rows <= mine <= plain + 4 * N * (rows + 3), (N, T, Lmax)
    for shape in ((1, 8, cap + 1), (0, 8, 2), (1, 0, 2), (1, 8, -1)):
        assert lib.em_ctc_seq_posteriors_renorm_workspace_bytes(*shape) == 0, shape


@pytest.mark.parametrize("what, want", [("no lpT", L.EM_ERR_BAD_ARG), ("no outputs", L.EM_ERR_BAD_ARG), ("N above Bm without mem_of", L.EM_ERR_BAD_ARG),
                                        ("ldT below Bm * T", L.EM_ERR_BAD_ARG), ("ws not aligned", L.EM_ERR_BAD_ARG),
                                        ("tokens above the cap", L.EM_ERR_UNSUPPORTED), ("no ws", L.EM_ERR_UNSUPPORTED),
                                        ("short ws", L.EM_ERR_UNSUPPORTED)])
def test_argument_checks(what, want):
    lib = L.load()
    buf = C.create_string_buffer(64)  # never read: every case returns in front of the launch
    p = (C.addressof(buf) + 15) & ~15
    need = int(lib.em_ctc_seq_posteriors_renorm_workspace_bytes(2, 8, 2))
    a = dict(lpT=p, ldT=16, xlens=p, Bm=2, T=8, targets=p, Lmax=2, ylens=p, mem_of=None, N=2, blank=0, nll=p, occ=p, peak=p, peak_t=p,
             blank_post=None, ws=p, ws_bytes=need, stream=None)
    a.update({"no lpT": dict(lpT=None), "no outputs": dict(occ=None), "N above Bm without mem_of": dict(N=3), "ldT below Bm * T": dict(ldT=15),
              "ws not aligned": dict(ws=p + 4), "tokens above the cap": dict(Lmax=int(lib.em_ctc_forced_align_max_tokens()) + 1),
              "no ws": dict(ws=None), "short ws": dict(ws_bytes=need - 1)}[what])
    assert lib.em_ctc_seq_posteriors_renorm(*a.values()) == want
