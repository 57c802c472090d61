"""What the resumable time-synchronous CTC search (em_ctc_tsync_extend; tests/test_gpu_ctc_tsync_stream.py) has that needs no
device: the slot allocator of the state slab, the constructor refusals of Speech2TextStreaming(search="tsync"), and the two
symbols in the header and in espnet_amd/lib.py."""
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------- the slot allocator
def _state(n_slots=3, slot_bytes=16):
    from espnet_amd.nets.beam_search_timesync import TsyncStreamState

    st = TsyncStreamState(n_slots, 24, slot_bytes, "cpu", K=6, W=4)
    st.slab.copy_(torch.arange(n_slots * slot_bytes, dtype=torch.uint8).reshape(n_slots, slot_bytes))
    return st


def test_acquire_gives_the_lowest_free_slot_and_release_returns_it():
    st = _state()
    assert (st.n_slots, st.n_free, st.live) == (3, 3, [])
    assert [st.acquire() for _ in range(3)] == [0, 1, 2]
    assert st.n_free == 0 and st.live == [0, 1, 2] and st.frames == {0: 0, 1: 0, 2: 0}
    st.release(1)
    assert st.n_free == 1 and st.live == [0, 2]
    assert st.acquire() == 1  # a released slot is reused before the slab grows
    st.release(2)
    st.release(0)
    assert st.acquire() == 0 and st.acquire() == 2
    with pytest.raises(ValueError, match="slot 7 is not in use"):
        st.release(7)
    st.release(1)
    with pytest.raises(ValueError, match="slot 1 is not in use"):
        st.release(1)


def test_grow_keeps_live_slots_indices_and_bytes():
    st = _state()
    a, b, c = st.acquire(), st.acquire(), st.acquire()
    st.frames[b] = 11
    st.release(a)
    before = st.slab.clone()
    st.grow()
    assert st.n_slots == 6 and st.slab.shape == (6, 16) and st.n_grown == 1
    assert torch.equal(st.slab[:3], before)  # every old slot at its old index, byte for byte
    assert st.live == [b, c] and st.frames[b] == 11 and st.n_free == 4
    assert [st.acquire() for _ in range(4)] == [0, 3, 4, 5]
    assert st.acquire() == 6 and st.n_slots == 12  # no free slot: the slab doubles by itself
    assert torch.equal(st.slab[:3], before)
    st.grow(20)
    assert st.n_slots == 20 and torch.equal(st.slab[:3], before)
    with pytest.raises(ValueError, match="holds 20 slots already"):
        st.grow(20)
    with pytest.raises(ValueError):
        _state(n_slots=0)


# ------------------------------------------------------------------------------------------- the constructor refusals
def test_constructor_refusals_need_no_device():
    """Raised before any model is built: the file names are never opened."""
    from espnet_amd.bin.asr_inference_streaming import Speech2TextStreaming

    with pytest.raises(NotImplementedError, match=r"search='tsync' with ctc_weight=0.3: the attention decoder is not scored "
                                                  r"time-synchronously on the MI355X path; pass ctc_weight=1.0"):
        Speech2TextStreaming("no.yaml", None, search="tsync", ctc_weight=0.3)
    with pytest.raises(NotImplementedError, match="lm_train_config: a neural LM is not scored time-synchronously"):
        Speech2TextStreaming("no.yaml", None, search="tsync", ctc_weight=1.0, lm_train_config="lm.yaml")
    for other in ("online", "greedy", "offline"):
        with pytest.raises(NotImplementedError, match=f"ngram_file with search='{other}'"):
            Speech2TextStreaming("no.yaml", None, search=other, ngram_file="x.arpa")
    with pytest.raises(NotImplementedError, match="ngram_file with search='online'"):  # (the default search of beam 20)
        Speech2TextStreaming("no.yaml", None, ngram_file="x.arpa")
    with pytest.raises(ValueError, match="tsync_max_frames"):
        Speech2TextStreaming("no.yaml", None, search="tsync", ctc_weight=1.0, tsync_max_frames=0)
    with pytest.raises(ValueError, match="ngram_scorer"):
        Speech2TextStreaming("no.yaml", None, search="tsync", ctc_weight=1.0, ngram_scorer="half")
    with pytest.raises(ValueError, match="search='beam'"):
        Speech2TextStreaming("no.yaml", None, search="beam")
    with pytest.raises(RuntimeError, match="MI355X only"):
        Speech2TextStreaming("no.yaml", None, search="tsync", ctc_weight=1.0, device="cpu")


def test_status_messages_name_the_parameter():
    from espnet_amd.nets.beam_search_timesync import BeamSearchTimeSync, TsyncTick

    st = _state()
    st.first_use[2] = dict(K=6, W=4, max_frames=24)
    outs = (torch.zeros(1, 1, 24),)
    with pytest.raises(RuntimeError, match="holds 20 frames and 9 more would exceed tsync_max_frames = 24"):
        BeamSearchTimeSync._raise_status(TsyncTick(outs, st, [2], [9], dict(K=6, W=4, max_frames=24)), 0, 1, 20)
    with pytest.raises(RuntimeError, match=r"W \(the slot was first used with 4, the call has 5\)"):
        BeamSearchTimeSync._raise_status(TsyncTick(outs, st, [2], [0], dict(K=6, W=5, max_frames=24)), 0, 2, 0)
    with pytest.raises(RuntimeError, match="never reset"):
        BeamSearchTimeSync._raise_status(TsyncTick(outs, st, [1], [0], dict(K=6, W=4, max_frames=24)), 0, 2, 0)


# ------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_and_in_the_header():
    import ctypes as C

    from espnet_amd import lib as L

    header = (REPO / "include" / "espnet_amd.h").read_text()
    for name, n_args in (("em_ctc_tsync_extend", 31), ("em_ctc_tsync_state_bytes", 3)):
        assert name in L.exported_symbols()
        m = re.search(rf"\b(?:int|size_t) {name}\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(L._SIGNATURES[name][1]), name
    assert L._SIGNATURES["em_ctc_tsync_state_bytes"][0] is C.c_size_t
    assert L._SIGNATURES["em_ctc_tsync_extend"][0] is C.c_int
    # the state is named PERSISTENT next to the entry, and the scratch paragraph does not claim it
    doc = header[header.index("em_ctc_tsync_extend: the same walk"): header.index("size_t em_ctc_tsync_state_bytes")]
    assert "PERSISTENT" in doc and "not scratch" in doc
    scratch = header[header.index("Scratch memory (every"): header.index("#ifndef ESPNET_AMD_H_")]
    assert "its `state` is NOT scratch" in scratch
    if L.library_path().exists():  # (a built tree: the sizes the header promises)
        lib = L.load()
        assert lib.em_ctc_tsync_state_bytes(1536, 15, 10) > 0 and lib.em_ctc_tsync_state_bytes(1536, 15, 10) % 8 == 0
        assert lib.em_ctc_tsync_state_bytes(1536, 65, 10) == 0 and lib.em_ctc_tsync_state_bytes(1536, 15, 33) == 0
        assert lib.em_ctc_tsync_state_bytes(0, 15, 10) == 0
