"""The host side of the resumable greedy transducer walk without a GPU: the slot allocator and the refusals that need no
device."""
import pytest
import torch


def test_stream_state_bookkeeping():
    from espnet_amd.asr.transducer.beam_search_transducer import TransducerStreamState

    st = TransducerStreamState(2, 64, "cpu", blank=0)
    assert st.n_free == 2 and not st.slab.any() and st.yseq[1] == [0]
    a, b = st.acquire(), st.acquire()
    assert (a, b) == (0, 1) and st.live == [0, 1]
    st.slab[1] = 7
    st.yseq[1], st.score[1], st.frames[1] = [0, 5], -1.5, 3
    c = st.acquire()  # no free slot: the slab doubles, the live slots keep their bytes and numbers
    assert c == 2 and st.n_slots == 4 and bool((st.slab[1] == 7).all()) and not st.slab[2:].any()
    st.release(1)
    with pytest.raises(ValueError, match="not in use"):
        st.release(1)
    assert st.acquire() == 1 and not st.slab[1].any()  # the lowest free slot, handed out reset
    assert (st.yseq[1], st.score[1], st.frames[1]) == ([0], 0.0, 0)
    with pytest.raises(ValueError, match="outside"):
        st.reset([4])


def test_extend_refuses_a_beam():
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.tasks.asr import ASRTask
    from tests.test_gpu_transducer import PEAKED, _config

    model = ASRTask.build_model(dict(_config(*PEAKED), compute_dtype="float32"))
    bs = BeamSearchTransducer(model.decoder, model.joint_network, beam_size=2)
    with pytest.raises(NotImplementedError, match="beam_size=2"):
        bs.extend(None, [0], torch.zeros(1, 4, 64), [4])
    assert hasattr(BeamSearchTransducer, "stream_state")
