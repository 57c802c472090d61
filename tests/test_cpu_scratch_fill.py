"""The scratch-poisoning helper (tests/scratch_fill.py) on the CPU: the byte patterns decode to the values its docstring
claims, the byte comparison treats a NaN as equal to itself, and `assert_scratch_independent` catches each of the four
things it asserts on a toy "entry point"."""
import math

import pytest
import torch

from tests import scratch_fill as sf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
def test_patterns_decode_as_claimed(dtype):
    t = torch.empty(3, 5, dtype=dtype)
    assert sf.byte_view(t).numel() == t.numel() * t.element_size()
    assert (sf.fill_bytes(t, sf.ZERO) == 0).all()
    sf.fill_bytes(t, sf.ONES)
    if dtype == torch.int32:
        assert (t == -1).all()
    else:
        assert torch.isnan(t).all()
    sf.fill_bytes(t, sf.BIG)
    if dtype == torch.int32:
        assert (t == 2139062143).all() and 2139062143 == 0x7F7F7F7F
    else:
        assert torch.isfinite(t).all()
        # exponent field 0xFE = 2^127 in both; mantissa 0x7F7F7F of 23 bits (f32), 0x7F of 7 bits (bf16)
        want = (1 + 0x7F7F7F / 2.0 ** 23) * 2.0 ** 127 if dtype == torch.float32 else (1 + 0x7F / 128.0) * 2.0 ** 127
        assert (t.double() == want).all()
        assert math.isclose(want, 3.39e38, rel_tol=2e-3)
        assert not torch.isfinite(t.float() * 2).any()  # (huge enough that one doubling overflows f32)


def test_byte_comparison_takes_nan_as_equal_and_tells_signed_zeros_apart():
    a = torch.tensor([1.0, float("nan"), 0.0])
    assert not torch.equal(a, a.clone())  # what a value comparison would say
    assert sf.bytes_equal(a, a.clone())
    assert not sf.bytes_equal(a, torch.tensor([1.0, float("nan"), -0.0]))
    assert not sf.bytes_equal(a, a.to(torch.bfloat16))
    n = sf.fill_bytes(torch.empty(4, dtype=torch.bfloat16), sf.ONES)
    assert sf.bytes_equal(n, n.clone())
    assert sf.raw_bytes(n).shape == (4, 2)


class _Toy:
    """out[:n] = 2 * x[:n] through a scratch of 8 floats; `bug` picks the way it goes wrong."""

    def __init__(self, bug=None):
        self.bug, self.calls = bug, 0
        self.x = torch.arange(1.0, 7.0)
        self.ws = torch.empty(8)
        self.out = torch.empty(6)
        self.n = 4
        self.defined = [torch.arange(6) < self.n]

    def call(self):
        self.calls += 1
        n = self.n
        if self.bug != "reads_pad":
            self.ws[:n] = self.x[:n]
            acc = self.ws[:n] * 2
        else:
            self.ws[:n - 1] = self.x[:n - 1]  # the last row is read but never written: 0 under ZERO, poison otherwise
            acc = self.ws[:n] * 2
        if self.bug == "arith_mask":
            acc = acc + 0.0 * self.ws[n:2 * n]  # a pad masked by arithmetic: 0 * NaN
        if self.bug == "max_pad":
            acc = torch.fmax(acc, self.ws[n:2 * n])  # a max that takes in the pad: fmax drops NaN
        if self.bug == "not_repeatable":
            acc = acc + self.calls
        self.out[:n] = acc
        if self.bug == "writes_outside":
            self.out[n] = 0.5

    def stale(self):
        self.ws.copy_(torch.arange(100.0, 108.0))


def test_helper_passes_a_clean_call_and_returns_the_zero_run():
    t = _Toy()
    ref = sf.assert_scratch_independent(t.call, t.ws, [t.out], t.defined, stale=t.stale)
    assert t.calls == 5  # ZERO, ZERO, ONES, BIG, STALE
    assert torch.equal(ref[0][:4], torch.tensor([2.0, 4.0, 6.0, 8.0]))
    assert torch.isnan(ref[0][4:]).all()  # the ZERO run's pre-fill is ONES


@pytest.mark.parametrize("bug,what", [("reads_pad", "depends on the scratch"), ("arith_mask", "depends on the scratch"),
                                      ("max_pad", "depends on the scratch"), ("not_repeatable", "not bit-repeatable"),
                                      ("writes_outside", "outside its defined region")])
def test_helper_catches(bug, what):
    t = _Toy(bug)
    with pytest.raises(AssertionError, match=what):
        sf.assert_scratch_independent(t.call, t.ws, [t.out], t.defined, stale=t.stale)


def test_max_over_a_pad_is_invisible_to_nan_and_visible_to_big():
    """Why BIG exists: fmax drops NaN."""
    t = _Toy("max_pad")
    for fill, same in ((sf.ONES, True), (sf.BIG, False)):
        sf.fill_bytes(t.ws, sf.ZERO)
        t.call()
        want = t.out.clone()
        sf.fill_bytes(t.ws, fill)
        t.call()
        assert sf.bytes_equal(t.out[:4], want[:4]) == same, fill


def test_helper_catches_an_element_the_call_never_writes():
    t = _Toy()
    t.defined = None  # the whole buffer is claimed as written, the call writes 4 of 6
    with pytest.raises(AssertionError, match="depends on the scratch|not finite"):
        sf.assert_scratch_independent(t.call, t.ws, [t.out], t.defined)


def test_helper_takes_returned_outputs_with_a_prefill_hook():
    state = {}
    ws = torch.empty(4)

    def call():
        out = sf.fill_bytes(torch.empty(3), state["pre"])
        ws[:3] = torch.tensor([1.0, 2.0, 3.0])
        out[:2] = ws[:2] + 1
        return [out]

    ref = sf.assert_scratch_independent(call, ws, None, [torch.tensor([True, True, False])],
                                        prefill=lambda b: state.__setitem__("pre", b))
    assert ref[0][:2].tolist() == [2.0, 3.0]
