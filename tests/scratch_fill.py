"""Scratch poisoning for the tests of "no output bit of an entry point depends on what its scratch held on entry"
(include/espnet_amd.h, "Scratch memory"; tests/test_gpu_scratch_independence.py, tests/test_cpu_scratch_fill.py).

Byte fills for a uint8 view of any tensor:
  ZERO  0x00
  ONES  0xFF   NaN in f32 (0xFFFFFFFF) and bf16 (0xFFFF), -1 in int32
  BIG   0x7F   +3.39e38 in f32 (0x7F7F7F7F) and bf16 (0x7F7F), finite; 2139062143 in int32.  fmaxf / v_max drop NaN, so a
               max-reduction or a compare that wrongly takes in a pad element cannot be seen with NaN poison: a finite
               huge value shows it.
STALE is not a byte pattern: the caller's `stale()` runs the same entry point to completion in the same scratch at
another, larger shape with other inputs, and the scratch is left as that call left it.

`assert_scratch_independent` runs one call under ZERO (twice), ONES, BIG and STALE and compares the outputs bit for bit;
the reference of every fill is the ZERO run of the same call, so no tolerance is involved.
"""
from typing import Callable, Optional, Sequence

import numpy as np
import torch

ZERO, ONES, BIG = 0x00, 0xFF, 0x7F
STALE = "stale"
FILL_NAMES = {ZERO: "ZERO", ONES: "ONES", BIG: "BIG", STALE: "STALE"}


def byte_view(t: torch.Tensor) -> torch.Tensor:
    """Every byte of a contiguous tensor as a flat uint8 view (shares its memory)."""
    assert t.is_contiguous(), "byte fills need a contiguous tensor"
    return t.reshape(-1).view(torch.uint8)


def fill_bytes(t: torch.Tensor, byte: int) -> torch.Tensor:
    if t.numel():
        byte_view(t).fill_(byte)
    return t


def raw_bytes(t: torch.Tensor) -> np.ndarray:
    """A host copy of the tensor's bytes, [numel][itemsize] uint8."""
    t = t.detach().contiguous()
    return byte_view(t).cpu().numpy().reshape(t.numel(), t.element_size()).copy()


def bytes_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality: a NaN equals a NaN of the same bits, +0 differs from -0."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw_bytes(a), raw_bytes(b))


def _element_mask(mask, t: torch.Tensor) -> np.ndarray:
    if mask is None:
        return np.ones(t.numel(), dtype=bool)
    m = torch.as_tensor(mask).to(torch.bool).cpu()
    return m.expand(t.shape).reshape(-1).numpy().copy()


def _finite(t: torch.Tensor) -> np.ndarray:
    return torch.isfinite(t.detach().float().cpu()).reshape(-1).numpy() if t.is_floating_point() else np.ones(t.numel(), bool)


def _first(bad: np.ndarray, shape) -> str:
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} of {bad.size} elements, first at {tuple(int(v) for v in np.unravel_index(i, tuple(shape) or (1,)))}"


def assert_scratch_independent(call: Callable, scratch, outputs: Optional[Sequence[torch.Tensor]], defined=None, *,
                               stale: Optional[Callable] = None, prefill: Optional[Callable] = None, finite=None,
                               names: Optional[Sequence[str]] = None, synchronize: Optional[Callable] = None):
    """`call()` runs the entry point on `scratch` (a tensor or several) and writes `outputs`.

    outputs  the tensors the call writes, pre-filled here before every run.  None: the call allocates its outputs and
             RETURNS them (the same shapes every run); `prefill(byte)` then tells the test's allocation shim which byte
             the next run's outputs start from.
    defined  per output None (the whole buffer is written) or a boolean mask, broadcastable to the output's shape, of the
             elements the header defines as written.
    stale    runs the other, larger call in the same scratch (omitted: no STALE leg).
    finite   per output None or the mask of the elements that must be finite, where the header itself defines an
             infinite value inside the written region (default: all of the defined region).

    Per fill: the scratch is set, the outputs are pre-filled with a pattern that differs between the runs (ONES for the
    ZERO runs, ZERO for all others: an element the call never writes shows as an inequality), the call runs, and the
    outputs are kept as raw bytes.  Then, in this order: two ZERO runs are bit-equal; every other fill gives the ZERO
    run's bytes over the defined region; float outputs are finite there; elements outside it still hold their pre-fill.
    Returns the ZERO run's outputs (host copies)."""
    scr = [scratch] if isinstance(scratch, torch.Tensor) else list(scratch)
    sync = synchronize or (torch.cuda.synchronize if any(t.is_cuda for t in scr) else (lambda: None))

    def run(fill):
        pre = ONES if fill == ZERO else ZERO
        if fill == STALE:
            stale()
        else:
            for t in scr:
                fill_bytes(t, fill)
        if prefill is not None:
            prefill(pre)
        for t in outputs or ():
            fill_bytes(t, pre)
        got = call()
        sync()
        outs = list(outputs) if outputs is not None else list(got)
        return pre, [o.detach().cpu().clone() for o in outs]

    pre0, ref = run(ZERO)
    tags = list(names) if names is not None else [f"output {i}" for i in range(len(ref))]
    masks = [_element_mask(None if defined is None else defined[i], o) for i, o in enumerate(ref)]
    fin = [m if finite is None or finite[i] is None else m & _element_mask(finite[i], o)
           for i, (o, m) in enumerate(zip(ref, masks))]
    raw0 = [raw_bytes(o) for o in ref]

    def outside_keeps(pre, outs, fill):
        for tag, o, m in zip(tags, outs, masks):
            bad = (raw_bytes(o) != pre).any(axis=1) & ~m
            assert not bad.any(), f"{tag}: written outside its defined region under {FILL_NAMES[fill]}: {_first(bad, o.shape)}"

    # 1. the premise: the call repeats itself on identical scratch
    _, again = run(ZERO)
    for tag, a, r in zip(tags, again, raw0):
        bad = (raw_bytes(a) != r).any(axis=1)
        assert not bad.any(), f"{tag}: not bit-repeatable on zero-filled scratch: {_first(bad, a.shape)}"
    runs = [(f, *run(f)) for f in (ONES, BIG) + ((STALE,) if stale is not None else ())]
    # 2. every other fill gives the ZERO run's bytes over the defined region
    for fill, _, outs in runs:
        for tag, o, r, m in zip(tags, outs, raw0, masks):
            bad = (raw_bytes(o) != r).any(axis=1) & m
            assert not bad.any(), f"{tag}: depends on the scratch contents ({FILL_NAMES[fill]} against ZERO): {_first(bad, o.shape)}"
    # 3. ... where float outputs are finite
    for fill, outs in [(ZERO, ref)] + [(f, o) for f, _, o in runs]:
        for tag, o, m in zip(tags, outs, fin):
            bad = ~_finite(o) & m
            assert not bad.any(), f"{tag}: not finite in its defined region under {FILL_NAMES[fill]}: {_first(bad, o.shape)}"
    # 4. elements outside it still hold their pre-fill
    outside_keeps(pre0, ref, ZERO)
    for fill, pre, outs in runs:
        outside_keeps(pre, outs, fill)
    return ref
