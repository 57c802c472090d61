"""CTC token posteriors without a GPU: the float64 forward-backward (tests/ctc_post_ref.py) pinned three ways."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests.ctc_align_ref import collapse
from tests.ctc_nll_ref import ctc_nll_ref
from tests.ctc_post_ref import ctc_post_ref


def _lp(T, V, seed):
    return torch.log_softmax(3.0 * torch.randn(T, V, generator=torch.Generator().manual_seed(seed), dtype=torch.float64), dim=-1)


@pytest.mark.parametrize("T,y", [(1, []), (1, [2]), (2, [1]), (7, [1, 2, 3]), (8, [2, 2, 1, 1]), (6, [2, 2, 1, 1]), (30, [3, 1, 4, 1, 5, 2])])
def test_frames_sum_to_one_and_nll_is_the_forward_value(T, y):
    lp = _lp(T, 6, 10 * T + len(y))
    nll, gamma, occ, peak, peak_t, bp = ctc_post_ref(lp.numpy(), y)
    assert np.abs(gamma.sum(axis=1) - 1.0).max() <= 1e-12
    assert abs(nll - ctc_nll_ref(lp, y)) <= 1e-12 * max(abs(nll), 1.0)
    assert abs(occ.sum() + bp.sum() - T) <= 1e-10 and np.all(peak_t >= 0) and np.all(peak <= 1.0 + 1e-12)


def test_no_path():
    nll, gamma, occ, peak, peak_t, bp = ctc_post_ref(_lp(5, 6, 1).numpy(), [2, 2, 1, 1])  # 6 frames needed
    assert nll == math.inf and not gamma.any() and not occ.any() and not peak.any() and list(peak_t) == [-1] * 4


def test_brute_force_over_all_labellings():
    """V = 3, T = 4, L = 2: gamma[t][s] is the posterior mass of the frame labellings whose path is in state s at t."""
    lp, y, T = _lp(4, 3, 7), [1, 2], 4
    want, total = np.zeros((T, 5)), 0.0
    for pi in itertools.product(range(3), repeat=T):
        if collapse(pi, 0) != y:
            continue
        p = math.exp(sum(float(lp[t, pi[t]]) for t in range(T)))
        total += p
        s = 0
        for t, v in enumerate(pi):  # the state of the path: tokens are distinct, so the label names it
            s = {1: 1, 2: 3}.get(v, s if s % 2 == 0 else s + 1)
            want[t, s] += p
    nll, gamma, *_ = ctc_post_ref(lp.numpy(), y)
    assert abs(nll + math.log(total)) <= 1e-12 and np.abs(gamma - want / total).max() <= 1e-12

