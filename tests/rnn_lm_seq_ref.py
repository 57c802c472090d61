"""Float64 restatement of ESPnetLanguageModel.nll (espnet2/lm/espnet_model.py:38-80) over a SequentialRNNLM of any of the four
cell kinds, torch gate order; plain torch on the CPU.  `LmParams(state_dict, rnn_type, round_to=torch.bfloat16)` restates on
the matrices as the device's bf16 mode holds them; nothing else is rounded."""
import torch

from tests import transducer_ref as R
from tests.transducer_lm_ref import LmParams, lm_step  # noqa: F401  (LmParams: the callers' constructor)


def step(p: LmParams, token: int, state):
    """The LM reads `token` from `state` -> (log-probabilities (V,), new state)."""
    if p.rnn_type in ("lstm", "gru"):
        return lm_step(p, token, state)[:2]
    x = p.embed[token]
    new = []
    for (w_ih, w_hh, b_ih, b_hh), st in zip(p.layers, state):
        g = (w_ih @ x + b_ih) + (w_hh @ st[0] + b_hh)
        x = torch.tanh(g) if p.rnn_type == "rnn_tanh" else torch.relu(g)
        new.append((x,))
    return R.log_softmax(p.out_w @ x + p.out_b), new


def nll(p: LmParams, text: torch.Tensor, lens: torch.Tensor):
    """text (B, L) int64, lens (B,) -> (nll (B, L + 1) float64, x_lengths (B,)): sentence b reads [sos | text[b]] from the
    zero state and position j scores text[b][j], position lens[b] scores eos (= sos = V - 1); 0.0 behind."""
    B, L = text.shape
    out = torch.zeros(B, L + 1, dtype=torch.float64)
    for b in range(B):
        state, tok = p.init_state(), p.sos
        for j in range(int(lens[b]) + 1):
            logp, state = step(p, tok, state)
            tok = int(text[b, j]) if j < int(lens[b]) else p.sos
            out[b, j] = -logp[tok]
    return out, lens + 1
