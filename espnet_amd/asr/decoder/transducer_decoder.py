"""TransducerDecoder: the prediction network of an RNN-T model as a decoder on the MI355X.

Mirrors espnet2/asr/decoder/transducer_decoder.py (constructor keywords; state-dict keys `embed.weight`,
`decoder.{l}.{weight,bias}_{ih,hh}_l0`: one single-layer torch.nn.LSTM / GRU per layer, input = hidden = hidden_size;
`init_state`, `score`, `batch_score`, `select_state`).  The torch.nn layers are parameter containers only: a step is
`em_transducer_dec_step` (csrc/transducer.hip) - embedding gather, the recurrent cells from caller-held states, then the
joint network's `lin_dec`, which is why `set_joint_network` hands the decoder its joint network.  The hidden size is
zero-padded to the GEMM K step at pack time like SequentialRNNLM's (hidden_size = 320 is a common recipe value), which
leaves every product unchanged.

A decoder state is what the device keeps for one hypothesis: (h in the compute dtype, f32 master state), each
(num_layers, padded hidden): the master state is the LSTM's c, the GRU's h (EmSearchBuffers.rnn_hs / rnn_cs layout).
"""
import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import torch

from espnet_amd import lib as L
from espnet_amd.packing import PackedModule

_KINDS = {"lstm": L.EM_LM_LSTM, "gru": L.EM_LM_GRU}


def pad64(v: int) -> int:
    return (v + 63) // 64 * 64


def padk(t: torch.Tensor, k: int) -> torch.Tensor:
    """Zero-pad the contraction dimension to k."""
    out = torch.zeros(t.size(0), k, dtype=torch.float32)
    out[:, : t.size(1)] = t.detach().to(torch.float32)
    return out


class TransducerDecoder(PackedModule):
    def __init__(self, vocab_size: int, rnn_type: str = "lstm", num_layers: int = 1, hidden_size: int = 320,
                 dropout: float = 0.0, dropout_embed: float = 0.0, embed_pad: int = 0,
                 compute_dtype: str = "bfloat16"):
        super().__init__()
        if rnn_type not in _KINDS:
            raise NotImplementedError(f"rnn_type={rnn_type!r}: the prediction network is lstm or gru")
        self.embed = torch.nn.Embedding(vocab_size, hidden_size, padding_idx=embed_pad)
        rnn = torch.nn.LSTM if rnn_type == "lstm" else torch.nn.GRU
        self.decoder = torch.nn.ModuleList([rnn(hidden_size, hidden_size, 1, batch_first=True) for _ in range(num_layers)])
        self.dlayers, self.dunits, self.dtype = num_layers, hidden_size, rnn_type
        self.odim, self.vocab_size = vocab_size, vocab_size
        self.ignore_id, self.blank_id = -1, embed_pad
        self.compute_dtype = compute_dtype
        self.joint_network = None

    @property
    def em_dtype(self) -> int:
        return L.DTYPES[self.compute_dtype]

    @property
    def dpad(self) -> int:
        return pad64(self.dunits)

    def set_joint_network(self, joint_network):
        """The joint network whose `lin_dec` closes a device step (a plain attribute: its parameters stay under
        `joint_network.` in the model's state dict)."""
        object.__setattr__(self, "joint_network", joint_network)

    def _build_pack(self, pk):
        A, F = pk.A, pk.F
        d, nh = self.dpad, self.dunits
        pk.embed = A(padk(self.embed.weight, d))
        layers = (L.EmRnnLayer * self.dlayers)()
        for l, rnn in enumerate(self.decoder):
            w_ih, w_hh, b_ih, b_hh = (getattr(rnn, k).detach().float().cpu()
                                      for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
            if self.dtype == "gru":  # r | z | n -> r | z | n_x | n_h (include/espnet_amd.h EmRnnLayer)
                zi, zh = torch.zeros(nh, w_ih.size(1)), torch.zeros(nh, w_hh.size(1))
                w_ih = torch.cat([w_ih, zi])
                w_hh = torch.cat([w_hh[: 2 * nh], zh, w_hh[2 * nh:]])
                b = torch.cat([b_ih[: 2 * nh] + b_hh[: 2 * nh], b_ih[2 * nh:], b_hh[2 * nh:]])
            else:
                b = b_ih + b_hh
            pk.fill(layers[l], dict(w_ih=A(padk(w_ih, d)), w_hh=A(padk(w_hh, d)), bias=F(b)))
        pk.layers = layers

    # ------------------------------------------------------------------ device step
    def weights(self, device):
        """(EmTransducerWeights, the packs it points into) for this decoder and its joint network on `device`."""
        if self.joint_network is None:
            raise RuntimeError("TransducerDecoder needs its joint network (set_joint_network) for a device step")
        device = torch.device(device)
        pd, pj = self.packed(device), self.joint_network.packed(device)
        key = (pd.serial, pj.serial)
        hit = self.__dict__.get("_weights")
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        w = L.EmTransducerWeights()
        w.kind, w.vocab, w.nhid, w.d, w.num_layers = _KINDS[self.dtype], self.vocab_size, self.dunits, self.dpad, self.dlayers
        w.joint, w.jp, w.blank = self.joint_network.joint_space_size, self.joint_network.jpad, self.blank_id
        w.embed = pd.embed.data_ptr()
        w.rnn = C.cast(pd.layers, C.POINTER(L.EmRnnLayer))
        w.lin_dec, w.lin_out, w.out_b = pj.lin_dec.data_ptr(), pj.lin_out.data_ptr(), pj.out_b.data_ptr()
        self.__dict__["_weights"] = (key, w, (pd, pj))
        return w, (pd, pj)

    def init_state(self, batch_size: int, device="cuda"):
        """Zero states for `batch_size` rows: (h, master), each (num_layers, batch_size, padded hidden).  The reference
        returns (h, c) of width H, with c None for gru; here the width is H padded to the GEMM K step and the second
        tensor is the f32 state the cells continue from (LSTM: c; GRU: h unrounded) - INTEGRATION.md, transducer."""
        return (torch.zeros(self.dlayers, batch_size, self.dpad, dtype=self.act_dtype, device=device),
                torch.zeros(self.dlayers, batch_size, self.dpad, dtype=torch.float32, device=device))

    @torch.no_grad()
    def step_device(self, tok: torch.Tensor, state, mask: Optional[torch.Tensor] = None, out=None):
        """`em_transducer_dec_step` for n rows: tok (n,) int32, state = (h, master) (layers, n, dpad).  Returns
        (dec_out (n, H) f32, dec_proj (n, jpad) f32, new state).  With `mask` (n,) int32 the rows with mask == 0 keep
        state and outputs: `out` = (dec_out, dec_proj) of the previous step is then required and updated in place."""
        hs, cs = state
        L.require_gpu(hs, "state")
        n, dev = int(tok.numel()), hs.device
        w, keep = self.weights(dev)
        hs_out, cs_out = torch.empty_like(hs), torch.empty_like(cs)
        if out is None:
            if mask is not None:
                raise ValueError("a masked step needs the previous outputs (`out`)")
            out = (torch.empty(n, self.dunits, dtype=torch.float32, device=dev),
                   torch.empty(n, w.jp, dtype=torch.float32, device=dev))
        L.check(L.load().em_transducer_dec_step(self.em_dtype, C.byref(w), L.ptr(tok), L.ptr(mask), n, L.ptr(hs), L.ptr(cs),
                                                L.ptr(hs_out), L.ptr(cs_out), L.ptr(out[0]), L.ptr(out[1]),
                                                L.current_stream_ptr()), "em_transducer_dec_step")
        return out[0], out[1], (hs_out, cs_out)

    @torch.no_grad()
    def teacher_forced_proj(self, ys: torch.Tensor, ylens: torch.Tensor, device=None) -> torch.Tensor:
        """The prediction network run over given transcripts: ys (N, Lmax) token ids, ylens (N,) -> dec_proj
        (Lmax + 1, N, jpad) f32 on the device, row (u, n) = lin_dec after candidate n has read blank, y_0 .. y_{u-1}
        (what `em_transducer_lattice_logp` reads).  Lmax + 1 enqueued calls of `em_transducer_dec_step` over all N rows,
        each writing its slice in place; the token column at u is blank at u = 0, then y_{u-1}, blank beyond a row's
        length (those rows' slices are never read).  No read-back."""
        if self.joint_network is None:
            raise RuntimeError("TransducerDecoder needs its joint network (set_joint_network) for a device step")
        ys = torch.as_tensor(ys)
        N, Lmax = int(ys.shape[0]), int(ys.shape[1])
        dev = torch.device(device) if device is not None else (ys.device if ys.is_cuda else torch.device("cuda"))
        ys = ys.to(dev, torch.long, non_blocking=True)
        lens = torch.as_tensor(ylens).to(dev, torch.long, non_blocking=True)
        cols = torch.full((Lmax + 1, N), self.blank_id, dtype=torch.long, device=dev)
        if Lmax > 0:
            inside = torch.arange(Lmax, device=dev).unsqueeze(0) < lens.unsqueeze(1)
            cols[1:] = torch.where(inside, ys, torch.full_like(ys, self.blank_id)).t()
        cols = cols.to(torch.int32).contiguous()
        w, keep = self.weights(dev)
        out = torch.empty(Lmax + 1, N, w.jp, dtype=torch.float32, device=dev)
        cur, nxt = self.init_state(N, dev), self.init_state(N, dev)
        lib, stream = L.load(), L.current_stream_ptr()
        for u in range(Lmax + 1):
            L.check(lib.em_transducer_dec_step(self.em_dtype, C.byref(w), L.ptr(cols[u]), None, N, L.ptr(cur[0]),
                                               L.ptr(cur[1]), L.ptr(nxt[0]), L.ptr(nxt[1]), None, L.ptr(out[u]), stream),
                    "em_transducer_dec_step")
            cur, nxt = nxt, cur
        return out

    # ------------------------------------------------------------------ the reference's decoder interface
    def select_state(self, states, idx: int):
        """The state of row idx of a batch of states, (layers, 1, dpad) each."""
        return (states[0][:, idx : idx + 1], states[1][:, idx : idx + 1])

    def create_batch_states(self, new_states: List[Tuple[torch.Tensor, torch.Tensor]]):
        return (torch.cat([s[0] for s in new_states], 1).contiguous(), torch.cat([s[1] for s in new_states], 1).contiguous())

    def score(self, hyp, cache: Dict[str, Any]):
        """One hypothesis: embeds hyp.yseq[-1] and runs the layers from hyp.dec_state.  Returns (dec_out (H,), new state,
        label (1,) tensor); `cache` is keyed by the label sequence and also keeps the row's lin_dec projection
        (`cache[key][2]`, what the joint primitive reads)."""
        key = "_".join(map(str, hyp.yseq))
        hit = cache.get(key)
        hs = hyp.dec_state[0]
        label = torch.full((1,), hyp.yseq[-1], dtype=torch.int32, device=hs.device)
        if hit is None:
            dec_out, dec_proj, state = self.step_device(label, (hs.contiguous(), hyp.dec_state[1].contiguous()))
            hit = cache[key] = (dec_out[0], state, dec_proj[0])
        return hit[0], hit[1], label

    def batch_score(self, hyps, dec_states=None, cache: Optional[Dict[str, Any]] = None, use_lm: bool = False):
        """A list of hypotheses in one launch (the rows the cache does not hold).  Returns (dec_out (n, H), batch of
        new states, labels (n,))."""
        cache = {} if cache is None else cache
        keys = ["_".join(map(str, h.yseq)) for h in hyps]
        todo = [i for i, k in enumerate(keys) if k not in cache]
        todo = [i for j, i in enumerate(todo) if keys[i] not in [keys[t] for t in todo[:j]]]
        dev = hyps[0].dec_state[0].device
        if todo:
            tok = torch.tensor([hyps[i].yseq[-1] for i in todo], dtype=torch.int32, device=dev)
            dec_out, dec_proj, st = self.step_device(tok, self.create_batch_states([hyps[i].dec_state for i in todo]))
            for j, i in enumerate(todo):
                cache[keys[i]] = (dec_out[j], self.select_state(st, j), dec_proj[j])
        labels = torch.tensor([h.yseq[-1] for h in hyps], dtype=torch.int32, device=dev)
        return (torch.stack([cache[k][0] for k in keys]), self.create_batch_states([cache[k][1] for k in keys]), labels)
