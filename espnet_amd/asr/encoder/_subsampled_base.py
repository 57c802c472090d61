"""The host layer the batch encoders share (ConformerEncoder, EBranchformerEncoder / BranchformerEncoder,
TransformerEncoder), the batch counterpart of `_contextual_block_base.py`: a Conv2dSubsampling front, a stack of layers,
`after_norm`, and one C-ABI call per batch that differs in its entry point, its weights struct and its positional operand.

The base owns the common constructor state, the subsampling / embed / after_norm part of the pack, the rel-pos tables,
`forward_device` (short-utterance check, the `olens` cache, one workspace per stream, the flags every entry point reads) and
a generic `unsupported_options`.  A subclass supplies its parameter containers, `_option_check`, `_build_pack`, the names
of its two C entries, and overrides two hooks where it differs:
  - `_call_operands`: the positional operand of this call plus the flags of its own (default: the rel-pos table, no flag);
  - `_ctc_ids_plan`: a context around the C call that arranges per-frame CTC ids (default: none, `last_ctc_ids` is None).
"""
import contextlib
import ctypes as C
import inspect
import math
import os
from typing import List, Optional, Tuple

import torch

from espnet_amd import lib as L
from espnet_amd.nets_utils import (SUBSAMPLING_CONVS, SUBSAMPLING_MIN_FRAMES, conv2d_subsampled_lengths,
                                   conv_out_size)
from espnet_amd.packing import PackedModule

LN_EPS = 1e-12  # transformer/layer_norm.py:23


class LayerNorm(torch.nn.LayerNorm):
    def __init__(self, nout):
        super().__init__(nout, eps=LN_EPS)


class _Conv2dSubsampling(torch.nn.Module):
    """Parameters of Conv2dSubsampling / Conv2dSubsampling6 / Conv2dSubsampling8
    (transformer/subsampling.py:386-409, 692-715, 785-808): `conv.{0,2[,4]}`, `out`."""

    def __init__(self, idim, odim, input_layer: str = "conv2d"):
        super().__init__()
        mods, cin = [], 1
        for k, s in SUBSAMPLING_CONVS[input_layer]:
            mods += [torch.nn.Conv2d(cin, odim, k, s), torch.nn.ReLU()]
            cin = odim
        self.conv = torch.nn.Sequential(*mods)
        self.out = torch.nn.Linear(odim * conv_out_size(idim, input_layer), odim)


def _fused_enabled(enc) -> bool:
    """The fused per-block kernels are the default where they apply; `enc.fused = False` or
    ESPNET_AMD_FUSED=0 keeps the one-operator-per-launch sequence (A/B measurements, bisecting)."""
    return bool(getattr(enc, "fused", True)) and os.environ.get("ESPNET_AMD_FUSED", "1") != "0"


def pack_conv1_frags(w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """conv.0 weight [256][9] + bias [256] (f32) -> the MFMA operand of the fused conv1 + conv2 kernel (include/espnet_amd.h,
    em_conv2d_sub12_bf16): per channel 32 bf16 k-slots  hi(w) | hi(w) | lo(w) | hi(b), lo(b), 0, 0, 0  with hi(x) = bf16(x),
    lo(x) = bf16(x - hi(x)), laid out [chunk][fragment][lg][lr][e] for channel 32 cc + 16 f + lr, k = 8 lg + e."""
    w1 = w1.detach().to(torch.float32).cpu().reshape(-1, 9)
    b1 = b1.detach().to(torch.float32).cpu()
    d = w1.shape[0]
    assert d % 32 == 0, d

    def hi(x):
        return x.to(torch.bfloat16).to(torch.float32)

    wh, bh = hi(w1), hi(b1)
    wl, bl = hi(w1 - wh), hi(b1 - bh)
    k = torch.zeros(d, 32)
    k[:, 0:9], k[:, 9:18], k[:, 18:27], k[:, 27], k[:, 28] = wh, wh, wl, bh, bl
    return k.reshape(d // 32, 2, 16, 4, 8).permute(0, 1, 3, 2, 4).contiguous().reshape(-1)


def pack_conv2_frags(w2: torch.Tensor) -> torch.Tensor:
    """conv.2 weight as [256][9 * 256] with column (kt*3 + kf) * 256 + c_in -> fragment-major
    [chunk cc][tap][wave w][fragment j][lg][lr][e] = w2[64 w + 16 (lr // 4) + 4 j + lr % 4][tap * 256 + 32 cc + 8 lg + e]:
    MFMA row lr of a wave's fragment j is an output channel chosen so that a lane's 16 results of a position
    (4 fragments x 4 rows) are 16 CONSECUTIVE channels - two 16-byte stores instead of four 8-byte ones."""
    n, k = w2.shape
    assert n % 256 == 0 and k == 9 * n, (n, k)  # (d = 512: one block of this layout per 256 output channels, 16 chunks each)
    halves = []
    for h0 in range(0, n, 256):
        u = w2.detach()[h0 : h0 + 256].reshape(4, 4, 4, 4, 9, n // 32, 4, 8)  # [w][q = lr // 4][j][r = lr % 4][tap][cc][lg][e]
        halves.append(u.permute(5, 4, 0, 2, 6, 1, 3, 7).contiguous().reshape(-1))
    return torch.cat(halves)


def rel_pos_table(T: int, d: int) -> torch.Tensor:
    """RelPositionalEncoding rows for a length-T input (embedding.py:286-332): row k is the
    sinusoid of relative position T-1-k.  Built on the host with the same fp32 torch ops the
    reference uses (`extend_pe`), once per distinct T."""
    pe_positive = torch.zeros(T, d)
    pe_negative = torch.zeros(T, d)
    position = torch.arange(0, T, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe_positive[:, 0::2] = torch.sin(position * div_term)
    pe_positive[:, 1::2] = torch.cos(position * div_term)
    pe_negative[:, 0::2] = torch.sin(-1 * position * div_term)
    pe_negative[:, 1::2] = torch.cos(-1 * position * div_term)
    return torch.cat([torch.flip(pe_positive, [0]), pe_negative[1:]], dim=0)


def resolve_rel_pos(rel_pos_type: str, pos_enc_layer_type: str, attention_layer_type: str) -> Tuple[str, str, bool]:
    """conformer_encoder.py:127-136, e_branchformer_encoder.py:226-235, branchformer_encoder.py:330-339: rel_pos_type
    "legacy" turns rel_pos / rel_selfattn into their legacy_ forms -> (the two layer types as the reference resolves
    them, whether both are the legacy ones)."""
    if rel_pos_type == "legacy":
        pos_enc_layer_type = "legacy_rel_pos" if pos_enc_layer_type == "rel_pos" else pos_enc_layer_type
        attention_layer_type = "legacy_rel_selfattn" if attention_layer_type == "rel_selfattn" else attention_layer_type
    elif rel_pos_type != "latest":
        raise ValueError("unknown rel_pos_type: " + rel_pos_type)
    legacy = pos_enc_layer_type == "legacy_rel_pos" and attention_layer_type == "legacy_rel_selfattn"
    return pos_enc_layer_type, attention_layer_type, legacy


def rows_ffn_packable(act_dtype: torch.dtype, d: int, ff) -> bool:
    """Shapes whose feed-forward modules the row-block launches take (csrc/ffn_rows.hip): the host packs their operand
    streams for these.  Mirrors the shape part of em_host::rows_ffn_ok (csrc/enc_host.h), which decides per call."""
    return act_dtype == torch.bfloat16 and d == 512 and bool(ff) and ff % 128 == 0 and ff >= 256


class SubsampledEncoderBase(PackedModule):
    _WS_FN, _ENC_FN = None, None  # C-ABI entry points of forward_device (include/espnet_amd.h)
    last_ctc_ids = None           # per-frame CTC arg-max ids of the last call: only an encoder with a CTC-ids plan has any

    def __init__(self, input_size: int, output_size: int, attention_heads: int, linear_units, num_blocks: int,
                 input_layer: str, compute_dtype: str, layer, legacy_relpos: bool = False, max_pos_emb_len: int = 5000):
        """`layer()` builds the parameter container of one block."""
        super().__init__()
        self._output_size, self._input_size = output_size, input_size
        self.heads, self.linear_units, self.num_blocks = attention_heads, linear_units, num_blocks
        self.interctc_layer_idx, self.interctc_use_conditioning = [], False
        self.compute_dtype = compute_dtype
        self.input_layer = input_layer
        self.legacy_relpos, self.max_pos_emb_len = legacy_relpos, max_pos_emb_len
        self.embed = _Conv2dSubsampling(input_size, output_size, input_layer)
        self.encoders = torch.nn.ModuleList([layer() for _ in range(num_blocks)])
        self.after_norm = LayerNorm(output_size)
        self._pos_cache, self._ws, self._olens_cache = {}, {}, {}

    # ------------------------------------------------------------------ options
    @staticmethod
    def _option_check(**options):
        """The constructor options the MI355X kernels do not cover -> (list of "name=value" strings, legacy rel-pos flag
        or None).  An empty list = the fast path applies.  Its keyword names are constructor parameter names."""
        raise NotImplementedError

    @classmethod
    def _unsupported(cls, args: dict):
        """`_option_check` on the constructor arguments `args` (a constructor passes its `locals()`), in front of its list
        the keywords the reference class does not take (collected by a constructor's `**unsupported`)."""
        foreign = [f"{k}={v!r} (not a {cls.__name__} keyword)" for k, v in args.get("unsupported", {}).items()]
        bad, legacy = cls._option_check(**{k: args[k] for k in inspect.signature(cls._option_check).parameters})
        return foreign + bad, legacy

    @classmethod
    def unsupported_options(cls, *args, **kwargs) -> List[str]:
        """The constructor arguments (positional or keyword, reference defaults applied; keywords the reference class does
        not take included) that fall outside the fast path, without building anything: what
        `espnet_amd.integration.espnet2_adapters` consults to hand such a configuration to the stock espnet2 class under
        the same yaml name."""
        ba = inspect.signature(cls.__init__).bind(None, *args, **kwargs)
        ba.apply_defaults()
        try:
            return cls._unsupported(ba.arguments)[0]
        except ValueError as e:
            return [str(e)]

    def output_size(self) -> int:
        return self._output_size

    # ------------------------------------------------------------------ packing (load time)
    @property
    def em_dtype(self) -> int:
        return L.DTYPES[self.compute_dtype]

    def invalidate(self):
        super().invalidate()
        self._pos_cache = {}

    def _pack_embed(self, pk, w) -> dict:
        """The tensors of the subsampling front and `after_norm`, which every weights struct names alike; sets
        `w.subsample` / `w.legacy_relpos`.  The caller adds its own and fills `w`."""
        A, F = pk.A, pk.F
        e, d = self.embed, self._output_size
        F2 = e.out.in_features // d
        t = {}
        t["conv1_w"] = F(e.conv[0].weight.reshape(d, 9))
        t["conv1_b"] = F(e.conv[0].bias)
        self._pack_subsampling(w, t, A, F)
        t["embed_w"] = A(e.out.weight.reshape(d, d, F2).permute(0, 2, 1).reshape(d, F2 * d))
        t["embed_b"] = F(e.out.bias)
        t["after_norm_g"], t["after_norm_b"] = F(self.after_norm.weight), F(self.after_norm.bias)
        return t

    def _pack_subsampling(self, w, t, A, F):
        """conv.2 (and conv.4): [d][k*k*d] with column (kt*k + kf)*d + c_in, the implicit GEMM's K order."""
        e, d = self.embed, self._output_size
        layer = self.input_layer
        w.subsample = {"conv2d": 4, "conv2d6": 6, "conv2d8": 8}[layer]
        w.legacy_relpos = int(self.legacy_relpos)
        k2 = e.conv[2].weight.size(-1)
        t["conv2_w"] = A(e.conv[2].weight.permute(0, 2, 3, 1).reshape(d, k2 * k2 * d))
        t["conv2_b"] = F(e.conv[2].bias)
        if layer == "conv2d" and d in (256, 512) and self.em_dtype == L.EM_BF16:
            # operands of the fused conv1 + conv2 kernel (csrc/subsample2.hip): the conv1 map is never materialised
            t["conv1_wf"] = A(pack_conv1_frags(e.conv[0].weight, e.conv[0].bias))
            t["conv2_wf"] = A(pack_conv2_frags(e.conv[2].weight.permute(0, 2, 3, 1).reshape(d, 9 * d)))
        if layer == "conv2d8":
            t["conv3_w"] = A(e.conv[4].weight.permute(0, 2, 3, 1).reshape(d, 9 * d))
            t["conv3_b"] = F(e.conv[4].bias)

    # ------------------------------------------------------------------ positional tables
    def _pos_emb(self, T: int, device) -> torch.Tensor:
        """(2T-1, d) rows for a length-T input: a contiguous row slice of one table built for a maximum
        length, exactly as the reference slices its `pe` buffer (embedding.py:329-332).  Row k of the
        slice is the sinusoid of relative position T-1-k whatever the table length, so the values are
        bit-identical to a table built for T; the table grows by doubling (built once per size)."""
        if self.legacy_relpos:
            return self._legacy_pos_emb(T, device)
        key = (str(device), self.em_dtype)
        tab = self._pos_cache.get(key)
        if tab is None or tab[0] < T:
            tmax = max(512, tab[0] * 2 if tab else 0)
            while tmax < T:
                tmax *= 2
            tab = (tmax, rel_pos_table(tmax, self._output_size).to(self.act_dtype).to(device))
            self._pos_cache[key] = tab
        tmax, table = tab
        return table[tmax - T : tmax + T - 1]

    def _legacy_pos_emb(self, T: int, device) -> torch.Tensor:
        """(T, d): LegacyRelPositionalEncoding rows (embedding.py:223-262 over PositionalEncoding(reverse=True)
        :50-82): the reference builds positions max_len-1 .. 0 once and uses the first T rows, so row k is the
        sinusoid of position max_len-1-k — a prefix of one table (rebuilt longer like `extend_pe` if needed)."""
        key = ("legacy", str(device), self.em_dtype)
        tab = self._pos_cache.get(key)
        if tab is None or tab.size(0) < T:
            n = max(T, self.max_pos_emb_len)
            d = self._output_size
            position = torch.arange(n - 1, -1, -1.0, dtype=torch.float32).unsqueeze(1)
            div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
            pe = torch.zeros(n, d)
            pe[:, 0::2] = torch.sin(position * div_term)
            pe[:, 1::2] = torch.cos(position * div_term)
            tab = pe.to(self.act_dtype).to(device)
            self._pos_cache[key] = tab
        return tab[:T]

    # ------------------------------------------------------------------ hooks
    def _call_operands(self, T: int, dev, pk) -> Tuple[torch.Tensor, int]:
        """(the positional operand of a call on T output frames, the flags of the subclass's own for it)."""
        return self._pos_emb(T, dev), 0

    def _ctc_ids_plan(self, w, enc_flags: int, B: int, T: int, T_f: int, dev):
        """A context the C call runs in; an encoder whose launch sequence can hand back per-frame CTC ids arranges them
        here and publishes them as `last_ctc_ids`."""
        return contextlib.nullcontext()

    # ------------------------------------------------------------------ forward
    def output_frames(self, T_f: int) -> int:
        return conv_out_size(T_f, self.input_layer)

    def forward_device(self, feats: torch.Tensor, flens: List[int], flens_dev: torch.Tensor,
                       mvn_partial: Optional[torch.Tensor] = None, isolate: bool = False):
        """feats (B,T_f,D) f32 on the GPU.  Returns (enc_out f32 (B,T,d), enc_act (B,T,d) in the
        compute dtype, olens list, olens_dev i32)."""
        L.require_gpu(feats, "feats")
        B, T_f, D = feats.shape
        # check_short_utt (subsampling.py:31-49) via conformer_encoder.py:360-369; the reference sees one
        # utterance per call, so in a padded batch every row is held to the same limit
        layer = self.input_layer
        lim = SUBSAMPLING_MIN_FRAMES[layer]
        short = [b for b, n in enumerate(flens) if n < lim] if T_f >= lim else list(range(B))
        if short:
            n0 = min(T_f, int(flens[short[0]]))
            raise L.TooShortUttError(
                f"has {n0} frames and is too short for subsampling "
                f"(it needs more than {lim} frames), return empty results", n0, lim, indices=short)
        dev = feats.device
        pk = self.packed(dev)
        w = pk.w
        lib = L.load()
        T = self.output_frames(T_f)
        if isolate:  # every utterance as if it were the whole batch: tmax = its own length
            olens = [conv2d_subsampled_lengths([n], int(n), layer)[0] for n in flens]
        else:  # the padded mask is sliced, so padded rows keep up to two frames more (subsampling.py:448)
            olens = conv2d_subsampled_lengths(flens, T_f, layer)
        okey = (tuple(olens), dev)
        olens_dev = self._olens_cache.get(okey)
        if olens_dev is None:  # kept on the device for repeating batch shapes (see encode_device)
            olens_dev = torch.tensor(olens, dtype=torch.int32).to(dev, non_blocking=True)
            if len(self._olens_cache) >= 8:
                self._olens_cache.pop(next(iter(self._olens_cache)))
            self._olens_cache[okey] = olens_dev
        need = getattr(lib, self._WS_FN)(self.em_dtype, C.byref(w), B, T_f)
        # one workspace per stream: independent utterance batches may be encoded concurrently on
        # different HIP streams
        skey = torch.cuda.current_stream().cuda_stream
        ws = self._ws.get(skey)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._ws[skey] = ws
        d = self._output_size
        enc_out = torch.empty(B, T, d, dtype=torch.float32, device=dev)
        enc_act = torch.empty(B, T, d, dtype=self.act_dtype, device=dev)
        enc_flags = (L.EM_ENC_ISOLATE_UTTS if isolate else 0) | (0 if _fused_enabled(self) else L.EM_ENC_NO_FUSED)
        # batches the caller keeps in flight on other HIP streams (bench.py's StepPipeline, the decode CLI's lanes set the
        # attribute): the library takes the 512-wide models' row-block launches from a smaller share of the chip then
        enc_flags |= L.EM_ENC_IN_FLIGHT(max(1, min(15, int(getattr(self, "batches_in_flight", 1) or 1))))
        pos, own_flags = self._call_operands(T, dev, pk)
        enc_flags |= own_flags
        with self._ctc_ids_plan(w, enc_flags, B, T, T_f, dev):
            rc = getattr(lib, self._ENC_FN)(
                self.em_dtype, C.byref(w), L.ptr(feats), L.ptr(mvn_partial), L.ptr(flens_dev),
                L.ptr(olens_dev), B, T_f, L.ptr(pos), L.ptr(ws),
                ws.numel(), L.ptr(enc_out), L.ptr(enc_act),
                enc_flags, L.current_stream_ptr())
        L.check(rc, self._ENC_FN)
        return enc_out, enc_act, olens, olens_dev

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states: torch.Tensor = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        flens = [int(v) for v in ilens.tolist()]
        flens_dev = torch.tensor(flens, dtype=torch.int32).to(xs_pad.device, non_blocking=True)
        enc_out, _, olens, _ = self.forward_device(xs_pad.to(torch.float32).contiguous(), flens,
                                                   flens_dev, None)
        return enc_out, torch.tensor(olens, dtype=torch.long, device=xs_pad.device), None
