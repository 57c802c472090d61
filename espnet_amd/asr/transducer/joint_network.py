"""JointNetwork of a transducer model on the MI355X.

Mirrors espnet2/asr_transducer/joint_network.py (constructor keywords; state-dict keys `lin_enc.{weight,bias}`,
`lin_dec.weight`, `lin_out.{weight,bias}`): forward(enc, dec) = lin_out(tanh(lin_enc(enc) + lin_dec(dec))).  The
torch.nn layers are parameter containers only.  On the device the three Linears are apart: `enc_proj` is ONE em_gemm over
all frames of a batch, `lin_dec` closes the prediction network's step (em_transducer_dec_step) and tanh + `lin_out` +
log-softmax are `em_transducer_joint_logp`, or the vocabulary-tile launch of the fused greedy walk
(em_transducer_greedy).  The joint space is zero-padded to the GEMM K step at pack time.
"""
import ctypes as C

import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.transducer_decoder import pad64, padk
from espnet_amd.packing import PackedModule


class JointNetwork(PackedModule):
    def __init__(self, output_size: int, encoder_size: int, decoder_size: int, joint_space_size: int = 256,
                 joint_activation_type: str = "tanh", compute_dtype: str = "bfloat16", **activation_parameters):
        super().__init__()
        if joint_activation_type != "tanh":
            raise NotImplementedError(f"joint_activation_type={joint_activation_type!r}: only tanh is on the device path")
        if encoder_size % 64 != 0:  # (lin_enc is one em_gemm on the encoder's own rows, which are not K-padded)
            raise NotImplementedError(f"encoder_size={encoder_size}: the joint network's lin_enc runs for encoder widths "
                                      "that are multiples of 64")
        self.lin_enc = torch.nn.Linear(encoder_size, joint_space_size)
        self.lin_dec = torch.nn.Linear(decoder_size, joint_space_size, bias=False)
        self.lin_out = torch.nn.Linear(joint_space_size, output_size)
        self.output_size, self.encoder_size, self.decoder_size = output_size, encoder_size, decoder_size
        self.joint_space_size = joint_space_size
        self.compute_dtype = compute_dtype

    @property
    def em_dtype(self) -> int:
        return L.DTYPES[self.compute_dtype]

    @property
    def jpad(self) -> int:
        return pad64(self.joint_space_size)

    def _build_pack(self, pk):
        jp, J = self.jpad, self.joint_space_size
        w_enc = torch.zeros(jp, self.encoder_size)
        w_enc[:J] = self.lin_enc.weight.detach().float().cpu()
        b_enc = torch.zeros(jp)
        b_enc[:J] = self.lin_enc.bias.detach().float().cpu()
        pk.lin_enc, pk.enc_b = pk.A(w_enc), pk.F(b_enc)
        pk.lin_dec = pk.A(padk(self.lin_dec.weight, pad64(self.decoder_size)))
        pk.lin_out, pk.out_b = pk.A(padk(self.lin_out.weight, jp)), pk.F(self.lin_out.bias)

    @torch.no_grad()
    def enc_proj_device(self, enc_act: torch.Tensor) -> torch.Tensor:
        """lin_enc(enc) + bias for all frames at once: enc_act (..., D) in the compute dtype -> (..., jpad) f32."""
        L.require_gpu(enc_act, "enc_act")
        if enc_act.dtype != self.act_dtype:
            enc_act = enc_act.to(self.act_dtype)
        enc_act = enc_act.contiguous()
        D = enc_act.shape[-1]
        if D != self.encoder_size:
            raise ValueError(f"enc_act has width {D}, the joint network was built for encoder_size={self.encoder_size}")
        M = enc_act.numel() // D
        p = self.packed(enc_act.device)
        out = torch.empty(*enc_act.shape[:-1], self.jpad, dtype=torch.float32, device=enc_act.device)
        a = L.EmGemmArgs(A=enc_act.data_ptr(), W=p.lin_enc.data_ptr(), C=out.data_ptr(), bias=p.enc_b.data_ptr(), M=M,
                         N=self.jpad, K=D, lda=D, ldc=self.jpad, scale=1.0)
        L.check(L.load().em_gemm(self.em_dtype, L.EM_EPI_SCALE_F32, L.EM_A_PLAIN, a, L.current_stream_ptr()),
                "em_gemm(joint lin_enc)")
        return out

    @torch.no_grad()
    def logp_device(self, decoder, enc_proj, dec_proj, enc_idx=None, dec_idx=None) -> torch.Tensor:
        """`em_transducer_joint_logp`: log_softmax(lin_out(tanh(enc_proj[enc_idx] + dec_proj[dec_idx]))) (n, V) f32 for n
        pairs of rows (an index vector of None: row r itself)."""
        dev = enc_proj.device
        n = int(enc_idx.numel()) if enc_idx is not None else int(dec_idx.numel()) if dec_idx is not None else int(enc_proj.shape[0])
        w, keep = decoder.weights(dev)
        z = torch.empty(n, self.jpad, dtype=self.act_dtype, device=dev)
        logp = torch.empty(n, self.output_size, dtype=torch.float32, device=dev)
        L.check(L.load().em_transducer_joint_logp(self.em_dtype, C.byref(w), L.ptr(enc_proj), L.ptr(enc_idx), L.ptr(dec_proj),
                                                  L.ptr(dec_idx), n, L.ptr(z), L.ptr(logp), L.current_stream_ptr()),
                "em_transducer_joint_logp")
        return logp

    # ------------------------------------------------------------------ likelihood of given transcripts (csrc/transducer_nll.hip)
    def lattice_workspace_bytes(self, decoder, device, N: int, T: int, Lmax: int) -> int:
        """`em_transducer_lattice_logp_workspace_bytes`: 0 when the shape is not covered in one call."""
        w, keep = decoder.weights(device)
        return int(L.load().em_transducer_lattice_logp_workspace_bytes(self.em_dtype, C.byref(w), N, T, Lmax))

    @torch.no_grad()
    def lattice_logp_device(self, decoder, enc_proj, xlens, dec_proj, targets, ylens, mem_of=None, out=None, ws=None):
        """`em_transducer_lattice_logp`: the blank's and the next label's log-probability at every node (t < xlens[m],
        u <= ylens[n]) of N candidates' lattices, lat (N, T, Lmax + 1, 2) f32; the other nodes are not written.
        enc_proj (Bm, T, jpad) f32 (`enc_proj_device`), xlens (Bm,) int32, dec_proj (Lmax + 1, N, jpad) f32
        (`TransducerDecoder.teacher_forced_proj`), targets (N, Lmax) int32, ylens (N,) int32, mem_of (N,) int32 or None,
        all on the device.  `out`: a lattice to write into; `ws`: a uint8 workspace (default: one of the size the library
        asks for)."""
        L.require_gpu(enc_proj, "enc_proj")
        dev = enc_proj.device
        Bm, T = int(enc_proj.shape[0]), int(enc_proj.shape[1])
        N, Lmax = int(dec_proj.shape[1]), int(dec_proj.shape[0]) - 1
        w, keep = decoder.weights(dev)
        lib = L.load()
        if ws is None:
            need = int(lib.em_transducer_lattice_logp_workspace_bytes(self.em_dtype, C.byref(w), N, T, Lmax))
            if need == 0:
                raise NotImplementedError(f"em_transducer_lattice_logp: {N} candidates x {T} frames x {Lmax} tokens are "
                                          "outside the shapes of one call")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        lat = out if out is not None else torch.empty(N, T, Lmax + 1, 2, dtype=torch.float32, device=dev)
        L.check(lib.em_transducer_lattice_logp(self.em_dtype, C.byref(w), L.ptr(enc_proj), L.ptr(xlens), Bm, T, L.ptr(dec_proj),
                                               L.ptr(targets), Lmax, L.ptr(ylens), L.ptr(mem_of), N, L.ptr(lat), L.ptr(ws),
                                               int(ws.numel()), L.current_stream_ptr()), "em_transducer_lattice_logp")
        return lat

    @torch.no_grad()
    def seq_nll_device(self, lat, xlens, ylens, mem_of=None) -> torch.Tensor:
        """`em_transducer_seq_nll`: the forward recursion over lat (N, T, Lmax + 1, 2) f32 -> -log p(y | x), (N,) f32;
        +inf for a candidate whose utterance has no frame.  xlens (Bm,), ylens (N,), mem_of (N,) or None: int32, device."""
        L.require_gpu(lat, "lat")
        N, T, Lmax = int(lat.shape[0]), int(lat.shape[1]), int(lat.shape[2]) - 1
        nll = torch.empty(N, dtype=torch.float32, device=lat.device)
        L.check(L.load().em_transducer_seq_nll(L.ptr(lat), L.ptr(xlens), int(xlens.numel()), T, Lmax, L.ptr(ylens),
                                               L.ptr(mem_of), N, L.ptr(nll), L.current_stream_ptr()), "em_transducer_seq_nll")
        return nll

    @torch.no_grad()
    def seq_align_device(self, lat, xlens, ylens, mem_of=None, ws=None):
        """`em_transducer_seq_align`: the best path through lat (N, T, Lmax + 1, 2) f32 and its back-trace.  Returns device
        tensors (tok_frame (N, Lmax) int32: the frame at which token u is emitted, -1 behind the transcript; tok_logp
        (N, Lmax) f32: the label's log-probability there, 0 behind it; frame_u (N, T) int32: the tokens emitted when the
        path leaves frame t, -1 behind the utterance; total (N,) f32: the path's log-probability, -inf without a path).
        xlens (Bm,), ylens (N,), mem_of (N,) or None: int32, device.  `ws`: a uint8 workspace for the back-pointers
        (default: one of the size the library asks for)."""
        L.require_gpu(lat, "lat")
        dev = lat.device
        N, T, Lmax = int(lat.shape[0]), int(lat.shape[1]), int(lat.shape[2]) - 1
        lib = L.load()
        if ws is None:
            ws = torch.empty(max(int(lib.em_transducer_seq_align_workspace_bytes(N, T, Lmax)), 1), dtype=torch.uint8,
                             device=dev)
        tok_frame = torch.empty(N, Lmax, dtype=torch.int32, device=dev)
        tok_logp = torch.empty(N, Lmax, dtype=torch.float32, device=dev)
        frame_u = torch.empty(N, T, dtype=torch.int32, device=dev)
        total = torch.empty(N, dtype=torch.float32, device=dev)
        L.check(lib.em_transducer_seq_align(L.ptr(lat), L.ptr(xlens), int(xlens.numel()), T, Lmax, L.ptr(ylens),
                                            L.ptr(mem_of), N, L.ptr(tok_frame), L.ptr(tok_logp), L.ptr(frame_u),
                                            L.ptr(total), L.ptr(ws), int(ws.numel()), L.current_stream_ptr()),
                "em_transducer_seq_align")
        return tok_frame, tok_logp, frame_u, total

    @torch.no_grad()
    def forward(self, enc_out: torch.Tensor, dec_out: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("JointNetwork.forward on broadcast (B, T, U) lattices is training only; decoding goes "
                                  "through enc_proj_device / em_transducer_joint_logp")
