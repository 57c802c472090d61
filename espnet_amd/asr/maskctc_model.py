"""MaskCTCModel (inference side) on the MI355X.

Mirrors espnet2/asr/maskctc_model.py MaskCTCModel for what decoding touches: the ESPnetASRModel attributes with the
vocabulary extended by `<mask>` (`vocab_size = V + 1`, `mask_token = V`, `token_list[-1] = "<mask>"`; the CTC head keeps the V
original labels), and the decoding procedure of MaskCTCInference for a ragged BATCH, on the device:

  greedy CTC with the frames' winning probabilities   CTC.frame_top_device       (em_ctc_frame_top)
  collapse with confidence, threshold                 em_maskctc_collapse
  K mask-predict passes of the MLM decoder            MLMDecoder.refine_device   (em_maskctc_refine)

One read-back (the token and mask counts of the batch) sits between the collapse and the refinement: it sizes the rows of
the decoder passes to the longest token sequence instead of T, and lets a batch without a masked token return at once.
Training (the masking of targets, the MLM loss) is out of scope.
"""
import torch

from espnet_amd import lib as L
from espnet_amd.asr.decoder.mlm_decoder import MLMDecoder
from espnet_amd.asr.espnet_model import EncoderState, ESPnetASRModel


class MaskCTCModel(ESPnetASRModel):
    def __init__(self, vocab_size: int, token_list, frontend, specaug, normalize, preencoder, encoder, postencoder,
                 decoder, ctc, joint_network=None, sym_mask: str = "<mask>", **kw):
        if joint_network is not None:
            raise NotImplementedError("MaskCTCModel with a joint network")
        if not isinstance(decoder, MLMDecoder):
            raise ValueError(f"MaskCTCModel needs an MLMDecoder (decoder: mlm), got {type(decoder).__name__}")
        token_list = list(token_list) + [sym_mask]  # maskctc_model.py: vocab_size += 1; token_list.append(sym_mask)
        vocab_size += 1
        super().__init__(vocab_size=vocab_size, token_list=token_list, frontend=frontend, specaug=specaug, normalize=normalize,
                         preencoder=preencoder, encoder=encoder, postencoder=postencoder, decoder=decoder, ctc=ctc, **kw)
        if self.ctc is None or self.decoder is None:
            raise ValueError("MaskCTCModel needs the CTC head and the decoder (0 < ctc_weight < 1)")
        if decoder.vocab_size != vocab_size or ctc.odim != vocab_size - 1:
            raise ValueError(f"MaskCTCModel: {vocab_size - 1} labels need a CTC head of {vocab_size - 1} and a decoder of "
                             f"{vocab_size} outputs, got {ctc.odim} and {decoder.vocab_size}")
        self.mask_token = vocab_size - 1

    @torch.no_grad()
    def decode_maskctc_device(self, st: EncoderState, n_iterations: int = 10, threshold_probability: float = 0.99,
                              trace: bool = False, ws: torch.Tensor = None):
        """MaskCTCInference.forward for the encoded batch `st` (`encode_device`).  Returns device tensors
          y      (B, Lp) int32  the decoded tokens, -1 behind an utterance's length (Lp: the batch's longest, at least 1);
          ylens  (B,)    int32  the token counts;
          tokens (B, Lp) int32  the greedy CTC tokens the decoding started from, -1 behind the length;
          conf   (B, Lp) f32    their confidences (the largest frame probability of each token's run), 0 behind it;
        with `trace` a fifth entry: None when no pass ran, else (y_in before the first pass, y after each pass (K, B, Lp),
        each pass's max logits and arg-max (K, B, Lp)).  An utterance's result does not depend on its companions."""
        return self._decode_maskctc(st.enc_out, st.olens_dev, n_iterations, threshold_probability, trace, ws)

    def collapse_device(self, ids: torch.Tensor, prob: torch.Tensor, olens_dev: torch.Tensor, threshold_probability: float):
        """`em_maskctc_collapse` on what `CTC.frame_top_device` returned: ids / prob (B, T), olens_dev (B,) int32 ->
        (tokens (B, T) int32, conf (B, T) f32, y_in (B, T) int32, counts (2, B) int32 = token counts | masked counts), all
        written whole (-1 / 0 behind the counts).  Only enqueues."""
        B, T = ids.shape
        i32 = dict(dtype=torch.int32, device=ids.device)
        tokens, y_in = torch.empty(B, T, **i32), torch.empty(B, T, **i32)
        conf = torch.empty(B, T, dtype=torch.float32, device=ids.device)
        counts = torch.empty(2, B, **i32)
        L.check(L.load().em_maskctc_collapse(L.ptr(ids), L.ptr(prob), L.ptr(olens_dev), B, T, T, self.blank_id,
                                             self.mask_token, float(threshold_probability), L.ptr(tokens), L.ptr(conf),
                                             L.ptr(y_in), L.ptr(counts[0]), L.ptr(counts[1]), L.current_stream_ptr()),
                "em_maskctc_collapse")
        return tokens, conf, y_in, counts

    def _decode_maskctc(self, enc_out, olens_dev, n_iterations, threshold_probability, trace=False, ws=None):
        K = int(n_iterations)
        if K < 1:
            raise NotImplementedError(f"maskctc_n_iterations={K}: the reference then fills one token per pass without a "
                                      "bound; the device chain has a fixed length (>= 1)")
        L.require_gpu(enc_out, "enc_out")
        ids, prob = self.ctc.frame_top_device(enc_out)
        tokens, conf, y_in, counts = self.collapse_device(ids, prob, olens_dev, threshold_probability)
        host = counts.cpu()  # the one read-back: the longest token sequence and whether anything is masked
        Lp = max(int(host[0].max()), 1)
        y = y_in[:, :Lp].contiguous()
        out = (y, counts[0], tokens[:, :Lp], conf[:, :Lp])
        tr = None
        if int(host[1].max()) > 0:
            y0 = y.clone() if trace else None
            tr = self.decoder.refine_device(enc_out, olens_dev, y, counts[0], counts[1], K, trace=trace, ws=ws)
            tr = (y0,) + tr if trace else None
        return out + (tr,) if trace else out
