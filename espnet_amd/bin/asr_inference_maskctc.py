#!/usr/bin/env python3
"""Mask-CTC decoding on the MI355X: `MaskCTCInference`, `Speech2Text`, `inference()` and the command line.

Mirrors espnet2/bin/asr_inference_maskctc.py (`Speech2Text.__call__` -> [(text, token, token_int, hyp)], the options and
the `1best_recog/{token,token_int,text}` files of `inference()`) and espnet2/asr/maskctc_model.py MaskCTCInference.  The
decoding itself - greedy CTC with confidences, the threshold, the K mask-predict passes of the MLM decoder - runs on the
device for a whole utterance batch (MaskCTCModel.decode_maskctc_device); `Speech2Text.batch_decode` is this project's
batched entry, `batch_size > 1` on the command line decodes length-bucketed batches through it.

Where the reference leaves a choice open this path fixes it: among equal scores the lowest position is filled first.
"""
import logging
from pathlib import Path
from typing import Any, List, Optional, Sequence, Union

import numpy as np
import torch

from espnet_amd.asr.maskctc_model import MaskCTCModel
from espnet_amd.bin.asr_inference import (_str2bool, _str2triple_str, _str_or_none, pack_modules, resolve_dtype)
from espnet_amd.lib import TooShortUttError
from espnet_amd.nets.beam_search import Hypothesis
from espnet_amd.tasks.asr import ASRTask
from espnet_amd.text.token_id_converter import TokenIDConverter, build_tokenizer

logger = logging.getLogger(__name__)


def _hypotheses(mask_token: int, y: torch.Tensor, ylens: torch.Tensor) -> List[Hypothesis]:
    """Host y (B, Lp), ylens (B,) -> one Hypothesis per utterance, yseq = [<mask>] + tokens + [<mask>] (maskctc_model.py)."""
    B, Lp = y.shape
    seq = torch.full((B, Lp + 2), mask_token, dtype=torch.int64)
    seq[:, 1 : Lp + 1] = y
    out = []
    for b, n in enumerate(ylens.tolist()):
        seq[b, n + 1] = mask_token
        out.append(Hypothesis(yseq=seq[b, : n + 2]))
    return out


class MaskCTCInference(torch.nn.Module):
    """Mask-CTC decoding of ONE encoded utterance (maskctc_model.py MaskCTCInference)."""

    def __init__(self, asr_model: MaskCTCModel, n_iterations: int, threshold_probability: float):
        super().__init__()
        if not isinstance(asr_model, MaskCTCModel):
            raise ValueError(f"MaskCTCInference needs a MaskCTCModel (model: maskctc), got {type(asr_model).__name__}")
        if int(n_iterations) < 1:
            raise NotImplementedError(f"maskctc_n_iterations={n_iterations}: the reference then fills one token per pass "
                                      "without a bound; the device chain has a fixed length (>= 1)")
        object.__setattr__(self, "asr_model", asr_model)  # (not a submodule: the model owns its parameters)
        self.mask_token = asr_model.mask_token
        self.n_iterations = int(n_iterations)
        self.threshold_probability = float(threshold_probability)
        self.converter = TokenIDConverter(token_list=asr_model.token_list)

    def ids2text(self, ids: List[int]) -> str:
        return "".join(self.converter.ids2tokens(ids)).replace("<mask>", "_").replace("<space>", " ")

    @torch.no_grad()
    def forward(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, d) on the GPU -> [Hypothesis]."""
        enc_out = enc_out.unsqueeze(0).to(torch.float32).contiguous()
        olens = torch.full((1,), enc_out.size(1), dtype=torch.int32, device=enc_out.device)
        y, ylens, _, _ = self.asr_model._decode_maskctc(enc_out, olens, self.n_iterations, self.threshold_probability)
        return _hypotheses(self.mask_token, y.cpu(), ylens.cpu())


class Speech2Text:
    def __init__(self, asr_train_config: Union[Path, str, None] = None, asr_model_file: Union[Path, str, None] = None,
                 token_type: Optional[str] = None, bpemodel: Optional[str] = None, device: str = "cuda",
                 batch_size: int = 1, dtype: str = "float32", maskctc_n_iterations: int = 10,
                 maskctc_threshold_probability: float = 0.99):
        if not str(device).startswith("cuda"):
            raise RuntimeError("espnet_amd.Speech2Text runs on an MI355X only (device='cuda'); no CPU fallback")
        if int(maskctc_n_iterations) < 1:  # (before anything is loaded)
            raise NotImplementedError(f"maskctc_n_iterations={maskctc_n_iterations}: the reference then fills one token "
                                      "per pass without a bound; the device chain has a fixed length (>= 1)")
        dtype = resolve_dtype(dtype)
        asr_model, asr_train_args = ASRTask.build_model_from_file(asr_train_config, asr_model_file, device,
                                                                  compute_dtype=dtype)
        if not isinstance(asr_model, MaskCTCModel):
            raise ValueError(f"asr_inference_maskctc needs a MaskCTCModel (model: maskctc), got {type(asr_model).__name__}")
        self.asr_model, self.asr_train_args = asr_model, asr_train_args
        self.device, self.dtype = device, dtype
        self.s2t = MaskCTCInference(asr_model, maskctc_n_iterations, maskctc_threshold_probability)
        if token_type is None:
            token_type = getattr(asr_train_args, "token_type", None)
        if bpemodel is None:
            bpemodel = getattr(asr_train_args, "bpemodel", None)
        if token_type is None or (token_type == "bpe" and bpemodel is None):
            self.tokenizer = None
        else:
            self.tokenizer = build_tokenizer(token_type=token_type, bpemodel=bpemodel)
        self.converter = self.s2t.converter
        pack_modules(device, [asr_model.frontend, asr_model.encoder, asr_model.ctc, asr_model.decoder])

    @torch.no_grad()
    def __call__(self, speech: Union[torch.Tensor, np.ndarray]):
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        speech = speech.unsqueeze(0).to(torch.float32)
        logger.info("speech length: " + str(speech.size(1)))
        return self.batch_decode(speech, [speech.size(1)])[0]

    @torch.no_grad()
    def batch_decode(self, speech: torch.Tensor, speech_lengths: Sequence[int]):
        """speech (B, N) zero padded (host or device), lengths host ints -> one [(text, token, token_int, hyp)] per
        utterance; row b is what `__call__` returns for utterance b alone (isolated-utterance encoding)."""
        speech = speech.to(self.device, torch.float32, non_blocking=True)
        st = self.asr_model.encode_device(speech, [int(n) for n in speech_lengths], isolate=True)
        y, ylens, _, _ = self.asr_model.decode_maskctc_device(st, self.s2t.n_iterations, self.s2t.threshold_probability)
        return [self._format(h) for h in _hypotheses(self.asr_model.mask_token, y.cpu(), ylens.cpu())]

    def _format(self, hyp: Hypothesis):
        """asr_inference_maskctc.py: strip the two ends, drop id 0, ids -> tokens -> text; a surviving <mask> is kept."""
        token_int = [x for x in hyp.yseq[1:-1].tolist() if x != 0]
        token = self.converter.ids2tokens(token_int)
        text = self.tokenizer.tokens2text(token) if self.tokenizer is not None else None
        return [(text, token, token_int, hyp)]

    @staticmethod
    def from_pretrained(model_tag: Optional[str] = None, **kwargs: Optional[Any]):
        if model_tag is not None:
            raise NotImplementedError("model zoo download needs network access (espnet_model_zoo)")
        return Speech2Text(**kwargs)


def inference(output_dir: str, batch_size: int = 1, dtype: str = "float32", ngpu: int = 1, seed: int = 0,
              num_workers: int = 1, log_level: Union[int, str] = "INFO", data_path_and_name_and_type=None,
              key_file: Optional[str] = None, asr_train_config: Optional[str] = None,
              asr_model_file: Optional[str] = None, model_tag: Optional[str] = None, token_type: Optional[str] = None,
              bpemodel: Optional[str] = None, allow_variable_data_keys: bool = False, maskctc_n_iterations: int = 10,
              maskctc_threshold_probability: float = 0.99):
    """espnet2/bin/asr_inference_maskctc.py `inference()`: the same keywords, `output_dir/1best_recog/{token,token_int,text}`
    in the key order of the input, the per-utterance TooShortUttError fallback; `batch_size > 1` decodes length-bucketed
    utterance batches (`Speech2Text.batch_decode`)."""
    from espnet_amd.fileio.datadir_writer import DatadirWriter

    if ngpu > 1:
        raise NotImplementedError("only single GPU decoding is supported")
    if ngpu < 1:
        raise RuntimeError("espnet_amd decodes on an MI355X only: pass --ngpu 1 (no CPU fallback)")
    logging.basicConfig(level=log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    torch.manual_seed(seed)
    np.random.seed(seed)
    speech2text = Speech2Text.from_pretrained(
        model_tag=model_tag, asr_train_config=asr_train_config, asr_model_file=asr_model_file, token_type=token_type,
        bpemodel=bpemodel, device="cuda", batch_size=batch_size, dtype=dtype, maskctc_n_iterations=maskctc_n_iterations,
        maskctc_threshold_probability=maskctc_threshold_probability)
    loader = ASRTask.build_streaming_iterator(
        data_path_and_name_and_type, dtype="float32", batch_size=batch_size, key_file=key_file, num_workers=num_workers,
        preprocess_fn=ASRTask.build_preprocess_fn(speech2text.asr_train_args, False),
        collate_fn=ASRTask.build_collate_fn(speech2text.asr_train_args, False),
        allow_variable_data_keys=allow_variable_data_keys, inference=True, ngpu=ngpu)

    def too_short():  # asr_inference_maskctc.py: the placeholder row of an utterance the subsampling cannot take
        return [(" ", ["<space>"], [2], Hypothesis(score=0.0, scores={}, states={}, yseq=[]))]

    def decode(keys, batch):
        speech, lens = batch["speech"], [int(n) for n in batch["speech_lengths"]]
        try:
            return speech2text.batch_decode(speech, lens)
        except TooShortUttError as e:
            bad = set(e.indices if e.indices is not None else range(len(keys)))
            for i in sorted(bad):
                logger.warning(f"Utterance {[keys[i]]} {e if len(bad) == 1 else 'is too short for subsampling'}")
            good = [i for i in range(len(keys)) if i not in bad]
            out = [too_short() for _ in keys]
            if good:
                sub = speech2text.batch_decode(speech[good, : max(lens[i] for i in good)], [lens[i] for i in good])
                for i, r in zip(good, sub):
                    out[i] = r
            return out

    pending, written = {}, 0
    with DatadirWriter(output_dir) as writer:
        for keys, batch in loader:
            assert len(keys) == batch["speech"].size(0)
            for k, res in zip(keys, decode(keys, batch)):
                pending[k] = res
            order = loader.key_order
            while written < len(order) and order[written] in pending:  # emit in input order
                key = order[written]
                text, token, token_int, _ = pending.pop(key)[0]
                w = writer["1best_recog"]
                w["token"][key] = " ".join(token)
                w["token_int"][key] = " ".join(map(str, token_int))
                if text is not None:
                    w["text"][key] = text
                written += 1
        assert not pending, sorted(pending)
    return dict(utterances=written)


def get_parser():
    """Option names, types and defaults of espnet2/bin/asr_inference_maskctc.py; `--config` yaml files work like
    config_argparse."""
    import argparse

    p = argparse.ArgumentParser(description="ASR Decoding with Mask-CTC (MI355X)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--config", type=str, default=None, help="yaml file with option defaults")
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO",
                   choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--ngpu", type=int, default=1, help="1 = decode on one MI355X; anything else is rejected")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64", "bfloat16"],
                   help="float32 = exact-f32 MFMA (the parity mode); bfloat16 = bf16 MFMA with f32 accumulation")
    p.add_argument("--num_workers", type=int, default=1, help="audio reader threads")
    g = p.add_argument_group("Input data related")
    g.add_argument("--data_path_and_name_and_type", type=_str2triple_str, required=True, action="append")
    g.add_argument("--key_file", type=_str_or_none)
    g.add_argument("--allow_variable_data_keys", type=_str2bool, default=False)
    g = p.add_argument_group("The model configuration related")
    for name in ("asr_train_config", "asr_model_file", "model_tag"):
        g.add_argument(f"--{name}", type=str)
    g = p.add_argument_group("Decoding related")
    g.add_argument("--batch_size", type=int, default=1, help="utterances per device batch")
    g.add_argument("--maskctc_n_iterations", type=int, default=10)
    g.add_argument("--maskctc_threshold_probability", type=float, default=0.99)
    g = p.add_argument_group("Text converter related")
    g.add_argument("--token_type", type=_str_or_none, default=None, choices=["char", "bpe", None])
    g.add_argument("--bpemodel", type=_str_or_none, default=None)
    return p


def main(cmd=None):
    import sys

    import yaml

    print(" ".join(sys.argv), file=sys.stderr)
    parser = get_parser()
    pre, _ = parser.parse_known_args(cmd)
    if pre.config is not None:  # config_argparse: yaml values become defaults, flags still win
        with open(pre.config, encoding="utf-8") as f:
            parser.set_defaults(**(yaml.safe_load(f) or {}))
    kwargs = vars(parser.parse_args(cmd))
    kwargs.pop("config", None)
    return inference(**kwargs)


if __name__ == "__main__":
    main()
