"""Perplexity of a text corpus under a trained language model: the "calc perplexity" stage of `asr.sh`
(espnet2/bin/lm_calc_perplexity.py:24-203) on the MI355X path.

    python -m espnet_amd.bin.lm_calc_perplexity --output_dir exp/lm/perplexity --batch_size 64 --dtype bfloat16 \
        --data_path_and_name_and_type dump/test/text,text,text --train_config exp/lm/config.yaml \
        --model_file exp/lm/valid.loss.ave.pth

Same keywords as the reference's `calc_perplexity`, same files: `<output_dir>/utt2ppl` and `utt2ntokens` (one
`key value` line per sentence, ntokens = the sentence's tokens + <eos>) and `ppl` (the corpus figure from the summed
nll and token counts).  The sentences of a batch are scored in one device enqueue (ESPnetLanguageModel.nll ->
TransformerLM.sequence_nll, csrc/lm_seq.hip).  Data entries are `path,text,text_int` (token ids per line) or
`path,text,text` (plain text, tokenised with the train config's token_type / bpemodel / token_list)."""
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from espnet_amd.bin.asr_inference import _str2bool, _str2triple_str, _str_or_none, resolve_dtype
from espnet_amd.fileio.datadir_writer import DatadirWriter
from espnet_amd.fileio.read_text import read_2columns_text
from espnet_amd.text.token_id_converter import TokenIDConverter, build_tokenizer

logger = logging.getLogger(__name__)


def read_text_entries(data_path_and_name_and_type: Sequence[Tuple[str, str, str]], train_args=None) -> Dict[str, np.ndarray]:
    """{key: token ids (int64)} of the one `text` entry the LM task takes (espnet2/tasks/lm.py required_data_names)."""
    entries = [(p, n, t) for p, n, t in data_path_and_name_and_type if n == "text"]
    if len(entries) != 1 or len(entries) != len(data_path_and_name_and_type):
        raise RuntimeError('lm_calc_perplexity takes exactly one data entry, named "text": '
                           f"{list(data_path_and_name_and_type)}")
    path, _, kind = entries[0]
    table = read_2columns_text(path)
    if kind == "text_int":
        return {k: np.array(v.split(), dtype=np.int64) for k, v in table.items()}
    if kind != "text":
        raise NotImplementedError(f'data type {kind!r} is outside this path ("text_int" | "text")')
    token_type = getattr(train_args, "token_type", None)
    if token_type is None:
        raise RuntimeError("a plain-text entry needs token_type in the train config")
    tokenizer = build_tokenizer(token_type, bpemodel=getattr(train_args, "bpemodel", None))
    conv = TokenIDConverter(train_args.token_list)
    return {k: np.array(conv.tokens2ids(tokenizer.text2tokens(v)), dtype=np.int64) for k, v in table.items()}


def perplexity(nll_sum: float, ntokens: int, log_base: Optional[float]) -> float:
    """lm_calc_perplexity.py:116-119: exp(nll / n), or log_base ** (nll / n / ln(log_base))."""
    if log_base is None:
        return np.exp(nll_sum / ntokens)
    return log_base ** (nll_sum / ntokens / np.log(log_base))


def write_perplexity(model, data: Dict[str, np.ndarray], keys: List[str], output_dir: Union[Path, str], batch_size: int,
                     log_base: Optional[float], device) -> float:
    """The scoring loop of the reference (:98-128): batches of `batch_size` sentences in key order through
    `model.nll(text, text_lengths)`; writes utt2ppl / utt2ntokens / ppl and returns the corpus perplexity."""
    total_nll, total_ntokens = 0.0, 0
    with DatadirWriter(output_dir) as writer:
        for s in range(0, len(keys), batch_size):
            ks = keys[s:s + batch_size]
            lens = torch.tensor([len(data[k]) for k in ks], dtype=torch.long)
            text = torch.zeros(len(ks), max(int(lens.max()), 1), dtype=torch.long)
            for i, k in enumerate(ks):
                text[i, : lens[i]] = torch.from_numpy(data[k])
            nll, lengths = model.nll(text.to(device), lens.to(device))
            nll = nll.detach().cpu().numpy().sum(1)
            lengths = lengths.detach().cpu().numpy()
            total_nll += nll.sum()
            total_ntokens += lengths.sum()
            for key, _nll, ntoken in zip(ks, nll, lengths):
                writer["utt2ppl"][key] = str(perplexity(_nll, ntoken, log_base))
                writer["utt2ntokens"][key] = str(ntoken)
    ppl = perplexity(total_nll, total_ntokens, log_base)
    with (Path(output_dir) / "ppl").open("w", encoding="utf-8") as f:
        f.write(f"{ppl}\n")
    return float(ppl)


def calc_perplexity(output_dir: str, batch_size: int, dtype: str, ngpu: int, seed: int, num_workers: int,
                    log_level: Union[int, str], data_path_and_name_and_type: Sequence[Tuple[str, str, str]],
                    key_file: Optional[str], train_config: Optional[str], model_file: Optional[str],
                    log_base: Optional[float], allow_variable_data_keys: bool):
    """espnet2/bin/lm_calc_perplexity.py:24-128."""
    from espnet_amd.tasks.lm import LMTask

    if batch_size < 1:
        raise ValueError(f"batch_size must be positive: {batch_size}")
    if ngpu > 1:
        raise NotImplementedError("only single GPU decoding is supported")
    if ngpu < 1:
        raise RuntimeError("espnet_amd scores on an MI355X only: pass --ngpu 1 (no CPU fallback)")
    logging.basicConfig(level=log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    torch.manual_seed(seed)
    np.random.seed(seed)
    model, train_args = LMTask.build_model_from_file(train_config, model_file, "cuda", compute_dtype=resolve_dtype(dtype))
    data = read_text_entries(data_path_and_name_and_type, train_args)
    keys = list(read_2columns_text(key_file)) if key_file is not None else list(data)
    missing = [k for k in keys if k not in data]
    if missing:
        raise RuntimeError(f"{len(missing)} keys of {key_file} are not in the text entry, e.g. {missing[0]}")
    ppl = write_perplexity(model, data, keys, output_dir, batch_size, log_base, torch.device("cuda"))
    logger.info(f"perplexity {ppl} over {len(keys)} sentences")
    return ppl


def _float_or_none(v: str):
    return None if v.strip().lower() in ("none", "null", "nil", "") else float(v)


def get_parser():
    """Option names, types and defaults of espnet2/bin/lm_calc_perplexity.py:131-193 (`--ngpu` defaults to 1 here: there
    is no CPU path)."""
    import argparse

    p = argparse.ArgumentParser(description="Calc perplexity (MI355X)", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--config", type=str, default=None, help="yaml file with option defaults")
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO",
                   choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--ngpu", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64", "bfloat16"])
    p.add_argument("--num_workers", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--log_base", type=_float_or_none, default=None,
                   help="The base of logarithm for Perplexity. If None, napier's constant is used.")
    g = p.add_argument_group("Input data related")
    g.add_argument("--data_path_and_name_and_type", type=_str2triple_str, required=True, action="append")
    g.add_argument("--key_file", type=_str_or_none)
    g.add_argument("--allow_variable_data_keys", type=_str2bool, default=False)
    g = p.add_argument_group("The model configuration related")
    g.add_argument("--train_config", type=str)
    g.add_argument("--model_file", type=str)
    return p


def main(cmd=None):
    import sys

    import yaml

    print(" ".join(sys.argv), file=sys.stderr)
    parser = get_parser()
    pre, _ = parser.parse_known_args(cmd)
    if pre.config is not None:
        with open(pre.config, encoding="utf-8") as f:
            parser.set_defaults(**(yaml.safe_load(f) or {}))
    kwargs = vars(parser.parse_args(cmd))
    kwargs.pop("config", None)
    return calc_perplexity(**kwargs)


if __name__ == "__main__":
    main()
