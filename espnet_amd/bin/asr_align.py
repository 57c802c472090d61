"""CTC segmentation: start time, end time and a confidence for each utterance of a text inside a long recording, the
tool of espnet2/bin/asr_align.py (class CTCSegmentation, built on the `ctc_segmentation` package) on the MI355X path.

    python -m espnet_amd.bin.asr_align --asr_train_config exp/asr/config.yaml --asr_model_file exp/asr/valid.acc.ave.pth \
        --audio lecture.wav --text utterances.txt --output segments.txt

The log-posteriors never leave the device: encoder -> `em_ctc_log_probs_t` -> `em_ctc_segment` (csrc/ctc_segment.hip;
include/espnet_amd.h states the trellis), and one D2H copy of first_frame / frame_lp / t_end / total / status per trellis
run; segments and confidences are float64 arithmetic on the host.  The reference package was not at hand when this was
written: the contract is this project's restatement (DESIGN.md 4s lists the known deviations: the band's shape, the tie
rule, the inclusive last window of the confidence).  `text_converter="classic"`, `gratis_blank` and
`replace_spaces_with_blanks` are not implemented."""
import logging
import math
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from espnet_amd.bin.asr_inference import _str2bool, _str_or_none, pack_modules, resolve_dtype
from espnet_amd.nets_utils import SUBSAMPLING_CONVS
from espnet_amd.tasks.asr import ASRTask
from espnet_amd.text.token_id_converter import TokenIDConverter, build_tokenizer

logger = logging.getLogger(__name__)


def build_ground_truth(utt_ids: Sequence[Sequence[int]], blank: int, names: Optional[Sequence[str]] = None):
    """[start] + sum_k([blank] + tokens_k) + [blank] -> (gt, utt_begin): utt_begin[k] is the separator column in front
    of utterance k, utt_begin[K] = C - 1.  The start symbol's value is never read (the blank id stands there).  An
    utterance with no tokens, or with a token equal to the blank id, raises ValueError naming it."""
    gt, begin = [int(blank)], []
    for k, toks in enumerate(utt_ids):
        who = names[k] if names is not None else f"utterance {k}"
        toks = [int(v) for v in toks]
        if not toks:
            raise ValueError(f"{who}: no tokens to align")
        if any(v == blank for v in toks):
            raise ValueError(f"{who}: the blank id {blank} cannot stand inside a text")
        begin.append(len(gt))
        gt += [int(blank)] + toks
    if not begin:
        raise ValueError("no utterances to align")
    begin.append(len(gt))
    return gt + [int(blank)], begin


def determine_segments(first_frame, frame_lp, t_end: int, utt_begin: Sequence[int], dur: float, n: int = 30):
    """[(start_s, end_s, confidence)] per utterance from one recording's trellis outputs, float64.  tm[c] =
    first_frame[c] * dur; between the separators p and q: start = max(tm[p+1] - 0.5, (tm[p] + tm[p-1]) / 2), end =
    min(tm[q-1] + 0.5, (tm[q] + tm[q-1]) / 2).  Confidence: over the frames [floor(start / dur), ceil(end / dur)), both
    clipped to [0, t_end], the minimum over every window of n frames (the last one included) of the mean frame_lp; the
    plain mean when there are at most n frames; -1e10 when there are none."""
    tm = np.asarray(first_frame, dtype=np.float64) * float(dur)
    flp = np.asarray(frame_lp, dtype=np.float64)
    csum = np.concatenate([[0.0], np.cumsum(flp)])
    out = []
    for k in range(len(utt_begin) - 1):
        p, q = int(utt_begin[k]), int(utt_begin[k + 1])
        start = max(tm[p + 1] - 0.5, (tm[p] + tm[p - 1]) / 2)
        end = min(tm[q - 1] + 0.5, (tm[q] + tm[q - 1]) / 2)
        s = min(max(int(math.floor(start / dur)), 0), int(t_end))
        e = min(max(int(math.ceil(end / dur)), 0), int(t_end))
        if e <= s:
            conf = -1e10
        elif e - s <= n:
            conf = float(flp[s:e].mean())
        else:
            t = np.arange(s, e - n + 1)
            conf = float(((csum[t + n] - csum[t]) / n).min())
        out.append((float(start), float(end), conf))
    return out


def get_partitions(n_samples: int, samples_per_frame: int, body_frames: int, overlap_frames: int):
    """Cut a recording of n_samples into partitions the encoder can take: [(sample_start, sample_end, drop_head,
    drop_tail)].  Partition p carries the body frames [p F, (p + 1) F) and `overlap_frames` more on each inner side,
    which are dropped from its encoder output; the last partition takes the remainder (a remainder shorter than the
    overlap, or than 16 frames, goes to the partition in front of it).  In nominal frames (samples // samples_per_frame)
    the kept frames sum to the whole; a recording of at most F frames is one partition, nothing dropped."""
    sps, F, ov = int(samples_per_frame), int(body_frames), int(overlap_frames)
    if sps < 1 or F < 1 or ov < 0:
        raise ValueError("samples_per_frame and body_frames must be positive, overlap_frames not negative")
    n_frames = int(n_samples) // sps
    if n_frames <= F:
        return [(0, int(n_samples), 0, 0)]
    P = -(-n_frames // F)
    if n_frames - (P - 1) * F < max(ov, 16):
        P -= 1
    parts = []
    for p in range(P):
        head, tail = (ov if p > 0 else 0), (ov if p < P - 1 else 0)
        s1 = int(n_samples) if p == P - 1 else ((p + 1) * F + tail) * sps
        parts.append(((p * F - head) * sps, s1, head, tail))
    return parts


class CTCSegmentationTask:
    """One recording's result (the reference's class of this name): `segments` = [(start_s, end_s, confidence)] per
    utterance, `str(task)` the segments file."""

    def __init__(self, name="audio", utt_ids=(), text=(), gt=(), utt_begin=(), print_utt_text=True, print_utt_score=True):
        self.name, self.utt_ids, self.text = name, list(utt_ids), list(text)
        self.ground_truth_mat, self.utt_begin_indices = list(gt), list(utt_begin)
        self.print_utt_text, self.print_utt_score = print_utt_text, print_utt_score
        self.segments = []
        self.first_frame = self.frame_lp = None
        self.t_end, self.total, self.status = 0, float("-inf"), 0
        self.window, self.clipped, self.index_duration, self.lpz_frames = 0, False, 0.0, 0

    def __str__(self):
        lines = []
        for utt_id, text, (start, end, score) in zip(self.utt_ids, self.text, self.segments):
            line = f"{utt_id} {self.name} {start:.2f} {end:.2f}"
            if self.print_utt_score:
                line += f" {score:.4f}"
            if self.print_utt_text:
                line += f" {text}"
            lines.append(line + "\n")
        return "".join(lines)


class CTCSegmentation:
    def __init__(self, asr_train_config: Union[Path, str, None] = None, asr_model_file: Union[Path, str, None] = None,
                 fs: int = 16000, ngpu: int = 1, batch_size: int = 1, dtype: str = "float32", device: str = "cuda",
                 kaldi_style_text: bool = True, text_converter: str = "tokenize", time_stamps: str = "auto",
                 token_type: Optional[str] = None, bpemodel: Optional[str] = None,
                 longest_audio_segments: float = 320.0, partitions_overlap_frames: int = 30,
                 partition_batch_size: int = 8, **ctc_segmentation_args):
        if text_converter == "classic":
            raise NotImplementedError('text_converter="classic" (character matching with multi-character tokens) is not '
                                      'implemented on the MI355X path; use text_converter="tokenize"')
        if text_converter != "tokenize":
            raise ValueError(f'text_converter must be "tokenize", not {text_converter!r}')
        if time_stamps not in ("auto", "fixed"):
            raise ValueError(f'time_stamps must be "auto" or "fixed", not {time_stamps!r}')
        if not str(device).startswith("cuda"):
            raise RuntimeError("espnet_amd.CTCSegmentation runs on an MI355X only (device='cuda'); no CPU fallback")
        asr_model, asr_train_args = ASRTask.build_model_from_file(asr_train_config, asr_model_file, device,
                                                                  compute_dtype=resolve_dtype(dtype))
        if getattr(asr_model, "ctc", None) is None:
            raise ValueError("CTC segmentation needs a CTC head (the model has ctc_weight == 0)")
        self.asr_model, self.asr_train_args = asr_model, asr_train_args
        self.device, self.fs = device, int(fs)
        self.kaldi_style_text, self.text_converter, self.time_stamps = kaldi_style_text, text_converter, time_stamps
        token_type = token_type if token_type is not None else getattr(asr_train_args, "token_type", None)
        bpemodel = bpemodel if bpemodel is not None else getattr(asr_train_args, "bpemodel", None)
        if token_type is None or (token_type == "bpe" and bpemodel is None):
            self.tokenizer = None
        else:
            self.tokenizer = build_tokenizer(token_type=token_type, bpemodel=bpemodel)
        self.converter = TokenIDConverter(token_list=asr_model.token_list)
        self.longest_audio_segments = float(longest_audio_segments)
        self.partitions_overlap_frames = int(partitions_overlap_frames)
        self.partition_batch_size = int(partition_batch_size)
        self.min_window_size, self.max_window_size = 8000, None
        self.score_min_mean_over_L = 30
        self.preamble_transition_cost_zero, self.backtrack_from_max_t = True, False
        self.print_utt_text = self.print_utt_score = True
        self.set_config(**ctc_segmentation_args)
        pack_modules(device, [asr_model.frontend, asr_model.encoder, asr_model.ctc])

    _SETTABLE = ("min_window_size", "max_window_size", "score_min_mean_over_L", "preamble_transition_cost_zero",
                 "backtrack_from_max_t", "print_utt_text", "print_utt_score", "time_stamps", "kaldi_style_text")

    def set_config(self, **kw):
        """The segmentation keywords of the reference; `gratis_blank` / `replace_spaces_with_blanks` must stay off."""
        for k, v in kw.items():
            if k in ("gratis_blank", "replace_spaces_with_blanks"):
                if v:
                    raise NotImplementedError(f"CTCSegmentation({k}={v!r}) is not implemented on the MI355X path")
            elif k in self._SETTABLE:
                if v is not None or k == "max_window_size":
                    setattr(self, k, v)
            else:
                raise TypeError(f"CTCSegmentation: unknown keyword {k!r}")

    # ------------------------------------------------------------------ timing
    @property
    def samples_per_frame(self) -> int:
        """Frontend hop x encoder subsampling (4, 6 or 8 from the encoder's `input_layer`)."""
        enc, fe = self.asr_model.encoder, self.asr_model.frontend
        layer = getattr(enc, "input_layer", "conv2d")
        if layer not in SUBSAMPLING_CONVS:
            raise ValueError(f"input_layer={layer!r}: no subsampling factor known for it")
        sub = 1
        for _, stride in SUBSAMPLING_CONVS[layer]:
            sub *= stride
        return sub * int(fe.hop_length)

    def index_duration(self, n_samples: int, n_frames: int) -> float:
        if self.time_stamps == "fixed":
            return self.samples_per_frame / float(self.fs)
        return n_samples / float(self.fs) / n_frames

    # ------------------------------------------------------------------ text
    def prepare_ground_truth(self, text, name="audio") -> CTCSegmentationTask:
        """text: one string of lines or a list of lines, `utt_id words ...` under kaldi_style_text, else plain
        utterances (ids `{name}_{index:04d}`) -> a task with the ground-truth columns and utt_begin, nothing run."""
        lines = text.splitlines() if isinstance(text, str) else list(text)
        lines = [ln.strip() for ln in lines if ln.strip()]
        if self.kaldi_style_text:
            pairs = [ln.split(maxsplit=1) for ln in lines]
            utt_ids, utts = [p[0] for p in pairs], [p[1] if len(p) > 1 else "" for p in pairs]
        else:
            utt_ids, utts = [f"{name}_{i:04d}" for i in range(len(lines))], lines
        if self.tokenizer is None:
            raise ValueError("CTC segmentation of text needs a tokenizer (token_type / bpemodel)")
        ids = [self.converter.tokens2ids(self.tokenizer.text2tokens(u)) for u in utts]
        gt, begin = build_ground_truth(ids, self.asr_model.blank_id, utt_ids)
        return CTCSegmentationTask(name, utt_ids, utts, gt, begin, self.print_utt_text, self.print_utt_score)

    # ------------------------------------------------------------------ log-posteriors
    def _partitions(self, n_samples: int):
        F = int(self.longest_audio_segments * self.fs) // self.samples_per_frame
        if n_samples <= self.longest_audio_segments * self.fs:
            return [(0, int(n_samples), 0, 0)]
        return get_partitions(n_samples, self.samples_per_frame, max(F, 1), self.partitions_overlap_frames)

    def log_probs_t(self, speech: torch.Tensor) -> torch.Tensor:
        """speech (N,) on the device -> lpT (V, T) f32 on the device.  A recording of one partition is encoded as it is;
        a longer one in batches of partitions (`encode_device(..., isolate=True)`), whose overlap frames are dropped and
        whose kept columns are concatenated on the device."""
        m = self.asr_model
        parts = self._partitions(int(speech.numel()))
        if len(parts) == 1:
            st = m.encode_device(speech[None], [int(speech.numel())], isolate=True)
            return m.ctc.log_probs_t_device(st.enc_act)
        kept = []
        for i in range(0, len(parts), self.partition_batch_size):
            chunk = parts[i:i + self.partition_batch_size]
            lens = [s1 - s0 for s0, s1, _, _ in chunk]
            batch = torch.zeros(len(chunk), max(lens), dtype=torch.float32, device=speech.device)
            for r, (s0, s1, _, _) in enumerate(chunk):
                batch[r, : s1 - s0] = speech[s0:s1]
            st = m.encode_device(batch, lens, isolate=True)
            Tm = int(st.enc_act.shape[1])
            lpT = m.ctc.log_probs_t_device(st.enc_act)
            for r, (_, _, head, tail) in enumerate(chunk):
                kept.append(lpT[:, r * Tm + head : r * Tm + int(st.olens[r]) - tail])
        return torch.cat(kept, dim=1)

    # ------------------------------------------------------------------ run
    @torch.no_grad()
    def __call__(self, speech: Union[torch.Tensor, np.ndarray], text, name: Optional[str] = None) -> CTCSegmentationTask:
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        return self.batch_call([speech], None, [text], [name] if name is not None else None)[0]

    @torch.no_grad()
    def batch_call(self, speeches, lengths=None, texts=(), names=None) -> List[CTCSegmentationTask]:
        """Several recordings through ONE trellis launch per window size.  speeches: a list of 1-D arrays / tensors, or a
        zero-padded (B, N) tensor with `lengths`.  Every recording is encoded on its own (so row b equals the single
        call bit for bit); the log-posteriors stay on the device while the window doubles."""
        from espnet_amd import lib as L

        B = len(speeches)
        if len(texts) != B:
            raise ValueError(f"{len(texts)} texts for {B} recordings")
        names = list(names) if names is not None else (["audio"] if B == 1 else [f"audio{b}" for b in range(B)])
        tasks = [self.prepare_ground_truth(t, n) for t, n in zip(texts, names)]  # the texts' refusals come first
        m = self.asr_model
        lpTs, n_samples = [], []
        for b in range(B):
            x = speeches[b]
            x = torch.as_tensor(x)[: int(lengths[b])] if lengths is not None else torch.as_tensor(x)
            n_samples.append(int(x.numel()))
            lpTs.append(self.log_probs_t(x.to(self.device, torch.float32, non_blocking=True).reshape(-1)))
        Ts = [int(t.shape[1]) for t in lpTs]
        T, V = max(Ts), m.ctc.odim
        if B == 1:
            lpT = lpTs[0].contiguous()
        else:
            lpT = torch.zeros(V, B * T, dtype=torch.float32, device=lpTs[0].device)
            for b, t in enumerate(lpTs):
                lpT[:, b * T : b * T + Ts[b]] = t
        del lpTs
        gts, clens = [t.ground_truth_mat for t in tasks], [len(t.ground_truth_mat) for t in tasks]
        for b in range(B):
            if clens[b] - 1 > Ts[b]:
                raise ValueError(f"{names[b]}: {Ts[b]} encoder frames cannot carry a text of {clens[b] - 1} columns")
        olens_d, gt_d, clens_d, Cmax = m.ctc._segment_inputs(Ts, gts, clens, V, T, lpT.device)
        cap = int(L.load().em_ctc_segment_max_window())
        w_max = min(int(self.max_window_size), cap) if self.max_window_size else cap
        W = max(1, min(int(self.min_window_size), w_max))
        while True:
            outs = m.ctc.segment_log_probs_t(lpT, int(lpT.shape[1]), olens_d, gt_d, Cmax, clens_d, B, T, m.blank_id, W,
                                             preamble_free=bool(self.preamble_transition_cost_zero),
                                             from_last_frame=bool(self.backtrack_from_max_t))
            first_frame, _, frame_lp, t_end, total, status = outs
            # the one D2H copy: int32 words travel as the bits of f32 columns of one matrix
            host = torch.cat([first_frame.view(torch.float32), frame_lp, t_end[:, None].view(torch.float32), total[:, None],
                              status[:, None].view(torch.float32)], dim=1).cpu().numpy()
            st = host[:, Cmax + T + 2].view(np.int32)
            # (a band narrower than the table that leaves no route at all is widened like one that clips the path)
            if not (st & (L.EM_SEG_CLIPPED | L.EM_SEG_NO_ROUTE)).any() or W >= w_max or W >= Cmax:
                break
            W = min(2 * W, w_max)
        for b, task in enumerate(tasks):
            row = host[b]
            task.status, task.window = int(st[b]), W
            task.first_frame = row[: clens[b]].view(np.int32).copy()
            task.frame_lp = row[Cmax : Cmax + Ts[b]].copy()
            task.t_end, task.total = int(row[Cmax + T : Cmax + T + 1].view(np.int32)[0]), float(row[Cmax + T + 1])
            task.lpz_frames = Ts[b]
            if task.status & L.EM_SEG_NO_ROUTE:
                raise RuntimeError(f"{names[b]}: no route through the trellis ({Ts[b]} frames, {clens[b]} columns, window {W})")
            task.clipped = bool(task.status & L.EM_SEG_CLIPPED)
            if task.clipped:
                logger.warning(f"{names[b]}: the path still touches the band's edge at window {W}; the segments may not be optimal")
            task.index_duration = self.index_duration(n_samples[b], Ts[b])
            task.segments = determine_segments(task.first_frame, task.frame_lp, task.t_end, task.utt_begin_indices,
                                               task.index_duration, int(self.score_min_mean_over_L))
        return tasks


def read_audio(path: Union[Path, str]):
    """(samples float32, rate) of a wav or flac file through the package's readers."""
    from espnet_amd.fileio.sound_scp import read_flac, read_wav

    x, rate = (read_flac if str(path).lower().endswith(".flac") else read_wav)(path, dtype="float32")
    return (x.mean(axis=1) if x.ndim == 2 else x).astype(np.float32, copy=False), int(rate)


def ctc_align(log_level: Union[int, str], asr_train_config: str, asr_model_file: str, audio: str, text: str,
              output: Optional[str] = None, print_utt_text: bool = True, print_utt_score: bool = True, **kwargs):
    """espnet2/bin/asr_align.py `ctc_align`: the segments file to `output` or stdout."""
    import sys

    logging.basicConfig(level=log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    aligner = CTCSegmentation(asr_train_config=asr_train_config, asr_model_file=asr_model_file,
                              print_utt_text=print_utt_text, print_utt_score=print_utt_score, **kwargs)
    speech, rate = read_audio(audio)
    if rate != aligner.fs:
        raise ValueError(f"{audio}: sampling rate {rate}, the aligner was built for fs={aligner.fs}")
    task = aligner(speech, Path(text).read_text(encoding="utf-8"), name=Path(audio).stem)
    if output is None:
        sys.stdout.write(str(task))
    else:
        Path(output).write_text(str(task), encoding="utf-8")
    return task


def _int_or_none(v: str):
    return None if v.strip().lower() in ("none", "null", "nil", "") else int(v)


def get_parser():
    """Option names of espnet2/bin/asr_align.py (`--ngpu` defaults to 1 here: there is no CPU path)."""
    import argparse

    p = argparse.ArgumentParser(description="ASR alignment: CTC segmentation (MI355X)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO",
                   choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--ngpu", type=int, default=1)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64", "bfloat16"])
    g = p.add_argument_group("Model configuration related")
    g.add_argument("--asr_train_config", type=str, required=True)
    g.add_argument("--asr_model_file", type=str, required=True)
    g.add_argument("--token_type", type=_str_or_none, default=None)
    g.add_argument("--bpemodel", type=_str_or_none, default=None)
    g = p.add_argument_group("Text converter related")
    g.add_argument("--kaldi_style_text", type=_str2bool, default=True)
    g.add_argument("--text_converter", type=str, default="tokenize", choices=["tokenize", "classic"])
    g = p.add_argument_group("CTC segmentation related")
    g.add_argument("--fs", type=int, default=16000)
    g.add_argument("--time_stamps", type=str, default="auto", choices=["auto", "fixed"])
    g.add_argument("--min_window_size", type=int, default=8000)
    g.add_argument("--max_window_size", type=_int_or_none, default=None)
    g.add_argument("--score_min_mean_over_L", type=int, default=30)
    g.add_argument("--preamble_transition_cost_zero", type=_str2bool, default=True)
    g.add_argument("--backtrack_from_max_t", type=_str2bool, default=False)
    g.add_argument("--longest_audio_segments", type=float, default=320.0)
    g.add_argument("--partitions_overlap_frames", type=int, default=30)
    g = p.add_argument_group("Input/output arguments")
    g.add_argument("--audio", type=str, required=True, help="wav or flac file")
    g.add_argument("--text", type=str, required=True, help="utterances, one per line (`utt_id text` under kaldi_style_text)")
    g.add_argument("--output", "-o", type=_str_or_none, default=None, help="the segments file (default: stdout)")
    g.add_argument("--print_utt_text", type=_str2bool, default=True)
    g.add_argument("--print_utt_score", type=_str2bool, default=True)
    return p


def main(cmd=None):
    kwargs = vars(get_parser().parse_args(cmd))
    if kwargs["ngpu"] != 1:
        raise RuntimeError("espnet_amd aligns on one MI355X: pass --ngpu 1 (no CPU path)")
    return ctc_align(**kwargs)


if __name__ == "__main__":
    main()
