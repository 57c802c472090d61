"""The candidate transcripts of a batch of utterances as `Speech2Text.batch_nll / batch_transducer_nll / batch_rescore`
take them: flattened and checked once on the host, handed out in slices, regrouped per utterance.  Host data only."""
from typing import Callable, Iterator, List, NamedTuple, Optional, Sequence

import numpy as np
import torch


def is_one_transcript(t) -> bool:
    """A string, a tensor / array or a flat sequence of ints (an empty one too) is ONE transcript, not a list of them."""
    if isinstance(t, str) or hasattr(t, "tolist"):
        return True
    return len(t) == 0 or all(isinstance(v, (int, np.integer)) for v in t)


class CandidateSlice(NamedTuple):
    u0: int               # the slice's utterances are u0 .. u1 - 1
    u1: int
    ids: List[List[int]]  # per candidate
    ylens: List[int]
    mem_of: List[int]     # utterance of each candidate, absolute ...
    mem_rel: List[int]    # ... and relative to u0
    ys: torch.Tensor      # (len(ids), width) int64, zero padded to the slice's own longest transcript


class CandidateBatch:
    """texts[b] is one transcript or a list of candidate transcripts of utterance b.  `to_ids` turns a transcript (a
    string or ids) into a list of ints and raises ValueError for what it cannot take; with `vocab_size` every id must
    lie in [0, vocab_size), and no id of `forbidden` ({id: name}) may occur.  Everything is checked here, on the host."""

    def __init__(self, texts: Sequence, n_utts: int, to_ids: Callable, vocab_size: Optional[int] = None,
                 forbidden: Optional[dict] = None):
        if len(texts) != n_utts:
            raise ValueError(f"{len(texts)} transcript entries for {n_utts} utterances")
        self.ids, self.mem_of, self.counts = [], [], []  # per candidate, per candidate (non-decreasing), per utterance
        for b, entry in enumerate(texts):
            group = [entry] if is_one_transcript(entry) else list(entry)
            self.counts.append(len(group))
            for y in map(to_ids, group):
                for v in y:
                    if forbidden and v in forbidden:
                        raise ValueError(f"token id {v} ({forbidden[v]}) cannot be aligned")
                    if vocab_size is not None and not 0 <= v < vocab_size:
                        raise ValueError(f"token ids must lie in [0, {vocab_size})")
                self.ids.append(y)
                self.mem_of.append(b)
        self.ylens = [len(y) for y in self.ids]

    def __len__(self) -> int:
        return len(self.ids)

    def slices(self, rows_per_call: int, min_width: int = 1) -> Iterator[CandidateSlice]:
        """The candidates in consecutive slices of up to `rows_per_call`; `ys` is at least `min_width` columns wide."""
        for s in range(0, len(self.ids), rows_per_call):
            ids, mo, ylens = (v[s : s + rows_per_call] for v in (self.ids, self.mem_of, self.ylens))
            ys = torch.zeros(len(ids), max(max(ylens), min_width), dtype=torch.long)
            for i, y in enumerate(ids):
                ys[i, : len(y)] = torch.tensor(y, dtype=torch.long)
            yield CandidateSlice(mo[0], mo[-1] + 1, ids, ylens, mo, [u - mo[0] for u in mo], ys)

    def regroup(self, values: Sequence) -> List[list]:
        """One value per candidate, in candidate order -> one list per utterance."""
        ends = np.cumsum(self.counts).tolist()
        return [list(values[e - n : e]) for n, e in zip(self.counts, ends)]
