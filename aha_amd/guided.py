"""Guided decoding on the caller's side of aha_hip_generate_batch_masked / aha_hip_engine_set_mask: packed allowed-token masks, the
constraint protocol and one real constraint.

A token mask is ceil(V / 32) uint32 words; id i is allowed iff bit i & 31 of word i >> 5 is set (include/aha_hip.h states the definition).
A constraint is a callable (seq, generated) -> packed words, or None for an unmasked step: seq is the prompt's index in the batch,
generated its tokens so far (empty for the first token).  HipInferenceModel.generate_batch_masked asks it once per live prompt per step;
with a HipEngine the caller asks it between steps and hands the words to HipEngine.set_mask.  Grammars, regular expressions and JSON
schemas are compiled by the caller into such a callable; this module only ships guided choice.
"""
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

Constraint = Callable[[int, Sequence[int]], Optional[np.ndarray]]


def mask_words(vocab_size: int) -> int:
    return (int(vocab_size) + 31) // 32


def pack_mask(allowed_ids: Iterable[int], vocab_size: int) -> np.ndarray:
    """The packed words that allow exactly allowed_ids (each 0 <= id < vocab_size; duplicates are fine)."""
    V = int(vocab_size)
    ids = np.unique(np.asarray(list(allowed_ids), dtype=np.int64).reshape(-1))
    if ids.size and (ids[0] < 0 or ids[-1] >= V):
        raise ValueError(f"allowed ids must lie in 0 .. {V - 1}")
    words = np.zeros(mask_words(V), dtype=np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return words


def unpack_mask(words: np.ndarray, vocab_size: int) -> np.ndarray:
    """The sorted ids < vocab_size that the packed words allow (bits at positions >= vocab_size are ignored)."""
    V = int(vocab_size)
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    if w.size != mask_words(V):
        raise ValueError(f"the mask has {w.size} words, a vocabulary of {V} needs {mask_words(V)}")
    ids = np.arange(V)
    return ids[((w[ids >> 5] >> (ids & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)]


class ChoiceConstraint:
    """guided_choice: every prompt's output is exactly one of `choices` (token-id sequences) followed by one of stop_ids.

    A trie over the choices: the allowed set is the children of the node the generated tokens lead to, plus the stop ids where a choice
    ends there (one choice may be a prefix of another: both continuing and stopping are then allowed).  Generation ends on the stop
    id, so nothing is asked after it.  A prefix that left the trie raises ValueError.  The object keeps no per-prompt state: it
    walks the trie from the root each call, so one instance serves every prompt of a batch and every request of an engine."""

    def __init__(self, choices: Sequence[Sequence[int]], stop_ids: Sequence[int], vocab_size: int):
        self.vocab_size = int(vocab_size)
        self.stop_ids = sorted({int(t) for t in stop_ids})
        if not choices or any(len(c) == 0 for c in choices):
            raise ValueError("choices must be non-empty token sequences")
        if not self.stop_ids:
            raise ValueError("a choice needs at least one stop id to end on")
        self.root: Dict = {}
        for c in choices:
            node = self.root
            for t in c:
                if not 0 <= int(t) < self.vocab_size:
                    raise ValueError(f"choice token {t} outside the vocabulary")
                node = node.setdefault(int(t), {})
            node[None] = True   # a choice ends here
        self._masks: Dict[int, np.ndarray] = {}   # id(node) -> packed words (the trie is immutable after construction)

    def _node(self, generated: Sequence[int]) -> Dict:
        node = self.root
        for n, t in enumerate(generated):
            if int(t) not in node:
                raise ValueError(f"generated prefix {[int(g) for g in generated[:n + 1]]} is not a prefix of any choice")
            node = node[int(t)]
        return node

    def allowed(self, generated: Sequence[int]) -> List[int]:
        """The sorted ids allowed after `generated`."""
        node = self._node(generated)
        ids = [t for t in node if t is not None]
        return sorted(set(ids + self.stop_ids)) if None in node else sorted(ids)

    def __call__(self, seq: int, generated: Sequence[int]) -> np.ndarray:
        node = self._node(generated)
        m = self._masks.get(id(node))
        if m is None:
            m = self._masks[id(node)] = pack_mask(self.allowed(generated), self.vocab_size)
        return m
