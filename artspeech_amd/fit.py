"""Fit to time: spans of tokens spoken in an exact number of frames (as_plan_set_fit; the rule: csrc/duration_fit.h).

    Fit.whole(2.4)                                   the utterance (every utterance of a batch) in 2.40 s
    Fit.whole([2.4, None, 1.0])                      per utterance; None: as predicted
    Fit([(0, 3, 9, 0.8), (0, 10, 12, 0.25)])         tokens 3..9 of utterance 0 in 0.8 s, tokens 10..12 in 0.25 s (indices inclusive)
    Fit.whole(2.4, hold=Fit.hold_pauses)             the pauses keep their predicted lengths, the speech absorbs the difference

A target is in seconds (one half-rate frame is 25 ms: rint(seconds * 40) frames) or, ``frames=True``, in half-rate frames.  ``hold``: a
predicate on a token id, or one mask per utterance, for the tokens that keep their own rounded durations.  Host logic only: `build` makes
the arrays of an ``as_fit`` for one batch, and says what every utterance's frame count will be when the spans cover it end to end -- the
call then needs no read-back."""
import numpy as np

from . import text

FRAMES_PER_SECOND = 40
MAX_SPANS, MAX_COUNT, D_MAX = 4096, 4096, 16384
PAUSE_IDS = frozenset(text.word_index_dictionary[c] for c in text._punctuation)      # space and punctuation


def seconds_to_frames(seconds):
    """rint(seconds * 40): half-rate frames of 25 ms, ties to even"""
    return int(np.rint(float(seconds) * FRAMES_PER_SECOND))


class Built:
    """the arrays of an as_fit for one batch (host, int32) and what the host knows of the result"""

    def __init__(self, span_tok, span_frames, lock, max_count, frames_hint):
        self.span_tok, self.span_frames, self.lock, self.max_count, self.frames_hint = span_tok, span_frames, lock, max_count, frames_hint

    @property
    def n_spans(self):
        return int(self.span_tok.shape[0])


class Fit:
    def __init__(self, spans, hold=None, frames=False):
        """spans: (utterance, first token, last token, target) with inclusive token indices into the utterance's cleaned tokens; last None:
        the utterance's last token.  frames: the targets are half-rate frames, not seconds."""
        self.spans = [(int(b), int(first), None if last is None else int(last), target) for b, first, last, target in spans]
        self.hold, self.in_frames, self._whole = hold, bool(frames), None

    @classmethod
    def whole(cls, targets, hold=None, frames=False):
        """every utterance end to end: one target for all of them, or a list with one per utterance (None: that utterance is not fitted)"""
        f = cls([], hold=hold, frames=frames)
        f._whole = list(targets) if isinstance(targets, (list, tuple, np.ndarray)) else float(targets)
        return f

    @staticmethod
    def hold_pauses(token):
        """hold=: a space or a punctuation mark (text.py's ids) keeps its own duration"""
        return int(token) in PAUSE_IDS

    def _target(self, t):
        t = int(t) if self.in_frames else seconds_to_frames(t)
        if t < 1:
            raise ValueError(f"fit: a target of {t} frames")
        return t

    def _spans_of(self, tok_lens):
        if self._whole is None:
            return self.spans
        per = self._whole if isinstance(self._whole, list) else [self._whole] * len(tok_lens)
        if len(per) != len(tok_lens):
            raise ValueError(f"fit: {len(per)} targets for {len(tok_lens)} utterances")
        return [(b, 0, None, t) for b, t in enumerate(per) if t is not None and tok_lens[b] > 0]

    def _lock(self, tok_lens, tokens):
        if self.hold is None:
            return None
        if callable(self.hold):
            if tokens is None:
                raise ValueError("fit: hold= as a predicate needs the token ids")
            flat = np.concatenate([np.asarray(t).reshape(-1)[:n] for t, n in zip(tokens, tok_lens)]) if tok_lens else np.zeros(0)
            return np.array([1 if self.hold(int(t)) else 0 for t in flat], np.int32)
        masks = list(self.hold)
        if len(masks) != len(tok_lens) or any(m is not None and len(m) != n for m, n in zip(masks, tok_lens)):
            raise ValueError("fit: hold= as masks takes one mask (or None) per utterance, one entry per token")
        return np.concatenate([np.zeros(n, np.int32) if m is None else (np.asarray(m) != 0).astype(np.int32)
                               for m, n in zip(masks, tok_lens)]) if tok_lens else np.zeros(0, np.int32)

    def build(self, tok_lens, tokens=None):
        """tok_lens: the batch's token counts; tokens: per utterance its token ids (for a hold= predicate) -> Built.  Spans are sorted by
        packed position; overlapping ones, or ones outside their utterance, raise ValueError."""
        tok_lens = [int(n) for n in tok_lens]
        off = np.concatenate([[0], np.cumsum(tok_lens)]).astype(np.int64)
        rows = []
        for b, first, last, target in self._spans_of(tok_lens):
            if not 0 <= b < len(tok_lens):
                raise ValueError(f"fit: span for utterance {b}: there are {len(tok_lens)}")
            last = tok_lens[b] - 1 if last is None else last
            if not 0 <= first <= last < tok_lens[b]:
                raise ValueError(f"fit: span {first}..{last} does not lie inside utterance {b}'s {tok_lens[b]} tokens")
            if last - first + 1 > MAX_COUNT:
                raise ValueError(f"fit: a span of {last - first + 1} tokens (at most {MAX_COUNT})")
            rows.append((int(off[b]) + first, last - first + 1, self._target(target), b))
        if not 1 <= len(rows) <= MAX_SPANS:
            raise ValueError(f"fit: {len(rows)} spans (1 .. {MAX_SPANS})")
        rows.sort()
        for (f0, c0, _, _), (f1, _, _, _) in zip(rows, rows[1:]):
            if f1 < f0 + c0:
                raise ValueError("fit: spans overlap")
        covered = [0] * len(tok_lens)
        total = [0] * len(tok_lens)
        for _, c, t, b in rows:
            if t < c:
                raise ValueError(f"fit: {t} frames for {c} tokens (a token has at least one frame)")
            covered[b] += c
            total[b] += t
        # the host knows the frame counts only where no span can turn out void on the device: every token in a span, nothing held (what
        # the held tokens leave the others depends on the predictor) and no target above one token's limit
        sure = self.hold is None and all(t <= D_MAX for _, _, t, _ in rows)
        hint = total if sure and all(covered[b] == tok_lens[b] for b in range(len(tok_lens))) else None
        return Built(np.array([[r[0], r[1]] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32), self._lock(tok_lens, tokens),
                     max(r[1] for r in rows), hint)
