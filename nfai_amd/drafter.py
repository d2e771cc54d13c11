"""Draft tokens for greedy speculative decoding without a second model: prompt lookup.

Text repeats itself (quoted passages, code identifiers, lists), so the tokens that followed the last occurrence of the current
n-gram are a cheap guess at what follows it now.  Pure host code; LlamaWindow.Verify decides how many of the guesses are kept, so
a wrong guess costs time, never correctness.
"""
from __future__ import annotations


class PromptLookupDrafter:
    """The lookup is a dict per n from n-gram to the index behind its most recent occurrence, extended by the tokens the history
    gained since the last call: a call costs the new tokens plus ngram_max dict lookups, whatever the length of the conversation
    (one list comparison at C speed checks that the history only grew; any other history is indexed from scratch)."""

    def __init__(self, ngram_max: int = 3):
        if ngram_max < 1:
            raise ValueError("PromptLookupDrafter: ngram_max must be at least 1")
        self.ngram_max = int(ngram_max)
        self._h: list[int] = []                                        # the history as of the last call
        self._ends = 0                                                 # n-grams ENDING below this index are in _next
        self._next = [dict() for _ in range(self.ngram_max + 1)]       # [n]: n-gram -> index of the token behind its latest occurrence

    def Propose(self, history, k: int, stop: int | None = None) -> list[int]:
        """At most k tokens that followed the most recent EARLIER occurrence of the last n tokens of `history`, for the largest n in
        ngram_max .. 1 that occurs at all; [] when none does.  The proposal ends where the history ends, and in front of the first
        `stop` token (a loop that ends at EOS never feeds it, so it must not ride as a draft either)."""
        h = self._h
        m = len(h)
        if not isinstance(history, list):
            history = history.tolist() if hasattr(history, "tolist") else list(history)
        if len(history) < m or history[:m] != h:
            h = self._h = []
            m = self._ends = 0
            self._next = [dict() for _ in range(self.ngram_max + 1)]
        h.extend(int(t) for t in history[m:])
        L = len(h)
        if L < 2:
            return []
        # every n-gram that ends in front of the last token has something behind it; the last one wins
        for e in range(self._ends, L - 1):
            for n in range(1, min(self.ngram_max, e + 1) + 1):
                self._next[n][tuple(h[e - n + 1:e + 1])] = e + 1
        self._ends = L - 1
        if k <= 0:
            return []
        for n in range(min(self.ngram_max, L - 1), 0, -1):
            at = self._next[n].get(tuple(h[L - n:]))
            if at is not None:
                out = h[at:at + k]
                if stop is not None and stop in out:
                    out = out[:out.index(stop)]
                return out
        return []
