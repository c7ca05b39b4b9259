"""Cycle search over a series of board hashes: a pure function, so hash collisions can be tested without a board."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, NamedTuple, Optional, Tuple


class Cycle(NamedTuple):
    """What :meth:`Simulation.find_cycle` found: the board first enters its cycle at generation ``transient`` and
    repeats every ``period`` generations; ``generation`` is where the search stopped (the board's generation, inside
    the cycle) and ``population`` the live cells there."""

    transient: int
    period: int
    generation: int
    population: int


def find_repeat(
    series: Iterable[int],
    seen: Dict[int, int],
    start: int,
    verify: Callable[[int, int], bool],
) -> Optional[Tuple[int, int]]:
    """Look the hashes ``series[i]`` of generations ``start + i`` up in ``seen`` (hash -> first generation, which is
    updated in place) and return the first confirmed repeat ``(g_prev, g)``: the earliest ``g`` whose hash was seen at
    an earlier generation ``g_prev`` and for which ``verify(g_prev, g)`` holds.  A hit the verifier rejects is a
    collision: the pair is dropped (the earlier generation keeps the hash) and the search goes on.  ``None`` when the
    series ends first.

    The first repeat of a deterministic sequence gives its least period, ``g - g_prev``, and ``g_prev`` is the first
    generation on the cycle -- as far as the hashes tell generations apart."""
    for i, h in enumerate(series):
        g = start + i
        h = int(h)
        g_prev = seen.get(h)
        if g_prev is None:
            seen[h] = g
        elif verify(g_prev, g):
            return g_prev, g
    return None
