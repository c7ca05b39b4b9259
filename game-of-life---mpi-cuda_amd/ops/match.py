"""Pattern matching: templates, their orientations and the numpy oracle.

A template is two equal-shape 0/1 arrays ``value`` and ``care`` of at most 32 x 32 cells and a ring width ``ring >= 0`` with
``2 * ring < min(shape)``; ``value <= care`` and some ``care`` cell is set.  It **matches at board cell (r, c)** when, for
every template cell ``(i, j)`` with ``care[i, j] = 1``, board cell ``(r - ring + i, c - ring + j)`` equals ``value[i, j]``;
coordinates wrap on the torus, cells outside a bounded board are dead, and only board cells are candidate positions.

A template built from a pattern with ``margin = m`` is the pattern padded by ``m`` dead cells on every side with ``care`` all
ones and ``ring = m``: a match means the pattern sits there, isolated by ``m`` cells, and the reported position is the board
cell under the pattern's top-left cell.

Orientation ids 0..3 are the template turned clockwise by 0, 90, 180 and 270 degrees, 4..7 the same turns of its left-right
mirror image (``value`` and ``care`` turn together, ``ring`` stays); a turned template equal to one of a lower id is dropped.

The matching itself is native (``csrc/src/core/match.cpp`` on the CPU, the ``k_match`` kernel on the HIP backend);
:func:`numpy_match` is the independent oracle, written with ``np.roll`` and zero padding.
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import numpy as np

from .._native import _gol

MAX_SIDE = 32


class MatchResult(NamedTuple):
    """What :meth:`Simulation.match` returns."""

    count: int               # matches over the requested orientations; always exact
    positions: np.ndarray    # (k, 2) int64 (row, col), sorted by (row, col, orientation); k = min(count, max_hits)
    orientation: np.ndarray  # (k,) uint8: the orientation id of each position
    truncated: bool          # count > max_hits: the positions are some max_hits of the matches


class Template:
    """An immutable match template: ``value`` and ``care`` (read-only uint8 arrays of one shape) and ``ring``.  Build one
    with :func:`match_template`."""

    __slots__ = ("value", "care", "ring", "native")

    def __init__(self, value, care, ring: int):
        value = np.array(value, dtype=np.uint8)
        care = np.array(care, dtype=np.uint8)
        native = _gol.MatchTemplate(value, care, int(ring))  # (ValueError on anything a template may not be)
        value.setflags(write=False)
        care.setflags(write=False)
        for k, v in (("value", value), ("care", care), ("ring", int(ring)), ("native", native)):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Template is immutable")

    @property
    def shape(self) -> Tuple[int, int]:
        return self.value.shape

    def __eq__(self, other):
        return (isinstance(other, Template) and self.ring == other.ring and self.shape == other.shape
                and bool((self.value == other.value).all()) and bool((self.care == other.care).all()))

    def __hash__(self):
        return hash((self.ring, self.shape, self.value.tobytes(), self.care.tobytes()))

    def __repr__(self):
        return f"Template({self.shape[0]} x {self.shape[1]}, ring={self.ring}, care={int(self.care.sum())} cells)"


def _binary(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"match: {what} is a 2-D array with at least one cell, got shape {a.shape}")
    bad = (a != 0) & (a != 1)
    if bad.any():
        raise ValueError(f"match: a cell of {what} is {a[bad].flat[0].item()!r}, not 0 or 1")
    return a.astype(np.uint8)


def match_template(pattern=None, margin: int = 1, *, value=None, care=None, ring: int = 0) -> Template:
    """``match_template(pattern, margin=1)``: the pattern (an RLE path, RLE text or a 0/1 array, what ``stamp()`` accepts)
    as given, padded by ``margin`` dead cells on every side, ``care`` all ones, ``ring = margin``.
    ``match_template(value=..., care=..., ring=0)``: the arrays as they are (``care`` defaults to all ones).
    ValueError on a cell that is not 0 or 1, a negative margin, a shape over 32 x 32, no care cell, a value outside care
    and ``2 * ring >= min(shape)``."""
    if value is not None or care is not None:
        if pattern is not None:
            raise ValueError("match_template: give a pattern or value/care, not both")
        if value is None:
            raise ValueError("match_template: care without value")
        value = _binary(value, "value")
        care = np.ones_like(value) if care is None else _binary(care, "care")
        if care.shape != value.shape:
            raise ValueError(f"match_template: value has shape {value.shape}, care {care.shape}")
        return Template(value, care, int(ring))
    if pattern is None:
        raise ValueError("match_template: no pattern")
    margin = int(margin)
    if margin < 0:
        raise ValueError(f"match: margin = {margin} is negative")
    if isinstance(pattern, (str, bytes)) or hasattr(pattern, "__fspath__") or isinstance(pattern, _gol.RlePattern):
        from ..models.life import Simulation
        from .rle import pattern_cells

        cells = pattern_cells(Simulation._pattern(pattern))
    else:
        cells = _binary(pattern, "the pattern")
    if max(cells.shape) + 2 * margin > MAX_SIDE:
        raise ValueError(
            f"match: a {cells.shape[0]} x {cells.shape[1]} pattern with margin {margin} makes a "
            f"{cells.shape[0] + 2 * margin} x {cells.shape[1] + 2 * margin} template, over {MAX_SIDE} x {MAX_SIDE}"
        )
    padded = np.pad(cells.astype(np.uint8), margin)
    return Template(padded, np.ones_like(padded), margin)


def as_template(pattern_or_template, margin: int = 1) -> Template:
    """A :class:`Template` as it is (``margin`` is not used), anything else through :func:`match_template`."""
    if isinstance(pattern_or_template, Template):
        return pattern_or_template
    return match_template(pattern_or_template, margin)


def want_all(orientations) -> bool:
    """``orientations=False`` (id 0 only) or ``"all"`` (every distinct one; ``True`` means the same)."""
    if orientations is False or orientations is None:
        return False
    if orientations is True or orientations == "all":
        return True
    raise ValueError(f"match: orientations must be False or 'all', got {orientations!r}")


def _turn(a: np.ndarray, k: int) -> np.ndarray:
    if k >= 4:
        a = np.fliplr(a)
    return np.ascontiguousarray(np.rot90(a, -(k & 3)))  # (clockwise)


def template_orientations(t: Template, orientations="all") -> List[Tuple[int, Template]]:
    """``[(id, template)]``: the distinct orientations of ``t`` in id order (``orientations=False``: id 0 alone).  Written
    in numpy, independently of the native ``MatchTemplate.orientations``."""
    out: List[Tuple[int, Template]] = []
    for k in range(8 if want_all(orientations) else 1):
        o = Template(_turn(t.value, k), _turn(t.care, k), t.ring)
        if not any(o == seen for _, seen in out):
            out.append((k, o))
    return out


def _bitmap(board: np.ndarray, t: Template, torus: bool) -> np.ndarray:
    H, W = board.shape
    th, tw = t.shape
    acc = np.ones((H, W), dtype=bool)
    if not torus:
        padded = np.zeros((H + th, W + tw), dtype=board.dtype)
        padded[t.ring:t.ring + H, t.ring:t.ring + W] = board
    for i, j in zip(*np.nonzero(t.care)):
        if torus:  # shifted[r, c] = board[r - ring + i, c - ring + j]
            shifted = np.roll(board, (t.ring - int(i), t.ring - int(j)), axis=(0, 1))
        else:
            shifted = padded[i:i + H, j:j + W]
        acc &= shifted == t.value[i, j]
    return acc


def numpy_match(board, template, boundary: str = "torus", orientations=False):
    """The oracle: ``(positions, orientation)``, a ``(k, 2)`` int64 array of (row, col) sorted by (row, col, orientation)
    and the ``(k,)`` uint8 orientation ids, of every match of ``template`` (a :class:`Template`) on the 0/1 array
    ``board`` under ``boundary`` (``"torus"`` or ``"dead"``)."""
    board = _binary(board, "the board")
    if boundary not in ("torus", "dead"):
        raise ValueError(f"match: boundary must be torus or dead, got {boundary!r}")
    if not isinstance(template, Template):
        raise ValueError(f"numpy_match: expected a Template (ops.match_template), got {type(template).__name__}")
    H, W = board.shape
    rows, cols, ids = [], [], []
    for k, t in template_orientations(template, orientations):
        if t.shape[0] > H or t.shape[1] > W:
            raise ValueError(f"match: the template is {t.shape[0]} x {t.shape[1]}, the board {H} x {W}")
        r, c = np.nonzero(_bitmap(board, t, boundary == "torus"))
        rows.append(r)
        cols.append(c)
        ids.append(np.full(r.shape, k, dtype=np.uint8))
    r, c, o = np.concatenate(rows), np.concatenate(cols), np.concatenate(ids)
    order = np.lexsort((o, c, r))
    return np.stack([r[order], c[order]], axis=1).astype(np.int64), o[order]
