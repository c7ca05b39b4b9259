"""RLE pattern text (the format of Golly and LifeWiki) <-> 0/1 cell arrays: thin wrappers over the native
reader and writer (csrc/src/io/rle.cpp)."""
from __future__ import annotations

import numpy as np

from .._native import _gol
from .bitpack import pack_cells, unpack_words


def pattern_from_cells(cells, rule: str = "", topology: str = "", bound_cols: int = 0, bound_rows: int = 0):
    """A 2-D 0/1 array -> native ``RlePattern`` (``rule``: any form the engine's rule parser takes, or "";
    ``topology``: "" or the header suffix's "T" / "P" with the board it names)."""
    cells = np.asarray(cells)
    if cells.ndim != 2 or cells.shape[0] < 1 or cells.shape[1] < 1:
        raise ValueError(f"a pattern is a 2-D array with at least one cell, got shape {cells.shape}")
    if rule:
        from .oracle import is_ltl_rule, ltl_rule_string, rule_string

        rule = ltl_rule_string(rule) if is_ltl_rule(rule) else rule_string(rule)
    return _gol.RlePattern(pack_cells(cells != 0), int(cells.shape[1]), rule, topology, int(bound_cols), int(bound_rows))


def pattern_cells(pattern) -> np.ndarray:
    """Native ``RlePattern`` -> (rows, cols) uint8 cells."""
    return unpack_words(pattern.words, pattern.cols)


def parse_rle(text: str):
    """RLE text -> ``(cells, rule)``: a (y, x) uint8 array and the header's rule in canonical form ("" when
    the header has none).  ValueError, naming the offending character or offset, on malformed text."""
    p = _gol.parse_rle(text)
    return pattern_cells(p), p.rule


def write_rle(cells, rule: str = "") -> str:
    """0/1 cells -> RLE text: canonical header, run-length coded rows without trailing dead cells, lines of at
    most 70 characters, a final ``!``."""
    return _gol.write_rle(pattern_from_cells(cells, rule))
