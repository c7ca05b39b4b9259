"""Connected components of a board: the result type, the orientation-free object hash and the numpy oracle.

**Neighbourhoods**: ``"von_neumann"`` (``|dr| + |dc| = 1``), ``"moore"`` (Chebyshev distance 1, the default) and ``"moore2"``
(Chebyshev distance <= 2: two live cells this close share a neighbour, so under Life they interact -- the pseudo-object
notion).  Two live cells are joined when one lies in the other's neighbourhood, and a **component** is a class of the
transitive closure; coordinates wrap on the torus (each soup of a batch is its own torus), nothing lies outside a bounded
board.

Per component: the **anchor** is its first cell in row-major order, its **label** ``1 + row * W + col`` of the anchor (a dead
cell has label 0), the **population** its number of cells.  The **bounding box** ``(r0, c0, rows, cols)`` is, on a bounded
board, the plain extents; on the torus, per axis of length ``L``, the extents of the coordinate ``x`` and of
``(x + L // 2) % L`` are taken, the frame with the smaller extent is kept (the plain one on a tie) and ``r0`` / ``c0`` is
reported in board coordinates, so ``r0 + rows`` may exceed ``H`` -- ``window(*bbox)`` wraps and returns the object.  A
component whose cyclic extent along an axis is at most ``L / 2`` gets its true box.  The **hash**: with ``A`` the component's
cells inside its box and ``A_k`` its orientation ``k`` (ids 0..3 clockwise quarter turns, 4..7 the same turns of the
left-right mirror image), ``h_k`` is the sum over the live ``(i, j)`` of ``A_k`` of ``sig_rho(i) * sig_gam(j)`` mod 2^64 (the two
32-bit mixes of the board signature, the product taken in 64 bits), and the hash is ``min_k h_k``: the same for all eight
orientations and wherever the object lies.  Objects are sorted by anchor (with a batch by soup, then anchor).

The labelling itself is native (``csrc/src/core/components.cpp`` on the CPU, the kernels of ``components_kernel.hip`` on the
HIP backend); :func:`numpy_components` is the independent oracle: vectorised hooking and pointer jumping over edge lists,
and a hash computed per cell from the formula above, with :func:`object_hash` (arrays turned with ``np.rot90``) beside it.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

NEIGHBOURHOODS = ("von_neumann", "moore", "moore2")


class Components(NamedTuple):
    """What :meth:`Simulation.components` returns (``SoupBatch.components``: :class:`SoupComponents`)."""

    count: int               # objects on the board; always exact
    anchor: np.ndarray       # (k, 2) int64 (row, col), sorted row-major; k = min(count, max_objects)
    population: np.ndarray   # (k,) uint32
    bbox: np.ndarray         # (k, 4) int64 (r0, c0, rows, cols); window(*bbox) is the object
    hash: np.ndarray         # (k,) uint64; empty with hashes=False
    truncated: bool          # count > max_objects: the arrays hold some max_objects of the objects


class SoupComponents(NamedTuple):
    """What :meth:`SoupBatch.components` returns: :class:`Components` plus the soup of every object."""

    count: int
    soup: np.ndarray         # (k,) int64; the objects are sorted by (soup, row, col)
    anchor: np.ndarray       # in the soup's own coordinates, as the boxes are
    population: np.ndarray
    bbox: np.ndarray
    hash: np.ndarray
    truncated: bool


def check_neighbourhood(neighbourhood, what: str = "components") -> str:
    if neighbourhood not in NEIGHBOURHOODS:
        raise ValueError(f"{what}: neighbourhood {neighbourhood!r} is not one of von_neumann, moore, moore2")
    return neighbourhood


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _rho(i) -> np.ndarray:
    """The row key of ``gol/signature.hpp`` as uint64."""
    with np.errstate(over="ignore"):
        return (_mix32(np.asarray(i).astype(np.uint32) ^ np.uint32(0x9E3779B9)) | np.uint32(1)).astype(np.uint64)


def _gam(j) -> np.ndarray:
    """The column key of ``gol/signature.hpp`` as uint64."""
    with np.errstate(over="ignore"):
        return (_mix32(np.asarray(j).astype(np.uint32) + np.uint32(0x7F4A7C15)) | np.uint32(1)).astype(np.uint64)


def _binary(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"components: {what} is a 2-D array with at least one cell, got shape {a.shape}")
    bad = (a != 0) & (a != 1)
    if bad.any():
        raise ValueError(f"components: a cell of {what} is {a[bad].flat[0].item()!r}, not 0 or 1")
    return a.astype(np.uint8)


def object_hash(cells) -> int:
    """The hash of a 0/1 array holding one object (empty rows and columns around it are cut off first): each of the eight
    orientations is built with ``np.fliplr`` / ``np.rot90``, keyed and summed; the minimum is the hash."""
    a = _binary(cells, "the object")
    rows, cols = np.nonzero(a.any(axis=1))[0], np.nonzero(a.any(axis=0))[0]
    if len(rows) == 0:
        raise ValueError("components: object_hash of an array without a live cell")
    a = a[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    best = None
    for k in range(8):
        t = np.rot90(np.fliplr(a) if k >= 4 else a, -(k & 3))
        i, j = np.nonzero(t)
        with np.errstate(over="ignore"):
            h = int((_rho(i) * _gam(j)).sum(dtype=np.uint64))
        best = h if best is None else min(best, h)
    return best


def _offsets(neighbourhood: str):
    """The half of the neighbourhood that comes later in row-major order (the relation is symmetric)."""
    if neighbourhood == "von_neumann":
        return [(0, 1), (1, 0)]
    reach = 1 if neighbourhood == "moore" else 2
    return [(dr, dc) for dr in range(0, reach + 1) for dc in range(-reach, reach + 1) if dr > 0 or dc > 0]


def _labels(board: np.ndarray, neighbourhood: str, torus: bool) -> np.ndarray:
    """For every cell the flat index of its component's first cell (dead cells: -1)."""
    H, W = board.shape
    live = board.astype(bool)
    flat = np.flatnonzero(live)
    node = np.full(H * W, -1, dtype=np.int64)
    node[flat] = np.arange(len(flat))
    node = node.reshape(H, W)
    src, dst = [], []
    for dr, dc in _offsets(neighbourhood):
        if torus:
            other = np.roll(node, (-dr, -dc), axis=(0, 1))  # other[r, c] = node[r + dr, c + dc]
            both = (node >= 0) & (other >= 0)
            src.append(node[both])
            dst.append(other[both])
        else:
            r0, r1 = max(0, -dr), min(H, H - dr)
            c0, c1 = max(0, -dc), min(W, W - dc)
            if r0 >= r1 or c0 >= c1:
                continue
            a = node[r0:r1, c0:c1]
            b = node[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
            both = (a >= 0) & (b >= 0)
            src.append(a[both])
            dst.append(b[both])
    a = np.concatenate(src) if src else np.zeros(0, np.int64)
    b = np.concatenate(dst) if dst else np.zeros(0, np.int64)
    # lab[x] <= x: a forest whose roots are the lowest nodes seen so far.  It starts from the rows' runs of live cells
    # (a node whose left neighbour in the row is live belongs to that neighbour's run), which every neighbourhood joins.
    starts = np.ones(len(flat), dtype=bool)
    starts[1:] = (np.diff(flat) != 1) | (flat[1:] % W == 0)
    lab = np.maximum.accumulate(np.where(starts, np.arange(len(flat), dtype=np.int64), 0))
    while True:
        la, lb = lab[a], lab[b]
        differ = la != lb
        if not differ.any():
            break
        a, b, la, lb = a[differ], b[differ], la[differ], lb[differ]
        lo, hi = np.minimum(la, lb), np.maximum(la, lb)
        np.minimum.at(lab, hi, lo)  # hook the higher root under the lower one
        while True:                 # compress: every node points at its root
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    out = np.full(H * W, -1, dtype=np.int64)
    out[flat] = flat[lab]
    return out.reshape(H, W)


def _axis_box(x: np.ndarray, obj: np.ndarray, k: int, L: int, torus: bool):
    """Per object the first coordinate and the extent along one axis, by the box rule."""
    def extent(v):
        mn = np.full(k, L, dtype=np.int64)
        mx = np.full(k, -1, dtype=np.int64)
        np.minimum.at(mn, obj, v)
        np.maximum.at(mx, obj, v)
        return mn, mx

    mn, mx = extent(x)
    if not torus:
        return mn, mx - mn + 1
    mn2, mx2 = extent((x + L // 2) % L)
    plain = (mx - mn) <= (mx2 - mn2)
    return np.where(plain, mn, (mn2 - L // 2) % L), np.where(plain, mx - mn, mx2 - mn2) + 1


def numpy_components(board, neighbourhood: str = "moore", boundary: str = "torus"):
    """The oracle: ``(labels, components)`` of the 0/1 array ``board`` under ``boundary`` (``"torus"`` or ``"dead"``):
    ``labels`` is an ``(H, W)`` int64 array (``1 + row * W + col`` of the anchor, 0 for a dead cell), ``components`` a
    :class:`Components` with every object."""
    board = _binary(board, "the board")
    check_neighbourhood(neighbourhood, "numpy_components")
    if boundary not in ("torus", "dead"):
        raise ValueError(f"components: boundary must be torus or dead, got {boundary!r}")
    torus = boundary == "torus"
    H, W = board.shape
    root = _labels(board, neighbourhood, torus)
    labels = root + 1
    r, c = np.nonzero(board)
    anchors, obj = np.unique(root[r, c], return_inverse=True)  # (sorted: the objects in anchor order)
    k = len(anchors)
    pop = np.bincount(obj, minlength=k).astype(np.uint32)
    r0, rows = _axis_box(r, obj, k, H, torus)
    c0, cols = _axis_box(c, obj, k, W, torus)
    i, j = (r - r0[obj]) % H, (c - c0[obj]) % W
    i2, j2 = rows[obj] - 1 - i, cols[obj] - 1 - j
    # orientation k maps box cell (i, j) to (row, col): the identity, three quarter turns, then the same of the mirror image
    turned = [(i, j), (j, i2), (i2, j2), (j2, i), (i, j2), (j2, i2), (i2, j), (j, i)]
    sums = np.zeros((8, k), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for t, (row, col) in enumerate(turned):
            np.add.at(sums[t], obj, _rho(row) * _gam(col))
    hashes = sums.min(axis=0) if k else np.zeros(0, np.uint64)
    anchor = np.stack([anchors // W, anchors % W], axis=1).astype(np.int64).reshape(k, 2)
    bbox = np.stack([r0, c0, rows, cols], axis=1).astype(np.int64).reshape(k, 4)
    return labels, Components(k, anchor, pop, bbox, hashes.astype(np.uint64), False)
