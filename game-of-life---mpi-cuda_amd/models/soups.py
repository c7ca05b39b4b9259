"""Soup batches: many small random tori ("soups") per launch, each run until it settles.

:class:`SoupBatch` drives a native ``_gol.SoupBatch`` (HIP: the ``step_soups`` kernel, one wave64 per soup with the board
in registers; CPU: the same per-soup program on packed words).  It is not a :class:`Simulation`: no engine, plan or
autotune, one rank, Moore rules on the torus.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from .._native import _gol

SIZES = (64, 128, 256)
MAX_SOUPS = 1 << 20


class SoupResult(NamedTuple):
    """What :meth:`SoupBatch.settle` returns, one entry per soup."""

    period: np.ndarray      # uint32; 0: not settled by ``generation``
    transient: np.ndarray   # int64; -1: not computed (no ``transient=True``, or not settled)
    generation: np.ndarray  # uint32; the generation of the hit, or ``max_gens``
    population: np.ndarray  # uint32; live cells at ``generation``


class SoupBatch:
    """``n`` independent square tori of side ``size`` (64, 128 or 256) under one Moore rule.

    Soup ``i`` starts as ``ops.random_board(size, size, (seed + i) mod 2**64)`` (pattern 5), or from a caller's array
    (:meth:`from_boards`).  :meth:`settle` runs Brent's search with exact board comparison (``ops.numpy_soup_settle`` states
    it) on every soup at once; :meth:`step` is the plain stepper.  ``V`` / ``H`` rules, ``boundary="dead"`` and
    ``compat=True`` are refused.  ``backend``: ``"hip"`` or ``"cpu"``; both give identical results.
    """

    def __init__(self, n: int, size: int = 64, rule: str = "B3/S23", backend: str = "hip", seed: int = 0, device: int = 0, *,
                 boundary: str = "torus", compat: bool = False, workgroup: int = 0, _boards=None, _tensor=None):
        n, size = int(n), int(size)
        if size not in SIZES:
            raise ValueError(f"soups: size {size} is not supported (a soup is a square torus of side 64, 128 or 256)")
        if not 1 <= n <= MAX_SOUPS:
            raise ValueError(f"soups: n = {n} is outside 1 .. 2^20")
        self._native = _gol.SoupBatch(n, size, str(rule), str(backend), int(device), str(boundary), bool(compat), int(workgroup))
        self.n, self.size, self.backend, self.device = n, size, str(backend), int(device)
        if _tensor is not None:
            self._native.init_cells(*_tensor)
        elif _boards is None:
            self._native.init_seed(int(seed) & ((1 << 64) - 1))
        else:
            self._native.init_boards(_boards)

    @classmethod
    def from_boards(cls, boards, rule: str = "B3/S23", backend: str = "hip", device: int = 0, **kw) -> "SoupBatch":
        """A batch of the ``(n, S, S)`` 0/1 array ``boards``, one soup per board."""
        b = np.asarray(boards)
        if b.ndim != 3 or b.shape[1] != b.shape[2]:
            raise ValueError(f"soups: boards of shape {b.shape} are not an (n, S, S) array")
        bad = (b != 0) & (b != 1)
        if bad.any():
            raise ValueError(f"soups: a board cell is {b[bad].flat[0].item()!r}, not 0 or 1")
        return cls(b.shape[0], b.shape[1], rule, backend, 0, device, _boards=np.ascontiguousarray(b, dtype=np.uint8), **kw)

    @classmethod
    def from_tensor(cls, boards, rule: str = "B3/S23", **kw) -> "SoupBatch":
        """A batch of the ``(n, S, S)`` torch tensor ``boards``, one soup per board, a cell alive iff its element ``!= 0``
        (dtypes and stream ordering: :mod:`gol_amd.ops.tensors`).  The backend follows the tensor: a CUDA tensor makes a
        ``hip`` batch on its device and is packed there by a kernel, a CPU tensor a ``cpu`` batch; a ``backend`` or
        ``device`` keyword that says otherwise is a ValueError."""
        from ..ops import tensors

        torch = tensors._torch()
        if not isinstance(boards, torch.Tensor):
            raise ValueError(f"soups: from_tensor expected a torch.Tensor, got {type(boards).__name__}")
        if boards.dim() != 3 or boards.shape[1] != boards.shape[2]:
            raise ValueError(f"soups: a tensor of shape {tuple(boards.shape)} is not (n, S, S)")
        if boards.device.type not in ("cuda", "cpu"):
            raise ValueError(f"soups: a tensor on {boards.device} is neither a CUDA nor a CPU tensor")
        backend = "hip" if boards.is_cuda else "cpu"
        device = boards.device.index if boards.is_cuda else 0
        if kw.get("backend", backend) != backend:
            raise ValueError(f"soups: a tensor on {boards.device} makes a {backend} batch, the call asks for backend {kw['backend']!r}")
        if boards.is_cuda and int(kw.get("device", device)) != device:
            raise ValueError(f"soups: the tensor is on {boards.device}, the call asks for device {kw['device']}")
        kw.pop("backend", None)
        kw.pop("device", None)
        tensors.dtype_code(boards.dtype, "soups: from_tensor")
        n, size = int(boards.shape[0]), int(boards.shape[1])
        if size not in SIZES:  # (before the tensor is made contiguous or anything else is touched)
            raise ValueError(f"soups: size {size} is not supported (a soup is a square torus of side 64, 128 or 256)")
        if not 1 <= n <= MAX_SOUPS:
            raise ValueError(f"soups: n = {n} is outside 1 .. 2^20")
        t = boards.contiguous()
        tensors.sync(t)
        return cls(n, size, rule, backend, 0, device, _tensor=tensors.handle(t), **kw)

    def boards_tensor(self, indices: Optional[Sequence[int]] = None, dtype=None, out=None):
        """The boards of the soups ``indices`` as a ``(k, S, S)`` tensor of 0 and 1 on the batch's side (``hip``: a CUDA
        tensor on the batch's device, unpacked there by a kernel; ``cpu``: a CPU tensor).  ``indices``: ``None`` (all) or a
        contiguous range (``range(a, b)`` or a sequence that spells one out); anything else is a ValueError, as is a
        wrong ``out`` (shape, dtype, contiguity, device).  The current torch stream is synchronised before the batch
        writes the tensor; the batch synchronises its stream before the call returns (a pending :meth:`step` included)."""
        from ..ops import tensors

        first, count = tensors.index_range(indices, self.n, "soups: boards_tensor")
        t = tensors.result((count, self.size, self.size), dtype, tensors.device_of(self.backend, self.device), out,
                           "soups: boards_tensor")
        tensors.sync(t)
        self._native.read_boards_cells(first, count, *tensors.handle(t))
        return t

    def step(self, generations: int = 1) -> "SoupBatch":
        """``generations`` steps of every soup, with no comparison.  Refused once :meth:`settle` has begun a search (the
        settled soups stand at different generations).  A search begun after stepping counts its saves from there."""
        if int(generations) < 0:
            raise ValueError(f"soups: step({generations}) is negative")
        self._native.step(int(generations))
        return self

    def settle(self, max_gens: int, transient: bool = False, chunk: int = 4096) -> SoupResult:
        """Run every soup that has not settled until it does or stands at generation ``max_gens``; ``transient`` also finds
        the exact transient of every settled soup.  One launch advances a soup by at most ``chunk`` generations; the
        result depends neither on ``chunk`` nor on how ``max_gens`` was reached over several calls."""
        self._native.settle(int(max_gens), bool(transient), int(chunk))
        return self.records()

    def synchronize(self) -> None:
        """Wait for the launches of :meth:`step` (HIP); every other call returns finished work."""
        self._native.synchronize()

    def records(self) -> SoupResult:
        return SoupResult(*self._native.records())

    def boards(self, indices: Optional[Sequence[int]] = None) -> np.ndarray:
        """The boards of the soups ``indices`` (default: all) as a ``(k, S, S)`` uint8 array; only they leave the device."""
        idx = list(range(self.n)) if indices is None else [int(i) for i in indices]
        return self._native.boards(idx)

    def match_counts(self, patterns, margin: int = 1, orientations="all") -> np.ndarray:
        """An ``(n, len(patterns))`` uint32 array: entry ``(i, t)`` is the number of matches of ``patterns[t]`` (what
        ``Simulation.match`` accepts: a pattern, isolated by ``margin`` dead cells, or an ``ops.Template``), summed over
        its requested orientations, on soup ``i``'s current board (a torus).  HIP: one ``k_match`` launch per oriented
        template over all soups; only the counts leave the device.  A pending :meth:`step` is included."""
        from ..ops.match import as_template, want_all

        all_ = want_all(orientations)
        templates = [[o for _, o in as_template(p, margin).native.orientations(all_)] for p in patterns]
        for ts in templates:
            for o in ts:
                if o.th > self.size or o.tw > self.size:
                    raise ValueError(f"soups: match_counts: the template is {o.th} x {o.tw} cells, a soup {self.size} x {self.size}")
        return self._native.match_counts(templates)

    def components(self, neighbourhood: str = "moore", max_objects: int = 1 << 20, hashes: bool = True):
        """The objects of every soup's current board, each soup its own torus: :class:`ops.SoupComponents` ``(count, soup,
        anchor, population, bbox, hash, truncated)`` sorted by ``(soup, row, col)``, anchors and boxes in the soup's own
        coordinates; the arguments are :meth:`Simulation.components`'s.  HIP: the labelling kernels run once over the whole
        store; only the counters and the records leave the device.  A pending :meth:`step` is included."""
        from ..ops.components import SoupComponents

        # (the native side refuses an unknown neighbourhood, max_objects < 1 and 2^31 cells or more, naming the value)
        count, soup, anchor, pop, bbox, h, truncated, _ = self._native.components(neighbourhood, int(max_objects), bool(hashes), True)
        return SoupComponents(int(count), soup, anchor, pop, bbox, h, bool(truncated))

    def component_counts(self, neighbourhood: str = "moore") -> np.ndarray:
        """An ``(n,)`` uint32 array: the objects of every soup.  Only the counters leave the device; a pending :meth:`step`
        is included."""
        return self._native.components(neighbourhood, 1, False, False)[7]

    def stats(self) -> dict:
        """``kernel`` (``soups@64``, ``soups@128``, ``soups@256``; ``:rule`` appended for the generic variant), ``launches``,
        ``settled``, ``reached`` (the generation of the unsettled soups), ``backend``, ``rule``, ``workgroup``."""
        return dict(self._native.stats())
