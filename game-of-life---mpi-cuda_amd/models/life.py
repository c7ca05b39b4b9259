"""The flagship "model": a Game of Life simulation on one rank of a (possibly multi-GPU) job.

Reference behaviour being reproduced (cited for parity checks):

* board = P stacked N x N tiles forming a (P*N) x N torus (``gol-main.c:76``, ``gol-main.c:84-87``);
* rule B3/S23 (``gol-with-cuda.cu:239-257``);
* patterns 0-4 (``gol-with-cuda.cu:55-171``) plus pattern 5 (seeded random, decomposition-invariant);
* per-rank dump files (``gol-main.c:17-28, 64-73, 134-139``).

The heavy lifting is native: :class:`Simulation` drives a ``_gol.Engine`` (HIP or CPU backend).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .._native import _gol
from ..ops.bitpack import unpack_words


def _tri(name: str) -> int:
    """GOL_* switch with an auto default: 1 on, 0 off, -1 auto (the engine decides by measurement)."""
    v = os.environ.get(name, "auto")
    return -1 if v == "auto" else int(int(v) != 0)


def default_backend() -> str:
    b = os.environ.get("GOL_BACKEND", "auto")
    if b != "auto":
        return b
    return "hip" if _gol.hip_device_count() > 0 else "cpu"


class Simulation:
    """One rank's view of a Game of Life job.

    Parameters
    ----------
    N:            the reference ``worldSize`` (per-rank tile side), or the global side with ``global_mode``.
    transport:    a ``_gol.Transport``; defaults to a single-rank transport.  See
                  :mod:`gol_amd.parallel` for torch.distributed / RCCL / thread transports.
    backend:      ``"hip"``, ``"cpu"`` or ``"auto"``.
    halo_depth:   generations per halo exchange (<= 128 in 1-D, <= 63 in 2-D; 0 = auto, as in
                  Engine::Engine: 128 for 1-D strips of >= 2048 rows with neighbours (or the
                  self-exchange) and for ranks that can run two sub-tiles, 56 for 2-D tiles of >= 2048
                  rows with neighbours, otherwise 32).
    rule:         the life-like rule, ``"B36/S23"`` or an alias (conway, life, highlife, daynight, seeds,
                  replicator); default B3/S23 (GOL_RULE).  A ``V`` or ``H`` directly after the second list counts the
                  von Neumann (N, S, W, E; digits 0..4) or hexagonal (N, S, W, E, NW, SE; digits 0..6) neighbourhood
                  instead of Moore's eight: ``"B13/S13V"``, ``"B2/S34H"``.  B3/S23 runs the specialised bit-sliced kernels;
                  any other B0-free rule the generic ones (HIP: ``step_rule``, CPU: a bit-sliced count),
                  without ``compat``, ``subtiles=2`` or the B3/S23-only kernels.
                  A third field makes a Generations rule: ``"B2/S345/C4"`` (also ``S.../B.../C<n>`` and the bare
                  ``345/2/4``, survive / birth / states), 3 to 9 states: 0 dead, 1 alive, 2 .. C-1 dying.  A live cell
                  that does not survive decays through the dying states, which count as no neighbour and cannot be born
                  (``ops.numpy_generations`` is the definition).  :attr:`states` gives C; :meth:`board`, :meth:`window`
                  and :meth:`set_board` then speak states, :meth:`state_counts` counts them, and :meth:`words`,
                  :meth:`population`, :meth:`density`, :meth:`fingerprint`, :meth:`signature`, :meth:`snapshot`,
                  :meth:`match` and :meth:`stamp` act on the live cells (state 1); a stamped cell is alive and not
                  dying, ``replace`` and ``clear`` leave dying cells dying.  HIP: ``step_gen`` runs every pass
                  (``stats()["kernel"]`` is ``gen@K``, eager launches, passes of at most
                  ``max_generations_depth(C)`` generations).  One rank, Moore, no recording mode, ``compat``,
                  ``subtiles=2``, ``self_exchange``, ``force_split`` or specialised kernel; checkpoints, ``save_rle``,
                  dumps and the tensor calls are refused in this version.
                  ``"R5,C0,M1,S34..58,B34..45,NM"`` (or the alias ``"bosco"``) is a Larger than Life rule: two states, the
                  (2R+1) x (2R+1) box around a cell with R from 1 to 7, the cell itself counted iff M is 1, birth and
                  survival by count intervals (``ops.numpy_ltl`` is the definition, ``ops.parse_ltl_rule`` the parser;
                  :attr:`ltl` holds ``(R, M, smin, smax, bmin, bmax)``, ``None`` for every other rule).  The board is
                  the ordinary two-state board: every reader and writer works.  HIP: ``step_ltl`` runs one generation
                  per pass (``stats()["kernel"]`` is ``ltl@1``, eager launches).  One rank, a board of at least
                  2R + 1 cells either way, no recording mode, ``compat``, ``subtiles=2``, ``self_exchange``,
                  ``force_split``, specialised kernel or ``kernel_depth`` / ``halo_depth`` above 1; checkpoints,
                  ``SoupBatch`` and ``ops.evolve`` refuse such a rule in this version.
    kernel_depth: generations per kernel pass (HIP; 0 = auto).  A superstep of halo_depth
                  generations runs as several kernel passes in 1-D (communication-avoiding halos).
    kernel:       HIP stencil kernel: ``"auto"`` (candidates timed at init), ``"temporal"``,
                  ``"tile"``, ``"pipe"`` (level-pipelined workgroups; geometry GOL_PIPE=nw,L,wg),
                  ``"resident"`` (test knob GOL_RESIDENT=tiles,nw: plan as for ``tiles`` CUs, 8 or 16 waves per
                  tile), ``"lds"`` or ``"rule"`` (the generic rule kernel, also for B3/S23; GOL_KERNEL).
    decomp/grid:  ``"1d"`` row strips (reference) or ``"2d"`` blocks, optional ``"PxxPy"`` grid.
    width:        board columns (0 = N: the reference's square tiles).  With ``width`` the per-rank
                  strip (or, in global mode, the board) is N rows x ``width`` columns.
    boundary:     ``"torus"`` (default, the reference) or ``"dead"``: a bounded board, every cell outside
                  ``[0, H) x [0, W)`` dead in every generation (GOL_BOUNDARY).  HIP: the bounded rule kernel
                  ``step_rule_bounded`` for every rule, B3/S23 included (generic-kernel speed); without
                  ``compat``, ``subtiles=2`` or the torus-only kernels.  Windows and stamps must lie inside
                  a bounded board.
    census:       census mode (default off; GOL_CENSUS): every generation :meth:`step` computes also yields the
                  global population of that generation, read with :meth:`census`.  HIP: the census kernel
                  ``step_census`` counts inside every pass, for every rule and either boundary (generic-kernel
                  speed, passes of at most ``max_census_depth`` generations, eager launches); without
                  ``compat``, ``subtiles=2`` or the specialised kernels.
    signature:    signature mode (default off; GOL_SIGNATURE): every generation :meth:`step` computes also yields the
                  board signature, a linear position-keyed 64-bit hash equal for every decomposition, and the
                  population of that generation, read with :meth:`signatures`; :meth:`find_cycle` is built on it.
                  HIP: the signature kernel ``step_signature`` hashes inside every pass, for every rule and either
                  boundary (generic-kernel speed, B3/S23 included; passes of at most ``max_signature_depth``
                  generations, eager launches); without ``census`` (it records the population already),
                  ``compat``, ``subtiles=2`` or the specialised kernels.
    film:         film mode (default off; GOL_FILM=r0,c0,rows,cols): ``(r0, c0, rows, cols)``, a window of the global board
                  in :meth:`window`'s coordinates (they wrap on the torus; on a bounded board the window lies inside; at most
                  2^22 cells).  Every generation :meth:`step` computes also yields the window's cells in that generation,
                  read with :meth:`film`.  HIP: the film kernel ``step_film`` stores the window's words inside every pass,
                  for every rule, neighbourhood and either boundary (generic-kernel speed, B3/S23 included; passes of at
                  most ``max_film_depth`` generations, eager launches; the frames wait in a device buffer of GOL_FILM_MB
                  MiB, default 64); without ``census``, ``signature``, ``compat``, ``subtiles=2`` or the specialised kernels.
    density_film: density-film mode (default off; GOL_DENSITY_FILM=block_rows[,block_cols]): ``(block_rows, block_cols)``, or
                  one int for square blocks, :meth:`density`'s block shape (``block_cols`` a multiple of 64; at most 2^20
                  blocks).  Every generation :meth:`step` computes also yields the density map of the whole board in that
                  generation, read with :meth:`density_film`.  HIP: the density kernel ``step_density`` counts the blocks
                  inside every pass, for every rule, neighbourhood and either boundary (generic-kernel speed, B3/S23
                  included; passes of at most ``max_density_depth`` generations, eager launches; the maps wait in a device
                  buffer of GOL_DENSITY_FILM_MB MiB, default 64); without ``census``, ``signature``, ``film``, ``compat``,
                  ``subtiles=2`` or the specialised kernels.
    envelope:     envelope mode (default off; GOL_ENVELOPE): the simulation keeps the OR of every generation of the board
                  since the last reset, one bit per cell: every cell that was ever alive.  :meth:`init`, :meth:`set_board`,
                  :meth:`restore` and :meth:`envelope_clear` reset it to the current board; :meth:`stamp` ORs the stamped
                  board in.  Read with :meth:`envelope`, :meth:`envelope_window`, :meth:`envelope_density` and
                  :meth:`envelope_population`.  HIP: a third board-sized buffer, and the envelope kernel ``step_envelope``
                  ORs into it inside every pass, for every rule, neighbourhood and either boundary (generic-kernel speed,
                  B3/S23 included; passes of at most ``max_envelope_depth`` generations, eager launches); without
                  ``census``, ``signature``, ``film``, ``density_film``, ``compat``, ``subtiles=2`` or the specialised kernels.
    compat:       reproduce the reference's halo quirks (frozen gen-0 halos, P<=2 swap).
    watchdog:     seconds without progress before the job is aborted (0 = off; GOL_WATCHDOG).
    """

    def __init__(
        self,
        N: int,
        transport=None,
        *,
        backend: str = "auto",
        global_mode: bool = False,
        decomp: str = "1d",
        grid: str = "",
        halo_depth: int = int(os.environ.get("GOL_HALO_DEPTH", "0")),
        kernel_depth: int = int(os.environ.get("GOL_KERNEL_DEPTH", "0")),
        overlap: bool = True,
        graph: bool = True,
        compat: bool = False,
        device: Optional[int] = None,
        kernel: str = os.environ.get("GOL_KERNEL", "auto"),
        rows_per_wave: int = 0,
        waves_target: int = 0,
        profile: bool = False,
        watchdog: float = float(os.environ.get("GOL_WATCHDOG", "0")),
        tile_waves: int = int(os.environ.get("GOL_TILE_WAVES", "8")),
        force_split: bool = os.environ.get("GOL_FORCE_SPLIT", "0") == "1",
        schedule: str = os.environ.get("GOL_SCHEDULE", "auto"),
        run_hint: int = 0,
        sub_occ: int = int(os.environ.get("GOL_SUB_OCC", "2")),
        self_exchange: bool = os.environ.get("GOL_SELF_EXCHANGE", "0") == "1",
        subtiles: int = -1 if os.environ.get("GOL_SUBTILES", "auto") == "auto" else int(os.environ["GOL_SUBTILES"]),
        width: int = 0,
        subtile_overlap: Optional[int] = None,
        rule: str = os.environ.get("GOL_RULE", "B3/S23"),
        boundary: Optional[str] = None,
        census: Optional[bool] = None,
        signature: Optional[bool] = None,
        film=None,
        density_film=None,
        envelope: Optional[bool] = None,
    ):
        self.transport = transport if transport is not None else _gol.SelfTransport()
        P, rank = self.transport.size(), self.transport.rank()
        self.backend = default_backend() if backend == "auto" else backend
        self.decomposition = _gol.make_decomposition(N, P, global_mode, decomp, grid, int(width))
        self.geometry = _gol.make_geometry(self.decomposition, rank)
        cfg = _gol.EngineConfig()
        cfg.backend = self.backend
        cfg.halo_depth = halo_depth
        cfg.kernel_depth = kernel_depth
        cfg.overlap = overlap
        cfg.graph = graph
        cfg.compat = compat
        cfg.kernel = kernel
        cfg.rule = rule  # (ValueError on a string that is no B0-free rule)
        if cfg.rule != "B3/S23":
            if compat:
                raise ValueError(f"compat=True with rule {cfg.rule}: the reference has one rule, B3/S23")
            if int(subtiles) == 2:
                raise ValueError(f"subtiles=2 runs B3/S23 only, not rule {cfg.rule}")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} implements B3/S23 only, not rule {cfg.rule}")
        if boundary is None:  # (read per call, so a test or a driver can set it between simulations)
            boundary = os.environ.get("GOL_BOUNDARY", "torus")
        cfg.boundary = boundary  # (ValueError on anything but torus or dead, naming it)
        self.states = int(_gol.parse_rule_states(cfg.rule))  # 2, or C of a Generations rule
        if cfg.boundary == "dead":
            if compat:
                raise ValueError("compat=True with boundary dead: the reference is a torus")
            if int(subtiles) == 2:
                raise ValueError("subtiles=2 implements the torus only, not boundary dead")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} implements the torus only, not boundary dead")
        if census is None:  # (read per call, as the boundary is)
            census = os.environ.get("GOL_CENSUS", "0").lower() in ("1", "true", "yes", "on")
        cfg.census = bool(census)
        if cfg.census:
            if compat:
                raise ValueError("census=True with compat=True: compat mode runs the reference's loop, not the census kernel")
            if int(subtiles) == 2:
                raise ValueError("census=True with subtiles=2: the sub-tile halves do not run the census kernel")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} counts no census: the census kernel runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_census_depth():
                raise ValueError(
                    f"census=True: kernel_depth {kernel_depth} exceeds the census kernel's deepest pass, "
                    f"{_gol.max_census_depth()} generations"
                )
        if signature is None:  # (read per call, as the census mode is)
            signature = os.environ.get("GOL_SIGNATURE", "0").lower() in ("1", "true", "yes", "on")
        cfg.signature = bool(signature)
        if cfg.signature:
            if cfg.census:
                raise ValueError("signature=True with census=True: signature mode already records the population")
            if compat:
                raise ValueError("signature=True with compat=True: compat mode runs the reference's loop, not the signature kernel")
            if int(subtiles) == 2:
                raise ValueError("signature=True with subtiles=2: the sub-tile halves do not run the signature kernel")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} records no signatures: the signature kernel runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_signature_depth():
                raise ValueError(
                    f"signature=True: kernel_depth {kernel_depth} exceeds the signature kernel's deepest pass, "
                    f"{_gol.max_signature_depth()} generations"
                )
        if film is None:  # (read per call, as the census mode is)
            env = os.environ.get("GOL_FILM", "")
            if env:
                try:
                    film = tuple(int(v) for v in env.split(","))
                except ValueError:
                    film = ()
                if len(film) != 4:
                    raise ValueError(f"GOL_FILM must be r0,c0,rows,cols (got {env!r})")
        if film is not None:
            film = tuple(int(v) for v in film)
            if len(film) != 4:
                raise ValueError(f"film must be (r0, c0, rows, cols), got {film!r}")
            r0, c0, rows, cols = film
            H, W = self.decomposition.H, self.decomposition.W
            if cfg.census or cfg.signature:
                raise ValueError("film with census=True or signature=True: one per-generation record per simulation")
            if compat:
                raise ValueError("film with compat=True: compat mode runs the reference's loop, not the film kernel")
            if int(subtiles) == 2:
                raise ValueError("film with subtiles=2: the sub-tile halves do not run the film kernel")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} stores no frames: the film kernel runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_film_depth():
                raise ValueError(
                    f"film: kernel_depth {kernel_depth} exceeds the film kernel's deepest pass, "
                    f"{_gol.max_film_depth()} generations"
                )
            if not (1 <= rows <= H and 1 <= cols <= W):
                raise ValueError(f"film: a window of {rows} x {cols} cells: rows must be in 1..{H} and columns in 1..{W} (the board)")
            if cfg.boundary == "dead" and (r0 < 0 or c0 < 0 or r0 + rows > H or c0 + cols > W):
                raise ValueError(
                    f"film: the {rows} x {cols} rectangle at ({r0}, {c0}) does not lie inside the bounded {H} x {W} board"
                )
            if rows * cols > _gol.film_max_cells:
                raise ValueError(
                    f"film: a window of {rows} x {cols} cells has more than 2^22 cells; read larger rectangles with window()"
                )
            cfg.film = film
        if density_film is None:  # (read per call, as the census mode is)
            env = os.environ.get("GOL_DENSITY_FILM", "")
            if env:
                try:
                    density_film = tuple(int(v) for v in env.split(","))
                except ValueError:
                    density_film = ()
                if len(density_film) not in (1, 2):
                    raise ValueError(f"GOL_DENSITY_FILM must be block_rows[,block_cols] (got {env!r})")
        if density_film is not None:
            if isinstance(density_film, (int, np.integer)):
                density_film = (density_film,)
            density_film = tuple(int(v) for v in density_film)
            if len(density_film) == 1:
                density_film = density_film * 2
            if len(density_film) != 2:
                raise ValueError(f"density_film must be (block_rows, block_cols) or one int, got {density_film!r}")
            brows, bcols = density_film
            H, W = self.decomposition.H, self.decomposition.W
            if cfg.census or cfg.signature or cfg.film is not None:
                raise ValueError("density_film with census=True, signature=True or film: one per-generation record per simulation")
            if compat:
                raise ValueError("density_film with compat=True: compat mode runs the reference's loop, not the density kernel")
            if int(subtiles) == 2:
                raise ValueError("density_film with subtiles=2: the sub-tile halves do not run the density kernel")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} counts no density maps: the density kernel runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_density_depth():
                raise ValueError(
                    f"density_film: kernel_depth {kernel_depth} exceeds the density kernel's deepest pass, "
                    f"{_gol.max_density_depth()} generations"
                )
            if brows < 1:
                raise ValueError(f"density_film: block_rows must be >= 1 (got {brows})")
            if bcols < 64 or bcols % 64:
                raise ValueError(f"density_film: block_cols must be a multiple of 64, the cells of a board word (got {bcols})")
            if min(brows, H) * min(bcols, -(-W // 64) * 64) > 0xFFFFFFFF:
                raise ValueError(f"density_film: a block of {brows} x {bcols} cells holds more than 2^32 - 1 cells, its count would not fit")
            grows, gcols = -(-H // brows), -(-W // bcols)
            if grows * gcols > _gol.density_film_max_blocks:
                raise ValueError(
                    f"density_film: blocks of {brows} x {bcols} cells make a grid of {grows} x {gcols} blocks, more than 2^20 "
                    "per generation; read finer grids with density()"
                )
            cfg.density_film = density_film
        if envelope is None:  # (read per call, as the census mode is)
            envelope = os.environ.get("GOL_ENVELOPE", "0") not in ("", "0")
        if envelope:
            if cfg.census or cfg.signature or cfg.film is not None or cfg.density_film is not None:
                raise ValueError(
                    "envelope with census=True, signature=True, film or density_film: one in-kernel record per simulation"
                )
            if compat:
                raise ValueError("envelope with compat=True: compat mode runs the reference's loop, not the envelope kernel")
            if int(subtiles) == 2:
                raise ValueError("envelope with subtiles=2: the sub-tile halves do not run the envelope kernel")
            if self.backend == "hip" and kernel in ("temporal", "tile", "pipe", "resident", "lds"):
                raise ValueError(f"kernel {kernel!r} keeps no envelope: the envelope kernel runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_envelope_depth():
                raise ValueError(
                    f"envelope: kernel_depth {kernel_depth} exceeds the envelope kernel's deepest pass, "
                    f"{_gol.max_envelope_depth()} generations"
                )
        if self.states > 2:  # a Generations rule: what this version does not run with one, each named
            r = cfg.rule

            def refuse(option: str, why: str):
                raise ValueError(f"{option} with the Generations rule {r}: {why}")

            if P > 1:
                raise ValueError(f"the Generations rule {r} on {P} ranks: Generations rules run on one rank")
            if cfg.census:
                refuse("census=True", "the census kernel counts two-state boards")
            if cfg.signature:
                refuse("signature=True", "the signature kernel hashes two-state boards")
            if cfg.film is not None:
                refuse("film", "the film kernel stores two-state frames")
            if cfg.density_film is not None:
                refuse("density_film", "the density kernel counts two-state boards")
            if envelope:
                refuse("envelope=True", "the envelope kernel records two-state boards")
            if bool(self_exchange):
                refuse("self_exchange=True", "the exchange of the decay planes is not built")
            if bool(force_split):
                refuse("force_split=True", "the split schedule's exchange of the decay planes is not built")
            if self.backend == "hip" and kernel not in ("auto", "rule"):
                refuse(f"kernel {kernel!r}", "step_gen runs every pass (use auto or rule)")
            if self.backend == "hip" and int(kernel_depth) > _gol.max_generations_depth(self.states):
                refuse(
                    f"kernel_depth {kernel_depth}",
                    f"the Generations kernel's deepest pass with {self.states} states is "
                    f"{_gol.max_generations_depth(self.states)} generations",
                )
        self.ltl = _gol.parse_ltl_rule(cfg.rule)  # (R, M, smin, smax, bmin, bmax) of a Larger than Life rule, else None
        if self.ltl is not None:  # what this version does not run with such a rule, each named
            r = cfg.rule

            def refuse_ltl(option: str, why: str):
                raise ValueError(f"{option} with the Larger than Life rule {r}: {why}")

            if P > 1:
                raise ValueError(f"the Larger than Life rule {r} on {P} ranks: Larger than Life rules run on one rank")
            if cfg.census:
                refuse_ltl("census=True", "the census kernel counts inside the radius-1 kernels")
            if cfg.signature:
                refuse_ltl("signature=True", "the signature kernel hashes inside the radius-1 kernels")
            if cfg.film is not None:
                refuse_ltl("film", "the film kernel stores frames inside the radius-1 kernels")
            if cfg.density_film is not None:
                refuse_ltl("density_film", "the density kernel counts inside the radius-1 kernels")
            if envelope:
                refuse_ltl("envelope=True", "the envelope kernel records inside the radius-1 kernels")
            if bool(self_exchange):
                refuse_ltl("self_exchange=True", "the exchange of halos of depth R is not built")
            if bool(force_split):
                refuse_ltl("force_split=True", "the split schedule is not built for a box of range R")
            if self.backend == "hip" and kernel not in ("auto", "rule"):
                refuse_ltl(f"kernel {kernel!r}", "step_ltl runs every pass (use auto or rule)")
            if int(kernel_depth) not in (0, 1):
                refuse_ltl(f"kernel_depth {kernel_depth}", "a pass is one generation (auto or 1)")
            if int(halo_depth) not in (0, 1):
                refuse_ltl(f"halo_depth {halo_depth}", "a superstep is one generation (auto or 1)")
            side = 2 * self.ltl[0] + 1
            H, W = self.decomposition.H, self.decomposition.W
            if H < side or W < side:
                raise ValueError(
                    f"rule {r} on a {H} x {W} board: the box of range {self.ltl[0]} needs a board of at least {side} x {side} "
                    "cells, so that no neighbour is counted twice"
                )
        cfg.envelope = bool(envelope)
        cfg.subtiles = int(subtiles)  # 2 / 0 / -1 auto: two sub-tiles per rank on two streams (HIP, 1-D)
        cfg.run_hint = int(run_hint)  # generations of the runs to come: one replay graph covers them
        cfg.rows_per_wave = rows_per_wave
        cfg.waves_target = waves_target
        cfg.profile = profile
        cfg.watchdog_s = float(watchdog)
        cfg.tile_waves = int(tile_waves)
        cfg.tune_tile_waves = "GOL_TILE_WAVES" not in os.environ
        cfg.sub_occ = int(sub_occ)
        # 1 on / 0 off / -1 auto: a candidate of the init-time schedule timing (GOL_* env defaults)
        if subtile_overlap is None:  # 0 off, 1 on (half 0's interior overlaps the exchange), auto: timed
            v = os.environ.get("GOL_SUBTILE_OVERLAP", "auto")
            subtile_overlap = -1 if v == "auto" else int(v)
        cfg.subtile_overlap = int(subtile_overlap)
        cfg.self_exchange = bool(self_exchange)
        cfg.force_split = bool(force_split)
        cfg.sched = schedule
        cfg.graph_rccl = _tri("GOL_GRAPH_RCCL")
        cfg.plan_xcds = int(os.environ.get("GOL_PLAN_XCDS", "8"))
        if self.backend == "hip":
            n = _gol.hip_device_count()
            if n <= 0:
                raise RuntimeError("backend 'hip' requested but no HIP device is visible")
            cfg.device = (rank if device is None else device) % n
        self.config = cfg
        self.engine = _gol.Engine.create(self.geometry, cfg, self.transport)
        self.pattern = None

    # -- lifecycle -------------------------------------------------------------------------
    def init(self, pattern: int = 5, seed: int = 0x5EED) -> "Simulation":
        self.pattern = _gol.make_pattern(pattern, self.decomposition, seed)
        self.engine.init(self.pattern)
        return self

    def step(self, generations: int = 1) -> "Simulation":
        self.engine.run(int(generations))
        return self

    run = step

    def synchronize(self) -> None:
        self.engine.synchronize()

    # -- state -----------------------------------------------------------------------------
    @property
    def generation(self) -> int:
        return self.engine.generation

    def words(self) -> np.ndarray:
        """Local tile as packed uint64 words, shape (h, ceil(w/64)); bit b of word c = column 64c+b."""
        return self.engine.tile_words()

    def board(self) -> np.ndarray:
        """Local tile as a (h, w) uint8 array of 0/1 cells; under a Generations rule, of the states 0 .. C-1."""
        if self.states > 2:
            return self.engine.state_tile()
        return unpack_words(self.words(), self.geometry.w)

    def set_board(self, cells: np.ndarray) -> None:
        """The local tile from a (h, w) array of 0/1 cells; under a Generations rule, of states (a value >= C is a
        ValueError that names it, and nothing is written)."""
        from ..ops.bitpack import pack_cells

        cells = np.asarray(cells)
        if cells.shape != (self.geometry.h, self.geometry.w):
            raise ValueError(f"expected a {(self.geometry.h, self.geometry.w)} board, got {cells.shape}")
        if self.states > 2:
            if cells.size and (int(cells.min()) < 0 or int(cells.max()) >= self.states):
                bad = int(cells.max()) if int(cells.max()) >= self.states else int(cells.min())
                raise ValueError(f"set_board: state {bad} on the board: rule {self.config.rule} has the states 0 .. {self.states - 1}")
            self.engine.set_state_tile(np.ascontiguousarray(cells, dtype=np.uint8))
            return
        self.engine.set_tile_words(pack_cells(cells))

    def state_counts(self) -> np.ndarray:
        """The cells of the global board in each state: a ``(C,)`` uint64 array (``[1]`` is :meth:`population`).  Needs
        a Generations rule.  HIP: counted on the device, only the counts leave it."""
        if self.states <= 2:
            raise ValueError(f"state_counts() needs a Generations rule (B<digits>/S<digits>/C<n>); rule {self.config.rule} has two states")
        return self.engine.state_counts()

    def _no_ltl(self, what: str) -> None:
        if self.ltl is not None:
            raise ValueError(
                f"{what} is not built for Larger than Life rules in this version (the rule is {self.config.rule}): "
                "a checkpoint's header holds the rule's code, which such a rule does not have"
            )

    def _two_states(self, what: str) -> None:
        if self.states > 2:
            raise ValueError(f"{what} is not built for Generations rules in this version (the rule is {self.config.rule})")

    # -- torch tensors (ops/tensors.py states the dtypes and the stream ordering) ----------------
    # On the HIP backend every tensor argument and result is a CUDA tensor on cuda:<device> and the cells never leave the
    # device (kernels: tensor_kernels.hip); on the CPU backend they are CPU tensors.  ``dtype``: torch.bool, uint8 (the
    # default), float16, bfloat16 or float32; ``out``: a contiguous tensor of the result's shape to fill instead of a new
    # one (it is returned).  Before the engine touches a CUDA tensor the current torch stream of its device is
    # synchronised; the engine synchronises its own stream before the call returns.  Argument errors are ValueErrors,
    # raised before anything is launched.
    def _tensor_device(self):
        from ..ops import tensors

        return tensors.device_of(self.backend, self.config.device)

    def _one_rank(self, what: str) -> None:
        P = self.transport.size()
        if P > 1:
            raise ValueError(f"{what}: this job has {P} ranks; the device-side {what} is built for one rank")

    def board_tensor(self, dtype=None, out=None):
        """This rank's tile as an ``(h, w)`` tensor of 0 and 1: :meth:`board` without the host.  Any rank count; no
        communication.  The current torch stream is synchronised before the engine writes the tensor, and the engine's
        stream before the call returns."""
        from ..ops import tensors

        self._two_states("board_tensor()")
        t = tensors.result((self.geometry.h, self.geometry.w), dtype, self._tensor_device(), out, "board_tensor")
        tensors.sync(t)
        self.engine.read_tile_cells(*tensors.handle(t))
        return t

    def load_tensor(self, cells) -> "Simulation":
        """:meth:`set_board` from an ``(h, w)`` tensor: a cell is alive iff its element ``!= 0`` (2, -1, 0.5 and NaN are
        alive, ``-0.0`` is dead).  Any rank count; ghosts, halos and the envelope follow as after :meth:`set_board`.  The
        current torch stream is synchronised before the engine reads the tensor."""
        from ..ops import tensors

        self._two_states("load_tensor()")
        t = tensors.check_input(cells, (self.geometry.h, self.geometry.w), self._tensor_device(), "load_tensor")
        tensors.sync(t)
        self.engine.write_tile_cells(*tensors.handle(t))
        return self

    def envelope_tensor(self, dtype=None, out=None):
        """``(start, cells)`` as :meth:`envelope` returns them, ``cells`` an ``(h, w)`` tensor.  Needs ``envelope=True``.
        Stream ordering as :meth:`board_tensor`."""
        from ..ops import tensors

        self._need_envelope("envelope_tensor()")
        t = tensors.result((self.geometry.h, self.geometry.w), dtype, self._tensor_device(), out, "envelope_tensor")
        tensors.sync(t)
        start = self.engine.read_envelope_cells(*tensors.handle(t))
        return int(start), t

    def window_tensor(self, r0: int, c0: int, rows: int, cols: int, dtype=None, out=None):
        """:meth:`window` as a ``(rows, cols)`` tensor: same coordinates, wrapping and bounded-board checks.  One rank
        only (more raise, naming the rank count).  Stream ordering as :meth:`board_tensor`."""
        from ..ops import tensors

        r0, c0, rows, cols = int(r0), int(c0), int(rows), int(cols)
        self._two_states("window_tensor()")
        self._one_rank("window_tensor")
        H, W = self.decomposition.H, self.decomposition.W
        if not (1 <= rows <= H and 1 <= cols <= W):
            raise ValueError(f"window_tensor: a window of {rows} x {cols} cells: rows must be in 1..{H} and columns in 1..{W} (the board)")
        self._check_inside("window_tensor", r0, c0, rows, cols)
        t = tensors.result((rows, cols), dtype, self._tensor_device(), out, "window_tensor")
        tensors.sync(t)
        self.engine.read_window_cells(r0, c0, rows, cols, *tensors.handle(t))
        return t

    def step_film(self, generations: int, dtype=None, out=None):
        """``generations`` generations whose frames go straight into a ``(generations, rows, cols)`` tensor ``f``:
        ``f[i]`` is the film window at generation ``g0 + 1 + i``, ``g0`` the generation before the call; what
        ``step(generations); film()`` returns, unpacked where the kernel stored it.  Needs ``film=...``, one rank and an
        empty film record (call :meth:`film_clear` first, otherwise a ValueError); afterwards the record is empty and
        starts at the generation reached, as after :meth:`film_clear`.  Stream ordering as :meth:`board_tensor`."""
        from ..ops import tensors

        generations = int(generations)
        if self.config.film is None:
            raise ValueError("step_film() needs a simulation built with film=(r0, c0, rows, cols) (or GOL_FILM)")
        self._one_rank("step_film")
        if generations < 0:
            raise ValueError(f"step_film: generations = {generations} is negative")
        _, _, rows, cols = self.config.film
        t = tensors.result((generations, rows, cols), dtype, self._tensor_device(), out, "step_film")
        tensors.sync(t)
        self.engine.run_film_cells(generations, *tensors.handle(t))  # (a non-empty record: ValueError, nothing has run)
        return t

    def population(self) -> int:
        """Global live-cell count (collective)."""
        return int(self.engine.population())

    def census(self):
        """``(start, counts)``: ``counts[i]`` is the global population at generation ``start + 1 + i``, a uint64 array
        with one entry per generation computed since the record was cleared (by :meth:`init`, :meth:`load_rle`,
        :meth:`restore` or :meth:`census_clear`).  Collective; every rank gets the same array.  Needs
        ``census=True``."""
        if not self.config.census:
            raise ValueError("census() needs a simulation built with census=True (or GOL_CENSUS=1)")
        start, counts = self.engine.census()
        return int(start), counts

    def census_clear(self) -> None:
        """Forget the recorded series; the next one starts at the generation reached."""
        if not self.config.census:
            raise ValueError("census_clear() needs a simulation built with census=True (or GOL_CENSUS=1)")
        self.engine.census_clear()

    def fingerprint(self) -> int:
        """Decomposition-invariant fingerprint of the global board (collective)."""
        return int(self.engine.fingerprint())

    def signature(self) -> int:
        """The board signature of the current global board (collective; any mode): the linear, position-keyed 64-bit
        hash that signature mode records for every generation (:func:`ops.numpy_signature` is its oracle)."""
        return int(self.engine.signature())

    def signatures(self):
        """``(start, signatures, populations)``: entry ``i`` of the two uint64 arrays is the board signature and the
        global population at generation ``start + 1 + i``, one entry per generation computed since the record was
        cleared (by :meth:`init`, :meth:`load_rle`, :meth:`restore` or :meth:`signatures_clear`; :meth:`stamp` leaves it
        running).  Collective; every rank gets the same arrays.  Needs ``signature=True``."""
        if not self.config.signature:
            raise ValueError("signatures() needs a simulation built with signature=True (or GOL_SIGNATURE=1)")
        start, sigs, pops = self.engine.signatures()
        return int(start), sigs, pops

    def signatures_clear(self) -> None:
        """Forget the recorded series; the next one starts at the generation reached."""
        if not self.config.signature:
            raise ValueError("signatures_clear() needs a simulation built with signature=True (or GOL_SIGNATURE=1)")
        self.engine.signatures_clear()

    def film(self):
        """``(start, frames)``: ``frames[i]`` is what ``window(r0, c0, rows, cols)`` would return at generation
        ``start + 1 + i``, a ``(n, rows, cols)`` uint8 array with one frame per generation computed since the record was
        cleared (by :meth:`init`, :meth:`load_rle`, :meth:`restore` or :meth:`film_clear`; :meth:`stamp` and
        :meth:`set_board` leave it running).  Collective; every rank gets the same array (:func:`ops.numpy_film` is its
        oracle).  Needs ``film=(r0, c0, rows, cols)``."""
        if self.config.film is None:
            raise ValueError("film() needs a simulation built with film=(r0, c0, rows, cols) (or GOL_FILM)")
        start, frames = self.engine.film()
        return int(start), frames

    def film_clear(self) -> None:
        """Forget the recorded frames; the next record starts at the generation reached."""
        if self.config.film is None:
            raise ValueError("film_clear() needs a simulation built with film=(r0, c0, rows, cols) (or GOL_FILM)")
        self.engine.film_clear()

    def density_film(self):
        """``(start, maps)``: ``maps[i]`` is what ``density(block_rows, block_cols)`` would return at generation
        ``start + 1 + i``, a ``(n, grid_rows, grid_cols)`` uint32 array with one map per generation computed since the
        record was cleared (by :meth:`init`, :meth:`load_rle`, :meth:`restore` or :meth:`density_film_clear`;
        :meth:`stamp` and :meth:`set_board` leave it running).  Collective; every rank gets the same array
        (:func:`ops.numpy_density_film` is its oracle).  Needs ``density_film=(block_rows, block_cols)``."""
        if self.config.density_film is None:
            raise ValueError("density_film() needs a simulation built with density_film=(block_rows, block_cols) (or GOL_DENSITY_FILM)")
        start, maps = self.engine.density_film()
        return int(start), maps

    def density_film_clear(self) -> None:
        """Forget the recorded maps; the next record starts at the generation reached."""
        if self.config.density_film is None:
            raise ValueError(
                "density_film_clear() needs a simulation built with density_film=(block_rows, block_cols) (or GOL_DENSITY_FILM)"
            )
        self.engine.density_film_clear()

    def _need_envelope(self, what: str) -> None:
        if not self.config.envelope:
            raise ValueError(f"{what} needs a simulation in envelope mode, built with envelope=True (or GOL_ENVELOPE=1)")

    def envelope(self):
        """``(start, cells)``: ``cells`` is this rank's tile of the envelope as :meth:`board` returns the board, a
        ``(h, w)`` uint8 array with a 1 for every cell that was alive in any of the generations ``start ..
        generation``; ``start`` is the generation of the last reset (:meth:`init`, :meth:`load_rle`, :meth:`set_board`,
        :meth:`restore`, :meth:`envelope_clear`).  :func:`ops.numpy_envelope` is its oracle.  Needs ``envelope=True``."""
        self._need_envelope("envelope()")
        start, words = self.engine.envelope()
        return int(start), unpack_words(words, self.geometry.w)

    def envelope_window(self, r0: int, c0: int, rows: int, cols: int) -> np.ndarray:
        """:meth:`window` of the envelope: same coordinates, wrapping and bounded-board checks.  Collective."""
        self._need_envelope("envelope_window()")
        self._check_inside("envelope_window", int(r0), int(c0), int(rows), int(cols))
        return self.engine.envelope_window(int(r0), int(c0), int(rows), int(cols))

    def envelope_density(self, block_rows: int, block_cols: Optional[int] = None) -> np.ndarray:
        """:meth:`density` of the envelope: ever-alive cells per block of the global board.  Collective."""
        self._need_envelope("envelope_density()")
        block_cols = block_rows if block_cols is None else block_cols
        if int(block_rows) < 1 or int(block_cols) < 64 or int(block_cols) % 64:
            raise ValueError(f"density blocks are >= 1 rows x a multiple of 64 columns, got {block_rows} x {block_cols}")
        return self.engine.envelope_density(int(block_rows), int(block_cols))

    def envelope_population(self) -> int:
        """The number of cells of the global board that were ever alive since the last reset (collective)."""
        self._need_envelope("envelope_population()")
        return int(self.engine.envelope_population())

    def envelope_clear(self) -> None:
        """Reset the envelope to the current board; it starts again at the generation reached."""
        self._need_envelope("envelope_clear()")
        self.engine.envelope_clear()

    def snapshot(self) -> None:
        """Keep a copy of the current board (a third board buffer, allocated on first use) for :meth:`snapshot_diff`."""
        self.engine.snapshot()

    def snapshot_diff(self) -> int:
        """The number of cells of the global board that differ from the last :meth:`snapshot` (collective)."""
        return int(self.engine.snapshot_diff())

    def find_cycle(self, max_generations: int, chunk: int = 256):
        """Step the board until it repeats: ``None`` when it has not within ``max_generations`` generations from the
        current one, else a :class:`ops.Cycle` ``(transient, period, generation, population)``: the board entered its
        cycle at generation ``transient`` (of the simulation's generation counter; the search starts at the current
        generation, so call it at generation 0 for the transient of the initial board), repeats every ``period``
        generations, and now stands at ``generation``, on the cycle, with ``population`` live cells.  Collective;
        every rank returns the same value.  Needs ``signature=True``.

        The board is stepped ``chunk`` generations at a time and each generation's signature looked up among the
        earlier ones.  A hit is confirmed on the device, cell by cell: the board is copied, stepped one candidate
        period further and compared.  So the period and the membership of the final board in the cycle are exact,
        whatever the hash does (a collision is dropped and the search goes on); the transient rests on the 64-bit
        signatures telling the generations before it apart.  The record of :meth:`signatures` is consumed.  The
        confirmation may step up to one period beyond ``max_generations``."""
        from ..ops.cycle import Cycle, find_repeat

        if not self.config.signature:
            raise ValueError("find_cycle() needs a simulation built with signature=True (or GOL_SIGNATURE=1)")
        max_generations, chunk = int(max_generations), int(chunk)
        if max_generations < 1 or chunk < 1:
            raise ValueError(f"find_cycle: max_generations and chunk must be >= 1, got {max_generations}, {chunk}")
        g0 = self.generation
        end = g0 + max_generations
        self.signatures_clear()
        seen = {self.signature(): g0}

        def verify(g_prev: int, g: int) -> bool:
            # the board stands at some G >= g: board(G) == board(G + p) proves the period (and G on the cycle)
            self.snapshot()
            self.step(g - g_prev)
            return self.snapshot_diff() == 0

        read_to = g0  # the generation the series has been searched up to
        while True:
            if self.generation == read_to:  # (else: generations stepped by a rejected confirmation are still unread)
                if read_to >= end:
                    return None
                self.step(min(chunk, end - read_to))
            start, sigs, _ = self.signatures()
            self.signatures_clear()
            read_to = start + len(sigs)
            hit = find_repeat(sigs, seen, start + 1, verify)
            if hit is not None:
                return Cycle(hit[0], hit[1] - hit[0], self.generation, self.population())

    def stats(self) -> dict:
        return self.engine.stats()

    def describe(self) -> str:
        return self.engine.describe()

    # -- views and patterns ----------------------------------------------------------------
    # Global board coordinates (on the torus they wrap; on a bounded board a rectangle lies inside the board); all of
    # these are collective, and every rank gets the same result.
    def window(self, r0: int, c0: int, rows: int, cols: int) -> np.ndarray:
        """``rows x cols`` cells of the global board from ``(r0, c0)`` on as a uint8 array.  The window may
        start anywhere (coordinates wrap), cross the board's seams and any rank boundary; it is at most the
        board's size.  On a bounded board (``boundary="dead"``) it must lie inside the board.  On the HIP backend
        only the window's bytes leave the device."""
        self._check_inside("window", int(r0), int(c0), int(rows), int(cols))
        if self.states > 2:  # (a Generations rule: the states 0 .. C-1)
            return self.engine.state_window(int(r0), int(c0), int(rows), int(cols))
        return self.engine.window(int(r0), int(c0), int(rows), int(cols))

    def _check_inside(self, what: str, r0: int, c0: int, rows: int, cols: int) -> None:
        """On a bounded board a rectangle must lie inside the board (nothing wraps); every rank raises alike."""
        H, W = self.decomposition.H, self.decomposition.W
        if self.config.boundary == "dead" and (r0 < 0 or c0 < 0 or r0 + rows > H or c0 + cols > W):
            raise ValueError(
                f"{what}: the {rows} x {cols} rectangle at ({r0}, {c0}) does not lie inside the bounded {H} x {W} board"
            )

    def density(self, block_rows: int, block_cols: Optional[int] = None) -> np.ndarray:
        """Live cells per ``block_rows x block_cols`` block of the global board: a uint32 array of
        ``ceil(H / block_rows) x ceil(W / block_cols)`` counts (edge blocks are partial).  ``block_cols``
        (default: ``block_rows``) must be a multiple of 64."""
        block_cols = block_rows if block_cols is None else block_cols
        if int(block_rows) < 1 or int(block_cols) < 64 or int(block_cols) % 64:
            raise ValueError(f"density blocks are >= 1 rows x a multiple of 64 columns, got {block_rows} x {block_cols}")
        return self.engine.density(int(block_rows), int(block_cols))

    @staticmethod
    def _pattern(pattern):
        """An RLE path, RLE text, a 2-D 0/1 array or a native RlePattern -> native RlePattern."""
        from ..ops.rle import pattern_from_cells

        if isinstance(pattern, _gol.RlePattern):
            return pattern
        if isinstance(pattern, os.PathLike):
            pattern = os.fspath(pattern)
        if isinstance(pattern, str):
            if "!" in pattern or "\n" in pattern:  # (no path holds RLE's end mark or a line break)
                return _gol.parse_rle(pattern)
            if not os.path.exists(pattern):
                raise FileNotFoundError(f"no RLE file {pattern!r}")
            return _gol.read_rle_file(pattern)
        return pattern_from_cells(pattern)

    def stamp(self, pattern, at="center", mode: str = "or") -> "Simulation":
        """Combine a pattern (an RLE path, RLE text or a 2-D 0/1 array) with the live board, its first cell at
        ``at = (row, col)`` or centred.  ``mode``: ``"or"``, ``"replace"`` (the pattern's bounding rectangle is
        overwritten), ``"xor"`` or ``"clear"`` (cells die where the pattern is live).  The pattern may cross
        the seams and rank boundaries (on a bounded board it must lie inside the board); one larger than the
        board is refused, and so is ``compat`` mode."""
        p = self._pattern(pattern)
        if mode not in ("or", "replace", "xor", "clear"):
            raise ValueError(f"stamp mode must be or, replace, xor or clear, got {mode!r}")
        H, W = self.decomposition.H, self.decomposition.W
        if p.rows > H or p.cols > W:
            raise ValueError(f"the pattern ({p.rows} x {p.cols}) is larger than the board ({H} x {W})")
        if self.config.compat:
            raise ValueError("stamp is refused in compat mode: its halos are frozen at generation 0")
        if isinstance(at, str):
            if at != "center":
                raise ValueError(f"at must be (row, col) or 'center', got {at!r}")
            at = ((H - p.rows) // 2, (W - p.cols) // 2)
        self._check_inside("stamp", int(at[0]), int(at[1]), p.rows, p.cols)
        self.engine.stamp(p, int(at[0]), int(at[1]), mode)
        return self

    # -- pattern matching (ops/match.py states what a template is and when it matches) -----------
    def _match_templates(self, what: str, pattern_or_template, margin: int, orientations):
        """The native ``[(orientation id, template)]`` of a call; every refusal is a ValueError, before any launch."""
        from ..ops.match import as_template, want_all

        self._one_rank(what)
        all_ = want_all(orientations)
        t = as_template(pattern_or_template, margin)
        H, W = self.decomposition.H, self.decomposition.W
        ts = t.native.orientations(all_)
        for _, o in ts:
            if o.th > H or o.tw > W:
                raise ValueError(f"{what}: the template is {o.th} x {o.tw} cells, the board {H} x {W}")
        return ts

    def match(self, pattern_or_template, *, margin: int = 1, orientations=False, max_hits: int = 1 << 20,
              positions: bool = True):
        """Where a pattern sits on the current board: :class:`ops.MatchResult` ``(count, positions, orientation,
        truncated)``.  ``pattern_or_template``: what :meth:`stamp` accepts, turned into a template with ``margin`` dead
        cells around it (``ops.match_template``), or an ``ops.Template``.  ``orientations``: ``False`` (as given) or
        ``"all"`` (the distinct ones of the eight turns and mirror images).  ``positions`` is a ``(k, 2)`` int64 array of
        the board cells under the pattern's top-left cell, sorted by (row, col, orientation), ``orientation`` their ids.
        ``count`` is always exact; with ``count > max_hits``, ``truncated`` is True and the positions are some ``max_hits``
        of the matches.  ``positions=False`` returns the count alone (empty arrays).  One rank only.  On the HIP backend
        the board stays on the device: only the counter and the positions leave it."""
        ts = self._match_templates("match", pattern_or_template, margin, orientations)
        max_hits = int(max_hits)
        if max_hits < 1:
            raise ValueError(f"match: max_hits = {max_hits} is less than 1")
        from ..ops.match import MatchResult

        count, pos, ids, truncated = self.engine.match(ts, max_hits, bool(positions))
        return MatchResult(int(count), pos, ids, bool(truncated))

    def count_matches(self, pattern_or_template, *, margin: int = 1, orientations=False) -> int:
        """``match(...).count`` with nothing but the counter leaving the device."""
        return self.match(pattern_or_template, margin=margin, orientations=orientations, positions=False).count

    def match_tensor(self, pattern_or_template, *, margin: int = 1, orientations=False, dtype=None, out=None):
        """The matches as an ``(h, w)`` tensor on the simulation's side: 1 where some requested orientation matches, else
        0.  Arguments as :meth:`match`; dtype, ``out``, stream ordering and errors as :meth:`board_tensor`."""
        from ..ops import tensors

        self._two_states("match_tensor()")
        ts = self._match_templates("match_tensor", pattern_or_template, margin, orientations)
        t = tensors.result((self.geometry.h, self.geometry.w), dtype, self._tensor_device(), out, "match_tensor")
        tensors.sync(t)
        self.engine.match_cells(ts, *tensors.handle(t))
        return t

    # -- connected components (ops/components.py states the neighbourhoods, the box rule and the hash) ----------
    def components(self, neighbourhood: str = "moore", max_objects: int = 1 << 20, hashes: bool = True):
        """The objects of the current board (under a Generations rule: of its live cells): :class:`ops.Components`
        ``(count, anchor, population, bbox, hash, truncated)``, sorted by anchor.  ``neighbourhood``: ``"von_neumann"``,
        ``"moore"`` or ``"moore2"`` (Chebyshev distance <= 2, the pseudo-object notion).  ``count`` is always exact; with
        ``count > max_objects``, ``truncated`` is True and the arrays hold some ``max_objects`` of the objects, each
        complete.  ``window(*bbox[i])`` is object ``i``; ``hash`` is the same for all eight orientations of an object, so
        ``np.unique(objs.hash, return_counts=True)`` is a census.  ``hashes=False`` leaves ``hash`` empty.  One rank only.
        On the HIP backend the board stays on the device: only the counter and the records leave it."""
        from ..ops.components import Components

        self._one_rank("components")  # (the native side refuses the neighbourhood, max_objects and 2^31 cells)
        count, _, anchor, pop, bbox, h, truncated, _ = self.engine.components(neighbourhood, int(max_objects), bool(hashes), True)
        return Components(int(count), anchor, pop, bbox, h, bool(truncated))

    def count_components(self, neighbourhood: str = "moore") -> int:
        """``components(...).count`` with nothing but the counter leaving the device."""
        self._one_rank("count_components")
        return int(self.engine.components(neighbourhood, 1, False, False)[0])

    def components_tensor(self, neighbourhood: str = "moore", dtype=None, out=None):
        """The labels as an ``(h, w)`` tensor on the simulation's side: ``1 + row * W + col`` of the anchor of the cell's
        object, 0 for a dead cell.  ``dtype``: ``torch.int32`` (the default) or ``torch.int64``; ``out``, stream ordering
        and errors as :meth:`match_tensor`."""
        import torch

        from ..ops import tensors
        from ..ops.components import check_neighbourhood

        what = "components_tensor"
        self._two_states("components_tensor()")
        check_neighbourhood(neighbourhood, what)  # (before a tensor is made; the native side checks the rest)
        self._one_rank(what)
        shape, device = (self.geometry.h, self.geometry.w), self._tensor_device()
        if out is None:
            dtype = torch.int32 if dtype is None else dtype
            if dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{what}: dtype {dtype} is not one of torch.int32, int64")
            t = torch.empty(shape, dtype=dtype, device=device)
        else:
            if not isinstance(out, torch.Tensor):
                raise ValueError(f"{what}: out must be a torch.Tensor, got {type(out).__name__}")
            if tuple(out.shape) != shape:
                raise ValueError(f"{what}: out has shape {tuple(out.shape)}, the result is {shape}")
            if out.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{what}: dtype {out.dtype} is not one of torch.int32, int64")
            if dtype is not None and out.dtype != dtype:
                raise ValueError(f"{what}: out has dtype {out.dtype}, the call asks for {dtype}")
            if not out.is_contiguous():
                raise ValueError(f"{what}: out is not contiguous (strides {tuple(out.stride())} for shape {tuple(out.shape)})")
            tensors.check_device(out, device, what)
            t = out
        tensors.sync(t)
        self.engine.components_labels(neighbourhood, t.data_ptr(), t.dtype == torch.int64, t.numel())
        return t

    def load_rle(self, path, at="center") -> "Simulation":
        """An empty board (generation 0) with the file's pattern on it.  Raises if the file names a rule
        other than the simulation's."""
        p = self._pattern(path)
        if p.rule and p.rule != self.config.rule:
            raise ValueError(f"the RLE pattern names rule {p.rule}, this simulation runs {self.config.rule}")
        if p.topology and self._topology_boundary(p.topology) != self.config.boundary:
            raise ValueError(
                f"the RLE pattern names topology {p.topology} (boundary {self._topology_boundary(p.topology)}), "
                f"this simulation runs boundary {self.config.boundary}"
            )
        self.init(0)
        return self.stamp(p, at=at, mode="or")

    @staticmethod
    def _topology_boundary(topology: str) -> str:
        """The boundary an RLE header's topology suffix stands for: P (plane) is dead edges, T the torus."""
        return "dead" if topology == "P" else "torus"

    def save_rle(self, path, window=None) -> None:
        """Write ``window = (r0, c0, rows, cols)`` (default: the whole board) as an RLE file with the
        simulation's rule.  The whole board of a bounded simulation also names its plane in the header
        (``rule = B3/S23:P<W>,<H>``).  Collective; rank 0 writes."""
        from ..ops.rle import pattern_from_cells

        self._two_states("save_rle()")  # (multi-state RLE is not written)
        H, W = self.decomposition.H, self.decomposition.W
        r0, c0, rows, cols = window if window is not None else (0, 0, H, W)
        cells = self.window(r0, c0, rows, cols)
        if self.geometry.rank == 0:
            if window is None and self.config.boundary == "dead":
                p = pattern_from_cells(cells, self.config.rule, "P", W, H)
            else:
                p = pattern_from_cells(cells, self.config.rule)
            _gol.write_rle_file(os.fspath(path), p)

    @classmethod
    def from_rle(cls, path, N: Optional[int] = None, *, at="center", **kw) -> "Simulation":
        """A simulation of side ``N`` under the file's rule (the default rule when it names none) with the
        file's pattern on an otherwise empty board.  A topology suffix in the file's rule field
        (``:P<w>,<h>`` plane = dead edges, ``:T<w>,<h>`` torus) sets the boundary unless the call does, and
        without ``N`` the board is the suffix's ``h`` rows x ``w`` columns."""
        p = cls._pattern(path)
        if p.topology:
            file_b = cls._topology_boundary(p.topology)
            if kw.get("boundary") is not None:
                c = _gol.EngineConfig()
                c.boundary = kw["boundary"]
                if c.boundary != file_b:
                    raise ValueError(
                        f"RLE file {path!r} names topology {p.topology} (boundary {file_b}), the call asks for {c.boundary}"
                    )
            kw["boundary"] = file_b
        if N is None:
            if not p.topology:
                raise ValueError(f"from_rle without N needs a board size in the file: {path!r} has no topology suffix")
            N = p.bound_rows
            kw.setdefault("width", p.bound_cols)
        if p.rule:
            if "rule" in kw:
                c = _gol.EngineConfig()
                c.rule = kw["rule"]
                if c.rule != p.rule:
                    raise ValueError(f"RLE file {path!r} names rule {p.rule}, the call asks for {c.rule}")
            kw["rule"] = p.rule
        return cls(N, **kw).load_rle(p, at=at)

    # -- I/O -------------------------------------------------------------------------------
    def dump(self, path: Optional[str] = None) -> str:
        """Write this rank's reference-format dump file (collective); returns the path."""
        self._two_states("dump()")
        if path is None:
            path = _gol.dump_filename(self.geometry.rank, self.decomposition.P)
        _gol.write_dumps(self.engine, path)
        return path

    def checkpoint(self, prefix: str) -> None:
        """Write ``<prefix>.gol`` (collective): the global board, each rank writing its own rectangle.

        The file does not depend on the decomposition: :meth:`restore` works on any rank count or
        grid with the same global board size.
        """
        self._two_states("checkpoint()")
        self._no_ltl("checkpoint()")
        _gol.save_checkpoint(self.engine, prefix, self.pattern.seed if self.pattern else 0)

    def restore(self, prefix: str) -> int:
        """Load this rank's rectangle of ``<prefix>.gol``; returns the snapshot's generation."""
        self._two_states("restore()")
        self._no_ltl("restore()")
        return int(_gol.load_checkpoint(self.engine, prefix))
