"""Independent oracles for testing the native engine.

* :func:`numpy_step` — byte-per-cell torus step (numpy roll), the plain reference.
* :func:`torch_step` — the same with a 3x3 ``conv2d`` and circular padding in fp32; runs on the GPU
  (PyTorch-ROCm) to cross-check large boards independently of the HIP kernels.
* :func:`numpy_step_rule` / :func:`torch_step_rule` — the same two for any life-like rule ``B.../S...``,
  with a rule parser of their own (independent of the native one).
* :func:`numpy_step_rule_bounded` — a life-like rule on a bounded board (dead cells beyond the edges), from a
  zero-padded neighbour count, written without the torus oracle.
* :func:`numpy_soup_settle` — one soup of a soup batch: Brent's search with exact board comparison, and the exact
  transient, on :func:`numpy_step_rule`.
* :func:`quirk_model` — the reference's actual behaviour (survey Q1-Q3): every rank steps its tile
  with x-wrap and CONSTANT ghost rows taken from the generation-0 boards, with the P <= 2 swap.
* :func:`initial_board` — pattern placement mirror (patterns 0-5) computed in Python, including the
  splitmix64-based random pattern, to check the native init bit-for-bit.
"""
from __future__ import annotations

import numpy as np

MASK64 = (1 << 64) - 1


def numpy_step(board: np.ndarray, generations: int = 1) -> np.ndarray:
    b = np.asarray(board, dtype=np.uint8)
    for _ in range(generations):
        n = sum(
            np.roll(np.roll(b, dy, axis=0), dx, axis=1)
            for dy in (-1, 0, 1)
            for dx in (-1, 0, 1)
            if dy or dx
        )
        b = ((n == 3) | ((b == 1) & (n == 2))).astype(np.uint8)
    return b


def torch_step(board, generations: int = 1, device=None):
    """B3/S23 on a torus with torch conv2d (fp32, exact for counts <= 8).  Returns a torch uint8 tensor."""
    import torch
    import torch.nn.functional as F

    if isinstance(board, torch.Tensor):  # e.g. a previous torch_step result, already on the device
        x = board.to(device=device if device is not None else board.device, dtype=torch.float32)[None, None]
    else:
        x = torch.as_tensor(np.asarray(board), dtype=torch.float32, device=device)[None, None]
    k = torch.ones(1, 1, 3, 3, dtype=torch.float32, device=x.device)
    k[0, 0, 1, 1] = 0
    for _ in range(generations):
        n = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), k)
        x = ((n == 3) | ((x == 1) & (n == 2))).to(torch.float32)
    return x[0, 0].to(torch.uint8)


_RULE_ALIASES = {
    "conway": "b3/s23",
    "life": "b3/s23",
    "highlife": "b36/s23",
    "daynight": "b3678/s34678",
    "seeds": "b2/s",
    "replicator": "b1357/s1357",
}


# The neighbours a rule counts, by its suffix, as 3 x 3 masks around the centre (rows downward, columns rightward):
# Moore (no suffix), von Neumann (V), hexagonal (H: the square-grid emulation without the NE and SW corners).
NEIGHBOURHOODS = {
    "": ((1, 1, 1), (1, 0, 1), (1, 1, 1)),
    "V": ((0, 1, 0), (1, 0, 1), (0, 1, 0)),
    "H": ((1, 1, 0), (1, 0, 1), (0, 1, 1)),
}


def parse_rule_nbhd(rule) -> tuple:
    """A rule as ``(birth, survive, nbhd)``: the masks of :func:`parse_rule` and the neighbourhood's suffix, ``""``
    (Moore), ``"V"`` (von Neumann) or ``"H"`` (hexagonal), a key of :data:`NEIGHBOURHOODS`.  Takes what
    :func:`parse_rule` takes, a rule string with the suffix directly after the second list (``"B2/S34H"``, either
    case), or a ``(birth, survive, nbhd)`` triple.  Digits beyond the neighbourhood's largest count (8, V: 4, H: 6)
    are refused, and B0 rules, as in the engine."""
    nbhd = ""
    if not isinstance(rule, str):
        vals = tuple(rule)
        if len(vals) == 3:
            nbhd = str(vals[2]).upper()
            if nbhd not in NEIGHBOURHOODS:
                raise ValueError(f"invalid rule {rule!r}: the neighbourhood is '', 'V' or 'H'")
            vals = vals[:2]
        birth, survive = (int(v) for v in vals)
        top = sum(sum(row) for row in NEIGHBOURHOODS[nbhd])
        if not (0 <= birth < (2 << top) and 0 <= survive < (2 << top)):
            raise ValueError(f"invalid rule {rule!r}: masks have bits 0..{top}")
    else:
        text = _RULE_ALIASES.get(rule.lower(), rule.lower())
        if text[-1:] in ("v", "h"):  # directly after the second list
            nbhd, text = text[-1].upper(), text[:-1]
        parts = text.split("/")
        if len(parts) != 2 or {p[:1] for p in parts} != {"b", "s"}:
            raise ValueError(f"invalid rule {rule!r}: expected B<digits>/S<digits>")
        top = sum(sum(row) for row in NEIGHBOURHOODS[nbhd])
        masks = {}
        for p in parts:
            digits = p[1:]
            if not all(c in "012345678"[: top + 1] for c in digits) or len(set(digits)) != len(digits):
                raise ValueError(f"invalid rule {rule!r}: digits are 0..{top}, each at most once")
            masks[p[0]] = sum(1 << int(c) for c in digits)
        birth, survive = masks["b"], masks["s"]
    if birth & 1:
        raise ValueError(f"invalid rule {rule!r}: B0 rules are out of scope (the dead background would come alive)")
    return birth, survive, nbhd


def parse_rule(rule) -> tuple:
    """A rule as ``(birth, survive)`` masks: bit c of birth / survive = a dead / live cell with c live
    neighbours is alive next generation.  Takes ``"B36/S23"`` (either order, either case, empty digit
    lists allowed), an alias (conway, life, highlife, daynight, seeds, replicator) or a mask pair.
    B0 rules are refused, as in the engine.  A neighbourhood suffix (``"B2/S34H"``) is accepted and not returned:
    :func:`parse_rule_nbhd` returns it."""
    return parse_rule_nbhd(rule)[:2]


def rule_string(rule) -> str:
    """Canonical ``B<digits>/S<digits>`` (digits ascending), then the neighbourhood's ``V`` or ``H``."""
    birth, survive, nbhd = parse_rule_nbhd(rule)
    digits = lambda m: "".join(str(c) for c in range(9) if (m >> c) & 1)  # noqa: E731
    return f"B{digits(birth)}/S{digits(survive)}{nbhd}"


def numpy_step_rule(board: np.ndarray, rule, generations: int = 1) -> np.ndarray:
    """Byte-per-cell torus step of a life-like rule (string, ``(birth, survive)`` pair or ``(birth, survive, nbhd)``
    triple): shifted adds over the rule's neighbourhood mask (:data:`NEIGHBOURHOODS`)."""
    birth, survive, nbhd = parse_rule_nbhd(rule)
    mask = NEIGHBOURHOODS[nbhd]
    lut = np.array([[(birth >> c) & 1 for c in range(9)], [(survive >> c) & 1 for c in range(9)]], dtype=np.uint8)
    b = np.asarray(board, dtype=np.uint8)
    for _ in range(generations):
        # the neighbour at (row + dy, column + dx) comes to the cell by a roll of (-dy, -dx)
        n = sum(
            np.roll(np.roll(b, -dy, axis=0), -dx, axis=1)
            for dy in (-1, 0, 1)
            for dx in (-1, 0, 1)
            if mask[dy + 1][dx + 1]
        )
        b = lut[b, n]
    return b


def numpy_step_rule_bounded(board: np.ndarray, rule, generations: int = 1) -> np.ndarray:
    """Byte-per-cell step of a life-like rule on a bounded board: every cell outside the array is dead in every
    generation.  Written on its own, from a neighbour count over a zero-padded copy (no roll, no torus oracle)."""
    birth, survive, nbhd = parse_rule_nbhd(rule)
    mask = NEIGHBOURHOODS[nbhd]
    b = np.asarray(board, dtype=np.uint8)
    if b.ndim != 2:
        raise ValueError(f"a board is a 2-D array, got shape {b.shape}")
    H, W = b.shape
    for _ in range(generations):
        pad = np.zeros((H + 2, W + 2), dtype=np.int32)
        pad[1:-1, 1:-1] = b
        n = np.zeros((H, W), dtype=np.int32)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if mask[dy][dx]:  # (pad is shifted by one: mask[dy][dx] is the neighbour at (row + dy - 1, column + dx - 1))
                    n += pad[dy : dy + H, dx : dx + W]
        alive = b == 1
        b = np.where(alive, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)
    return b


def parse_generations_rule(rule) -> tuple:
    """A rule string as ``(birth, survive, states)``: a Generations rule ``B<digits>/S<digits>/C<n>``, ``S.../B.../C<n>``
    (either case) or the bare ``<survive digits>/<birth digits>/<n>`` with ``n`` from 2 to 9 and no leading zero, or a
    two-state Moore rule as :func:`parse_rule` takes it (``states`` 2).  ``C2`` is the two-state rule.  A parser of its
    own, independent of the native one.  A ``V`` or ``H`` suffix together with ``/C`` is refused, and B0, as in the engine."""
    if not isinstance(rule, str):
        birth, survive, states = (int(v) for v in rule)
        if not (0 <= birth < 512 and 0 <= survive < 512 and 2 <= states <= 9) or birth & 1:
            raise ValueError(f"invalid rule {rule!r}: masks have bits 0..8 (B0 is out of scope), states run from 2 to 9")
        return birth, survive, states
    text = _RULE_ALIASES.get(rule.lower(), rule.lower())
    parts = text.split("/")
    if len(parts) == 3:
        if all(p.isdigit() or p == "" for p in parts) and parts[2] != "":  # bare: survive / birth / states
            parts = ["b" + parts[1], "s" + parts[0], "c" + parts[2]]
        count = parts[2]
        if count[:1] != "c" or not count[1:].isdigit() or (len(count) > 2 and count[1] == "0") or not 2 <= int(count[1:]) <= 9:
            raise ValueError(f"invalid rule {rule!r}: the third field is C<n>, n from 2 to 9 without leading zeros")
        if parts[1][-1:] in ("v", "h"):
            raise ValueError(f"invalid rule {rule!r}: a V or H suffix together with /C")
        birth, survive, nbhd = parse_rule_nbhd("/".join(parts[:2]))
        return birth, survive, int(count[1:])
    birth, survive, nbhd = parse_rule_nbhd(rule)
    if nbhd:
        raise ValueError(f"invalid rule {rule!r}: Generations rules count the Moore neighbourhood")
    return birth, survive, 2


def parse_rule_states(rule) -> int:
    """The states of a rule string: 2 for a life-like rule (any neighbourhood), C for a Generations rule
    ``B<digits>/S<digits>/C<n>``."""
    if is_ltl_rule(rule):
        parse_ltl_rule(rule)
        return 2
    if isinstance(rule, str) and rule.count("/") < 2:
        parse_rule_nbhd(rule)
        return 2
    return parse_generations_rule(rule)[2]


_B0_TEXT = "B0 rules are out of scope (the dead background would come alive)"
LTL_MAX_RANGE = 7  # counts of up to (2 * 7 + 1) ** 2 = 225 fit 8 bit planes


def is_ltl_rule(rule) -> bool:
    """Whether a rule string names the Larger than Life family: the alias ``bosco``, or a string that begins with the
    ``R`` field (``replicator`` is a life-like alias).  Says nothing about validity."""
    if not isinstance(rule, str):
        return False
    low = rule.lower()
    return low == "bosco" or (len(low) >= 2 and low[0] == "r" and low != "replicator")


def _ltl_number(rule, text: str, what: str) -> int:
    if not text or not text.isascii() or not text.isdigit():
        raise ValueError(f"invalid rule {rule!r}: {text!r} in {what} is not a number")
    if len(text) > 1 and text[0] == "0":
        raise ValueError(f"invalid rule {rule!r}: {text!r} in {what} has a leading zero")
    if len(text) > 4:
        raise ValueError(f"invalid rule {rule!r}: {text!r} in {what} is out of range")
    return int(text)


def parse_ltl_rule(rule) -> tuple:
    """A Larger than Life rule as ``(R, M, smin, smax, bmin, bmax)``: Golly's
    ``R<r>,C<c>,M<m>,S<smin>..<smax>,B<bmin>..<bmax>[,N<n>]`` (letters in either case, the fields in this order) or the
    alias ``bosco`` (``R5,C0,M1,S34..58,B34..45,NM``), or such a 6-tuple.  ``r`` runs from 1 to 7, ``c`` is 0 or 2 (two
    states; history states are not built), ``m`` 0 or 1, ``n`` is ``M`` (the box; ``NN`` and ``NC`` are not built) or
    missing; intervals need ``min <= max <= (2r+1)**2`` and ``bmin >= 1`` (B0).  Refused as well: a field twice or
    missing, spaces, leading zeros, a trailing comma.  A parser of its own, independent of the native one."""
    if not isinstance(rule, str):
        r, m, smin, smax, bmin, bmax = (int(v) for v in rule)
        c = 0
    else:
        text = rule.lower()
        if text == "bosco":
            text = "r5,c0,m1,s34..58,b34..45,nm"
        if not is_ltl_rule(text):
            raise ValueError(f"invalid rule {rule!r}: not a Larger than Life rule (R<r>,C<c>,M<m>,S<a>..<b>,B<a>..<b>[,NM])")
        if any(ch.isspace() for ch in text):
            raise ValueError(f"invalid rule {rule!r}: spaces in a Larger than Life rule")
        if text.endswith(","):
            raise ValueError(f"invalid rule {rule!r}: a trailing comma")
        seen = {}
        for field in text.split(","):
            letter, rest = field[:1], field[1:]
            if letter == "" or letter not in "rcmsbn":
                raise ValueError(f"invalid rule {rule!r}: unknown field {field!r} (the fields are R, C, M, S, B and N)")
            if letter in seen:
                raise ValueError(f"invalid rule {rule!r}: field {letter.upper()} twice")
            if letter == "n":
                if rest in ("n", "c"):
                    name = "NN, the von Neumann" if rest == "n" else "NC, the circular"
                    raise ValueError(f"invalid rule {rule!r}: {name} neighbourhood of range R, is not built; NM (the box) only")
                if rest != "m":
                    raise ValueError(f"invalid rule {rule!r}: neighbourhood {field!r}: NM (the box) only")
                seen[letter] = "m"
            elif letter in "sb":
                lo, dots, hi = rest.partition("..")
                if not dots:
                    raise ValueError(f"invalid rule {rule!r}: field {field!r} is not {letter.upper()}<min>..<max>")
                what = f"{letter.upper()}<min>..<max>"
                seen[letter] = (_ltl_number(rule, lo, what), _ltl_number(rule, hi, what))
            else:
                seen[letter] = _ltl_number(rule, rest, f"{letter.upper()}<n>")
        for letter in "rcmsb":
            if letter not in seen:
                raise ValueError(f"invalid rule {rule!r}: field {letter.upper()} is missing")
        if "".join(seen) not in ("rcmsb", "rcmsbn"):
            raise ValueError(f"invalid rule {rule!r}: the fields come in the order R,C,M,S,B[,N]")
        r, c, m = seen["r"], seen["c"], seen["m"]
        (smin, smax), (bmin, bmax) = seen["s"], seen["b"]
    if not 1 <= r <= LTL_MAX_RANGE:
        raise ValueError(f"invalid rule {rule!r}: range R{r}: Larger than Life rules run with R1 to R{LTL_MAX_RANGE}")
    if c >= 3:
        raise ValueError(f"invalid rule {rule!r}: C{c}: Larger than Life rules with history states (C >= 3) are not built")
    if c == 1:
        raise ValueError(f"invalid rule {rule!r}: C1: the state count is C0 or C2 (two states)")
    if m not in (0, 1):
        raise ValueError(f"invalid rule {rule!r}: M{m}: the middle flag is M0 or M1")
    box = (2 * r + 1) ** 2
    for name, lo, hi in (("S", smin, smax), ("B", bmin, bmax)):
        if not 0 <= lo <= hi <= box:
            raise ValueError(f"invalid rule {rule!r}: {name}{lo}..{hi}: an interval needs min <= max <= (2*{r}+1)^2 = {box}")
    if bmin == 0:
        raise ValueError(f"invalid rule {rule!r}: {_B0_TEXT}")
    return r, m, smin, smax, bmin, bmax


def ltl_rule_string(rule) -> str:
    """Canonical ``R<r>,C0,M<m>,S<smin>..<smax>,B<bmin>..<bmax>,NM``: always all six fields, with ``C0``."""
    r, m, smin, smax, bmin, bmax = parse_ltl_rule(rule)
    return f"R{r},C0,M{m},S{smin}..{smax},B{bmin}..{bmax},NM"


def numpy_ltl(board: np.ndarray, rule, gens: int, boundary: str = "torus") -> np.ndarray:
    """The oracle of the Larger than Life rules: ``gens`` generations of the 0/1 array ``board`` under ``rule`` (a string
    or ``(R, M, smin, smax, bmin, bmax)``), Golly's semantics.  ``n`` is the number of live cells in the
    ``(2R+1) x (2R+1)`` box around a cell, the cell itself counted iff M is 1; a dead cell is born iff
    ``bmin <= n <= bmax``, a live cell survives iff ``smin <= n <= smax``.  Plain numpy: summed rolls on the torus
    (``boundary="torus"``), a zero pad on a bounded board (``"dead"``)."""
    R, M, smin, smax, bmin, bmax = parse_ltl_rule(rule)
    if boundary not in ("torus", "dead"):
        raise ValueError(f"boundary must be torus or dead, got {boundary!r}")
    b = np.asarray(board, dtype=np.uint8)
    if b.ndim != 2:
        raise ValueError(f"a board is a 2-D array, got shape {b.shape}")
    H, W = b.shape
    if H < 2 * R + 1 or W < 2 * R + 1:
        raise ValueError(f"a {H} x {W} board is smaller than the {2 * R + 1} x {2 * R + 1} box of range {R}")
    for _ in range(int(gens)):
        live = b.astype(np.int32)
        if boundary == "torus":
            cols = sum(np.roll(live, dx, axis=1) for dx in range(-R, R + 1))
            n = sum(np.roll(cols, dy, axis=0) for dy in range(-R, R + 1))
        else:
            pad = np.zeros((H + 2 * R, W + 2 * R), dtype=np.int32)
            pad[R : R + H, R : R + W] = live
            cols = sum(pad[:, dx : dx + W] for dx in range(2 * R + 1))
            n = sum(cols[dy : dy + H, :] for dy in range(2 * R + 1))
        if not M:
            n = n - live
        alive = b == 1
        b = np.where(alive, (n >= smin) & (n <= smax), (n >= bmin) & (n <= bmax)).astype(np.uint8)
    return b


def numpy_generations(board: np.ndarray, rule, gens: int, boundary: str = "torus") -> np.ndarray:
    """The oracle of the Generations rules: ``gens`` generations of the state array ``board`` (uint8, states 0 .. C-1)
    under ``rule`` (a string, or ``(birth, survive, states)``) and returns the state array.  State 0 is dead, 1 alive,
    2 .. C-1 dying.  Only state 1 counts as a neighbour (Moore; ``boundary`` ``"torus"``: ``np.roll``, ``"dead"``: zero
    padding).  ``0 -> 1`` iff the count is in B; ``1 -> 1`` iff it is in S, else ``1 -> 2``; ``s -> s + 1`` for
    ``2 <= s < C-1`` and ``C-1 -> 0`` whatever the count.  With two states this is the life-like rule."""
    birth, survive, states = parse_generations_rule(rule)
    if boundary not in ("torus", "dead"):
        raise ValueError(f"boundary must be torus or dead, got {boundary!r}")
    b = np.asarray(board, dtype=np.uint8)
    if b.ndim != 2:
        raise ValueError(f"a board is a 2-D array, got shape {b.shape}")
    if b.size and int(b.max()) >= states:
        raise ValueError(f"state {int(b.max())} on the board: the rule has the states 0 .. {states - 1}")
    H, W = b.shape
    for _ in range(int(gens)):
        live = (b == 1).astype(np.int32)
        if boundary == "torus":
            n = sum(np.roll(np.roll(live, dy, axis=0), dx, axis=1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
        else:
            pad = np.zeros((H + 2, W + 2), dtype=np.int32)
            pad[1:-1, 1:-1] = live
            n = sum(pad[dy : dy + H, dx : dx + W] for dy in (0, 1, 2) for dx in (0, 1, 2) if (dy, dx) != (1, 1))
        born = (b == 0) & (((birth >> n) & 1) == 1)
        stays = (b == 1) & (((survive >> n) & 1) == 1)
        nxt = np.zeros_like(b)
        nxt[born | stays] = 1
        if states > 2:
            nxt[(b == 1) & ~stays] = 2
            dying = (b >= 2) & (b < states - 1)
            nxt[dying] = b[dying] + 1  # (C-1 -> 0: left at zero)
        b = nxt
    return b


def numpy_census(board: np.ndarray, rule, gens: int, bounded: bool = False, return_board: bool = False):
    """The populations after generations ``1 .. gens`` of ``board`` under ``rule`` as a uint64 array (the oracle of
    the engines' census mode), on the torus or, ``bounded``, on a board with dead edges.  One generation of
    :func:`numpy_step_rule` / :func:`numpy_step_rule_bounded` at a time; ``return_board`` also returns the last
    board."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    b = np.asarray(board, dtype=np.uint8)
    counts = np.zeros(int(gens), dtype=np.uint64)
    for g in range(int(gens)):
        b = step(b, rule, 1)
        counts[g] = int(b.sum(dtype=np.uint64))
    return (counts, b) if return_board else counts


def _sig_mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def numpy_signature(board: np.ndarray) -> int:
    """The board signature of a 2-D 0/1 array (the oracle of ``signature()`` and of signature mode), from cells, not
    from packed words: a live cell at row ``r``, column ``x`` adds ``2**((x % 64) // 2) * (rho(r) * gam(2 * (x // 64) +
    x % 2) mod 2**32)``, the sum taken mod ``2**64``, with ``rho(r) = mix32(r ^ 0x9E3779B9) | 1`` and ``gam(j) =
    mix32(j + 0x7F4A7C15) | 1``."""
    b = np.asarray(board)
    if b.ndim != 2:
        raise ValueError("numpy_signature takes a 2-D board")
    m = np.uint64(0xFFFFFFFF)
    rows = np.arange(b.shape[0], dtype=np.uint64)
    cols = np.arange(b.shape[1], dtype=np.uint64)
    rho = _sig_mix32((rows & m) ^ np.uint64(0x9E3779B9)) | np.uint64(1)
    gam = _sig_mix32((np.uint64(2) * (cols // np.uint64(64)) + (cols & np.uint64(1)) + np.uint64(0x7F4A7C15)) & m) | np.uint64(1)
    shift = (cols % np.uint64(64)) // np.uint64(2)
    r, c = np.nonzero(b)
    key = (rho[r] * gam[c]) & m  # (< 2**64: both factors are below 2**32)
    with np.errstate(over="ignore"):
        terms = key << shift[c]  # (key < 2**32, shift <= 31: no bit is lost)
        return int(terms.sum(dtype=np.uint64))  # wraps mod 2**64


def numpy_signatures(board: np.ndarray, rule, gens: int, bounded: bool = False, return_board: bool = False):
    """The signatures after generations ``1 .. gens`` of ``board`` under ``rule`` as a uint64 array (the oracle of the
    engines' signature mode), on the torus or, ``bounded``, on a board with dead edges.  ``return_board`` also returns
    the last board."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    b = np.asarray(board, dtype=np.uint8)
    sigs = np.zeros(int(gens), dtype=np.uint64)
    for g in range(int(gens)):
        b = step(b, rule, 1)
        sigs[g] = numpy_signature(b)
    return (sigs, b) if return_board else sigs


def numpy_film(board: np.ndarray, rule, gens: int, rect, bounded: bool = False, return_board: bool = False):
    """The window ``rect = (r0, c0, rows, cols)`` of ``board`` after generations ``1 .. gens`` under ``rule`` as a
    ``(gens, rows, cols)`` uint8 array (the oracle of the engines' film mode), on the torus or, ``bounded``, on a board
    with dead edges.  One generation of :func:`numpy_step_rule` / :func:`numpy_step_rule_bounded` at a time; each frame
    is taken with ``np.take(..., mode="wrap")`` on both axes, so the window's coordinates wrap as ``window()``'s do.
    ``return_board`` also returns the last board."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    r0, c0, rows, cols = (int(v) for v in rect)
    b = np.asarray(board, dtype=np.uint8)
    frames = np.zeros((int(gens), rows, cols), dtype=np.uint8)
    ri, ci = np.arange(r0, r0 + rows), np.arange(c0, c0 + cols)
    for g in range(int(gens)):
        b = step(b, rule, 1)
        frames[g] = np.take(np.take(b, ri, axis=0, mode="wrap"), ci, axis=1, mode="wrap")
    return (frames, b) if return_board else frames


def numpy_density_film(board: np.ndarray, rule, gens: int, blocks, bounded: bool = False, return_board: bool = False):
    """The density maps of ``board`` after generations ``1 .. gens`` under ``rule`` as a ``(gens, grid_rows, grid_cols)``
    uint32 array (the oracle of the engines' density-film mode), on the torus or, ``bounded``, on a board with dead
    edges.  ``blocks`` is ``(block_rows, block_cols)`` or one int; a map holds the live cells of every block of that
    shape, ``ceil(H / block_rows) x ceil(W / block_cols)`` of them, the last of a row or column partial.  One
    generation of :func:`numpy_step_rule` / :func:`numpy_step_rule_bounded` at a time; the block sums are taken here,
    with ``np.add.reduceat`` along both axes.  ``return_board`` also returns the last board."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    if isinstance(blocks, (int, np.integer)):
        blocks = (blocks, blocks)
    br, bc = (int(v) for v in blocks)
    b = np.asarray(board, dtype=np.uint8)
    H, W = b.shape
    ri, ci = np.arange(0, H, br), np.arange(0, W, bc)
    maps = np.zeros((int(gens), len(ri), len(ci)), dtype=np.uint32)
    for g in range(int(gens)):
        b = step(b, rule, 1)
        maps[g] = np.add.reduceat(np.add.reduceat(b.astype(np.uint32), ri, axis=0), ci, axis=1)
    return (maps, b) if return_board else maps


def numpy_soup_settle(board: np.ndarray, rule, max_gens: int, transient: bool = False):
    """One soup of a soup batch (``SoupBatch.settle``), byte per cell on :func:`numpy_step_rule`: Brent's search with exact
    board comparison.  The soup keeps a copy of its board saved at generation ``s`` and a window ``w``, at first ``s = 0``
    and ``w = 1``.  After each step to generation ``g``: a board equal to the copy means settled, ``period = g - s``,
    ``generation = g``, and the soup stops; otherwise ``g - s == w`` saves the board, ``s = g``, ``w *= 2`` (the saves fall at
    generations 0, 1, 3, 7, ...).  A soup that reaches ``max_gens`` without a hit has ``period = 0`` and ``generation =
    max_gens``.  ``population`` is the live cells of the board at ``generation``.  ``transient`` (for a settled soup): two
    copies restart from the initial board, one is advanced ``period`` generations, and both are stepped until they are
    equal; the number of steps is the transient (-1 without the option or for an unsettled soup).
    Returns ``(period, transient, generation, population, final_board)``."""
    init = np.asarray(board, dtype=np.uint8)
    b, saved = init, init
    g, s, w, period = 0, 0, 1, 0
    while g < int(max_gens):
        b = numpy_step_rule(b, rule, 1)
        g += 1
        if np.array_equal(b, saved):
            period = g - s
            break
        if g - s == w:
            saved, s, w = b, g, 2 * w
    tr = -1
    if transient and period:
        x, y = init, numpy_step_rule(init, rule, period)
        tr = 0
        while not np.array_equal(x, y):
            x, y = numpy_step_rule(x, rule, 1), numpy_step_rule(y, rule, 1)
            tr += 1
    return period, tr, g, int(b.sum(dtype=np.uint64)), b


def numpy_envelope(board: np.ndarray, rule, gens: int, bounded: bool = False, return_board: bool = False):
    """The envelope of ``board`` over generations ``0 .. gens`` under ``rule`` as a uint8 array of the board's shape (the
    oracle of the engines' envelope mode): a 1 for every cell alive in the board itself or after any of the ``gens``
    generations, on the torus or, ``bounded``, on a board with dead edges.  One generation of :func:`numpy_step_rule` /
    :func:`numpy_step_rule_bounded` at a time, ORed here.  ``return_board`` also returns the last board."""
    step = numpy_step_rule_bounded if bounded else numpy_step_rule
    b = np.asarray(board, dtype=np.uint8)
    env = (b != 0).astype(np.uint8)
    for _ in range(int(gens)):
        b = step(b, rule, 1)
        env |= b
    return (env, b) if return_board else env


def torch_step_rule(board, rule, generations: int = 1, device=None):
    """A life-like rule on a torus with torch conv2d (fp32, exact for counts <= 8).  Returns a torch uint8 tensor."""
    import torch
    import torch.nn.functional as F

    birth, survive, nbhd = parse_rule_nbhd(rule)
    if isinstance(board, torch.Tensor):
        x = board.to(device=device if device is not None else board.device, dtype=torch.float32)[None, None]
    else:
        x = torch.as_tensor(np.asarray(board), dtype=torch.float32, device=device)[None, None]
    # (conv2d is a cross-correlation: the kernel is the neighbourhood mask as it stands)
    k = torch.tensor(NEIGHBOURHOODS[nbhd], dtype=torch.float32, device=x.device)[None, None]
    lut = torch.tensor(
        [(birth >> c) & 1 for c in range(9)] + [(survive >> c) & 1 for c in range(9)], dtype=torch.float32, device=x.device
    )
    for _ in range(generations):
        n = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), k)
        x = lut[(x * 9 + n).to(torch.int64)]
    return x[0, 0].to(torch.uint8)


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def random_word(seed: int, grow: int, gword: int, gwords: int) -> int:
    return _mix64(((seed * 0xD1B54A32D192ED03) & MASK64) ^ _mix64((grow * gwords + gword) & MASK64))


def _mix64_np(z: np.ndarray) -> np.ndarray:
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def random_board(H: int, W: int, seed: int) -> np.ndarray:
    """Pattern 5 on an H x W global board, vectorised (identical to the native counter hash)."""
    gw = (W + 63) // 64
    with np.errstate(over="ignore"):
        r = np.arange(H, dtype=np.uint64)[:, None]
        c = np.arange(gw, dtype=np.uint64)[None, :]
        idx = r * np.uint64(gw) + c
        sm = np.uint64((seed * 0xD1B54A32D192ED03) & MASK64)
        words = _mix64_np(sm ^ _mix64_np(idx))
    from .bitpack import unpack_words

    return unpack_words(words, W)


def strips(H: int, N: int, P: int, per_rank: bool):
    if per_rank:
        return [(s * N, (s + 1) * N) for s in range(P)]
    base, extra = divmod(H, P)
    out, pos = [], 0
    for s in range(P):
        n = base + (1 if s < extra else 0)
        out.append((pos, pos + n))
        pos += n
    return out


def initial_board(pattern: int, N: int, P: int = 1, per_rank: bool = True, seed: int = 0x5EED) -> np.ndarray:
    """Global initial board for the reference patterns (gol-with-cuda.cu:55-171) + pattern 5."""
    H = N * P if per_rank else N
    W = N
    b = np.zeros((H, W), dtype=np.uint8)
    st = strips(H, N, P, per_rank)

    def flat(s, f):
        r0, r1 = st[s]
        hs = r1 - r0
        if 0 <= f < hs * W:
            b[r0 + f // W, f % W] = 1

    if pattern == 0:
        pass
    elif pattern == 1:
        b[:] = 1
    elif pattern == 2:
        for s, (r0, r1) in enumerate(st):
            hs = r1 - r0
            off = (hs - 1) * W
            for j in range(127, 137):
                if off + j < hs * W:
                    flat(s, off + j)
    elif pattern == 3:
        flat(0, 0)
        flat(0, W - 1)
        if P > 1:
            hs = st[-1][1] - st[-1][0]
            flat(P - 1, (hs - 1) * W)
            flat(P - 1, (hs - 1) * W + W - 1)
    elif pattern == 4:
        flat(0, 0)
        flat(0, 1)
        flat(0, W - 1)
    elif pattern == 5:
        b = random_board(H, W, seed)
    else:
        raise ValueError(f"Pattern {pattern} has not been implemented")
    return b


def _step_with_ghosts(tile: np.ndarray, above: np.ndarray, below: np.ndarray) -> np.ndarray:
    ext = np.vstack([above[None, :], tile, below[None, :]]).astype(np.uint8)
    n = sum(
        np.roll(ext, dx, axis=1)[1 + dy : 1 + dy + tile.shape[0]]
        for dy in (-1, 0, 1)
        for dx in (-1, 0, 1)
        if dy or dx
    )
    return ((n == 3) | ((tile == 1) & (n == 2))).astype(np.uint8)


def quirk_model(init: np.ndarray, P: int, generations: int) -> np.ndarray:
    """Reference behaviour (GOL_COMPAT=reference): frozen gen-0 halos, swapped for P <= 2."""
    H, W = init.shape
    N = H // P
    tiles = [init[r * N : (r + 1) * N].copy() for r in range(P)]
    above, below = [], []
    for r in range(P):
        prev, nxt = tiles[(r - 1) % P], tiles[(r + 1) % P]
        if P >= 3:
            above.append(prev[-1].copy())
            below.append(nxt[0].copy())
        else:
            above.append(prev[0].copy())
            below.append(nxt[-1].copy())
    for _ in range(generations):
        tiles = [_step_with_ghosts(tiles[r], above[r], below[r]) for r in range(P)]
    return np.vstack(tiles)
