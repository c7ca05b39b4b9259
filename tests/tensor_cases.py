"""Shared by test_tensors.py (CPU backend) and test_gpu_tensors.py (MI355X): the cases of the tensor readers and writers,
their numpy references (computed once per board, rule, boundary and generation count, left read-only) and the checks.

Every comparison is exact.  A result is first checked bit for bit to hold nothing but the dtype's 0 and 1 (``exact01``:
0x3C00 for float16, 0x3F80 for bfloat16, 0x3F800000 for float32), then compared with the numpy twin as uint8."""
import functools

import numpy as np
import torch

from gol_amd.ops import numpy_envelope, numpy_film, numpy_step_rule, numpy_step_rule_bounded, random_board

DTYPES = ["bool", "uint8", "float16", "bfloat16", "float32"]
FLOATS = ["float16", "bfloat16", "float32"]
SIZED = ["uint8", "float16", "float32"]  # one dtype per element size: 1, 2 and 4 bytes
SIDES = [1, 2, 3, 63, 64, 65, 127, 137, 200]
BOARDS = [(n, n) for n in SIDES] + [(137, 200)]
# the device's extra shapes: a 7-cell row (no full 16-byte line in a row), 63 words with a one-cell tail word
GPU_BOARDS = BOARDS + [(130, 7), (50, 3969)]
HIGHLIFE = "B36/S23"
GENS = 3  # odd: the current buffer is the second one
SEED = 21

_ONE = {"bool": 1, "uint8": 1, "float16": 0x3C00, "bfloat16": 0x3F80, "float32": 0x3F800000}
_BITS = {"bool": torch.uint8, "uint8": torch.uint8, "float16": torch.int16, "bfloat16": torch.int16, "float32": torch.int32}


def dt(name):
    return getattr(torch, name)


def bid(shape):
    return f"{shape[0]}x{shape[1]}"


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def board_after(H, W, seed, rule, boundary, gens):
    """The H x W pattern-5 board of ``seed`` after ``gens`` generations."""
    step = numpy_step_rule_bounded if boundary == "dead" else numpy_step_rule
    return _frozen(step(random_board(H, W, seed), rule, gens))


@functools.lru_cache(maxsize=None)
def film_of(H, W, seed, rule, boundary, gens, rect):
    return _frozen(numpy_film(random_board(H, W, seed), rule, gens, rect, bounded=boundary == "dead"))


@functools.lru_cache(maxsize=None)
def envelope_of(H, W, seed, rule, gens):
    return _frozen(numpy_envelope(random_board(H, W, seed), rule, gens))


def exact01(t, name):
    """The tensor holds nothing but the bit patterns of its dtype's 0 and 1; returns it as a uint8 numpy array."""
    assert t.dtype == dt(name), (t.dtype, name)
    bits = t.contiguous().view(_BITS[name]).cpu()
    one = _ONE[name]
    ok = (bits == 0) | (bits == one)
    assert bool(ok.all()), f"{name}: {int((~ok).sum())} elements are neither 0 nor 1 bit for bit; first: {bits[~ok].flatten()[:4].tolist()}"
    return (bits == one).to(torch.uint8).numpy()


def assert_cells(t, name, ref):
    got = exact01(t, name)
    assert got.shape == tuple(ref.shape), (got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{name}: {len(bad)} cells of {got.size} differ; first at {bad[0].tolist()}")


def torus_window(board, r0, c0, rows, cols):
    H, W = board.shape
    return board[np.ix_((r0 + np.arange(rows)) % H, (c0 + np.arange(cols)) % W)]


def odd_cells(shape, name, seed):
    """``(tensor, alive)``: a CPU tensor of the dtype with the odd values (floats: 0, 1, 2, -1, 0.5, -0.0 and NaN; uint8:
    0, 1, 2, 255; bool: both) and the uint8 array of the cells that count as alive (``!= 0``)."""
    rng = np.random.default_rng(seed)
    if name == "bool":
        pick = rng.integers(0, 2, size=shape)
        return torch.from_numpy(pick.astype(np.bool_)), pick.astype(np.uint8)
    if name == "uint8":
        vals = np.array([0, 1, 2, 255], np.uint8)
        pick = rng.integers(0, len(vals), size=shape)
        return torch.from_numpy(vals[pick]), (vals[pick] != 0).astype(np.uint8)
    vals = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5, -0.0, float("nan")], dtype=torch.float32)
    alive = np.array([0, 1, 1, 1, 1, 0, 1], np.uint8)
    pick = rng.integers(0, len(alive), size=shape)
    # (every one of them is exact in float16 and bfloat16: the sign of -0.0 and the NaN survive the cast)
    return vals[torch.from_numpy(pick)].to(dt(name)), alive[pick]


SENTINEL = 7


def guarded(shape, name, offset, device):
    """``(store, view)``: a flat sentinel-filled tensor and a contiguous ``shape`` view of it that starts ``offset``
    elements in (so its address is off 16-byte alignment by ``offset`` elements) and ends 9 elements before the end.
    bool views a uint8 store, whose sentinel bytes a bool tensor could not hold."""
    numel = int(np.prod(shape))
    base = torch.uint8 if name == "bool" else dt(name)
    store = torch.full((offset + numel + 9,), SENTINEL, dtype=base, device=device)
    view = store[offset : offset + numel]
    if name == "bool":
        view = view.view(torch.bool)
    return store, view.view(shape)


def assert_guard(store, shape, offset):
    numel = int(np.prod(shape))
    head, tail = store[:offset].cpu(), store[offset + numel :].cpu()
    assert bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all()), (
        f"sentinel overwritten: {int((head != SENTINEL).sum())} elements before, {int((tail != SENTINEL).sum())} after the slice")
