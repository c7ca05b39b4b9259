"""Torch tensors in and out of the native core, and :func:`evolve`.

The native side takes ``(data_ptr, element type code, numel)`` and converts between dense elements and the packed
split words where the words are: on the HIP backend with the kernels of ``tensor_kernels.hip`` on CUDA tensors of the
simulation's device, on the CPU backend with a host loop on CPU tensors.  There is no libtorch dependency, and ``torch`` is
imported here only when one of these functions runs.

Element types: ``torch.bool`` and ``torch.uint8`` (one byte per cell), ``torch.float16``, ``torch.bfloat16`` and
``torch.float32``.  Results hold exactly 0 and 1.  On the way in a cell is alive iff its element ``!= 0``: ``-0.0`` is dead,
NaN is alive.

Stream ordering: before the native side reads or writes a CUDA tensor, the caller's current torch stream on that device is
synchronised (:func:`sync`); the native side runs on its own stream and synchronises it before it returns.  So work queued
on the current stream before a call is seen by it, and a result is complete when the call returns.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

SIZES = (64, 128, 256)


def _torch():
    import torch

    return torch


def dtype_code(dtype, what: str) -> int:
    """The native element type code of a torch dtype; ``ValueError`` naming any other dtype."""
    torch = _torch()
    codes = {torch.bool: 0, torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}
    if dtype not in codes:
        raise ValueError(f"{what}: dtype {dtype} is not one of torch.bool, uint8, float16, bfloat16, float32")
    return codes[dtype]


def device_of(backend: str, index: int):
    """Where a backend's tensors live: ``cuda:<index>`` for ``hip``, the CPU for ``cpu``."""
    torch = _torch()
    return torch.device("cuda", int(index)) if backend == "hip" else torch.device("cpu")


def check_device(t, device, what: str) -> None:
    if t.device != device:
        side = "HIP" if device.type == "cuda" else "CPU"
        raise ValueError(f"{what}: the tensor is on {t.device}, this {side} backend takes tensors on {device}")


def check_input(t, shape: Tuple[int, ...], device, what: str):
    """A tensor argument of the given shape on the backend's device, made contiguous; ``ValueError`` otherwise."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected a tensor of shape {tuple(shape)}, got {tuple(t.shape)}")
    dtype_code(t.dtype, what)
    check_device(t, device, what)
    return t.contiguous()


def result(shape: Tuple[int, ...], dtype, device, out, what: str):
    """The tensor a reader fills: ``out`` after its checks (shape, dtype, contiguity, device), else ``torch.empty``."""
    torch = _torch()
    if out is None:
        dtype = torch.uint8 if dtype is None else dtype
        dtype_code(dtype, what)
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if not isinstance(out, torch.Tensor):
        raise ValueError(f"{what}: out must be a torch.Tensor, got {type(out).__name__}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: out has shape {tuple(out.shape)}, the result is {tuple(shape)}")
    dtype_code(out.dtype, what)
    if dtype is not None and out.dtype != dtype:
        raise ValueError(f"{what}: out has dtype {out.dtype}, the call asks for {dtype}")
    if not out.is_contiguous():
        raise ValueError(f"{what}: out is not contiguous (strides {tuple(out.stride())} for shape {tuple(out.shape)})")
    check_device(out, device, what)
    return out


def sync(t) -> None:
    """Synchronise torch's current stream on the tensor's device (CUDA tensors; see the module docstring)."""
    if t.is_cuda:
        _torch().cuda.current_stream(t.device).synchronize()


def handle(t, what: str = "tensor"):
    """``(data_ptr, element type code, numel)`` of a contiguous tensor."""
    return t.data_ptr(), dtype_code(t.dtype, what), t.numel()


def index_range(indices: Optional[Sequence[int]], n: int, what: str) -> Tuple[int, int]:
    """``(first, count)`` of ``indices``: ``None`` (all ``n``) or a non-empty run of consecutive ascending indices inside
    ``0 .. n - 1`` (a ``range`` of step 1, or any sequence that spells one out); ``ValueError`` otherwise."""
    if indices is None:
        return 0, n
    idx = [int(i) for i in indices]
    if not idx:
        raise ValueError(f"{what}: indices {indices!r} are empty")
    if any(b != a + 1 for a, b in zip(idx, idx[1:])):
        shown = indices if isinstance(indices, range) else idx[:8]
        raise ValueError(f"{what}: indices {shown!r} are no contiguous range (first, first + 1, ...); use boards() for a selection")
    if idx[0] < 0 or idx[-1] >= n:
        raise ValueError(f"{what}: indices {idx[0]} .. {idx[-1]} are outside 0 .. {n - 1}")
    return idx[0], len(idx)


def evolve(x, generations: int, rule: str = "B3/S23"):
    """``generations`` steps of every board of ``x`` under a Moore ``rule`` on the torus: ``x`` is one ``(S, S)`` board or a
    batch ``(B, S, S)``, ``S`` 64, 128 or 256, at most 2^20 boards, of any accepted dtype (nonzero = alive).  Returns a new
    tensor of the same shape, dtype and device holding 0 and 1.

    The backend follows ``x.device``: a CUDA tensor runs the soup kernel ``step_soups`` (one wave64 per board, the board in
    registers) between a pack and an unpack kernel and never leaves the device; a CPU tensor runs the CPU backend.
    Stream ordering is the module's: the current stream is synchronised first, the result is complete on return."""
    from ..models.soups import SoupBatch

    torch = _torch()
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"evolve: expected a torch.Tensor, got {type(x).__name__}")
    if x.dim() not in (2, 3) or x.shape[-1] != x.shape[-2] or x.shape[-1] not in SIZES:
        raise ValueError(f"evolve: a tensor of shape {tuple(x.shape)} is not (S, S) or (B, S, S) with S in 64, 128, 256")
    if x.dim() == 3 and not 1 <= x.shape[0] <= (1 << 20):
        raise ValueError(f"evolve: a batch of {x.shape[0]} boards is outside 1 .. 2^20")
    if int(generations) < 0:
        raise ValueError(f"evolve: generations = {generations} is negative")
    dtype_code(x.dtype, "evolve")
    if x.device.type not in ("cuda", "cpu"):
        raise ValueError(f"evolve: a tensor on {x.device} is neither a CUDA nor a CPU tensor")
    boards = x.reshape((-1,) + tuple(x.shape[-2:]))
    batch = SoupBatch.from_tensor(boards, rule=rule)
    batch.step(int(generations))
    return batch.boards_tensor(dtype=x.dtype).reshape(x.shape)
