"""Guard-banded buffers for the caller-workspace contract (tests/test_workspace_contract_cpu.py, tests/test_gpu_workspace_contract.py).
Not a test module.

A buffer under test lies between two guards of GUARD bytes: `whole` = [guard | interior | guard].  GUARD is a multiple of the 256-byte
granule of the library's workspace carve, so the interior keeps the alignment of the allocation.  The whole allocation is painted with
one pattern before a call; afterwards `guards_intact` compares both guards byte for byte with a copy taken before the call.

The patterns (FILLS): 0x00; 0xFF (NaN or the largest value in every number format the library keeps in a workspace); "random" (seeded
bytes); "stale" - what the same operation left behind after a call on a larger or denser input.  A stale arena cannot be painted: the
GPU test makes one by running that call in a "random" arena and not refilling it."""
import torch

GUARD = 4096
FILLS = (0x00, 0xFF, "random", "stale")


def paint(t: torch.Tensor, fill, seed: int = 0) -> torch.Tensor:
    """Fill the uint8 tensor `t` with the pattern `fill` (0x00, 0xFF or "random"; "stale" starts from "random")."""
    if fill in ("random", "stale"):
        g = torch.Generator().manual_seed(0x5EED + int(seed) + t.numel())
        t.copy_(torch.randint(0, 256, (t.numel(),), dtype=torch.uint8, generator=g))
    else:
        t.fill_(int(fill))
    return t


def arena(nbytes: int, fill, device="cpu", seed: int = 0):
    """-> (whole, interior): uint8 tensors, interior = whole[GUARD:GUARD + nbytes] (a view), all of `whole` painted with `fill`."""
    nbytes = int(nbytes)
    whole = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
    paint(whole, fill, seed)
    return whole, whole[GUARD:GUARD + nbytes]


def typed_arena(shape, dtype, fill, device="cpu", seed: int = 0):
    """-> (whole, tensor): an output buffer of `shape` and `dtype` whose storage is the interior of an arena painted with `fill`."""
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    whole, interior = arena(n * torch.empty((), dtype=dtype).element_size(), fill, device, seed)
    return whole, interior.view(dtype).view(shape)


def guards_intact(whole: torch.Tensor, nbytes: int, fill_before: torch.Tensor) -> bool:
    """Both guards of `whole` equal those of `fill_before` (a clone of `whole` taken before the call) byte for byte."""
    nbytes = int(nbytes)
    assert whole.numel() == fill_before.numel() == 2 * GUARD + nbytes
    return bool(torch.equal(whole[:GUARD], fill_before[:GUARD]) and torch.equal(whole[GUARD + nbytes:], fill_before[GUARD + nbytes:]))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shapes, dtypes and bytes (NaNs and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)))
