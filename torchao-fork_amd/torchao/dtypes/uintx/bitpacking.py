"""Bit packing of 1- to 7-bit codes into shards of 4, 2 and 1 bits (the storage of ``UintxLayout``).

The format is the reference's (torchao/dtypes/uintx/bitpacking.py ``pack`` / ``unpack``), written
here from its definition and pinned by the fixtures under tests/golden/uintx_*.npz:

* a code of ``b`` bits is cut into the parts of the set bits of ``b``, widest first and lowest in
  the code: 3 = 2 + 1 bits at positions 0 and 2, 7 = 4 + 2 + 1 bits at positions 0, 4 and 6;
* every part is a uint8 tensor of its own, ``size * w / 8`` long along the packed dimension;
* inside a shard of width ``w`` (``S = 8 / w`` fields per byte) field ``f`` of byte ``i`` holds the
  part of element ``f * (size / S) + i``: the dimension is cut into ``S`` contiguous segments, not
  into neighbouring elements.

csrc/uintx.hip reads these shards in place.
"""

from typing import List

import torch

__all__ = ["pack", "unpack", "shard_widths"]


def shard_widths(elem_size: int) -> List[int]:
    """The shard widths of a code of ``elem_size`` bits, in storage order: 7 -> [4, 2, 1]."""
    if not 1 <= elem_size <= 7:
        raise ValueError(f"elem_size must be in 1..7, got {elem_size}")
    return [w for w in (4, 2, 1) if elem_size & w]


def pack(data: torch.Tensor, elem_size: int, dim: int = -1) -> List[torch.Tensor]:
    """uint8 codes below ``2 ** elem_size`` -> the list of packed uint8 shards along ``dim``,
    whose size must be a multiple of 8."""
    torch._assert(data.dtype == torch.uint8, "data must be uint8")
    size = data.shape[dim]
    torch._assert(size % 8 == 0, f"pack dimension size ({size}) is not divisible by 8")
    shards, pos = [], 0
    for w in shard_widths(elem_size):
        part = (data >> pos) & ((1 << w) - 1)
        fields = 8 // w
        seg = size // fields
        shard = part.narrow(dim, 0, seg).clone()
        for f in range(1, fields):
            shard |= part.narrow(dim, f * seg, seg) << (f * w)
        shards.append(shard)
        pos += w
    return shards


def unpack(shards: List[torch.Tensor], elem_size: int, dim: int = -1) -> torch.Tensor:
    """The inverse of ``pack``: uint8 codes, 8 / elem_size times the shards' total size."""
    widths = shard_widths(elem_size)
    torch._assert(len(shards) == len(widths),
                  f"uint{elem_size} has {len(widths)} shards, got {len(shards)}")
    out, pos = None, 0
    for w, shard in zip(widths, shards):
        torch._assert(shard.dtype == torch.uint8, "shards must be uint8")
        mask = (1 << w) - 1
        part = torch.cat([(shard >> (f * w)) & mask for f in range(8 // w)], dim=dim)
        out = part << pos if out is None else out | (part << pos)
        pos += w
    return out
