"""The swizzled ("blocked") layout of block scales (reference torchao/prototype/mx_formats/utils.py
``to_blocked`` / ``from_blocked``): the layout cuBLAS wants for block-scaled matmuls and the one a
reference NVFP4 checkpoint stores its weight scales in.

A [rows, cols] matrix of one-byte scales is cut into tiles of 128 rows x 4 columns, row tiles
outermost; each tile is stored as 32 x 16 bytes, scale (r, c) of the tile at byte
``(r % 32) * 16 + (r // 32) * 4 + c``. With ``ncb = ceil(cols / 4)``, scale (r, c) of the matrix is at

    (((r // 128) * ncb + c // 4) * 32 + r % 32) * 16 + ((r % 128) // 32) * 4 + c % 4

(csrc/nvfp4_host.h ``nvfp4_scale_offset`` is the same expression). Rows and columns past the matrix
are zero bytes.
"""

import torch


def ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


def _blocked_index(rows: int, cols: int, device) -> torch.Tensor:
    """int64 [rows, cols]: where scale (r, c) lives in the flat blocked buffer."""
    r = torch.arange(rows, device=device).unsqueeze(1)
    c = torch.arange(cols, device=device).unsqueeze(0)
    tile = (r // 128) * ceil_div(cols, 4) + c // 4
    return (tile * 32 + r % 32) * 16 + ((r % 128) // 32) * 4 + c % 4


def to_blocked(input_matrix: torch.Tensor, use_triton_kernel: bool = False) -> torch.Tensor:
    """[rows, cols] -> flat [ceil(rows / 128) * 128 * ceil(cols / 4) * 4], zero padded.
    ``use_triton_kernel`` is the reference's argument and picks nothing here."""
    rows, cols = input_matrix.shape
    size = ceil_div(rows, 128) * 128 * ceil_div(cols, 4) * 4
    # one-byte float dtypes have no scatter kernel everywhere: move the bytes
    byte_like = input_matrix.element_size() == 1
    src = input_matrix.contiguous().view(torch.uint8) if byte_like else input_matrix
    out = torch.zeros(size, dtype=src.dtype, device=src.device)
    out[_blocked_index(rows, cols, src.device).reshape(-1)] = src.reshape(-1)
    return out.view(input_matrix.dtype) if byte_like else out


def from_blocked(blocked_tensor: torch.Tensor, original_rows: int,
                 original_cols: int) -> torch.Tensor:
    """The inverse of ``to_blocked``: flat blocked buffer -> [original_rows, original_cols]."""
    byte_like = blocked_tensor.element_size() == 1
    src = blocked_tensor.view(torch.uint8) if byte_like else blocked_tensor
    out = src.reshape(-1)[_blocked_index(original_rows, original_cols, src.device)]
    return out.view(blocked_tensor.dtype) if byte_like else out
