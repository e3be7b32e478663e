"""``Float8MMConfig`` at the reference's module path (torchao/float8/inference.py:28-44), so that a
``Float8Layout(mm_config=...)`` it pickled loads here with ``torch.load(weights_only=True)``."""

from typing import NamedTuple

import torch

__all__ = ["Float8MMConfig"]


class Float8MMConfig(NamedTuple):
    """Options of the reference's scaled mm, carried on the weight's ``Float8Layout`` by the float8
    dynamic-activation config for API and checkpoint compatibility. The kernels here have one
    accumulation mode (fp32) and need no padding, so none of the fields changes a result."""

    emulate: bool = False
    use_fast_accum: bool = False
    pad_inner_dim: bool = False


torch.serialization.add_safe_globals([Float8MMConfig])
