"""Float8 inference configuration (the reference's ``torchao.float8`` holds its training stack too,
which is out of scope here)."""

from torchao.float8.inference import Float8MMConfig

__all__ = ["Float8MMConfig"]
