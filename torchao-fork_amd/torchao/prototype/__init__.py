"""Prototype workflows (reference torchao/prototype). Served here: ``mx_formats`` (MXFP8 inference)."""
