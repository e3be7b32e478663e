"""Prototype workflows (reference torchao/prototype). Served here: ``mx_formats`` (MXFP8 inference),
``blockwise_fp8_inference`` and ``awq`` (activation-aware scales for the weight-only configs)."""
