from .float8_layout import Float8AQTTensorImpl, Float8Layout, Float8MMConfig

__all__ = ["Float8AQTTensorImpl", "Float8Layout", "Float8MMConfig"]
