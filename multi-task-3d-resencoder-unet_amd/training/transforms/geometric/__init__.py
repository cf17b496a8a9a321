from .geometry import RandomFlipWithNormals, RandomRotate90WithNormals  # noqa: F401
