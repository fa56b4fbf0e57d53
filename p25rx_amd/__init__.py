from .scan import Scanner  # noqa: F401
