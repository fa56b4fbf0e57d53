from .scan import Keys, Scanner  # noqa: F401
