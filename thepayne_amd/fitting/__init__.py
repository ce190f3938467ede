from .sedfit import SEDFit  # noqa: F401
