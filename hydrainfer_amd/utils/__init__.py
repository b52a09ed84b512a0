import functools


def keyword_argument(name: str, default=None):
    """Class decorator for a dataclass that declares `name` with `field(default=..., init=False)`: the constructor takes
    it BY KEYWORD ONLY and sets it behind the generated __init__, which keeps its signature — and with it positional
    construction — exactly as it is.  The field itself stands wherever it is declared and takes part in repr and
    comparison like any other."""
    def wrap(cls):
        init = cls.__init__

        @functools.wraps(init)
        def __init__(self, *args, **kw):
            value = kw.pop(name, default)
            init(self, *args, **kw)
            setattr(self, name, value)
        cls.__init__ = __init__
        return cls
    return wrap
