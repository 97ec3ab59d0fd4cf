"""Exception hierarchy (reference: honeybadgermpc/exceptions.py)."""


class HoneyBadgerMPCError(Exception):
    """Base class of the errors raised by this package's protocol layer."""


class PreprocessingExhausted(HoneyBadgerMPCError):
    """A protocol needed more preprocessed values than the caller handed in (share_comparison.equal: test bits whose opened
    value is zero are drawn again from spare rows)."""
