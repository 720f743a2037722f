"""The argument checks that soil.py and erosion.py share: each takes the caller's name `who` ("diffuse_batch",
"ErosionBatch.evolve") as the message's prefix, raises ValueError on a bad argument and returns the value as the C call
takes it.  A number is a numbers.Real that is no bool (a Python or numpy scalar alike), a count a numbers.Integral.
The plane checks stay with their callers: the two files word them differently."""
import ctypes as C
import math
import numbers

from . import _abi


def number(who, name, v, lo=0):
    """`v` as a float: a finite number, >= `lo` unless that is None."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (lo is not None and v < lo):
        raise ValueError("%s: %s must be a finite number%s, got %r" % (who, name, "" if lo is None else " >= %d" % lo, v))
    return float(v)


def count(who, name, v, lo=1, below=2 ** 31):
    """`v` as an int: an integer in [lo, below), without an upper end when `below` is None."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or (below is not None and v >= below):
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, name, lo, v))
    return int(v)


def exponent(who, v):
    """`v` as a float: the slope exponent of stream_power_n, a finite number in [1, 16]."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 1 or v > 16:
        raise ValueError("%s: n must be a finite number in 1 .. 16 (a slope exponent below 1 needs a safeguarded solve "
                         "per cell), got %r" % (who, v))
    return float(v)


def edge(who, v):
    if isinstance(v, bool) or v not in (_abi.D4, _abi.D8):
        raise ValueError("%s: edge must be d4 or d8, got %r" % (who, v))
    return int(v)


def kind(who, v, kinds, note=""):
    if v not in kinds:
        names = ["%r" % k for k in kinds]
        raise ValueError("%s: kind must be %s or %s%s, got %r" % (who, ", ".join(names[:-1]), names[-1], note, v))


def border(who, v):
    """1 for "fixed", 0 for "free"."""
    if v not in ("fixed", "free"):
        raise ValueError("%s: border must be 'fixed' or 'free', got %r" % (who, v))
    return int(v == "fixed")


def first_axis(who, v):
    if isinstance(v, bool) or v not in (0, 1):
        raise ValueError("%s: first_axis must be 0 or 1, got %r" % (who, v))
    return int(v)


def kappa_or_diffusivity(who, kappa, diffusivity):
    """Exactly one of the two is given; the number, if it is that one, is finite and >= 0."""
    if (kappa is None) == (diffusivity is None):
        raise ValueError("%s: exactly one of kappa and diffusivity must be given" % who)
    if kappa is not None:
        number(who, "kappa", kappa)


def valid_temperature(T):
    """Whether soil_random_weighted, soil_random_weighted_batch and soil_multiflow take `T` (soil_hip.h): as a
    float32 it is 0 or a normal positive number.  They refuse anything else (ValueError here)."""
    t = C.c_float(float(T)).value
    return t == 0.0 or 2.0 ** -126 <= t < math.inf


def draw(who, T, offset):
    """The temperature and the offset of a random_weighted draw."""
    if T is None or isinstance(T, bool) or not isinstance(T, numbers.Real) or not math.isfinite(T):
        raise ValueError("%s: kind 'random_weighted' needs a finite temperature T, got %r" % (who, T))
    if not valid_temperature(T):
        raise ValueError("%s: T must be 0 or a normal positive float32, got %r" % (who, T))
    count(who, "offset", offset, lo=0, below=None)
