"""NumPy restatement of the engine's device RNG (csrc/util.hip, k_randn), in float64.

A counter stream: element i of a draw depends only on (seed, offset + i).  Two
consecutive counters g = 2q, 2q + 1 share one Box-Muller pair: the hashes h1, h2 of q give
u1 in (0, 1] and u2 in [0, 1), the even counter takes sqrt(-2 ln u1) cos(2 pi u2), the
odd one the sine.  The engine draws the initial codes with (seed, first local element)
and the initial filters with (seed ^ 0xd0d0d0d0, 0); tests/test_gpu_init.py and
tests/test_gpu_multirank.py compare those draws with this module element by element.
Needs no GPU.
"""
import numpy as np

FILTER_SEED_XOR = 0xD0D0D0D0   # the filters' stream: seed ^ this (session2d.cpp / session_hs.cpp)

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def mix64(x):
    """The splitmix64 finaliser on uint64 arrays (wrap-around multiplies)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * _M1
        x = x ^ (x >> np.uint64(27))
        x = x * _M2
        x = x ^ (x >> np.uint64(31))
    return x


def randn_ref(count, seed, offset=0):
    """Elements offset .. offset + count - 1 of the N(0, 1) stream of ``seed``, float64."""
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        g = np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(int(count), dtype=np.uint64)
        q = g >> np.uint64(1)
        h1 = mix64(seed ^ mix64(np.uint64(2) * q + np.uint64(1)))
        h2 = mix64(h1 + _GOLD)
    # (h >> 11) < 2^53 converts to float64 exactly; + 1 reaches 2^53 at most, exact too
    u1 = ((h1 >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53   # (0, 1]
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53           # [0, 1)
    rr = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where((g & np.uint64(1)) != 0, rr * np.sin(ang), rr * np.cos(ang))
