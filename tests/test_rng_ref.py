"""CPU checks of tests/rng_ref.py, the NumPy restatement of the device RNG (csrc/util.hip):
the GPU tests compare the engine's draws with it, so it must not drift itself."""
import math

import numpy as np

from rng_ref import mix64, randn_ref

M64 = (1 << 64) - 1


def _mix_int(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def _randn_int(g, seed):
    """k_randn for one counter in Python integers (no wrap-around to get wrong)."""
    q = g >> 1
    h1 = _mix_int(seed ^ _mix_int((2 * q + 1) & M64))
    h2 = _mix_int((h1 + 0x9E3779B97F4A7C15) & M64)
    u1 = ((h1 >> 11) + 1) * 2.0 ** -53
    u2 = (h2 >> 11) * 2.0 ** -53
    rr = math.sqrt(-2.0 * math.log(u1))
    return rr * (math.sin(2 * math.pi * u2) if g & 1 else math.cos(2 * math.pi * u2))


def test_mix64_known_values():
    # the splitmix64 finaliser: 0 is its fixed point, 1 maps to the published value
    assert int(mix64(np.uint64(0))) == 0
    assert int(mix64(np.uint64(1))) == 0x5692161D100B05E5
    xs = [1, 2, 0xDEADBEEF, M64, 1 << 63, 0x9E3779B97F4A7C15]
    assert [int(v) for v in mix64(np.array(xs, dtype=np.uint64))] == [_mix_int(x) for x in xs]


def test_first_values_are_pinned():
    """Literals recorded from the restatement (and equal to the integer version below):
    seed 0 from the start, seed 12345 from the odd offset 585 (the second half of a
    Box-Muller pair first), and the filters' stream of seed 7."""
    np.testing.assert_allclose(
        randn_ref(6, 0),
        [-0.04483544510742624, 1.2119428786220687, 0.3557285797732026, 0.46241444147035193,
         0.43341317963907816, 0.09511734465885176], rtol=0, atol=2e-15)
    np.testing.assert_allclose(
        randn_ref(4, 12345, 585),
        [1.4693003375725557, 0.3376968228098321, 1.4417538000509966, 0.6979561949984815],
        rtol=0, atol=2e-15)
    np.testing.assert_allclose(
        randn_ref(3, 7 ^ 0xD0D0D0D0),
        [0.4618353250994573, 1.892195447079254, 0.38497575229409686], rtol=0, atol=2e-15)


def test_matches_python_integer_version():
    for seed, off in [(0, 0), (12345, 585), (M64, (1 << 33) + 7), (7 ^ 0xD0D0D0D0, 1)]:
        want = [_randn_int(off + i, seed) for i in range(64)]
        np.testing.assert_allclose(randn_ref(64, seed, off), want, rtol=0, atol=1e-14)


def test_offsets_compose():
    """A draw at offset o equals the tail of the draw at offset 0 (or at any earlier
    offset), bit for bit: at an odd offset, where the first element is the sine half of a
    pair, and above 2^32, where a 32-bit counter would wrap."""
    a = randn_ref(2000, 5)
    assert np.array_equal(a[585:], randn_ref(2000 - 585, 5, 585))
    assert np.array_equal(a[586:], randn_ref(2000 - 586, 5, 586))
    big = 1 << 33
    assert np.array_equal(randn_ref(100, 5, big)[7:], randn_ref(93, 5, big + 7))
    assert not np.array_equal(randn_ref(93, 5, big + 7), randn_ref(93, 5, 7))
    assert randn_ref(0, 5).shape == (0,) and randn_ref(3, 5).dtype == np.float64


def test_stream_is_standard_normal():
    x = randn_ref(200000, 3)
    # mean and std of 2e5 draws: sigma 2.2e-3 and 1.6e-3; bounds at about 4.5 sigma
    assert abs(x.mean()) < 1e-2 and abs(x.std() - 1) < 7e-3
    assert abs(np.corrcoef(x[0::2], x[1::2])[0, 1]) < 1.5e-2   # the two halves of a pair
    assert abs(np.corrcoef(x[:-2:2], x[2::2])[0, 1]) < 1.5e-2  # neighbouring pairs
    assert np.abs(x).max() <= math.sqrt(2 * 53 * math.log(2))  # u1 >= 2^-53
    assert not np.array_equal(x[:100], randn_ref(100, 4))
