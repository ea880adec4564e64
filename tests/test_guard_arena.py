"""tests/guard_arena.py on the CPU: GuardArena.check() is all that stands between a stray store and a green footprint test
(tests/test_gpu_footprint.py, tests/test_gpu_footprint_lwe.py), so its layout promises and its sensitivity are pinned here on numpy
arenas -- both word types, aligned and one word past a 16-byte boundary, with one read-only operand, one written operand and one written
operand that asks for 16-byte alignment (a workspace).  Every single-word change outside the call's outputs must raise, and the message
must name the band or the operand it hit."""
import numpy as np
import pytest

from guard_arena import GuardArena, pattern, splitmix64

RO_WORDS, W_WORDS, WA_WORDS = 37, 21, 64      # odd counts: the slices end off every boundary
W_GUARD, WA_GUARD, W_LEAD = 300, 513, 19

CASES = [(dt, odd) for dt in (np.uint32, np.uint64) for odd in (False, True)]
IDS = ["%s-%s" % (np.dtype(dt).name, "odd" if odd else "aligned") for (dt, odd) in CASES]


def make(dtype, odd, seed=41):
    """operands in arena order: ro (read-only, data), w (written, data, bands of its own sizes), wa (written, a word count, aligned)"""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    ro = rng.integers(0, top, size=RO_WORDS, dtype=dtype, endpoint=True)
    w = rng.integers(0, top, size=W_WORDS, dtype=dtype, endpoint=True)
    ar = GuardArena(dtype, device=False, seed=seed, odd=odd)
    ar.take("ro", ro).take("w", w, written=True, guard=W_GUARD, lead=W_LEAD).take("wa", WA_WORDS, written=True, guard=WA_GUARD, aligned=True)
    return ar.build(), ro, w


def start_of(ar, name):
    """arena word index of the slice, from its address"""
    isz = ar.dtype.itemsize
    off = ar[name].ctypes.data - ar._t.ctypes.data
    assert off % isz == 0
    return off // isz


def raises_once(ar, idx, unchanged=()):
    """flip one bit of arena word idx, expect check() to raise, put the word back; returns the message"""
    keep = ar._t[idx].copy()
    ar._t[idx] ^= ar.dtype.type(1)
    with pytest.raises(AssertionError) as e:
        ar.check(unchanged=unchanged)
    ar._t[idx] = keep
    ar.check(unchanged=unchanged)          # restored: green again, so every case below fails on its own change alone
    msg = str(e.value)
    assert msg.startswith("1 words outside the call's outputs changed; the first is arena word %d: " % idx), msg
    return msg


@pytest.mark.parametrize("dtype,odd", CASES, ids=IDS)
def test_slices_start_where_promised(dtype, odd):
    ar, ro, w = make(dtype, odd)
    isz = np.dtype(dtype).itemsize
    want = isz if odd else 0
    assert ar["ro"].ctypes.data % 16 == want and ar["w"].ctypes.data % 16 == want
    assert ar["wa"].ctypes.data % 16 == 0                      # aligned=True holds in an odd arena too
    assert ar["ro"].dtype == dtype and ar["ro"].size == RO_WORDS and ar["w"].size == W_WORDS and ar["wa"].size == WA_WORDS
    # the slices are views of ONE allocation, in the order taken, with at least the bands asked for between them
    s_ro, s_w, s_wa = (start_of(ar, x) for x in ("ro", "w", "wa"))
    assert s_ro >= 256 and s_w >= s_ro + RO_WORDS + 256 + W_LEAD and s_wa >= s_w + W_WORDS + W_GUARD + 256
    assert ar.total == s_wa + WA_WORDS + WA_GUARD and ar._t.size == ar.total
    # initial content: the data given, pattern words where a count was given, pattern words in every band
    assert np.array_equal(ar["ro"], ro) and np.array_equal(ar["w"], w)
    pat = pattern(ar.total, ar.seed, dtype)
    assert np.array_equal(ar["wa"], pat[s_wa:s_wa + WA_WORDS])
    for lo, hi in ((0, s_ro), (s_ro + RO_WORDS, s_w), (s_w + W_WORDS, s_wa), (s_wa + WA_WORDS, ar.total)):
        assert np.array_equal(ar._t[lo:hi], pat[lo:hi])


@pytest.mark.parametrize("dtype,odd", CASES, ids=IDS)
def test_untouched_and_fully_overwritten_outputs_pass(dtype, odd):
    ar, ro, w = make(dtype, odd)
    got = ar.check()
    assert sorted(got) == ["w", "wa"] and np.array_equal(got["w"], w) and got["wa"].size == WA_WORDS
    assert got["w"].dtype == dtype and not np.shares_memory(got["w"], ar._t)
    new_w, new_wa = np.arange(W_WORDS, dtype=dtype), np.full(WA_WORDS, np.iinfo(dtype).max, dtype=dtype)
    ar["w"][:] = new_w
    ar["wa"][:] = new_wa
    got = ar.check()
    assert np.array_equal(got["w"], new_w) and np.array_equal(got["wa"], new_wa)
    assert np.array_equal(ar.check(unchanged=("ro",))["w"], new_w)     # naming a read-only operand changes nothing


@pytest.mark.parametrize("dtype,odd", CASES, ids=IDS)
def test_every_single_word_outside_the_outputs_is_caught_and_named(dtype, odd):
    ar, ro, w = make(dtype, odd)
    s_ro, s_w, s_wa = (start_of(ar, x) for x in ("ro", "w", "wa"))
    # the word immediately before and immediately after each written slice
    assert "band between operand ro and operand w (1 words before it)" in raises_once(ar, s_w - 1)
    assert "band between operand w and operand wa (%d words before it)" % (s_wa - s_w - W_WORDS) in raises_once(ar, s_w + W_WORDS)
    assert "band between operand w and operand wa (1 words before it)" in raises_once(ar, s_wa - 1)
    assert "band behind operand wa (1 words past its end)" in raises_once(ar, s_wa + WA_WORDS)
    # the two ends of the arena
    assert "band behind operand wa (%d words past its end)" % WA_GUARD in raises_once(ar, ar.total - 1)
    assert "band between the head of the arena and operand ro (%d words before it)" % s_ro in raises_once(ar, 0)
    # the read-only operand: first, inner and last word
    for j in (0, 5, RO_WORDS - 1):
        assert "read-only operand ro, word %d" % j in raises_once(ar, s_ro + j)
    # a written slice the call must leave alone
    for j in (0, W_WORDS - 1):
        assert "operand w, word %d" % j in raises_once(ar, s_w + j, unchanged=("w",))
    assert "operand wa, word 7" in raises_once(ar, s_wa + 7, unchanged=("w", "wa"))
    # ... and the same words pass when the slice is not named
    ar["w"][0] ^= dtype(1)
    ar.check()
    with pytest.raises(AssertionError):
        ar.check(unchanged=("w",))


@pytest.mark.parametrize("dtype,odd", CASES, ids=IDS)
def test_first_and_last_changed_word_are_both_reported(dtype, odd):
    ar, _, _ = make(dtype, odd)
    s_ro, s_wa = start_of(ar, "ro"), start_of(ar, "wa")
    ar._t[s_ro + 2] ^= dtype(4)
    ar._t[s_wa + WA_WORDS + 9] ^= dtype(4)
    with pytest.raises(AssertionError) as e:
        ar.check()
    msg = str(e.value)
    assert msg.startswith("2 words outside") and "read-only operand ro, word 2" in msg
    assert "the last is word %d: band behind operand wa (10 words past its end)" % (s_wa + WA_WORDS + 9) in msg


@pytest.mark.parametrize("dtype,odd", CASES, ids=IDS)
def test_a_shifted_or_repeated_copy_of_a_band_does_not_pass_for_the_band(dtype, odd):
    """the pattern is position dependent: splitmix64(seed + word index), its high half for 32-bit words"""
    ar, _, _ = make(dtype, odd)
    s_w, s_wa = start_of(ar, "w"), start_of(ar, "wa")
    lo, hi = s_wa + WA_WORDS, ar.total
    band = ar._t[lo:hi].copy()
    assert (band[1:] != band[:-1]).all()                       # no two neighbours alike: a shift changes every word
    ar._t[lo:hi - 1] = band[1:]                                # the band shifted down by one word
    with pytest.raises(AssertionError) as e:
        ar.check()
    assert str(e.value).startswith("%d words outside" % (WA_GUARD - 1)) and "band behind operand wa (1 words past its end)" in str(e.value)
    ar._t[lo:hi] = band
    ar.check()
    ar._t[lo + 1:hi] = band[:-1]                               # shifted up by one word
    with pytest.raises(AssertionError):
        ar.check()
    ar._t[lo:hi] = band
    ar._t[lo:lo + W_GUARD] = ar._t[s_w + W_WORDS:s_w + W_WORDS + W_GUARD]      # another band of the same arena, word for word
    with pytest.raises(AssertionError) as e:
        ar.check()
    assert str(e.value).startswith("%d words outside" % W_GUARD)
    ar._t[lo:hi] = band
    ar.check()


def test_pattern_is_splitmix64_of_seed_plus_index():
    """the published constants (Steele, Lea, Flood: SplittableRandom), on Python ints"""
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    want = [sm(1000 + i) for i in range(50)]
    assert [int(x) for x in splitmix64(np.arange(50, dtype=np.uint64) + np.uint64(1000))] == want
    assert [int(x) for x in pattern(50, 1000, np.uint64)] == want
    assert [int(x) for x in pattern(50, 1000, np.uint32)] == [x >> 32 for x in want]
    assert sm(0) == 0xE220A8397B1DCDAF                        # the first output of a splitmix64 stream seeded with 0
    assert pattern(50, 1000, np.uint32).dtype == np.uint32 and pattern(50, 1000, np.uint64).dtype == np.uint64


def test_two_seeds_give_two_patterns_and_take_refuses_a_second_use_of_a_name():
    a, _, _ = make(np.uint64, False, seed=1)
    b, _, _ = make(np.uint64, False, seed=2)
    assert a.total == b.total and not (a.pattern == b.pattern).any()
    ar = GuardArena(np.uint32, device=False, seed=3).take("x", 4)
    with pytest.raises(AssertionError):
        ar.take("x", 4)
    ar.build()
    with pytest.raises(AssertionError):
        ar.take("y", 4)
