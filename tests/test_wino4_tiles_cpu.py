"""The packed tiles of the dilated F(4,3) launches (csrc/common.hpp: wino4_pk_*; csrc/conv_wino4.hip EPI 7, TTSAMD_WINO4 bit 7)
restated in numpy: a row of n outputs at dilation d has G = ceil(n / 4d) groups of 4 d columns = T = d G tuples, tuple t holds the
columns (t / d) 4d + t % d + j d (j = 0..3), tile i the tuples [64 i, 64 i + 64).  Every column of a row must belong to exactly one
tuple of one tile, through the (q0, r0) of the tile as the kernel computes them; the tile counts on the benchmark's own lengths must be
the ones the change was sized with; and the strip positions a tile reads must fit the strip lengths the kernel declares."""
import numpy as np
import pytest

# positions per row of the per-wave strip in the packed form, by kernel size -- static_assert'ed with the same numbers beside Wino4Geo in
# csrc/conv_wino4.hip ("strip lengths of the packed form")
STRIP = {3: 320, 7: 320, 11: 332}
NPOS = {3: 6, 7: 10, 11: 14}            # window positions of a tuple: (k - 1) + 4


def pk_tuples(n, d):
    return d * (-(-n // (4 * d)))


def pk_tiles(n, d):
    return -(-pk_tuples(n, d) // 64)


def pk_tile_columns(i, d):
    """first columns of the 64 slots of tile i, as the kernel forms them: q0 + ((r0 + pe) / d) 4d + (r0 + pe) % d"""
    q0, r0 = (64 * i // d) * 4 * d, 64 * i % d
    s = r0 + np.arange(64)
    return q0, r0, q0 + (s // d) * 4 * d + s % d


@pytest.mark.parametrize('d', [1, 3, 5])
def test_every_column_once(d):
    for n in list(range(1, 701)) + [1028, 1284, 1357, 2048, 28672]:
        T = pk_tuples(n, d)
        hits = np.zeros(n + 4 * d * 64 + 64, dtype=np.int64)
        for i in range(pk_tiles(n, d)):
            _, _, c0 = pk_tile_columns(i, d)
            live = 64 * i + np.arange(64) < T                  # slots past the row's last tuple: computed, never stored
            assert (c0[~live] >= n).all(), (n, d, i)
            for j in range(4):
                np.add.at(hits, c0[live] + j * d, 1)
        assert (hits[:n] == 1).all(), (n, d)
        assert pk_tiles(n, d) == -(-T // 64)
        # a tile past the last has its first group at or past the row's end (the kernel's early return)
        assert (64 * pk_tiles(n, d) // d) * 4 * d >= n
        if d == 1:
            assert pk_tiles(n, 1) == -(-n // 256)               # the plain map


def test_tiles_of_1028_and_1284():
    assert pk_tuples(1028, 5) == 260 and pk_tiles(1028, 5) == 5
    assert [64 * i % 5 for i in range(5)] == [0, 4, 3, 2, 1]
    assert pk_tuples(1028, 3) == 258 and sorted({64 * i % 3 for i in range(pk_tiles(1028, 3))}) == [0, 1, 2]
    assert pk_tuples(1284, 5) == 325 and pk_tiles(1284, 5) == 6


def test_tile_counts_on_the_benchmark_lengths():
    """live time tiles of one conv on the bench's batch (synth_durations(32, 64): 14 341 frames) per HiFi-GAN stage, plain -> packed"""
    from ttsamd import synth
    frames = synth.synth_durations(32, 64).sum(axis=1).astype(np.int64)
    assert int(frames.sum()) == 14341
    want = {(256, 3): (469, 464), (256, 5): (493, 464), (128, 3): (3654, 3602), (128, 5): (3838, 3607), (64, 3): (7296, 7187), (64, 5): (7663, 7191)}
    for (c, d), (plain, packed) in want.items():
        lens = frames * {256: 8, 128: 64, 64: 128}[c]
        w = (256 // (4 * d)) * 4 * d
        assert int((-(-lens // w)).sum()) == plain, (c, d)
        assert sum(pk_tiles(int(n), d) for n in lens) == packed, (c, d)


@pytest.mark.parametrize('d', [3, 5])
@pytest.mark.parametrize('k', [3, 7, 11])
def test_spans_fit_the_strip(k, d):
    """strip column 0 is the window start of column q0 rounded down to a multiple of 4 positions; a slot reads NPOS positions at stride d"""
    pad = (k - 1) // 2
    worst = 0
    for i in range(0, 40):
        q0, r0, c0 = pk_tile_columns(i, d)
        a = (q0 - pad * d) & ~3
        lo = c0 - pad * d - a
        hi = lo + (NPOS[k] - 1) * d
        assert lo.min() >= 0
        worst = max(worst, int(hi.max()) + 1)
    assert worst <= STRIP[k], (k, d, worst)
    # from its first group's start a tile's outputs span at most 264 columns at d = 3 and 278 at d = 5
    assert int(pk_tile_columns(1 if d == 5 else 2, d)[2].max()) + 3 * d + 1 - pk_tile_columns(1 if d == 5 else 2, d)[0] == (278 if d == 5 else 264)


def test_bit_7_without_bit_3_is_rejected():
    """bit 7 says how the F(4,3) kernel runs its dilated launches; without bit 3 it runs none: an error, not an ignored bit"""
    from ttsamd import lib
    for bad in (128, 128 + 7, 128 + 119, 256):
        with pytest.raises(lib.TtsAmdError):
            lib.set_option('TTSAMD_WINO4', bad)
    assert lib.get_option('TTSAMD_WINO4') is None
    try:
        lib.set_option('TTSAMD_WINO4', 255)
        assert lib.get_option('TTSAMD_WINO4') == '255'
        lib.set_option('TTSAMD_WINO4', 128 + 8)
    finally:
        lib.set_option('TTSAMD_WINO4', None)
