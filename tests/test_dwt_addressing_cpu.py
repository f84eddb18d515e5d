"""CPU test: the forward transform launcher's choice between 32-bit offsets into plane descriptors and 64-bit addresses
(include/spiht_hip.h: spiht_dwt_addr32; common.h: dwt_narrow_ok).  Host arithmetic only -- nothing is allocated."""


def _addr32():
    from spiht_amd import _lib
    return _lib.lib().spiht_dwt_addr32


def test_launcher_picks_wide_addressing_where_offsets_do_not_fit():
    f = _addr32()
    G = 1 << 30
    # the benchmark's level 1 (1080 x 1920, bior2.2, level 7) and a small picture
    assert f(1080, 1920, 542, 962, 1111, 1949, 0, 0, 0) == 1
    assert f(3, 3, 4, 4, 8, 8, 0, 0, 0) == 1
    # float64 input plane: 11585^2 * 8 bytes is the last size under 2^30
    assert 11585 * 11585 * 8 < G <= 11586 * 11586 * 8
    assert f(11585, 11585, 8, 8, 16, 16, 0, 0, 0) == 1
    assert f(11586, 11586, 8, 8, 16, 16, 0, 0, 0) == 0
    assert f(1, G // 8, 8, 8, 16, 16, 0, 0, 0) == 0 and f(1, G // 8 - 1, 8, 8, 16, 16, 0, 0, 0) == 1
    # the packed array (4 bytes a cell) and the approximation (8 bytes a sample)
    assert f(64, 64, 8, 8, 16384, 16383, 0, 0, 0) == 1
    assert f(64, 64, 8, 8, 16384, 16384, 0, 0, 0) == 0
    assert f(64, 64, 11585, 11585, 16, 16, 0, 0, 0) == 1
    assert f(64, 64, 11586, 11586, 16, 16, 0, 0, 0) == 0
    # rows of a tile below the level's last row are addressed (and dropped): (out_h + 64) rows must stay under 2^31
    assert f(64, 64, 1, 8, 2, (1 << 31) // (65 * 4) - 1, 0, 0, 0) == 1
    assert f(64, 64, 1, 8, 2, (1 << 31) // (65 * 4) + 1, 0, 0, 0) == 0
    assert f(64, 64, 1, (1 << 31) // (65 * 8) - 1, 2, 8, 0, 0, 0) == 1
    assert f(64, 64, 1, (1 << 31) // (65 * 8) + 1, 2, 8, 0, 0, 0) == 0
    # an 8- / 16-bit view goes by the byte span of its strides, not by its pixel count
    assert f(1080, 1920, 542, 962, 1111, 1949, 1, 1920, 1) == 1
    assert f(1080, 1920, 542, 962, 1111, 1949, 2, 4 * 1920 * 2 + 12, 8) == 1
    sh = (G - 1 - 1920) // 1079  # the longest row stride whose span 1079 * sh + 1919 + 1 stays under 2^30
    assert f(1080, 1920, 542, 962, 1111, 1949, 1, sh, 1) == 1
    assert f(1080, 1920, 542, 962, 1111, 1949, 1, sh + 1, 1) == 0
    assert f(2, 1920, 542, 962, 1111, 1949, 1, G, 1) == 0
    assert f(1080, 2, 542, 962, 1111, 1949, 2, 4, G) == 0
    assert f(1080, 1920, 542, 962, 1111, 1949, 1, -1920, 1) == 0
    # nonsense sizes never take the narrow path
    assert f(0, 8, 8, 8, 8, 8, 0, 0, 0) == 0 and f(8, 8, 0, 8, 8, 8, 0, 0, 0) == 0
