"""convnet.use_small_tiles: when ConvStackMFMA takes the 64-row tile form (latency mode) by itself.  One threshold, SMALL_TILE_LIMIT, on
the launch's 128-row tile count; host arithmetic, no GPU.  The rule is checked at its candidate limit of 256 tiles (fewer than one
128-row workgroup per CU); the limit that ships is the one the measurement supports (profiles/latency/NOTES.md) and is checked for what
it has to be: one non-negative number that leaves the 64-frame launches alone."""
import ctypes

import pytest

from magnet_amd import convnet


@pytest.fixture(autouse=True)
def candidate_limit(monkeypatch):
    monkeypatch.setattr(convnet, "SMALL_TILE_LIMIT", 256)


def _row_tiles(hip_lib, n_img, h, wp, bm):
    per = ctypes.c_int32(-1)
    return hip_lib.magnet_conv_row_tiles(n_img, h, wp, bm, ctypes.byref(per))


def test_at_the_candidate_limit_one_frame_says_yes_and_the_bench_batch_no(hip_lib):
    assert convnet.use_small_tiles(1, 120, 162)                   # ScanNet grid: 152 tiles of 128 rows
    assert convnet.use_small_tiles(1, 88, 306)                    # KITTI grid: 211
    assert not convnet.use_small_tiles(64, 120, 162)              # 4 864
    assert convnet.use_small_tiles(1, 120, 162, by_image=False) and not convnet.use_small_tiles(64, 120, 162, by_image=False)


@pytest.mark.parametrize("h,wp", [(120, 162), (88, 306), (24, 34), (7, 16)])
def test_at_the_candidate_limit_the_rule_is_monotone_in_the_number_of_images(hip_lib, h, wp):
    """Once a batch is large enough for the 128-row form, every larger batch is (for both ways of counting)."""
    for by_image in (True, False):
        said = [convnet.use_small_tiles(n, h, wp, by_image) for n in range(1, 70)]
        assert said == sorted(said, reverse=True), (h, wp, by_image)


@pytest.mark.parametrize("n_img,h,wp", [(1, 120, 162), (2, 120, 162), (8, 120, 162), (64, 120, 162), (1, 88, 306), (3, 9, 16), (4, 7, 16), (2, 10, 15)])
def test_counts_are_the_librarys(hip_lib, n_img, h, wp):
    n = _row_tiles(hip_lib, n_img, h, wp, 128)
    assert convnet.tiles_128(n_img, h, wp) == n
    assert convnet.tiles_128(n_img, h, wp, by_image=False) == -(-n_img * (h + 2) * wp // 128)
    assert convnet.use_small_tiles(n_img, h, wp) == (n < convnet.SMALL_TILE_LIMIT)


def test_the_64_row_counts_of_one_frame(hip_lib):
    """What the issue's numbers rest on: one frame is 152 tiles of 128 rows (155 flat) and 304 of 64 rows (309 flat); KITTI's 88 x 306
    gives 421 (431 flat)."""
    assert _row_tiles(hip_lib, 1, 120, 162, 128) == 152 and convnet.tiles_128(1, 120, 162, by_image=False) == 155
    assert _row_tiles(hip_lib, 1, 120, 162, 64) == 304 and -(-122 * 162 // 64) == 309
    assert _row_tiles(hip_lib, 1, 88, 306, 64) == 421 and -(-90 * 306 // 64) == 431


def test_the_shipped_limit_is_one_threshold(hip_lib, monkeypatch):
    """The limit that ships (0 after the measurement: the rule says no everywhere and "auto" keeps the 128-row launches)."""
    monkeypatch.undo()
    lim = convnet.SMALL_TILE_LIMIT
    assert isinstance(lim, int) and 0 <= lim <= 256
    assert not convnet.use_small_tiles(64, 120, 162)
    for n in (1, 2, 3, 4, 8):
        assert convnet.use_small_tiles(n, 120, 162) == (convnet.tiles_128(n, 120, 162) < lim)
