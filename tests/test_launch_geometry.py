"""The launch geometry of the post-processing kernels on the host (no GPU): quad_grid / quad_blocks / quad_chunks (ofdis_quad.h)
and xcd_frame_map (ofdis_dev.h) through the test library, whose two launch limits a test can lower (tests/launch_hooks.py).

The launchers of ofdis_interp / tfilter / trajfilter / gmotion / stabilize walk the frames of a call in chunks of at most
QUAD_MAX_BLOCKS workgroups (quad_chunks), and their kernels turn a workgroup index into (frame of the chunk, block of the
frame) with xcd_frame_map.  Walked here by that loop itself, with a callback that records instead of launching, every (frame,
block) of the clip must come up exactly once: for one launch and for many, for chunks below 8 frames (consecutive blocks) and
from 8 (the XCD mapping with its padded last group).

The core launchers (patch search, densification, warp, derivatives, the per-stage TV and stereo systems, the finish) launch
every frame at once on the grid of xcd_grid (ofdis_dev.h); the same coverage is required of it, and slot_rows
(ofdis_kernels.h) is pinned at its thresholds."""
import numpy as np
import pytest

from launch_hooks import QUAD_MAX_BLOCKS, chunk_walk, launch_limits, quad_grid, slot_rows, xcd_frame_map, xcd_grid

# (w, h) with 1, 3 and 7 workgroups of 256 quads per frame
SHAPES = {1: (4, 1), 3: (64, 48), 7: (4, 7 * 256)}
# frames per launch the limit is chosen for: 11 is rounded down to 8, None is the product's limit (one launch)
CHUNKS = [1, 3, 8, 11, 16, None]


def _covered(nframes, w, h):
    """every (frame of the clip, block) the launches of one call work on, with repetitions: [(frame, blk)], and the walk"""
    bpf, walk = chunk_walk(nframes, w, h)
    cells = []
    for f0, n, blocks in walk:
        frame, blk = xcd_frame_map(blocks, bpf, n)
        assert (blk >= 0).all() and (blk < bpf).all() and (frame >= 0).all()
        live = frame < n   # (the kernels return where frame >= n: the padding of the last group of 8)
        cells.append(np.stack([f0 + frame[live], blk[live]], 1))
    return bpf, walk, np.concatenate(cells)


@pytest.mark.parametrize("bpf", sorted(SHAPES))
@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunks-of-{c or 'everything'}")
def test_chunk_walk_covers_every_block_of_every_frame_once(bpf, chunk):
    w, h = SHAPES[bpf]
    limit = chunk * bpf if chunk else 0
    want_chunk = None if chunk is None else (chunk if chunk < 8 else chunk & ~7)
    with launch_limits(quad_max_blocks=limit):
        for nframes in range(1, 41):
            got_bpf, walk, cells = _covered(nframes, w, h)
            what = f"{nframes} frames, bpf {bpf}, limit {limit}"
            assert got_bpf == bpf, what
            # the walk itself: consecutive chunks of the expected size, the last one ragged
            size = nframes if want_chunk is None else min(want_chunk, nframes)
            assert [f0 for f0, _, _ in walk] == list(range(0, nframes, size)), what
            assert all(n == min(size, nframes - f0) for f0, n, _ in walk), what
            if limit:
                assert all(blocks <= limit for _, _, blocks in walk), what
            # every (frame, blk) of the clip exactly once
            want = np.stack(np.meshgrid(np.arange(nframes), np.arange(bpf), indexing="ij"), -1).reshape(-1, 2)
            got = cells[np.lexsort((cells[:, 1], cells[:, 0]))]
            assert got.shape == want.shape and np.array_equal(got, want), what


def test_a_frames_blocks_share_an_xcd_from_8_frames():
    """what the mapping is for: from 8 frames all workgroups of a frame have the same index mod 8; below, they are consecutive"""
    for nframes, bpf in ((8, 3), (11, 7), (27, 1)):
        frame, blk = xcd_frame_map(-(-nframes // 8) * 8 * bpf, bpf, nframes)
        for f in range(nframes):
            assert len(set(np.flatnonzero(frame == f) % 8)) == 1
    frame, blk = xcd_frame_map(7 * 3, 3, 7)
    assert np.array_equal(frame, np.repeat(np.arange(7), 3)) and np.array_equal(blk, np.tile(np.arange(3), 7))


@pytest.mark.parametrize("bpf", [1, 3, 7])
@pytest.mark.parametrize("nframes", [1, 7, 8, 9, 27])
def test_core_grid_covers_every_block_of_every_frame_once(nframes, bpf):
    """the core launchers (patch search, densification, warp, derivatives, TV system and finish, stereo system): the grid xcd_grid
    gives them, walked by xcd_frame_map as their kernels do, reaches every (frame, block) exactly once; the rest is the
    padding of the last group of 8 frames, which the kernels skip"""
    blocks = xcd_grid(nframes, bpf)
    assert blocks == -(-nframes // 8) * 8 * bpf
    frame, blk = xcd_frame_map(blocks, bpf, nframes)
    assert (blk >= 0).all() and (blk < bpf).all() and (frame >= 0).all()
    live = frame < nframes
    got = np.stack([frame[live], blk[live]], 1)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    want = np.stack(np.meshgrid(np.arange(nframes), np.arange(bpf), indexing="ij"), -1).reshape(-1, 2)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_core_grid_counts_in_64_bits_and_refuses_what_an_int_cannot_index():
    assert xcd_grid(65535, 32767) == 65536 * 32767          # (2^31 - 65536: the largest multiple that fits)
    assert xcd_grid(65535, 32768) is None                   # 2^31 blocks: wrapped to 0 in 32-bit arithmetic
    assert xcd_grid(8, (1 << 28) - 1) == (1 << 31) - 8 and xcd_grid(8, 1 << 28) is None
    assert xcd_grid(1, 1 << 40) is None


def test_rows_per_frame_slot():
    assert [slot_rows(h) for h in (1, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64]


@pytest.mark.parametrize("nframes,w,h,bpf,chunk", [(16384, 1024, 436, 436, 9616), (65535, 1920, 1080, 2025, 2064),
                                                    (1, 8191, 8191, 65528, 1)])
def test_product_limits(nframes, w, h, bpf, chunk):
    """limits = 0, the product's: every launch stays within 2^22 workgroups, and the chunk is a multiple of 8 where it is at least
    8.  16384 pairs of 1024x436 (the headline batch) take two launches of 9616 and 6768; 1920x1080 takes chunks of 2064 frames."""
    with launch_limits(0, 0):
        assert quad_grid(nframes, w, h) == (bpf, chunk)
        got_bpf, walk = chunk_walk(nframes, w, h)
    assert sum(n for _, n, _ in walk) == nframes and len(walk) == -(-nframes // chunk)
    assert all(blocks <= QUAD_MAX_BLOCKS for _, _, blocks in walk)
    assert chunk < 8 or chunk % 8 == 0
    if (w, h) == (1024, 436):
        assert [n for _, n, _ in walk] == [9616, 6768]


def test_limits_return_to_the_product_values_after_a_failure():
    with pytest.raises(RuntimeError):
        with launch_limits(quad_max_blocks=3, grid_max_blocks=1):
            assert quad_grid(27, 4, 1) == (1, 3)
            raise RuntimeError("a failing test body")
    assert quad_grid(27, 4, 1) == (1, 27) and quad_grid(16384, 1024, 436) == (436, 9616)
