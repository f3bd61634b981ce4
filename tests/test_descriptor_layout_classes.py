"""CPU: the layout lists of tests/test_gpu_bof.py and tests/test_gpu_kmeans.py hold a member of every layout class of the
track-description chain, the classes derived from the launchers' own choices (tests/layout_classes.py through the host-only
hooks bof_assign_shape, km_geom and km_finish_log2te of the test library) -- not from a comment that restates the dispatch.

A class is what a kernel does differently from one C = nxy^2 nt to the next: which bof_assign_kernel<NK, TG>, how many k-steps
either channel length has and whether its last one, and its last 16-byte fragment, is cut; the lanes and passes of the k-means
sum, the passes a channel fills and whether the last is cut, the bytes of the 9 C channel's last dword; the finish kernel's thread
split on either channel.  Deleting a layout from a list so that a class loses its last member fails here.

Also: ofdis_track_descriptor_dims and ofdis_codebook_train_work_bytes against the header's statement for every C."""
import os

import pytest

import layout_classes as LC
import test_gpu_bof as B
import test_gpu_kmeans as K
from of_dis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_C = sorted({LC.cells(s) for s in LC.PAIRS})


def test_the_public_ranges_give_32_pairs_and_28_values_of_C():
    assert len(LC.PAIRS) == 32 and len(ALL_C) == 28 and ALL_C[0] == 1 and ALL_C[-1] == 128


def test_the_hooks_agree_with_what_the_kernels_need():
    """the choices themselves: every channel fits the kernel picked for it"""
    for C in ALL_C:
        nk, NK, TG = LC.bof_shape(C)
        assert nk == -(-9 * C // 64) and (NK, TG) in ((2, 8), (6, 3), (18, 1)) and nk <= NK, (C, nk, NK, TG)
        assert NK == min(v for v in (2, 6, 18) if v >= nk), (C, nk, NK)   # the smallest kernel that holds the channel
        assert 16 <= NK * TG <= 18                                         # fragments of four registers per lane
        np_, el, rl = LC.km_geom(C)
        nd = -(-9 * C // 4)
        assert el in (4, 8, 16, 32, 64) and np_ in (1, 5) and el * np_ >= nd and rl == 4 * el * np_, (C, np_, el, rl)
        assert (np_ == 1 and (el == 4 or el // 2 < nd)) or (np_ == 5 and el == 64 and nd > 64), (C, np_, el)
        for n in (8 * C, 9 * C):
            te = LC.km_finish_split(n)
            assert te in (16, 128, 256) and 256 % te == 0 and (te >= n or te == 256), (C, n, te)


def test_the_sweep_has_one_layout_for_every_C_and_keeps_the_three():
    assert sorted(LC.cells(s) for s in B.SWEEP_LAYOUTS) == ALL_C
    assert all(s in LC.PAIRS for s in B.SWEEP_LAYOUTS)
    assert B.LAYOUTS == K.LAYOUTS == [(1, 1), (2, 3), (4, 8)] and all(s in B.SWEEP_LAYOUTS for s in B.LAYOUTS)
    assert sorted(B.NEW_LAYOUTS + B.LAYOUTS) == sorted(B.SWEEP_LAYOUTS) and len(B.NEW_LAYOUTS) == 25
    assert K.NEW_LAYOUTS is B.NEW_LAYOUTS


def test_the_sweep_has_a_member_of_every_class():
    assert not LC.missing(B.SWEEP_LAYOUTS), LC.missing(B.SWEEP_LAYOUTS)
    # what the issue named as never run is among the classes, so the assertion above is about them
    classes = {C: LC.layout_class(C) for C in ALL_C}
    assert {c.variant for c in classes.values()} == {(2, 8), (6, 3), (18, 1)}
    assert {c.el for c in classes.values()} == {4, 8, 16, 32, 64} and {c.mod4 for c in classes.values()} == {0, 1, 2, 3}
    assert any(c.el == 64 and c.np == 1 for c in classes.values())
    assert any(c.np == 5 and c.passes[1] < 5 for c in classes.values())
    assert any(c.variant == (18, 1) and c.cut_fragment and c.nk[1] < 9 for c in classes.values())
    assert {c.finish for c in classes.values()} == {(16, 16), (16, 128), (128, 128), (128, 256), (256, 256)}


@pytest.mark.parametrize("drop", B.SWEEP_LAYOUTS, ids=B._id)
def test_a_sweep_without_one_layout_misses_a_class(drop):
    """every layout of the sweep is the last member of its class: the check above notices any single deletion"""
    lost = LC.missing([s for s in B.SWEEP_LAYOUTS if s != drop])
    assert list(lost.values()) == [[LC.cells(drop)]], (drop, lost)


def test_the_subsets_have_a_member_of_every_class_they_are_for():
    variants = [LC.layout_class(LC.cells(s)).variant for s in B.SECOND_WORKGROUP_LAYOUTS]
    assert sorted(variants) == [(2, 8), (6, 3), (18, 1)], variants
    for s, variant in zip(B.STRUCTURED_LAYOUTS, ((6, 3), (18, 1))):   # a cut last fragment and k-step in both
        c = LC.layout_class(LC.cells(s))
        assert c.variant == variant and c.cut_fragment and c.cut_kstep, (s, c)
    long_layouts = K.LAYOUTS + K.LONG_SEGMENT_LAYOUTS
    assert not LC.missing(long_layouts, LC.sum_class), LC.missing(long_layouts, LC.sum_class)
    assert not LC.missing(long_layouts, LC.finish_class), LC.missing(long_layouts, LC.finish_class)
    assert {LC.layout_class(LC.cells(s)).mod4 for s in K.LAYOUTS + K.TAIL_BYTES_LAYOUTS} == {0, 1, 2, 3}
    assert [LC.layout_class(LC.cells(s)).mod4 for s in K.TAIL_BYTES_LAYOUTS] == [2, 3]
    nxy, nt = B.END_TO_END_16_CELLS[7:]
    assert LC.layout_class(nxy * nxy * nt).variant == (6, 3) and LC.sum_class(nxy * nxy * nt)[:2] == (64, 1)
    assert LC.finish_class(nxy * nxy * nt) == (128, 256)
    assert len(set(long_layouts)) == len(long_layouts) and all(s in B.SWEEP_LAYOUTS for s in long_layouts)


def test_the_codebook_sizes_come_from_the_tile_of_the_layouts_kernel():
    assert [B._nwords((4, 1), w) for w in B.SWEEP_NWORDS] == [5, 49, 109]   # <6, 3>: tiles of 48
    for s in B.SWEEP_LAYOUTS:
        tile = 16 * LC.bof_shape(LC.cells(s))[2]
        sizes = [B._nwords(s, w) for w in B.SWEEP_NWORDS]
        assert sizes == [5, tile + 1, 2 * tile + 13] and sizes[2] <= max(B.NWORDS), (s, sizes)   # (the codebook of _data has 300)
        assert sizes[0] < tile and sizes[2] % 16 and -(-sizes[2] // tile) == 3


def test_the_descriptor_size_is_33_C():
    for nxy, nt in LC.PAIRS:
        assert capi.track_descriptor_dims(12, nxy, nt) == 33 * nxy * nxy * nt == B._layout(nxy, nt)["dims"]


def _work_bytes(M, C, K_):
    """include/ofdis.h on ofdis_codebook_train_work_bytes, restated: prev, dist and rank int32 / u32 [M][4]; off u32 [4][K + 1];
    order u32 [4][M]; slab u32 [4][ceil(M / 256)][2][RL]; every section a multiple of 8 bytes (ofdis_kmeans.hip).  RL: the entries
    of the longest channel padded to the lanes that sum them -- a power of two of lanes from 4 up to 64 in one pass, or five
    passes of 64 -- 4 entries per lane"""
    nd = -(-9 * C // 4)
    lanes = 5 * 64 if nd > 64 else max(4, 1 << (nd - 1).bit_length())
    RL = 4 * lanes
    assert 16 <= RL <= 1280
    up8 = lambda b: (b + 7) // 8 * 8
    return 3 * 16 * M + up8(16 * (K_ + 1)) + 16 * M + 4 * -(-M // 256) * 2 * RL * 4


def test_the_work_buffer_is_the_layout_the_header_documents():
    for nxy, nt in LC.PAIRS:
        C = nxy * nxy * nt
        for M, K_ in ((1, 1), (200, 5), (256, 4), (257, 300), (709, 37), (100000, 4000)):
            assert capi.codebook_train_work_bytes(M, nxy, nt, K_) == _work_bytes(M, C, K_), (nxy, nt, M, K_)
        # the slab row of the hook is the header's RL: one more chunk adds 4 channels x 2 rows x RL entries of 4 bytes
        step = capi.codebook_train_work_bytes(257, nxy, nt, 1) - capi.codebook_train_work_bytes(256, nxy, nt, 1) - 64
        assert step == 32 * LC.km_geom(C)[2], (nxy, nt, step)


def test_the_table_of_the_design_document_is_the_generated_one():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert LC.table() in text, "DESIGN.md: regenerate the table with `python tests/layout_classes.py`"
