"""CPU: of_dis_amd/segments.py: label_segments_ref, the numpy statement of include/ofdis.h's section "Segments", on maps whose
results are written out by hand, its records against direct numpy sums, its flow handling, and its numbering against
scipy.ndimage.label where scipy is installed.  The device call against this model: tests/test_gpu_segments.py."""
import numpy as np
import pytest

from of_dis_amd import capi, segments as S

_f32 = np.float32


def _map(text):
    """rows of digits -> uint8 [h, w]"""
    return np.array([[int(ch) for ch in row] for row in text.split()], np.uint8)


def _seg(label, **kw):
    kw.setdefault("codes", 1 << 1)
    kw.setdefault("max_segments", 8)
    seg, rec, info = S.label_segments_ref(label, **kw)
    return seg[0], rec[0], info[0]


def test_the_constants_are_the_bindings():
    for name in ("SEG_MAX_SEGMENTS", "SEG_RECORD_FIELDS", "SEG_INFO_FIELDS", "SEG_MOVING"):
        assert getattr(S, name) == getattr(capi, name), name
    assert (S.SEG_MAX_SEGMENTS, S.SEG_RECORD_FIELDS, S.SEG_INFO_FIELDS, S.SEG_MOVING) == (1 << 24, 12, 4, 2)


def test_the_model_does_not_import_scipy():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(S))
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
        [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert names and not any("scipy" in n for n in names), names


def test_two_blobs_touching_only_diagonally():
    m = _map("""1100
                1100
                0011
                0011""")
    seg, rec, info = _seg(m, conn=8)
    assert info.tolist() == [1, 1, 1, 8]
    assert (seg == (m == 1)).all()
    assert rec[0].tolist() == [8, 0, 0, 0, 3, 3, 12, 12, 0, 0, 0, 0]
    seg, rec, info = _seg(m, conn=4)
    assert info.tolist() == [2, 2, 2, 8]
    assert seg.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 2, 2], [0, 0, 2, 2]]
    assert rec[0].tolist() == [4, 0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0]
    assert rec[1].tolist() == [4, 10, 2, 2, 3, 3, 10, 10, 0, 0, 0, 0]


def test_a_u_shape_is_one_component_numbered_from_its_first_arm():
    m = _map("""10001
                10001
                11111""")
    for conn in (4, 8):
        seg, rec, info = _seg(m, conn=conn)
        assert info.tolist() == [1, 1, 1, 9]
        assert (seg == m).all()
        assert rec[0].tolist() == [9, 0, 0, 0, 4, 2, 0 + 4 + 0 + 4 + 10, 0 + 0 + 1 + 1 + 10, 0, 0, 0, 0]


def test_a_ring_with_a_blob_inside():
    m = _map("""11111
                10001
                10101
                10001
                11111""")
    for conn in (4, 8):
        seg, rec, info = _seg(m, conn=conn)
        assert info.tolist() == [2, 2, 2, 17]
        want = m.astype(np.int32)
        want[2, 2] = 2
        assert (seg == want).all()
        assert rec[0, :6].tolist() == [16, 0, 0, 0, 4, 4] and rec[1].tolist() == [1, 12, 2, 2, 2, 2, 2, 2, 0, 0, 0, 0]


def test_min_area_removes_the_first_component_and_the_numbers_shift():
    m = _map("""10110
                00110
                00001""")
    seg, rec, info = _seg(m, conn=4, min_area=2)
    assert info.tolist() == [3, 1, 1, 6]
    assert seg.tolist() == [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0]]
    assert rec[0].tolist() == [4, 2, 2, 0, 3, 1, 10, 2, 0, 0, 0, 0]
    for min_area in (0, 1):   # max(min_area, 1): both keep everything
        seg, rec, info = _seg(m, conn=4, min_area=min_area)
        assert info.tolist() == [3, 3, 3, 6]
        assert seg.tolist() == [[1, 0, 2, 2, 0], [0, 0, 2, 2, 0], [0, 0, 0, 0, 3]]
    seg, rec, info = _seg(m, conn=8, min_area=2)   # the corner pixel joins the block
    assert info.tolist() == [2, 1, 1, 6]
    assert seg.tolist() == [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 1]]
    seg, rec, info = _seg(m, conn=8, min_area=100)
    assert info.tolist() == [2, 0, 0, 6] and not seg.any() and not rec.any()


def test_max_segments_below_nkept_numbers_all_and_records_the_first():
    m = _map("10101 00000 10101")
    fill = np.full((1, 2, 12), -7, np.int64)
    seg, rec, info = S.label_segments_ref(m[None], codes=2, conn=8, max_segments=2, records_fill=fill)
    assert info[0].tolist() == [6, 6, 2, 6]
    assert seg[0].tolist() == [[1, 0, 2, 0, 3], [0, 0, 0, 0, 0], [4, 0, 5, 0, 6]]
    assert rec[0, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] and rec[0, 1].tolist() == [1, 2, 2, 0, 2, 0, 2, 0, 0, 0, 0, 0]
    seg, rec, info = S.label_segments_ref(m[None], codes=2, conn=8, max_segments=8, records_fill=np.full((1, 8, 12), -7, np.int64))
    assert info[0].tolist() == [6, 6, 6, 6] and (rec[0, 6:] == -7).all() and (rec[0, :6, 0] == 1).all()


def test_bytes_of_8_or_more_are_never_foreground():
    m = np.array([[0, 8, 9, 255, 16, 7, 128, 1]], np.uint8)
    seg, rec, info = _seg(m, codes=0xFF, conn=4)
    assert seg.tolist() == [[1, 0, 0, 0, 0, 2, 0, 3]] and info.tolist() == [3, 3, 3, 3]
    seg, rec, info = _seg(m, codes=1 << 7, conn=4)
    assert seg.tolist() == [[0, 0, 0, 0, 0, 1, 0, 0]]


def test_codes_with_two_bits_set():
    m = _map("0120 2100 0002")
    seg, rec, info = _seg(m, codes=(1 << 1) | (1 << 2), conn=4)
    assert seg.tolist() == [[0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 2]] and info.tolist() == [2, 2, 2, 5]
    seg, rec, info = _seg(m, codes=1 << 2, conn=4)
    assert seg.tolist() == [[0, 0, 1, 0], [2, 0, 0, 0], [0, 0, 0, 3]]
    seg, rec, info = _seg(m, codes=1 << 0, conn=8)   # the zeros: the corner pixel alone, the other six joined by a diagonal
    assert info.tolist() == [2, 2, 2, 7] and rec[:2, 0].tolist() == [1, 6]


def test_rejected_arguments_raise():
    m = np.zeros((1, 2, 2), np.uint8)
    for kw in (dict(codes=0), dict(codes=0x100), dict(conn=6), dict(min_area=-1), dict(max_segments=0),
               dict(max_segments=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            S.label_segments_ref(m, **kw)


def test_records_against_direct_sums():
    rng = np.random.default_rng(5)
    label = (rng.random((2, 23, 41)) < 0.55).astype(np.uint8)
    flow = (rng.standard_normal((2, 23, 41, 2)) * 5).astype(_f32)
    seg, rec, info = S.label_segments_ref(label, flow, codes=2, conn=4, min_area=3, max_segments=500)
    assert (info[:, 1] < info[:, 0]).all() and (info[:, 1] >= 5).all() and (info[:, 2] == info[:, 1]).all()
    ys, xs = np.mgrid[0:23, 0:41]
    for m in range(2):
        assert info[m, 3] == label[m].sum() and seg[m].max() == info[m, 1]
        q = np.rint(flow[m] * _f32(256.0)).astype(np.int64)
        for k in range(1, int(info[m, 1]) + 1):
            on = seg[m] == k
            assert on.sum() >= 3
            want = [on.sum(), np.flatnonzero(on)[0], xs[on].min(), ys[on].min(), xs[on].max(), ys[on].max(), xs[on].sum(), ys[on].sum(),
                    on.sum(), q[..., 0][on].sum(), q[..., 1][on].sum(), 0]
            assert rec[m, k - 1].tolist() == [int(v) for v in want], (m, k)
        assert not rec[m, info[m, 1]:].any()
        roots = rec[m, :info[m, 1], 1]
        assert (np.diff(roots) > 0).all()


def test_flow_nan_infinity_and_out_of_range_are_left_out_of_nflow():
    label = np.ones((1, 1, 8), np.uint8)
    above = np.nextafter(_f32(4096.0), _f32(np.inf))
    flow = np.zeros((1, 1, 8, 2), _f32)
    flow[0, 0, :, 0] = [1.0, np.nan, np.inf, -np.inf, 4096.0, above, -4096.0, 0.501953125]
    flow[0, 0, :, 1] = [2.0, 0.0, 0.0, 0.0, -above, 0.0, 0.25, np.nan]
    seg, rec, info = S.label_segments_ref(label, flow, codes=2, conn=4, max_segments=1)
    # usable: pixels 0 and 6 (4096 itself is usable, the next float is not; a NaN in either component takes the pixel out)
    assert rec[0, 0].tolist() == [8, 0, 0, 0, 7, 0, 28, 0, 2, 256 - 4096 * 256, 512 + 64, 0]
    # rintf rounds to nearest even: 0.501953125 * 256 = 128.5 -> 128; 0.505859375 * 256 = 129.5 -> 130
    flow[0, 0, :, 1] = 0.0
    flow[0, 0, :, 0] = [0.501953125, 0.505859375, -0.501953125, 0, 0, 0, 0, 0]
    seg, rec, info = S.label_segments_ref(label, flow, codes=2, conn=4, max_segments=1)
    assert rec[0, 0, 8:11].tolist() == [8, 128 + 130 - 128, 0]
    # without flow the three are 0
    assert S.label_segments_ref(label, None, codes=2, conn=4, max_segments=1)[1][0, 0, 8:].tolist() == [0, 0, 0, 0]


def test_one_map_as_a_2d_array_and_maps_do_not_interact():
    rng = np.random.default_rng(9)
    label = (rng.random((3, 9, 17)) < 0.5).astype(np.uint8)
    all3 = S.label_segments_ref(label, codes=2, conn=8, max_segments=64)
    for m in range(3):
        one = S.label_segments_ref(label[m], codes=2, conn=8, max_segments=64)
        for a, b in zip(all3, one):
            assert (a[m] == b[0]).all()


@pytest.mark.parametrize("density", [0.1, 0.5, 0.6, 0.9])
@pytest.mark.parametrize("conn", [4, 8])
def test_the_numbering_is_scipys(conn, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 10) + conn)
    label = (rng.random((1, 70, 300)) < density).astype(np.uint8)
    seg, _, info = S.label_segments_ref(label, codes=2, conn=conn, max_segments=1)
    structure = np.ones((3, 3), int) if conn == 8 else ndimage.generate_binary_structure(2, 1)
    want, n = ndimage.label(label[0], structure)
    assert n == info[0, 0] == info[0, 1] and (seg[0] == want).all()


def test_work_bytes_formula():
    assert S.segments_work_bytes(1, 1, 1) == 8 + 16
    assert S.segments_work_bytes(3, 64, 16) == 3 * (8 * 1024 + 16 * 4)
    assert S.segments_work_bytes(1, 300, 70) == 8 * 21000 + 16 * 83
    assert S.segments_work_bytes(1, 8193, 1) == 0 and S.segments_work_bytes(0, 4, 4) == 0
