"""The launch hook of the segment labelling (tests/csrc/ofdis_launch_hooks_segments.hip): launch_label_segments of the TEST
library, whose GRID_MAX_BLOCKS a test lowers through launch_hooks.launch_limits so that every one of its grid-stride kernels
makes a second trip at test sizes.  libofdis_hip.so is a separate object: nothing here changes what it does."""
import numpy as np

import launch_hooks
from of_dis_amd import segments as S


def work_bytes(nmaps, w, h):
    return int(launch_hooks.hooks().ofdis_test_segments_work_bytes(nmaps, w, h))


def label_segments(gpu, label, flow, codes, conn, min_area, max_segments, records_fill):
    """launch_label_segments of the test library on the null stream -> (segments, records, info) as capi.label_segments"""
    nmaps, h, w = label.shape
    flow = np.ascontiguousarray(flow, np.float32) if flow is not None else None
    rshape = (nmaps, max_segments, S.SEG_RECORD_FIELDS)
    with gpu.DeviceCall() as c:
        launch_hooks.launch("label_segments", c.input(label), c.input(flow), nmaps, w, h, codes, conn, min_area, max_segments,
                            c.output((nmaps, h, w), np.int32), c.output(rshape, np.int64, fill=records_fill),
                            c.output((nmaps, S.SEG_INFO_FIELDS), np.int64), c.work(work_bytes(nmaps, w, h)))
        return c.results()
