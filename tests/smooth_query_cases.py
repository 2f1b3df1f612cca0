"""Inputs of the query tests (tests/test_smooth_query_host.py, tests/test_gpu_track_smooth_query.py) -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

import smooth_cases as sc
import smooth_query_restated as sqr


def frames_of(ds, x_full):
    n0 = sc.ns(ds)
    return np.array(np.asarray(x_full)[n0:n0 + 6 * ds.num_frames]).reshape(ds.num_frames, 6)


def inserted(ds, x_full, frame_time, t):
    """The AUGMENTED problem of a query at t (not a frame time): a frame without detections inserted at t, at the pose the definition gives it
    (the geodesic between its neighbours, the end frame's pose outside the sequence).  Returns (data set, x_full, frame_time, its index)."""
    F = ds.num_frames
    times = sqr.times_of(F, frame_time)
    a, kind = sqr.locate(times, t)
    assert kind != "on"
    pos = a + 1
    z = frames_of(ds, x_full)
    zm = sqr.pose(z, times, t)
    n0 = sc.ns(ds)
    x = np.asarray(x_full)
    z2 = np.concatenate([z[:pos], zm[None, :], z[pos:]])
    frame = np.asarray(ds.obs_frame)
    out = sc.copy_of(ds, num_frames=F + 1, frame_ids=np.arange(F + 1, dtype=np.int32),
                     obs_frame=(frame + (frame >= pos)).astype(frame.dtype), x_full=np.concatenate([x[:n0], z2.reshape(-1), x[n0 + 6 * F:]]),
                     x_truth=None)
    return out, np.array(out.x_full), np.concatenate([times[:pos], [t], times[pos:]]), pos
