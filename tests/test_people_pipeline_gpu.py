"""GPU: MultiViewPipeline.process_people — the 2D stage per person box, association, gathering and
triangulation are exactly the calls it is documented to make, on 3 frames x 2 views with two person
slots whose order is swapped between the views."""
import numpy as np
import pytest
import torch

from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
T, V, P = 3, 2, 2
ASSOC = dict(max_cost_px=2000.0, trunc_px=1e4)      # seeded random weights: the skeletons of two views never agree
MIN_CONF = -1e30                                    # ... and their heatmap maxima may be negative


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import hrnet, ops, pipeline
    from mvpose.estimator import BatchPoseEstimator
    cams = syn.make_rig(V, seed=3)
    est = BatchPoseEstimator(hrnet.random_state_dict(5), max_frames=5)      # 11 rows: chunks of 5, 5 and 1
    p = pipeline.MultiViewPipeline(syn.reference_camera_params(cams), estimator=est, mode=ops.TRI_ROBUST,
                                   inlier_px=1e4, min_conf=MIN_CONF, refine="heatmap")
    frames = torch.from_numpy(syn.make_skeleton_frames(T * V, seed=12)[0]).cuda().reshape(T, V, 720, 1280, 3)
    rng = np.random.default_rng(4)
    left = np.array([100.0, 80.0, 560.0, 640.0]) + rng.uniform(-30, 30, (T, V, 4))
    right = np.array([700.0, 60.0, 1180.0, 660.0]) + rng.uniform(-30, 30, (T, V, 4))
    boxes = np.stack([left, right], 2)                                     # (T, V, P, 4)
    boxes[:, 1] = boxes[:, 1, ::-1]                                        # view 1 lists them the other way round
    boxes[1, 0, 1] = np.nan                                                # an empty slot
    return p, est, frames, boxes


def test_process_people_is_its_documented_calls(setup):
    from mvpose import ops, people
    p, est, frames, boxes = setup
    out = p.process_people(frames, bboxes=boxes, **ASSOC)
    k = out["kpts_2d_people"]
    assert tuple(k.shape) == (T, P, 17, 3, V) and k.dtype == torch.float32
    # the 2D stage on the non-empty (camera-frame, slot) rows, in that order, in chunks of max_frames
    flat = frames.reshape(T * V, 720, 1280, 3)
    fb = boxes.reshape(T * V, P, 4)
    rows = [(f, s) for f in range(T * V) for s in range(P) if np.isfinite(fb[f, s]).all()]
    assert len(rows) == 11
    want = torch.full((T * V, P, 17, 3), float("nan"), device="cuda")
    want_g = torch.full((T * V, P, 17, 6), float("nan"), dtype=torch.float64, device="cuda")
    for i in range(0, len(rows), est.max_frames):
        chunk = rows[i:i + est.max_frames]
        f = torch.tensor([r[0] for r in chunk], device="cuda")
        r = est.run(flat.index_select(0, f), bboxes=np.stack([fb[a, b] for a, b in chunk]))
        for n, (a, b) in enumerate(chunk):
            want[a, b, :, :2], want[a, b, :, 2] = r["keypoints"][n], r["scores"][n]
            want_g[a, b] = r["gaussians"][n]
    want = want.reshape(T, V, P, 17, 3).permute(0, 2, 3, 4, 1)
    assert torch.equal(_bits(k), _bits(want))
    assert torch.equal(_bits(out["heatmaps_2d_people"]), _bits(want_g.reshape(T, V, P, 17, 6)))
    assert torch.isnan(k[1, 1, :, :, 0]).all() and torch.isfinite(k[1, 0, :, :, 0]).all()
    # association, gathering and triangulation are the ops calls on those keypoints
    g, c, _, _ = ops.associate_views(k, p.cams, p.camera_indices, min_conf=p.min_conf, **ASSOC)
    assert torch.equal(out["people_group"], g) and torch.equal(out["people_count"], c)
    print("groups", g.cpu().tolist(), "counts", c.cpu().tolist(), "lowest score", float(k[:, :, :, 2].nan_to_num(9.0).min()))
    assert tuple(g.shape) == (T, V, P) and (g[1, 0].cpu().tolist()[1] == -1) and int(c[:, 1].min()) >= 1
    k2, g2, dropped = people.gather_groups(k, g, p.camera_indices, P, gauss=out["heatmaps_2d_people"])
    assert torch.equal(_bits(out["kpts_2d"]), _bits(k2)) and torch.equal(_bits(out["heatmaps_2d"]), _bits(g2))
    assert tuple(k2.shape) == (T, P, 17, 3, V) and tuple(g2.shape) == (T, P, V, 17, 6) and not dropped.any()
    xyz, inl, err = ops.triangulate_robust(k2, p.cams, p.camera_indices, inlier_px=p.inlier_px, min_conf=p.min_conf)
    assert torch.equal(_bits(out["kpts_3d_seed"]), _bits(xyz)) and torch.equal(out["tri_inliers"], inl)
    assert torch.equal(_bits(out["tri_reproj_err"]), _bits(err))
    assert tuple(xyz.shape) == (T, P, 17, 3) and torch.isfinite(xyz).any()
    rx, cov, cost, status = ops.triangulate_refine(
        k2.reshape(T * P, 17, 3, V), p.cams, p.camera_indices, xyz.reshape(T * P, 17, 3), weights="heatmap",
        gauss=g2.reshape(T * P, V, 17, 6), mask=inl.reshape(T * P, 17, V), min_conf=p.min_conf, cov_floor=p.cov_floor)
    assert torch.equal(_bits(out["kpts_3d"]), _bits(rx.reshape(T, P, 17, 3)))
    assert torch.equal(_bits(out["kpts_3d_cov"]), _bits(cov.reshape(T, P, 17, 3, 3)))
    assert torch.equal(out["tri_refine_status"], status.reshape(T, P, 17))
    # fewer groups than slots asked for: the second group is dropped and counted
    one = p.process_people(frames, bboxes=boxes, max_groups=1, **ASSOC)
    assert tuple(one["kpts_3d"].shape) == (T, 1, 17, 3)
    assert torch.equal(_bits(one["kpts_3d_seed"]), _bits(xyz[:, :1]))
    assert torch.equal(one["people_dropped"], (c[:, 0].long() - 1).clamp(min=0))
    with pytest.raises(ValueError):
        p.process_people(frames)                              # no boxes and no detector
    with pytest.raises(ValueError):
        p.process_people(frames, bboxes=boxes[:, :, 0])


def test_process_people_with_the_detector(setup):
    """bboxes=None takes each camera-frame's first max_people NMS detections above bbox_thr: the
    same outputs as handing over those boxes, read from nms()."""
    from mvpose import pipeline, rtmdet
    p0, est, frames, _ = setup
    det = rtmdet.RTMDetector(rtmdet.peaked_state_dict(), max_batch=4)
    cams = syn.make_rig(V, seed=3)
    p = pipeline.MultiViewPipeline(syn.reference_camera_params(cams), estimator=est, detector=det, inlier_px=1e4)
    flat = frames.reshape(T * V, 720, 1280, 3)
    boxes = np.full((T * V, P, 4), np.nan)
    for i in range(0, T * V, det.max_batch):
        for n, d in enumerate(det.nms(det.detect(flat[i:i + det.max_batch]))):
            d = d[:P][d[:P, 4] > p.bbox_thr]
            boxes[i + n, :len(d)] = d[:, :4]
    assert np.isfinite(boxes[:, 0]).all()                     # the peaked detector finds the rendered person
    a = p.process_people(frames, max_people=P, **ASSOC)
    b = p.process_people(frames, bboxes=boxes.reshape(T, V, P, 4), **ASSOC)
    assert sorted(a) == sorted(b)
    for key in a:
        x, y = a[key], b[key]
        assert torch.equal(_bits(x), _bits(y)) if x.is_floating_point() else torch.equal(x, y), key
    det.close()
