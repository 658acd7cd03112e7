"""The rule the six analytics that follow track ids share (csrc/pave_tracked.h), on the
device: the frames of tests/tracked_cases.py go to a PoseSmoother, a ZoneMonitor without zones, a PostureMonitor, a
FootfallMap, a TrackTrails and a GroundPlane (an identity plane whose bounds hold every anchor, so that "placed" is
"takes part") with equal max_tracks, max_age and thresholds.  After every step id, frame and dropped of every camera
are torch.equal across the six and equal to the numpy reference, and so is last in the live slots.  The last step is one
update_many of 33 frames: a camera's frames on both sides of the 32-entry launch split.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import tracked_cases as TC

pytestmark = pytest.mark.gpu

FIELDS = ('id', 'frame', 'dropped', 'last')


def analytics(S):
    from pavenet_amd import FootfallMap, GroundPlane, PoseSmoother, PostureMonitor, TrackTrails, ZoneMonitor
    kw = dict(cameras=TC.CAMERAS, max_tracks=S, max_age=TC.MAX_AGE, score_thr=TC.SCORE_THR)
    plane = GroundPlane(TC.K, **kw)
    for c in range(TC.CAMERAS):
        plane.set_plane(c, matrix=np.eye(3))
    return [('PoseSmoother', PoseSmoother(TC.K, **kw), 'smooth_many'),
            ('ZoneMonitor', ZoneMonitor(TC.K, **kw), 'update_many'),
            ('PostureMonitor', PostureMonitor(TC.K, **kw), 'update_many'),
            ('FootfallMap', FootfallMap(TC.K, TC.SIZE, **kw), 'update_many'),
            ('TrackTrails', TrackTrails(TC.K, length=4, **kw), 'update_many'), ('GroundPlane', plane, 'update_many')]


def item(camera, kpts, bboxes, ids, keep):
    """A frame of the script as a (camera, result, ids) item: the tuple form, or the dict form when it has a keep."""
    kp, bb = torch.from_numpy(kpts).cuda(), torch.from_numpy(bboxes).cuda()
    result = (bb, None, kp) if keep is None else dict(bboxes=bb, kpts=kp, keep=torch.from_numpy(keep).cuda())
    return camera, result, torch.from_numpy(ids).cuda()


@pytest.mark.parametrize('S', [2, 4])
def test_one_slot_rule_on_the_device(S):
    devs, refs = analytics(S), TC.references(S)
    zone_ref = dict((name, ref) for name, ref, _ in refs)['ZoneRef']
    steps = TC.script()
    assert [len(s) for s in steps] == [1] * 10 + [33]
    for n, step in enumerate(steps):
        for camera, kpts, bboxes, ids, keep in step:
            for _, ref, method in refs:
                getattr(ref, method)(kpts, bboxes, ids, keep=keep, camera=camera)
        items = [item(*frame) for frame in step]
        for name, dev, method in devs:
            outs = getattr(dev, method)(items)
            assert len(outs) == len(items), (n, name)
        for c in range(TC.CAMERAS):
            want = {k: torch.from_numpy(np.array(v)) for k, v in TC.shared(zone_ref.state(c)).items()}
            first = None
            for name, dev, _ in devs:
                got = TC.shared(dev.state(c))
                for field in FIELDS:
                    g = got[field]
                    assert g.is_cuda and g.dtype == torch.int32 and g.shape == want[field].shape, (n, c, name, field)
                    assert torch.equal(g.cpu(), want[field]), \
                        f'step {n} camera {c} {name} {field}: {g.cpu().tolist()} for {want[field].tolist()}'
                    if first is not None:
                        assert torch.equal(g, first[field]), (n, c, name, field)
                first = first or got
    for c in range(TC.CAMERAS):      # the script got where it was meant to: both launches of the last step ran
        assert int(devs[0][1].state(c)['frame']) == (23, 20)[c] and int(devs[0][1].state(c)['dropped']) > 0
