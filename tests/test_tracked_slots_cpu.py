"""The six numpy references restate DESIGN section 17 step 2 independently of each other.  On the script of
tests/tracked_cases.py they must leave the same id, frame and dropped after every frame, and the same last in every
live slot; the hand-made frames must do what the script's header says they do."""
import numpy as np
import pytest

from tests import tracked_cases as TC


def run(S):
    """-> per frame of the script, in order: (camera, {reference: shared state of that camera after the frame})."""
    refs = TC.references(S)
    trace = []
    for step in TC.script():
        for camera, kpts, bboxes, ids, keep in step:
            after = {}
            for name, ref, method in refs:
                getattr(ref, method)(kpts, bboxes, ids, keep=keep, camera=camera)
                after[name] = {k: np.array(v) for k, v in TC.shared(ref.state(camera)).items()}
            trace.append((camera, after))
    return trace


@pytest.mark.parametrize('S', [2, 4])
def test_the_references_agree_on_the_shared_rule(S):
    trace = run(S)
    assert len(trace) == 10 + 33
    for f, (camera, after) in enumerate(trace):
        want = after['ZoneRef']
        for name, got in after.items():
            for field in ('id', 'frame', 'dropped', 'last'):
                assert np.array_equal(got[field], want[field]), (f, camera, name, field)


@pytest.mark.parametrize('S', [2, 4])
def test_the_script_does_what_it_says(S):
    trace = run(S)
    cam0 = [after['ZoneRef'] for camera, after in trace[:10] if camera == 0]
    cam1 = [after['ZoneRef'] for camera, after in trace[:10] if camera == 1]

    def ids(st):
        return st['id'].tolist()
    assert ids(cam0[0])[:2] == [1, 2] and cam0[0]['dropped'] == 0          # the second copy of id 1; 0 and -1 stay out
    if S == 2:
        assert ids(cam0[1]) == [1, 2] and cam0[1]['dropped'] == 2          # ids 3 and 4 find no slot; 5 and 6 take no part
        assert ids(cam0[3]) == [1, 2] and cam0[3]['last'].tolist() == [3, 4] and cam0[3]['dropped'] == 7
        assert ids(cam1[3]) == [5, 6] and cam1[3]['last'].tolist() == [4, 3] and cam1[3]['dropped'] == 4
    else:
        assert ids(cam0[1]) == [1, 2, 3, 4] and cam0[1]['dropped'] == 0
        assert ids(cam0[3]) == [1, 2, 3, 4] and cam0[3]['last'].tolist() == [3, 4, 4, 2] and cam0[3]['dropped'] == 4
        assert ids(cam1[3]) == [5, 6, 7, 8] and cam1[3]['dropped'] == 2
    assert cam0[2]['last'].tolist()[0] == 3 and cam0[2]['dropped'] == cam0[1]['dropped']   # id 1 at max_age: no birth
    assert ids(cam0[4]) == [1, 2, 3, 0][:S] and cam0[4]['frame'] == 5      # an empty frame: the clock; id 4 expires
    assert ids(cam1[0])[:2] == [5, 6] and cam1[2]['last'].tolist()[1] == 3                  # id 6 at max_age
    last = {camera: after['ZoneRef'] for camera, after in trace}
    assert last[0]['frame'] == 6 + 17 and last[1]['frame'] == 4 + 16
    assert last[0]['dropped'] > cam0[5]['dropped'] and last[1]['dropped'] > cam1[3]['dropped']   # the random frames drop
