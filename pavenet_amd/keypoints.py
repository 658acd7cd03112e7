"""Left/right key-point permutations for horizontally flipped test-time augmentations
(opera/core/keypoint/transforms.py:157-192 kpt_flip / kpt_mapping_back).

Written from the public key-point orders:
* COCO (17): nose, left/right eye, left/right ear, left/right shoulder, left/right elbow, left/right wrist,
  left/right hip, left/right knee, left/right ankle;
* CrowdPose (14): left/right shoulder, left/right elbow, left/right wrist, left/right hip, left/right knee,
  left/right ankle, head, neck.
The reference picks the pairs by K alone (17 -> COCO, 14 -> CrowdPose) and raises NotImplementedError for any
other K, so its 15-point PoseTrack models cannot run flip TTA; neither can they here.
"""
COCO_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
CROWDPOSE_FLIP_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]


def flip_pairs(num_keypoints):
    """kpt_mapping_back's choice of pairs by K."""
    if num_keypoints == 17:
        return COCO_FLIP_PAIRS
    if num_keypoints == 14:
        return CROWDPOSE_FLIP_PAIRS
    raise NotImplementedError(f'flip test-time augmentation has left/right pairs for K = 17 (COCO) and K = 14 '
                              f'(CrowdPose) only, as the reference; got K = {num_keypoints}')


def flip_permutation(num_keypoints):
    """perm with flipped[k] = kpts[perm[k]] (every pair swapped, the rest in place)."""
    perm = list(range(num_keypoints))
    for a, b in flip_pairs(num_keypoints):
        perm[a], perm[b] = b, a
    return perm
