"""``opera.VideoPoseV1`` (L6): backbone -> neck -> head, ``simple_test`` restated from
opera/models/detectors/videoposev1.py:18-190 and mmdet SingleStageDetector.extract_feat
(third_party/mmdetection/mmdet/models/detectors/single_stage.py:47).

Native additions: ``forward_device`` keeps the whole clip batch on the device and returns
fixed-shape result tensors (no host sync); B >= 1 clips per call (the reference asserts B = 1,
videoposev1.py:175-177).

Test-time augmentation (videoposev1.py:192-261, petr.py:118-187): ``aug_test`` / ``aug_test_device`` run one
``forward_device`` per augmentation and merge the results with box NMS in one launch (``ops.aug_merge_nms``);
``forward`` dispatches an augmentation list of more than one entry to ``aug_test`` as mmdet's
``BaseDetector.forward_test`` does.
"""
import numpy as np
import torch

from .bricks import BaseModule, batch_invariant_scope
from .registry import DETECTORS, MMDET_MODELS


def bbox_kpt2result(bboxes, labels, kpts, num_classes):
    """opera/core/keypoint/transforms.py:132-154."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)], \
            [np.zeros((0, kpts.size(1), 3), dtype=np.float32) for _ in range(num_classes)]
    if isinstance(bboxes, torch.Tensor):
        bboxes = bboxes.detach().cpu().numpy()
        labels = labels.detach().cpu().numpy()
        kpts = kpts.detach().cpu().numpy()
    return [bboxes[labels == i, :] for i in range(num_classes)], \
        [kpts[labels == i, :, :] for i in range(num_classes)]


@DETECTORS.register_module()
class VideoPoseV1(BaseModule):

    # bricks.set_batch_invariant: every output of a clip a function of that clip's input and canvas only
    batch_invariant = False

    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None):
        super().__init__(init_cfg)
        backbone = dict(backbone)
        if pretrained:
            backbone['pretrained'] = pretrained
        # the reference detectors derive from mmdet's SingleStageDetector, whose __init__ builds
        # its parts through mmdet's registry (single_stage.py:29-38): bare names such as
        # 'HRNet' resolve in the mmdet scope, 'opera.X' walks up to the root and down again
        self.backbone = MMDET_MODELS.build(backbone)
        self.neck = MMDET_MODELS.build(neck) if neck is not None else None
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg)
        bbox_head.update(test_cfg=test_cfg)
        self.bbox_head = MMDET_MODELS.build(bbox_head)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg

    @property
    def with_neck(self):
        return self.neck is not None

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def extract_feats(self, imgs):
        """mmdet BaseDetector.extract_feats: one feature pyramid per augmentation."""
        return [self.extract_feat(img) for img in imgs]

    @torch.no_grad()
    def forward_device(self, img, img_metas, rescale=False, force_score_topk=None, strict=False,
                       **head_kwargs):
        """img [B, T, 3, H, W] on the device; img_metas: one dict per clip.  Returns the
        head's fixed-shape device result dict (see VideoPoseHeadMulFrames.get_bboxes).

        Frame-sharded multi-GPU: pass ``frame_shard=FrameShard(T, rank, world)`` and only the
        rank's frames, img [B, T_loc, 3, H, W] (frames t with t % world == rank, in order).

        strict=True: the forward runs under ``census.LaunchCensus`` (after one un-counted warm-up of these
        shapes, which builds the per-shape constant tables) and raises ``census.FallbackError`` if a torch /
        vendor compute operator (GEMM, convolution, attention, normalisation, pooling, ...) ran on a device
        tensor, i.e. if a module-level gate dropped off the hand-written path; the census of the last strict
        call stays in ``self.last_census``."""
        if strict:
            from .census import LaunchCensus
            key = (tuple(img.shape), str(img.device),
                   tuple((tuple(m['batch_input_shape']), tuple(m['img_shape'][:2])) for m in img_metas),
                   bool(rescale), force_score_topk is not None, tuple(sorted(head_kwargs)))
            warm = self.__dict__.setdefault('_strict_warm', set())
            if key not in warm:
                self.forward_device(img, img_metas, rescale=rescale, force_score_topk=force_score_topk,
                                    **head_kwargs)
                warm.add(key)
            with LaunchCensus(where=strict == 'where') as census:    # strict='where': record the call sites too
                res = self.forward_device(img, img_metas, rescale=rescale, force_score_topk=force_score_topk,
                                          **head_kwargs)
            self.last_census = census
            census.raise_on_fallback(f'{type(self).__name__}.forward_device(strict=True)')
            return res
        if self.batch_invariant and head_kwargs.get('frame_shard') is not None:
            raise NotImplementedError('batch-invariant inference (set_batch_invariant) does not cover frame_shard=')
        with batch_invariant_scope(self):
            feat = self.extract_feat(img)
            head_kwargs.setdefault('last_level_only', True)   # get_bboxes reads [-1] only
            outs = self.bbox_head(feat, img_metas, **head_kwargs)
            return self.bbox_head.get_bboxes(outs, img_metas, rescale=rescale,
                                             force_score_topk=force_score_topk)

    @torch.no_grad()
    def simple_test(self, img, img_metas, rescale=False):
        """videoposev1.py:159-190 -> per clip (bbox_results, kpt_results) lists of numpy arrays."""
        res = self.forward_device(img, img_metas, rescale=rescale)
        results_list = self.bbox_head.results_to_list(res)
        return [bbox_kpt2result(b, l, k, self.bbox_head.num_classes) for b, l, k in results_list]

    def _tta_cfg(self):
        cfg = self.test_cfg if self.test_cfg is not None else {}
        missing = [k for k in ('nms', 'score_thr', 'max_per_img') if cfg.get(k) is None]
        if missing:
            raise ValueError(f'test-time augmentation needs test_cfg.{missing[0]} (missing: {", ".join(missing)}); '
                             "the reference's flip-test config sets score_thr=0.0, max_per_img=100, "
                             "nms=dict(type='soft_nms', iou_thr=0.5)")
        return cfg

    @torch.no_grad()
    def aug_test_device(self, imgs, img_metas, strict=False, force_topk_proposals=None, force_score_topk=None):
        """imgs / img_metas: one entry per augmentation (mmdet's nesting: img_metas[a] is the list of per-image
        metas), every augmentation with the same B >= 1 images -> fixed-shape device dict: bboxes [B, M, 5]
        (soft-NMS decayed scores), labels [B, M], kpts [B, M, K, 3] (score channel 1), keep [B, M] int32,
        inds [B, M] (rows of the concatenated per-augmentation results), count [B]; results in original-image
        pixels.  force_*: one entry (or None) per augmentation, passed to that augmentation's forward_device.

        strict=True: each augmentation's forward runs strict (forward_device), and the merge runs under a census
        too (``self.last_merge_census``): it must issue no ATen launch and no host sync."""
        from . import ops
        from .keypoints import flip_permutation
        from .tta import aug_meta, parse_nms_cfg
        A = len(imgs)
        if A == 0 or len(img_metas) != A:
            raise ValueError('aug_test: one img_metas entry per augmentation')
        cfg = self._tta_cfg()
        method, iou_thr, sigma, min_score, offset = parse_nms_cfg(cfg['nms'])
        perm = flip_permutation(self.bbox_head.num_keypoints)
        metas = [aug_meta(m) for m in img_metas]
        fp = force_topk_proposals if force_topk_proposals is not None else [None] * A
        fs = force_score_topk if force_score_topk is not None else [None] * A
        results = []
        for a in range(A):
            kw = {} if fp[a] is None else dict(force_topk_proposals=fp[a])
            results.append(self.forward_device(imgs[a], img_metas[a], rescale=False, force_score_topk=fs[a],
                                               strict=strict, **kw))

        def merge():
            return ops.aug_merge_nms([r['bboxes'] for r in results], [r['kpts'] for r in results],
                                     [r['keep'] for r in results], [m[0] for m in metas], [m[1] for m in metas],
                                     [m[2] for m in metas], perm, score_thr=float(cfg['score_thr']),
                                     max_num=int(cfg['max_per_img']), method=method, iou_thr=iou_thr,
                                     sigma=sigma, min_score=min_score, offset=offset)
        if not strict:
            m = merge()
        else:
            from .census import FallbackError, LaunchCensus
            with LaunchCensus() as census:
                m = merge()
            self.last_merge_census = census
            s = census.summary()
            if s['fallback_ops'] or s['aten_launches'] or s['host_syncs']:
                raise FallbackError(f'{type(self).__name__}.aug_test_device(strict=True): the merge ran ATen '
                                    f'operators on the device: {s}')
        return dict(bboxes=m['dets'], labels=m['labels'], kpts=m['kpts'], keep=m['keep'], inds=m['inds'],
                    count=m['count'])

    @torch.no_grad()
    def aug_test(self, imgs, img_metas, rescale=False):
        """videoposev1.py:225-261 / petr.py:151-187 -> per image (bbox_results, kpt_results); results are in
        original-image pixels whatever `rescale` says, as in the reference."""
        res = self.aug_test_device(imgs, img_metas)
        results_list = self.bbox_head.results_to_list(res)
        return [bbox_kpt2result(b, l, k, self.bbox_head.num_classes) for b, l, k in results_list]

    def show_result(self, img, result, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241),
                    mask_color=None, thickness=4, font_size=10, win_name='', show=False, wait_time=0, out_file=None,
                    **style):
        """videoposev1.py:263-350 / petr.py:189 on the device (``render.show_result``): a drawn copy of the [H, W, 3]
        uint8 BGR `img` with the poses and boxes of `result` (one image's entry of ``simple_test``), hard-edged and
        without text; show=True / out_file= raise NotImplementedError.  **style: radius, kpt_thr, skeleton."""
        from .render import show_result
        return show_result(self, img, result, score_thr=score_thr, bbox_color=bbox_color, text_color=text_color,
                           mask_color=mask_color, thickness=thickness, font_size=font_size, win_name=win_name,
                           show=show, wait_time=wait_time, out_file=out_file, **style)

    def forward(self, img, img_metas, return_loss=False, rescale=False, **kwargs):
        if return_loss:
            raise NotImplementedError('pavenet_amd is a forward (inference) path')
        if isinstance(img, (list, tuple)):  # mmdet forward_test nests one level per augmentation
            if len(img) > 1:   # mmdet BaseDetector.forward_test (base.py:114-156): several augmentations
                return self.aug_test(list(img), list(img_metas), rescale=rescale)
            img, img_metas = img[0], img_metas[0]
        return self.simple_test(img, img_metas, rescale=rescale)
