"""Detector (cosypose_amd/detector_trunk.py): a detector checkpoint's state dict and uint8 frames in, the `detections` collection out.
The float32 trunk is bit-equal to the twin's chained fmaf chains (tests/test_detector_trunk.py) and everything behind it is the same device
code on both sides, so this test checks the WIRING: the level order, the 'pool' level, the sizes and input_resize."""
import numpy as np
import pytest
import torch

import dettrunk_case as case
import dettrunk_ref as ref
from cosypose_amd import Detector, detections_from_frames
from cosypose_amd import detector_trunk as dt

pytestmark = pytest.mark.gpu
RESIZE = (48, 64)


def frames():
    rng = np.random.RandomState(31)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for h, w in case.E2E_FRAMES]


@pytest.fixture(scope='module')
def detector():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in case.detector_weights().items()}
    return Detector.from_state_dict(sd, case.E2E_LABELS, input_resize=RESIZE)


def both_ways(detector, fr, output_masks):
    seen = {}

    def twin_backbone(images):
        """the trunk's five maps computed by the twin from the very images detector_input made, and uploaded"""
        seen['shape'] = tuple(images.shape)
        return [torch.from_numpy(m).cuda() for m in ref.trunk32(case.trunk_net(), images.cpu().numpy())]
    options = dict(min_size=min(RESIZE), max_size=max(RESIZE), output_masks=output_masks, sizes=dt.ANCHOR_SIZES, aspect_ratios=dt.ASPECT_RATIOS)
    got = detector.get_detections(fr, output_masks=output_masks)
    with torch.no_grad():
        want = detections_from_frames(fr, twin_backbone, detector.heads.rpn_head, detector.heads.box_head, detector.heads.mask_head,
                                      detector.category_id_to_label, **options)
    print(f'{len(got)} detections, labels {sorted(set(got.infos["label"]))}, images {sorted(set(got.infos["batch_im_id"]))}, network input {seen["shape"]}')
    assert len(got) == len(want)
    assert got.infos['batch_im_id'].tolist() == want.infos['batch_im_id'].tolist() and got.infos['label'].tolist() == want.infos['label'].tolist()
    assert np.array_equal(got.infos['score'].values.astype(np.float32).view(np.int32), want.infos['score'].values.astype(np.float32).view(np.int32))
    assert torch.equal(got.bboxes.view(torch.int32), want.bboxes.view(torch.int32))
    assert hasattr(got, 'masks') == output_masks
    if output_masks:
        assert got.masks.dtype == torch.bool and got.masks.any() and torch.equal(got.masks, want.masks)
    return got, seen['shape']


def test_get_detections_equals_the_chain_fed_the_twins_trunk(detector):
    """the two frames of 37 x 53 and 45 x 40 as one batch: kept sets, labels, scores and boxes to the bit.  detections_from_heads pastes masks
    only for frames of one size, so the masks are compared on a second batch, of two 45 x 40 frames"""
    got, shape = both_ways(detector, frames(), False)
    assert shape == (2, 3, 64, 64)                                  # 37 x 53 -> 44 x 64, 45 x 40 -> 54 x 48, padded to multiples of 32
    assert len(got) > 3 and set(got.infos['batch_im_id']) == {0, 1}
    rng = np.random.RandomState(32)
    same = [torch.from_numpy(rng.randint(0, 256, (45, 40, 3)).astype(np.uint8)).cuda() for _ in range(2)]
    got, shape = both_ways(detector, same, True)
    assert shape == (2, 3, 64, 64) and len(got) > 3 and tuple(got.masks.shape[1:]) == (45, 40)


def test_the_interface_is_the_references(detector):
    channels_first = torch.stack([f[:37, :40] for f in frames()]).permute(0, 3, 1, 2)
    a = detector(channels_first.contiguous(), detection_th=0.3, one_instance_per_class=True)
    b = detector.get_detections(channels_first.permute(0, 2, 3, 1).contiguous(), detection_th=0.3, one_instance_per_class=True)
    assert not hasattr(a, 'masks') and len(a) == len(b) and (a.infos['score'] > 0.3).all() and a.infos['label'].is_unique
    assert torch.equal(a.bboxes, b.bboxes)
    with pytest.raises((ValueError, TypeError), match='uint8'):
        detector.get_detections([f.float() for f in frames()])
    with pytest.raises((ValueError, TypeError), match='uint8'):
        detector(torch.zeros(1, 3, 40, 40, device='cuda'))
