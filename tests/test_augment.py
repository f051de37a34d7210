"""GPU tests of the training / validation augmentation (om_augment, csrc/augment.hip; orienmask_amd.augment) against the float64
restatement (tests/augment_np.py) and the reference's own results (tests/golden/aug_*.npz)."""
import os

import numpy as np
import pytest
import torch

import augment_np as A
from conftest import ANCHOR_MASK, ANCHORS_YOLOV4, GOLDEN, golden_files, post_cfg
from test_augment_cpu import check_image
from orienmask_amd import augment, synth, transform

pytestmark = pytest.mark.gpu

FIXTURES = golden_files("aug_")
MEAN = [123.675, 116.280, 103.530]


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _planned(name, transport_uint8=True):
    meta, samples, out = A.load_fixture(os.path.join(GOLDEN, name))
    _, planned, _ = A.plan_fixture(meta, samples, transport_uint8)
    return meta, samples, out, planned


def _host(result):
    image, anno = result[0], result[1]
    return [image.cpu()] + [a.cpu() for a in anno]


def _train_pipeline(size, **resize):
    r = dict(type="Resize", size=list(size), pad_needed=True, warp_p=0.25, jitter=0.3, random_place=True, pad_p=0.75, pad_ratio=0.75,
             pad_value=MEAN)
    r.update(resize)
    return [dict(type="ColorJitter", brightness=0.2, contrast=0.5, saturation=0.5, hue=0.1),
            dict(type="RandomCrop", p=0.5, image_min_iou=0.64, bbox_min_iou=0.64), r, dict(type="RandomHorizontalFlip", p=0.5),
            dict(type="ToTensor"), dict(type="Normalize", mean=[0, 0, 0], std=[255, 255, 255])]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_images_masks_and_targets(dev, name):
    """Images within the stated bound of the float64 restatement (seam pixels counted against the allowance), for every fixture and
    every jitter order; masks bit-exact to the restatement and to the reference's fixture; bbox / cls / index bit-exact."""
    meta, samples, out, planned = _planned(name)
    res = transform.to_device(transform.collate(planned), dev)
    image, (bbox, cls, index, mask), info = res
    assert image.device == dev and mask.device == dev and bbox.device == dev and mask.dtype == torch.bool
    assert list(image.shape) == meta["out_shapes"]["image"] and list(mask.shape) == meta["out_shapes"]["mask"]
    image, mask = image.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(bbox.cpu().numpy().view(np.uint32), out["bbox"].view(np.uint32))
    assert torch.equal(cls.cpu(), torch.from_numpy(out["cls"])) and torch.equal(index.cpu(), torch.from_numpy(out["index"]))
    assert info == planned_info(planned)
    assert np.array_equal(mask, out["mask"])
    first = 0
    for k, (s, p) in enumerate(zip(samples, planned)):
        check_image(image[k], A.render_image(s['image'], p['aug']), s['image'], p['aug'], "%s image %d" % (name, k))
        n = len(s['mask'])
        if n:
            assert np.array_equal(mask[first:first + n], A.render_masks(np.stack(s['mask']), p['aug']))
        first += n


def planned_info(planned):
    return [p['info'] for p in planned]


def test_uint8_transport_bit_identical_to_float32(dev):
    for name in ("aug_train_a.npz", "aug_orders.npz", "aug_val.npz"):
        _, _, _, p8 = _planned(name, True)
        _, _, _, p32 = _planned(name, False)
        b8, b32 = transform.collate(p8), transform.collate(p32)
        assert b8.image.dtype == torch.uint8 and b32.image.dtype == torch.float32
        for a, b in zip(_host(transform.to_device(b8, dev)), _host(transform.to_device(b32, dev))):
            assert torch.equal(a, b), name


def test_mixed_batch_equals_per_sample_launches(dev):
    """Landscape, portrait and tiny sources, 0 / 1 / many GTs, in one launch set, against one launch set per sample; also at an
    output size whose mask plane is not a multiple of 16 bytes (the byte-store path)."""
    for size in ((64, 96), (15, 17)):
        tf = transform.build_transform(dict(type="COCOTransform", pipeline=_train_pipeline(size)))
        import random
        random.seed(5)
        torch.manual_seed(5)
        specs = [(1, 72, 104, 12, False), (2, 110, 60, 1, True), (3, 9, 7, 0, False), (4, 40, 50, 3, True), (5, 128, 192, 2, False)]
        planned = [tf(synth.synth_coco_sample(*s)) for s in specs]
        whole = _host(transform.to_device(transform.collate(planned), dev))
        first = 0
        for k, p in enumerate(planned):
            one = _host(transform.to_device(transform.collate([p]), dev))
            n = p['bbox'].shape[0]
            assert torch.equal(whole[0][k], one[0][0]), (size, k)
            assert torch.equal(whole[1][first:first + n], one[1]) and torch.equal(whole[2][first:first + n], one[2])
            assert torch.equal(whole[4][first:first + n], one[4]), (size, k)
            first += n
        src = [synth.synth_coco_sample(*s) for s in specs]
        first = 0
        for k, (s, p) in enumerate(zip(src, planned)):
            n = len(s['mask'])
            if n:
                assert np.array_equal(whole[4][first:first + n].numpy(), A.render_masks(np.stack(s['mask']), p['aug']))
            check_image(whole[0][k].numpy(), A.render_image(s['image'], p['aug']), s['image'], p['aug'], "mixed %s %d" % (size, k))
            first += n


def test_two_runs_bit_identical(dev):
    _, _, _, planned = _planned("aug_orders.npz")
    pb = transform.collate(planned)
    assert pb.any_contrast
    a = _host(transform.to_device(pb, dev))
    b = _host(transform.to_device(pb, dev))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_zero_gt_batch(dev):
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=_train_pipeline((32, 48))))
    planned = [tf(synth.synth_coco_sample(s, 30, 40, 0)) for s in range(3)]
    image, (bbox, cls, index, mask), info = transform.to_device(transform.collate(planned), dev)
    assert tuple(mask.shape) == (0, 32, 48) and mask.dtype == torch.bool and mask.device == dev
    assert tuple(bbox.shape) == (0, 4) and tuple(cls.shape) == (0,) and index.tolist() == [0, 0, 0, 0]
    assert tuple(image.shape) == (3, 3, 32, 48) and torch.isfinite(image).all()


def test_no_host_sync_and_dataloader(dev):
    """to_device does no D2H and no host synchronisation; device_batches over a DataLoader(collate_fn=collate, pin_memory=True)."""
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=_train_pipeline((64, 64))))
    samples = [synth.synth_coco_sample(s, 48 + s, 64, 4) for s in range(4)]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(samples)

        def __getitem__(self, i):
            return tf(dict(samples[i], mask=list(samples[i]['mask']), info=dict(samples[i]['info'])))

    loader = torch.utils.data.DataLoader(DS(), batch_size=2, num_workers=0, collate_fn=transform.collate, pin_memory=True)
    batches = list(loader)
    assert all(b.image.is_pinned() and b.meta.is_pinned() for b in batches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [transform.to_device(b, dev) for b in batches]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert [tuple(o[0].shape) for o in outs] == [(2, 3, 64, 64)] * 2
    again = list(transform.device_batches(batches, dev))
    for o, a in zip(outs, again):
        assert torch.equal(o[0], a[0]) and all(torch.equal(x, y) for x, y in zip(o[1], a[1]))


def test_feeds_training_loss_and_validate(dev):
    """to_device(collate(...)) goes into orienmask_amd.train.OrienMaskYOLOMultiScaleLoss (forward + backward) and tester.validate
    unchanged."""
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import validate
    from orienmask_amd.train import OrienMaskYOLOMultiScaleLoss
    H = W = 96
    cfg = dict(grid_size=[[H // 32, W // 32], [H // 16, W // 16], [H // 8, W // 8]], image_size=[H, W], anchors=ANCHORS_YOLOV4,
               anchor_mask=ANCHOR_MASK, num_classes=80, center_region=0.6, valid_region=0.6, label_smooth=False,
               obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20], scales_weight=[1, 1, 1])
    loss = OrienMaskYOLOMultiScaleLoss(**cfg)
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0), strict=True)
    net = net.to(dev)
    train_tf = transform.build_transform(dict(type="COCOTransform", pipeline=_train_pipeline((H, W))))
    image, target = transform.to_device(transform.collate([train_tf(synth.synth_coco_sample(s, 80, 100, 5, with_info=False))
                                                           for s in range(2)]), dev)
    with torch.no_grad():
        predict = net(image)
    leaves = [(b.detach().requires_grad_(), o.detach().requires_grad_()) for b, o in predict]
    loss_sum, loss_log, _ = loss(leaves, target, training=True)
    loss_sum.backward()
    assert torch.isfinite(loss_sum).item() and all(torch.isfinite(b.grad).all() and torch.isfinite(o.grad).all() for b, o in leaves)
    val_tf = transform.build_transform(dict(type="COCOTransform", pipeline=[
        dict(type="Resize", size=[H, W], pad_needed=False, warp_p=0., jitter=0., random_place=False, pad_p=0., pad_ratio=0.,
             pad_value=MEAN), dict(type="ToTensor"), dict(type="Normalize", mean=[0, 0, 0], std=[255, 255, 255])]))
    planned = [transform.collate([val_tf(synth.synth_coco_sample(10 * b + s, 70 + s, 90, 4, image_id=s)) for s in range(2)])
               for b in range(2)]
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((H, W)))
    from orienmask_amd.eval import OrienMaskYOLOMultiScaleLoss as ValLoss
    val = validate(net, ValLoss(**cfg), post, transform.device_batches(planned, dev))
    assert "val_loss" in val and np.isfinite(val["val_loss"])
