"""CPU: the COCOTransform planner and the float64 restatement against the reference's own results (tests/golden/aug_*.npz,
tools/gen_golden_augment.py), and the restatement's power to tell plausible bugs apart."""
import json
import os

import numpy as np
import pytest
import torch

import augment_np as A
from conftest import GOLDEN, golden_files
from orienmask_amd import augment, transform

FIXTURES = golden_files("aug_")
# |device or float32 composition - float64 restatement| on the 0..255 scale before Normalize (DESIGN.md "Training augmentation")
PIXEL_BOUND = 1e-3
SEAM_EPS = 0.05          # degrees: taps whose float64 hue lies this close to 0/360 may flip across the seam
SEAM_ALLOWANCE = 0.02    # fraction of an image's pixels that may exceed PIXEL_BOUND, all of them seam pixels


def _json(x):
    return json.loads(json.dumps(x))


def _load(name):
    return A.load_fixture(os.path.join(GOLDEN, name))


def check_image(got, want, image, plan, what):
    """got / want: [3,H,W] normalised; the bound and the seam allowance on the 0..255 scale."""
    std = np.asarray(plan['std'], np.float64)[:, None, None]
    err = (np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) * std).max(axis=0)
    bad = err > PIXEL_BOUND
    if not bad.any():
        return 0
    seam = A.render_seam(image, plan, SEAM_EPS)
    assert seam is not None and not (bad & ~seam).any(), "%s: %d pixels off by up to %g outside the hue seam" % (
        what, int((bad & ~(seam if seam is not None else False)).sum()), float(err[bad & ~(seam if seam is not None else False)].max()))
    assert bad.sum() <= SEAM_ALLOWANCE * bad.size, "%s: %d seam pixels over the allowance" % (what, int(bad.sum()))
    return int(bad.sum())


def test_fixtures_exist_and_are_small():
    assert len(FIXTURES) >= 8
    for f in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 520 * 1024, f
    meta, samples, _ = _load("aug_orders.npz")
    _, planned, _ = A.plan_fixture(meta, samples)
    assert len({tuple(code for code, _ in p['aug']['ops']) for p in planned}) == 24       # every order of the four jitter ops


@pytest.mark.parametrize("name", FIXTURES)
def test_planner_reproduces_reference_draws_boxes_and_info(name):
    meta, samples, out = _load(name)
    draws, planned, _ = A.plan_fixture(meta, samples)
    assert _json(draws) == meta["draws"]
    pb = augment.collate(planned)
    assert pb.info is not None and _json([dict(i) for i in pb.info]) == meta["info"]
    bbox = torch.cat([p['bbox'] for p in planned]).numpy()
    cls = torch.cat([p['cls'] for p in planned]).numpy()
    assert bbox.dtype == np.float32 and cls.dtype == np.int64
    assert np.array_equal(bbox.view(np.uint32), out["bbox"].view(np.uint32))        # bit for bit
    assert np.array_equal(cls, out["cls"])
    lay = pb.layout
    meta_buf = pb.meta.numpy()
    index = meta_buf[lay["index"][0]:lay["index"][0] + lay["index"][1]].view(np.int64)
    assert np.array_equal(index, out["index"])
    assert list(out["image"].shape) == meta["out_shapes"]["image"] == [pb.B, 3] + list(pb.out_hw)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_call_log_and_pixels(name):
    meta, samples, out = _load(name)
    _, planned, _ = A.plan_fixture(meta, samples)
    log = []
    for s, p in zip(samples, planned):
        log += A.expected_cv2_log(p['aug'], True, len(s['mask']))
    assert log == meta["cv2"]
    first = 0
    for k, (s, p) in enumerate(zip(samples, planned)):
        want = A.render_image(s['image'], p['aug'])
        check_image(out["image"][k], want, s['image'], p['aug'], "%s image %d" % (name, k))
        n = len(s['mask'])
        masks = A.render_masks(np.stack(s['mask']) if n else np.zeros((0,) + s['image'].shape[:2], np.uint8), p['aug'])
        assert np.array_equal(masks, out["mask"][first:first + n]), "%s masks of image %d" % (name, k)
        first += n


MUTATIONS = ["image_edge", "hue_wrap", "nearest_float", "flip_before_pad", "no_mask_perm"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_restatement_catches_mutation(mut):
    """Each plausible bug changes some fixture's pixels (beyond the bound) or masks."""
    caught = []
    for name in FIXTURES:
        meta, samples, out = _load(name)
        _, planned, _ = A.plan_fixture(meta, samples)
        first = 0
        for k, (s, p) in enumerate(zip(samples, planned)):
            n = len(s['mask'])
            img = A.render_image(s['image'], p['aug'], mut=(mut,))
            std = np.asarray(p['aug']['std'], np.float64)[:, None, None]
            if (np.abs(img - out["image"][k]) * std).max() > 0.5:
                caught.append((name, k, "image"))
            if n:
                masks = A.render_masks(np.stack(s['mask']), p['aug'], mut=(mut,))
                if not np.array_equal(masks, out["mask"][first:first + n]):
                    caught.append((name, k, "mask"))
            first += n
    assert caught, "mutation %s is not caught by any fixture" % mut


def test_uint8_transport_is_exact_and_planning_identical():
    meta, samples, _ = _load("aug_train_a.npz")
    _, p8, _ = A.plan_fixture(meta, samples, transport_uint8=True)
    _, p32, _ = A.plan_fixture(meta, samples, transport_uint8=False)
    for a, b, s in zip(p8, p32, samples):
        assert a['image'].dtype == np.uint8 and b['image'].dtype == np.float32
        assert np.array_equal(a['image'].astype(np.float32), s['image'])
        assert np.array_equal(a['mask'], b['mask']) and torch.equal(a['bbox'], b['bbox'])
    assert augment.collate(p8).image.dtype == torch.uint8 and augment.collate(p32).image.dtype == torch.float32
    frac = dict(samples[0]); frac['image'] = samples[0]['image'] + np.float32(0.5)
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=meta["pipeline"]))
    assert tf(frac)['image'].dtype == np.float32            # not exactly uint8: stays float32


def test_collate_layout_and_zero_gt_batch():
    from orienmask_amd import synth
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=[dict(type="Resize", size=(32, 48), pad_needed=False),
                                                                        dict(type="ToTensor")]))
    batch = [tf(synth.synth_coco_sample(s, 20 + s, 30, 0)) for s in range(3)]
    pb = augment.collate(batch)
    assert pb.N == 0 and pb.B == 3 and pb.mask.numel() == 0 and pb.any_contrast is False
    rows = pb.meta.numpy()[:3 * augment.AUG_SAMPLE_DTYPE.itemsize].view(augment.AUG_SAMPLE_DTYPE)
    assert rows['image_off'].tolist() == [0, 20 * 30 * 3, 20 * 30 * 3 + 21 * 30 * 3]
    assert rows['n_ops'].tolist() == [0, 0, 0] and rows['scale_x'][0] == 1.0 / (48 / 30)
    for off, _ in pb.layout.values():
        assert off % 16 == 0
    import pickle
    assert pickle.loads(pickle.dumps(batch[0]))['aug']['out'] == (32, 48)


def test_unsupported_pipelines_raise():
    T = transform.COCOTransform
    with pytest.raises(NotImplementedError):
        T.ShortEdgeResize([544], 800)
    with pytest.raises(NotImplementedError):
        T.Pad(32)
    with pytest.raises(NotImplementedError):
        T.Resize((64, 64), pad_needed=True, pad_value=127.5)        # scalar pad on 3 channels: cv2's broadcast is not restated
    with pytest.raises(NotImplementedError):
        T.Resize((64, 64), interpolation='nearest')
    with pytest.raises(NotImplementedError):
        T([T.Resize((64, 64), pad_needed=False), T.ColorJitter(0.2), T.ToTensor()])      # out of order
    with pytest.raises(NotImplementedError):
        T([T.Resize((64, 64), pad_needed=False)])                                          # no ToTensor
    T.Resize((64, 64), pad_needed=False)                                                   # never pads: the scalar default is fine
    cfg = dict(type="COCOTransform", pipeline=[dict(type="ShortEdgeResize", short_length=[544], max_size=800), dict(type="ToTensor")])
    with pytest.raises(NotImplementedError):
        transform.build_transform(cfg)


def test_to_device_refuses_cpu():
    from orienmask_amd import lib, synth
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=[dict(type="Resize", size=(16, 16), pad_needed=False),
                                                                        dict(type="ToTensor")]))
    pb = transform.collate([tf(synth.synth_coco_sample(1, 10, 10, 1))])
    with pytest.raises(lib.OrienMaskHipError):
        transform.to_device(pb, "cpu")
