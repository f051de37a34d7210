"""om_preprocess_batch, FastCOCOTransform.batch and infer_loop(batch_size=B) on the GPU.

The comparator is always the existing float path on ONE image alone:
    expected[i] = full(pad_value);  expected[i][:, top:top+rh, left:left+rw] = tf(float32_rgb(image_i)[None])[0]
compared with torch.equal.  om_preprocess itself is pinned against the reference's fixtures and the float64 sweep
(tests/test_hip_parity.py, tests/test_geometry_sweep.py), so equality transfers both pins to the batched kernel."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import post_cfg
from orienmask_amd import lib as omlib, synth
from orienmask_amd.transform import FastCOCOTransform as T, STAGE_RING

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PAD = 0.5
KINDS = ("u8_rgb", "u8_bgr", "f32")


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _tf(*resize):
    return T(list(resize) + [T.Normalize(MEAN, STD)])


def _photo(seed, h, w, kind):
    """A numpy [h,w,3] image: uint8, or float32 with fractional values in [0, 255]."""
    rng = np.random.default_rng(seed)
    if kind == "f32":
        return (rng.random((h, w, 3)) * 255).astype(np.float32)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _float_rgb(image, order):
    """What the host conversion in front of the float path makes of an image: float32, RGB."""
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else image
    a = a.astype(np.float32)
    return np.ascontiguousarray(a[:, :, ::-1] if order == "bgr" else a)


def _expected(tf, images, order, rows, H, W, dev, pad_value=PAD):
    out = torch.full((len(images), 3, H, W), pad_value, dtype=torch.float32, device=dev)
    for i, (im, r) in enumerate(zip(images, rows)):
        alone = tf(torch.from_numpy(_float_rgb(im, order)).to(dev)[None])[0]
        assert tuple(alone.shape) == (3, r.rh, r.rw)
        out[i, :, r.top:r.top + r.rh, r.left:r.left + r.rw] = alone
    return out


GEOMETRIES = {
    "1x1_to_32x32": ((1, 1), (T.Resize((32, 32)),)),
    "7x7_to_5x9_small_blend": ((7, 7), (T.Resize((5, 9)),)),
    "5x13_to_64x96_upscale": ((5, 13), (T.Resize((64, 96)),)),
    "240x320_to_544x544": ((240, 320), (T.Resize((544, 544)),)),
    "600x333_short_edge": ((600, 333), (T.ShortEdgeResize(160, 256),)),
    "37x50_no_resize": ((37, 50), ()),
}


@pytest.mark.parametrize("divisor", [32, 0])            # 0: out_w = the resized width (9, 89, 50: the scalar store path)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_geometry_table(dev, name, kind, divisor):
    (h, w), resize = GEOMETRIES[name]
    tf = _tf(*resize)
    order = "bgr" if kind == "u8_bgr" else "rgb"
    image = _photo(sum(map(ord, name)), h, w, kind)
    H, W, rows = tf.plan_batch([(h, w)], divisor)
    want = _expected(tf, [image], order, rows, H, W, dev)
    for src in (image, torch.from_numpy(image).to(dev)):             # through the staging buffer, and read in place
        x, pads = tf.batch([src], size_divisor=divisor, pad_value=PAD, channel_order=order, device=dev)
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, H, W) and pads == [rows[0].pad_info]
        assert torch.equal(x, want), name
    if kind == "u8_rgb":                                             # __call__ and padded take uint8 [n,h,w,3] device tensors
        pair = torch.from_numpy(np.stack([image, image[::-1].copy()])).to(dev)
        both, pad_info = tf.padded(pair, divisor, PAD) if divisor else (tf(pair), None)
        ref, ref_info = tf.padded(pair.float(), divisor, PAD) if divisor else (tf(pair.float()), None)
        assert torch.equal(both, ref) and pad_info == ref_info


def test_mixed_call_of_nineteen_images(dev):
    """More than OM_PRE_BATCH images (two launches), five sizes, both element types, host and device images in one call."""
    assert 19 > omlib.OM_PRE_BATCH
    tf = _tf(T.ShortEdgeResize(160, 256))
    sizes = [(120, 160), (160, 120), (97, 233), (600, 333), (31, 17)]
    images = [_photo(100 + i, *sizes[i % 5], "f32" if i % 3 == 1 else "u8") for i in range(19)]
    given = [torch.from_numpy(im).to(dev) if i % 4 == 2 else (torch.from_numpy(im) if i % 4 == 3 else im)
             for i, im in enumerate(images)]
    H, W, rows = tf.plan_batch([im.shape[:2] for im in images])
    assert len({(r.rh, r.rw) for r in rows}) == 5 and any(r.pad_info[0] != r.pad_info[1] for r in rows)
    for order in ("rgb", "bgr"):
        x, pads = tf.batch(given, pad_value=PAD, channel_order=order)
        assert tuple(x.shape) == (19, 3, H, W) and pads == [r.pad_info for r in rows]
        want = _expected(tf, images, order, rows, H, W, dev)
        for i in range(19):
            assert torch.equal(x[i], want[i]), (order, i)


def test_uint8_images_at_any_byte_address(dev):
    """Device views that start at byte offsets 1, 2 and 3 (mod 4) of one buffer, back to back, the last ending exactly at the
    buffer's end: the same results as the images in allocations of their own."""
    tf = _tf(T.Resize((64, 96)))
    shapes = [(3, 5), (7, 9), (5, 13)]                  # 45, 189 and 195 bytes: starts 1, 46 and 235
    images = [_photo(200 + i, h, w, "u8") for i, (h, w) in enumerate(shapes)]
    offsets, off = [], 1
    for im in images:
        offsets.append(off)
        off += im.size
    total = off
    assert [o % 4 for o in offsets] == [1, 2, 3]
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    views = []
    for im, o in zip(images, offsets):
        buf[o:o + im.size] = torch.from_numpy(im).reshape(-1).to(dev)
        views.append(buf[o:o + im.size].view(*im.shape))
    assert views[2].data_ptr() + images[2].size == buf.data_ptr() + buf.numel()
    assert [(v.data_ptr() - buf.data_ptr()) % 4 for v in views] == [1, 2, 3]
    for order in ("rgb", "bgr"):
        got, _ = tf.batch(views, pad_value=PAD, channel_order=order)
        aligned, _ = tf.batch([torch.from_numpy(im).to(dev) for im in images], pad_value=PAD, channel_order=order)
        H, W, rows = tf.plan_batch(shapes)
        assert torch.equal(got, aligned) and torch.equal(got, _expected(tf, images, order, rows, H, W, dev))


def test_host_inputs_and_the_staging_ring(dev):
    tf = _tf(T.ShortEdgeResize(160, 256))
    sizes = [(120, 160), (97, 233), (31, 17)]

    def make(seed):
        return [_photo(seed + i, *sizes[i], "f32" if i == 1 else "u8") for i in range(3)]

    images = make(300)
    on_device, pads = tf.batch([torch.from_numpy(im).to(dev) for im in images], pad_value=PAD, channel_order="bgr")
    from_numpy, pads_n = tf.batch(images, pad_value=PAD, channel_order="bgr", device=dev)
    from_host, pads_h = tf.batch([torch.from_numpy(im) for im in images], pad_value=PAD, channel_order="bgr", device=dev)
    strided = [np.ascontiguousarray(im[:, ::-1])[:, ::-1] for im in images]        # the same values behind negative strides
    from_views, _ = tf.batch(strided, pad_value=PAD, channel_order="bgr", device=dev)
    assert torch.equal(from_numpy, on_device) and torch.equal(from_host, on_device) and torch.equal(from_views, on_device)
    assert pads == pads_n == pads_h
    # more calls back to back than the ring has buffers, different images each, no synchronise in between: each its own result
    sets = [make(400 + 10 * k) for k in range(STAGE_RING + 2)]
    torch.cuda.synchronize(dev)
    outs = [tf.batch(s, pad_value=PAD, device=dev)[0] for s in sets]
    H, W, rows = tf.plan_batch(sizes)
    for s, x in zip(sets, outs):
        assert torch.equal(x, _expected(tf, s, "rgb", rows, H, W, dev))
    assert sum(slot is not None for slot in tf._ring) == STAGE_RING and all(slot[0].is_pinned() for slot in tf._ring)
    buffers = [slot[0].data_ptr() for slot in tf._ring]
    tf.batch(sets[0], pad_value=PAD, device=dev)
    assert [slot[0].data_ptr() for slot in tf._ring] == buffers                    # no pinned allocation per call


def test_refusals_name_the_image(dev):
    a = torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev)
    out = torch.full((2, 3, 32, 32), 7.0, device=dev)
    mean, std = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), a.data_ptr())
    good = [8, 8, 16, 16, 8, 8, omlib.OM_PRE_U8, 0]

    def call(rows, n=2, images=ptrs):
        geom = np.asarray(rows, dtype=np.int32)
        omlib.launch("om_preprocess_batch", dev, images, geom.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, mean, std, 32, 32,
                     0.0, out)

    call([good, good])
    for bad, what in (([8, 8, 16, 16, 17, 8, 1, 0], "does not fit"), ([8, 8, 16, 40, 0, 0, 1, 0], "does not fit"),
                      ([8, 8, 16, 16, 8, -1, 1, 0], "does not fit"), ([8, 8, 16, 16, 8, 8, 1 | 4, 0], "unknown flag"),
                      ([8, 8, 16, 16, 8, 8, 1, 9], "unknown flag"), ([8, 0, 16, 16, 8, 8, 1, 0], "bad shape")):
        out.fill_(7.0)
        with pytest.raises(omlib.OrienMaskHipError, match=r"image 1: .*%s" % what):
            call([good, bad])
        assert bool((out == 7.0).all())                 # a refused call launches nothing, the good first row included
    with pytest.raises(omlib.OrienMaskHipError, match="image 1: null pointer"):
        call([good, good], images=(ctypes.c_void_p * 2)(a.data_ptr(), None))
    with pytest.raises(omlib.OrienMaskHipError, match="n = 0"):
        call([good, good], n=0)
    with pytest.raises(omlib.OrienMaskHipError, match="null argument"):
        omlib.launch("om_preprocess_batch", dev, ptrs, None, 2, mean, std, 32, 32, 0.0, out)
    f = torch.zeros(8 * 8 * 3 + 1, dtype=torch.float32, device=dev)
    with pytest.raises(omlib.OrienMaskHipError, match="image 0: a float32 image must be 4-byte aligned"):
        call([[8, 8, 16, 16, 8, 8, 0, 0]], n=1, images=(ctypes.c_void_p * 1)(f.data_ptr() + 2))


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("bbox", "cls", "mask"))


def test_batched_infer_loop(dev):
    """infer_loop(batch_size=4) over five uint8 BGR numpy photos of three sizes: the detections of postprocess(model(x)) on the
    same two groups assembled from the float path, per image in input order."""
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import infer_loop
    sd = synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0)          # the weights of test_tester_and_infer_loops
    net = OrienMaskYOLOFPNPlus(3, 80).eval().set_precision("f32")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((544, 544)))
    tf = T([T.Resize((544, 544)), T.Normalize((0, 0, 0), (255, 255, 255))])
    sizes = [(240, 320), (256, 320), (272, 320), (240, 320), (256, 320)]
    photos = [synth.synth_photo_batch(900 + i, 1, h, w)[0] for i, (h, w) in enumerate(sizes)]       # float32 RGB, integer values
    bgr = [np.ascontiguousarray(p.numpy().astype(np.uint8)[:, :, ::-1]) for p in photos]
    want = []
    with torch.no_grad():
        for group in (photos[:4], photos[4:]):
            x = torch.cat([tf.padded(p.to(dev)[None])[0] for p in group], 0)
            want += [{k: v.clone() for k, v in d.items()} for d in post(net(x))]
    print("detections per image:", [int(d["bbox"].shape[0]) for d in want])
    assert sum(int(d["bbox"].shape[0]) for d in want) > 0
    cells = getattr(net, "latency_cells", None)
    dets, pads, log = infer_loop(net, tf, post, bgr, dev, warmup=1, batch_size=4, channel_order="bgr")
    assert len(dets) == 5 and all(_same(a, b) for a, b in zip(dets, want))
    assert pads == [[0, 0, 0, 0, 544, 544]] * 5
    assert set(log) == {"Main Loop", "Load data", "Forward & Postprocess"}
    assert getattr(net, "latency_cells", None) == cells
    seen = []

    def visualizer(det, image, pad_info):
        seen.append(image)
        return len(seen)

    dets_e, pads_e, log_e, shows = infer_loop(net, tf, post, bgr, dev, warmup=0, use_graph=False, batch_size=4, channel_order="bgr",
                                              visualizer=visualizer)
    assert all(_same(a, b) for a, b in zip(dets_e, want)) and pads_e == pads and shows == [1, 2, 3, 4, 5]
    assert set(log_e) == {"Main Loop", "Load data", "Forward & Postprocess", "Visualize"}
    for image, p in zip(seen, photos):                  # float32 RGB on the device, as the one-image loop hands it over
        assert image.is_cuda and image.dtype == torch.float32 and torch.equal(image.cpu(), p)
    # batch_size=1 with float32 images: the loop as it was
    dets_1, pads_1, log_1 = infer_loop(net, tf, post, photos, dev, warmup=1, batch_size=1)
    assert set(log_1) == {"Main Loop", "Load data", "Forward & Postprocess"} and pads_1 == pads
    with torch.no_grad():
        for p, d in zip(photos, dets_1):
            again = post(net(tf.padded(p.to(dev)[None])[0]))[0]
            assert _same(again, d)
