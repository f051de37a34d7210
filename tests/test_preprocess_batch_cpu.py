"""The host side of FastCOCOTransform.batch (om_preprocess_batch): the plan of a batch of images of their own sizes, the layout
of the staging buffer and the geometry table the entry takes.  Nothing here needs a GPU or the built library; the formulas are
written out again below (the reference's collate_plus / infer.pad arithmetic), not taken from the code under test."""
import math

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository on sys.path)
from orienmask_amd import lib as omlib
from orienmask_amd.transform import FastCOCOTransform as T, fill_stage, geom_rows, stage_layout

NORM = T.Normalize((123.675, 116.28, 103.53), (58.395, 57.12, 57.375))


def expected_plan(targets, divisor):
    H, W = max(t[0] for t in targets), max(t[1] for t in targets)
    if divisor:
        H, W = int(math.ceil(H / divisor) * divisor), int(math.ceil(W / divisor) * divisor)
    rows = []
    for rh, rw in targets:
        left, top = (W - rw) // 2, (H - rh) // 2
        right, down = W - rw - left, H - rh - top
        rows.append((rh, rw, top, left, [left, right, top, down, H, W]))
    return H, W, rows


def short_edge(h, w, short, longest):
    scale = min(short / min(h, w), longest / max(h, w))
    return int(h * scale + 0.5), int(w * scale + 0.5)


def check(tf, shapes, targets, divisor=32):
    H, W, rows = tf.plan_batch(shapes, size_divisor=divisor)
    eh, ew, erows = expected_plan(targets, divisor)
    assert (H, W) == (eh, ew)
    assert [(r.rh, r.rw, r.top, r.left, r.pad_info) for r in rows] == erows
    for r in rows:                      # the pads add up, the odd pixel goes right / down
        left, right, top, down, hh, ww = r.pad_info
        assert left + r.rw + right == ww == W and top + r.rh + down == hh == H
        assert right - left in (0, 1) and down - top in (0, 1)
    return H, W, rows


def test_plan_batch_single_square_image():
    _, _, rows = check(T([NORM]), [(544, 544)], [(544, 544)])
    assert rows[0].pad_info == [0, 0, 0, 0, 544, 544]


def test_plan_batch_fixed_resize_over_mixed_sizes():
    tf = T([T.Resize((544, 544)), NORM])
    shapes = [(480, 640), (333, 500), (1, 1), (1080, 1920)]
    _, _, rows = check(tf, shapes, [(544, 544)] * 4)
    assert all(r.pad_info == [0, 0, 0, 0, 544, 544] for r in rows)


def test_plan_batch_short_edge_resize_different_targets():
    tf = T([T.ShortEdgeResize(160, 256), NORM])
    shapes = [(120, 160), (160, 120), (97, 233)]
    targets = [short_edge(h, w, 160, 256) for h, w in shapes]
    assert targets == [(160, 213), (213, 160), (107, 256)]          # by hand: scales 4/3, 4/3 and 256/233
    H, W, rows = check(tf, shapes, targets)
    assert (H, W) == (224, 256)
    assert [r.pad_info for r in rows] == [[21, 22, 32, 32, 224, 256], [48, 48, 5, 6, 224, 256], [0, 0, 58, 59, 224, 256]]
    assert any(r.pad_info[0] != r.pad_info[1] for r in rows) and any(r.pad_info[2] != r.pad_info[3] for r in rows)


def test_plan_batch_without_divisor_and_without_resize():
    tf = T([T.ShortEdgeResize(160, 256), NORM])
    shapes = [(120, 160), (160, 120), (97, 233)]
    H, W, _ = check(tf, shapes, [short_edge(h, w, 160, 256) for h, w in shapes], divisor=0)
    assert (H, W) == (213, 256)
    H, W, rows = check(T([NORM]), [(37, 50), (64, 41)], [(37, 50), (64, 41)], divisor=0)      # no resize: its own size
    assert (H, W) == (64, 50) and rows[0].pad_info == [0, 0, 13, 14, 64, 50]


@pytest.mark.parametrize("pipeline,shape", [([T.Resize((544, 544))], (480, 640)), ([T.ShortEdgeResize(160, 256)], (600, 333)),
                                            ([], (97, 233)), ([T.Resize((100, 77))], (5, 13))])
@pytest.mark.parametrize("divisor", [32, 0])
def test_plan_batch_of_one_is_what_padded_reports(pipeline, shape, divisor):
    """`padded` computes its pad_info in _run, in front of the launch: the same arithmetic, written here as _run has it."""
    tf = T(list(pipeline) + [NORM])
    h, w = shape
    rh, rw = tf._resize.target(h, w) if tf._resize else (h, w)
    oh, ow = (int(math.ceil(rh / divisor) * divisor), int(math.ceil(rw / divisor) * divisor)) if divisor else (rh, rw)
    left, top = (ow - rw) // 2, (oh - rh) // 2
    H, W, rows = tf.plan_batch([shape], size_divisor=divisor)
    assert (H, W) == (oh, ow) and rows[0].pad_info == [left, ow - rw - left, top, oh - rh - top, oh, ow]
    assert (rows[0].rh, rows[0].rw, rows[0].top, rows[0].left) == (rh, rw, top, left)


def test_plan_batch_refuses_an_empty_list():
    with pytest.raises(ValueError):
        T([NORM]).plan_batch([])


def test_stage_layout_is_back_to_back_in_input_order():
    items = [(5, 13, 1), (7, 7, 1), (1, 1, 1), (240, 320, 1)]
    offsets, total = stage_layout(items)
    assert offsets == [0, 195, 195 + 147, 195 + 147 + 3] and total == 195 + 147 + 3 + 240 * 320 * 3
    assert any(o % 4 for o in offsets)                       # uint8 images start at any byte
    # float32 images begin at the next multiple of 4, everything else at the very next byte
    offsets, total = stage_layout([(5, 13, 1), (2, 3, 4), (1, 1, 1), (1, 1, 1), (1, 2, 4)])
    assert offsets == [0, 196, 268, 271, 276] and total == 276 + 24


def test_fill_stage_puts_mixed_dtypes_where_the_table_says():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (5, 13, 3), dtype=np.uint8)
    b = rng.random((2, 3, 3)).astype(np.float32)
    c = torch.from_numpy(rng.integers(0, 256, (3, 4, 3), dtype=np.uint8))
    d = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)[:, ::-1, ::-1]          # negative strides: cv2's BGR -> RGB view, mirrored
    e = torch.from_numpy(rng.random((6, 2, 3)).astype(np.float32)).permute(1, 0, 2)      # a host tensor that is not contiguous
    images = [a, b, c, d, e]
    offsets, total = stage_layout([tuple(im.shape[:2]) + (1 if str(im.dtype).endswith("uint8") else 4,) for im in images])
    assert offsets == [0, 196, 268, 304, 376] and total == 376 + 144
    buf = torch.full((total + 8,), 0xAB, dtype=torch.uint8)
    fill_stage(buf, images, offsets)
    raw = buf.numpy()
    used = np.zeros(total + 8, dtype=bool)
    for im, off in zip(images, offsets):
        want = np.ascontiguousarray(im.numpy() if isinstance(im, torch.Tensor) else im)
        got = raw[off:off + want.nbytes].view(want.dtype).reshape(want.shape)
        assert np.array_equal(got, want)
        assert off % want.itemsize == 0
        used[off:off + want.nbytes] = True
    assert (raw[~used] == 0xAB).all() and (~used[:total]).sum() <= 3 * 2       # only alignment gaps in front of the two float images


def test_geom_rows_and_flags():
    assert (omlib.OM_PRE_U8, omlib.OM_PRE_BGR, omlib.OM_PRE_BATCH) == (1, 2, 16)
    tf = T([T.ShortEdgeResize(160, 256), NORM])
    shapes = [(120, 160), (97, 233)]
    _, _, rows = tf.plan_batch(shapes)
    g = geom_rows(shapes, [True, False], rows, "bgr")
    assert g.dtype == np.int32 and g.shape == (2, 8) and g.flags["C_CONTIGUOUS"]
    # targets 160 x 213 and 107 x 256 in a 160 x 256 output: tops 0 and (160 - 107) // 2, lefts (256 - 213) // 2 and 0
    assert g.tolist() == [[120, 160, 160, 213, 0, 21, omlib.OM_PRE_U8 | omlib.OM_PRE_BGR, 0],
                          [97, 233, 107, 256, 26, 0, omlib.OM_PRE_BGR, 0]]
    g = geom_rows(shapes, [True, False], rows, "rgb")
    assert g[:, 6].tolist() == [omlib.OM_PRE_U8, 0] and g[:, 7].tolist() == [0, 0]


def test_batch_refuses_what_it_cannot_pack():
    from orienmask_amd.transform import _as_image
    with pytest.raises(TypeError):
        _as_image(np.zeros((4, 4, 3), dtype=np.float64), 0)
    with pytest.raises(ValueError):
        _as_image(np.zeros((4, 4), dtype=np.uint8), 1)
    with pytest.raises(TypeError):
        _as_image([[1, 2, 3]], 2)
    with pytest.raises(ValueError):
        T([NORM])._batch([np.zeros((4, 4, 3), dtype=np.uint8)], 32, 0, "grb", None)
