"""InferenceVisualizer (orienmask_amd/visualizer.py, csrc/visualize.hip) against fixtures made by the reference's own
utils/visualizer.py (tools/gen_golden_vis.py, tests/golden/vis_*.npz)."""
import contextlib
import ctypes
import hashlib
import inspect
import io
import json
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files

VIS_FILES = golden_files("vis_")
NEAR_HALF = 2e-3


class RecordingCV2(types.ModuleType):
    """The cv2 stand-in tools/gen_golden_vis.py ran the reference under: drawing calls are recorded and do nothing;
    getTextSize is a fixed function of the text."""
    FONT_HERSHEY_DUPLEX = 2
    LINE_AA = 16

    def __init__(self):
        super().__init__("cv2")
        self.log = []

    def _rec(self, name, args, kwargs):
        self.log.append([name, [a if not isinstance(a, np.ndarray) else "image" for a in args], dict(kwargs)])

    def rectangle(self, *args, **kwargs):
        self._rec("rectangle", args, kwargs)

    def putText(self, *args, **kwargs):
        self._rec("putText", args, kwargs)

    def getTextSize(self, *args, **kwargs):
        self._rec("getTextSize", args, kwargs)
        text = args[0]
        return (6 * len(text) + 1, 9 + len(text) % 3), 3


def _load(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


def _case(g, device):
    """(detections, image, pad_info, constructor kwargs) of a fixture, on `device`."""
    from orienmask_amd import synth
    K, Hn, Wn = (int(v) for v in g["mask_shape"])
    masks = np.unpackbits(g["mask_bits"], axis=1)[:, :Hn * Wn].reshape(K, Hn, Wn).astype(bool)
    h, w = (int(v) for v in g["size"])
    image = synth.synth_photo_batch(int(g["photo_seed"]), 1, h, w)[0]
    dets = dict(bbox=torch.from_numpy(g["bbox"]).to(device), cls=torch.from_numpy(g["cls"]).to(device),
                mask=torch.from_numpy(masks).to(device))
    return dets, image.to(device), [int(v) for v in g["pad_info"]], json.loads(str(g["ctor"]))


def _near_half(g):
    h, w = (int(v) for v in g["size"])
    return np.unpackbits(g["near_half_bits"])[:h * w * 3].reshape(h, w, 3).astype(bool)


def _check_u8(got, want, near, tag):
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    bad = (diff > 0) & ~near
    assert not bad.any(), "%s: %d pixels differ away from a rounding boundary (first at %s)" % (
        tag, int(bad.sum()), np.argwhere(bad)[0].tolist())
    assert diff.max() <= 1, tag


def _rect_calls(log):
    return [c for c in log if c[0] == "rectangle" and c[2].get("thickness") is not None]


def _paint_outlines(img, log):
    """cv2.rectangle(..., thickness=1) of each recorded outline call, clipped to the image, in call order."""
    out = img.copy()
    h, w = out.shape[:2]
    on = np.zeros((h, w), dtype=bool)
    for _, args, _ in _rect_calls(log):
        (x1, y1), (x2, y2), color = args[1], args[2], args[3]
        xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        m = np.zeros((h, w), dtype=bool)
        cx0, cx1 = max(xa, 0), min(xb, w - 1)
        cy0, cy1 = max(ya, 0), min(yb, h - 1)
        for y in (y1, y2):
            if 0 <= y < h and cx0 <= cx1:
                m[y, cx0:cx1 + 1] = True
        for x in (x1, x2):
            if 0 <= x < w and cy0 <= cy1:
                m[cy0:cy1 + 1, x] = True
        out[m] = np.array(color, dtype=np.float64).round().astype(np.uint8)
        on |= m
    return out, on


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_fixtures_present():
    assert {"vis_vga.npz", "vis_letterbox.npz", "vis_small.npz", "vis_none.npz", "vis_nomask.npz", "vis_overlap.npz"} <= set(VIS_FILES)


def test_signature_mirrors_reference():
    from orienmask_amd.visualizer import InferenceVisualizer
    ref = json.loads(str(_load("vis_vga.npz")["signature"]))
    ours = list(inspect.signature(InferenceVisualizer.__init__).parameters)
    assert ours == ref + ["draw"]
    defaults = {k: p.default for k, p in inspect.signature(InferenceVisualizer.__init__).parameters.items()}
    assert (defaults["with_mask"], defaults["conf_thresh"], defaults["alpha"], defaults["line_thickness"]) == (True, 0.3, 0.5, 1)


def test_registry_builds_reference_config():
    """config/base.py:259-267 (coco_visualizer) through builder.build, unchanged; building touches no device."""
    from orienmask_amd import builder, visualizer
    cfg = dict(type="InferenceVisualizer", dataset="COCO", with_mask=True, conf_thresh=0.3, alpha=0.6, line_thickness=1)
    v = builder.build(cfg, visualizer, device=torch.device("cuda", 0))
    assert isinstance(v, visualizer.InferenceVisualizer)
    assert (v.with_mask, v.conf_thresh, v.alpha, v.line_thickness, v.draw) == (True, 0.3, 0.6, 1, "auto")
    assert v.classes[0] == "person" and len(v.classes) == 80
    assert cfg["type"] == "InferenceVisualizer"


def test_tables_match_reference():
    from orienmask_amd.visualizer import CLASSES, PALETTE, CAT2LABEL
    blob = json.dumps({"classes": {k: list(v) for k, v in sorted(CLASSES.items())}, "palette": [list(p) for p in PALETTE]})
    for name in VIS_FILES:
        assert hashlib.sha1(blob.encode()).hexdigest() == str(_load(name)["tables_sha1"]), name
    assert len(CAT2LABEL["COCO"]) == 80 and len(CAT2LABEL["VOC"]) == 20


def test_constructor_rejects_what_it_cannot_do():
    from orienmask_amd import lib
    from orienmask_amd.visualizer import InferenceVisualizer
    with pytest.raises(lib.OrienMaskHipError):
        InferenceVisualizer("COCO", "cpu")
    with pytest.raises(ValueError):
        InferenceVisualizer("COCO", "cuda", line_thickness=2, draw="device")
    with pytest.raises(ValueError):
        InferenceVisualizer("COCO", "cuda", draw="matplotlib")
    InferenceVisualizer("VOC", "cuda", line_thickness=2, draw="cv2")


@pytest.mark.parametrize("name", VIS_FILES)
def test_recover_shape_bbox_cpu(name):
    """The classmethod on CPU tensors gives the rectangle corners the reference passed to cv2."""
    from orienmask_amd.visualizer import InferenceVisualizer
    g = _load(name)
    ctor = json.loads(str(g["ctor"]))
    bbox = torch.from_numpy(g["bbox"])
    kept = bbox[bbox[:, -1] > ctor["conf_thresh"]]
    h, w = (int(v) for v in g["size"])
    want = [[a[1][0], a[1][1], a[2][0], a[2][1]] for _, a, _ in _rect_calls(json.loads(str(g["calls"])))]
    got = InferenceVisualizer._recover_shape_bbox(kept[:, :4], w, h, [int(v) for v in g["pad_info"]])
    assert got.dtype == torch.int64
    assert got.tolist() == want


def test_vis_image_struct_size():
    from orienmask_amd import lib
    assert ctypes.sizeof(lib.VisImage) == 7 * 8 + 12 * 4          # seven pointers, eleven int32 and a float


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev(built):
    from orienmask_amd import lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def fake_cv2(monkeypatch):
    cv2 = RecordingCV2()
    monkeypatch.setitem(sys.modules, "cv2", cv2)
    return cv2


def _run(v, dets, image, pad, seed):
    random.seed(seed)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = v(dets, image, pad)
    return out, buf.getvalue().splitlines()


@pytest.mark.gpu
@pytest.mark.parametrize("name", VIS_FILES)
def test_parity_with_reference(dev, fake_cv2, name):
    from orienmask_amd.visualizer import InferenceVisualizer
    g = _load(name)
    dets, image, pad, ctor = _case(g, dev)
    v = InferenceVisualizer(device=dev, **ctor)
    before = image.clone()
    out, lines = _run(v, dets, image, pad, int(g["rand_seed"]))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == tuple(image.shape)
    near = _near_half(g)
    _check_u8(out, g["result"], near, name)
    assert json.loads(json.dumps(fake_cv2.log)) == json.loads(str(g["calls"])), name      # tuples as the fixture's JSON lists
    assert lines == json.loads(str(g["stdout"])), name
    assert torch.equal(image, before)
    if "float_residual" in g:
        random.seed(int(g["rand_seed"]))
        _, f = v._composite_float(dets, image, pad)
        want = g["result"].astype(np.float32) + g["float_residual"].astype(np.float32)
        err = np.abs(f.cpu().numpy() - want).max()
        assert err < NEAR_HALF, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vis_vga.npz", "vis_letterbox.npz", "vis_overlap.npz"])
def test_device_outlines(dev, name):
    """draw='device': the fixture's image with the recorded thickness-1 rectangles painted on it (later boxes win)."""
    from orienmask_amd.visualizer import InferenceVisualizer
    g = _load(name)
    dets, image, pad, ctor = _case(g, dev)
    v = InferenceVisualizer(device=dev, draw="device", **ctor)
    out, lines = _run(v, dets, image, pad, int(g["rand_seed"]))
    want, on = _paint_outlines(g["result"], json.loads(str(g["calls"])))
    assert on.any()
    _check_u8(out, want, _near_half(g) & ~on[:, :, None], name)
    assert lines == json.loads(str(g["stdout"]))


@pytest.mark.gpu
def test_batch_equals_single_calls(dev):
    from orienmask_amd.visualizer import InferenceVisualizer
    cases = [_case(_load(n), dev) for n in ("vis_small.npz", "vis_letterbox.npz", "vis_overlap.npz")]
    v = InferenceVisualizer("COCO", dev, alpha=0.6)
    random.seed(5)
    batch = v.composite([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    random.seed(5)
    single = [v.composite([c[0]], [c[1]], [c[2]])[0] for c in cases]
    assert [tuple(b.shape) for b in batch] == [tuple(c[1].shape) for c in cases]
    for b, s in zip(batch, single):
        assert b.dtype == torch.uint8 and torch.equal(b, s)


@pytest.mark.gpu
def test_alpha_zero_and_nothing_kept_round_the_image(dev, fake_cv2):
    from orienmask_amd.visualizer import InferenceVisualizer
    g = _load("vis_letterbox.npz")
    dets, image, pad, ctor = _case(g, dev)
    image = image + 0.49 * torch.rand(image.shape, generator=torch.Generator().manual_seed(3)).to(dev)   # fractional, < 255.5
    image[0, :4, 0] = torch.tensor([0.5, 1.5, 2.5, 254.5], device=dev)                          # ties: half to even
    want = image.round().to(torch.uint8).cpu().numpy()
    before = image.clone()
    out, _ = _run(InferenceVisualizer(device=dev, **dict(ctor, alpha=0.0)), dets, image, pad, 1)
    assert np.array_equal(out, want)
    n_calls = len(fake_cv2.log)
    out2, lines = _run(InferenceVisualizer(device=dev, **dict(ctor, conf_thresh=1.0)), dets, image, pad, 1)
    assert np.array_equal(out2, want) and lines == [] and len(fake_cv2.log) == n_calls       # nothing kept: nothing drawn
    assert torch.equal(image, before)


@pytest.mark.gpu
def test_1080p_full_masks_memory(dev, fake_cv2):
    """K=100 full-image masks on a 1080 x 1920 photo: the reference's formulation needs > 2.5 GB of temporaries."""
    from orienmask_amd import synth
    from orienmask_amd.visualizer import InferenceVisualizer
    K = 100
    image = synth.synth_photo_batch(3, 1, 1080, 1920)[0].to(dev)
    g = torch.Generator().manual_seed(0)
    bbox = torch.cat([torch.rand(K, 4, generator=g) * 0.5 + 0.25, torch.rand(K, 1, generator=g) * 0.6 + 0.35], 1).to(dev)
    dets = dict(bbox=bbox, cls=torch.arange(K, device=dev) % 80, mask=torch.ones(K, 544, 544, dtype=torch.bool, device=dev))
    v = InferenceVisualizer("COCO", dev, alpha=0.6)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out, lines = _run(v, dets, image, [0, 0, 0, 0, 544, 544], 2)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(dev) - base
    assert grew < 64 << 20, grew
    assert len(lines) == K and out.shape == (1080, 1920, 3)
    # every mask covers every pixel with value 1: the composite is a closed form of the colours in area order (all areas tie:
    # kept order), checked on a few pixels in float64
    alpha = np.float32(0.6)
    cols = np.array([c[1][3] for c in _rect_calls(fake_cv2.log)], dtype=np.float64)
    img = image[::271, ::397].double().cpu().numpy()
    acc = img * (1 - float(alpha)) ** K
    for k in range(K):
        acc = acc + cols[k] * float(alpha) * (1 - float(alpha)) ** k
    assert np.abs(out[::271, ::397].astype(np.float64) - acc).max() <= 1.0


@pytest.mark.gpu
def test_infer_loop_visualize(dev, fake_cv2):
    """infer.py -v: infer_loop(..., visualizer=v) times 'Visualize' and returns what calling v afterwards returns."""
    from orienmask_amd import synth
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import infer_loop
    from orienmask_amd.transform import FastCOCOTransform
    from orienmask_amd.visualizer import InferenceVisualizer
    from conftest import post_cfg
    sd = synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0)
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((544, 544)))
    tf = FastCOCOTransform([FastCOCOTransform.Resize((544, 544)), FastCOCOTransform.Normalize((0, 0, 0), (255, 255, 255))])
    imgs = [synth.synth_photo_batch(910 + i, 1, 240 + 16 * i, 320)[0] for i in range(2)]
    v = InferenceVisualizer("COCO", dev, conf_thresh=0.005, alpha=0.6)
    random.seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        dets, pads, log, shows = infer_loop(net, tf, post, imgs, dev, warmup=1, visualizer=v)
    assert set(log) == {"Main Loop", "Load data", "Forward & Postprocess", "Visualize"}
    assert len(shows) == 2 and sum(int(d["bbox"].shape[0]) for d in dets) > 0
    random.seed(9)
    for d, p, img, s in zip(dets, pads, imgs, shows):
        with contextlib.redirect_stdout(io.StringIO()):
            again = v(d, img.to(dev), p)
        assert isinstance(s, np.ndarray) and np.array_equal(s, again)
