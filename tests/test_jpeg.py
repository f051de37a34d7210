"""The JPEG decoder on the GPU: orienmask_amd.jpeg.JpegDecoder (om_jpeg_entropy_decode on the host, om_jpeg_decode_batch on the
device) against PIL's pixels in tests/golden/jpeg_cases.npz -- exact equality, the arithmetic is integer.  The fixture file is
all these tests read: no PIL is needed here.  No test hands a broken stream to a kernel: the host's validation stands between
bad bytes and the device, and tests/test_jpeg_cpu.py tests that.
"""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_np as J
import workspace_poison as wp
from conftest import post_cfg
from orienmask_amd import jpeg as omjpeg, lib as omlib, synth
from orienmask_amd.transform import FastCOCOTransform as T

pytestmark = pytest.mark.gpu

CASES = J.load_cases()
GOOD = [c for c in CASES if c.kind == J.SUPPORTED]
BY = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def decoder(dev):
    return omjpeg.JpegDecoder(dev, threads=8)


def _mixed(n):
    pick = [c for c in GOOD if "_q75" in c.name and c.name.startswith("noise")]
    return (pick[::5] + pick)[:n]                  # a stride coprime to the four samplings the table cycles through


def test_every_supported_fixture_equals_pil(dev, decoder):
    """All 198 supported streams in ONE call (13 launch sets): every size, sampling, quality, table layout and restart interval
    of the table, each image its own geometry."""
    before = decoder.stats()["device"]
    got = decoder.decode([c.data for c in GOOD])
    assert len(got) == len(GOOD) and decoder.stats()["device"] - before == len(GOOD)
    torch.cuda.synchronize(dev)
    bad = []
    for g, c in zip(got, GOOD):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == c.rgb.shape and g.is_contiguous(), c.name
        if not np.array_equal(g.cpu().numpy(), c.rgb):
            bad.append(c.name)
    assert bad == []


def test_one_call_across_the_launch_limit_equals_per_image_calls(dev, decoder):
    cases = _mixed(omlib.OM_JPEG_BATCH + 1)
    assert len({c.rgb.shape for c in cases}) > 5 and len({c.name.split("_")[2] for c in cases}) == 4
    together = decoder.decode([c.data for c in cases])
    for g, c in zip(together, cases):
        alone = decoder.decode([c.data])[0]
        assert torch.equal(g, alone) and np.array_equal(g.cpu().numpy(), c.rgb), c.name


def test_result_does_not_depend_on_workspace_or_output_contents(dev):
    """om_jpeg_decode_batch on caller-owned memory under tests/workspace_poison.py's fills: the workspace (the component planes)
    and the output (whose bytes between the images keep their fill)."""
    cases = [BY[n] for n in ("noise_17x33_420_q75", "noise_9x17_422_q75", "noise_5x3_444_q75", "noise_15x31_grey_q75",
                             "noise_3x4_420_q75", "checker_33x65_420_q100")]
    recs = [J.info(c.data) for c in cases]
    p = omjpeg.plan(recs)
    stage = np.zeros(p.stage_bytes, np.uint8)
    for k, c in enumerate(cases):
        end = p.coef_off[k + 1] if k + 1 < len(cases) else p.coef_elems
        rec = omjpeg.host_entropy_decode(c.data, stage[:p.quant_stage_off].view(np.int16)[p.coef_off[k]:end],
                                         stage[p.quant_stage_off:].view(np.uint16)[p.quant_off[k]:p.quant_off[k] + 192])
        assert rec[omlib.OM_JPEG_I_SUPPORTED]
    staged = torch.from_numpy(stage).to(dev)
    coef, quant = staged[:p.quant_stage_off], staged[p.quant_stage_off:]
    desc = p.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ws_bytes = omlib.workspace_bytes("om_jpeg_workspace_bytes", desc, len(cases))
    assert ws_bytes == sum(-(-int(r[omlib.OM_JPEG_I_BLOCKS]) * 64 // 16) * 16 for r in recs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(p.out_bytes, dtype=torch.uint8, device=dev)
    pattern = wp.CurrentPattern()

    def run():
        omlib.launch("om_jpeg_decode_batch", dev, desc, len(cases), coef, p.coef_elems, quant, p.quant_elems, ws, ws_bytes, out, p.out_bytes)
        host = out.cpu()
        gaps = torch.ones(p.out_bytes, dtype=torch.bool)
        images = []
        for off, c in zip(p.out_off, cases):
            gaps[off:off + c.rgb.size] = False
            images.append(host[off:off + c.rgb.size].clone())
        assert (host[gaps] == pattern.value).all(), "a byte of the output outside the images was written"
        return images

    base = wp.agree(run, [ws, out, pattern])
    for g, c in zip(base, cases):
        assert np.array_equal(g.numpy().reshape(c.rgb.shape), c.rgb), c.name
    # a row that does not fit its buffers is refused before anything is launched
    for args in ((coef, p.coef_elems - 64, quant, p.quant_elems, ws, ws_bytes, out, p.out_bytes),
                 (coef, p.coef_elems, quant, p.quant_elems - 1, ws, ws_bytes, out, p.out_bytes),
                 (coef, p.coef_elems, quant, p.quant_elems, ws, ws_bytes - 16, out, p.out_bytes),
                 (coef, p.coef_elems, quant, p.quant_elems, ws, ws_bytes, out, p.out_bytes - 16)):
        wp.fill(out, 0x7C)
        with pytest.raises(omlib.OrienMaskHipError):
            omlib.launch("om_jpeg_decode_batch", dev, desc, len(cases), *args)
        assert (out.cpu() == 0x7C).all()


def test_decode_then_batch_equals_batch_of_the_fixture_pixels(dev, decoder):
    tf = T([T.Resize((64, 96)), T.Normalize((123.675, 116.28, 103.53), (58.395, 57.12, 57.375))])
    cases = _mixed(5)
    x, pads = tf.batch(decoder.decode([c.data for c in cases]))
    want, want_pads = tf.batch([c.rgb.copy() for c in cases], device=dev)
    assert torch.equal(x, want) and pads == want_pads


def test_infer_loop_from_jpeg_bytes(dev, decoder):
    """infer_loop(decoder=...) over four streams: the detections of the same loop over the fixture pixels."""
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import infer_loop
    sd = synth.synth_state_dict(1, obj_bias=-22.0, head_gain=4.0)          # the weights and size of smoke()
    net = OrienMaskYOLOFPNPlus(3, 80).eval().set_precision("f32")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((96, 96)))
    tf = T([T.Resize((96, 96)), T.Normalize((0, 0, 0), (255, 255, 255))])
    cases = [BY[n] for n in ("noise_33x65_420_q75", "ramp_33x65_422_q100", "noise_17x33_444_q75", "noise_16x16_grey_q75")]
    want, want_pads, _ = infer_loop(net, tf, post, [c.rgb.copy() for c in cases], dev, warmup=1, batch_size=4)
    dets, pads, log = infer_loop(net, tf, post, [c.data for c in cases], dev, warmup=1, batch_size=4, decoder=decoder)
    print("detections per image:", [int(d["bbox"].shape[0]) for d in want])
    assert len(dets) == 4 and pads == want_pads and sum(int(d["bbox"].shape[0]) for d in want) > 0
    for a, b in zip(dets, want):
        assert all(torch.equal(a[k], b[k]) for k in ("bbox", "cls", "mask"))
    assert set(log) == {"Main Loop", "Load data", "Forward & Postprocess"}
    # one image at a time goes through the same path
    dets_1, pads_1, _ = infer_loop(net, tf, post, [c.data for c in cases[:2]], dev, warmup=0, batch_size=1, decoder=decoder)
    assert pads_1 == want_pads[:2]
    with torch.no_grad():
        for c, d in zip(cases, dets_1):
            again = post(net(tf.batch([c.rgb.copy()], device=dev)[0]))[0]
            assert all(torch.equal(again[k], d[k]) for k in ("bbox", "cls", "mask"))
    with pytest.raises(ValueError):
        infer_loop(net, tf, post, [cases[0].data], dev, warmup=0, decoder=decoder, channel_order="bgr")


def test_a_rejected_stream_raises_before_any_launch(dev):
    d = omjpeg.JpegDecoder(dev, threads=2)
    launched = []
    real = d._launch
    d._launch = lambda p, staged: (launched.append(len(p.desc)), real(p, staged))[1]
    for bad in ("truncated_20", "undefined_code", "bad_restart_number"):
        with pytest.raises(omjpeg.JpegError, match="item 1"):
            d.decode([GOOD[0].data, BY[bad].data, GOOD[1].data])
    assert launched == [] and d.stats()["device"] == 0
    got = d.decode([GOOD[0].data, GOOD[1].data])                               # ... and the decoder is still usable
    assert launched == [2] and all(np.array_equal(g.cpu().numpy(), c.rgb) for g, c in zip(got, GOOD[:2]))


def test_unsupported_streams_take_the_fallback_or_raise(dev):
    items = [GOOD[3].data, BY["progressive"].data, BY["exif_orientation_6"].data, BY["range_beyond_8x147"].data, GOOD[9].data]
    d = omjpeg.JpegDecoder(dev, on_unsupported="raise")
    with pytest.raises(omjpeg.JpegError, match=r"item 1 .*progressive"):
        d.decode(items)
    with pytest.raises(omjpeg.JpegError, match=r"item 0 .*orientation"):
        d.decode(items[2:])
    with pytest.raises(omjpeg.JpegError, match=r"item 0 .*range"):
        d.decode(items[3:])
    if omjpeg.default_imread_bytes() is None:
        pytest.skip("no host reader (cv2 or PIL) is importable: nothing to fall back to")
    d = omjpeg.JpegDecoder(dev)
    got = d.decode(items)
    assert d.stats() == {"device": 2, "fallback": 3, "reasons": {"progressive": 1, "orientation": 1, "range": 1}}
    assert all(g.is_cuda and g.dtype == torch.uint8 and g.ndim == 3 for g in got)
    assert np.array_equal(got[0].cpu().numpy(), GOOD[3].rgb) and np.array_equal(got[4].cpu().numpy(), GOOD[9].rgb)
    try:
        import cv2  # noqa: F401
    except ImportError:                                                        # PIL read them: the fixture's own pixels
        for g, name in zip(got[1:4], ("progressive", "exif_orientation_6", "range_beyond_8x147")):
            assert np.array_equal(g.cpu().numpy(), BY[name].rgb), name
