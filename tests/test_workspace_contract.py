"""GPU: no entry's result depends on what its caller-provided memory held on entry (tests/workspace_poison.py).

Every entry below works in memory the caller allocates -- workspaces, scratch, outputs -- and the Python side allocates it with
torch.empty and keeps it.  Each test hands the entry that memory filled with 0x00, 0xFF, 0x7C and 0x01 in turn (agree): the
DEFINED part of the outputs must be the same bytes every time, and the 0x00 result is then held to the expectation the entry's own
tests use, imported from them.  Where a Python wrapper allocates outputs itself, the entry is called the way the wrapper calls it
(lib.launch) on buffers of the test's own; where that would restate pages of argument plumbing (augmentation, COCO evaluation,
segmentation decode, visualiser, RLE strings) the wrapper itself runs with every torch.empty it makes poisoned
(workspace_poison.FreshAllocations).  stale() cases run a loud call, then a quiet one, on one cached Python object against a fresh
object whose workspace was 0xFF.

Entries pinned here (each: include/orienmask_hip.h says "contents undefined on entry" for its workspace)
  om_forward, om_forward_f16              test_forward, test_forward_latency_split_k, test_forward_wide_3x3, test_forward_two_streams,
                                          test_forward_stale_after_a_loud_batch
  om_postprocess                          test_postprocess_s9
  om_model_attach_postprocess             test_postprocess_attached_to_the_forward
  om_postprocess_candidates / _masks      test_postprocess_candidates_then_masks, test_postprocess_masks_case
  om_nms_ex                               test_nms
  om_loss, om_loss_backward               test_loss_and_backward, test_loss_stale_workspace_most_few_none
  om_loss_targets                         test_loss_targets
  om_augment, om_segm_decode              test_augment, test_segm_decode_through_the_loader
  om_cocoeval_masks / _mask_stats         test_cocoeval_masks
  om_visualize                            test_visualize
  om_recover_masks_rle_strings            test_rle_strings
  om_bn_act_forward / _backward (+ _bf16) test_bn_act_two_launch_form
  om_conv2d_grad_weight (+ _bf16_)        test_conv_grad_weight_multi_split
  om_sgd_clip_step, om_sgd_clip_ema_step  test_sgd_partials, test_valid_since_is_a_real_dependence (the positive control)

Poison cannot make a kernel wait.  Read from the code before the first run: the words a kernel polls or draws tickets from, and
where the entry itself clears them on its stream before the first reader.
  om_forward / om_forward_f16   per layer SYNC_WORDS ints: [0..7] the tile / slot queues (atomicAdd: conv_igemm*.hip,
                                conv_wino*.hip, conv3x3_f16.hip), [8] conv_wino14.hip's wide-form queue, [SK_FLAG_OFF + s] the
                                stream-K "slot s has published" flags -- the ONLY polled words of the library, conv_wino24.hip:314
                                and conv_wino.hip:223, both bounded spins that report OM_STATUS_SK_TIMEOUT -- and, in the same
                                words, conv_igemm_split.hip's split-K arrival counters (kflags, :455 / :748: counted, never
                                waited for); behind them the status word.  All cleared by launch_zero_words in forward_impl,
                                om_model.cpp:952, before layer 0 is launched, on the stream every layer then runs on (each
                                sub-batch of set_streams clears its own part on its own stream).  The partial-tile area is data:
                                every part is written before the counter that admits its reader is incremented.
  single-layer entries          a library-owned ticket block, cleared per call: om_layer_entries.cpp:32.
  om_postprocess*               hist1 [B][L1_BINS] and list_count [B] (atomicAdd / one relaxed load, post.hip:221-232): cleared in
                                om_postprocess_detect, post.hip:1288, and om_postprocess_candidates, post.hip:1326; tile_count is
                                stored by every decode workgroup (post.hip:277 / :295) before the select kernel reads it.  Nothing
                                is polled.  om_postprocess_masks / _assemble read det_par, which post_detpar_kernel / the select
                                kernel's tail write for every row below the count.
  om_nms_ex                     three kernels in stream order (post.hip:1390-1395), no atomics, no polling.
  om_loss                       the result vector with its flag word (atomicOr, loss.hip:86) is cleared in loss_run before
                                loss_match_kernel; the match records and partial sums are written by the kernel in front of their
                                reader.  om_loss_backward reads what om_loss left (poison goes in before om_loss only).
  om_cocoeval_masks / om_segm_decode  the bitmaps are cleared by launch_coco_raster's stage 1; no polling.
  om_recover_masks_rle_strings  str_cursor is "zeroed by the caller" (coco_format.py zeroes hdr): a caller-initialised word.
  om_sgd_clip_*                 partials are written by the norm kernel before the finish kernel sums them; valid_since, the clip
                                state and the EMA state are caller-initialised (the positive control below).
  om_augment, om_visualize, om_bn_act_*, om_conv2d*_grad_*   no queue, flag or counter: partial sums and per-mask records, each
                                written by the launch in front of its reader.
Nothing was found uncleared, so no poisoned run was withheld."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import orienmask_ref as R
from orienmask_amd import lib as omlib
from orienmask_amd import synth
from workspace_poison import PATTERNS, CurrentPattern, FreshAllocations, WorkspaceDependence, agree, fill, stale

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _cpu(t):
    return t.detach().contiguous().cpu()


# =====================================================================================================================
# forward
# =====================================================================================================================
FWD_SEEDS = (8, 31)          # tests/test_layer_audit.py's synthetic weights and images
_ORACLE = {}


def _weights():
    return synth.synth_state_dict(FWD_SEEDS[0], obj_bias=-16.0, head_gain=4.0)


def _net(dev, precision):
    from test_hip_parity import _hip_model
    return _hip_model(_weights(), dev, precision)


def _oracle(precision, shape):
    key = ("f16" if precision == "f16" else "f32", shape)
    if key not in _ORACLE:
        x = synth.synth_image_batch(FWD_SEEDS[1], *shape)
        with torch.no_grad():
            _ORACLE[key] = (R.forward_f16 if precision == "f16" else R.forward)(_weights(), x)
    return _ORACLE[key]


def _forward_owned(net, x):
    """model._forward's allocations and launch (orienmask_amd/model.py), with every buffer in the test's hands: -> (run, owned).
    run() launches and returns the defined outputs on the host: the six head views of Prediction (the channels behind bbox_dim are
    not defined) and the status word of every sub-batch."""
    from orienmask_amd.model import HEAD_PIX_STRIDE
    L = omlib.load()
    dev = x.device
    B, _, H, W = x.shape
    precision = net.precision
    f16, split = precision == "f16", precision == "f32_split"
    net.packed_weights(dev)
    if f16:
        net.packed_weights_f16(dev)
    if split:
        net.packed_weights_split(dev)
    h = net._handle
    omlib.call("om_model_set_precision", h, 1 if split else 0)
    n_sub = net.n_streams if (net.n_streams > 1 and B % net.n_streams == 0) else 1
    Bs = B // n_sub
    nbytes = (L.om_forward_f16_workspace_bytes if f16 else L.om_forward_workspace_bytes)(h, Bs, H, W)
    ws_each = (nbytes + 255) // 256 * 256
    ws = torch.empty(ws_each * n_sub, dtype=torch.uint8, device=dev)
    A = net.num_anchors
    bbox_dim = A * (5 + net.num_classes)
    heads = [torch.empty((B, H // s, W // s, HEAD_PIX_STRIDE), dtype=torch.float32, device=dev) for s in (32, 16, 8)]
    oriens = torch.empty((B, 6 * A, H // 4, W // 4), dtype=torch.float32, device=dev)
    fwd = "om_forward_f16" if f16 else "om_forward"
    side = [torch.cuda.Stream(device=dev) for _ in range(n_sub)] if n_sub > 1 else None

    def launch(i, stream=None):
        omlib.launch(fwd, dev, h, x[i * Bs:], Bs, H, W, heads[0][i * Bs:], heads[1][i * Bs:], heads[2][i * Bs:], oriens[i * Bs:],
                     ws.data_ptr() + i * ws_each, ws_each, stream=stream)

    def run():
        if n_sub == 1:
            launch(0)
        else:
            cur = torch.cuda.current_stream(dev)
            for i in range(n_sub):
                side[i].wait_stream(cur)           # behind the fill of this pattern
                launch(i, side[i])
            for i in range(n_sub):
                cur.wait_stream(side[i])
        out = {"bbox%d" % s: _cpu(t[..., :bbox_dim]) for s, t in zip((32, 16, 8), heads)}
        out["oriens"] = _cpu(oriens)
        if not f16:
            off = L.om_forward_status_offset(h, Bs, H, W)
            out["status"] = _cpu(ws.view(n_sub, ws_each)[:, off:off + 4].clone().view(torch.int32).reshape(n_sub))
        return out

    return run, [ws, oriens] + heads


def _hold_to_oracle(base, precision, shape):
    """The heads against the CPU oracle under the bars of tests/test_hip_parity.py (REL_TOL / F16_FWD_TOL of each tensor's scale)."""
    from test_hip_parity import F16_FWD_TOL, REL_TOL, _rel_err
    tol = F16_FWD_TOL if precision == "f16" else REL_TOL
    ref = _oracle(precision, shape)
    A2 = ref[0][1].shape[1]
    for i, s in enumerate((32, 16, 8)):
        got_b = base["bbox%d" % s].permute(0, 3, 1, 2)
        got_o = base["oriens"][:, i * A2:(i + 1) * A2]
        assert got_b.shape == ref[i][0].shape and got_o.shape == ref[i][1].shape
        assert torch.isfinite(got_b).all() and torch.isfinite(got_o).all()
        assert _rel_err(got_b, ref[i][0]) < tol and _rel_err(got_o, ref[i][1]) < tol, (precision, shape, s)
    if "status" in base:
        assert not base["status"].any(), "the forward's status word is set"


@pytest.mark.parametrize("shape", [(3, 64, 96), (1, 160, 128)], ids=["b3-64x96", "b1-160x128"])
@pytest.mark.parametrize("precision", ["f32", "f32_split", "f16"])
def test_forward(dev, precision, shape):
    """The whole live-range-shared workspace -- activations, Winograd scratch, partial-tile area, tickets, status word -- and the
    four head tensors, at the two small shapes of the layer audit."""
    net = _net(dev, precision)
    x = synth.synth_image_batch(FWD_SEEDS[1], *shape).to(dev)
    run, owned = _forward_owned(net, x)
    _hold_to_oracle(agree(run, owned), precision, shape)


def _split_k_parts(net, B, H, W):
    """{layer: parts} for the layers the plan gives to the implicit GEMM's deep-ring forms in latency mode: launch_tile_split's
    rule (conv_igemm_split.hip) on the tile layer_kernels() reports -- at most 8, 512 / tiles, k-steps / 16."""
    from orienmask_amd import arch
    specs = {s.name: s for s in arch.model_convs(type(net).__name__)}
    info = {l["name"]: l for l in net._layers}
    out = {}
    for name, kern in net.layer_kernels(B, H, W):
        if not kern.startswith("conv_igemm_split_kernel<") or "gather" in kern:
            continue
        bm, bn = (int(v) for v in kern[kern.index("<") + 1:kern.index(">")].split(",")[:2])
        if (bm, bn) not in ((128, 64), (64, 64)):
            continue
        spec = specs[name]
        div = arch.layer_div(spec)
        M = B * (H // div) * (W // div)
        tiles = -(-M // bm) * (info[name]["cout_pad"] // bn)
        if tiles > 256:
            continue
        ksteps = spec.ksize * spec.ksize * (spec.cin // 16)
        out[name] = max(1, min(8, 512 // tiles, ksteps // 16))
    return out


def _smallest_split_k_size(net):
    for H, W in sorted(((h, w) for h in range(32, 193, 32) for w in range(32, 193, 32)), key=lambda s: (s[0] * s[1], s)):
        parts = _split_k_parts(net, 1, H, W)
        if any(v > 1 for v in parts.values()):
            return (1, H, W), parts
    raise AssertionError("no size up to 192 x 192 cuts a k loop")


def test_forward_latency_split_k(dev):
    """Latency mode at the smallest size at which a layer's k loop is cut into parts: the parts' raw accumulators meet in the
    partial-tile area and the arrival counters live in the ticket words."""
    net = _net(dev, "f32_split").set_latency_mode(True)
    shape, parts = _smallest_split_k_size(net)
    assert max(parts.values()) > 1, parts
    print("latency mode, %s: k loops cut in %s" % (shape, {k: v for k, v in parts.items() if v > 1}))
    x = synth.synth_image_batch(FWD_SEEDS[1], *shape).to(dev)
    run, owned = _forward_owned(net, x)
    _hold_to_oracle(agree(run, owned), "f32_split", shape)


def test_forward_wide_3x3(dev):
    """The 140 strips of 32 x 544 of test_forward_wide_3x3_switch_is_bit_identical: the wide 3x3 form's transformed input lives in
    the workspace between its two kernels.  Expectation: that test's own -- the heads of the forward with the switch off."""
    L = omlib.load()
    B, H, W = 140, 32, 544
    x = synth.synth_image_batch(34, B, H, W).to(dev)
    was = L.om_get_wino14_wide()
    try:
        omlib.check(L.om_set_wino14_wide(1), "om_set_wino14_wide")
        net = _net(dev, "f32_split")
        assert any(v.startswith("wino14_wide_kernel") for _, v in net.layer_kernels(B, H, W))
        run, owned = _forward_owned(net, x)
        base = agree(run, owned)
        omlib.check(L.om_set_wino14_wide(0), "om_set_wino14_wide")
        assert not any(v.startswith("wino14_wide_kernel") for _, v in net.layer_kernels(B, H, W))
        fill(owned[0], 0xFF)
        off, _ = _forward_owned(net, x)
        want = off()
    finally:
        L.om_set_wino14_wide(was)
    assert not base["status"].any()
    for k in base:
        assert torch.equal(base[k], want[k]), k


def test_forward_two_streams(dev):
    """set_streams(2) at B = 2: each sub-batch clears and uses its own half of the workspace on its own stream."""
    shape = (2, 64, 96)
    net = _net(dev, "f32_split").set_streams(2)
    x = synth.synth_image_batch(FWD_SEEDS[1], *shape).to(dev)
    run, owned = _forward_owned(net, x)
    base = agree(run, owned)
    assert base["status"].numel() == 2
    _hold_to_oracle(base, "f32_split", shape)
    one, _ = _forward_owned(net.set_streams(1), x)
    want = one()
    for k in ("bbox32", "bbox16", "bbox8", "oriens"):
        assert torch.equal(base[k], want[k]), k


@pytest.mark.parametrize("slot", [0, 1], ids=["model._workspace", "_slot_workspaces"])
def test_forward_stale_after_a_loud_batch(dev, slot):
    """One net, its cached workspace (slot 0) or a pipeline slot's: a batch scaled until the split operands leave their range
    (NaN activations, the status word set), then an ordinary batch -- equal to the ordinary batch on a new net whose freshly
    allocated workspace held 0xFF."""
    shape = (2, 64, 96)
    x = synth.synth_image_batch(FWD_SEEDS[1], *shape).to(dev)
    loud = x * 3.0e3
    net = _net(dev, "f32_split")

    def through(n, batch):
        with torch.no_grad(), n.workspace_slot(slot):
            pred = n(batch)
        out = {"h%d%d" % (i, j): _cpu(t) for i, pair in enumerate(pred) for j, t in enumerate(pair)}
        out["status"] = _cpu(pred.status)
        return out

    def run_loud():
        print("status word of the loud batch: %d" % through(net, loud)["status"].item())

    def fresh():
        with FreshAllocations(0xFF):
            return through(_net(dev, "f32_split"), x)

    want = stale(run_loud, lambda: through(net, x), fresh)
    assert want["status"].item() == 0 and (net._workspace if slot == 0 else net._slot_workspaces[slot])


# =====================================================================================================================
# postprocess
# =====================================================================================================================
def _post_buffers(post, B, dev):
    return dict(bbox=torch.empty((B, post.nms_post, 5), dtype=torch.float32, device=dev),
                cls=torch.empty((B, post.nms_post), dtype=torch.long, device=dev),
                mask=torch.empty((B, post.nms_post, post.image_h, post.image_w), dtype=torch.uint8, device=dev),
                count=torch.empty((B,), dtype=torch.int32, device=dev),
                keep=torch.empty((B, post.nms_post), dtype=torch.int32, device=dev))


def _defined_detections(o, pattern, B):
    """The defined part of the postprocess outputs: the counts, the rows below each count; mask rows at or beyond the count keep
    their fill (tests/test_post_directed.py::_check_masks)."""
    counts = _cpu(o["count"])[:B]
    out = {"count": counts}
    for b, n in enumerate(counts.tolist()):
        assert 0 <= n <= o["bbox"].shape[1], (b, n)
        for k in ("bbox", "cls", "keep", "mask"):
            out["%s%d" % (k, b)] = _cpu(o[k][b, :n])
        assert bool((o["mask"][b, n:] == pattern).all()), (b, "mask rows at or beyond count[b] were written", hex(pattern))
    return out


def _check_s9(base, members):
    from test_post_directed import _check_exact, _expected_select
    for b, m in enumerate(members):
        if m is None:
            assert int(base["count"][b]) == 0
            continue
        r = dict(bbox=base["bbox%d" % b], cls=base["cls%d" % b], mask=base["mask%d" % b].view(torch.bool))
        _check_exact(r, base["keep%d" % b], _expected_select(m.id), ("S9", b, m.id))


def _s9(dev):
    import post_cases as K
    from test_post_directed import _hip_post, _to_device
    members = [K.select_cases()[cid] if cid else None for cid in K.S9_MEMBERS]
    cfg = dict(nms_pre=400, nms_post=400)
    assert all(m is None or m.cfg == cfg for m in members)
    predict = _to_device(K.cat_batch([m.predict if m else K.empty_predict() for m in members]), dev, "model")
    return members, predict, _hip_post(dev, **cfg)


def test_postprocess_s9(dev):
    """om_postprocess on the S9 batch (the radix path, the list path at total == nms_pre, an empty image): keys, tile counts,
    histograms, the candidate list, the detections' mask constants and every output poisoned."""
    members, predict, post = _s9(dev)
    B = 3
    bboxes, pix = post._bbox_nhwc(predict)
    oriens = post._oriens_nchw(predict)
    cfg = post.cfg_struct(pix)
    ws = torch.empty(omlib.workspace_bytes("om_postprocess_workspace_bytes", ctypes.byref(cfg), B), dtype=torch.uint8, device=dev)
    o = _post_buffers(post, B, dev)
    pat = CurrentPattern()

    def run():
        omlib.launch("om_postprocess", dev, ctypes.byref(cfg), bboxes[0], bboxes[1], bboxes[2], oriens, B, o["bbox"], o["cls"],
                     o["mask"], o["count"], o["keep"], ws, ws.numel())
        return _defined_detections(o, pat.value, B)

    _check_s9(agree(run, [ws, pat] + list(o.values())), members)


def test_postprocess_candidates_then_masks(dev):
    """The S9 batch through om_postprocess_candidates, batched_nms per image and om_postprocess_masks, as eval.py's
    _launch_foreign composes them: the candidates' defined rows, then the masks.  The composed detections are the fused ones."""
    from orienmask_amd.eval import batched_nms
    members, predict, post = _s9(dev)
    B = 3
    bboxes, pix = post._bbox_nhwc(predict)
    oriens = post._oriens_nchw(predict)
    cfg = post.cfg_struct(pix)
    ws = torch.empty(omlib.workspace_bytes("om_postprocess_workspace_bytes", ctypes.byref(cfg), B), dtype=torch.uint8, device=dev)
    cd = torch.empty((B, post.nms_pre, 5), dtype=torch.float32, device=dev)
    cc = torch.empty((B, post.nms_pre), dtype=torch.long, device=dev)
    cf = torch.empty((B, post.nms_pre), dtype=torch.int32, device=dev)
    cn = torch.empty((B,), dtype=torch.int32, device=dev)

    def candidates():
        omlib.launch("om_postprocess_candidates", dev, ctypes.byref(cfg), bboxes[0], bboxes[1], bboxes[2], B, cd, cc, cf, cn, ws, ws.numel())
        counts = _cpu(cn)
        out = {"count": counts}
        for b, n in enumerate(counts.tolist()):
            assert 0 <= n <= post.nms_pre
            out.update({"dets%d" % b: _cpu(cd[b, :n]), "cls%d" % b: _cpu(cc[b, :n]), "field%d" % b: _cpu(cf[b, :n])})
        return out

    cand = agree(candidates, [ws, cd, cc, cf, cn])
    dets = torch.zeros((B, post.nms_post, 5), dtype=torch.float32, device=dev)
    field = torch.zeros((B, post.nms_post), dtype=torch.int32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    final = {"count": torch.zeros(B, dtype=torch.int32)}
    for b, n in enumerate(cand["count"].tolist()):
        kd, kc, keep = (batched_nms(cand["dets%d" % b].to(dev), cand["cls%d" % b].to(dev)) if n else
                        (torch.zeros((0, 5), device=dev), torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev)))
        if keep.numel() > post.nms_post:
            _, topk = kd[:, -1].topk(post.nms_post)
            kd, kc, keep = kd[topk], kc[topk], keep[topk]
        k = int(keep.numel())
        dets[b, :k], count[b] = kd, k
        field[b, :k] = cand["field%d" % b].to(dev)[keep]
        final["count"][b] = k
        final.update({"bbox%d" % b: _cpu(kd), "cls%d" % b: _cpu(kc), "keep%d" % b: _cpu(keep.to(torch.int32))})
    out_mask = torch.empty((B, post.nms_post, post.image_h, post.image_w), dtype=torch.uint8, device=dev)
    pat = CurrentPattern()

    def masks():
        omlib.launch("om_postprocess_masks", dev, ctypes.byref(cfg), oriens, B, dets, field, count, out_mask, ws, ws.numel())
        out = {}
        for b, n in enumerate(final["count"].tolist()):
            out["mask%d" % b] = _cpu(out_mask[b, :n])
            assert bool((out_mask[b, n:] == pat.value).all()), (b, "mask rows at or beyond count[b] were written")
        return out

    final.update(agree(masks, [ws, out_mask, pat]))
    _check_s9(final, members)


def test_postprocess_masks_case(dev):
    """om_postprocess_masks on one directed mask case (every field, two images of 12 and 16 detections in 16 rows)."""
    import post_cases as K
    from test_post_directed import _check_masks, _hip_post
    case = K.mask_cases()["F1_64x96_mask1"]
    oriens, dets, fields, counts = (t.contiguous().to(dev) for t in (case.oriens, case.dets, case.fields, case.counts))
    B = oriens.shape[0]
    post = _hip_post(dev, case.size, case.anchor_mask, nms_pre=max(400, case.nms_post), nms_post=case.nms_post)
    cfg = post.cfg_struct(255)
    ws = torch.empty(omlib.workspace_bytes("om_postprocess_workspace_bytes", ctypes.byref(cfg), B), dtype=torch.uint8, device=dev)
    out_mask = torch.empty((B, case.nms_post, case.size[0], case.size[1]), dtype=torch.uint8, device=dev)

    def run():
        omlib.launch("om_postprocess_masks", dev, ctypes.byref(cfg), oriens, B, dets, fields, counts, out_mask, ws, ws.numel())
        return {"mask%d" % b: _cpu(out_mask[b, :int(case.counts[b])]) for b in range(B)}

    agree(run, [ws, out_mask])
    # the 0x00 result under the existing checker, whose "untouched" byte is 0xAB
    out_mask.fill_(0xAB)
    fill(ws, 0x00)
    run()
    _check_masks(out_mask.cpu(), K.expected_masks(case), case.counts, case.id)


def test_postprocess_attached_to_the_forward(dev):
    """eval.launch_step's form: the postprocess attached to the forward, decode + select on the library's second stream.  Both
    workspaces and every output of both poisoned.  Expectation: test_launch_step_same_bits_as_two_calls' -- the two calls."""
    from test_hip_parity import _hip_post
    from orienmask_amd.model import HEAD_PIX_STRIDE
    size, B = (96, 96), 2
    sd = synth.synth_state_dict(1, obj_bias=-22.0, head_gain=4.0)          # smoke()'s weights and image: detections in both images
    from test_hip_parity import _hip_model
    net = _hip_model(sd, dev, "f32_split")
    x = synth.synth_image_batch(21, B, *size).to(dev)
    post = _hip_post(size, dev, nms_pre=400, nms_post=100)
    with torch.no_grad():
        want = post(net(x))
    want_keep = [k.clone() for k in post.last_keep]
    assert sum(int(d["cls"].numel()) for d in want) > 0
    fwd, owned = _forward_owned(net, x)
    cfg = post.cfg_struct(HEAD_PIX_STRIDE)
    ws = torch.empty(omlib.workspace_bytes("om_postprocess_workspace_bytes", ctypes.byref(cfg), B), dtype=torch.uint8, device=dev)
    o = _post_buffers(post, B, dev)
    pat = CurrentPattern()
    h = net._ensure_handle()

    def run():
        omlib.call("om_model_attach_postprocess", h, ctypes.byref(cfg), o["bbox"], o["cls"], o["mask"], o["count"], o["keep"], ws, ws.numel())
        try:
            out = fwd()
        finally:
            omlib.call("om_model_attach_postprocess", h, None, None, None, None, None, None, None, 0)
        out.update(_defined_detections(o, pat.value, B))
        return out

    base = agree(run, owned + [ws, pat] + list(o.values()))
    assert not base["status"].any()
    for b, w in enumerate(want):
        assert torch.equal(base["bbox%d" % b], w["bbox"].cpu()) and torch.equal(base["cls%d" % b], w["cls"].cpu())
        assert torch.equal(base["mask%d" % b].view(torch.bool), w["mask"].cpu()) and torch.equal(base["keep%d" % b], want_keep[b].cpu())


def test_postprocess_stale_cached_workspace(dev):
    """post._ws: the all-pass batch (every pair passes: all keys, all tiles, a full candidate list), then the S9 batch, on one
    OrienMaskYOLOPostProcess, against a new one whose workspace and outputs held 0xFF."""
    import post_cases as K
    from test_post_directed import _hip_post, _to_device
    members, predict, post = _s9(dev)
    loud = _to_device(K.all_pass_predict(3), dev, "model")

    def through(p, pred):
        res = p(pred)
        out = {"count": torch.tensor([int(r["bbox"].shape[0]) for r in res])}
        for b, r in enumerate(res):
            out.update({"bbox%d" % b: _cpu(r["bbox"]), "cls%d" % b: _cpu(r["cls"]), "mask%d" % b: _cpu(r["mask"]).view(torch.uint8),
                        "keep%d" % b: _cpu(p.last_keep[b])})
        return out

    def fresh():
        with FreshAllocations(0xFF):
            return through(_hip_post(dev, nms_pre=400, nms_post=400), predict)

    _check_s9(stale(lambda: through(post, loud), lambda: through(post, predict), fresh), members)


# =====================================================================================================================
# NMS
# =====================================================================================================================
@pytest.mark.parametrize("semantics", [0, 1], ids=["cpu", "cuda"])
def test_nms(dev, semantics):
    """om_nms_ex at n = 1, 64, 65 and the sizes of test_nms_beyond_one_workgroup (the bit matrix in the workspace): sorted
    boxes, the suppression bit matrix, keep and n_keep poisoned.  keep is defined below n_keep."""
    import nms_cases as N
    L = omlib.load()
    by_n = {c["dets"].shape[0]: c for c in N.cases(("blocks",))}
    for n in (1, 64, 65, 4000, 9000):
        c = by_n[n]
        d = torch.from_numpy(c["dets"]).to(dev)
        thr = float(c["thr"])
        keep = torch.empty(n, dtype=torch.long, device=dev)
        n_keep = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(L.om_nms_workspace_bytes(n), dtype=torch.uint8, device=dev)

        def run():
            omlib.launch("om_nms_ex", dev, d, n, thr, semantics, keep, n_keep, ws, ws.numel())
            k = int(n_keep.item())
            assert 0 < k <= n
            return {"n_keep": _cpu(n_keep), "keep": _cpu(keep[:k])}

        base = agree(run, [keep, n_keep, ws])
        want = c["keep"].tolist() if semantics == 1 else R.nms_cpu(torch.from_numpy(c["dets"]), thr).tolist()
        assert base["keep"].tolist() == want, (n, semantics)


# =====================================================================================================================
# loss
# =====================================================================================================================
LOSS_ORDINARY, LOSS_CROWDED = "seams", "ladder_300_7_pile9"      # 22 GTs in one image; 300 + 7 with a pile of nine on one cell
_LOSS_REF = {}


def _loss_case(name):
    """(cfg, heads, target, restatement) -- 'none' is N = 0: two images of loss_cases' ladder without a single GT."""
    import loss_cases
    import loss_crowd_checks as checks
    if name not in _LOSS_REF:
        if name == "none":
            cfg, heads, target = loss_cases._ladder((64, 96), [0, 0], 7)
            assert target[0].shape[0] == 0
            ref = loss_cases.run_restatement(loss_cases.MemoNP(**cfg), heads, target)
        else:
            cfg, heads, target = loss_cases.build(name)
            ref = loss_cases.reference(name)
        checks.check_near_zero(ref.near, name)
        _LOSS_REF[name] = (cfg, heads, target, ref)
    return _LOSS_REF[name]


def _check_loss_values(loss, host_result, ref, name, dev):
    import loss_crowd_checks as checks
    from test_loss import METRICS, SIDS, TERMS
    assert int(host_result[omlib.OM_LOSS_FLAG_OFF:].view(torch.int32)[0]) == 0
    _, log, mlog = loss.aggregate(host_result, False, None)
    got = [([log[sid + "_" + k] for k in TERMS], [mlog[sid + "_" + k] for k in METRICS]) for sid in SIDS]
    checks.check_values(got, checks.restatement_values(ref), name)


@pytest.mark.parametrize("name", [LOSS_ORDINARY, LOSS_CROWDED, "none"])
def test_loss_and_backward(dev, name):
    """om_loss, then om_loss_backward on what it left: the match records, both partial-sum areas, the result vector and both
    heads' gradients poisoned before om_loss (the backward reads om_loss's workspace)."""
    import loss_cases
    import loss_crowd_checks as checks
    from orienmask_amd.train import _Call
    from test_loss import _to
    from test_loss_grad import _train_loss
    cfg, heads, target, ref = _loss_case(name)
    predict, tgt = _to(dev, heads, target)
    loss = _train_loss(cfg)
    B, N = predict[0][0].shape[0], int(tgt[0].shape[0])
    ws = torch.empty(loss.workspace_bytes(B, N), dtype=torch.uint8, device=dev)
    fwd = loss.prepare(predict, tgt, workspace=ws)
    call = _Call(loss, [(True, True)] * len(predict), fwd)
    bwd, gb, go = call.bind(torch.tensor(loss_cases.GOUT, device=dev))

    def run():
        fwd()
        bwd()
        out = {"result": _cpu(fwd.result)}
        for s in range(len(gb)):
            out.update({"gbbox%d" % s: _cpu(gb[s]), "gorien%d" % s: _cpu(go[s])})
        return out

    base = agree(run, [ws, fwd.result] + gb + go)
    _check_loss_values(loss, base["result"], ref, name, dev)
    checks.check_grads([(base["gbbox%d" % s].numpy(), base["gorien%d" % s].numpy()) for s in range(len(gb))], ref.grads, name)


@pytest.mark.parametrize("name", [LOSS_ORDINARY, LOSS_CROWDED, "none"])
def test_loss_targets(dev, name):
    """om_loss_targets (scale S08, where the crowded case's pile is), called as loss.targets() calls it."""
    import loss_crowd_checks as checks
    from test_loss import _loss, _to
    cfg, heads, target, ref = _loss_case(name)
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    scale = 2
    bboxes = [p[0] for p in predict]
    B = bboxes[0].shape[0]
    gt_bbox, gt_cls, gt_index, gt_mask, N = loss._targets(tgt, B, dev)
    nA, (gh, gw) = len(loss.anchor_mask[scale]), loss.grids[scale]
    H, W, C = loss.image_h, loss.image_w, int(loss.num_classes)
    f = dict(device=dev, dtype=torch.float32)
    out = dict(bbox_pos_mask=torch.empty(B, nA, gh, gw, **f), bbox_neg_mask=torch.empty(B, nA, gh, gw, **f),
               bbox_pos_scale=torch.empty(B, nA, gh, gw, **f), txy=torch.empty(B, nA, gh, gw, 2, **f),
               twh=torch.empty(B, nA, gh, gw, 2, **f), tiou=torch.empty(B, nA, gh, gw, **f), tcls=torch.empty(B, nA, gh, gw, C, **f),
               orien_mask=torch.empty(B, nA, H, W, dtype=torch.int32, device=dev), torien=torch.empty(B, nA, H, W, 2, **f))
    cfg_s = loss.cfg_struct()
    for s, b in enumerate(bboxes):
        for i, v in enumerate(b.stride()):
            cfg_s.bbox_stride[s][i] = v
    ws = torch.empty(loss.workspace_bytes(B, N) + 512, dtype=torch.uint8, device=dev)
    bb = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in bboxes])

    def run():
        omlib.launch("om_loss_targets", dev, ctypes.byref(cfg_s), bb, B, gt_bbox, gt_cls, gt_index, gt_mask, N, scale,
                     *[out[k] for k in ("bbox_pos_mask", "bbox_neg_mask", "bbox_pos_scale", "txy", "twh", "tiou", "tcls", "orien_mask",
                                        "torien")], ws, ws.numel())
        return {k: _cpu(v) for k, v in out.items()}

    base = agree(run, [ws] + list(out.values()))
    checks.check_targets({k: v.numpy() for k, v in base.items()}, ref.values[scale][2], loss.cfg_struct().label_smooth, (name, scale))


def test_loss_stale_workspace_most_few_none(dev):
    """loss._ws is kept whenever it is large enough, so a smaller N lays another layout over old bytes: the crowded case, then
    the ordinary one, then N = 0, on one Loss object -- each against a new object whose workspace held 0xFF.  (The three cases have
    different image sizes: each gets a loss of its own configuration sharing ONE workspace, the largest.)"""
    from test_loss import _loss, _to
    names = [LOSS_CROWDED, LOSS_ORDINARY, "none"]
    cases = {n: _loss_case(n) for n in names}
    dev_in = {n: _to(dev, cases[n][1], cases[n][2]) for n in names}
    losses = {n: _loss(cases[n][0]) for n in names}
    need = {n: losses[n].workspace_bytes(dev_in[n][0][0][0].shape[0], int(dev_in[n][1][0].shape[0])) for n in names}
    assert need[LOSS_CROWDED] == max(need.values()) and need["none"] == min(need.values()), need

    def through(loss, n):
        return {"result": _cpu(loss.launch(*dev_in[n]))}

    kept = None
    for prev, n in zip(names, names[1:]):
        def run_loud():
            through(losses[prev], prev)

        def run_quiet():
            losses[n]._ws = losses[prev]._ws           # the one kept workspace, larger than this call needs
            out = through(losses[n], n)
            assert losses[n]._ws is losses[prev]._ws and losses[n]._ws.numel() == need[LOSS_CROWDED]
            return out

        def fresh():
            with FreshAllocations(0xFF):
                return through(_loss(cases[n][0]), n)

        if kept is not None:
            losses[prev]._ws = kept
        want = stale(run_loud, run_quiet, fresh)
        kept = losses[n]._ws
        _check_loss_values(losses[n], want["result"], cases[n][3], n, dev)


# =====================================================================================================================
# wrappers that allocate for themselves: every torch.empty they make is poisoned
# =====================================================================================================================
def test_augment(dev):
    """om_augment: the grey-mean reduction's workspace and both outputs (transform.to_device's torch.empty), on the grey-mean
    batch (contrast: the reduction runs) and two degenerate geometries with masks."""
    import augment_cases as K
    from test_augment_directed import _launch
    gray, geo = K.graymean_cases(), K.geometry_cases()[:2]
    fresh = FreshAllocations()

    def run():
        with fresh:
            out = {"gray": _launch(gray, dev)[0]}
            for c in geo:
                image, masks = _launch([c], dev)
                out["image_" + c.id], out["masks_" + c.id] = image, masks[0].view(np.uint8)
        return out

    base = agree(run, [fresh])
    for k, c in enumerate(gray):
        K.check_image(base["gray"][k], c)
        K.check_pad(base["gray"][k], c)
    for c in geo:
        K.check_image(base["image_" + c.id][0], c)
        K.check_pad(base["image_" + c.id][0], c)
        K.check_masks(base["masks_" + c.id].view(bool), c)


def test_segm_decode_through_the_loader(dev):
    """om_segm_decode + om_augment as transform.to_device runs them on segmentation samples: the decode's bitmap workspace, its
    mask scratch and the augmentation's buffers.  Expectation: test_end_to_end_equals_the_mask_path's -- the mask path's tensors."""
    import segm_decode_np as S
    from test_segm_decode import _both_ways
    samples = S.end_to_end_samples()
    fresh = FreshAllocations()
    kept = {}

    def run():
        with fresh:
            (got, _, pb_s), (want, _, pb_m) = _both_ways(samples, (96, 96), 2, dev)
        assert pb_s.segm is not None and pb_s.mask.numel() == 0 and pb_m.segm is None
        kept["want"] = want
        return {name: t.view(torch.uint8) if t.dtype == torch.bool else t for name, t in zip(("image", "bbox", "cls", "index", "mask"), got)}

    base = agree(run, [fresh])
    assert base["mask"].shape == (8, 96, 96) and base["mask"].any()
    for (name, a), b in zip(base.items(), kept["want"]):
        assert torch.equal(a.view(b.dtype) if b.dtype == torch.bool else a, b), name


def test_cocoeval_masks(dev):
    """om_cocoeval_masks + om_cocoeval_mask_stats through COCOEvaluator._build_masks: the bitmap workspace (cleared by the raster
    kernels' first stage) and the statistics, on polygons, counts and strings of the mask table."""
    import cocoeval_bitmap_np as Bm
    import cocoeval_cases as C
    import cocoeval_np as ref
    from test_cocoeval_kernels import _build, _evaluator
    cases = [c for c in C.mask_cases() if c[0].startswith(("polys_", "star_65", "counts_checker", "string_column_straddle"))]
    assert len(cases) >= 4
    fresh = FreshAllocations()

    def run():
        with fresh:
            ev, anns = _evaluator(cases, dev)
            words, stats, hw = _build(ev, anns, dev)
        out = {"stats": np.ascontiguousarray(stats), "hw": np.ascontiguousarray(hw)}
        out.update({"words%d" % i: w for i, w in enumerate(words)})
        return out

    base = agree(run, [fresh])
    for i, (name, h, w, segm) in enumerate(cases):
        want = ref.ann_mask(segm, h, w, strict=False)
        assert tuple(base["hw"][i]) == want.shape, name
        got, padding = Bm.unpack(base["words%d" % i], *want.shape)
        assert np.array_equal(got, want) and not padding, name
        assert tuple(int(v) for v in base["stats"][i]) == Bm.stats_of(want), name


def test_visualize(dev):
    """om_visualize with device outlines on the overlapping-masks fixture: the per-mask records in its workspace and the output."""
    from orienmask_amd.visualizer import InferenceVisualizer
    from test_visualizer import _case, _check_u8, _load, _near_half, _paint_outlines, _run
    name = "vis_overlap.npz"
    g = _load(name)
    dets, image, pad, ctor = _case(g, dev)
    fresh = FreshAllocations()

    def run():
        with fresh:
            out, lines = _run(InferenceVisualizer(device=dev, draw="device", **ctor), dets, image, pad, int(g["rand_seed"]))
        assert lines == json.loads(str(g["stdout"]))
        return {"out": out}

    base = agree(run, [fresh])
    want, on = _paint_outlines(g["result"], json.loads(str(g["calls"])))
    assert on.any()
    _check_u8(base["out"], want, _near_half(g) & ~on[:, :, None], name)


def test_rle_strings(dev):
    """om_recover_masks_rle_strings through COCOFormatter: the run-length scratch, the string bytes and the header's offsets
    (the cursor words are zeroed by the caller, as the header asks).  All five reference-generated cases as one batch, and with
    first-guess buffers so small that every mask takes the overflow path into worst-case buffers."""
    from orienmask_amd.coco_format import COCOFormatter
    from test_oracle_golden import _coco_cases
    infos, dets, want = [], [], []
    for i, (name, info, masks, bbox, xywh, seg) in enumerate(_coco_cases()):
        K = masks.shape[0]
        b5 = torch.cat([torch.from_numpy(bbox)[:, :4], torch.linspace(0.9, 0.1, K).reshape(K, 1)], dim=1).float()
        infos.append(dict(info, id=100 + i))
        dets.append(dict(bbox=b5.to(dev), cls=torch.arange(K, dtype=torch.int64, device=dev) % 80, mask=torch.from_numpy(masks).to(dev)))
        want += [R.rle_to_string(R.rle_counts(seg[k])) for k in range(K)]
    fresh = FreshAllocations()

    def run():
        out = {}
        with fresh:
            for max_runs, per_mask in ((8192, 4096), (4, 4096), (8192, 3)):
                fmt = COCOFormatter(list(range(1, 81)), with_mask=True)
                fmt.MAX_RUNS, fmt.BYTES_PER_MASK = max_runs, per_mask
                res = fmt.to_coco_format(infos, dets)
                text = "\n".join(s["segmentation"]["counts"] for s in res["segm"])
                out["strings_%d_%d" % (max_runs, per_mask)] = np.frombuffer(text.encode("ascii"), np.uint8)
                out["boxes_%d_%d" % (max_runs, per_mask)] = np.array([b["bbox"] for b in res["bbox"]], np.float64)
        return out

    base = agree(run, [fresh])
    for k, v in base.items():
        if k.startswith("strings"):
            assert bytes(v).decode("ascii").split("\n") == want, k


# =====================================================================================================================
# training kernels: the full pattern set where their own tests use 0xFF
# =====================================================================================================================
BN_SHAPE = (2, 3, 92, 90)      # 16 560 elements per channel: just above BN_FUSED_MAX = 16 384 (bn_act.hip), planes a multiple of 8


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_act_two_launch_form(dev, training):
    """om_bn_act_forward / _backward and their _bf16 forms at the smallest shape that takes the STATS + APPLY launches: the
    per-workgroup partial sums in the workspace, y, dx, the save vectors, dgamma and dbeta poisoned before each launch."""
    import bn_act_np as N
    import test_bn_act as F32T
    import test_bn_act_bf16 as BF
    L = omlib.load()
    B, C, H, W = BN_SHAPE
    assert B * H * W > 16384 and (B * H * W - 16384) < 256
    d = BF._inputs(BN_SHAPE, 77)
    st = omlib.current_stream_ptr(dev)
    results = {}
    for bf16 in (False, True):
        sfx = "_bf16" if bf16 else ""
        x, dy, res = (BF._act(dev, d[k], bf16, 0) for k in ("x", "dy", "res"))
        y, y0, dx = (BF._act(dev, d["x"], bf16, 0, fill="nan") for _ in range(3))
        sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(L.om_bn_act_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=dev)
        assert ws.numel() > 0
        par = {k: torch.from_numpy(d[k]).to(dev) for k in ("gamma", "beta")}
        state = {}
        owned = [ws, y, y0, dx, sm, si, dg, db]
        refill = CurrentPattern()

        def run():
            rm, rv = torch.from_numpy(d["rm"]).to(dev), torch.from_numpy(d["rv"]).to(dev)
            nbt = torch.tensor(7, dtype=torch.long, device=dev)
            for out, r in ((y0, None), (y, res)):
                fill(ws, refill.value)
                omlib.check(getattr(L, "om_bn_act_forward" + sfx)(
                    _vp(x), B, C, H, W, _vp(par["gamma"]), _vp(par["beta"]), _vp(rm), _vp(rv), _vp(nbt), int(training), N.MOMENTUM, N.EPS,
                    N.SLOPE, _vp(r), _vp(out), _vp(sm), _vp(si), _vp(ws), ws.numel(), st), "om_bn_act_forward" + sfx)
                if out is y0:
                    rm, rv = torch.from_numpy(d["rm"]).to(dev), torch.from_numpy(d["rv"]).to(dev)
            fill(ws, refill.value)
            omlib.check(getattr(L, "om_bn_act_backward" + sfx)(
                _vp(x), _vp(dy), B, C, H, W, _vp(par["gamma"]), _vp(par["beta"]), _vp(sm), _vp(si), int(training), N.SLOPE, _vp(dx),
                _vp(dg), _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward" + sfx)
            torch.cuda.synchronize(dev)
            state.update(y=y.clone(), dx=dx.clone(), save_mean=sm[:C].clone(), save_invstd=si[:C].clone(), rm=rm, rv=rv, dgamma=dg.clone(),
                         dbeta=db.clone(), nbt=nbt)
            bits = (lambda t: t.view(torch.int16)) if bf16 else (lambda t: t)
            return dict(y=_cpu(bits(y)), y0=_cpu(bits(y0)), dx=_cpu(bits(dx)), save_mean=_cpu(sm[:C]), save_invstd=_cpu(si[:C]),
                        rm=_cpu(rm), rv=_cpu(rv), dgamma=_cpu(dg), dbeta=_cpu(db), nbt=_cpu(nbt))

        base = agree(run, owned + [refill])
        results[bf16] = (base, dict(state))
    # float32 entry points: against float64 under test_bn_act's bars (twice torch-CPU's float32 error, the sign mask in its band)
    base, _ = results[False]
    got = {k: v.numpy() for k, v in base.items()}
    got["nbt"] = int(base["nbt"])
    assert got["nbt"] == (9 if training else 7)
    truth = N.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], training, d["res"])
    ref = F32T._torch_cpu(d, training, True)
    what = (BN_SHAPE, "train" if training else "eval")
    F32T._check_mask(got, d, truth, what)
    mine, theirs = F32T._errors(got, d, training, True, truth), F32T._errors(ref, d, training, True, truth)
    for k, e in mine.items():
        assert e <= max(2 * theirs[k], F32T.FLOOR), (what, k, e, theirs[k])
    # bf16 entry points: the rounded float32 block, bit for bit (test_bn_act_bf16._compare; two forwards here: nbt counts both)
    g16, r32 = results[True][1], results[False][1]
    for k in BF.BF16_OUT:
        BF._same_as_rounded(g16[k], r32[k], what + (k,))
    for k in BF.F32_OUT:
        assert np.array_equal(BF._words(g16[k]), BF._words(r32[k])), what + (k,)
    assert int(g16["nbt"]) == int(r32["nbt"])


def test_conv_grad_weight_multi_split(dev):
    """om_conv2d_grad_weight and om_conv2d_bf16_grad_weight at the multi-split case test_case_list_has_a_multi_split_and_a_single_split_dw
    names: the splits' partial dw / db in the workspace."""
    import conv_grad_bf16_np as Cb
    import test_conv_grad as CG
    import test_conv_grad_bf16 as CB
    import train_step as T
    L = omlib.load()
    case = CB.MULTI_SPLIT
    B, cin, cout, ks, stride, H, W = case
    geom = (B, cin, H, W, cout, ks, stride)
    st = omlib.current_stream_ptr(dev)
    # ---- bf16: integer data, on which every sum is exact (test_exact_on_integer_data)
    assert L.om_conv2d_bf16_grad_workspace_bytes(*geom) > 0
    d = Cb.integer_inputs(*case, seed=sum(case) + 11)
    t = Cb.truth(d)
    x, dy = CB._bf16_dev(dev, d["x_bits"]), CB._bf16_dev(dev, d["dy_bits"])
    dw, db = torch.empty(d["w"].shape, device=dev), torch.empty(cout, device=dev)
    ws = torch.empty(L.om_conv2d_bf16_grad_workspace_bytes(*geom), dtype=torch.uint8, device=dev)

    def run_bf16():
        omlib.check(L.om_conv2d_bf16_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw), T.vp(db), T.vp(ws), ws.numel(), st),
                    "om_conv2d_bf16_grad_weight")
        return {"dw": _cpu(dw), "db": _cpu(db)}

    base = agree(run_bf16, [ws, dw, db])
    assert np.array_equal(base["dw"].numpy().astype(np.float64), t["dw"]) and np.array_equal(base["db"].numpy().astype(np.float64), t["db"])
    # ---- float32: against float64 under test_conv_grad's bar
    need = L.om_conv2d_grad_workspace_bytes(*geom)
    assert need > 0
    d32, truth, ref = CG._reference(case, 17, ("dw", "db"))
    x32, dy32 = torch.from_numpy(d32["x"]).to(dev), torch.from_numpy(d32["dy"]).to(dev)
    dw32, db32 = torch.empty(d32["w"].shape, device=dev), torch.empty(cout, device=dev)
    ws32 = torch.empty(need, dtype=torch.uint8, device=dev)

    def run_f32():
        omlib.check(L.om_conv2d_grad_weight(T.vp(x32), T.vp(dy32), *geom, T.vp(dw32), T.vp(db32), T.vp(ws32), ws32.numel(), st),
                    "om_conv2d_grad_weight")
        return {"dw": _cpu(dw32), "db": _cpu(db32)}

    base = agree(run_f32, [ws32, dw32, db32])
    for k in ("dw", "db"):
        g = base[k].numpy()
        assert np.isfinite(g).all()
        e, theirs = CG.G.rel_max(g, truth[k]), CG.G.rel_max(ref[k], truth[k])
        assert e <= max(2 * theirs, CG.FLOOR), (case, k, e, theirs)


class _ClipBuffers(CurrentPattern):
    """plan.partials (and, for the positive control, valid_since) filled with the current pattern before every clipped step."""

    def __init__(self, monkeypatch, also_valid_since=False):
        super().__init__()
        from orienmask_amd import optim as O
        real = getattr(O._Plan.clip_buffers, "real", O._Plan.clip_buffers)      # a second instance replaces the first
        me = self

        def clip_buffers(plan):
            first = plan.partials is None
            partials, valid_since = real(plan)
            fill(partials, me.value)
            if also_valid_since and first:
                fill(valid_since, me.value)
            return partials, valid_since

        clip_buffers.real = real
        monkeypatch.setattr(O._Plan, "clip_buffers", clip_buffers)


def _sgd_outputs(steps):
    out = {}
    for s, (ps, bufs, shadows, updates) in enumerate(steps):
        for i, p in enumerate(ps):
            if bufs[i] is not None:
                out["buf%d_%d" % (s, i)] = bufs[i]          # in front of the parameter it moves: the first difference names the cause
            out["p%d_%d" % (s, i)] = p
            if shadows is not None:
                out["ema%d_%d" % (s, i)] = shadows[i]
        if updates is not None:
            out["updates%d" % s] = np.int64(updates)
    return out


@pytest.mark.parametrize("name", ["clip_below_one", "skip"])
def test_sgd_partials(dev, monkeypatch, name):
    """om_sgd_clip_ema_step and om_sgd_clip_step (the same case without the average) with plan.partials poisoned before every
    step; momentum buffers and shadows come from torch.empty_like and are poisoned too.  Expectation: test_ema's yardstick."""
    import ema_cases as K
    import optim_np as N
    from test_ema import _check_buffers, _run
    case, want = K.CASES[name], K.reference(name)
    clip = _ClipBuffers(monkeypatch)
    fresh = FreshAllocations()
    for ema in (True, False):
        def run():
            with fresh:
                return _sgd_outputs(_run(dev, case, ema=ema)[0])

        base = agree(run, [clip, fresh])
        for s, (wp, wb, we, wk, _) in enumerate(want):
            for i in range(len(wp)):
                assert N.same_bits(base["p%d_%d" % (s, i)], wp[i]), (name, ema, s, "parameter", i)
                if ema:
                    assert N.same_bits(base["ema%d_%d" % (s, i)], we[i]), (name, s, "shadow", i)
            _check_buffers([base.get("buf%d_%d" % (s, i)) for i in range(len(wp))], wb, (name, ema, s))
            if ema:
                assert int(base["updates%d" % s]) == wk


def test_valid_since_is_a_real_dependence(dev, monkeypatch):
    """The positive control.  include/orienmask_hip.h: valid_since of om_sgd_clip_step is "zeroed by the caller once" -- the one
    kind of word the contract lets an entry trust.  With nonfinite='skip' and a non-zero dampening, a valid_since of 0x01 bytes says
    "an update was applied at step 72340172838076673": the first step then blends the gradient into the (zero) buffer with
    1 - dampening instead of copying it.  agree() must report exactly that: the tool sees a dependence where there is one."""
    import ema_cases as K
    import optim_np as N
    from test_ema import _run
    case = K._random_case(21, [1003, 18], steps=1, hypers=N.HYPER_SETS["dampening"], max_norm=1.0e6, nonfinite="skip")
    assert case["hypers"]["dampening"] != 0 and case["hypers"]["momentum"] != 0
    clip = _ClipBuffers(monkeypatch, also_valid_since=True)

    def run():
        return _sgd_outputs(_run(dev, case, ema=False)[0])

    with pytest.raises(WorkspaceDependence) as e:
        agree(run, [clip], patterns=(0x00, 0x01))
    assert e.value.pattern == 0x01 and e.value.output.startswith("buf0_"), str(e.value)
    clip_only = _ClipBuffers(monkeypatch)           # partials alone: no dependence (valid_since zeroed by the caller, as asked)
    agree(run, [clip_only], patterns=PATTERNS)
