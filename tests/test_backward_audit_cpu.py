"""CPU tests of the backward audit's harness (tests/backward_audit.py): it captures every node of both training models, passes on
torch's own float32 arithmetic, and its judge rejects seven corrupted float32 gradients on in-network inputs by a wide margin.  No GPU:
the models run with torch-CPU float32 behind the same wrappers on orienmask_amd.train's globals that the GPU audit uses, and once with
backend='torch' and the wrappers on torch.nn.functional.  The same for the all-HIP step (conv_forward='hip', route_backend='hip'):
torch float32 behind all four wrappers, a frozen backbone, a split output left out of the backward, and eight more corruptions: three
of a forward y miss their bars by TEETH, four of a route node fail their bit checks, and one unit in the last place of a y breaks
the tie."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_audit as A
import bn_act_np as N
import conv_grad_np as G
from orienmask_amd import synth, train

TEETH = 8.0        # every corruption must miss its bar by at least this factor (measured: 2.1e3 at the least, pytest -s prints them)


def _net(model, wseed, **kw):
    net = getattr(train, model)(3, 80, **kw)
    net.load_state_dict(synth.synth_state_dict(wseed, obj_bias=-16.0, head_gain=4.0, model=model), strict=True)
    return net.train()


def _hip_wiring(cap):
    return A.hip_targets(cap, conv2d=A.torch_conv2d, bn_leaky=A.torch_bn_leaky)


def _allhip_wiring(cap):
    """torch float32 behind all four wrappers: a model with conv_forward='hip' and route_backend='hip' as well."""
    return A.hip_targets(cap, conv2d=A.torch_conv2d, bn_leaky=A.torch_bn_leaky, routes=True, upsample_concat=A.torch_upsample_concat,
                         split_channels=A.torch_split_channels)


ALL_HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")      # tests/test_trainer.py's HIP
_CAPTURES = {}      # id -> Capture: computed once, the records' inputs are never modified


def _capture(cid):
    if cid not in _CAPTURES:
        model, (B, H, W), wseed, wiring = {"plus-96-b2": ("OrienMaskYOLOFPNPlus", (2, 96, 96), 8, "hip"),
                                           "yolo-64x96-b2": ("OrienMaskYOLO", (2, 64, 96), 8, "hip"),
                                           "plus-64-b1-torch": ("OrienMaskYOLOFPNPlus", (1, 64, 64), 8, "torch"),
                                           "plus-allhip-64-b2": ("OrienMaskYOLOFPNPlus", (2, 64, 64), 8, "allhip"),
                                           "yolo-allhip-64x96-b2": ("OrienMaskYOLO", (2, 64, 96), 8, "allhip")}[cid]
        if wiring == "hip":
            net, targets = _net(model, wseed, backend="hip", conv_backend="hip"), _hip_wiring
        elif wiring == "allhip":
            net, targets = _net(model, wseed, **ALL_HIP), _allhip_wiring
        else:
            net, targets = _net(model, wseed, backend="torch"), A.torch_targets
        _CAPTURES[cid] = A.run_step(net, synth.synth_image_batch(31, B, H, W), targets, A.cotangent_backward(5)), net
    return _CAPTURES[cid]


@pytest.mark.parametrize("cid,model", [("plus-96-b2", "OrienMaskYOLOFPNPlus"), ("yolo-64x96-b2", "OrienMaskYOLO"),
                                       ("plus-64-b1-torch", "OrienMaskYOLOFPNPlus"), ("plus-allhip-64-b2", "OrienMaskYOLOFPNPlus"),
                                       ("yolo-allhip-64x96-b2", "OrienMaskYOLO")])
def test_harness_captures_every_node_and_passes_on_float32(cid, model):
    """Every ConvBNLeaky block and every convolution of arch.model_convs is recorded once, with its y, its dy, its own
    input gradient (none for backbone.conv1) and its parameter gradients; torch's float32 ties with its own isolated re-run and
    stays inside every bar.  With all four options 'hip': every convolution is recorded as a HIP forward and its y is tied and
    judged too, every expected route node is recorded once with all its gradients and passes every bit check, and the chain of
    bits from node to node is whole."""
    cap, net = _capture(cid)
    allhip = "allhip" in cid
    blocks, convs, routes = A.expected_nodes(model)
    assert sorted(r["name"] for r in cap.blocks) == sorted(blocks) and len(blocks) == {"OrienMaskYOLOFPNPlus": 86, "OrienMaskYOLO": 83}[model]
    assert sorted(r["name"] for r in cap.convs) == sorted(convs) and len(convs) == len(blocks) + 4
    assert sum(r["bias"] for r in cap.convs) == 4
    params = dict(net.named_parameters())
    seen = set()
    missed = []
    for r in cap.convs:
        first = r["name"] == "backbone.conv1"
        assert r["x_requires_grad"] != first and (r["dx"] is None) == first, r["name"]
        assert r["dy"] is not None and r["dw"] is not None and (r["db"] is not None) == r["bias"], r["name"]
        assert r["y"] is not None and r["y"].shape == r["dy"].shape and (r["b"] is not None) == r["bias"], r["name"]
        assert r["forward"] == ("hip" if allhip else "torch") and ("y" in A.conv_wants(r)) == allhip, r["name"]
        prefix = r["name"] + (".conv_block.0" if r["name"] in blocks else "")
        assert A.same_bits(r["dw"], params[prefix + ".weight"].grad.numpy())
        if r["bias"]:
            assert A.same_bits(r["b"], params[prefix + ".bias"].detach().numpy())
        seen.update([prefix + ".weight"] + ([prefix + ".bias"] if r["bias"] else []))
        again = A.torch_conv_rerun(r)
        assert not A.differing(r, again, A.conv_wants(r)), r["name"]
        missed += [s for s in A.judge_conv(r, again) if A.over_bar(s) > 1]
    for r in cap.blocks:
        assert all(r[k] is not None for k in ("dy", "dx", "dgamma", "dbeta")), r["name"]
        residual = r["name"].endswith(".conv.1") and "torch" not in cid       # backend 'torch' adds the residual outside the block
        assert (r["res"] is not None) == residual and (r["dres"] is not None) == residual, r["name"]
        assert r["training"] and r["nbt"] == r["nbt0"] + 1
        seen.update([r["name"] + ".conv_block.1.weight", r["name"] + ".conv_block.1.bias"])
        again = A.torch_block_rerun(r)
        assert not A.differing(r, again, A.BLOCK_TIED), r["name"]
        missed += [s for s in A.judge_block(r, again) if A.over_bar(s) > 1]
    assert seen == set(params)
    assert not missed, missed
    assert not A.chaining_faults(cap)
    if not allhip:
        assert not cap.cats and not cap.splits
        return
    assert not A.route_mismatches(cap, model)
    assert [(len(r.scales), r.scales) for r in routes[:3]] == [(2, (2, 1)), (2, (2, 1)), (4, (8, 4, 2, 1)) if "Plus" in model else (2, (2, 1))]
    assert routes[3].sizes == (6, 6, 6)
    for r in cap.cats:
        assert r["dy"] is not None and all(g is not None and g.shape == s.shape for g, s in zip(r["dsrc"], r["srcs"])), r["name"]
    for r in cap.splits:
        assert r["dx"] is not None and all(d is not None and d.shape == o.shape for d, o in zip(r["dys"], r["outs"])), r["name"]
    for r in cap.cats + cap.splits:
        again = A.torch_route_rerun(r)
        assert not A.route_differing(r, again), r["name"]
        wrong = [e for e in A.judge_route(r, again) if not e.ok]
        assert not wrong, wrong


def test_eval_mode_blocks_are_recorded_as_such():
    net = train.OrienMaskYOLOFPNPlus(3, 80, backbone_batchnorm_eval=True, backend="hip", conv_backend="hip").train()
    cap = A.run_step(net, synth.synth_image_batch(31, 2, 32, 32), _hip_wiring, A.cotangent_backward(5))
    for r in cap.blocks:
        assert r["training"] == (not r["name"].startswith("backbone.")), r["name"]
        assert r["nbt"] == r["nbt0"] + int(r["training"])
        if not r["training"]:
            assert A.same_bits(r["rm"], r["rm0"]) and A.same_bits(r["rv"], r["rv0"])


def _judge_everything(cap):
    """Ties and judges every recorded node against torch's float32 re-runs -> what failed."""
    bad = list(A.chaining_faults(cap))
    for r in cap.convs:
        again = A.torch_conv_rerun(r)
        bad += [(r["name"], k) for k in A.differing(r, again, A.conv_wants(r))] + [s for s in A.judge_conv(r, again) if A.over_bar(s) > 1]
    for r in cap.blocks:
        again = A.torch_block_rerun(r)
        bad += [(r["name"], k) for k in A.differing(r, again, A.block_tied(r))] + [s for s in A.judge_block(r, again) if A.over_bar(s) > 1]
    for r in cap.cats + cap.splits:
        again = A.torch_route_rerun(r)
        bad += [(r["name"], k) for k in A.route_differing(r, again)] + [e for e in A.judge_route(r, again) if not e.ok]
    return bad


def test_a_frozen_backbone_is_recorded_with_forward_results_only():
    """No hook goes on a tensor that does not require grad: the backbone's nodes keep y and no gradient, neck32.0 and skip4 have no
    input gradient, the backbone's features are concat sources without a gradient, and every node is still tied and judged."""
    net = _net("OrienMaskYOLOFPNPlus", 8, **ALL_HIP)
    net.backbone.requires_grad_(False)
    cap = A.run_step(net, synth.synth_image_batch(31, 2, 32, 32), _allhip_wiring, A.cotangent_backward(5))
    assert all((p.grad is not None) == (not n.startswith("backbone.")) for n, p in net.named_parameters())
    for r in cap.convs:
        backbone = r["name"].startswith("backbone.")
        assert r["y"] is not None and (r["dy"] is None) == backbone and (r["dw"] is None) == backbone, r["name"]
        fed = r["name"] in ("neck32.0", "skip4")          # by the backbone alone: no input gradient
        assert (r["dx"] is None) == (backbone or fed), r["name"]
        assert A.conv_wants(r) == (("y",) if backbone else ("y",) + (() if fed else ("dx",)) + ("dw",) + (("db",) if r["bias"] else ()))
    for r in cap.blocks:
        backbone = r["name"].startswith("backbone.")
        assert all((r[k] is None) == backbone for k in ("dy", "dx", "dgamma", "dbeta")) and r["dres"] is None, r["name"]
        assert A.block_tied(r) == (("y", "rm", "rv", "nbt") if backbone else A.BLOCK_TIED)
    assert not A.route_mismatches(cap, "OrienMaskYOLOFPNPlus")
    got = {r["name"]: [g is not None for g in r["dsrc"]] for r in cap.cats}
    assert got == {"cat.neck16": [True, False], "cat.neck8": [True, False], "cat.neck4": [True] * 4}
    assert not _judge_everything(cap)


def _capture_without_orien16():
    def backward(heads):
        used = [i for i in range(6) if i != 3]          # heads: bbox32, orien32, bbox16, orien16, bbox8, orien8
        cot = N.cotangents(5, [t.shape for t in heads])
        torch.autograd.backward([heads[i] for i in used], [torch.from_numpy(cot[i]) for i in used])
    if "no-orien16" not in _CAPTURES:
        net = _net("OrienMaskYOLOFPNPlus", 8, **ALL_HIP)
        _CAPTURES["no-orien16"] = A.run_step(net, synth.synth_image_batch(31, 2, 32, 32), _allhip_wiring, backward), net
    return _CAPTURES["no-orien16"][0]


def test_a_split_output_left_out_of_the_backward_is_recorded_without_a_dy():
    """orien16 takes no part in the backward: its dy is None, and the judge wants exact zeros in its channels of dx."""
    cap = _capture_without_orien16()
    rec, = cap.splits
    assert [d is not None for d in rec["dys"]] == [True, False, True] and not rec["dx"][:, 6:12].any() and rec["dx"][:, :6].any()
    assert not _judge_everything(cap)


# ---------------------------------------------------------------------------------------------------------------- teeth
def _conv(name):
    return next(r for r in _capture("plus-96-b2")[0].convs if r["name"] == name)


def _block(name):
    return next(r for r in _capture("plus-96-b2")[0].blocks if r["name"] == name)


def _worst(scores, grad):
    worst = max((s for s in scores if s.grad == grad), key=A.over_bar)
    print("%-28s %-7s %-8s corrupted %.3g  torch-cpu %.3g  bar %.3g  -> %.1f x the bar" % (worst.node, worst.grad, worst.metric, worst.err,
                                                                                        worst.yard, worst.bar, A.over_bar(worst)))
    return worst


def _f32(rec, want):
    return {k: v.copy() for k, v in G.gradients(A.conv_inputs(rec), torch.float32, want).items()}


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv5.3.conv.1", "neck4.0", "orien_head.4"])
def test_teeth_dw_without_the_last_input_row(name):
    """dw of the lowest-scale output channel computed without the last input row of the last image.  Measured: the scale metric
    6e-3 ... 7e-2 (9.7e3 x its bar at the least), the per-element metric 0.13 ... 0.59 (3.7e4 x at the least)."""
    rec = _conv(name)
    got = _f32(rec, A.conv_wants(rec))
    co = int(np.abs(A.conv_reference(rec)[0]["dw"]).max(axis=(1, 2, 3)).argmin())
    d = A.conv_inputs(rec)
    d["x"] = d["x"].copy()
    d["x"][-1, :, -1, :] = 0
    got["dw"][co] = G.gradients(d, torch.float32, ("dw",))["dw"][co]
    scores = [s for s in A.judge_conv(rec, got) if s.grad == "dw"]
    assert all(A.over_bar(s) >= TEETH for s in scores), scores           # both metrics
    _worst(scores, "dw")
    assert all(A.over_bar(s) <= 1 for s in A.judge_conv(rec, got) if s.grad != "dw")


@pytest.mark.parametrize("name", ["backbone.conv3.1.conv.1", "neck16.1", "orien_head.4"])
def test_teeth_dx_without_a_corner_tap(name):
    """dx of a 3x3 layer without the tap that reaches the first image's corner pixel (0, 0) from the output at (1, 1)."""
    rec = _conv(name)
    assert rec["ksize"] == 3 and rec["stride"] == 1
    got = _f32(rec, A.conv_wants(rec))
    got["dx"][0, :, 0, 0] -= rec["dy"][0, :, 1, 1] @ rec["w"][:, :, 0, 0]
    assert A.over_bar(_worst(A.judge_conv(rec, got), "dx")) >= TEETH


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv4.2.conv.0", "neck8.3", "bbox_head16.1"])
def test_teeth_dx_from_bfloat16_operands(name):
    """dx from operands rounded to bfloat16 before the products (exact sums): what a reduced-precision matrix instruction gives.
    Measured: 2e-3 ... 3e-3 of scale, 8e-3 ... 1e-2 per element; 2.1e3 x the bar at the least -- the smallest margin of the seven."""
    rec = _conv(name)
    got = _f32(rec, A.conv_wants(rec))
    w, dy = (torch.from_numpy(rec[k]).bfloat16().double() for k in ("w", "dy"))
    got["dx"] = torch.nn.grad.conv2d_input(rec["x"].shape, w, dy, stride=rec["stride"], padding=rec["ksize"] // 2).float().numpy()
    scores = [s for s in A.judge_conv(rec, got) if s.grad == "dx"]
    assert all(A.over_bar(s) >= TEETH for s in scores), scores           # both metrics
    _worst(scores, "dx")


def _block_f32(rec):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in A.torch_block_rerun(rec).items()}


def _truth_backward(rec, positive=None, images=None):
    truth = A.block_reference(rec)[0]
    sl = slice(None, images)
    pos = truth["z"] > 0 if positive is None else positive
    return N.backward(rec["h"][sl], rec["dy"][sl], rec["gamma"], truth["mean"], truth["invstd"], pos[sl], rec["training"], rec["slope"])


BLOCKS = ["backbone.conv1", "backbone.conv4.5.conv.1", "neck32.2", "orien_head.3"]


@pytest.mark.parametrize("name", BLOCKS)
def test_teeth_dh_without_the_dgamma_term(name):
    """dh without the xhat * dgamma / n term in the channel whose dh is smallest.  The per-tensor metric may not see one low-scale
    channel; the per-channel metric must."""
    rec = _block(name)
    got = _block_f32(rec)
    truth = A.block_reference(rec)[0]
    dx, dgamma, _ = _truth_backward(rec)
    c = int(np.abs(dx).max(axis=(0, 2, 3)).argmin())
    n = rec["h"].size // rec["h"].shape[1]
    xhat = (rec["h"][:, c].astype(np.float64) - truth["mean"][c]) * truth["invstd"][c]
    got["dx"][:, c] += (rec["gamma"][c] * truth["invstd"][c] * xhat * dgamma[c] / n).astype(np.float32)
    worst = _worst(A.judge_block(rec, got), "dh")
    assert worst.metric == "channel" and A.over_bar(worst) >= TEETH


@pytest.mark.parametrize("name", BLOCKS)
def test_teeth_dgamma_over_one_image_less(name):
    rec = _block(name)
    got = _block_f32(rec)
    got["dgamma"] = _truth_backward(rec, images=rec["h"].shape[0] - 1)[1].astype(np.float32)
    assert A.over_bar(_worst(A.judge_block(rec, got), "dgamma")) >= TEETH


@pytest.mark.parametrize("name", BLOCKS)
def test_teeth_slope_on_the_positive_side_of_one_channel(name):
    """The backward of one channel multiplies by the slope where z > 0 and by 1 elsewhere; the forward (and so the mask) is right."""
    rec = _block(name)
    got = _block_f32(rec)
    c = rec["h"].shape[1] // 2
    pos = got["y0"] > 0
    pos[:, c] = ~pos[:, c]
    dx, dgamma, dbeta = _truth_backward(rec, positive=pos)
    got["dx"][:, c], got["dgamma"][c], got["dbeta"][c] = dx[:, c], dgamma[c], dbeta[c]
    scores = A.judge_block(rec, got)
    for k in ("dh", "dgamma", "dbeta"):
        assert A.over_bar(_worst(scores, k)) >= TEETH


def test_teeth_dbias_from_the_previous_calls_dy():
    """A head's dbias summed from the dy of the head whose backward ran before it (a stale buffer's stand-in)."""
    rec, before = _conv("bbox_head16.1"), _conv("bbox_head8.1")
    got = _f32(rec, A.conv_wants(rec))
    got["db"] = before["dy"].sum(axis=(0, 2, 3), dtype=np.float32)
    assert A.over_bar(_worst(A.judge_conv(rec, got), "db")) >= TEETH


def test_tie_fails_on_one_unit_in_the_last_place():
    rec = _conv("neck8.1")
    again = A.torch_conv_rerun(rec)
    assert not A.differing(rec, again, A.conv_wants(rec))
    i = int(np.abs(again["dw"]).argmax())
    again["dw"] = again["dw"].copy()
    again["dw"].flat[i] = np.nextafter(again["dw"].flat[i], np.float32(np.inf))
    assert A.differing(rec, again, A.conv_wants(rec)) == ["dw"]
    assert all(A.over_bar(s) <= 1 for s in A.judge_conv(rec, again))          # far below what (b) can see
    blk = _block("backbone.conv3.1.conv.1")
    again = _block_f32(blk)
    assert not A.differing(blk, again, A.BLOCK_TIED)
    again["dx"].flat[7] = np.nextafter(again["dx"].flat[7], np.float32(np.inf))
    assert A.differing(blk, again, A.BLOCK_TIED) == ["dx"]
    blk = dict(blk, dres=again["dx"])
    assert "dres" in A.differing(blk, again, A.BLOCK_TIED)


# ---------------------------------------------------------------------------------------------------------------- teeth: forward and routes
ALLHIP = "plus-allhip-64-b2"          # FPNPlus 64 x 64, B = 2: cat.neck4's scale-8 source is a 2 x 2 map


def _fconv(name):
    return next(r for r in _capture(ALLHIP)[0].convs if r["name"] == name)


def _route(name, cap=None):
    cap = cap or _capture(ALLHIP)[0]
    return next(r for r in cap.cats + cap.splits if r["name"] == name)


def _conv_f32(rec):
    """torch's float32 results at the node (y and the gradients), as copies."""
    return {k: v.copy() for k, v in A.torch_conv_rerun(rec).items()}


def _forward_f32(rec, x=None, w=None, dtype=torch.float32):
    x, w = (torch.from_numpy(rec[k] if v is None else v).to(dtype) for k, v in (("x", x), ("w", w)))
    b = torch.from_numpy(rec["b"]).to(dtype) if rec["b"] is not None else None
    return F.conv2d(x, w, b, rec["stride"], rec["ksize"] // 2)


def _only_y_fails(rec, got):
    scores = A.judge_conv(rec, got)
    assert all(A.over_bar(s) <= 1 for s in scores if s.grad != "y")
    return [s for s in scores if s.grad == "y"]


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv4.0", "backbone.conv6.0"])
def test_teeth_y_without_the_last_input_column(name):
    """y of a stride-2 3x3 layer computed without the taps of the last input column (even widths: the last output column's third
    tap).  Both metrics."""
    rec = _fconv(name)
    assert rec["ksize"] == 3 and rec["stride"] == 2 and rec["x"].shape[3] % 2 == 0
    got = _conv_f32(rec)
    x = rec["x"].copy()
    x[:, :, :, -1] = 0
    got["y"] = _forward_f32(rec, x=x).numpy()
    scores = _only_y_fails(rec, got)
    assert len(scores) == 2 and all(A.over_bar(s) >= TEETH for s in scores), scores
    _worst(scores, "y")


@pytest.mark.parametrize("name", ["backbone.conv5.3.conv.0", "neck16.0", "skip32.0", "orien_head.5"])
def test_teeth_y_of_the_lowest_scale_channel_without_the_last_input_channel(name):
    """y of the lowest-scale output channel of a 1x1 layer without its last input channel.  The per-tensor metric may not see one
    low-scale channel; the per-element metric must."""
    rec = _fconv(name)
    assert rec["ksize"] == 1
    got = _conv_f32(rec)
    co = int(np.abs(A.conv_reference(rec)[0]["y"]).max(axis=(0, 2, 3)).argmin())
    w = rec["w"].copy()
    w[:, -1] = 0
    got["y"][:, co] = _forward_f32(rec, w=w).numpy()[:, co]
    worst = _worst(_only_y_fails(rec, got), "y")
    assert worst.metric == "element" and A.over_bar(worst) >= TEETH


@pytest.mark.parametrize("name", ["backbone.conv1", "backbone.conv3.0", "backbone.conv4.2.conv.0", "neck8.3", "bbox_head16.1"])
def test_teeth_y_from_bfloat16_operands(name):
    """y from operands rounded to bfloat16 before the products (exact sums).  Both metrics."""
    rec = _fconv(name)
    got = _conv_f32(rec)
    x, w = (torch.from_numpy(rec[k]).bfloat16().float().numpy() for k in ("x", "w"))
    got["y"] = _forward_f32(rec, x=x, w=w, dtype=torch.float64).float().numpy()
    scores = _only_y_fails(rec, got)
    assert len(scores) == 2 and all(A.over_bar(s) >= TEETH for s in scores), scores
    _worst(scores, "y")


def _route_f32(rec):
    again = A.torch_route_rerun(rec)
    return {k: ([a.copy() if a is not None else None for a in v] if isinstance(v, list) else (v.copy() if v is not None else None))
            for k, v in again.items()}


def _failed(rec, got):
    return sorted((e.what, e.check) for e in A.judge_route(rec, got) if not e.ok)


def test_teeth_concat_whose_scale_8_source_is_read_one_row_early():
    """cat.neck4's scale-8 source read at row (y + 1) // 8 (the last rows at the last source row): y fails its bit check, and
    nothing else does."""
    rec = _route("cat.neck4")
    assert rec["scales"] == [8, 4, 2, 1] and rec["srcs"][0].shape[2:] == (2, 2)
    got = _route_f32(rec)
    assert not _failed(rec, got)
    c, h = rec["srcs"][0].shape[1], rec["srcs"][0].shape[2]
    rows = np.minimum((np.arange(rec["y"].shape[2]) + 1) // 8, h - 1)
    got["y"][:, :c] = rec["srcs"][0][:, :, rows[:, None], (np.arange(rec["y"].shape[3]) // 8)[None, :]]
    assert _failed(rec, got) == [("y", "bits")]
    assert A.route_differing(rec, got) == ["y"]


@pytest.mark.parametrize("name,i", [("cat.neck4", 0), ("cat.neck4", 1), ("cat.neck16", 0)])
def test_teeth_concat_gradient_summed_column_first(name, i):
    """A source gradient whose s x s block is summed column by column: a valid float32 sum of the same terms, so it stays inside
    within_bound, and not the stated order, so the bit check fails.  The two checks are independent."""
    rec = _route(name)
    s, c = rec["scales"][i], rec["srcs"][i].shape[1]
    off = sum(a.shape[1] for a in rec["srcs"][:i])
    B, _, H, W = rec["dy"].shape
    blk = rec["dy"][:, off:off + c].reshape(B, c, H // s, s, W // s, s)
    acc = blk[:, :, :, 0, :, 0].copy()
    for q in range(s):
        for r in range(s):
            if r or q:
                acc = (acc + blk[:, :, :, r, :, q]).astype(np.float32)
    got = _route_f32(rec)
    got["dsrc"][i] = acc
    assert _failed(rec, got) == [("dsrc%d" % i, "bits")]
    bound = next(e for e in A.judge_route(rec, got) if e.check == "bound")
    print("%-12s dsrc%d scale %d column-first: %s" % (name, i, s, bound.detail))
    assert bound.ok
    got["dsrc"][i] = (acc.astype(np.float64) * (1 + 2.0 ** -12)).astype(np.float32)      # a real error leaves the bound as well
    assert ("dsrc", "bound") in _failed(rec, got)


def test_teeth_split_with_two_outputs_swapped():
    rec = _route("split.orien")
    got = _route_f32(rec)
    assert not _failed(rec, got)
    got["outs"][1], got["outs"][2] = got["outs"][2], got["outs"][1]
    assert _failed(rec, got) == [("out1", "bits"), ("out2", "bits")]
    assert A.route_differing(rec, got) == ["out1", "out2"]


def test_teeth_split_dx_with_stale_values_where_an_output_had_no_gradient():
    """dx keeps what the buffer held before (the previous call's values) in the channels of the output that received no gradient."""
    rec = _route("split.orien", _capture_without_orien16())
    assert [d is not None for d in rec["dys"]] == [True, False, True]
    got = _route_f32(rec)
    assert not _failed(rec, got)
    got["dx"][:, 6:12] = rec["dys"][0]
    assert _failed(rec, got) == [("dx", "bits")]
    got["dx"][:, 6:12] = -0.0          # not even the sign of the zeros may differ
    assert _failed(rec, got) == [("dx", "bits")]


def test_tie_fails_on_one_unit_in_the_last_place_of_a_forward_y():
    rec = _fconv("neck8.1")
    again = _conv_f32(rec)
    assert A.conv_wants(rec)[0] == "y" and not A.differing(rec, again, A.conv_wants(rec))
    i = int(np.abs(again["y"]).argmax())
    again["y"].flat[i] = np.nextafter(again["y"].flat[i], np.float32(np.inf))
    assert A.differing(rec, again, A.conv_wants(rec)) == ["y"]
    assert all(A.over_bar(s) <= 1 for s in A.judge_conv(rec, again))          # far below what (b) can see
    cat = _route("cat.neck8")
    again = _route_f32(cat)
    assert not A.route_differing(cat, again)
    again["y"].flat[11] = np.nextafter(again["y"].flat[11], np.float32(np.inf))
    assert A.route_differing(cat, again) == ["y"] and _failed(cat, again) == [("y", "bits")]
    blk = next(r for r in _capture(ALLHIP)[0].blocks if r["name"] == "neck8.1")
    assert not A.chaining_faults(_capture(ALLHIP)[0])
    h = blk["h"]
    try:
        blk["h"] = again_h = h.copy()
        again_h.flat[3] = np.nextafter(again_h.flat[3], np.float32(np.inf))
        assert A.chaining_faults(_capture(ALLHIP)[0]) == ["neck8.1: h is not the convolution's y"]
    finally:
        blk["h"] = h
