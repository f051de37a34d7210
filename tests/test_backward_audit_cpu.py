"""CPU tests of the backward audit's harness (tests/backward_audit.py): it captures every node of both training models, passes on
torch's own float32 arithmetic, and its judge rejects seven corrupted float32 results on in-network inputs by a wide margin.  No GPU:
the models run with torch-CPU float32 behind the same wrappers on orienmask_amd.train's globals that the GPU audit uses, and once with
backend='torch' and the wrappers on torch.nn.functional."""
import numpy as np
import pytest
import torch

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


_CAPTURES = {}      # id -> Capture: computed once, the records' inputs are never modified


def _capture(cid):
    if cid not in _CAPTURES:
        model, (B, H, W), wseed, wiring = {"plus-96-b2": ("OrienMaskYOLOFPNPlus", (2, 96, 96), 8, "hip"),
                                           "yolo-64x96-b2": ("OrienMaskYOLO", (2, 64, 96), 8, "hip"),
                                           "plus-64-b1-torch": ("OrienMaskYOLOFPNPlus", (1, 64, 64), 8, "torch")}[cid]
        if wiring == "hip":
            net, targets = _net(model, wseed, backend="hip", conv_backend="hip"), _hip_wiring
        else:
            net, targets = _net(model, wseed, backend="torch"), A.torch_targets
        _CAPTURES[cid] = A.run_step(net, synth.synth_image_batch(31, B, H, W), targets, A.cotangent_backward(5)), net
    return _CAPTURES[cid]


@pytest.mark.parametrize("cid,model", [("plus-96-b2", "OrienMaskYOLOFPNPlus"), ("yolo-64x96-b2", "OrienMaskYOLO"),
                                       ("plus-64-b1-torch", "OrienMaskYOLOFPNPlus")])
def test_harness_captures_every_node_and_passes_on_float32(cid, model):
    """Every ConvBNLeaky block and every convolution of arch.model_convs is recorded once, with its dy, its own
    input gradient (none for backbone.conv1) and its parameter gradients; torch's float32 ties with its own isolated re-run and
    stays inside every bar."""
    cap, net = _capture(cid)
    blocks, convs = A.expected_nodes(model)
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
        prefix = r["name"] + (".conv_block.0" if r["name"] in blocks else "")
        assert A.same_bits(r["dw"], params[prefix + ".weight"].grad.numpy())
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


def test_eval_mode_blocks_are_recorded_as_such():
    net = train.OrienMaskYOLOFPNPlus(3, 80, backbone_batchnorm_eval=True, backend="hip", conv_backend="hip").train()
    cap = A.run_step(net, synth.synth_image_batch(31, 2, 32, 32), _hip_wiring, A.cotangent_backward(5))
    for r in cap.blocks:
        assert r["training"] == (not r["name"].startswith("backbone.")), r["name"]
        assert r["nbt"] == r["nbt0"] + int(r["training"])
        if not r["training"]:
            assert A.same_bits(r["rm"], r["rm0"]) and A.same_bits(r["rv"], r["rv0"])


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
