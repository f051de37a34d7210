"""CPU tests of the amp audit's harness (tests/backward_audit.py, its amp='bf16' part; the GPU audit is tests/test_amp_audit.py).

No GPU: the models are built with amp='bf16', conv_forward='hip', conv_grad='hip', route_backend='hip' and run on CPU tensors with
stand-ins behind the recording wrappers on orienmask_amd.train's conv2d_bf16, conv_bn_leaky_frozen, bn_leaky, upsample_concat and
split_channels.  The stand-ins have those functions' signatures and the arithmetic the headers state: float32 accumulation on the
widened operands, the weight rounded with bf16_np.quantise, dw not rounded, one bf16_np.round_bits on every bf16 output, the dy of a
float32-output head rounded once.  Both models are captured completely, and every tie, rounding identity, bar and chaining check
passes.  Then nine corruptions of in-network records are each rejected by the check named in its test; pytest -s prints by what
factor the bar-based ones miss their bars."""
import numpy as np
import pytest
import torch

import backward_audit as A
import bf16_np as Q
import conv_grad_np as G
from orienmask_amd import synth, train

TEETH = 8.0        # test_backward_audit_cpu's: a corruption judged by a bar must miss it by at least this factor
AMP = dict(backend="hip", conv_backend="torch", amp="bf16", conv_forward="hip", conv_grad="hip", route_backend="hip")
CASES = {"plus-96-b2": ("OrienMaskYOLOFPNPlus", (2, 96, 96), {}), "yolo-96-b2": ("OrienMaskYOLO", (2, 96, 96), {}),
         "plus-frozen2-64-b2": ("OrienMaskYOLOFPNPlus", (2, 64, 64), dict(frozen_stages=2))}
_CAPTURES = {}      # id -> (Capture, net): computed once, the records' inputs are never modified


def _capture(cid):
    if cid not in _CAPTURES:
        model, (B, H, W), kw = CASES[cid]
        net = getattr(train, model)(3, 80, **dict(AMP, **kw))
        net.load_state_dict(synth.synth_state_dict(8, obj_bias=-16.0, head_gain=4.0, model=model), strict=True)
        net.train()
        assert not torch.backends.cudnn.deterministic
        cap = A.run_step(net, synth.synth_image_batch(31, B, H, W), A.standin_targets, A.cotangent_backward(5), deterministic=False)
        _CAPTURES[cid] = cap, net
    return _CAPTURES[cid]


def _audit(cid, cap, model):
    return A.amp_audit(cid, cap, model, A.cpu_amp_conv_rerun, A.cpu_amp_block_rerun, A.cpu_frozen_rerun, A.cpu_amp_route_rerun,
                       emit=lambda text: None)


def _is(a, dtype):
    return a is not None and a.dtype == dtype


@pytest.mark.parametrize("cid", ["plus-96-b2", "yolo-96-b2"])
def test_harness_captures_every_node_of_the_amp_step_and_passes_on_the_stand_ins(cid):
    """Every convolution, block and route node of expected_nodes is recorded once at 2 x 3 x 96 x 96: bf16 tensors as uint16 bits with
    the type remembered, the float32 quantities float32, a head's y and dy float32 with round_bits(dy) beside it; every tie,
    rounding identity, bar and chaining check passes."""
    cap, net = _capture(cid)
    model = CASES[cid][0]
    blocks, convs, routes = A.expected_nodes(model)
    assert sorted(r["name"] for r in cap.blocks) == sorted(blocks) and len(blocks) == {"OrienMaskYOLOFPNPlus": 86, "OrienMaskYOLO": 83}[model]
    assert sorted(r["name"] for r in cap.convs) == sorted(convs) and len(convs) == len(blocks) + 4 and not cap.frozen
    assert [r["name"] for r in cap.cats + cap.splits] == [r.name for r in routes]
    assert cap.head_dtypes == ["float32"] * 6 and cap.image.dtype == np.float32
    params = dict(net.named_parameters())
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in params.values())
    for r in cap.convs:
        head, first = r["bias"], r["name"] == "backbone.conv1"
        assert r["forward"] == "hip" and r["backward"] == "hip" and r["out_dtype"] == ("float32" if head else "bfloat16"), r["name"]
        assert _is(r["x"], np.uint16) and _is(r["w"], np.float32) and _is(r["y"], np.float32 if head else np.uint16), r["name"]
        assert _is(r["dy"], r["y"].dtype) and _is(r["dy_bits"], np.uint16) and r["dy"].shape == r["y"].shape, r["name"]
        assert (r["dx"] is None) == first and (first or _is(r["dx"], np.uint16)) and r["x_requires_grad"] != first, r["name"]
        assert _is(r["dw"], np.float32) and (r["db"] is not None) == head and (not head or _is(r["db"], np.float32)), r["name"]
        assert set(r["bf16"]) == {"x"} | (set() if head else {"y", "dy"}) | (set() if first else {"dx"}), (r["name"], r["bf16"])
        if head:          # the cotangent of a head is not bf16-valued: the rounding in the node's backward is a real one
            assert not np.array_equal(Q.widen(r["dy_bits"]), r["dy"]), r["name"]
        else:
            assert r["dy_bits"] is r["dy"]
        prefix = r["name"] + (".conv_block.0" if r["name"] in blocks else "")
        assert A.same_bits(r["dw"], params[prefix + ".weight"].grad.numpy()) and A.same_bits(r["w"], params[prefix + ".weight"].detach().numpy())
    assert sum(r["bias"] for r in cap.convs) == 4
    for r in cap.blocks:
        assert all(_is(r[k], np.uint16) for k in ("h", "y", "dy", "dx")), r["name"]
        assert all(_is(r[k], np.float32) for k in ("gamma", "beta", "rm0", "rv0", "rm", "rv", "dgamma", "dbeta")), r["name"]
        residual = r["name"].endswith(".conv.1")
        assert (r["res"] is not None) == residual and (not residual or (_is(r["res"], np.uint16) and _is(r["dres"], np.uint16))), r["name"]
        assert r["training"] and r["nbt"] == r["nbt0"] + 1
    for r in cap.cats:
        assert _is(r["y"], np.uint16) and _is(r["dy"], np.uint16), r["name"]
        assert all(_is(s, np.uint16) and _is(g, np.uint16) and g.shape == s.shape for s, g in zip(r["srcs"], r["dsrc"])), r["name"]
    for r in cap.splits:          # orien_head.5 leaves its convolution as float32: the split is the float32 node
        assert _is(r["x"], np.float32) and _is(r["dx"], np.float32) and all(_is(o, np.float32) for o in r["outs"]), r["name"]
    failures, worst = _audit(cid, cap, model)
    assert not failures, "\n".join(failures)
    assert {k[0] for k in worst} == {"conv", "block"} and {k[1] for k in worst if k[0] == "conv"} == {"y", "dx", "dw", "db"}


def test_a_bf16_tensor_and_a_float32_tensor_of_the_same_values_differ():
    """same_bits compares bits of like dtypes: bf16 bits against the float32 tensor of the same values is a difference, never a
    cast."""
    bits = Q.round_bits(np.array([1.0, -2.5, 3.0], np.float32))
    assert A.same_bits(bits, bits.copy()) and not A.same_bits(bits, Q.widen(bits)) and not A.same_bits(Q.widen(bits), bits)
    assert not A.same_bits(bits, bits.view(np.int16))
    t = torch.tensor([1.0, -2.5, 3.0]).to(torch.bfloat16)
    assert A.same_bits(A._as_numpy(t), bits) and A.same_bits(A.bits_of(A.bf16_tensor(bits)), bits)


def test_frozen_blocks_are_recorded_as_one_node_each():
    """frozen_stages=2: backbone.conv1 and stage conv2 (4 layers) are one node each with x, w, the BatchNorm's parameters and running
    statistics, the residual and y; nothing of theirs takes a gradient; backbone.conv3.0, the first trainable layer, owes no dx;
    every tie, the fused block's identity, the bars and the chain of bits hold."""
    cap, net = _capture("plus-frozen2-64-b2")
    blocks, convs, _ = A.expected_nodes("OrienMaskYOLOFPNPlus")
    want = ["backbone.conv1", "backbone.conv2.0", "backbone.conv2.1.conv.0", "backbone.conv2.1.conv.1"]
    assert [r["name"] for r in cap.frozen] == want
    assert sorted(r["name"] for r in cap.convs + cap.frozen) == sorted(convs)
    assert sorted(r["name"] for r in cap.blocks + cap.frozen) == sorted(blocks)
    assert [r["x_name"] for r in cap.frozen] == [None] + want[:3] and [r["res_name"] for r in cap.frozen] == [None, None, None, want[1]]
    for r in cap.frozen:
        assert all(_is(r[k], np.uint16) for k in ("x", "y")) and all(_is(r[k], np.float32) for k in ("w", "gamma", "beta", "rm0", "rv0"))
        assert not r["training"]
    first = next(r for r in cap.convs if r["name"] == "backbone.conv3.0")
    assert first["x_name"] == want[3] and not first["x_requires_grad"] and first["dx"] is None and first["dw"] is not None
    assert A.conv_wants(A.amp_conv_as_f32(first)) == ("y", "dw")
    assert all((p.grad is None) == any(n.startswith(w + ".") for w in want) for n, p in net.named_parameters())
    failures, worst = _audit("plus-frozen2-64-b2", cap, "OrienMaskYOLOFPNPlus")
    assert not failures, "\n".join(failures)
    assert ("frozen", "y", "element") in worst and ("frozen", "running_var", "scale") in worst


def test_a_frozen_block_that_touches_a_buffer_is_refused_at_capture():
    net = train.OrienMaskYOLOFPNPlus(3, 80, **dict(AMP, frozen_stages=1)).train()

    def touching(x, weight, bn, **kw):
        bn.num_batches_tracked.add_(1)
        return A.standin_conv_bn_leaky_frozen(x, weight, bn, **kw)

    def targets(cap):
        return [t if t[1] != "conv_bn_leaky_frozen" else t[:3] + (touching,) for t in A.standin_targets(cap)]
    with pytest.raises(AssertionError, match="touched its BatchNorm's buffers"):
        A.run_step(net, synth.synth_image_batch(31, 1, 32, 32), targets, A.cotangent_backward(5), deterministic=False)


# ---------------------------------------------------------------------------------------------------------------- teeth
PLUS = "plus-96-b2"


def _conv(name, cid=PLUS):
    return next(r for r in _capture(cid)[0].convs if r["name"] == name)


def _failed(exact):
    return sorted((e.what, e.check) for e in exact if not e.ok)


def _clean(rec):
    """The re-run of a convolution record, as copies; it passes everything as it is."""
    again = {k: v.copy() for k, v in A.cpu_amp_conv_rerun(rec).items()}
    untied, exact, scores = A.amp_conv_findings(rec, again)
    assert not untied and not _failed(exact) and all(A.over_bar(s) <= 1 for s in scores), rec["name"]
    return again


def _over(scores, grad, metric):
    s, = [s for s in scores if s.grad == grad and s.metric == metric]
    print("%-28s %-4s %-8s corrupted %.3g  torch-cpu %.3g  bar %.3g  -> %.1f x the bar" % (s.node, s.grad, s.metric, s.err, s.yard, s.bar,
                                                                                        A.over_bar(s)))
    return A.over_bar(s)


def _operands(rec, **kw):
    f = A.amp_conv_as_f32(rec)
    return dict(dict(x=f["x"], w=f["w"], dy=f["dy"], stride=rec["stride"], ksize=rec["ksize"]), **kw)


@pytest.mark.parametrize("name", ["backbone.conv2.0", "neck8.3", "orien_head.4"])
def test_teeth_y_truncated_instead_of_rounded(name):
    """The bf16 y as the upper half of the float32 y (round toward zero): the one-rounding identity rejects it; so does the tie."""
    rec = _conv(name)
    again = _clean(rec)
    again["y16"] = (again["y32"].view(np.uint32) >> 16).astype(np.uint16)
    share = float((again["y16"] != Q.round_bits(again["y32"])).mean())
    assert 0.3 < share < 0.7          # about half of all elements round up
    untied, exact, scores = A.amp_conv_findings(rec, again)
    assert _failed(exact) == [("y", "rounding")] and untied == ["y"]
    assert all(A.over_bar(s) <= 1 for s in scores)          # the float32 quantities are untouched


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv4.2.conv.0", "neck8.3", "bbox_head16.1"])
def test_teeth_dx_with_the_unrounded_master_weight(name):
    """dx from the float32 master weight instead of quantise(w), what the forward multiplied by: both float64 metrics."""
    rec = _conv(name)
    again = _clean(rec)
    again["dx32"] = G.gradients(_operands(rec, w=rec["w"]), torch.float32, ("dx",))["dx"]
    again["dx16"] = Q.round_bits(again["dx32"])
    _, exact, scores = A.amp_conv_findings(rec, again)
    assert not _failed(exact)          # rounded once, so only the float64 judge can see it
    assert _over(scores, "dx", "element") >= TEETH and _over(scores, "dx", "scale") >= TEETH
    assert all(A.over_bar(s) <= 1 for s in scores if s.grad != "dx")


@pytest.mark.parametrize("name", ["bbox_head32.1", "bbox_head8.1", "orien_head.5"])
def test_teeth_a_heads_dw_from_the_unrounded_float32_dy(name):
    """A float32-output head whose dw (and db) is summed from the float32 dy that reached it, not from round_bits(dy): the tie breaks
    and both float64 metrics of dw miss their bars."""
    rec = _conv(name)
    assert rec["out_dtype"] == "float32" and rec["dy"].dtype == np.float32
    again = _clean(rec)
    again.update(G.gradients(_operands(rec, dy=rec["dy"]), torch.float32, ("dw", "db")))
    untied, _, scores = A.amp_conv_findings(rec, again)
    assert untied == ["dw", "db"]
    assert _over(scores, "dw", "scale") >= TEETH and _over(scores, "dw", "element") >= TEETH


@pytest.mark.parametrize("name", ["backbone.conv1", "backbone.conv2.0", "backbone.conv5.3.conv.1", "neck32.4", "neck4.0", "bbox_head16.1"])
def test_teeth_dw_rounded_to_bf16(name):
    """dw rounded to bf16 and widened, which is what conv2d_bf16_backward(backend='torch') returns: the bars separate a float32
    accumulated dw from a bf16 one.  Both metrics."""
    rec = _conv(name)
    again = _clean(rec)
    again["dw"] = Q.quantise(again["dw"])
    untied, _, scores = A.amp_conv_findings(rec, again)
    assert untied == ["dw"]
    assert _over(scores, "dw", "scale") >= TEETH and _over(scores, "dw", "element") >= TEETH
    assert all(A.over_bar(s) <= 1 for s in scores if s.grad != "dw")


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv4.0", "backbone.conv6.0"])
def test_teeth_stride_2_dx_without_its_last_odd_column(name):
    """dx of a stride-2 layer whose last input column (odd index W - 1: the parity class with one column tap) is not written but
    left as zeros: the per-element metric."""
    rec = _conv(name)
    assert rec["stride"] == 2 and rec["x"].shape[3] % 2 == 0
    again = _clean(rec)
    again["dx32"][:, :, :, -1] = 0
    again["dx16"] = Q.round_bits(again["dx32"])
    _, exact, scores = A.amp_conv_findings(rec, again)
    assert not _failed(exact) and _over(scores, "dx", "element") >= TEETH


@pytest.mark.parametrize("name", ["backbone.conv2.0", "backbone.conv5.3.conv.1", "neck32.4", "neck4.0", "orien_head.4"])
def test_teeth_dw_without_the_last_output_pixel_of_the_batch(name):
    """dw summed without the last output pixel of the last image (the tail of the last chunk of pixels): the per-element metric."""
    rec = _conv(name)
    again = _clean(rec)
    dy = A.amp_conv_as_f32(rec)["dy"].copy()
    dy[-1, :, -1, -1] = 0
    again["dw"] = G.gradients(_operands(rec, dy=dy), torch.float32, ("dw",))["dw"]
    _, _, scores = A.amp_conv_findings(rec, again)
    assert _over(scores, "dw", "element") >= TEETH


def test_teeth_a_frozen_block_that_used_batch_statistics():
    """The fused frozen block normalised with the batch's statistics instead of the running ones: the exact identity rejects it (and
    the tie)."""
    cap = _capture("plus-frozen2-64-b2")[0]
    for rec in cap.frozen:
        again = A.cpu_frozen_rerun(rec)
        untied, exact, scores = A.frozen_findings(rec, again)
        assert not untied and not _failed(exact) and all(A.over_bar(s) <= 1 for s in scores), rec["name"]
        again["y"] = A.cpu_frozen_rerun(rec, training=True)["y"]
        untied, exact, _ = A.frozen_findings(rec, again)
        assert _failed(exact) == [("y", "identity")] and untied == ["y"], rec["name"]


@pytest.mark.parametrize("name,i", [("cat.neck4", 0), ("cat.neck4", 1), ("cat.neck16", 0)])
def test_teeth_a_bf16_route_gradient_rounded_per_addend(name, i):
    """A source gradient whose block sum is rounded to bf16 after every addition instead of once at the end: the bit check."""
    cap = _capture(PLUS)[0]
    rec = next(r for r in cap.cats if r["name"] == name)
    again = A.cpu_amp_route_rerun(rec)
    assert not A.route_differing(rec, again) and not _failed(A.judge_route(rec, again))
    s, c = rec["scales"][i], rec["srcs"][i].shape[1]
    off = sum(a.shape[1] for a in rec["srcs"][:i])
    dy = Q.widen(rec["dy"])
    B, _, H, W = dy.shape
    blk = dy[:, off:off + c].reshape(B, c, H // s, s, W // s, s)
    acc = blk[:, :, :, 0, :, 0].copy()
    for r in range(s):
        for q in range(s):
            if r or q:
                acc = Q.quantise((acc + blk[:, :, :, r, :, q]).astype(np.float32))
    again["dsrc"] = list(again["dsrc"])
    again["dsrc"][i] = Q.round_bits(acc)
    assert _failed(A.judge_route(rec, again)) == [("dsrc%d" % i, "bits")]
    assert A.route_differing(rec, again) == ["dsrc%d" % i]


def test_teeth_one_bit_flipped_in_a_bf16_y():
    """The lowest bit of one element of a bf16 y: the tie of a convolution, of a block and of a concat, and the chain of bits."""
    rec = _conv("neck8.1")
    again = _clean(rec)
    again["y16"].flat[5] ^= 1
    untied, exact, scores = A.amp_conv_findings(rec, again)
    assert untied == ["y"] and all(A.over_bar(s) <= 1 for s in scores)
    cap = _capture(PLUS)[0]
    blk = next(r for r in cap.blocks if r["name"] == "backbone.conv3.1.conv.1")
    again = A.cpu_amp_block_rerun(blk)
    assert not A.amp_block_findings(blk, again)[0]
    again["bf16"]["y"] = again["bf16"]["y"].copy()
    again["bf16"]["y"].flat[7] ^= 1
    untied, exact, _ = A.amp_block_findings(blk, again)
    assert untied == ["y"] and _failed(exact) == [("y", "rounding")]
    cat = next(r for r in cap.cats if r["name"] == "cat.neck8")
    again = A.cpu_amp_route_rerun(cat)
    again["y"] = again["y"].copy()
    again["y"].flat[11] ^= 1
    assert A.route_differing(cat, again) == ["y"] and _failed(A.judge_route(cat, again)) == [("y", "bits")]
    assert not A.amp_chaining_faults(cap)
    h = blk["h"]
    try:
        blk["h"] = h.copy()
        blk["h"].flat[3] ^= 1
        assert A.amp_chaining_faults(cap) == ["backbone.conv3.1.conv.1: h is not the convolution's y"]
    finally:
        blk["h"] = h
    first = _conv("backbone.conv1")
    x = first["x"]
    try:
        first["x"] = (Q.widen(x).view(np.uint32) >> 16).astype(np.uint16) ^ 1          # any other cast of the image
        assert A.amp_chaining_faults(cap) == ["backbone.conv1: x is not round_bits(image)"]
    finally:
        first["x"] = x
