"""Teacher-forced audit of every node of one amp='bf16' training step against float64 (harness: tests/backward_audit.py, its amp part;
the harness itself without a GPU: tests/test_amp_audit_cpu.py; the float32 twin: tests/test_backward_audit.py).

One forward and backward of a training model built with backend='hip', conv_backend='torch', amp='bf16', conv_forward='hip',
conv_grad='hip', route_backend='hip' -- the step whose every node is this package's and which is advertised as bit-repeatable --
runs on the GPU with cudnn.deterministic OFF and recording wrappers on orienmask_amd.train's conv2d_bf16, conv_bn_leaky_frozen,
bn_leaky, upsample_concat and split_channels.  A bf16 tensor is recorded as its uint16 bits.  Every node is then run again alone
through the C ABI, outputs pre-filled with NaN bits, on a workspace of the call's own filled with 0xFF, and

  tie        everything the model's own step produced at the node equals the re-run bit for bit: y, dx (bf16), dw, db (float32) of a
             convolution; y, the running buffers, dh, dgamma, dbeta of a block; y of a fused frozen block; a concat's y and source
             gradients, the split's outputs and dx.  A difference means the model context changed a result: the grow-only workspace
             conv2d_bf16_backward shares with every other call of the stream, the order of grad_input and grad_weight on it,
             dy.to(bfloat16).contiguous() on a head's float32 cotangent, a stale or aliased buffer.
  rounding   no tolerance is introduced for a bf16 quantity; it is judged through the identities include/orienmask_hip.h states.  A
             convolution's bf16 y / dx equals bf16_np.round_bits of the float32-output call on the same operands; a block's bf16 y
             and dh equal round_bits of om_bn_act_forward / _backward on the widened h, dy and residual, and the float32 outputs of the
             two are bit-equal; a frozen block's y equals round_bits of om_bn_act_forward(eval) on the float32-output
             om_conv2d_bf16_forward of the same x and w, residual included; a concat's y is a bit copy and a source gradient
             round_bits of route_np.backward on the widened dy, whose unrounded sums are inside route_np.within_bound.
  float64    the float32 quantities behind those identities go through the float32 audit's judges unchanged: the float32 y, dx and
             dw, db of a convolution through judge_conv on the operands the kernel multiplies -- widen(x), widen(round_bits(dy)),
             quantise(w) -- over the scale and per element, yardstick torch-CPU float32 with oneDNN on and off (for db also
             F.conv2d's own backward), bar 2 x yardstick, floors test_conv_fwd.FLOOR / test_conv_grad.FLOOR; the float32 block
             through judge_block (2 x, dh per channel 4 x, the mask inside BAND on at most FLIP_SHARE, num_batches_tracked exact).
  chaining   backbone.conv1's x has the bits of round_bits(image); every block's h those of its convolution's y; the x of every
             other convolution and frozen block, every concat source, a frozen block's residual and the split's x those of the
             output of the node that made them; the six heads leave the model as float32.

pytest -s prints one line per node, quantity and metric, the worst fraction of its bar per quantity and the node counts and duration
per configuration; those of the first MI355X run are in DESIGN.md 3.30."""
import time

import numpy as np
import pytest
import torch

import backward_audit as A
from test_backward_audit import _loss_backward
from orienmask_amd import lib as omlib, synth, train

pytestmark = pytest.mark.gpu

AMP = dict(backend="hip", conv_backend="torch", amp="bf16", conv_forward="hip", conv_grad="hip", route_backend="hip")
# (id, model, (B, H, W), synth_state_dict seed, cotangent: "cot" = bn_act_np.cotangents or "loss" = the HIP training loss, frozen_stages)
CONFIGS = [
    ("amp-plus-loss-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, "loss", 0),        # the trainer's step; neck32.4 at k = 18 pixels
    ("amp-plus-160x128-b3", "OrienMaskYOLOFPNPlus", (3, 160, 128), 9, "cot", 0),       # non-square, odd batch, a multi-split dw
    ("amp-yolo-64x96-b2", "OrienMaskYOLO", (2, 64, 96), 8, "cot", 0),                  # the two-source cat.neck4
    ("amp-plus-64-b1", "OrienMaskYOLOFPNPlus", (1, 64, 64), 8, "cot", 0),              # 2 x 2 maps: 4-pixel dw chains, x 8 up-sampling
    ("amp-plus-frozen2-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, "cot", 2),      # fused frozen blocks in front of a trainable stage
]
FROZEN2 = ["backbone.conv1", "backbone.conv2.0", "backbone.conv2.1.conv.0", "backbone.conv2.1.conv.1"]
# dw geometries (B, cin, H, W, cout, ksize, stride) the configurations contain: the stem of amp-plus-160x128-b3, neck32.4 of amp-plus-64-b1
MULTI_SPLIT, SINGLE_SPLIT = (3, 3, 160, 128, 32, 3, 1), (1, 1024, 2, 2, 512, 1, 1)
HOLDS = {"amp-plus-160x128-b3": (MULTI_SPLIT, True), "amp-plus-64-b1": (SINGLE_SPLIT, False)}


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _expect(cid, cap, frozen):
    """What the nodes of an amp step must have recorded: types, gradients, and which nodes are frozen."""
    u16, f32 = np.uint16, np.float32
    assert [r["name"] for r in cap.frozen] == frozen, cid
    for r in cap.convs:
        head = r["bias"]
        owes_dx = r["name"] != ("backbone.conv1" if not frozen else "backbone.conv3.0")
        assert r["forward"] == "hip" and r["backward"] == "hip" and r["out_dtype"] == ("float32" if head else "bfloat16"), (cid, r["name"])
        assert r["x"].dtype == u16 and r["w"].dtype == f32 and r["y"].dtype == (f32 if head else u16), (cid, r["name"])
        assert r["dy"] is not None and r["dy"].dtype == r["y"].dtype and r["dy_bits"].dtype == u16, (cid, r["name"])
        assert r["x_requires_grad"] == owes_dx and (r["dx"] is not None) == owes_dx and (not owes_dx or r["dx"].dtype == u16), (cid, r["name"])
        assert r["dw"] is not None and r["dw"].dtype == f32 and (r["db"] is not None) == head, (cid, r["name"])
    for r in cap.blocks:
        assert all(r[k] is not None and r[k].dtype == u16 for k in ("h", "y", "dy", "dx")), (cid, r["name"])
        assert all(r[k] is not None and r[k].dtype == f32 for k in ("gamma", "beta", "rm", "rv", "dgamma", "dbeta")), (cid, r["name"])
        assert r["training"] and (r["res"] is not None) == r["name"].endswith(".conv.1"), (cid, r["name"])
    for r in cap.frozen:
        assert r["x"].dtype == u16 and r["y"].dtype == u16 and (r["res"] is not None) == r["name"].endswith(".conv.1"), (cid, r["name"])
    for r in cap.cats:
        assert r["y"].dtype == u16 and r["dy"] is not None and all(g is not None and g.dtype == u16 for g in r["dsrc"]), (cid, r["name"])
    for r in cap.splits:
        assert r["x"].dtype == f32 and r["dx"] is not None and all(d is not None and d.dtype == f32 for d in r["dys"]), (cid, r["name"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_amp_audit(dev, cfg):
    """Every node of one amp step: tied bit for bit to its isolated re-run, every rounding identity exact, the float32 quantities
    within the float32 audit's bars against float64, the chain of bits from node to node whole (module docstring)."""
    cid, model, (B, H, W), wseed, cotangent, frozen_stages = cfg
    started = time.perf_counter()
    sd, x = synth.synth_state_dict(wseed, obj_bias=-16.0, head_gain=4.0, model=model), synth.synth_image_batch(31, B, H, W)
    net = getattr(train, model)(3, 80, frozen_stages=frozen_stages, **AMP)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    assert not torch.backends.cudnn.deterministic          # the amp step's claim: it needs no deterministic flag
    backward = _loss_backward(dev, B, H, W) if cotangent == "loss" else A.cotangent_backward(5)
    cap = A.run_step(net, x.to(dev), lambda c: A.hip_targets(c, convs=False, routes=True, amp=True), backward, deterministic=False)
    torch.cuda.synchronize(dev)
    assert not torch.backends.cudnn.deterministic
    frozen = FROZEN2 if frozen_stages == 2 else []
    blocks, all_convs, routes = A.expected_nodes(model)
    assert sorted(r["name"] for r in cap.blocks + cap.frozen) == sorted(blocks)
    assert sorted(r["name"] for r in cap.convs + cap.frozen) == sorted(all_convs)
    assert [r["name"] for r in cap.cats + cap.splits] == [r.name for r in routes]
    assert all((p.grad is not None) == p.requires_grad and (p.grad is None or p.grad.dtype == torch.float32) for p in net.parameters())
    assert all(p.requires_grad != any(n.startswith(f + ".") for f in frozen) for n, p in net.named_parameters())
    del net
    _expect(cid, cap, frozen)
    if cotangent == "loss":          # the loss's head gradients are not bf16-valued: the node's own rounding of dy is a real one
        heads = [r for r in cap.convs if r["bias"]]
        assert all(not np.array_equal(A.Q.widen(r["dy_bits"]), r["dy"]) for r in heads), cid
    if cid in HOLDS:          # this configuration really runs the dw geometry it is in the list for
        geom, multi = HOLDS[cid]
        assert geom in [r["x"].shape + (r["w"].shape[0], r["ksize"], r["stride"]) for r in cap.convs], (cid, geom)
        assert (omlib.load().om_conv2d_bf16_grad_workspace_bytes(*geom) > 0) == multi, (cid, geom)

    failures, worst = A.amp_audit(cid, cap, model, A.hip_amp_conv_rerun(dev), A.hip_amp_block_rerun(dev), A.hip_frozen_rerun(dev),
                                  A.hip_route_rerun(dev))
    for (kind, grad, metric), s in sorted(worst.items()):
        print("%-22s worst %-6s %-12s %-8s %.2f of its bar (kernel %.3g, torch-cpu %.3g, ratio %.2f) at %s" % (
            cid, kind, grad, metric, A.over_bar(s), s.err, s.yard, s.err / max(s.yard, 1e-30), s.node))
    print("%-22s nodes: %d convolutions, %d blocks, %d frozen blocks, %d concats, %d splits; %.1f s" % (
        cid, len(cap.convs), len(cap.blocks), len(cap.frozen), len(cap.cats), len(cap.splits), time.perf_counter() - started))
    torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)


def test_the_configurations_hold_a_multi_split_and_a_single_split_dw(dev):
    """om_conv2d_bf16_grad_weight sums through the workspace only where the pixels are split over several workgroups: the
    configuration list has such a layer (the stem at 3 x 160 x 128) and one that needs no workspace (neck32.4 on a 2 x 2 map)."""
    L = omlib.load()
    ids = {c[0]: c for c in CONFIGS}
    assert ids["amp-plus-160x128-b3"][2] == (3, 160, 128) and ids["amp-plus-64-b1"][2] == (1, 64, 64)
    assert L.om_conv2d_bf16_grad_workspace_bytes(*MULTI_SPLIT) > 0 and L.om_conv2d_bf16_grad_workspace_bytes(*SINGLE_SPLIT) == 0
    assert {cid: multi for cid, (_, multi) in HOLDS.items()} == {"amp-plus-160x128-b3": True, "amp-plus-64-b1": False}
