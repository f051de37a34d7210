"""Teacher-forced audit of every HIP autograd node of one training step against float64 (harness: tests/backward_audit.py).

One forward and backward of a training model built with backend='hip', conv_backend='hip' runs on the GPU with recording wrappers on
orienmask_amd.train's conv2d and bn_leaky: every convolution (the four plain heads included) and every BatchNorm + LeakyReLU block
is recorded with the tensors the MODEL handed it -- LeakyReLU outputs with a common mode, residual sums, the dy that the layers
behind it produced -- and with the gradients it returned: its own input gradient (a hook on an alias of the input; none for
backbone.conv1, whose input is the image), the gradient for its residual, and its parameters' .grad.  Each node is then run again
alone through the C ABI on a workspace of its own, and

  (a) bit tie.  Everything the model's own step produced at that node -- dx / dh, dw, dbias, dgamma, dbeta, the block's y and running
      buffers -- equals the isolated re-run bit for bit, and the residual's gradient equals dy.  The kernels are run-to-run
      bit-identical, so a difference means the model context changed a result: the grow-only workspace all calls of one stream share
      (train._workspace), launch order, a stale or aliased buffer, a dy that was not made contiguous.  The tie carries (b) over to
      all .grad tensors of the real step.  The model runs under torch's deterministic-convolution flag (test_conv_grad.py's
      reproducible_forward: the forward convolution is torch's).
  (b) float64.  Truth is float64 on the CPU from the recorded float32 inputs; the yardstick is torch's own float32 on the CPU on
      the same inputs.
        convolution  dx, dw, dbias: max |got - truth| / max |truth| (tests/conv_grad_np.py).  dx, dw also per element:
                     max |got - truth| / (N + |truth|) with N the L2 norm of the products that make the element (torch.nn.grad's
                     two functions on the squared operands, then a square root; the forward audit's N).  Yardstick: the LARGER
                     error of torch.nn.grad in float32 with oneDNN on and off -- in-network the two differ by up to 2.4x -- and
                     for dbias also of F.conv2d's own backward (backward_audit._yardsticks_conv).  Bar: kernel <= 2 x yardstick,
                     floor 2e-7 (test_conv_grad.py's).
        block        y, save_mean, save_invstd, running_mean, running_var, dgamma, dbeta, dh: maximum error over the tensor's
                     scale against tests/bn_act_np.py, gradients under the implementation's own sign mask; bar: kernel <= 2 x
                     torch-CPU's, floor 1e-7 (test_bn_act.py's).  dh also per channel (max error of channel c over max |truth| of
                     channel c, worst channel: in-network the channels' scales spread 100x), bar 4 x torch-CPU's: a plain numpy
                     float32 evaluation of the backward formula already reaches 2.34 x.  The mask differs from the float64 one
                     only where |z| < 1e-5 |gamma|, on at most 1e-4 of the elements; num_batches_tracked exactly.
      Kernel and yardstick are float32 evaluations that differ in summation order only; the bars are not fitted to the kernels.

The all-HIP step (conv_forward='hip', route_backend='hip' as well: what orienmask_amd.trainer runs; the `allhip` configurations).
The forward convolution and the route nodes are then HIP nodes too, and are audited in the same way:
  (a) the model's own y of every convolution equals om_conv2d_forward alone on the recorded x, w and bias; a concat's y and every
      source gradient, the split's outputs and dx equal om_route_concat_forward / _backward alone on the recorded tensors.
  (b) y against F.conv2d in float64 (tests/conv_fwd_np.py), over the tensor's scale and per element with N = sqrt(conv2d(x^2, w^2));
      yardstick the larger error of torch-CPU float32 F.conv2d with oneDNN on and off; bar 2 x yardstick, floor 2e-7
      (test_conv_fwd.py's).  A route node has no tolerance: y equals route_np.forward and every source gradient route_np.backward
      bit for bit, the gradients are also within route_np.within_bound of the float64 block sums (an independent check: a sum in
      another order stays inside the bound and fails the bits); the split's outputs are x's channel slices, its dx the
      concatenation of the recorded dys.
  chaining: every block's h has the bits of its convolution's y, every concat source the bits of the block output that made it,
      the split's x those of orien_head.5's y.
plus-allhip-frozen-64-b1 freezes the backbone's parameters (the reference's freeze_backbone; this package's constructor refuses
the argument because the reference's DarkNet53 cannot run it, so the test sets requires_grad itself): the backbone's nodes then
have forward results only, its features reach cat.neck16 and cat.neck8 as sources that take no gradient (a null pointer in the
kernel call) and neck32.0 and skip4 need no input gradient; _expect_frozen states this, the unfrozen configurations keep _expect.

Configurations: the smallest that reach every geometry and mode (CONFIGS).  pytest -s prints one line per node, quantity and metric,
the worst ratio per quantity and the node counts and duration per configuration; those of the first MI355X runs are in DESIGN.md
3.20 and 3.25.  Out of scope: the SyncBatchNorm nodes (tests/test_bn_sync.py), the residual add and autograd's accumulation over a
tensor's consumers (torch's), the loss backward (tests/test_loss_grad.py).
"""
import os
import time

import numpy as np
import pytest
import torch

import backward_audit as A
from conftest import GOLDEN, fixture_weights_and_input
import train_step as T
from orienmask_amd import builder, synth, train

pytestmark = pytest.mark.gpu

# (id, model, (B, H, W), weights: a synth_state_dict seed or a tests/golden fixture (weights and input), backbone BatchNorm in eval
# mode, cotangent: "cot" = bn_act_np.cotangents or "loss" = the HIP training loss, conv_backend, forward: "torch" = conv_forward and
# route_backend 'torch', "hip" = both 'hip' (all four options: the trainer's step), "hip-frozen" = both 'hip' and the backbone's
# parameters frozen)
CONFIGS = [
    ("plus-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "cot", "hip", "torch"),
    ("plus-loss-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "loss", "hip", "torch"),
    ("plus-bneval-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), "train_step_bneval_f96_b2.npz", True, "cot", "hip", "torch"),
    ("plus-160x128-b3", "OrienMaskYOLOFPNPlus", (3, 160, 128), 9, False, "cot", "hip", "torch"),
    ("yolo-64x96-b2", "OrienMaskYOLO", (2, 64, 96), 8, False, "cot", "hip", "torch"),
    ("plus-64-b1", "OrienMaskYOLOFPNPlus", (1, 64, 64), 8, False, "cot", "hip", "torch"),
    ("plus-96-b2-torchconv", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "cot", "torch", "torch"),      # the default: only bn_leaky nodes
    ("plus-allhip-loss-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "loss", "hip", "hip"),       # the step the trainer runs
    ("plus-allhip-160x128-b3", "OrienMaskYOLOFPNPlus", (3, 160, 128), 9, False, "cot", "hip", "hip"),
    ("yolo-allhip-64x96-b2", "OrienMaskYOLO", (2, 64, 96), 8, False, "cot", "hip", "hip"),                  # the two-source cat.neck4
    ("plus-allhip-64-b1", "OrienMaskYOLOFPNPlus", (1, 64, 64), 8, False, "cot", "hip", "hip"),              # a 2 x 2 map up-sampled x 8
    ("plus-allhip-frozen-64-b1", "OrienMaskYOLOFPNPlus", (1, 64, 64), 8, False, "cot", "hip", "hip-frozen"),
]


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _loss_backward(dev, B, H, W):
    loss_fn = builder.build(T.loss_cfg(H, W), train)
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, B, H, W, 6))

    def backward(heads):
        loss, _, _ = loss_fn(((heads[0], heads[1]), (heads[2], heads[3]), (heads[4], heads[5])), target, training=True)
        assert torch.isfinite(loss)
        loss.backward()
    return backward


def _expect(cid, kind, rec, bneval):
    """What a node of a model whose every parameter trains must have recorded."""
    if kind == "conv":
        first = rec["name"] == "backbone.conv1"
        assert rec["x_requires_grad"] != first and (rec["dx"] is None) == first, (cid, rec["name"], "input gradient")
        assert rec["dw"] is not None and (rec["db"] is not None) == rec["bias"], (cid, rec["name"])
    elif kind == "block":
        assert rec["training"] == (not (bneval and rec["name"].startswith("backbone."))), (cid, rec["name"])
        assert (rec["res"] is not None) == rec["name"].endswith(".conv.1"), (cid, rec["name"])
        assert all(rec[k] is not None for k in ("dx", "dgamma", "dbeta")), (cid, rec["name"])
    elif kind == "cat":
        assert rec["dy"] is not None and all(g is not None for g in rec["dsrc"]), (cid, rec["name"])
    else:
        assert rec["dx"] is not None and all(d is not None for d in rec["dys"]), (cid, rec["name"])


def _expect_frozen(cid, kind, rec, bneval):
    """The same for a model whose backbone's parameters are frozen: a backbone node has its forward results and no gradient at
    all; neck32.0 and skip4, whose input is the backbone's, need no input gradient; a concat's source from the backbone takes none."""
    backbone = rec["name"].startswith("backbone.")
    if kind == "conv":
        assert rec["x_requires_grad"] == (not backbone and rec["name"] not in ("neck32.0", "skip4")), (cid, rec["name"], "input gradient")
        assert (rec["dx"] is not None) == rec["x_requires_grad"] and (rec["dy"] is None) == backbone, (cid, rec["name"])
        assert (rec["dw"] is None) == backbone and (rec["db"] is not None) == rec["bias"], (cid, rec["name"])
        assert A.conv_wants(rec)[:1] == ("y",) and ("dw" in A.conv_wants(rec)) != backbone, (cid, rec["name"])
    elif kind == "block":
        assert rec["training"] and (rec["res"] is not None) == rec["name"].endswith(".conv.1"), (cid, rec["name"])
        assert all((rec[k] is None) == backbone for k in ("dy", "dx", "dgamma", "dbeta")) and (rec["dres"] is None), (cid, rec["name"])
    elif kind == "cat":
        assert rec["dy"] is not None, (cid, rec["name"])
        assert [g is not None for g in rec["dsrc"]] == [not n.startswith("backbone.") for n in rec["src_names"]], (cid, rec["name"])
        assert [g is not None for g in rec["dsrc"]] == rec["src_requires_grad"], (cid, rec["name"])
    else:
        assert rec["dx"] is not None and all(d is not None for d in rec["dys"]), (cid, rec["name"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_backward_audit(dev, cfg):
    """Every HIP autograd node of one training step: (a) tied bit for bit to its isolated re-run, (b) within the bars against
    float64, the route nodes equal to their restatement, the chain of bits from node to node whole (module docstring)."""
    cid, model, (B, H, W), weights, bneval, cotangent, conv_backend, forward = cfg
    started = time.perf_counter()
    if isinstance(weights, str):
        g = np.load(os.path.join(GOLDEN, weights))
        sd, x = fixture_weights_and_input(g)
        assert tuple(x.shape) == (B, 3, H, W) and bool(int(g["bneval"])) == bneval
        gseed = int(g["gseed"])
    else:
        sd, x, gseed = synth.synth_state_dict(weights, obj_bias=-16.0, head_gain=4.0, model=model), synth.synth_image_batch(31, B, H, W), 5
    allhip, frozen = forward != "torch", forward == "hip-frozen"
    options = dict(conv_forward="hip", route_backend="hip") if allhip else {}
    net = getattr(train, model)(3, 80, backbone_batchnorm_eval=bneval, backend="hip", conv_backend=conv_backend, **options)
    net.load_state_dict(sd, strict=True)
    if frozen:
        # what freeze_backbone=True asks of the reference's backbone (model/base.py:66-69); the constructor itself refuses the
        # argument, because the reference's DarkNet53 cannot run it
        net.backbone.requires_grad_(False)
    net = net.to(dev).train()
    convs = conv_backend == "hip"
    backward = _loss_backward(dev, B, H, W) if cotangent == "loss" else A.cotangent_backward(gseed)
    cap = A.run_step(net, x.to(dev), lambda c: A.hip_targets(c, convs=convs, routes=allhip), backward)
    torch.cuda.synchronize(dev)
    blocks, all_convs, routes = A.expected_nodes(model)
    assert sorted(r["name"] for r in cap.blocks) == sorted(blocks)
    assert sorted(r["name"] for r in cap.convs) == (sorted(all_convs) if convs else [])
    assert all((p.grad is not None) == p.requires_grad for p in net.parameters())
    assert all(p.requires_grad != (frozen and n.startswith("backbone.")) for n, p in net.named_parameters())
    assert all(r["forward"] == ("hip" if allhip else "torch") for r in cap.convs)
    assert [r["name"] for r in cap.cats + cap.splits] == ([r.name for r in routes] if allhip else [])
    del net

    expect = _expect_frozen if frozen else _expect
    rerun_conv, rerun_block, rerun_route = A.hip_conv_rerun(dev), A.hip_block_rerun(dev), A.hip_route_rerun(dev)
    failures, worst = A.chaining_faults(cap) + (A.route_mismatches(cap, model) if allhip else []), {}
    for kind, records in (("conv", cap.convs), ("block", cap.blocks), ("cat", cap.cats), ("split", cap.splits)):
        for rec in records:
            expect(cid, kind, rec, bneval)
            if kind == "conv":
                again = rerun_conv(rec)
                untied = A.differing(rec, again, A.conv_wants(rec))
                scores = A.judge_conv(rec, again)
            elif kind == "block":
                again = rerun_block(rec)
                untied = A.differing(rec, again, A.block_tied(rec))
                scores = A.judge_block(rec, again)
            else:
                again = rerun_route(rec)
                untied = A.route_differing(rec, again)
                scores = []
            tie = "  tie " + ("ok" if not untied else "BROKEN: " + ",".join(untied))
            if untied:
                failures.append("%s %s: the model's own %s differ from the isolated re-run's" % (cid, rec["name"], ", ".join(untied)))
            for s in scores:
                text = A.line(cid, rec, s, tie)
                print(text)
                if A.over_bar(s) > 1:
                    failures.append(text)
                key = (kind, s.grad, s.metric)
                if key not in worst or A.over_bar(s) > A.over_bar(worst[key]):
                    worst[key] = s
            for e in A.judge_route(rec, again) if kind in ("cat", "split") else []:
                text = A.route_line(cid, rec, e, tie)
                print(text)
                if not e.ok:
                    failures.append(text)
    for (kind, grad, metric), s in sorted(worst.items()):
        print("%-18s worst %-5s %-12s %-8s %.2f of its bar (kernel %.3g, torch-cpu %.3g, ratio %.2f) at %s" % (
            cid, kind, grad, metric, A.over_bar(s), s.err, s.yard, s.err / max(s.yard, 1e-30), s.node))
    print("%-18s nodes: %d convolutions, %d blocks, %d concats, %d splits; %.1f s" % (
        cid, len(cap.convs), len(cap.blocks), len(cap.cats), len(cap.splits), time.perf_counter() - started))
    torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)
