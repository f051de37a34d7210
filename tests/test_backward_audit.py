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

Configurations: the smallest that reach every geometry and mode (CONFIGS).  pytest -s prints one line per node, gradient and metric
and the worst ratio per gradient; those of the first MI355X run are in DESIGN.md 3.20.  Out of scope: the SyncBatchNorm nodes
(tests/test_bn_sync.py), torch's glue ops (cat, split, up-sampling, the residual add), the loss backward (tests/test_loss_grad.py).
"""
import os

import numpy as np
import pytest
import torch

import backward_audit as A
from conftest import ANCHOR_MASK, ANCHORS_YOLOV4, GOLDEN, fixture_weights_and_input
from orienmask_amd import builder, synth, train

pytestmark = pytest.mark.gpu

# (id, model, (B, H, W), weights: a synth_state_dict seed or a tests/golden fixture (weights and input), backbone BatchNorm in eval
# mode, cotangent: "cot" = bn_act_np.cotangents or "loss" = the HIP training loss, conv_backend)
CONFIGS = [
    ("plus-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "cot", "hip"),
    ("plus-loss-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "loss", "hip"),
    ("plus-bneval-96-b2", "OrienMaskYOLOFPNPlus", (2, 96, 96), "train_step_bneval_f96_b2.npz", True, "cot", "hip"),
    ("plus-160x128-b3", "OrienMaskYOLOFPNPlus", (3, 160, 128), 9, False, "cot", "hip"),
    ("yolo-64x96-b2", "OrienMaskYOLO", (2, 64, 96), 8, False, "cot", "hip"),
    ("plus-64-b1", "OrienMaskYOLOFPNPlus", (1, 64, 64), 8, False, "cot", "hip"),
    ("plus-96-b2-torchconv", "OrienMaskYOLOFPNPlus", (2, 96, 96), 8, False, "cot", "torch"),      # the default: only bn_leaky nodes
]


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _loss_backward(dev, B, H, W):
    cfg = dict(type="OrienMaskYOLOMultiScaleLoss", grid_size=[[H // 32, W // 32], [H // 16, W // 16], [H // 8, W // 8]],
               image_size=[H, W], anchors=ANCHORS_YOLOV4, anchor_mask=ANCHOR_MASK, num_classes=80, center_region=0.6,
               valid_region=0.6, label_smooth=False, obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20],
               scales_weight=[1, 1, 1], scales_id=["S32", "S16", "S08"])
    loss_fn = builder.build(cfg, train)
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, B, H, W, 6))

    def backward(heads):
        loss, _, _ = loss_fn(((heads[0], heads[1]), (heads[2], heads[3]), (heads[4], heads[5])), target, training=True)
        assert torch.isfinite(loss)
        loss.backward()
    return backward


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_backward_audit(dev, cfg):
    """Every HIP autograd node of one training step: (a) tied bit for bit to its isolated re-run, (b) within the bars against
    float64 (module docstring)."""
    cid, model, (B, H, W), weights, bneval, cotangent, conv_backend = cfg
    if isinstance(weights, str):
        g = np.load(os.path.join(GOLDEN, weights))
        sd, x = fixture_weights_and_input(g)
        assert tuple(x.shape) == (B, 3, H, W) and bool(int(g["bneval"])) == bneval
        gseed = int(g["gseed"])
    else:
        sd, x, gseed = synth.synth_state_dict(weights, obj_bias=-16.0, head_gain=4.0, model=model), synth.synth_image_batch(31, B, H, W), 5
    net = getattr(train, model)(3, 80, backbone_batchnorm_eval=bneval, backend="hip", conv_backend=conv_backend)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    convs = conv_backend == "hip"
    backward = _loss_backward(dev, B, H, W) if cotangent == "loss" else A.cotangent_backward(gseed)
    cap = A.run_step(net, x.to(dev), lambda c: A.hip_targets(c, convs=convs), backward)
    torch.cuda.synchronize(dev)
    blocks, all_convs = A.expected_nodes(model)
    assert sorted(r["name"] for r in cap.blocks) == sorted(blocks)
    assert sorted(r["name"] for r in cap.convs) == (sorted(all_convs) if convs else [])
    assert all(p.grad is not None for p in net.parameters())
    del net

    rerun_conv, rerun_block = A.hip_conv_rerun(dev), A.hip_block_rerun(dev)
    failures, worst = [], {}
    for kind, records in (("conv", cap.convs), ("block", cap.blocks)):
        for rec in records:
            if kind == "conv":
                first = rec["name"] == "backbone.conv1"
                assert rec["x_requires_grad"] != first and (rec["dx"] is None) == first, (cid, rec["name"], "input gradient")
                assert rec["dw"] is not None and (rec["db"] is not None) == rec["bias"], (cid, rec["name"])
                again = rerun_conv(rec)
                untied = A.differing(rec, again, A.conv_wants(rec))
                scores = A.judge_conv(rec, again)
            else:
                assert rec["training"] == (not (bneval and rec["name"].startswith("backbone."))), (cid, rec["name"])
                assert (rec["res"] is not None) == rec["name"].endswith(".conv.1"), (cid, rec["name"])
                assert all(rec[k] is not None for k in ("dx", "dgamma", "dbeta")), (cid, rec["name"])
                again = rerun_block(rec)
                untied = A.differing(rec, again, A.BLOCK_TIED)
                scores = A.judge_block(rec, again)
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
    for (kind, grad, metric), s in sorted(worst.items()):
        print("%-18s worst %-5s %-12s %-8s %.2f of its bar (kernel %.3g, torch-cpu %.3g, ratio %.2f) at %s" % (
            cid, kind, grad, metric, A.over_bar(s), s.err, s.yard, s.err / max(s.yard, 1e-30), s.node))
    torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)
