"""What the model-level tests of the training path share (test_bn_act, test_conv_grad, test_conv_fwd, test_route, test_frozen_stages,
test_optim and their CPU companions): the two models' layer cases, the loss configuration, one forward and backward of a model on a
recorded fixture, and build_train_model -> the HIP loss -> backward -> the HIP SGD step."""
import contextlib
import ctypes

import numpy as np
import torch

from conftest import ANCHOR_MASK, ANCHORS_YOLOV4, fixture_weights_and_input
import bn_act_np as N
from orienmask_amd import arch, builder, synth, train
from orienmask_amd import optim as O


def layer_cases(size):
    """Every distinct (cin, cout, ksize, stride, H, W) of the two models' convolutions at this image size; H, W are the input's."""
    out = []
    for spec in list(arch.fpnplus_convs()) + list(arch.yolo_convs()):
        d = arch.layer_div(spec)
        case = (spec.cin, spec.cout, spec.ksize, spec.stride, size[0] // d * spec.stride, size[1] // d * spec.stride)
        if case not in out:
            out.append(case)
    return out


# (B, cin, cout, ksize, stride, H, W): every distinct convolution of the two models at 96 x 96 and 160 x 128, B = 2
SWEEP = [(2,) + c for c in layer_cases((96, 96))] + [(2,) + c for c in layer_cases((160, 128)) if c not in layer_cases((96, 96))]


def case_id(case):
    return "x".join(map(str, case))


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def loss_cfg(h, w):
    return dict(type="OrienMaskYOLOMultiScaleLoss", grid_size=[[h // 32, w // 32], [h // 16, w // 16], [h // 8, w // 8]],
                image_size=[h, w], anchors=ANCHORS_YOLOV4, anchor_mask=ANCHOR_MASK, num_classes=80, center_region=0.6,
                valid_region=0.6, label_smooth=False, obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20],
                scales_weight=[1, 1, 1], scales_id=["S32", "S16", "S08"])


def models(**kw):
    return [train.OrienMaskYOLOFPNPlus(3, 80, **kw), train.OrienMaskYOLO(3, 80, **kw)]


def step(net, x, cot):
    """One forward and backward with the cotangents `cot`.  -> the six heads."""
    heads = [t for pair in net(x) for t in pair]
    torch.autograd.backward(heads, cot)
    return heads


def rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


def recorded_step(dev, g, deterministic=False, **model_kw):
    """The FPN-Plus model of fixture `g` (its weights, input, BatchNorm mode and cotangents) built with model_kw, one step on `dev`;
    deterministic: the step runs under cudnn.flags(deterministic=True).  Heads and gradients are finite.  -> (heads, {name: grad},
    relative-L2 errors of the heads against g's, of the recorded gradients against g's grad_%d, the net)."""
    sd, x = fixture_weights_and_input(g)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backbone_batchnorm_eval=bool(int(g["bneval"])), **model_kw)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    cot = [torch.from_numpy(c).to(dev) for c in N.cotangents(int(g["gseed"]), [g[k].shape for k in N.HEAD_KEYS])]
    with torch.backends.cudnn.flags(deterministic=True) if deterministic else contextlib.nullcontext():
        heads = [t.detach() for t in step(net, x.to(dev), cot)]
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert all(torch.isfinite(h).all() for h in heads), model_kw
    assert all(v is not None and torch.isfinite(v).all() for v in grads.values()), model_kw
    herr = [N.rel_l2(h.cpu().numpy(), g[k]) for k, h in zip(N.HEAD_KEYS, heads)]
    gerr = [N.rel_l2(grads[n].cpu().numpy(), g["grad_%d" % i]) for i, n in enumerate(N.GRAD_NAMES)]
    return heads, grads, herr, gerr, net


def trainer_steps(dev, model_cfg, n, on_output=None):
    """trainer/trainer.py:42-55 with this package's pieces: from seed 3, build_train_model(FPN-Plus with model_cfg) -> the HIP loss
    -> backward -> the HIP SGD step, n times on one 96 x 96 batch of 2; on_output is called with the model's output of every step.
    The loss and every gradient are finite and no parameter is left unchanged by a step.  -> (the losses' bits, the parameters
    after each step, the net)."""
    h = w = 96
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, 2, h, w, 6))
    x = synth.synth_image_batch(8, 2, h, w).to(dev)
    torch.manual_seed(3)
    with torch.cuda.device(dev):
        net = builder.build_train_model(dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None,
                                             freeze_backbone=False, backbone_batchnorm_eval=False, **model_cfg))
    assert net.training and next(net.parameters()).device == dev
    loss_fn = builder.build(loss_cfg(h, w), train)
    optimizer = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, net)
    assert type(optimizer) is O.SGD
    losses, params = [], []
    for _ in range(n):
        optimizer.zero_grad()
        before = [p.detach().clone() for p in net.parameters()]
        out = net(x)
        if on_output is not None:
            on_output(out)
        loss, _, _ = loss_fn(out, target, training=True)
        assert torch.isfinite(loss)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
        optimizer.step()
        torch.cuda.synchronize(dev)
        unchanged = [name for (name, p), b in zip(net.named_parameters(), before) if torch.equal(p.detach(), b)]
        assert not unchanged, unchanged[:5]
        losses.append(loss.detach().cpu().numpy().view(np.uint32).copy())
        params.append([p.detach().clone() for p in net.parameters()])
    return losses, params, net
