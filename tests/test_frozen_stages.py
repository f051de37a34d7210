"""GPU tests of frozen_stages on the training models (orienmask_amd.train) at 96 x 96, B = 2: the frozen prefix with every HIP
option is the fused kernel chained layer by layer; a frozen model's heads and trainable gradients against a float64 CPU model
with the same weights and frozen stages, judged by the backend='torch' frozen model on the same GPU; a whole step repeats its bits;
a frozen step allocates less; the Trainer runs, checkpoints and resumes with a frozen model."""
import os
import types

import numpy as np
import pytest
import torch

import bn_act_np as N
import loss_counter_cases as cases
import train_step as T
from orienmask_amd import arch, builder, synth, train
from orienmask_amd import optim as O

pytestmark = pytest.mark.gpu

HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")
FLOOR = 2e-7
SIZE, BATCH = 96, 2


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _stage(name):
    return int(name.split(".")[1][len("conv"):]) if name.startswith("backbone.conv") else 7


def _randomise_buffers(net, seed):
    """Running statistics that are not BatchNorm's initial (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, buf in net.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))


@pytest.fixture(scope="module")
def weights():
    """One set of weights and buffers (CPU) for every model of this file."""
    torch.manual_seed(13)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    _randomise_buffers(net, 17)
    return {k: v.clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope="module")
def image():
    return synth.synth_image_batch(8, BATCH, SIZE, SIZE)


def _model(dev, weights, k, **kw):
    net = train.OrienMaskYOLOFPNPlus(3, 80, frozen_stages=k, **kw)
    net.load_state_dict(weights, strict=True)
    return net.to(dev).train()


# ---------------------------------------------------------------------------------------------------------------- the prefix
def test_frozen_prefix_is_the_fused_kernel_chained_by_hand(dev, weights, image):
    """k = 6, every HIP option, train() mode: the four backbone features equal, bit for bit, conv_bn_leaky_frozen called layer by
    layer on the same modules' parameters (model/backbone/darknet.py:47-54 with the blocks of :14-15)."""
    net = _model(dev, weights, 6, **HIP)
    mods = dict(net.named_modules())
    last = {idx: "backbone.conv%d.%d.conv.1" % (idx, nblocks) for idx, _, nblocks in arch.DARKNET_STAGES}
    seen = {}
    hooks = [mods[name].register_forward_hook(lambda m, args, out, idx=idx: seen.__setitem__(idx, out)) for idx, name in last.items()]
    x = image.to(dev)
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()

    def layer(name, t, residual=None):
        blk = mods[name]
        conv, bn = blk.conv_block[0], blk.conv_block[1]
        assert blk.frozen and not bn.training
        return train.conv_bn_leaky_frozen(t, conv.weight, bn, residual=residual, stride=conv.stride, padding=conv.padding)

    t = layer("backbone.conv1", x)
    for idx, _, nblocks in arch.DARKNET_STAGES:
        t = layer("backbone.conv%d.0" % idx, t)
        for j in range(1, nblocks + 1):
            t = layer("backbone.conv%d.%d.conv.1" % (idx, j), layer("backbone.conv%d.%d.conv.0" % (idx, j), t), residual=t)
        if idx >= 3:
            assert seen[idx].grad_fn is None
            assert torch.isfinite(t).all() and torch.equal(t, seen[idx]), idx
    assert sorted(seen) == [2, 3, 4, 5, 6]


# ---------------------------------------------------------------------------------------------------------------- accuracy
MARGIN = 2.0        # |beta| of a trainable BatchNorm channel in the accuracy test: this much beyond the largest possible |xhat|
CLEAR = 1.0         # every trainable pre-activation of the float64 model must be at least this far from zero
DEFAULTS = dict(backend="hip")      # conv_backend, conv_forward and route_backend 'torch': the models' default backends


def _weights_clear_of_zero(weights, k):
    """The file's weights with beta = +M on the even and -M on the odd channels of every BatchNorm behind stage k (gamma is 1
    there: BatchNorm's and _init_weights' initial value).  A trainable block normalises with batch statistics, so its
    pre-activation is z = xhat + beta, and among n = B * H * W values of zero mean and unit (biased) variance none exceeds
    sqrt(n - 1) in magnitude: with M = sqrt(n - 1) + MARGIN for the block's own map, half the channels run on each side of
    LeakyReLU and no element can come within MARGIN of zero (the test asserts |z| >= CLEAR on the float64 model).  Without this a float32 model
    takes the other side of LeakyReLU than the float64 model on a few of the ~5e6 trainable pre-activations -- behind the 18-sample
    BatchNorm layers of the 3 x 3 maps its z differs by ~1e-5 -- and each such element moves single gradient entries by a finite
    amount, in tensors that chance picks, for torch's float32 evaluation as for ours: an error that measures no arithmetic."""
    out = dict(weights)
    for spec in arch.fpnplus_convs():
        if spec.bn and _stage(spec.name) > k:
            name = spec.name + ".conv_block.1."
            assert torch.equal(weights[name + "weight"], torch.ones(spec.cout)), name
            n = BATCH * (SIZE // arch.layer_div(spec)) ** 2
            beta = torch.full((spec.cout,), (n - 1) ** 0.5 + MARGIN)
            beta[1::2] *= -1
            out[name + "bias"] = beta
    return out


def test_heads_and_gradients_against_float64(dev, weights, image, monkeypatch):
    """k = 3.  Truth: the backend='torch' model in float64 on the CPU, same weights, same frozen stages.  For EVERY head and EVERY
    trainable gradient, the maximum error over the truth's scale (bn_act_np.rel_max's measure) of the all-HIP model, and of the model with
    the default backends (F.conv2d, then the HIP BatchNorm block's eval kernel in the frozen stages), is at most twice that of the
    backend='torch' frozen model on the same GPU, floor 2e-7.  The weights keep every trainable pre-activation clear of zero
    (_weights_clear_of_zero), on both sides of LeakyReLU.  Also, per model: no frozen block's output has a grad_fn, frozen
    parameters get no gradient, frozen buffers keep their bits.  The project's aggregate (rms over tensors of the relative-L2
    error, tests/test_conv_fwd.py) is asserted on top."""
    k = 3
    weights = _weights_clear_of_zero(weights, k)
    frozen = [s.name for s in arch.fpnplus_convs() if _stage(s.name) <= k]
    got, cot = {}, None
    for label, kw in (("torch", dict(backend="torch")), ("hip", HIP), ("default", DEFAULTS)):
        net = _model(dev, weights, k, **kw)
        assert (net.backend, net.conv_backend, net.conv_forward, net.route_backend) == \
            {"torch": ("torch",) * 4, "hip": ("hip",) * 4, "default": ("hip", "torch", "torch", "torch")}[label]
        outputs = {}
        hooks = [m.register_forward_hook(lambda m, args, out, name=name: outputs.__setitem__(name, (out.grad_fn, out.requires_grad)))
                 for name, m in net.named_modules() if name in frozen]
        heads = [t for pair in net(image.to(dev)) for t in pair]
        for h in hooks:
            h.remove()
        assert sorted(outputs) == sorted(frozen) and all(v == (None, False) for v in outputs.values()), label
        if cot is None:
            cot = [torch.from_numpy(c) for c in N.cotangents(29, [h.shape for h in heads])]
        torch.autograd.backward(heads, [c.to(dev) for c in cot])
        torch.cuda.synchronize(dev)
        grads = {}
        for n, p in net.named_parameters():
            if n.split(".conv_block.")[0] in frozen:
                assert p.grad is None and not p.requires_grad, (label, n)
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), (label, n)
                grads[n] = p.grad.cpu().numpy()
        for n, b in net.named_buffers():
            if _stage(n) <= k:
                assert torch.equal(b.cpu(), weights[n]), (label, n)
        assert not torch.equal(net.state_dict()["backbone.conv4.0.conv_block.1.running_mean"].cpu(),
                               weights["backbone.conv4.0.conv_block.1.running_mean"])
        got[label] = ([h.detach().cpu().numpy() for h in heads], grads)
        del net, heads

    # the float64 model, with the least |z| and the sides taken over its trainable blocks (the calls with training=True)
    seen = {"least": float("inf"), "positive": 0, "negative": 0}
    batch_norm = train.F.batch_norm

    def recording(x, rm, rv, w, b, training, *rest):
        z = batch_norm(x, rm, rv, w, b, training, *rest)
        if training:
            seen["least"] = min(seen["least"], float(z.detach().abs().min()))
            seen["positive"] += int((z.detach() > 0).sum())
            seen["negative"] += int((z.detach() < 0).sum())
        return z

    truth_net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", frozen_stages=k)
    truth_net.load_state_dict(weights, strict=True)
    truth_net = truth_net.double().train()
    monkeypatch.setattr(train.F, "batch_norm", recording)
    want_heads = [h.detach().numpy() for h in T.step(truth_net, image.double(), [c.double() for c in cot])]
    monkeypatch.undo()
    want_grads = {n: p.grad.numpy() for n, p in truth_net.named_parameters() if p.grad is not None}
    assert sorted(want_grads) == sorted(got["hip"][1]) == sorted(got["torch"][1]) and len(want_grads) == 266 - 3 * len(frozen)
    print("float64 trainable pre-activations: least |z| %.3g, %d positive, %d negative" % (seen["least"], seen["positive"], seen["negative"]))
    assert seen["least"] >= CLEAR and min(seen["positive"], seen["negative"]) > 0.4 * (seen["positive"] + seen["negative"])

    # A beta gradient that is zero in exact arithmetic has no scale of its own: where every element of a channel is on one side of
    # LeakyReLU and the block feeds only 1x1 blocks with batch statistics, beta is a per-channel constant that those statistics
    # remove, and the float64 gradient is rounding noise (1e-16 ... 1e-13 here, against 1e-3 ... 26 for the others).  Its error is
    # taken over the scale of the same block's gamma gradient, which is built from the same dz.
    scale_of = {}
    for n, t in want_grads.items():
        gamma = want_grads.get(n[:-len("bias")] + "weight") if n.endswith("conv_block.1.bias") else None
        scale_of[n] = gamma if gamma is not None and np.abs(t).max() < 1e-9 * np.abs(gamma).max() else t
    zero = [n for n, t in want_grads.items() if scale_of[n] is not t]
    assert all(n.endswith("conv_block.1.bias") for n in zero) and len(zero) < 30, zero
    print("beta gradients that are zero in exact arithmetic: %d" % len(zero))

    errs, agg = {}, {}
    for label, (heads, grads) in got.items():
        triples = [("head%d" % i, h, w, w) for i, (h, w) in enumerate(zip(heads, want_heads))]
        triples += [(n, g, want_grads[n], scale_of[n]) for n, g in grads.items()]
        errs[label] = {n: float(np.abs(g - w).max() / np.abs(sc).max()) for n, g, w, sc in triples}
        agg[label] = {n: float(np.linalg.norm((g - w).ravel()) / np.linalg.norm(sc.ravel())) for n, g, w, sc in triples}
    rms = lambda v: float(np.sqrt(np.mean(np.square(list(v)))))      # noqa: E731
    failures = []
    for label in ("hip", "default"):
        ratios = {n: errs[label][n] / max(errs["torch"][n], FLOOR / 2) for n in errs[label]}
        for n in sorted(ratios, key=ratios.get)[-4:]:
            print("%-8s %-44s ours %.3g  torch %.3g  ratio %.2f" % (label, n, errs[label][n], errs["torch"][n], ratios[n]))
        print("%-8s heads: ours %s  torch %s" % (label, ["%.2g" % errs[label]["head%d" % i] for i in range(6)],
                                                ["%.2g" % errs["torch"]["head%d" % i] for i in range(6)]))
        above = [(n, errs[label][n], errs["torch"][n]) for n in errs[label] if errs[label][n] > max(2 * errs["torch"][n], FLOOR)]
        print("%-8s %d of %d tensors above the bar: %s" % (label, len(above), len(ratios), above))
        failures += [(label,) + a for a in above]
        for what, pick in (("heads", lambda n: n.startswith("head")), ("trainable gradients", lambda n: not n.startswith("head"))):
            ours, theirs = (rms(v for n, v in agg[lb].items() if pick(n)) for lb in (label, "torch"))
            print("%-8s %s: relative-L2 error, rms over tensors: ours %.3g  torch %.3g  ratio %.2f" % (label, what, ours, theirs, ours / theirs))
            if ours > max(2 * theirs, FLOOR):
                failures.append((label, what, ours, theirs))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- a whole step
def _train_step(dev, k, x, target):
    """build_train_model -> the HIP loss -> backward -> the HIP SGD step.  -> (net, optimizer, loss bits, peak bytes of the step)."""
    torch.manual_seed(3)
    with torch.cuda.device(dev):
        net = builder.build_train_model(dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None,
                                             freeze_backbone=False, backbone_batchnorm_eval=False, frozen_stages=k, **HIP))
    loss_fn = builder.build(T.loss_cfg(SIZE, SIZE), train)
    optimizer = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, net)
    assert type(optimizer) is O.SGD
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    loss, _, _ = loss_fn(net(x), target, training=True)
    loss.backward()
    optimizer.step()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert torch.isfinite(loss)
    return net, optimizer, loss.detach().cpu().numpy().view(np.uint32).copy(), peak


@pytest.fixture(scope="module")
def step_inputs(dev, image):
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, BATCH, SIZE, SIZE, 6))
    return image.to(dev), target


def test_one_step_repeats_its_bits_and_moves_only_the_trainable_tensors(dev, step_inputs):
    """k = 3, twice from the same seed: the loss and every parameter are bit-identical; the HIP SGD holds exactly the trainable
    tensors; the frozen weights and buffers are the initial ones, every trainable parameter moved."""
    k = 3
    torch.manual_seed(3)
    initial = train.OrienMaskYOLOFPNPlus(3, 80, frozen_stages=k, **HIP).state_dict()
    runs = [_train_step(dev, k, *step_inputs)[:3] for _ in range(2)]
    net, optimizer, _ = runs[0]
    held = [id(p) for g in optimizer.param_groups for p in g["params"]]
    assert held == [id(p) for n, p in net.named_parameters() if _stage(n) > k]
    assert len(held) == len(list(net.parameters())) - 3 * sum(1 for s in arch.fpnplus_convs() if _stage(s.name) <= k)
    params = dict(net.named_parameters())
    for n, v in net.state_dict().items():
        if _stage(n) <= k:
            assert torch.equal(v.cpu(), initial[n]), n
            assert n not in params or params[n].grad is None, n
        elif n in params:
            assert not torch.equal(v.cpu(), initial[n]), n
    assert np.array_equal(runs[0][2], runs[1][2])
    differ = [n for (n, a), b in zip(runs[0][0].state_dict().items(), runs[1][0].state_dict().values()) if not torch.equal(a, b)]
    assert not differ, differ[:5]


def test_a_frozen_step_allocates_less(dev, step_inputs):
    """No saved activations and no gradients for the backbone's 52 layers: the peak of one step over what was allocated before it
    (parameters, buffers, inputs) with k = 6 is strictly below that of k = 0 on the same inputs."""
    peaks = {}
    for k in (0, 6):
        net, optimizer, _, peaks[k] = _train_step(dev, k, *step_inputs)
        del net, optimizer
    print("peak bytes of one step over its start: k=0 %d  k=6 %d" % (peaks[0], peaks[6]))
    assert peaks[6] < peaks[0]


# ---------------------------------------------------------------------------------------------------------------- the Trainer
def _trainer_run(dev, tmp, name, resume=None, **kw):
    """tests/test_trainer.py's small configuration (6 images of 64 x 64, B = 2, accumulate 2: two steps per epoch), k = 4."""
    from orienmask_amd.tester import SyntheticLossLoader
    from orienmask_amd.trainer import Trainer
    config = dict(n_gpu=1, accumulate=2, epochs=2, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off", log_freq=1,
                  log_dir=str(tmp), name=name,
                  model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=cases.NUM_CLASSES, frozen_stages=4, **HIP),
                  loss=dict(type="OrienMaskYOLOMultiScaleLoss", **cases.loss_kwargs()),
                  optimizer=dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4),
                  lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[4], gamma=0.5))
    config.update(kw)
    torch.manual_seed(7)
    model = builder.build(config["model"], train).to(dev)
    initial = {k: v.clone() for k, v in model.state_dict().items()}
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
    scheduler = builder.build(config["lr_scheduler"], O, optimizer=optimizer)
    loader = SyntheticLossLoader(6, cases.BATCH, size=(cases.IMAGE, cases.IMAGE), seed=0, gts_per_image=cases.GTS_PER_IMAGE,
                                 num_classes=cases.NUM_CLASSES, device=dev)
    t = Trainer(model, loss, optimizer, scheduler, config, loader, None, None, dev, types.SimpleNamespace(resume=resume, weights=None),
                sync_free=True)
    t.train()
    torch.cuda.synchronize(dev)
    return t, initial


def test_trainer_trains_checkpoints_and_resumes_a_frozen_model(dev, tmp_path):
    """Epoch 1 is two steps: the checkpoint written after it holds the initial frozen weights and buffers, bit for bit, and moved
    trainable ones.  Resuming from it reproduces the steps of epoch 2 bit for bit (weights, buffers and momentum)."""
    full, initial = _trainer_run(dev, tmp_path, "frozen")
    assert full.lr_scheduler.last_epoch == 4
    ckpt = os.path.join(full.checkpoint_dir, "epoch1.pth")
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    assert list(saved) == list(initial)
    names = {n for n, _ in full.model.named_parameters()}
    for sd in (saved, {k: v.cpu() for k, v in full.model.state_dict().items()}):
        for n, v in sd.items():
            assert torch.isfinite(v).all(), n
            if _stage(n) <= 4:
                assert torch.equal(v, initial[n].cpu()), n
            elif n in names:
                assert not torch.equal(v, initial[n].cpu()), n
    resumed, _ = _trainer_run(dev, tmp_path, "frozen", resume=ckpt, save_freq=5)
    assert resumed.start_epoch == 2
    a, b = full.model.state_dict(), resumed.model.state_dict()
    for n in a:
        assert torch.equal(a[n], b[n]), n
    momentum = lambda t: [s["momentum_buffer"] for _, s in sorted(t.optimizer.state_dict()["state"].items())]      # noqa: E731
    ma, mb = momentum(full), momentum(resumed)
    assert len(ma) == len(mb) == sum(1 for p in full.model.parameters() if p.requires_grad)
    assert all(torch.equal(x, y) for x, y in zip(ma, mb))
