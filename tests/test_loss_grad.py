"""GPU tests of the loss's backward (om_loss_backward, csrc/loss.hip; orienmask_amd.train) against the reference's own gradients
(tests/golden/grad_loss_*.npz) and the float64 restatement (tests/loss_grad_np.py), and of its autograd wiring."""
import os

import numpy as np
import pytest
import torch

from conftest import ANCHOR_MASK, ANCHORS_YOLOV4, GOLDEN, golden_files
import loss_grad_np

pytestmark = pytest.mark.gpu

FIXTURES = golden_files("grad_loss_")


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _train_loss(cfg):
    from orienmask_amd.train import OrienMaskYOLOMultiScaleLoss
    return OrienMaskYOLOMultiScaleLoss(**cfg)


def _target(dev, target):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in target)


def _hip_grads(dev, cfg, heads, target, gout=1.0, loss=None):
    """(loss_sum, loss_log, [(g_bbox, g_orien)]) with the heads as leaves on the device"""
    leaves = [(b.to(dev).requires_grad_(), o.to(dev).requires_grad_()) for b, o in heads]
    loss = loss or _train_loss(cfg)
    loss_sum, log, _ = loss(leaves, _target(dev, target), training=True)
    assert loss_sum.grad_fn is not None
    flat = [t for p in leaves for t in p]
    grads = torch.autograd.grad(loss_sum, flat, torch.tensor(gout, device=dev))
    return loss_sum, log, [(grads[2 * s], grads[2 * s + 1]) for s in range(len(leaves))]


def _cfg(size, scales=3, anchors=3, **kw):
    h, w = size
    c = dict(grid_size=[[h // 32, w // 32], [h // 16, w // 16], [h // 8, w // 8]][3 - scales:], image_size=[h, w],
             anchors=ANCHORS_YOLOV4, anchor_mask=[m[3 - anchors:] for m in ANCHOR_MASK][3 - scales:], num_classes=80,
             center_region=0.6, valid_region=0.6, label_smooth=False, obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20],
             scales_weight=[1, 1, 1][3 - scales:], scales_id=["S32", "S16", "S08"][3 - scales:])
    c.update(kw)
    return c


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_gradients(dev, name):
    """Every scale and both heads against the reference's autograd: |g - g_ref| <= 1e-5 |g_ref| + 1e-6 max|g_ref| and exactly the
    same zero elements (xy / wh / cls off the positives, obj on ignored cells, orientation outside every ROI), except at most the
    fixture's near-saturation count; the loss values are the values-only path's, bit for bit."""
    from orienmask_amd.loss import OrienMaskYOLOMultiScaleLoss as ValuesLoss
    g, cfg, heads, target, gout = loss_grad_np.load_grad_fixture(os.path.join(GOLDEN, name))
    loss_sum, log, grads = _hip_grads(dev, cfg, heads, target, gout)
    v_sum, v_log, _ = ValuesLoss(**cfg)([(b.to(dev), o.to(dev)) for b, o in heads], _target(dev, target), training=True)
    assert log == v_log and torch.equal(loss_sum.detach(), v_sum)
    assert abs(loss_sum.item() - float(g["loss_sum"])) <= 1e-5 * abs(float(g["loss_sum"]))
    for s, (gb, go) in enumerate(grads):
        rb, ro = loss_grad_np.fixture_grads(g, s, tuple(gb.shape), tuple(go.shape))
        near = g["near_%d" % s]
        nb, no = loss_grad_np.mismatches(gb.cpu().numpy(), rb), loss_grad_np.mismatches(go.cpu().numpy(), ro)
        assert nb <= near[0] + near[1], (name, s, "bbox", nb, near)
        assert no <= near[2], (name, s, "orien", no, near)
    dense = [(gb.cpu().numpy(), loss_grad_np.fixture_grads(g, s, tuple(gb.shape), tuple(go.shape))[0])
             for s, (gb, go) in enumerate(grads)]
    assert loss_grad_np.planted_mismatches(g, dense) == [], name


def _random_case(seed):
    from orienmask_amd import synth
    rng = np.random.default_rng(seed)
    size = [(160, 128), (96, 96), (128, 160)][seed % 3]
    scales, anchors = 1 + seed % 2, 1 + (seed // 2) % 2
    C = [80, 1][(seed // 4) % 2]
    B = int(rng.integers(1, 4))
    counts = [int(rng.integers(0, 25)) if rng.random() < 0.85 else 0 for _ in range(B)]
    cfg = _cfg(size, scales, anchors, num_classes=C, label_smooth=bool(seed % 3 == 0),
               weight=[1, 2, 1, 0.5, 1, 20, 10], scales_weight=[1.5, 0.5][2 - scales:])
    heads = synth.synth_heads(3000 + seed, B, _cfg(size)["grid_size"], num_anchors=anchors, num_classes=C, regime="sparse")
    heads = [(b.clone(), o.clone()) for b, o in heads][3 - scales:]
    target = synth.synth_targets(4000 + seed, B, size[0], size[1], counts, num_classes=C)
    return cfg, heads, target


@pytest.mark.parametrize("seed", range(8))
def test_random_cases_match_restatement(dev, seed):
    """Seeded random cases (1-2 scales, 1-2 anchors, 1 and 80 classes, label smoothing on and off, non-unit weights) against the
    float64 restatement, within its own near-saturation counts; a channels-last bbox head gives the contiguous head's gradients
    bit for bit."""
    cfg, heads, target = _random_case(seed)
    _, _, grads = _hip_grads(dev, cfg, heads, target, 1.25)
    want = loss_grad_np.LossGradNP(**cfg).grad([(b.numpy(), o.numpy()) for b, o in heads], target, 1.25)
    for s, ((gb, go), (rb, ro, near)) in enumerate(zip(grads, want)):
        assert loss_grad_np.mismatches(gb.cpu().numpy(), rb) <= near[0] + near[1], (seed, s, "bbox")
        assert loss_grad_np.mismatches(go.cpu().numpy(), ro) <= near[2], (seed, s, "orien")
    cl = [(b.contiguous(memory_format=torch.channels_last), o) for b, o in heads]
    _, _, g_cl = _hip_grads(dev, cfg, cl, target, 1.25)
    for (a, ao), (b, bo) in zip(grads, g_cl):
        assert b.stride() == b.contiguous(memory_format=torch.channels_last).stride()
        assert torch.equal(a, b.contiguous()) and torch.equal(ao, bo)


class _Heads(torch.nn.Module):
    """A small conv stack that produces the three scales' heads at 96 x 96 (the network's own backward is out of scope: torch's)."""

    def __init__(self, C=80):
        super().__init__()
        torch.manual_seed(0)
        self.stem = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.box = torch.nn.ModuleList([torch.nn.Conv2d(8, 3 * (5 + C), 1) for _ in range(3)])
        self.orien = torch.nn.ModuleList([torch.nn.Conv2d(8, 6, 1) for _ in range(3)])

    def forward(self, x):
        f = torch.relu(self.stem(x))
        q = torch.nn.functional.avg_pool2d(f, 4)
        out = []
        for s, k in enumerate((32, 16, 8)):
            out.append((self.box[s](torch.nn.functional.avg_pool2d(f, k)) - 2.0, self.orien[s](q)))
        return out


def _net_case(dev, B=2, seed=0):
    from orienmask_amd import synth
    cfg = _cfg((96, 96))
    net = _Heads().to(dev)
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 3, 96, 96)).astype(np.float32)).to(dev)
    tgt = _target(dev, synth.synth_targets(50 + seed, B, 96, 96, 6))
    return cfg, net, x, tgt


def _param_grads(net):
    return [p.grad.clone() for p in net.parameters()]


def test_autograd_wiring(dev):
    """loss_sum.backward() gives the parameters what torch.autograd.backward(heads, HIP head gradients) gives; two live calls
    combine as (0.5 l1 + 2 l2); two runs give bit-identical head gradients; the backward is once_differentiable; heads without
    grad take the values-only path."""
    cfg, net, x, tgt = _net_case(dev)
    loss = _train_loss(cfg)

    def run():
        net.zero_grad()
        heads = [t for p in net(x) for t in p]
        for t in heads:
            t.retain_grad()
        loss([(heads[2 * s], heads[2 * s + 1]) for s in range(3)], tgt, training=True)[0].backward()
        return [t.grad.clone() for t in heads], _param_grads(net)

    g_heads, via_loss = run()
    net.zero_grad()
    torch.autograd.backward([t for p in net(x) for t in p], g_heads)
    # torch's own conv backward sums in an order of its choosing: equal up to float32 rounding
    for a, b in zip(via_loss, _param_grads(net)):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max())), float((a - b).abs().max())
    # a second identical run: the HIP head gradients bit-identical
    g2, _ = run()
    assert all(torch.equal(a, b) for a, b in zip(g_heads, g2))
    # two live graphs before one backward: each call keeps its own workspace
    x2 = x.flip(-1)
    net.zero_grad()
    l1 = loss(net(x), tgt, training=True)[0]
    l2 = loss(net(x2), tgt, training=True)[0]
    (0.5 * l1 + 2 * l2).backward()
    both = _param_grads(net)
    net.zero_grad()
    (0.5 * loss(net(x), tgt, training=True)[0]).backward()
    first = _param_grads(net)
    net.zero_grad()
    (2 * loss(net(x2), tgt, training=True)[0]).backward()
    for a, b, c in zip(both, first, _param_grads(net)):
        assert torch.allclose(a, b + c, rtol=1e-5, atol=1e-6 * float((b + c).abs().max()))
    # once_differentiable: differentiating the gradients again raises
    heads = net(x)
    ls = loss(heads, tgt, training=True)[0]
    gg = torch.autograd.grad(ls, [heads[0][0]], torch.ones((), device=dev, requires_grad=True), create_graph=True)[0]
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gg.sum().backward()
    # a head changed in place between forward and backward: autograd's version check raises
    heads = net(x)
    ls = loss(heads, tgt, training=True)[0]
    with torch.no_grad():
        heads[1][0].add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        ls.backward()
    # no head requires grad: the values-only path, no graph
    with torch.no_grad():
        heads = net(x)
    s0, log0, _ = loss(heads, tgt, training=True)
    assert s0.grad_fn is None and not s0.requires_grad
    s1, log1, _ = loss(net(x), tgt, training=True)
    assert log0 == log1
    # leaves that require grad under torch.no_grad(): no graph, the values
    leaves = [(b.detach().requires_grad_(), o.detach().requires_grad_()) for b, o in heads]
    with torch.no_grad():
        s2, log2, _ = loss(leaves, tgt, training=True)
    assert s2.grad_fn is None and log2 == log0


def test_backward_does_not_sync(dev):
    cfg, net, x, tgt = _net_case(dev)
    loss = _train_loss(cfg)
    loss_sum = loss(net(x), tgt, training=True)[0]
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss_sum.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize(dev)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_peak_memory_bs32(dev):
    """At bs 32, 544 x 544 with 50 GTs per image forward plus backward allocate at most the workspace, the gradients and 2 MB."""
    from orienmask_amd import synth
    B, H = 32, 544
    cfg = _cfg((H, H))
    heads = [(b.to(dev).requires_grad_(), o.to(dev).requires_grad_()) for b, o in synth.synth_heads(77, B, cfg["grid_size"],
                                                                                                     regime="sparse")]
    target = synth.synth_targets(78, B, H, H, 50)
    tgt = _target(dev, target)
    loss = _train_loss(cfg)
    ws = loss.workspace_bytes(B, len(target[0]))
    grads = sum(t.numel() * 4 for p in heads for t in p)
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    loss_sum = loss(heads, tgt, training=True)[0]
    g = torch.autograd.grad(loss_sum, [t for p in heads for t in p])
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert peak <= ws + grads + 2 * 1024 * 1024, (peak, ws, grads)
    assert all(torch.isfinite(t).all() for t in g)
