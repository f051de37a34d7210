"""CPU tests of frozen_stages (orienmask_amd.train.OrienMaskYOLOFPNPlus / OrienMaskYOLO, ConvBNLeaky(frozen=True)) with
backend='torch' at 64 x 64, B = 2: a model built with frozen_stages=k against an unfrozen model with the same weights whose stages
<= k were frozen by hand (requires_grad_(False), BatchNorm .eval()); the checkpoint keys; the argument checks; the plumbing through
builder.build_optimizer, train.convert_sync_batchnorm and builder.build_train_model.  No GPU compute."""
import pytest
import torch

import train_step as T
from orienmask_amd import arch, builder, train
from orienmask_amd import optim as O

CASES = [("OrienMaskYOLOFPNPlus", 0), ("OrienMaskYOLOFPNPlus", 1), ("OrienMaskYOLOFPNPlus", 3), ("OrienMaskYOLOFPNPlus", 6),
         ("OrienMaskYOLO", 3)]


def _stage(name):
    """backbone.conv{i}[...] -> i; anything outside the backbone -> 7 (never frozen)."""
    return int(name.split(".")[1][len("conv"):]) if name.startswith("backbone.conv") else 7


def _randomise_buffers(net, seed):
    """Running statistics that are not BatchNorm's initial (0, 1), and a counter that is not 0."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, buf in net.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
            elif name.endswith("num_batches_tracked"):
                buf.fill_(5)


def _pair(name, k):
    """(the frozen_stages=k model, the comparison model frozen by hand), both in train() mode with the same weights."""
    torch.manual_seed(13)
    net = getattr(train, name)(3, 80, backend="torch", frozen_stages=k)
    _randomise_buffers(net, 17)
    hand = getattr(train, name)(3, 80, backend="torch")
    hand.load_state_dict(net.state_dict(), strict=True)
    net.train()
    hand.train()
    for mod_name, m in hand.named_modules():
        if isinstance(m, train.ConvBNLeaky) and _stage(mod_name) <= k:
            m.requires_grad_(False)
            m.conv_block[1].eval()
    return net, hand


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 64, generator=g)
    with torch.no_grad():
        shapes = [t.shape for pair in train.OrienMaskYOLO(3, 80, backend="torch").eval()(x) for t in pair]
    return x, [torch.randn(s, generator=g) for s in shapes]


@pytest.mark.parametrize("name,k", CASES, ids=["%s-k%d" % c for c in CASES])
def test_equals_the_model_frozen_by_hand(batch, name, k):
    x, cot = batch
    net, hand = _pair(name, k)
    assert net.frozen_stages == k and net.training
    frozen_names = [n for n, _ in net.named_parameters() if _stage(n) <= k]
    assert len(frozen_names) == 3 * sum(1 for s in arch.model_convs(name, 3, 80) if _stage(s.name) <= k)
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == frozen_names
    for mod_name, m in net.named_modules():
        if isinstance(m, train.ConvBNLeaky):
            assert m.frozen == (_stage(mod_name) <= k), mod_name
            assert m.conv_block[1].training == (not m.frozen), mod_name
    before = {n: b.clone() for n, b in net.named_buffers()}

    heads, want = T.step(net, x, cot), T.step(hand, x, cot)
    for h, w in zip(heads, want):
        assert torch.isfinite(h).all() and torch.equal(h, w)
    theirs = dict(hand.named_parameters())
    for n, p in net.named_parameters():
        if n in frozen_names:
            assert p.grad is None and theirs[n].grad is None, n
        else:
            assert p.grad is not None and torch.equal(p.grad, theirs[n].grad), n

    # the frozen stages' buffers are untouched (the counter included); the first trainable stage's moved
    nxt = "backbone.conv%d." % (k + 1) if k < 6 else "neck32.0."
    moved = 0
    for n, b in net.named_buffers():
        if _stage(n) <= k:
            assert torch.equal(b, before[n]), n
        elif n.startswith(nxt):
            assert not torch.equal(b, before[n]), n
            moved += 1
    assert moved >= 3
    assert all(torch.equal(b, dict(hand.named_buffers())[n]) for n, b in net.named_buffers())

    # .training tells the truth across mode changes, whichever module the call is made on
    net.eval()
    assert not any(m.training for m in net.modules())
    net.train()
    net.backbone.train()
    for m in net.modules():
        if isinstance(m, train.ConvBNLeaky):
            m.train()
            assert m.training and m.conv_block[1].training == (not m.frozen)


def test_frozen_block_refuses_an_input_that_requires_grad():
    blk = train.ConvBNLeaky(4, 8, 3, padding=1, backend="torch", frozen=True).train()
    assert not blk.conv_block[1].training and not any(p.requires_grad for p in blk.parameters())
    x = torch.randn(2, 4, 5, 5)
    y = blk(x, residual=torch.randn(2, 8, 5, 5))
    assert y.grad_fn is None and not y.requires_grad
    with pytest.raises(RuntimeError, match="x requires grad"):
        blk(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="residual requires grad"):
        blk(x, residual=torch.randn(2, 8, 5, 5, requires_grad=True))
    with torch.no_grad():
        assert blk(x.clone().requires_grad_(True)).grad_fn is None
    blk.conv_block[1].train()                   # by hand, on the sub-module: the block puts it back
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    blk(x)
    assert not blk.conv_block[1].training
    assert all(torch.equal(v, before[k]) for k, v in blk.state_dict().items())


def test_frozen_stages_is_orthogonal_to_backbone_batchnorm_eval(batch):
    """With backbone_batchnorm_eval the unfrozen backbone stages normalise with their running statistics too, but still train."""
    x, cot = batch
    torch.manual_seed(3)
    net = train.OrienMaskYOLO(3, 80, backend="torch", frozen_stages=2, backbone_batchnorm_eval=True).train()
    before = {n: b.clone() for n, b in net.named_buffers()}
    T.step(net, x, cot)
    for n, p in net.named_parameters():
        assert (p.grad is None) == (_stage(n) <= 2), n
    for n, b in net.named_buffers():
        assert torch.equal(b, before[n]) == (_stage(n) <= 6), n


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def _without(sd, drop):
    """sd without the keys `drop` selects, with torch's version metadata kept: a BatchNorm of the current version (2) must find
    its counter, only older checkpoints get one filled in by torch itself."""
    out = type(sd)((k, v) for k, v in sd.items() if not drop(k))
    out._metadata = sd._metadata
    return out


def test_checkpoint_keys_and_the_missing_counter():
    plain = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", frozen_stages=3)
    assert list(net.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert all(a.shape == b.shape for a, b in zip(net.parameters(), plain.parameters()))
    assert "backbone.conv1.conv_block.1.num_batches_tracked" in net.state_dict()
    _randomise_buffers(plain, 9)
    sd = plain.state_dict()
    # what the reference's FrozenBatchNorm2d would write: no counter for the frozen blocks
    lean = _without(sd, lambda k: k.endswith("num_batches_tracked") and _stage(k) <= 3)
    assert len(lean) == len(sd) - sum(1 for s in arch.fpnplus_convs() if _stage(s.name) <= 3)
    assert net.load_state_dict(lean, strict=True).missing_keys == []
    assert "backbone.conv1.conv_block.1.num_batches_tracked" not in lean      # the caller's dict is not filled in
    for k, v in net.state_dict().items():
        if k in lean:
            assert torch.equal(v, sd[k]), k
        else:
            assert int(v) == 0, k                # the block keeps its own counter
    net.load_state_dict(sd, strict=True)          # and a full checkpoint loads as before
    assert int(net.state_dict()["backbone.conv1.conv_block.1.num_batches_tracked"]) == 5
    # an unfrozen block still needs its counter, in the frozen model and in the plain one
    holed = _without(sd, lambda k: k == "backbone.conv4.0.conv_block.1.num_batches_tracked")
    for m in (net, plain):
        with pytest.raises(RuntimeError, match="backbone.conv4.0.conv_block.1.num_batches_tracked"):
            m.load_state_dict(holed, strict=True)
    with pytest.raises(RuntimeError, match="num_batches_tracked"):
        plain.load_state_dict(lean, strict=True)


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("bad", [True, False, 7, -1, 2.0, "3", None])
def test_bad_frozen_stages_raise(bad):
    with pytest.raises(ValueError, match="frozen_stages"):
        train.OrienMaskYOLOFPNPlus(3, 80, frozen_stages=bad)


def test_freeze_backbone_still_raises_and_names_the_argument():
    for freeze in (True, 3):
        with pytest.raises(NotImplementedError, match="frozen_stages"):
            train.OrienMaskYOLOFPNPlus(3, 80, freeze_backbone=freeze)
        with pytest.raises(NotImplementedError, match="frozen_stages"):
            train.OrienMaskYOLO(3, 80, freeze_backbone=freeze, frozen_stages=2)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_optimizer_holds_only_the_trainable_tensors(monkeypatch):
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", frozen_stages=6)
    monkeypatch.setattr(O, "SGD", torch.optim.SGD)         # a CPU box: look at what the class is called with
    opt = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, net)
    held = [p for g in opt.param_groups for p in g["params"]]
    outside = [s for s in arch.fpnplus_convs() if not s.name.startswith("backbone.")]
    assert len(outside) == len(list(arch.fpnplus_convs())) - 52
    assert len(held) == sum(3 if s.bn else 2 for s in outside)
    assert [id(p) for p in held] == [id(p) for n, p in net.named_parameters() if not n.startswith("backbone.")]
    grouped = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4,
                                           param_groups=dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)), 1, net)
    assert sorted(id(p) for g in grouped.param_groups for p in g["params"]) == sorted(id(p) for p in held)


def test_convert_sync_batchnorm_leaves_frozen_blocks_alone():
    net = train.convert_sync_batchnorm(train.OrienMaskYOLO(3, 80, frozen_stages=4))
    blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
    assert any(m.frozen for m in blocks) and any(not m.frozen for m in blocks)
    assert all(m.sync == (not m.frozen) for m in blocks)


def test_build_train_model_passes_frozen_stages_through(monkeypatch):
    """The builder hands the config's keys to the model class (the move to the current device is taken out: no GPU here)."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, frozen_stages=4)
    net = builder.build_train_model(cfg)
    assert net.frozen_stages == 4 and cfg["frozen_stages"] == 4
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == [n for n, _ in net.named_parameters() if _stage(n) <= 4]
    del cfg["frozen_stages"]
    plain = builder.build_train_model(cfg)
    assert plain.frozen_stages == 0 and all(p.requires_grad for p in plain.parameters())
    with pytest.raises(ValueError, match="frozen_stages"):
        builder.build_train_model(dict(cfg, frozen_stages=True))
