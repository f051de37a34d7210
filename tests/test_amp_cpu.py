"""CPU tests of mixed precision (amp='bf16' of orienmask_amd.train's models and ConvBNLeaky): the bit-level bf16 rounding the GPU
tests pin the kernels to, the option's refusals, the 'torch' comparator on CPU tensors, the C-ABI surface of the _bf16 entry points
and the plumbing through builder.build_train_model and tools/train.py.  No GPU compute."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
import bf16_np as Q
from orienmask_amd import builder, lib as omlib, train

ENTRIES = ("om_bn_act_forward", "om_bn_act_backward", "om_bn_sync_stats", "om_bn_sync_forward", "om_bn_sync_backward_sums",
           "om_bn_sync_backward_dx", "om_route_concat_forward", "om_route_concat_backward")


def _torch_bits(a):
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _f32(words):
    return np.array(words, dtype=np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the rounding
DIRECTED = {
    "tie, kept bit even: down": ([0x3f808000, 0xbf808000, 0x40008000], [0x3f80, 0xbf80, 0x4000]),
    "tie, kept bit odd: up": ([0x3f818000, 0xbf818000, 0x40018000], [0x3f82, 0xbf82, 0x4002]),
    "one ulp either side of a tie": ([0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001], [0x3f80, 0x3f81, 0x3f81, 0x3f82]),
    "carry into the exponent": ([0x3fffffff, 0x3fff8000, 0x3fff7fff], [0x4000, 0x4000, 0x3fff]),
    "largest finite values round to inf": ([0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff], [0x7f80, 0xff80, 0x7f80, 0x7f7f]),
    "subnormals": ([0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x807fffff, 0x00010000],
                   [0x0000, 0x0000, 0x0000, 0x0001, 0x0002, 0x0080, 0x8080, 0x0001]),
    "zeros": ([0x00000000, 0x80000000], [0x0000, 0x8000]),
    "infinities": ([0x7f800000, 0xff800000], [0x7f80, 0xff80]),
}


@pytest.mark.parametrize("what", list(DIRECTED))
def test_rounding_restatement_on_directed_words(what):
    words, want = DIRECTED[what]
    a = _f32(words)
    got = Q.round_bits(a)
    assert got.tolist() == want, (what, [hex(v) for v in got])
    assert _torch_bits(a).tolist() == want, what


def test_rounding_restatement_equals_torch_on_random_bit_patterns():
    rng = np.random.default_rng(20)
    words = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    words = words[(words & 0x7fffffff) <= 0x7f800000]              # NaNs excluded
    assert words.size > 1000000
    a = words.view(np.float32)
    assert np.array_equal(Q.round_bits(a), _torch_bits(a))
    # every tie and every near-tie of one binade, and the words next to the exponent carry
    dense = (np.arange(0x3f800000 - 0x20000, 0x3f800000 + 0x20000, dtype=np.uint32)).view(np.float32)
    assert np.array_equal(Q.round_bits(dense), _torch_bits(dense))


def test_widening_is_exact_and_quantise_is_idempotent():
    bits = np.arange(1 << 16, dtype=np.uint16)
    bits = bits[(bits & 0x7fff) <= 0x7f80]
    wide = Q.widen(bits)
    assert np.array_equal(wide.view(np.uint32), bits.astype(np.uint32) << 16)
    assert np.array_equal(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float().numpy().view(np.uint32), wide.view(np.uint32))
    assert np.array_equal(Q.round_bits(wide), bits)
    a = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    assert np.array_equal(Q.quantise(Q.quantise(a)).view(np.uint32), Q.quantise(a).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_bf16_entries_are_declared_bound_and_exported(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    L = omlib.load()
    for name in ENTRIES:
        assert re.search(r"^int %s_bf16\(" % name, header, re.M), name
        assert omlib.SIGNATURES[name + "_bf16"] == omlib.SIGNATURES[name] and hasattr(L, name + "_bf16")
    # refused by their own names before anything is launched
    rc = L.om_bn_act_forward_bf16(None, 2, 4, 3, 3, None, None, None, None, None, 1, 0.1, 1e-5, 0.1, None, None, None, None, None, 0, None)
    assert rc != 0 and b"om_bn_act_forward_bf16" in L.om_last_error()
    rc = L.om_bn_act_backward_bf16(None, None, 2, 4, 3, 3, None, None, None, None, 1, 0.1, None, None, None, None, 0, None)
    assert rc != 0 and b"om_bn_act_backward_bf16" in L.om_last_error()
    rc = L.om_route_concat_forward_bf16(None, None, None, 0, 1, 1, 1, None, None)
    assert rc != 0 and b"om_route_concat_forward_bf16" in L.om_last_error()
    rc = L.om_route_concat_backward_bf16(None, None, None, 5, 1, 1, 1, None, None)
    assert rc != 0 and b"om_route_concat_backward_bf16" in L.om_last_error()


# ---------------------------------------------------------------------------------------------------------------- the option
@pytest.mark.parametrize("cls", [train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO])
def test_amp_refuses_the_float32_only_convolutions(cls):
    with pytest.raises(ValueError, match="amp"):
        cls(3, 80, amp="bf16", conv_backend="hip")
    with pytest.raises(ValueError, match="amp"):
        cls(3, 80, amp="bf16", conv_backend="hip", conv_forward="hip")
    for bad in ("fp16", "bfloat16", True, 16):
        with pytest.raises(ValueError, match="amp"):
            cls(3, 80, amp=bad, backend="torch")
    assert cls(3, 80, backend="torch").amp is None


def test_block_option_and_refusals():
    with pytest.raises(ValueError, match="amp"):
        train.ConvBNLeaky(4, 8, 1, amp="bf16", conv_backend="hip")
    with pytest.raises(ValueError, match="amp"):
        train.ConvBNLeaky(4, 8, 1, amp="bf16", conv_backend="hip", conv_forward="hip")
    with pytest.raises(ValueError, match="amp"):
        train.ConvBNLeaky(4, 8, 1, amp="fp16")
    blk = train.ConvBNLeaky(4, 8, 3, padding=1, backend="torch", amp="bf16")
    x = torch.randn(2, 4, 5, 5)
    y = blk(x)
    assert y.dtype == torch.bfloat16 and not torch.is_autocast_enabled("cpu")
    # a residual of the block's element type is added; the other type is refused, in both directions
    assert blk(x, residual=y.detach()).dtype == torch.bfloat16
    with pytest.raises(ValueError, match="residual"):
        blk(x, residual=y.detach().float())
    plain = train.ConvBNLeaky(4, 8, 3, padding=1, backend="torch")
    assert plain(x).dtype == torch.float32
    with pytest.raises(ValueError, match="residual"):
        plain(x, residual=y.detach())
    # the HIP block has no CPU path under amp either
    with pytest.raises(omlib.OrienMaskHipError, match="CPU|MI355X"):
        train.ConvBNLeaky(4, 8, 1, amp="bf16")(x)
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in blk.parameters())


def test_amp_model_on_the_cpu_comparator():
    """backend 'torch' under amp at 2 x 3 x 64 x 64: float32 heads, bf16 block outputs, float32 parameters, gradients and buffers,
    the reference's state_dict keys, the float32 model's head shapes.  (How close the heads are to float64 is judged on the GPU,
    tests/test_amp_model.py: with 8 values per channel at this size the batch statistics amplify any rounding.)"""
    torch.manual_seed(2)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", amp="bf16")
    ref = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    ref.load_state_dict(net.state_dict(), strict=True)
    assert net.amp == "bf16" and all(m.amp == "bf16" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    seen = {}
    for name, m in net.named_modules():
        if isinstance(m, train.ConvBNLeaky):
            m.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, out.dtype))
    x = torch.randn(2, 3, 64, 64)
    out = net(x)
    heads = [t for pair in out for t in pair]
    assert len(seen) == sum(isinstance(m, train.ConvBNLeaky) for m in net.modules()) == 86 and set(seen.values()) == {torch.bfloat16}
    assert all(h.dtype == torch.float32 for h in heads) and not torch.is_autocast_enabled("cpu")
    want = [t for pair in ref(x) for t in pair]
    assert [h.shape for h in heads] == [w.shape for w in want]
    assert all(torch.isfinite(h).all() for h in heads)
    keys = [str(k) for k in np.load(os.path.join(GOLDEN, "model_keys.npz"))["OrienMaskYOLOFPNPlus_state_dict"]]
    sd = net.state_dict()
    assert list(sd) == keys
    assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    sum(h.sum() for h in heads).backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() for p in net.parameters())
    # checkpoints move both ways, strictly
    ref.load_state_dict(sd, strict=True)
    net.load_state_dict(ref.state_dict(), strict=True)
    assert int(sd["backbone.conv1.conv_block.1.num_batches_tracked"]) == 1
    # frozen stages run their eval phase in bf16 too
    frozen = train.OrienMaskYOLO(3, 80, backend="torch", amp="bf16", frozen_stages=2)
    out = frozen(x)
    assert all(t.dtype == torch.float32 for pair in out for t in pair)


def test_convert_sync_batchnorm_keeps_amp():
    net = train.convert_sync_batchnorm(train.OrienMaskYOLO(3, 80, amp="bf16"))
    blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
    assert net.amp == "bf16" and all(m.amp == "bf16" and m.sync for m in blocks)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_build_train_model_passes_amp_through(monkeypatch):
    """The builder hands the config's keys to the model class (the move to the current device is taken out: no GPU here)."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, backend="torch", amp="bf16")
    net = builder.build_train_model(cfg)
    assert net.amp == "bf16" and cfg["amp"] == "bf16"
    del cfg["amp"]
    assert builder.build_train_model(cfg).amp is None
    with pytest.raises(ValueError, match="amp"):
        builder.build_train_model(dict(cfg, amp="bf16", conv_backend="hip"))


def test_train_tool_carries_amp_into_the_model_config():
    spec = importlib.util.spec_from_file_location("om_tools_train", os.path.join(REPO, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = dict(model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80), seed=1)
    args = tool.parse_args(["--config", "c.json", "--amp", "bf16", "--frozen-stages", "2"])
    out = tool.apply_overrides(config, args)
    assert out["model"] == dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, amp="bf16", frozen_stages=2)
    assert "amp" not in config["model"]                                    # the caller's dict is not mutated
    assert tool.apply_overrides(config, tool.parse_args(["--config", "c.json"])) is config
    with pytest.raises(SystemExit):
        tool.parse_args(["--config", "c.json", "--amp", "fp16"])
