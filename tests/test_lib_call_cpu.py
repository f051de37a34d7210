"""orienmask_amd.lib's call path (raw_args, call, launch's lookup, workspace_bytes) without a GPU: the library loads on a CPU-only
machine and refuses null pointers by name before it touches HIP."""
import ctypes

import pytest
import torch

from orienmask_amd import lib as omlib

# om_bn_act_forward with every pointer null: refused by name, nothing is launched
NULL_BN_FORWARD = (None, 2, 4, 3, 3, None, None, None, None, None, 1, 0.1, 1e-5, 0.1, None, None, None, None, None, 0, None)


def test_raw_args_turns_tensors_into_their_addresses_and_nothing_else():
    t = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    view = t[1:, 2:]                                     # starts 8 floats into the storage
    cfg, arr, h = omlib.LossCfg(), (ctypes.c_float * 3)(1, 2, 3), ctypes.c_void_p(64)
    ref, big, flt = ctypes.byref(cfg), 1 << 40, 0.1
    args = (t, view, torch.nn.Parameter(t), None, 7, flt, big, ref, arr, h, t.data_ptr() + 8, torch.empty(0))
    out = omlib.raw_args(args)
    assert out[0] == t.data_ptr() and type(out[0]) is int
    assert out[1] == view.data_ptr() == t.data_ptr() + 8 * 4 and out[1] != view.untyped_storage().data_ptr()
    assert out[2] == t.data_ptr()
    for got, want in zip(out[3:11], args[3:11]):
        assert got is want
    assert out[11] == 0                                  # an empty tensor is null, as ctypes.c_void_p(t.data_ptr()) was
    assert len(out) == len(args)


def test_call_raises_with_the_symbol_and_the_librarys_message(built):
    L = omlib.load()
    with pytest.raises(omlib.OrienMaskHipError) as raw:
        omlib.check(L.om_bn_act_forward(*NULL_BN_FORWARD), "om_bn_act_forward")
    with pytest.raises(omlib.OrienMaskHipError) as e:
        omlib.call("om_bn_act_forward", *NULL_BN_FORWARD)
    text = str(e.value)
    assert text == str(raw.value)
    assert text.startswith("om_bn_act_forward failed (code ")
    assert text.endswith(L.om_last_error().decode()) and L.om_last_error()
    # the bf16 entry reports its own name
    with pytest.raises(omlib.OrienMaskHipError, match=r"^om_bn_act_forward_bf16 failed \(code "):
        omlib.call("om_bn_act_forward_bf16", *NULL_BN_FORWARD)


def test_call_converts_tensors(built):
    """A CPU tensor in the place of a device pointer reaches the library as an address: x, gamma, beta, the statistics and y given,
    one value per channel in training mode is what it refuses (never dereferenced on the host)."""
    p = torch.zeros(64)
    with pytest.raises(omlib.OrienMaskHipError, match="more than 1 value per channel"):
        omlib.call("om_bn_act_forward", p, 1, 8, 1, 1, p, p, p, p, None, 1, 0.1, 1e-5, 0.1, None, p[32:], p, p, None, 0, None)


@pytest.mark.parametrize("name", ["om_no_such_entry", "hipMalloc", "load"])
def test_unknown_symbol_is_a_library_error(built, name):
    for fn, args in ((omlib.call, ()), (omlib.workspace_bytes, ()), (omlib.launch, (torch.device("cuda", 0),))):
        with pytest.raises(omlib.OrienMaskHipError, match=name):
            fn(name, *args)


def test_workspace_bytes(built):
    assert omlib.workspace_bytes("om_bn_act_workspace_bytes", 2, 1024, 3, 3) == 1024 * 16
    with pytest.raises(omlib.OrienMaskHipError) as e:
        omlib.workspace_bytes("om_bn_act_workspace_bytes", 0, 8, 4, 4)
    with pytest.raises(omlib.OrienMaskHipError) as raw:
        omlib.check(-1, "om_bn_act_workspace_bytes")
    assert str(e.value) == str(raw.value) and str(e.value).startswith("om_bn_act_workspace_bytes failed (code -1)")
