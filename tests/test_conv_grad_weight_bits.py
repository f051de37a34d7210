"""GPU test that pins the BITS of the convolutions' weight and bias gradients (om_conv2d_grad_weight and
om_conv2d_bf16_grad_weight, csrc/conv_dw.hip) through the C ABI.

The other suites hold exactness on integers and accuracy bars, which a reordered sum passes.  Here the sha256 of the dw bytes and of
the db bytes, and the workspace size, of seven cases per type are compared with tests/golden/conv_grad_weight_bits.json, recorded
once on an MI355X from the build before the two types' kernels became one.  The order of every addition is a function of the shape
and of the device's compute-unit count only (the splits depend on it), so the JSON records that count and a device with another
count FAILS the test: it cannot judge.

The cases are the smallest that reach every instantiation of the kernel (WCO 1, 2, 4 x 1x1, 3x3), one split and several, an open
chain (K no multiple of 32) and tail tiles in both channel dimensions.  Outputs are pre-filled with NaN, the workspace with 0xff.

    python tests/test_conv_grad_weight_bits.py      # on an MI355X: writes the JSON (not to be repeated once the golden is committed)"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import conv_grad_bf16_np as C
import conv_grad_np as G
import train_step as T
from orienmask_amd import lib as omlib

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "conv_grad_weight_bits.json")
SEED = 20261021
# (B, cin, cout, ksize, stride, H, W)
CASES = [(2, 3, 32, 3, 1, 96, 96),        # WCO 1, 3x3, several splits
         (5, 32, 64, 3, 2, 8, 8),         # WCO 2, 3x3 stride 2, one split, K = 80
         (3, 5, 7, 3, 2, 17, 17),         # tails, K = 243
         (2, 40, 130, 3, 1, 9, 7),        # WCO 4, 3x3, tail tiles in cout and cin
         (2, 64, 255, 1, 1, 17, 17),      # WCO 4, 1x1, several splits
         (4, 64, 32, 1, 1, 17, 17),       # WCO 1, 1x1, several splits
         (2, 8, 40, 1, 1, 5, 5)]          # WCO 2, 1x1, K = 50, open chain
TYPES = ("f32", "bf16")


def _key(case):
    return ",".join(str(v) for v in case)


def _compute_units(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _measure(dev, typ, case):
    """-> dict(workspace_bytes, dw, db): the query's answer and the sha256 of the two outputs' bytes."""
    L = omlib.load()
    B, cin, cout, ks, stride, H, W = case
    geom = (B, cin, H, W, cout, ks, stride)
    if typ == "f32":
        d = G.inputs(*case, SEED)
        x, dy = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["dy"]).to(dev)
        query, entry, name = L.om_conv2d_grad_workspace_bytes, L.om_conv2d_grad_weight, "om_conv2d_grad_weight"
    else:
        d = C.inputs(*case, SEED)
        x, dy = (torch.from_numpy(d[k].view(np.int16)).to(dev).view(torch.bfloat16) for k in ("x_bits", "dy_bits"))
        query, entry, name = L.om_conv2d_bf16_grad_workspace_bytes, L.om_conv2d_bf16_grad_weight, "om_conv2d_bf16_grad_weight"
    need = int(query(*geom))
    ws = torch.full((max(need, 16),), 255, dtype=torch.uint8, device=dev)
    dw = torch.full(d["w"].shape, float("nan"), device=dev)
    db = torch.full((cout,), float("nan"), device=dev)
    omlib.check(entry(T.vp(x), T.vp(dy), *geom, T.vp(dw), T.vp(db), T.vp(ws), need, omlib.current_stream_ptr(dev)), name)
    torch.cuda.synchronize(dev)
    dw, db = dw.cpu().numpy(), db.cpu().numpy()
    assert np.isfinite(dw).all() and np.isfinite(db).all(), (typ, case, "an element of dw or db was not written")
    return dict(workspace_bytes=need, dw=hashlib.sha256(dw.tobytes()).hexdigest(), db=hashlib.sha256(db.tobytes()).hexdigest())


def record(dev=None):
    """Writes the JSON from the library as built.  The golden stands for the order of the sums at the time the two types' kernels
    were merged; recording it again from a later build would pin nothing."""
    dev = dev or torch.device("cuda:0")
    out = dict(compute_units=_compute_units(dev), seed=SEED)
    for typ in TYPES:
        out[typ] = {_key(case): _measure(dev, typ, case) for case in CASES}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(dev):
    with open(PATH) as f:
        g = json.load(f)
    assert g["seed"] == SEED
    cus = _compute_units(dev)
    if cus != g["compute_units"]:
        pytest.fail("this device has %d compute units, the golden was recorded with %d: the weight gradient's splits, and so its "
                    "bits, depend on the count, so this test cannot judge here" % (cus, g["compute_units"]))
    return g


@pytest.mark.parametrize("case", CASES, ids=T.case_id)
@pytest.mark.parametrize("typ", TYPES)
def test_bits_are_the_recorded_ones(dev, golden, typ, case):
    want, got = golden[typ][_key(case)], _measure(dev, typ, case)
    print(typ, case, got)
    assert got["workspace_bytes"] == want["workspace_bytes"], (typ, case, "the split rule changed")
    assert got["dw"] == want["dw"], (typ, case, "dw has other bits")
    assert got["db"] == want["db"], (typ, case, "db has other bits")


@pytest.mark.parametrize("typ", TYPES)
def test_cases_reach_both_split_modes(dev, golden, typ):
    """A change of the split rule cannot make the multi-split (or the single-split) path vanish from this file unnoticed."""
    L = omlib.load()
    query = L.om_conv2d_grad_workspace_bytes if typ == "f32" else L.om_conv2d_bf16_grad_workspace_bytes
    sizes = [int(query(B, cin, H, W, cout, ks, stride)) for B, cin, cout, ks, stride, H, W in CASES]
    assert sizes == [golden[typ][_key(case)]["workspace_bytes"] for case in CASES]
    assert sum(s > 0 for s in sizes) >= 2, sizes
    assert sum(s == 0 for s in sizes) >= 2, sizes


if __name__ == "__main__":
    print(json.dumps(record(), indent=1, sort_keys=True))
