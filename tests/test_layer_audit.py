"""Teacher-forced audit of every layer of the HIP forward against float64.

Each layer's INPUT is taken from what the HIP forward itself stored (keep_activations(True) + layer_output): the previous layer's
output, the up-sampled / concatenated slices in front of neck16.0 / neck8.0 / neck4.0, the residual source of every *.conv.1.  The
layer's output is recomputed from that input in float64 on the GPU (torch matmul over gathered patches: conv, BatchNorm folded in
float64 from the state dict with eps = 1e-5, LeakyReLU 0.1, residual; bias only for the plain heads) and compared with the layer's
HIP output.  Each layer's error is then that layer's alone, at its true shape, tile and wiring inside the network -- where the
end-to-end checks (1e-4 of the heads' scale; 1e-2 under fp16) cannot see a layer that is 50x outside its own kernel's bound, nor
an error confined to low-scale channels, one M tile, one N tile of a ragged cout or one image.

Which elements.  A layer with fewer than FULL_PIXELS output pixels is rebuilt whole.  A larger one is rebuilt at a sampled set
of output pixels, with ALL output channels: the first and last row, in implicit-GEMM row order (b, y, x), of every M tile of the
tile size layer_kernels() reports; every image-border pixel of the first and last image; for Winograd layers complete output
rows y = 0..3 (mod 4) of the first, a middle and the last row group (first and last image); and RANDOM_PIXELS seeded uniform
pixels.

Bounds.  Let s_c be the folded BatchNorm scale of output channel c (1 for the plain heads) and N = ||w x||_2 = sqrt(conv(x^2, w^2))
the L2 norm of the products that make one output element, computed alongside it.  A fp32-accumulated dot product of K terms with
(relative) operand error u per product is off by at most u ||w x||_1 <= u sqrt(K) N; the errors of a real kernel are not all of
one sign and scale with N, which -- unlike the tensor's largest value -- is small exactly where the channel is small, so the
per-element bound sees a wrong low-scale channel that a tensor-scale check cannot.
  * f32 and f32_split (fp32 outputs):
      per layer      max |got - want| <= SCALE_TOL = 1e-5 x max |want|.  The single-layer tests hold their kernels to 2e-6 on
                     zero-mean data; inside the network the inputs are LeakyReLU outputs with a large common mode, the sums
                     cancel more, and the first MI355X run measured up to 2.9e-6 (f32, backbone.conv5.0) and 4.9e-6 (split
                     operands, trained weights, backbone.conv5.4.conv.1) -- each element of those layers within its own
                     bound below, so the per-element bound is the tight pin and this one the coarse one;
      per element    |got - want| <= EPS |s_c| N + 2^-22 (|want| + |t_c| + |res|): the first term is the convolution sum
                     (operand representation + accumulation order, Winograd transforms included), the second the fp32 epilogue:
                     the folded scale s_c and shift t_c are stored in fp32 and the multiply-add, LeakyReLU and the residual add
                     round to fp32 (a few roundings of 2^-24 each of the result, of the shift where it cancels against the sum,
                     and of the residual where |res| exceeds the result; no res term without a residual).
  * f16 (fp16 activations and weights, fp32 accumulation, one rounding to fp16; the reference rounds x and w exactly as the
    forward does -- weights to fp16 but the stem's, which reads the fp32 image):
      per element    |got - want| <= 1/2 ulp_fp16(want) + EPS16 |s_c| N + 2^-22 (|want| + |t_c| + |res|) -- one final
                     rounding, the sum, and the same fp32 epilogue as above; the fp32-output heads have no rounding term;
      per layer      at least 98 % of the elements equal fp16(want) exactly (test_conv_f16_layer_matches_torch's rule).
    F16_FWD_TOL of the end-to-end tests stays; this is the first tight pin of the fp16 forward inside the network.
  EPS, EPS_WINO and EPS16 were set from the first MI355X run: 4x the worst observed EPS_obs = max (|got - want| - epilogue
  terms) / (|s_c| N) over all layers and configurations (printed per layer with pytest -s; see the constants).  The Winograd
  kernels (wino*: fp32 F(2x2) / F(2x4), split-operand F(4,3) along the rows) get their own EPS_WINO, 4x larger: their rounding
  happens on TRANSFORMED tiles, which mix 6 input columns with coefficients up to 5, so an element's error follows the magnitude
  of its tile's neighbours rather than its own products -- largest under the trained weights' outlier channels.
  * Split-operand runs also assert that the forward's status word is 0 (the range guard did not re-run the batch with fp32
    operands; had it, the audit would read the split workspace, so it is an error here rather than a silent f32 audit).

Teeth (inside test_layer_audit, fp32-output configurations).  For the sampled elements of a few layers the output of fp16-OPERAND arithmetic (x and w rounded
to fp16, products summed exactly) -- what split operands with their lo halves dropped would give -- must be rejected by the
per-element check by a factor of at least TEETH = 8 on the GEMM-form layers (measured: 20x at the least) -- the worst element's error is at
least 8x its bound -- and of TEETH_WINO = 2 on the Winograd layers, whose EPS_WINO is 4x looser (measured: 5.4x at the least).  One element
whose channel is swapped with its neighbour inside one N tile must fail the check too.

The wiring table (wiring()) is written once here and pinned against the oracle's own forward on the CPU
(tests/test_host_cpu.py::test_audit_wiring_table_matches_the_oracle), and
tests/test_host_cpu.py::test_layer_audit_covers_every_chooser_kernel ties the configurations below to the tile chooser.
"""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, fixture_weights_and_input
from oracle import orienmask_ref as R
from orienmask_amd import arch, lib as omlib, synth

pytestmark = pytest.mark.gpu

FULL_PIXELS = 65536
RANDOM_PIXELS = 4096
SCALE_TOL = 1e-5
# 4x the worst EPS_obs of the first MI355X run (module docstring): GEMM-form kernels (implicit GEMM, stem) 1.35e-5 (f32,
# backbone.conv6.0 at bs 6); Winograd kernels 5.35e-5 (split operands, trained weights, backbone.conv4.1.conv.1); fp16 2.08e-6
EPS = 5.4e-5
EPS_WINO = 2.14e-4
EPS16 = 8.3e-6
TEETH = 8.0
TEETH_WINO = 2.0
TEETH_LAYERS = ("backbone.conv4.0", "backbone.conv5.3.conv.1", "neck16.0", "neck4.0", "orien_head.4")

# (id, model class name, precision, weights, (B, H, W)); weights: "synth" = synth_state_dict(8, obj_bias=-16, head_gain=4) of the
# model, or a tests/golden fixture whose weights AND input are used
AUDIT_CONFIGS = [
    ("f32-b1-544", "OrienMaskYOLOFPNPlus", "f32", "synth", (1, 544, 544)),
    ("f32-b6-544", "OrienMaskYOLOFPNPlus", "f32", "synth", (6, 544, 544)),
    ("f32-b2-320x416", "OrienMaskYOLOFPNPlus", "f32", "synth", (2, 320, 416)),
    ("split-b32-544", "OrienMaskYOLOFPNPlus", "f32_split", "synth", (32, 544, 544)),
    ("split-b1-160x128", "OrienMaskYOLOFPNPlus", "f32_split", "synth", (1, 160, 128)),
    ("split-b3-64x96", "OrienMaskYOLOFPNPlus", "f32_split", "synth", (3, 64, 96)),
    ("split-stress-b2-544", "OrienMaskYOLOFPNPlus", "f32_split", "fwd_stress_f544_b2.npz", (2, 544, 544)),
    ("split-trained-b2-544", "OrienMaskYOLOFPNPlus", "f32_split", "fwd_trained_f544_b2.npz", (2, 544, 544)),
    ("f16-b2-544", "OrienMaskYOLOFPNPlus", "f16", "synth", (2, 544, 544)),
    ("f16-b1-160x128", "OrienMaskYOLOFPNPlus", "f16", "synth", (1, 160, 128)),
    ("yolo-split-b2-320x416", "OrienMaskYOLO", "f32_split", "synth", (2, 320, 416)),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# wiring: what every layer reads
def wiring(model="OrienMaskYOLOFPNPlus"):
    """{layer: (inputs, residual)} in graph order.  inputs: list of (producer, nearest up-sampling factor) concatenated along the
    channels in this order ("x" is the image); residual: the producer added after the activation, or None."""
    plus = model == "OrienMaskYOLOFPNPlus"
    t = {"backbone.conv1": ([("x", 1)], None)}
    prev = "backbone.conv1"
    for idx, _, nblocks in arch.DARKNET_STAGES:
        s = "backbone.conv%d" % idx
        t[s + ".0"] = ([(prev, 1)], None)
        prev = s + ".0"
        for j in range(1, nblocks + 1):
            b = "%s.%d.conv" % (s, j)
            t[b + ".0"] = ([(prev, 1)], None)
            t[b + ".1"] = ([(b + ".0", 1)], prev)         # x + conv(conv(x)): the block's input is the residual
            prev = b + ".1"
    x32, x16, x8, x4 = "backbone.conv6.4.conv.1", "backbone.conv5.8.conv.1", "backbone.conv4.8.conv.1", "backbone.conv3.2.conv.1"

    def neck(p, first):
        t[p + ".0"] = (first, None)
        for i in range(1, 5):
            t["%s.%d" % (p, i)] = ([("%s.%d" % (p, i - 1), 1)], None)

    neck("neck32", [(x32, 1)])
    neck("neck16", [("route32.0", 2), (x16, 1)])            # up-sampled route first, backbone feature second
    neck("neck8", [("route16.0", 2), (x8, 1)])
    neck("neck4", [("skip32.0", 8), ("skip16.0", 4), ("skip8.0", 2), ("skip4", 1)] if plus else [("route8.0", 2), (x4, 1)])
    t["route32.0"] = ([("neck32.4", 1)], None)
    t["route16.0"] = ([("neck16.4", 1)], None)
    if not plus:
        t["route8.0"] = ([("neck8.4", 1)], None)
    for s in (8, 16, 32):
        t["bbox_head%d.0" % s] = ([("neck%d.4" % s, 1)], None)
        t["bbox_head%d.1" % s] = ([("bbox_head%d.0" % s, 1)], None)
    if plus:
        for s in (32, 16, 8):
            t["skip%d.0" % s] = ([("neck%d.4" % s, 1)], None)
        t["skip4"] = ([(x4, 1)], None)
    t["orien_head.0"] = ([("neck4.4", 1)], None)
    for i in range(1, 6):
        t["orien_head.%d" % i] = ([("orien_head.%d" % (i - 1), 1)], None)
    order = [s.name for s in arch.model_convs(model)]
    assert sorted(order) == sorted(t), set(order) ^ set(t)
    return {n: t[n] for n in order}


def record_oracle_calls(forward, sd, x):
    """Run an oracle forward with _cbl / _plain wrapped: {name: (input, residual or None, output)}."""
    rec = {}
    raw_cbl, raw_plain = R._cbl, R._plain

    def cbl(sd_, name, x_, stride=1, res=None):
        out = raw_cbl(sd_, name, x_, stride, res)
        rec[name] = (x_, res, out)
        return out

    def plain(sd_, name, x_):
        out = raw_plain(sd_, name, x_)
        rec[name] = (x_, None, out)
        return out

    R._cbl, R._plain = cbl, plain
    try:
        forward(sd, x)
    finally:
        R._cbl, R._plain = raw_cbl, raw_plain
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU audit
@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _tile_m(kernel):
    m = re.search(r"<(\d+),(\d+)", kernel)
    return int(m.group(1)) if m else 0


def _sample_pixels(B, Ho, Wo, kernel, seed):
    """Flat (b, y, x) row indices of the output pixels to rebuild (sorted, unique)."""
    M = B * Ho * Wo
    if M < FULL_PIXELS:
        return torch.arange(M)
    idx = [torch.from_numpy(np.random.default_rng(seed).integers(0, M, RANDOM_PIXELS))]
    bm = _tile_m(kernel)
    if bm:
        starts = torch.arange(0, M, bm)
        idx += [starts, torch.clamp(starts + bm - 1, max=M - 1)]
    ys, xs = torch.arange(Ho), torch.arange(Wo)
    for b in sorted({0, B - 1}):
        base = b * Ho * Wo
        idx += [base + xs, base + (Ho - 1) * Wo + xs, base + ys * Wo, base + ys * Wo + Wo - 1]
        if "wino" in kernel:
            groups = sorted({0, (Ho // 4) // 2, (Ho - 1) // 4})
            rows = torch.tensor([y for g in groups for y in range(4 * g, min(4 * g + 4, Ho))])
            idx.append((base + rows[:, None] * Wo + xs[None, :]).reshape(-1))
    return torch.unique(torch.cat(idx))


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _folded(sd, spec, dev):
    """(weights float64 [cout, k*k*cin] in (ky, kx, c) order, scale s_c, shift) of a layer; BatchNorm folded in float64."""
    if spec.bn:
        p = spec.name + ".conv_block."
        w = sd[p + "0.weight"]
        s = sd[p + "1.weight"].double() / torch.sqrt(sd[p + "1.running_var"].double() + arch.BN_EPS)
        shift = sd[p + "1.bias"].double() - sd[p + "1.running_mean"].double() * s
    else:
        w = sd[spec.name + ".weight"]
        s = torch.ones(spec.cout, dtype=torch.float64)
        shift = sd[spec.name + ".bias"].double()
    return w, s.to(dev), shift.to(dev)


def _ulp16(v):
    """fp16 unit in the last place at |v| (subnormal spacing 2^-24 below 2^-14)."""
    _, e = torch.frexp(v.abs())
    return torch.clamp(torch.ldexp(torch.ones_like(v), (e - 11).to(torch.int32)), min=2.0 ** -24)


def _layer_reference(parts, w, s, shift, spec, pix, Ho, Wo, res_view, f16_weights):
    """float64 output, product norm, fp16-operand output and residual at flat output pixels `pix` (all channels).
    parts: NHWC views [B, Hi, Wi, C_i] at the layer's input resolution, concatenated along C."""
    dev = s.device
    k, st, pad = spec.ksize, spec.stride, spec.ksize // 2
    wd = w.to(dev)
    if f16_weights:
        wd = wd.half()
    wm = wd.double().permute(0, 2, 3, 1).reshape(spec.cout, -1)          # [cout, (ky, kx, c)]
    wm16 = wd.half().double().permute(0, 2, 3, 1).reshape(spec.cout, -1)
    K = wm.shape[1]
    Hi, Wi = parts[0].shape[1], parts[0].shape[2]
    want, norm, want16, resv = [], [], [], []
    chunk = max(256, (1 << 25) // K)
    for c0 in range(0, pix.numel(), chunk):
        p = pix[c0:c0 + chunk].to(dev)
        b, y, x = p // (Ho * Wo), (p // Wo) % Ho, p % Wo
        cols = []
        for ky in range(k):
            for kx in range(k):
                yy, xx = y * st + ky - pad, x * st + kx - pad
                ok = ((yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)).double()[:, None]
                yc, xc = yy.clamp(0, Hi - 1), xx.clamp(0, Wi - 1)
                cols.append(torch.cat([v[b, yc, xc].double() for v in parts], 1) * ok)
        patch = torch.cat(cols, 1)                                        # [n, (ky, kx, c)]
        want.append(patch @ wm.t())
        norm.append(torch.sqrt((patch * patch) @ (wm * wm).t()))
        want16.append(patch.half().double() @ wm16.t())
        if res_view is not None:
            resv.append(res_view[b, y, x].double())
    want, norm, want16 = torch.cat(want), torch.cat(norm), torch.cat(want16)
    res = torch.cat(resv) if resv else None

    def epilogue(acc):
        out = acc * s + shift
        if spec.bn:
            out = torch.where(out > 0, out, out * arch.LEAKY_SLOPE)
        return out + res if res is not None else out

    return epilogue(want), s.abs() * norm, epilogue(want16), res


def _check(got, want, sn, shift, res, f16_out, eps):
    """(ratio tensor to the per-element bound, observed eps tensor)."""
    epi = 2.0 ** -22 * (want.abs() + shift.abs())
    if res is not None:
        epi = epi + 2.0 ** -22 * res.abs()
    d = (got - want).abs()
    if f16_out:
        epi = epi + 0.5 * _ulp16(want)
    bound = eps * sn + epi
    ratio = d / bound.clamp(min=1e-300)
    eps_obs = torch.where(sn > 0, torch.clamp(d - epi, min=0) / sn.clamp(min=1e-300), torch.zeros_like(d))
    return ratio, eps_obs


def _model(model, precision, sd, dev):
    from orienmask_amd import model as M
    net = getattr(M, model)(3, 80).eval().set_precision(precision)
    net.load_state_dict(sd, strict=True)
    return net.to(dev)


def _weights_and_input(cfg_model, weights, shape):
    B, H, W = shape
    if weights == "synth":
        return (synth.synth_state_dict(8, obj_bias=-16.0, head_gain=4.0, model=cfg_model),
                synth.synth_image_batch(31, B, H, W))
    g = np.load(GOLDEN + "/" + weights)
    assert (int(g["batch"]), *[int(v) for v in g["size"]]) == (B, H, W)
    return fixture_weights_and_input(g)


@pytest.mark.parametrize("cfg", AUDIT_CONFIGS, ids=[c[0] for c in AUDIT_CONFIGS])
def test_layer_audit(dev, cfg):
    """Every layer of one configuration, teacher-forced, against float64 (module docstring: samples and bounds); and the
    bounds' teeth on TEETH_LAYERS (fp32-operand configurations)."""
    cid, model, precision, weights, (B, H, W) = cfg
    sd, x = _weights_and_input(model, weights, (B, H, W))
    net = _model(model, precision, sd, dev)
    net.keep_activations(True)
    xd = x.to(dev)
    with torch.no_grad():
        out = net(xd)
    torch.cuda.synchronize()
    if precision == "f32_split":
        assert out.flags() == 0, "%s: the range guard tripped (the batch would be re-run with fp32 operands)" % cid
    f16 = precision == "f16"
    kernels = dict(net.layer_kernels(B, H, W))
    specs = {s.name: s for s in arch.model_convs(model)}
    heads = {"bbox_head32.1": out[0][0], "bbox_head16.1": out[1][0], "bbox_head8.1": out[2][0],
             "orien_head.5": torch.cat([out[0][1], out[1][1], out[2][1]], 1)}
    shape = (B, 3, H, W)

    def view(name):
        return _nhwc(heads[name] if name in heads else net.layer_output(name, shape))

    failures, teeth = [], []
    worst_eps = 0.0
    for li, (name, (inputs, res_name)) in enumerate(wiring(model).items()):
        spec = specs[name]
        div = arch.layer_div(spec)
        Ho, Wo = H // div, W // div
        Hi, Wi = Ho * spec.stride, Wo * spec.stride
        parts = []
        for p, _ in inputs:
            v = _nhwc(xd) if p == "x" else view(p)
            if v.shape[1] != Hi:            # a producer stored at its own resolution: read it up-sampled
                u = Hi // v.shape[1]
                v = v.repeat_interleave(u, 1).repeat_interleave(u, 2)
            assert v.shape[1:3] == (Hi, Wi), (name, p, tuple(v.shape))
            parts.append(v)
        got_full = view(name)
        up = got_full.shape[1] // Ho
        if up > 1:          # an up-sampling layer stores its output replicated at the concat buffer's resolution
            own = got_full[:, ::up, ::up]
            assert torch.equal(got_full, own.repeat_interleave(up, 1).repeat_interleave(up, 2)), (cid, name, "replication")
            got_full = own
        assert got_full.shape[1:] == (Ho, Wo, spec.cout), (cid, name, tuple(got_full.shape))
        kern = kernels[name]
        pix = _sample_pixels(B, Ho, Wo, kern, seed=li)
        w, s, shift = _folded(sd, spec, dev)
        f16_weights = f16 and name != "backbone.conv1"
        want, sn, want16, res = _layer_reference(parts, w, s, shift, spec, pix, Ho, Wo,
                                                 view(res_name) if res_name else None, f16_weights)
        pd = pix.to(dev)
        got = got_full[pd // (Ho * Wo), (pd // Wo) % Ho, pd % Wo].double()
        f16_out = f16 and name not in heads
        if f16_out:
            want_r = want.half().double()
        assert torch.isfinite(got).all(), (cid, name, "non-finite output")
        eps = EPS16 if f16 else EPS_WINO if "wino" in kern else EPS
        ratio, eps_obs = _check(got, want, sn, shift, res, f16_out, eps)
        scale = want.abs().max().item()
        scale_err = (got - want).abs().max().item() / max(scale, 1e-30)
        j = int(torch.argmax(ratio).item())
        n, c = j // spec.cout, j % spec.cout
        pv = int(pix[n]); where = (pv // (Ho * Wo), c, (pv // Wo) % Ho, pv % Wo)
        worst = ratio.view(-1)[j].item()
        eobs = eps_obs.max().item()
        worst_eps = max(worst_eps, eobs)
        line = "%-22s %-26s %-42s px %7d  scale err %.2e  worst ratio %.3f at (b,c,y,x)=%s  eps_obs %.2e" % (
            cid, name, kern, pix.numel(), scale_err, worst, where, eobs)
        if f16_out:
            exact = (got == want_r).double().mean().item()
            line += "  fp16-exact %.4f" % exact
            if exact < 0.98:
                failures.append("%s: only %.4f of the elements equal fp16(want)" % (line, exact))
        print(line)
        if worst > 1.0:
            failures.append(line)
        if not f16 and scale_err > SCALE_TOL:
            failures.append("%s: tensor-scale error %.2e > %.0e" % (line, scale_err, SCALE_TOL))
        if not f16 and name in TEETH_LAYERS:
            r16, _ = _check(want16, want, sn, shift, res, False, eps)
            swapped = got.clone()
            swapped[0, 0], swapped[0, 1] = got[0, 1], got[0, 0]
            rs, _ = _check(swapped, want, sn, shift, res, False, eps)
            teeth.append((name, kern, r16.max().item(), rs.max().item()))
            print("%-22s %-26s teeth: fp16-operand worst ratio %.1f, channel 0<->1 swap ratio %.3g" % (cid, name, teeth[-1][2],
                                                                                                     teeth[-1][3]))
    print("%-22s worst eps_obs over the layers: %.3e" % (cid, worst_eps))
    del net, out, heads
    torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)
    for name, kern, r16, rs in teeth:
        need = TEETH_WINO if "wino" in kern else TEETH
        assert r16 >= need, (cid, name, kern, "fp16-operand arithmetic is only %.1f x its bound (< %g)" % (r16, need))
        assert rs > 1.0, (cid, name, "a swapped channel pair passes the per-element check")
