"""One fused convolution layer (convolution, per-channel scale and shift, LeakyReLU 0.1, residual) as a test case: the host tensors
of a seeded draw and their float64 expectation, for the tests of the single-layer entries in tests/test_hip_parity.py.  Plain torch
on the CPU; tests/test_conv_cases_cpu.py holds the expectation to a per-pixel evaluation that does not use conv2d.

The draw order is part of the contract -- x (NCHW), w / sqrt(cin k k), rand + 0.5, randn * 0.2, then the residual when there is
one -- so that a test that moves its construction here keeps feeding its kernel the same bits."""
import torch


class LayerCase:
    """LayerCase(seed, (B, H, W, cin, cout, k, stride, leaky, use_res), half=False).  Attributes: x, w, scale, shift, res (NCHW,
    res None without a residual; x, w and res are rounded to fp16 after the draw when `half`), want = expected(x) in float64, g
    the generator (for further draws behind the case's own), and the shape fields."""

    def __init__(self, seed, shape, half=False):
        self.B, self.H, self.W, self.cin, self.cout, self.k, self.stride, self.leaky, self.use_res = shape
        B, H, W, cin, cout, k, stride = shape[:7]
        self.Ho, self.Wo = H // stride, W // stride
        self.g = g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        self.scale = torch.rand(cout, generator=g) + 0.5
        self.shift = torch.randn(cout, generator=g) * 0.2
        res = torch.randn(B, cout, self.Ho, self.Wo, generator=g) if self.use_res else None
        if half:
            x, w, res = x.half(), w.half(), res.half() if self.use_res else None
        self.x, self.w, self.res = x, w, res
        self.want = self.expected(x)

    def expected(self, x):
        """The layer's float64 output (NCHW) for the input x"""
        want = torch.nn.functional.conv2d(x.double(), self.w.double(), None, self.stride, self.k // 2)
        want = want * self.scale.double().view(1, -1, 1, 1) + self.shift.double().view(1, -1, 1, 1)
        if self.leaky:
            want = torch.where(want > 0, want, want * 0.1)
        if self.use_res:
            want = want + self.res.double()
        return want

    def padded(self, cout_pad, e=None):
        """scale and shift as the kernels read them: cout_pad long, zero beyond cout; with the exponents e of split weights
        (cout_pad of them), the scale is the split one, scale * 2^-e"""
        sp = torch.zeros(cout_pad); sp[:self.cout] = self.scale
        hp = torch.zeros(cout_pad); hp[:self.cout] = self.shift
        if e is not None:
            sp = (sp.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double())).float()
        return sp, hp

    @staticmethod
    def nhwc(t, dev):
        """an NCHW host tensor as a contiguous NHWC device tensor (None stays None)"""
        return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dev)

