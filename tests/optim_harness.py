"""What the GPU tests of the optimizer steps (test_optim.py, test_clip.py, test_adam.py, test_optim_forms.py) share: the device
fixture, parameters from arrays, tensors read back in storage order, and the lines that set a step's gradients."""
import numpy as np
import pytest
import torch

from orienmask_amd import optim as O


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _param(dev, a):
    return torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev))


def _np(t):
    """The tensor's values in STORAGE order (a channels_last weight is updated in storage order)."""
    t = t.detach()
    flat = torch.as_strided(t, (t.numel(),), (1,)) if O._is_dense(t) and t.numel() else t.reshape(-1)
    return flat.cpu().numpy()


def _np_grad(p):
    """The gradient in the parameter's storage order."""
    g = p.grad.detach()
    if g.stride() != p.stride():
        g = torch.empty_like(p).copy_(g)
    return _np(g)


def _set_grads(dev, params, grads):
    """One step's gradients: None (no gradient), a tensor of the parameter's shape as it is (whatever its strides), or values to
    be laid out as the parameter."""
    for p, g in zip(params, grads):
        if g is None or (isinstance(g, torch.Tensor) and g.shape == p.shape):
            p.grad = g
        else:
            p.grad = (g if isinstance(g, torch.Tensor) else torch.from_numpy(np.asarray(g, np.float32)).to(dev)).view_as(p)
