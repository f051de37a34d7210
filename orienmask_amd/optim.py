"""The reference's ``optim`` package on the HIP path: ``builder.build(config["lr_scheduler"], orienmask_amd.optim, ...)``.

  SGD            torch.optim.SGD with the same constructor whose ``step()`` is ONE launch of om_sgd_step (csrc/optim.hip) over
                 every tensor of every parameter group
  HipAdam, HipAdamW   torch.optim.Adam / AdamW in the same way (om_adam_step)
  param_groups   the reference's optim/param_groups.py: one group per parameter with its own lr / weight_decay
  WarmupLR, PolyLR, StepWarmUpLR    the reference's optim/lr_scheduler.py
  everything else of torch.optim and torch.optim.lr_scheduler, re-exported as the reference's package re-exports it, so any other
  optimizer or scheduler type named in a config resolves to torch's -- ``Adam`` and ``AdamW`` included: the HIP Adam step is
  reached as ``type="HipAdam"`` / ``"HipAdamW"``.

The three classes subclass torch's: ``param_groups``, ``state``, ``state_dict()`` / ``load_state_dict()``, ``add_param_group``,
``zero_grad`` and torch's schedulers work as they are, and a checkpoint moves both ways between them and torch's classes.  The
arithmetic is torch's on the CPU in float32, bit for bit (Adam: except where torch's vectorised sqrt is not correctly rounded).
``step()`` never synchronises and, after a parameter's first step, allocates nothing.  What the kernels do not take is refused:
parameters that are not dense float32 tensors on a GPU, sparse gradients, ``differentiable=True``, tensor hyper-parameters, and for
Adam ``amsgrad``, ``capturable``, ``foreach=True``, ``fused=True``.  There is no eager fallback.

Four keyword-only options, attributes of the optimizer (``state_dict()`` keeps torch's keys):

  max_grad_norm=X     ``torch.nn.utils.clip_grad_norm_(params, X)`` followed by ``step()``, bit for bit, in three launches, except
                      that ``p.grad`` is NOT modified.  ``grad_norm_stats()`` reads what the steps saw (one small read; it
                      synchronises).  Every parameter must be on one device.
  nonfinite="skip"    (with max_grad_norm) a step whose gradient norm is Inf or NaN leaves parameters, state and shadows
                      bit-unchanged; the host does not learn of it during the step.  Adam's ``state[p]["step"]`` then lives on the
                      device and is read back by ``state_dict()``.  Known edge (SGD): resuming from a checkpoint taken before any
                      APPLIED step with ``dampening != 0`` makes the first applied step ``buf = (1 - dampening) * d``.
  ema_decay=D, ema_warmup=True    a float32 shadow per parameter, a bit copy of the parameter at the first ``step()``, updated inside
                      the step kernel at every APPLIED step: ``e += (p' - e) * (1 - d_k)`` with ``d_k = D``, or with warm-up
                      ``min(D, (1 + k) / (10 + k))``.  ``ema_swap()`` / ``with ema_applied():`` exchange parameters and shadows in
                      place; ``ema_state_dict(model)`` / ``load_ema_state_dict(model, state_dict, updates)`` / ``ema_updates()`` are
                      the checkpoint's side.  Every parameter must be on one device.

How a step works, the rounding of every operation and the protocols of the device-side words: DESIGN.md section 3.16.
"""
import contextlib as _contextlib
import numpy as _np
import torch as _torch
from torch.optim import *                   # noqa: F401,F403  (the reference's optim/__init__.py:1)
from torch.optim.lr_scheduler import *      # noqa: F401,F403  (optim/lr_scheduler.py:3)
from torch.optim import SGD as _TorchSGD, Adam as _TorchAdam, AdamW as _TorchAdamW
from torch.optim.lr_scheduler import LRScheduler as _LRScheduler, MultiStepLR as _MultiStepLR

from . import lib as _lib

OM_SGD_CHUNK = 4096         # include/orienmask_hip.h
OM_SGD_SKIP, OM_SGD_FIRST, OM_SGD_NESTEROV, OM_SGD_MAXIMIZE, OM_SGD_HAS_MOMENTUM, OM_SGD_HAS_WD = 1, 2, 4, 8, 16, 32
OM_SGD_DEVICE_FIRST = 64    # "first step" is decided on the device (om_sgd_clip_step's valid_since)
OM_CLIP_SKIP_NONFINITE = 1  # om_sgd_clip_step's mode bits
# om_sgd_clip_step's state block, in 8-byte words (NORM, COEF, SUM, MAX are float64, the others int64)
(OM_CLIP_NORM_OFF, OM_CLIP_COEF_OFF, OM_CLIP_SKIP_OFF, OM_CLIP_STEPS_OFF, OM_CLIP_SUM_OFF, OM_CLIP_MAX_OFF, OM_CLIP_CLIPPED_OFF,
 OM_CLIP_NONFINITE_OFF, OM_CLIP_FIRST_NONFINITE_OFF, OM_CLIP_STATE_DOUBLES) = range(10)
NONFINITE_MODES = ("propagate", "skip")
# om_sgd_clip_ema_step's EMA state block, in 8-byte words (UPDATES is int64, OMD float64)
OM_EMA_UPDATES_OFF, OM_EMA_OMD_OFF, OM_EMA_STATE_DOUBLES = range(3)
OM_ADAM_SKIP, OM_ADAM_MAXIMIZE, OM_ADAM_HAS_WD, OM_ADAM_DECOUPLED, OM_ADAM_DEVICE_COUNTED = 1, 2, 4, 8, 16
OM_ADAM_ROW_BYTES = 96
ADAM_BIAS_MAX_ROWS = 2 ** 20    # the longest bias table of the device-counted Adam step
# om_sgd_tensor / om_sgd_chunk as numpy records
TENSOR_ROW = _np.dtype([("param", "<u8"), ("grad", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("neg_lr", "<f4"), ("weight_decay", "<f4"),
                        ("momentum", "<f4"), ("one_minus_dampening", "<f4"), ("flags", "<u4"), ("reserved", "<u4", (3,))])
assert TENSOR_ROW.itemsize == 64
# om_adam_tensor (csrc/optim.hip)
ADAM_ROW = _np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("n", "<i8"), ("lr", "<f8"),
                      ("w", "<f4"), ("beta2", "<f4"), ("omb2", "<f4"), ("eps", "<f4"), ("weight_decay", "<f4"), ("dm", "<f4"),
                      ("nss", "<f4"), ("bc2s", "<f4"), ("bias_table", "<i4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
assert ADAM_ROW.itemsize == OM_ADAM_ROW_BYTES
_RING = 4                   # pinned staging buffers per device


def plan_chunks(counts):
    """The work list of om_sgd_step for tensors of ``counts`` elements: int32 [n_chunks, 2] rows (tensor, chunk), tensor by
    tensor; chunk k of a tensor covers its elements [k * OM_SGD_CHUNK, min(n, (k + 1) * OM_SGD_CHUNK))."""
    counts = _np.asarray(counts, dtype=_np.int64).reshape(-1)
    if counts.size == 0 or (counts <= 0).any():
        raise ValueError("every tensor needs at least one element")
    per = (counts + (OM_SGD_CHUNK - 1)) // OM_SGD_CHUNK
    if int(per.max()) >= 2 ** 31 or int(per.sum()) >= 2 ** 31 or counts.size >= 2 ** 31:
        raise ValueError("too many chunks for the 32-bit chunk list")
    tensor = _np.repeat(_np.arange(counts.size, dtype=_np.int64), per)
    first = _np.cumsum(per) - per
    chunk = _np.arange(int(per.sum()), dtype=_np.int64) - _np.repeat(first, per)
    return _np.ascontiguousarray(_np.stack([tensor, chunk], axis=1).astype(_np.int32))


def chunk_ranges(plan, counts):
    """(tensor, start, stop) of every row of ``plan`` as the kernel derives them."""
    counts = _np.asarray(counts, dtype=_np.int64).reshape(-1)
    tensor = plan[:, 0].astype(_np.int64)
    start = plan[:, 1].astype(_np.int64) * OM_SGD_CHUNK
    stop = _np.minimum(start + OM_SGD_CHUNK, counts[tensor])
    return tensor, start, stop


def _layout(t):
    """Strides of the dimensions that have more than one element (the others do not place anything)."""
    return tuple(st for sz, st in zip(t.shape, t.stride()) if sz != 1)


def _is_dense(t):
    """True when the tensor's elements fill numel() consecutive storage slots, each once (any permutation of a contiguous one)."""
    expect = 1
    for st, sz in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if st != expect:
            return False
        expect *= sz
    return True


def _check_param(p, who="orienmask_amd.optim.SGD"):
    if not isinstance(p, _torch.Tensor):
        raise TypeError("optimizer can only optimize Tensors, but one of the params is " + _torch.typename(p))
    if not p.is_cuda or p.dtype != _torch.float32 or p.layout is not _torch.strided:
        raise _lib.OrienMaskHipError("%s updates float32 tensors on an MI355X device; got %s %s on %s "
                                     "(there is no CPU or eager fallback)" % (who, p.layout, p.dtype, p.device))
    if p.numel() == 0:
        raise _lib.OrienMaskHipError("%s: a parameter without elements" % who)
    if not _is_dense(p):
        raise _lib.OrienMaskHipError("%s: a parameter must be dense in its storage (shape %s, strides %s)"
                                     % (who, tuple(p.shape), p.stride()))


def _conform_state(p, b, who, what):
    """State tensor ``b`` (``what``: its key in ``state[p]``) as the kernel walks it: checked against parameter ``p``, and copied
    into the parameter's storage order where it has another."""
    if not isinstance(b, _torch.Tensor) or b.shape != p.shape:
        raise _lib.OrienMaskHipError("%s: %s does not match its parameter's shape" % (who, what))
    if b.device != p.device or b.dtype != _torch.float32 or b.layout is not _torch.strided:
        raise _lib.OrienMaskHipError("%s: %s must be float32 on the parameter's device; got %s on %s"
                                     % (who, what, b.dtype, b.device))
    if _layout(b) != _layout(p):
        nb = _torch.empty_like(p, requires_grad=False)
        nb.copy_(b)
        b = nb
    return b


class _Plan:
    """One device's tables."""

    def __init__(self, device, params, group_of, row=None):
        row = TENSOR_ROW if row is None else row
        self.device = device
        self.params = params
        self.group_of = group_of                          # slot -> index into optimizer.param_groups
        n = len(params)
        self.n = n
        counts = [p.numel() for p in params]
        self.layouts = [_layout(p) for p in params]
        self.strides = [p.stride() for p in params]
        self.rows = _np.zeros(n, dtype=row)
        self.rows["n"] = counts
        self.param_ptrs = [p.data_ptr() for p in params]
        self.rows["param"] = self.param_ptrs
        self.states = [None] * n                          # optimizer.state[p], once the parameter has one
        self.bufs = [None] * n
        self.base_flags = [0] * n
        self.has_mom = [False] * n
        self.hyper = {}                                   # group index -> the values its rows were written from
        self.group_slots = {}
        for i, g in enumerate(group_of):
            self.group_slots.setdefault(g, []).append(i)
        self.group_slots = {g: _np.asarray(s, dtype=_np.int64) for g, s in self.group_slots.items()}
        chunks = plan_chunks(counts)
        self.n_chunks = int(chunks.shape[0])
        self.chunks = _torch.from_numpy(chunks).to(device)
        self.table = _torch.empty(n * row.itemsize, dtype=_torch.uint8, device=device)
        self.staging = [_torch.empty(n * row.itemsize, dtype=_torch.uint8).pin_memory() for _ in range(_RING)]
        self.staging_rows = [s.numpy().view(row) for s in self.staging]
        self.events = [_torch.cuda.Event() for _ in range(_RING)]
        self.turn = 0
        self.signature = [p.numel() for p in params]
        self.device_first = [False] * n                   # rows whose first step the device decides (clipping, nonfinite="skip")
        self.partials = self.valid_since = None           # om_sgd_clip_step's buffers, once a clipped step needs them
        self.shadows = None                               # the EMA shadows, slot by slot (None: not averaged), and the device
        self.shadow_ptrs = None                           # array of their addresses om_sgd_ema_step reads

    def set_shadows(self, shadows):
        """The plan's shadows, one per slot; their addresses go to the device once (again only if one is replaced)."""
        self.shadows = list(shadows)
        ptrs = _np.asarray([0 if e is None else e.data_ptr() for e in self.shadows], dtype=_np.uint64).view(_np.int64)
        self.shadow_ptrs = _torch.from_numpy(ptrs).to(self.device)

    def stage(self):
        """The host rows into the next pinned staging buffer -> (buffer, the event to record behind its copy)."""
        k = self.turn
        self.turn = (k + 1) % _RING
        ev = self.events[k]
        if not ev.query():
            ev.synchronize()                              # the copy out of this staging buffer, _RING steps ago, has not run yet
        self.staging_rows[k][:] = self.rows
        return self.staging[k], ev

    def clip_buffers(self):
        if self.partials is None:
            self.partials = _torch.empty(self.n_chunks, dtype=_torch.float64, device=self.device)
            self.valid_since = _torch.zeros(self.n, dtype=_torch.int64, device=self.device)
        return self.partials, self.valid_since


def check_clip(max_grad_norm, nonfinite, who="orienmask_amd.optim.SGD"):
    """The refusals of the two clipping options (``who`` names the class in the message)."""
    if nonfinite not in NONFINITE_MODES:
        raise ValueError("%s: nonfinite must be one of %s, got %r" % (who, NONFINITE_MODES, nonfinite))
    if max_grad_norm is None:
        if nonfinite == "skip":
            raise ValueError("%s: nonfinite='skip' needs max_grad_norm (the decision is taken from the gradient norm; a large "
                             "bound such as 1e30 skips without clipping)" % who)
        return
    if isinstance(max_grad_norm, _torch.Tensor):
        raise _lib.OrienMaskHipError("%s: max_grad_norm is a tensor; the step takes a Python number (reading a tensor back "
                                     "would synchronise)" % who)
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)):
        raise ValueError("%s: max_grad_norm must be a positive finite number or None, got %r" % (who, max_grad_norm))
    as_f32 = float(_np.float32(max_grad_norm)) if abs(max_grad_norm) < 3.5e38 else float("inf")
    if not (max_grad_norm > 0 and as_f32 > 0 and _np.isfinite(as_f32)):
        raise ValueError("%s: max_grad_norm must be positive and finite in float32, got %r" % (who, max_grad_norm))


def check_ema(ema_decay, ema_warmup=True, who="orienmask_amd.optim.SGD"):
    """The refusals of the two EMA options (``who`` names the class in the message)."""
    if ema_decay is None:
        return
    if isinstance(ema_decay, _torch.Tensor):
        raise _lib.OrienMaskHipError("%s: ema_decay is a tensor; the step takes a Python number (reading a tensor back would "
                                     "synchronise)" % who)
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < ema_decay < 1.0:
        raise ValueError("%s: ema_decay must be a number inside (0, 1) or None, got %r" % (who, ema_decay))
    if not isinstance(ema_warmup, (bool, int)):
        raise ValueError("%s: ema_warmup must be True or False, got %r" % (who, ema_warmup))


def ema_decay_at(k, decay, warmup=True):
    """d_k, the decay of EMA update number k (from 0), in float64: ``decay``, or with warm-up min(decay, (1 + k) / (10 + k))."""
    d = float(decay)
    return min(d, (1.0 + k) / (10.0 + k)) if warmup else d


class _HipStep:
    """What the HIP steps share, mixed in ahead of torch's optimizer class: the per-device plans (table rows in a pinned staging
    ring, the chunk list), the clip launches' buffers and statistics, the EMA shadows with their swap and checkpoint side.  A
    class names itself (_NAME), its row type (_ROW) and its swap entry (_SWAP_ENTRY), fills the rows in _step_plan and launches in
    _launch_plain / _launch_clipped."""

    _NAME = "orienmask_amd.optim.SGD"
    _ROW = TENSOR_ROW
    _SWAP_ENTRY = "om_ema_swap"

    def _init_hip(self, max_grad_norm, nonfinite, ema_decay, ema_warmup):
        self._plans = None
        # attributes, not defaults and not param-group entries: state_dict() keeps torch's keys
        self.max_grad_norm = max_grad_norm
        self.nonfinite = nonfinite
        self._clip_state = None                           # the device state block of the clipped step, once one ran
        self._clip_steps = 0                              # clipped step() calls so far: the step number the kernels latch
        self.ema_decay = ema_decay
        self.ema_warmup = ema_warmup
        self._ema_shadows = {}                            # parameter -> shadow; survives a rebuilt plan (load_state_dict)
        self._ema_state = None                            # the device EMA block of the clipped step, once such a step ran
        self._ema_k = 0                                   # EMA updates applied so far, as far as the host knows:
        self._ema_on_device = False                       # True after a step that may have been skipped: the device word counts
        self._ema_word_valid = False                      # the device word holds _ema_k (or, _ema_on_device, the count itself)

    def _retire_plans(self):
        """The plans are dropped (the next step builds them again); a class with state on the device alone fetches it first."""
        self._plans = None

    def _check(self, p):
        _check_param(p)

    def _launch_step(self, plan, clip, skip_mode, ema):
        """Stage the plan's rows and launch the step in its form: plain, averaged, clipped, clipped and averaged."""
        staging, ev = plan.stage()
        dev = plan.device
        stream = _torch.cuda.current_stream(dev)
        tables = (staging, plan.table, plan.n, plan.chunks, plan.n_chunks)
        with _lib.on_device(dev):
            if clip is None and ema is None:
                self._launch_plain(plan, tables, stream, None, 0.0)
            elif clip is None:
                if self._ema_on_device:                   # the step form changed after skip mode: the count comes back, once
                    self.ema_updates()
                omd = float(_np.float32(1.0 - ema_decay_at(self._ema_k, *ema)))
                self._launch_plain(plan, tables, stream, plan.shadow_ptrs, omd)
                self._ema_k += 1
                self._ema_word_valid = False
            else:
                partials, words = plan.clip_buffers()
                if self._clip_state is None or self._clip_state.device != dev:
                    self._clip_state = _torch.zeros(OM_CLIP_STATE_DOUBLES, dtype=_torch.float64, device=dev)
                self._clip_steps += 1
                clip_args = (partials, self._clip_state, words, clip, OM_CLIP_SKIP_NONFINITE if skip_mode else 0, self._clip_steps)
                if ema is None:
                    self._launch_clipped(plan, tables, stream, clip_args, None)
                else:
                    self._launch_clipped(plan, tables, stream, clip_args,
                                         (plan.shadow_ptrs, self._ema_block(dev), float(ema[0]), int(bool(ema[1]))))
                    if skip_mode:
                        self._ema_on_device = True        # only the device knows whether this step was applied
                    elif not self._ema_on_device:
                        self._ema_k += 1                  # the device word does the same
            ev.record(stream)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans = None                                # load_state_dict replaces every state dict and momentum buffer

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = None

    def add_param_group(self, param_group):
        if not isinstance(param_group, dict):
            raise TypeError("param_group must be a dict, but got " + _torch.typename(param_group))
        params = param_group["params"]
        params = [params] if isinstance(params, _torch.Tensor) else list(params)
        for p in params:
            self._check(p)
        if param_group.get("differentiable", False):
            raise _lib.OrienMaskHipError("%s: differentiable=True is not supported" % self._NAME)
        self._retire_plans()
        super().add_param_group(dict(param_group, params=params))

    # ---- tables -------------------------------------------------------------------------------------------------------------
    def _structure(self):
        return [len(g["params"]) for g in self.param_groups]

    def _build_plans(self):
        per_device = {}
        for gi, group in enumerate(self.param_groups):
            if group.get("differentiable", False):
                raise _lib.OrienMaskHipError("%s: differentiable=True is not supported" % self._NAME)
            for p in group["params"]:
                self._check(p)
                params, group_of = per_device.setdefault(p.device, ([], []))
                params.append(p)
                group_of.append(gi)
        if getattr(self, "max_grad_norm", None) is not None and len(per_device) > 1:
            raise _lib.OrienMaskHipError("%s: max_grad_norm needs every parameter on one device (the norm is global); got %s"
                                         % (self._NAME, sorted(str(d) for d in per_device)))
        averaging = getattr(self, "ema_decay", None) is not None
        if averaging and len(per_device) > 1:
            raise _lib.OrienMaskHipError("%s: ema_decay needs every parameter on one device (one count of updates, one swap); "
                                         "got %s" % (self._NAME, sorted(str(d) for d in per_device)))
        self._plans = [_Plan(dev, params, group_of, self._ROW) for dev, (params, group_of) in per_device.items()]
        if averaging:
            for plan in self._plans:
                plan.set_shadows([self._shadow_of(p) for p in plan.params])
        self._built_for = self._structure()
        self._built_clip = self._clip_key()

    def _current_plans(self):
        """The plans, built again where the groups or the form of the step changed since they were built."""
        if getattr(self, "_plans", None) is None or self._built_for != self._structure() or self._built_clip != self._clip_key():
            self._build_plans()
        return self._plans

    def _clip_key(self):
        return (getattr(self, "max_grad_norm", None) is not None, getattr(self, "nonfinite", "propagate"),
                getattr(self, "ema_decay", None) is not None)

    def _shadow_of(self, p):
        """The parameter's shadow: kept if it still fits the parameter, else a bit copy of the parameter as it is now."""
        e = self._ema_shadows.get(p)
        if e is None or e.shape != p.shape or e.device != p.device:
            e = _torch.empty_like(p, requires_grad=False)                   # dense parameter: same strides
            e.copy_(p.detach())
        elif _layout(e) != _layout(p):
            old, e = e, _torch.empty_like(p, requires_grad=False)
            e.copy_(old)
        self._ema_shadows[p] = e
        return e

    def _param_moved(self, plan, i, p, ptr):
        """The parameter's data was replaced (p.data = ..., module.to(...)): the row follows it."""
        self._check(p)
        if p.numel() != plan.signature[i]:
            self._plans = None
            raise _lib.OrienMaskHipError("%s: a parameter changed its element count; step again" % self._NAME)
        plan.layouts[i] = _layout(p)
        plan.strides[i] = p.stride()
        plan.param_ptrs[i] = ptr
        plan.rows["param"][i] = ptr
        if plan.shadows is not None and plan.shadows[i] is not None and _layout(plan.shadows[i]) != plan.layouts[i]:
            shadows = list(plan.shadows)
            shadows[i] = self._shadow_of(p)                                 # the same values in the new storage order
            plan.set_shadows(shadows)

    def _conform_grad(self, p, g):
        """A gradient in the parameter's storage order (the kernel walks the three tensors element by element in that order)."""
        if g.layout is not _torch.strided:
            raise _lib.OrienMaskHipError("%s does not support sparse gradients (got %s)" % (self._NAME, g.layout))
        out = _torch.empty_like(p, requires_grad=False)                  # dense parameter: same strides
        out.copy_(g)
        return out

    def _ema_block(self, dev):
        """The device block of om_sgd_clip_ema_step with its count word in step with the host's (a fill, no read)."""
        if self._ema_state is None or self._ema_state.device != dev:
            self._ema_state = _torch.zeros(OM_EMA_STATE_DOUBLES, dtype=_torch.int64, device=dev)
            self._ema_word_valid = self._ema_k == 0 and not self._ema_on_device
        if not self._ema_word_valid:
            self._ema_state[OM_EMA_UPDATES_OFF:OM_EMA_UPDATES_OFF + 1].fill_(self._ema_k)
            self._ema_word_valid = True
        return self._ema_state

    def step(self, closure=None):
        """One optimization step; ``closure`` (optional) re-evaluates the model and returns the loss, as torch's does."""
        loss = None
        if closure is not None:
            with _torch.enable_grad():
                loss = closure()
        _lib.load()
        max_norm, nonfinite = getattr(self, "max_grad_norm", None), getattr(self, "nonfinite", "propagate")
        check_clip(max_norm, nonfinite, self._NAME)
        decay, warmup = getattr(self, "ema_decay", None), getattr(self, "ema_warmup", True)
        check_ema(decay, warmup, self._NAME)
        plans = self._current_plans()
        with _torch.no_grad():
            for plan in plans:
                self._step_plan(plan, None if max_norm is None else float(max_norm), nonfinite == "skip",
                                None if decay is None else (decay, warmup))
        return loss

    # ---- weight EMA -----------------------------------------------------------------------------------------------------------
    def _ema_plan(self, what):
        """The one plan of an averaging optimizer, built if need be (its shadows are then bit copies of the parameters)."""
        if getattr(self, "ema_decay", None) is None:
            raise _lib.OrienMaskHipError("%s.%s: averaging is not enabled (ema_decay is None)" % (self._NAME, what))
        check_ema(self.ema_decay, self.ema_warmup, self._NAME)
        return self._current_plans()[0]

    def ema_updates(self):
        """The number of EMA updates applied so far: the host's count, or with nonfinite="skip" (only the device knows which
        steps were applied) one small device-to-host read of the count word.  That read synchronises; step() never does.  The
        count carries over when the form of the step changes between steps."""
        if self._ema_on_device:
            self._ema_k = int(self._ema_state[OM_EMA_UPDATES_OFF:OM_EMA_UPDATES_OFF + 1].cpu().numpy()[0])
            self._ema_on_device = False                   # until the next step that may be skipped
        return self._ema_k

    def ema_shadow(self, p):
        """The shadow tensor of parameter ``p`` (the live tensor the step kernel updates), or None where ``p`` is not averaged."""
        plan = self._ema_plan("ema_shadow")
        for q, e in zip(plan.params, plan.shadows):
            if q is p:
                return e
        return None

    def ema_swap(self):
        """Exchange every averaged parameter with its shadow, in place, in one launch on the current stream (om_ema_swap).  The
        tensors keep their addresses: nothing is allocated and no plan is rebuilt.  Twice restores both, bit for bit."""
        _lib.load()
        plan = self._ema_plan("ema_swap")
        for i, p in enumerate(plan.params):
            ptr = p.data_ptr()
            if ptr != plan.param_ptrs[i]:
                self._param_moved(plan, i, p, ptr)
        staging, ev = plan.stage()
        dev = plan.device
        stream = _torch.cuda.current_stream(dev)
        with _lib.on_device(dev):
            _lib.launch(self._SWAP_ENTRY, dev, staging, plan.table, plan.n, plan.chunks, plan.n_chunks, plan.shadow_ptrs, stream=stream)
            ev.record(stream)

    @_contextlib.contextmanager
    def ema_applied(self):
        """``with optimizer.ema_applied():`` the parameters hold the averaged weights inside the block and their own again after it
        (ema_swap on entry and on exit)."""
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()

    def _ema_names(self, model):
        """[(state_dict key, shadow)] of the parameters of ``model`` this optimizer averages, matched by tensor identity; a
        parameter shared by two modules appears under both names."""
        plan = self._ema_plan("ema_state_dict")
        shadow = {id(p): e for p, e in zip(plan.params, plan.shadows)}
        return [(name, shadow[id(p)]) for name, p in model.named_parameters(remove_duplicate=False) if id(p) in shadow]

    def ema_state_dict(self, model):
        """``model.state_dict()`` with every parameter this optimizer averages replaced by a copy of its shadow.  Buffers (the
        BatchNorm running statistics are moving averages already) and parameters the optimizer does not hold (frozen stages)
        are the live tensors."""
        named = self._ema_names(model)
        out = model.state_dict()
        with _torch.no_grad():
            for name, e in named:
                if name in out:
                    out[name] = e.clone()
        return out

    def load_ema_state_dict(self, model, state_dict, updates):
        """The inverse of ema_state_dict: the shadows from ``state_dict`` (keys and shapes of the averaged parameters of ``model``
        must be there; other entries are not read) and the count of applied updates."""
        if isinstance(updates, bool) or not isinstance(updates, int) or updates < 0:
            raise ValueError("%s.load_ema_state_dict: updates must be a non-negative int, got %r" % (self._NAME, updates))
        named = self._ema_names(model)
        for name, e in named:
            if name not in state_dict:
                raise _lib.OrienMaskHipError("%s.load_ema_state_dict: no entry %r in the state dict" % (self._NAME, name))
            if tuple(state_dict[name].shape) != tuple(e.shape):
                raise _lib.OrienMaskHipError("%s.load_ema_state_dict: %r has shape %s, the parameter %s"
                                             % (self._NAME, name, tuple(state_dict[name].shape), tuple(e.shape)))
        with _torch.no_grad():
            for name, e in named:
                e.copy_(state_dict[name])
        self._ema_k, self._ema_on_device, self._ema_word_valid = updates, False, False

    def ema_reset(self):
        """Forget the shadows and the count: the next plan copies the parameters as they are then."""
        self._ema_shadows = {}
        self._ema_k, self._ema_on_device, self._ema_word_valid = 0, False, False
        self._plans = None

    def grad_norm_stats(self, reset=True):
        """What the clipped steps since the last reset saw, as ONE small device-to-host read of the state block the step kernels
        keep (this synchronises; step() never does): ``steps`` (clipped step() calls), ``mean_norm`` and ``max_norm`` over the
        steps whose norm was finite (nan where there was none), ``clipped_steps`` (finite norm, coefficient < 1),
        ``nonfinite_steps`` (with nonfinite="skip": the steps that were skipped), ``first_nonfinite_step`` (the 1-based count of
        this optimizer's clipped step() calls at the first non-finite norm, 0 = none; latched, never reset), ``last_norm`` and
        ``last_coef`` (float32 values of the latest step).  ``reset``: the running counts start again."""
        if getattr(self, "max_grad_norm", None) is None and getattr(self, "_clip_state", None) is None:
            raise _lib.OrienMaskHipError("%s.grad_norm_stats: clipping is not enabled (max_grad_norm is None)" % self._NAME)
        if getattr(self, "_clip_state", None) is None:
            block = _np.zeros(OM_CLIP_STATE_DOUBLES, dtype=_np.float64)
        else:
            block = self._clip_state.cpu().numpy()
            if reset:
                self._clip_state[OM_CLIP_STEPS_OFF:OM_CLIP_FIRST_NONFINITE_OFF].zero_()
        words = block.view(_np.int64)
        steps, nonfinite = int(words[OM_CLIP_STEPS_OFF]), int(words[OM_CLIP_NONFINITE_OFF])
        finite = steps - nonfinite
        return dict(steps=steps, mean_norm=float(block[OM_CLIP_SUM_OFF]) / finite if finite else float("nan"),
                    max_norm=float(block[OM_CLIP_MAX_OFF]) if finite else float("nan"),
                    clipped_steps=int(words[OM_CLIP_CLIPPED_OFF]), nonfinite_steps=nonfinite,
                    first_nonfinite_step=int(words[OM_CLIP_FIRST_NONFINITE_OFF]),
                    last_norm=float(block[OM_CLIP_NORM_OFF]), last_coef=float(block[OM_CLIP_COEF_OFF]))


class SGD(_HipStep, _TorchSGD):
    """torch.optim.SGD (same constructor, same state, same state_dict) whose step is one HIP launch; see the module docstring."""

    def __init__(self, params, *args, max_grad_norm=None, nonfinite="propagate", ema_decay=None, ema_warmup=True, **kwargs):
        check_clip(max_grad_norm, nonfinite)
        check_ema(ema_decay, ema_warmup)
        super().__init__(params, *args, **kwargs)
        if self.defaults.get("differentiable"):
            raise _lib.OrienMaskHipError("orienmask_amd.optim.SGD: differentiable=True is not supported (the step is a HIP kernel "
                                         "outside autograd)")
        self._init_hip(max_grad_norm, nonfinite, ema_decay, ema_warmup)

    @staticmethod
    def _write_hyper(plan, gi, key):
        lr, wd, momentum, dampening, nesterov, maximize = key
        for v, name in ((lr, "lr"), (wd, "weight_decay"), (momentum, "momentum"), (dampening, "dampening")):
            if isinstance(v, _torch.Tensor):
                raise _lib.OrienMaskHipError("orienmask_amd.optim.SGD: %s is a tensor; the step takes Python numbers (reading a "
                                             "tensor back would synchronise)" % name)
        slots = plan.group_slots[gi]
        rows = plan.rows
        rows["neg_lr"][slots] = -float(lr)
        rows["weight_decay"][slots] = float(wd)
        rows["momentum"][slots] = float(momentum)
        rows["one_minus_dampening"][slots] = 1.0 - float(dampening)          # in double, rounded once (torch: alpha=1 - dampening)
        flags = ((OM_SGD_NESTEROV if nesterov else 0) | (OM_SGD_MAXIMIZE if maximize else 0) |
                 (OM_SGD_HAS_MOMENTUM if momentum != 0 else 0) | (OM_SGD_HAS_WD if wd != 0 else 0))
        for i in slots.tolist():
            plan.base_flags[i] = flags
            plan.has_mom[i] = momentum != 0
        plan.hyper[gi] = key

    def _step_plan(self, plan, clip=None, skip_mode=False, ema=None):
        """One device's step; ``clip``: None, or float max_grad_norm (then ``skip_mode``: nonfinite == "skip"); ``ema``: None, or
        (ema_decay, ema_warmup)."""
        groups = self.param_groups
        for gi in plan.group_slots:
            g = groups[gi]
            key = (g["lr"], g["weight_decay"], g["momentum"], g["dampening"], g["nesterov"], g["maximize"])
            if plan.hyper.get(gi) != key:
                self._write_hyper(plan, gi, key)
        params, layouts, strides, states, bufs, has_mom = plan.params, plan.layouts, plan.strides, plan.states, plan.bufs, plan.has_mom
        rows = plan.rows
        flags = list(plan.base_flags)
        grad_ptrs = [0] * plan.n
        keep = []
        active = 0
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                flags[i] = OM_SGD_SKIP
                continue
            ptr = p.data_ptr()
            if ptr != plan.param_ptrs[i]:
                self._param_moved(plan, i, p, ptr)
            if g.layout is not _torch.strided or (g.stride() != strides[i] and _layout(g) != layouts[i]):
                g = self._conform_grad(p, g)
                keep.append(g)
            grad_ptrs[i] = g.data_ptr()
            if has_mom[i]:
                st = states[i]
                if st is None:
                    st = states[i] = self.state[p]
                b = st.get("momentum_buffer")
                if b is None and skip_mode:
                    # this step may be skipped: zeros (a checkpoint taken before an applied step holds no garbage), and from now
                    # on the device decides which step is the tensor's first
                    b = _torch.zeros_like(p, requires_grad=False)
                    st["momentum_buffer"] = b
                    plan.device_first[i] = True
                    bufs[i] = None
                elif b is None:
                    b = _torch.empty_like(p, requires_grad=False)      # written, not read, by this step (OM_SGD_FIRST)
                    st["momentum_buffer"] = b
                    flags[i] |= OM_SGD_FIRST
                    bufs[i] = None
                if plan.device_first[i]:
                    flags[i] |= OM_SGD_DEVICE_FIRST
                if b is not bufs[i]:
                    nb = _conform_state(p, b, self._NAME, "momentum_buffer")
                    if nb is not b:
                        st["momentum_buffer"] = b = nb
                    bufs[i] = b
                    rows["buf"][i] = b.data_ptr()
            active += 1
        if active == 0:
            return
        rows["grad"] = grad_ptrs
        rows["flags"] = flags
        self._launch_step(plan, clip, skip_mode, ema)
        del keep

    def _launch_plain(self, plan, tables, stream, shadows, omd):
        if shadows is None:
            _lib.launch("om_sgd_step", plan.device, *tables, stream=stream)
        else:
            _lib.launch("om_sgd_ema_step", plan.device, *tables, shadows, omd, stream=stream)

    def _launch_clipped(self, plan, tables, stream, clip_args, ema_args):
        if ema_args is None:
            _lib.launch("om_sgd_clip_step", plan.device, *tables, *clip_args, stream=stream)
        else:
            _lib.launch("om_sgd_clip_ema_step", plan.device, *tables, *clip_args, *ema_args, stream=stream)


# ---- the Adam family -------------------------------------------------------------------------------------------------------------
def adam_bias_corrections(beta1, beta2, step):
    """(bc1, bc2s) of step number ``step`` (a Python float, as torch's _get_value returns it) in torch's own expressions,
    evaluated in Python doubles: ``1 - beta1 ** step`` and ``(1 - beta2 ** step) ** 0.5`` (``** 0.5`` is not ``sqrt``)."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return bias_correction1, bias_correction2 ** 0.5


def adam_bias_table(beta1, beta2):
    """The bias table of ``(beta1, beta2)`` for the device-counted step: float64 [rows, 2], row k = adam_bias_corrections(beta1,
    beta2, float(k)).  It ends with the first row whose two values are both exactly 1.0; from there on both stay 1.0 (the kernel
    uses 1.0 beyond the table).  Betas that need more than ADAM_BIAS_MAX_ROWS rows are refused."""
    beta1, beta2 = float(beta1), float(beta2)
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError("orienmask_amd.optim: betas must lie in [0, 1), got %r" % ((beta1, beta2),))
    if adam_bias_corrections(beta1, beta2, float(ADAM_BIAS_MAX_ROWS - 1)) != (1.0, 1.0):
        raise _lib.OrienMaskHipError("orienmask_amd.optim: nonfinite='skip' keeps the step counts on the device and reads the bias "
                                     "corrections from a table; betas %r need more than %d rows until both corrections are 1.0"
                                     % ((beta1, beta2), ADAM_BIAS_MAX_ROWS))
    rows = []
    k = 0
    while True:
        rows.append(adam_bias_corrections(beta1, beta2, float(k)))
        if rows[-1] == (1.0, 1.0):
            break
        k += 1
    return _np.asarray(rows, dtype=_np.float64).reshape(-1, 2)


class _HipAdamStep(_HipStep):
    """HipAdam's and HipAdamW's step (the base class decides ``decoupled_weight_decay``); see the module docstring."""

    _ROW = ADAM_ROW
    _SWAP_ENTRY = "om_adam_ema_swap"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), *args, max_grad_norm=None, nonfinite="propagate", ema_decay=None,
                 ema_warmup=True, **kwargs):
        check_clip(max_grad_norm, nonfinite, self._NAME)
        check_ema(ema_decay, ema_warmup, self._NAME)
        self._check_args(lr, betas)
        super().__init__(params, lr, betas, *args, **kwargs)                # torch's constructor, next in the MRO
        for group in self.param_groups:
            self._check_group(group)
        self._init_hip(max_grad_norm, nonfinite, ema_decay, ema_warmup)
        self._bias_ids = {}                               # (beta1, beta2) -> table id, in the order the tables were built
        self._bias_tables = []                            # float64 [rows, 2] each
        self._bias_dev = None                             # (device, rows tensor, directory tensor, tables in them)
        if nonfinite == "skip":
            for group in self.param_groups:               # a pair of betas the table cannot hold is refused here already
                self._bias_table_id(*group["betas"])

    @classmethod
    def _check_args(cls, lr, betas):
        """Ahead of torch's constructor, which turns tensor betas into numbers with a read-back."""
        if isinstance(lr, _torch.Tensor) or any(isinstance(b, _torch.Tensor) for b in betas):
            raise _lib.OrienMaskHipError("%s: lr and betas are Python numbers here; a tensor would have to be read back at every "
                                         "step" % cls._NAME)

    def _check_group(self, group):
        name = self._NAME
        if group.get("amsgrad", False):
            raise _lib.OrienMaskHipError("%s: amsgrad=True is not supported (there is no eager fallback)" % name)
        for key in ("capturable", "differentiable", "foreach", "fused"):
            if group.get(key, False):
                raise _lib.OrienMaskHipError("%s: %s=True is not supported: the step is this project's HIP kernel, not one of "
                                             "torch's implementations" % (name, key))
        for key in ("lr", "eps", "weight_decay"):
            if isinstance(group.get(key), _torch.Tensor):
                raise _lib.OrienMaskHipError("%s: %s is a tensor; the step takes Python numbers (reading a tensor back would "
                                             "synchronise)" % (name, key))
        if any(isinstance(b, _torch.Tensor) for b in group.get("betas", ())):
            raise _lib.OrienMaskHipError("%s: betas are tensors; the step takes Python numbers" % name)

    def add_param_group(self, param_group):
        if isinstance(param_group, dict):
            self._check_group(param_group)
        super().add_param_group(param_group)

    def _check(self, p):
        _check_param(p, self._NAME)

    # ---- step counts ------------------------------------------------------------------------------------------------------------
    def _device_counted(self):
        return getattr(self, "max_grad_norm", None) is not None and getattr(self, "nonfinite", "propagate") == "skip"

    def _sync_steps(self):
        """With nonfinite="skip" only the device knows which steps were applied: ONE small device-to-host read per plan brings the
        per-tensor counts into ``state[p]["step"]``.  Not called by step(); between two calls ``state[p]["step"]`` is stale.  The
        read is ordered behind the work of the CURRENT stream only: a caller who stepped on another stream synchronises with it
        first, as for any read of the parameters."""
        for plan in getattr(self, "_plans", None) or ():
            if not getattr(plan, "counted", False) or plan.valid_since is None:
                continue
            counts = plan.valid_since.cpu().numpy()
            for i, p in enumerate(plan.params):
                plan.steps[i] = float(counts[i])
                st = self.state.get(p)
                if st is not None and "step" in st:
                    st["step"].fill_(float(counts[i]))

    def _retire_plans(self):
        self._sync_steps()
        self._plans = None

    def _build_plans(self):
        self._sync_steps()
        super()._build_plans()
        counted = self._device_counted()
        for plan in self._plans:
            plan.counted = counted
            plan.moments = [None] * plan.n                # (exp_avg, exp_avg_sq) as the rows hold them
            plan.step_tensors = [None] * plan.n
            plan.steps = [0.0] * plan.n                   # the host's copy of state[p]["step"]
            plan.nss, plan.bc2s = [0.0] * plan.n, [1.0] * plan.n          # the rows' two per-step scalars, written as columns
            for i, p in enumerate(plan.params):
                st = self.state.get(p)
                if st is not None and "step" in st:
                    if st["step"].device.type != "cpu":   # a checkpoint of a fused or capturable torch optimizer
                        st["step"] = st["step"].cpu()
                    plan.steps[i] = float(st["step"])     # a CPU scalar, as torch keeps it unless capturable or fused
            if counted:
                plan.clip_buffers()
                plan.valid_since.copy_(_torch.tensor(plan.steps, dtype=_torch.float64).to(_torch.int64))

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def _bias_table_id(self, beta1, beta2):
        key = (float(beta1), float(beta2))
        if key not in self._bias_ids:
            self._bias_tables.append(adam_bias_table(*key))
            self._bias_ids[key] = len(self._bias_tables) - 1
        return self._bias_ids[key]

    def _bias_buffers(self, dev):
        """The bias tables on the device, one after the other, and their directory (first row, rows); uploaded when one is new."""
        if self._bias_dev is None or self._bias_dev[0] != dev or self._bias_dev[3] != len(self._bias_tables):
            lengths = [t.shape[0] for t in self._bias_tables]
            first = _np.cumsum([0] + lengths[:-1])
            rows = _np.concatenate(self._bias_tables, axis=0) if lengths else _np.ones((1, 2))
            directory = _np.stack([first, lengths], axis=1).astype(_np.int64) if lengths else _np.zeros((1, 2), _np.int64)
            self._bias_dev = (dev, _torch.from_numpy(_np.ascontiguousarray(rows)).to(dev),
                              _torch.from_numpy(_np.ascontiguousarray(directory)).to(dev), len(lengths))
        return self._bias_dev[1], self._bias_dev[2], self._bias_dev[3]

    # ---- rows -------------------------------------------------------------------------------------------------------------------
    def _write_hyper(self, plan, gi, key):
        group = self.param_groups[gi]
        self._check_group(group)
        lr, (beta1, beta2), eps, wd, maximize, decoupled = key
        slots = plan.group_slots[gi]
        rows = plan.rows
        lr, beta1, beta2, wd = float(lr), float(beta1), float(beta2), float(wd)
        rows["lr"][slots] = lr
        rows["w"][slots] = 1 - beta1                      # in double, rounded once (torch: lerp_'s weight=1 - beta1)
        rows["beta2"][slots] = beta2
        rows["omb2"][slots] = 1 - beta2
        rows["eps"][slots] = float(eps)
        rows["weight_decay"][slots] = wd
        rows["dm"][slots] = 1 - lr * wd
        if plan.counted:
            rows["bias_table"][slots] = self._bias_table_id(beta1, beta2)
        flags = ((OM_ADAM_MAXIMIZE if maximize else 0) | (OM_ADAM_HAS_WD if wd != 0 else 0) |
                 (OM_ADAM_DECOUPLED if decoupled else 0) | (OM_ADAM_DEVICE_COUNTED if plan.counted else 0))
        for i in slots.tolist():
            plan.base_flags[i] = flags
        plan.hyper[gi] = key
        plan.scalars = {}                                 # (group, step) -> (nss, bc2s), as long as no group changes

    def _step_plan(self, plan, clip=None, skip_mode=False, ema=None):
        groups = self.param_groups
        for gi in plan.group_slots:
            g = groups[gi]
            key = (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["maximize"], g.get("decoupled_weight_decay", False))
            if plan.hyper.get(gi) != key:
                self._write_hyper(plan, gi, key)
        params, layouts, strides, states, moments = plan.params, plan.layouts, plan.strides, plan.states, plan.moments
        rows, steps, group_of, scalars, counted = plan.rows, plan.steps, plan.group_of, plan.scalars, plan.counted
        nss, bc2s_col = plan.nss, plan.bc2s
        flags = list(plan.base_flags)
        grad_ptrs = [0] * plan.n
        keep = []
        stepped = []
        active = 0
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                flags[i] = OM_ADAM_SKIP
                continue
            active += 1
            ptr = p.data_ptr()
            if ptr != plan.param_ptrs[i]:
                self._param_moved(plan, i, p, ptr)
            if g.layout is not _torch.strided or (g.stride() != strides[i] and _layout(g) != layouts[i]):
                g = self._conform_grad(p, g)
                keep.append(g)
            grad_ptrs[i] = g.data_ptr()
            st = states[i]
            if st is None:
                st = states[i] = self.state[p]
            if "exp_avg" not in st:                       # torch's _init_group, at the parameter's first gradient
                st["step"] = _torch.tensor(0.0, dtype=_torch.get_default_dtype())
                st["exp_avg"] = _torch.zeros_like(p, memory_format=_torch.preserve_format, requires_grad=False)
                st["exp_avg_sq"] = _torch.zeros_like(p, memory_format=_torch.preserve_format, requires_grad=False)
                moments[i] = None
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if moments[i] is None or m is not moments[i][0] or v is not moments[i][1]:
                nm, nv = _conform_state(p, m, self._NAME, "exp_avg"), _conform_state(p, v, self._NAME, "exp_avg_sq")
                if nm is not m:
                    st["exp_avg"] = m = nm
                if nv is not v:
                    st["exp_avg_sq"] = v = nv
                moments[i] = (m, v)
                rows["exp_avg"][i] = m.data_ptr()
                rows["exp_avg_sq"][i] = v.data_ptr()
                plan.step_tensors[i] = st["step"]
            if not counted:
                # the host knows every count: this step's two scalars, as torch's _single_tensor_adam evaluates them
                k = steps[i] = steps[i] + 1.0
                sk = (group_of[i], k)
                pair = scalars.get(sk)
                if pair is None:
                    grp = groups[group_of[i]]
                    bc1, bc2s = adam_bias_corrections(grp["betas"][0], grp["betas"][1], k)
                    if len(scalars) > 4096:
                        scalars.clear()
                    pair = scalars[sk] = (-(grp["lr"] / bc1), bc2s)
                nss[i], bc2s_col[i] = pair
                stepped.append(plan.step_tensors[i])
        if active == 0:
            return
        if stepped:
            _torch._foreach_add_(stepped, 1)              # state[p]["step"], CPU scalars: as torch advances them
            rows["nss"] = nss
            rows["bc2s"] = bc2s_col
        rows["grad"] = grad_ptrs
        rows["flags"] = flags
        self._launch_step(plan, clip, skip_mode, ema)
        del keep

    def _launch_plain(self, plan, tables, stream, shadows, omd):
        _lib.launch("om_adam_step", plan.device, *tables, shadows, omd, stream=stream)

    def _launch_clipped(self, plan, tables, stream, clip_args, ema_args):
        partials, state, counts, max_norm, mode, step = clip_args
        bias, directory, n_tables = self._bias_buffers(plan.device) if plan.counted else (None, None, 0)
        shadows, ema_state, decay, warmup = ema_args if ema_args is not None else (None, None, 0.0, 0)
        _lib.launch("om_adam_clip_step", plan.device, *tables, partials, state, counts, bias, directory, n_tables, max_norm, mode,
                    step, shadows, ema_state, decay, warmup, stream=stream)


class HipAdam(_HipAdamStep, _TorchAdam):
    """torch.optim.Adam (same constructor, same state, same state_dict) whose step is this project's HIP launch, with SGD's
    ``max_grad_norm`` / ``nonfinite`` / ``ema_decay`` / ``ema_warmup``; see the module docstring."""

    _NAME = "orienmask_amd.optim.HipAdam"


class HipAdamW(_HipAdamStep, _TorchAdamW):
    """torch.optim.AdamW with the same step: the decay is ``p *= 1 - lr * weight_decay`` ahead of the update."""

    _NAME = "orienmask_amd.optim.HipAdamW"


# ---- optim/param_groups.py ------------------------------------------------------------------------------------------------------
_NORM_TYPES = (_torch.nn.BatchNorm1d, _torch.nn.BatchNorm2d, _torch.nn.BatchNorm3d, _torch.nn.SyncBatchNorm, _torch.nn.GroupNorm,
               _torch.nn.InstanceNorm1d, _torch.nn.InstanceNorm2d, _torch.nn.InstanceNorm3d, _torch.nn.LayerNorm,
               _torch.nn.LocalResponseNorm)


def param_groups(model, base_lr=1e-3, weight_decay=1e-4, norm_weight_decay=0.0, bias_lr_factor=1.0, bias_weight_decay=1e-4):
    """The reference's optim/param_groups.py: one ``{"params": [p], "lr", "weight_decay"}`` per trainable parameter, in
    ``model.modules()`` order, a shared parameter once.  Parameters of normalisation modules get ``norm_weight_decay``; a parameter
    named ``bias`` elsewhere gets ``base_lr * bias_lr_factor`` and ``bias_weight_decay``.

    Kept, not repaired: the reference never resets the decay for the next parameter (optim/param_groups.py:32 assigns the
    variable to itself), so the decay CARRIES OVER from one parameter to the next.  After the first normalisation module every
    later convolution weight gets ``norm_weight_decay``, and after a bias the weights that follow get ``bias_weight_decay``, until
    the next norm or bias changes it again.  conv / BatchNorm / conv with bias / conv gives decays weight_decay, norm, norm, norm,
    bias (the bias), bias.  This returns what the reference returns (tests/golden/optim_param_groups.npz), as aug_crop_quirk does
    for the crop."""
    groups = []
    seen = set()
    decay = weight_decay                                  # carried from parameter to parameter (see above)
    for module in model.modules():
        is_norm = isinstance(module, _NORM_TYPES)
        for name, value in module.named_parameters(recurse=False):
            if not value.requires_grad or value in seen:
                continue
            seen.add(value)
            lr = base_lr
            if is_norm:
                decay = norm_weight_decay
            elif name == "bias":
                lr = base_lr * bias_lr_factor
                decay = bias_weight_decay
            groups.append({"params": [value], "lr": lr, "weight_decay": decay})
    return groups


# ---- optim/lr_scheduler.py ------------------------------------------------------------------------------------------------------
class WarmupLR:
    """optim/lr_scheduler.py:7-21: the warm-up learning rate at iteration ``iters`` of ``warmup_iter``, in double."""

    def __init__(self, warmup_type, warmup_iter, warmup_ratio):
        if warmup_type not in ("const", "linear", "power"):
            raise AssertionError("warmup_type must be 'const', 'linear' or 'power', got %r" % (warmup_type,))
        self.type = warmup_type
        self.iter = warmup_iter
        self.ratio = warmup_ratio

    def get_warmup_lr(self, iters, base_lr):
        if self.type == "const":
            return base_lr * self.ratio
        if self.type == "linear":
            return base_lr * (self.ratio + (1 - self.ratio) * iters / self.iter)
        return base_lr * ((iters / self.iter) ** self.ratio)


class PolyLR(_LRScheduler):
    """optim/lr_scheduler.py:24-32: base_lr * (1 - last_epoch / max_iter) ** power."""

    def __init__(self, optimizer, max_iter, power=0.9, last_epoch=-1):
        self.max_iter = max_iter
        self.power = power
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        import math
        return [base_lr * math.pow(1 - self.last_epoch / self.max_iter, self.power) for base_lr in self.base_lrs]


class StepWarmUpLR(_MultiStepLR):
    """optim/lr_scheduler.py:35-48: the warm-up rate while last_epoch <= warmup_iter, torch's MultiStepLR after it (its chained
    form: the rate the optimizer holds, times gamma at a milestone -- so the rate after the warm-up is the LAST warm-up rate,
    which is base_lr for 'linear' and 'power' and base_lr * warmup_ratio for 'const', as in the reference)."""

    def __init__(self, warmup_type, warmup_iter, warmup_ratio, optimizer, milestones, gamma=0.1, last_epoch=-1):
        self.warmup = WarmupLR(warmup_type, warmup_iter, warmup_ratio)
        super().__init__(optimizer, milestones, gamma, last_epoch)

    def get_lr(self):
        if self.last_epoch > self.warmup.iter:
            return super().get_lr()
        return [self.warmup.get_warmup_lr(self.last_epoch, base_lr) for base_lr in self.base_lrs]
