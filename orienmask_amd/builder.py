"""The reference's type-keyed registry for the inference path, and the builders of the training path up to ``build_trainer``.

Mirrors /root/reference/trainer/builder.py:61-77: ``build(cfg, module)`` looks ``cfg['type']`` up in a
module and calls it with the remaining keys; ``build_postprocess`` pops ``nms`` and injects the bound
NMS function as ``nms_func``.  Reference config dicts (/root/reference/config/base.py:219-236) go in
unchanged; unlike the reference, the caller's dicts are not mutated.
"""
import functools

from . import eval as _eval
from . import model as _model


def build(config, module, **kwargs):
    cfg = dict(config)
    cfg.update(kwargs)
    return getattr(module, cfg.pop("type"))(**cfg)


def build_func_partial(config, module, **kwargs):
    cfg = dict(config)
    cfg.update(kwargs)
    return functools.partial(getattr(module, cfg.pop("type")), **cfg)


def build_postprocess(config, device):
    """/root/reference/trainer/builder.py:73-77: `nms` is optional (no entry -> the default batched_nms)."""
    cfg = dict(config)
    nms_config = cfg.pop("nms", None)
    nms = build_func_partial(nms_config, _eval) if nms_config else None
    return build(cfg, _eval, nms_func=nms, device=device)


def build_model(config, device, weights=None):
    """config['model'] -> HIP-backed model on `device`, optionally loading a reference checkpoint
    ({'state_dict': ...} or a raw state_dict, strict) as infer.py:79-83 does."""
    import torch
    from .pack import unwrap_checkpoint
    cfg = dict(config)
    cfg["pretrained"] = None
    net = build(cfg, _model)
    if weights is not None:
        sd = torch.load(weights, map_location="cpu", weights_only=False) if isinstance(weights, str) else weights
        net.load_state_dict(unwrap_checkpoint(sd), strict=True)
    return net.to(device).eval()


def load_checkpoint(path_or_obj):
    """Reads what the reference's trainer writes (/root/reference/trainer/base.py:143-152):
    {'epoch', 'state_dict', 'optimizer', 'lr_scheduler', 'monitor_best', 'config'} -- or a bare state_dict,
    which infer.py also accepts (/root/reference/infer.py:81-83).  Returns (state_dict, train_config or None)."""
    import torch
    obj = torch.load(path_or_obj, map_location="cpu", weights_only=False) if isinstance(path_or_obj, str) else path_or_obj
    if isinstance(obj, dict) and isinstance(obj.get("state_dict"), dict):
        return obj["state_dict"], obj.get("config")
    return obj, None


def build_tester(config, checkpoint, test_loader, device=None, on_batch=None):
    """trainer/builder.py:43-58 on the HIP path: the MODEL config comes from the checkpoint's own
    train config (builder.py:45,50), weights are loaded strictly (:52), the postprocess from the test config.
    `checkpoint` is a path or an already loaded object; `test_loader` any iterable of batches."""
    import torch
    from .tester import Tester
    state_dict, train_config = load_checkpoint(checkpoint)
    if train_config is None or "model" not in train_config:
        raise ValueError("checkpoint has no 'config' with a 'model' entry (needed by build_tester, builder.py:45)")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(train_config["model"], device, weights=state_dict)
    postprocess = build_postprocess(config["postprocess"], device=device)
    return Tester(model, postprocess, test_loader, device, on_batch=on_batch)


def build_optimizer(config, accumulate, model, is_distributed=False):
    """trainer/builder.py:118-130 against orienmask_amd.optim: the learning rate is divided by `accumulate`; an optional
    `param_groups` entry is resolved by orienmask_amd.optim.param_groups with `base_lr` / `weight_decay` injected from the
    optimizer's; a DistributedDataParallel wrapper is looked through (`.module`).  `config['type']` "SGD", "HipAdam" and "HipAdamW" are
    the HIP steps (with their `max_grad_norm` / `nonfinite` / `ema_decay` / `ema_warmup` keys), any other torch.optim name -- "Adam"
    and "AdamW" included -- is torch's.  The caller's dicts are not mutated."""
    import copy
    from . import optim as _optim
    model = model.module if is_distributed else model
    cfg = copy.deepcopy(config)
    cfg["lr"] = cfg["lr"] / accumulate
    groups_cfg = cfg.pop("param_groups", None)
    if groups_cfg:
        groups_cfg["base_lr"] = cfg["lr"]
        groups_cfg["weight_decay"] = cfg["weight_decay"]
        params = _optim.param_groups(model, **groups_cfg)
    else:
        params = [p for p in model.parameters() if p.requires_grad]
    return build(cfg, _optim, params=params)


def build_train_model(config, is_distributed=False, ignore_pretrained=False):
    """trainer/builder.py:80-88 against orienmask_amd.train: the model of config (a reference `model` dict, optionally with
    `backend`, `conv_backend`, `conv_forward`, `route_backend`, `frozen_stages`, `amp` and `conv_grad`, which are passed on to the model class) on the current device, in training mode as a freshly built nn.Module is.  The caller's dict is not mutated.
    is_distributed=True is the reference's lines 85-87: the blocks are converted to synchronised batch statistics
    (train.convert_sync_batchnorm, the default process group) and the model is returned inside DistributedDataParallel on the
    current device.  It needs an initialised default process group and raises NotImplementedError without one."""
    import torch
    from . import train as _train
    if is_distributed:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise NotImplementedError("build_train_model(is_distributed=True): SyncBatchNorm / DistributedDataParallel need an initialised "
                                      "default process group; call torch.distributed.init_process_group first")
    cfg = dict(config)
    if ignore_pretrained:
        cfg["pretrained"] = None
    net = build(cfg, _train)
    dev = torch.device("cuda", torch.cuda.current_device())
    net = net.to(dev)
    if is_distributed:
        from torch.nn.parallel import DistributedDataParallel
        net = DistributedDataParallel(_train.convert_sync_batchnorm(net), device_ids=[dev.index])
    return net


class DeviceLoader:
    """A DataLoader whose collate is orienmask_amd.transform.collate, seen as the loader the epoch loops expect: iterating it
    yields the reference collate's tuples on `device` (transform.device_batches); ``len``, ``dataset``, ``sampler`` and
    ``batch_size`` are the DataLoader's."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, device
        self.dataset, self.sampler, self.batch_size = loader.dataset, getattr(loader, "sampler", None), loader.batch_size

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from . import transform as _transform
        return _transform.device_batches(self.loader, self.device)


def build_dataloader(config, device, is_distributed=False):
    """trainer/builder.py:91-105 against orienmask_amd.transform: the transform (COCOTransform), the dataset (COCODataset /
    VOCDataset), the collate (`collate`, the default) and torch's DataLoader, wrapped in a DeviceLoader; with is_distributed a
    DistributedSampler replaces `shuffle`.  The caller's dicts are not mutated."""
    import copy
    from . import transform as _transform
    cfg = copy.deepcopy(config)
    dataset_cfg = cfg.pop("dataset")
    dataset = build(dataset_cfg, _transform, transform=_transform.build_transform(cfg.pop("transform")))
    collate_fn = build_func_partial(cfg.pop("collate", {"type": "collate"}), _transform)
    if is_distributed:
        from torch.utils.data.distributed import DistributedSampler
        cfg["sampler"] = DistributedSampler(dataset, shuffle=cfg.pop("shuffle", False))
    return DeviceLoader(build(cfg, _transform, dataset=dataset, collate_fn=collate_fn), device)


def build_trainer(config, args, device, train_loader=None, sync_free=None):
    """trainer/builder.py:22-40 on the HIP path: seeds, loaders, postprocess, the training model, the loss with a backward
    (orienmask_amd.train), the optimizer (lr / accumulate), the scheduler and ``orienmask_amd.trainer.<config['trainer']>``.
    `args` carries ``resume`` and ``weights`` (either makes the model ignore ``pretrained``).  `train_loader`: use this
    loader instead of building config['train_loader'] (tools/train.py --synthetic); a config without a 'val_loader' entry trains
    without validation; `sync_free` is passed to the trainer."""
    import random
    import numpy as np
    import torch
    from . import optim as _optim
    from . import train as _train
    from . import trainer as _trainer
    from .dist import world_info
    random.seed(config["seed"])
    np.random.seed(config["seed"])
    torch.manual_seed(config["seed"])
    torch.cuda.manual_seed_all(config["seed"])
    is_distributed = world_info()[1] > 1
    if train_loader is None:
        train_loader = build_dataloader(config["train_loader"], device, is_distributed)
    val_loader = build_dataloader(config["val_loader"], device, is_distributed) if config.get("val_loader") else None
    postprocess = build_postprocess(config["postprocess"], device=device) if config.get("postprocess") else None
    ignore_pretrained = bool(getattr(args, "resume", None) or getattr(args, "weights", None))
    model = build_train_model(config["model"], is_distributed, ignore_pretrained)
    loss = build(config["loss"], _train)
    optimizer = build_optimizer(config["optimizer"], config["accumulate"], model, is_distributed)
    lr_scheduler = build(config["lr_scheduler"], _optim, optimizer=optimizer)
    trainer_type = getattr(_trainer, config.get("trainer", "Trainer"))
    return trainer_type(model, loss, optimizer, lr_scheduler, config, train_loader, val_loader, postprocess, device, args,
                        sync_free=sync_free)
