"""CPU: the dataset half of builder.build_trainer -- build_dataloader and DeviceLoader over a two-image dataset in the reference's
format, without iterating onto a device."""
import random

import torch

import segm_decode_np as S
from test_segm_decode_cpu import write_dataset


def _loader_config(tmp_path, **kw):
    list_file, image_dir, anno_file, src = write_dataset(str(tmp_path))
    cfg = dict(type="DataLoader", batch_size=2, shuffle=False, num_workers=0, drop_last=False, pin_memory=False,
               dataset=dict(type="COCODataset", list_file=list_file, image_dir=image_dir, anno_file=anno_file),
               transform=dict(type="COCOTransform", pipeline=S.train_pipeline((96, 96))),
               collate=dict(type="collate"))
    cfg.update(kw)
    return cfg, src


def test_build_dataloader_resolves_the_reference_config(tmp_path):
    from orienmask_amd import builder, transform
    cfg, src = _loader_config(tmp_path)
    before = repr(cfg)
    loader = builder.build_dataloader(cfg, torch.device("cpu"))
    assert repr(cfg) == before                                        # the caller's dicts are not mutated
    assert isinstance(loader, builder.DeviceLoader) and isinstance(loader.loader, transform.DataLoader)
    inner = loader.loader
    assert isinstance(inner.dataset, transform.COCODataset) and isinstance(inner.dataset.transform, transform.COCOTransform)
    assert inner.collate_fn.func is transform.collate and inner.batch_size == 2 and not inner.drop_last and inner.num_workers == 0
    assert isinstance(inner.sampler, torch.utils.data.SequentialSampler)
    # what the trainer reads off a loader
    assert len(loader) == 1 and loader.batch_size == 2 and loader.dataset is inner.dataset and loader.sampler is inner.sampler
    assert len(loader.dataset.CAT2LABEL) == 80 and loader.dataset.with_mask
    # the host half runs: one planned batch of both images (the device half is tests/test_segm_decode.py's)
    random.seed(1)
    torch.manual_seed(1)
    (planned,) = list(inner)
    assert planned.N == 6 and planned.segm is not None and [i["id"] for i in planned.info] == [s["info"]["id"] for s in src]
    # the collate entry is optional, as in the reference
    cfg.pop("collate")
    assert builder.build_dataloader(cfg, torch.device("cpu")).loader.collate_fn.func is transform.collate


def test_build_dataloader_distributed_takes_a_sampler_for_shuffle(tmp_path):
    import torch.distributed as dist
    from torch.utils.data.distributed import DistributedSampler
    from orienmask_amd import builder
    cfg, _ = _loader_config(tmp_path, shuffle=True)
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"), rank=0, world_size=1)
    try:
        loader = builder.build_dataloader(cfg, torch.device("cpu"), is_distributed=True)
    finally:
        dist.destroy_process_group()
    assert isinstance(loader.sampler, DistributedSampler) and loader.sampler.shuffle is True
    assert loader.sampler is loader.loader.sampler and cfg["shuffle"] is True
    loader.sampler.set_epoch(3)                                       # what Trainer._train_epoch calls
    assert loader.sampler.epoch == 3 and len(loader) == 1
