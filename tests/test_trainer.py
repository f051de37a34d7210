"""GPU: orienmask_amd.trainer.Trainer end to end on the trainable model with every HIP backend (bit-repeatable), the HIP SGD step
and SyntheticLossLoader: 6 images of 64 x 64, B = 2, accumulate = 2, 2 epochs.  The sync-free loop against the reference's loop from
the same seed, resume from the sync-free run's epoch1.pth, and no synchronising call between two counter reads."""
import os
import types

import pytest
import torch

import loss_counter_cases as cases

pytestmark = pytest.mark.gpu

HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")
SYNC_DEBUG = hasattr(torch.cuda, "set_sync_debug_mode")


def _config(tmp_path, name, **kw):
    c = dict(n_gpu=1, accumulate=2, epochs=2, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off", log_freq=1,
             log_dir=str(tmp_path), name=name,
             model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=cases.NUM_CLASSES, **HIP),
             loss=dict(type="OrienMaskYOLOMultiScaleLoss", **cases.loss_kwargs()),
             optimizer=dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4),
             lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[4], gamma=0.5))
    c.update(kw)
    return c


def _run(dev, config, sync_free, resume=None):
    from orienmask_amd import builder, optim, train
    from orienmask_amd.tester import SyntheticLossLoader
    from orienmask_amd.trainer import Trainer

    class Recording(Trainer):
        """Keeps every epoch's log; in the sync-free loop, from epoch 2 on, everything between two reads of the counter runs
        under torch.cuda.set_sync_debug_mode('error'): a synchronising call there raises.  (Epoch 1 is left out: it builds the
        optimizer's tables and the kernels' workspaces, as the first epoch of a resumed run does.)  Where the mode does not exist, this part is skipped and the test only
        compares the two loops' results."""
        results, strict = None, False

        def _log_result(self, result):
            self.results = (self.results or []) + [dict(result)]
            super()._log_result(result)

        def _checked(self, read, n_iter):
            if self.strict:
                torch.cuda.set_sync_debug_mode("default")
            try:
                return super()._checked(read, n_iter)
            finally:
                if self.strict:
                    self.strict_reads += 1
                    torch.cuda.set_sync_debug_mode("error")

        def _train_epoch(self, epoch):
            self.strict = self.sync_free and SYNC_DEBUG and epoch >= 2 and self.start_epoch == 1
            self.strict_reads = 0
            if self.strict:
                torch.cuda.set_sync_debug_mode("error")
            try:
                return super()._train_epoch(epoch)
            finally:
                if self.strict:
                    torch.cuda.set_sync_debug_mode("default")
                    self.strict = False

    torch.manual_seed(7)
    model = builder.build(config["model"], train).to(dev)
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
    scheduler = builder.build(config["lr_scheduler"], optim, optimizer=optimizer)
    loader = SyntheticLossLoader(6, cases.BATCH, size=(cases.IMAGE, cases.IMAGE), seed=0, gts_per_image=cases.GTS_PER_IMAGE,
                                 num_classes=cases.NUM_CLASSES, device=dev)
    t = Recording(model, loss, optimizer, scheduler, config, loader, None, None, dev,
                  types.SimpleNamespace(resume=resume, weights=None), sync_free=sync_free)
    t.train()
    torch.cuda.synchronize(dev)
    return t


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev = torch.device("cuda:0")
    tmp = tmp_path_factory.mktemp("trainer")
    free = _run(dev, _config(tmp, "free"), sync_free=True)
    strict_reads = free.strict_reads
    host = _run(dev, _config(tmp, "host", save_freq=5), sync_free=False)
    resumed = _run(dev, _config(tmp, "free", save_freq=5), sync_free=True, resume=os.path.join(free.checkpoint_dir, "epoch1.pth"))
    return free, host, resumed, strict_reads


def _momentum(t):
    sd = t.optimizer.state_dict()["state"]
    return [sd[k]["momentum_buffer"] for k in sorted(sd)]


def test_both_loops_train_the_same_weights(runs):
    free, host, _, _ = runs
    assert free.sync_free and not host.sync_free
    a, b = free.model.state_dict(), host.model.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ma, mb = _momentum(free), _momentum(host)
    assert len(ma) == len(mb) == len(list(free.model.parameters()))
    for x, y in zip(ma, mb):
        assert torch.equal(x, y)
    assert all(torch.isfinite(v).all() for v in a.values()) and free.lr_scheduler.last_epoch == 4       # 2 steps per epoch


def test_train_logs_agree(runs):
    """Raw keys equal, derived keys within the bound of tests/loss_counter_cases.py."""
    free, host, _, _ = runs
    raw = cases.raw_keys(free.loss)
    assert len(free.results) == len(host.results) == 2
    for fr, hr in zip(free.results, host.results):
        assert list(fr) == list(hr) == ["train_loss"] + ["train_" + k for k in free.loss.loss_id]
        for key in fr:
            print(key, fr[key], hr[key])
            if key[len("train_"):] in raw:
                assert fr[key] == hr[key], key
            else:
                assert abs(fr[key] - hr[key]) <= cases.DERIVED_BOUND * abs(hr[key]), (key, fr[key], hr[key])
        assert fr["train_loss"] > 0


def test_resume_reproduces_epoch_two(runs):
    free, _, resumed, _ = runs
    assert resumed.start_epoch == 2 and len(resumed.results) == 1
    a, b = free.model.state_dict(), resumed.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(_momentum(free), _momentum(resumed)):
        assert torch.equal(x, y)
    assert resumed.results[0] == free.results[1]


def test_no_synchronising_call_between_counter_reads(runs):
    """The sync-free run of the fixture went through epoch 2 with set_sync_debug_mode('error') outside the counter reads (see
    Recording); it finished, so nothing raised.  Skipped parts where the mode is unavailable: this whole check."""
    free, _, _, strict_reads = runs
    if not SYNC_DEBUG:
        pytest.skip("torch.cuda.set_sync_debug_mode is not available: the sync check of the sync-free batches is skipped")
    assert strict_reads == 3             # steps 4 and 6 (writer_freq 2) and the end of the epoch: the batches lie between them
    assert torch.cuda.get_sync_debug_mode() == 0


def test_train_tool_on_synthetic_images(built, tmp_path):
    """tools/train.py --config <json> --synthetic N: builder.build_trainer end to end, without a dataset."""
    import importlib.util
    import json
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("om_train_tool", os.path.join(repo, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = _config(tmp_path, "tool", seed=3, epochs=1, train_loader=dict(batch_size=cases.BATCH))
    path = tmp_path / "config.json"
    path.write_text(json.dumps(config))
    tool.main(["--config", str(path), "--synthetic", "4"])
    (run,) = [d for d in os.listdir(tmp_path) if d.startswith("tool_")]
    ck = torch.load(os.path.join(tmp_path, run, "epoch1.pth"), weights_only=False, map_location="cpu")
    assert ck["epoch"] == 1 and ck["config"]["epochs"] == 1 and ck["config"]["val_loader"] is None
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values())
    assert os.path.exists(os.path.join(tmp_path, run, "train.log"))


def test_validation_epoch_and_its_table(built, tmp_path):
    """One epoch with a 2-batch validation loader and a stub COCOMetrics: Trainer._val_epoch (the deferred counter through
    tester.validate, the val/* scalars) and the VAL / COCO branch of _log_result.  The val_log against the host path's validate on
    the same weights: raw keys equal, derived keys within the bound of tests/loss_counter_cases.py."""
    import json
    from orienmask_amd import builder, optim, train
    from orienmask_amd.tester import SyntheticLossLoader, validate
    from orienmask_amd.trainer import Trainer
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev = torch.device("cuda:0")

    class Coco:
        """The COCOMetrics surface the trainer and validate touch."""
        with_mask, metric_keys = True, ["AP", "AP50"]
        bbox_eval_stats, segm_eval_stats = [0.25, 0.5], [0.125, 0.375]

        def reset(self):
            self.bbox_results, self.segm_results = [], []

        def to_coco_format(self, info, detections):
            return dict(bbox=[i["id"] for i in info], segm=[i["id"] for i in info])

        def update_results(self, fmt):
            self.bbox_results += fmt["bbox"]
            self.segm_results += fmt["segm"]

        def coco_eval(self):
            assert self.bbox_results == self.segm_results == [0, 1, 2, 3]
            return dict(bbox_AP=0.25, bbox_AP50=0.5, segm_AP=0.125, segm_AP50=0.375)

    class Recording(Trainer):
        results = None

        def _log_result(self, result):
            self.results = (self.results or []) + [dict(result)]
            super()._log_result(result)

    config = _config(tmp_path, "val", epochs=1, save_freq=5)
    torch.manual_seed(7)
    model = builder.build(config["model"], train).to(dev)
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
    scheduler = builder.build(config["lr_scheduler"], optim, optimizer=optimizer)
    kw = dict(size=(cases.IMAGE, cases.IMAGE), gts_per_image=cases.GTS_PER_IMAGE, num_classes=cases.NUM_CLASSES, device=dev)
    train_loader, val_loader = SyntheticLossLoader(2, cases.BATCH, seed=0, **kw), SyntheticLossLoader(4, cases.BATCH, seed=50, **kw)
    t = Recording(model, loss, optimizer, scheduler, config, train_loader, val_loader, lambda predict: None, dev,
                  types.SimpleNamespace(resume=None, weights=None), coco_metrics=Coco())
    assert t.sync_free
    t.train()
    (result,) = t.results
    val_keys = ["val_loss"] + ["val_" + k for k in loss.loss_id + loss.metric_id] + ["val_bbox_AP", "val_bbox_AP50", "val_segm_AP",
                                                                                      "val_segm_AP50"]
    assert list(result) == ["train_loss"] + ["train_" + k for k in loss.loss_id] + val_keys
    assert not model.training                                         # _val_epoch left the model in eval mode, as the reference's
    want = validate(model, loss, None, val_loader)                    # the host path, one rank, same weights
    raw = cases.raw_keys(loss)
    for key, w in want.items():
        if key[len("val_"):] in raw:
            assert result[key] == w, key
        else:
            assert abs(result[key] - w) <= cases.DERIVED_BOUND * abs(w), (key, result[key], w)
    assert result["val_loss"] > 0 and result["val_cross_scale_obj_neg"] >= 0
    log = open(os.path.join(t.checkpoint_dir, "train.log")).read()
    assert "VAL |" in log and "BBOX |" in log and "SEGM |" in log and "avg_iou |" in log
    assert "BBOX 0.250 0.500" in log and "SEGM 0.125 0.375" in log
    path = os.path.join(t.checkpoint_dir, "scalars.jsonl")
    if os.path.exists(path):                                          # else a SummaryWriter's event file holds them
        tags = {json.loads(line)["tag"] for line in open(path)}
        assert {"val/loss", "val/bbox_AP", "val/S08_recall50", "val/cross_scale_loss_sum"} <= tags
