"""CPU: orienmask_amd.trainer's loop, checkpoints and resume with a stub model (two nn.Linear layers) and a stub loss callable,
sync_free=False (the reference's loop: it works with any loss callable)."""
import glob
import json
import os
import types

import pytest
import torch
import torch.nn as nn

N_BATCHES = 5
CHECKPOINT_KEYS = {"epoch", "state_dict", "optimizer", "lr_scheduler", "monitor_best", "config"}       # trainer/base.py:146-153


class StubLoss:
    """The loss contract of the loop: (loss, loss_log, metric_log) and the key lists _log_result reads."""
    scales_prefix = ["S0"]
    loss_suffix = ["mse", "loss_sum"]
    metric_suffix = []
    loss_id = ["S0_mse", "S0_loss_sum", "cross_scale_mse", "cross_scale_loss_sum"]
    metric_id = []

    def __init__(self, nan_at=None):
        self.calls, self.nan_at = 0, nan_at

    def __call__(self, predict, label, training=True):
        self.calls += 1
        loss = ((predict - label[0]) ** 2).mean()
        if self.calls == self.nan_at:
            loss = loss * float("nan")
        v = loss.item()
        return loss, {"S0_mse": v, "S0_loss_sum": v, "cross_scale_mse": v, "cross_scale_loss_sum": v, "loss_sum": v}, {}


def _loader():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(4, 6, generator=g), (torch.randn(4, 2, generator=g),), [dict(id=i)]) for i in range(N_BATCHES)]


def _config(tmp_path, name, **kw):
    c = dict(n_gpu=0, accumulate=2, epochs=2, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off", log_freq=1,
             log_dir=str(tmp_path), name=name, model=dict(type="stub", hidden=8),
             optimizer=dict(type="SGD", lr=0.05, momentum=0.9, weight_decay=1e-4),
             lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[5], gamma=0.5))
    c.update(kw)
    return c


def _parts(config):
    from orienmask_amd import optim
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(6, config["model"]["hidden"]), nn.Linear(config["model"]["hidden"], 2))
    oc = dict(config["optimizer"])
    oc.pop("type")
    oc["lr"] = oc["lr"] / config["accumulate"]
    optimizer = torch.optim.SGD(model.parameters(), **oc)
    sc = dict(config["lr_scheduler"])
    scheduler = getattr(optim, sc.pop("type"))(optimizer=optimizer, **sc)
    return model, optimizer, scheduler


def _trainer(config, loss=None, resume=None, weights=None, cls=None, val_loader=None):
    from orienmask_amd.trainer import Trainer
    model, optimizer, scheduler = _parts(config)
    args = types.SimpleNamespace(resume=resume, weights=weights)
    return (cls or Trainer)(model, loss or StubLoss(), optimizer, scheduler, config, _loader(), val_loader, None,
                            torch.device("cpu"), args, sync_free=False)


def test_optimizer_steps_every_accumulate_batches_and_at_the_last(built, tmp_path):
    t = _trainer(_config(tmp_path, "steps", epochs=1))
    stepped_at, zeroed_at = [], []
    zero = t.optimizer.zero_grad
    t.optimizer.register_step_post_hook(lambda opt, a, k: stepped_at.append(t.loss.calls))
    t.optimizer.zero_grad = lambda *a, **k: (zeroed_at.append(t.loss.calls), zero(*a, **k))[1]
    t.train()
    assert stepped_at == [2, 4, 5] == zeroed_at
    assert t.lr_scheduler.last_epoch == 3
    assert t.sync_free is False
    # the scalars went somewhere: a SummaryWriter's event file, or scalars.jsonl with the reference's tags
    path = os.path.join(t.checkpoint_dir, "scalars.jsonl")
    if os.path.exists(path):
        tags = {json.loads(line)["tag"] for line in open(path)}
        assert {"lr/group0", "train/loss", "train/S0_mse"} <= tags
    else:
        assert glob.glob(os.path.join(t.checkpoint_dir, "events.*"))
    assert json.load(open(os.path.join(t.checkpoint_dir, "config.json"))) == t.config
    log = open(os.path.join(t.checkpoint_dir, "train.log")).read()
    assert "|    TRAIN |" in log and "| loss_sum |" in log and "ALL |" in log          # the plain-text table


def test_checkpoint_has_exactly_the_reference_keys(built, tmp_path):
    t = _trainer(_config(tmp_path, "keys", epochs=2, save_freq=2))
    t.train()
    d = t.checkpoint_dir
    # val_freq 1 and monitor off: every epoch takes the _save_checkpoint(epoch) branch; epoch 1 is no multiple of save_freq
    assert sorted(f for f in os.listdir(d) if f.endswith(".pth")) == ["epoch2.pth"]
    ck = torch.load(os.path.join(d, "epoch2.pth"), weights_only=False)
    assert set(ck) == CHECKPOINT_KEYS and ck["epoch"] == 2 and ck["config"] == t.config
    assert set(ck["state_dict"]) == set(t.model.state_dict())


def test_temp_checkpoint_when_not_a_validation_epoch(built, tmp_path):
    t = _trainer(_config(tmp_path, "temp", epochs=1, val_freq=2, save_freq=5))
    t.train()
    ck = torch.load(os.path.join(t.checkpoint_dir, "temp.pth"), weights_only=False)
    assert set(ck) == CHECKPOINT_KEYS and ck["epoch"] == 1
    assert sorted(f for f in os.listdir(t.checkpoint_dir) if f.endswith(".pth")) == ["temp.pth"]


def _equal_state(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal_state(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if hasattr(a, "__dict__") and type(a) is type(b) and type(a).__eq__ is object.__eq__:
        return _equal_state(vars(a), vars(b))           # a plain object in a scheduler's state (StepWarmUpLR's WarmupLR)
    return a == b


def test_resume_reproduces_the_uninterrupted_run(built, tmp_path):
    """2 epochs, resume, 2 more == 4 uninterrupted: state_dict, optimizer state (momentum buffers) and scheduler state."""
    whole = _trainer(_config(tmp_path, "whole", epochs=4))
    whole.train()
    first = _trainer(_config(tmp_path, "first", epochs=2))
    first.train()
    resumed = _trainer(_config(tmp_path, "first", epochs=4), resume=os.path.join(first.checkpoint_dir, "epoch2.pth"))
    assert resumed.start_epoch == 3 and resumed.checkpoint_dir == first.checkpoint_dir
    resumed.train()
    assert _equal_state(whole.model.state_dict(), resumed.model.state_dict())
    assert _equal_state(whole.optimizer.state_dict(), resumed.optimizer.state_dict())
    assert _equal_state(whole.lr_scheduler.state_dict(), resumed.lr_scheduler.state_dict())
    assert whole.optimizer.state_dict()["state"][0]["momentum_buffer"].abs().max() > 0
    assert not _equal_state(first.model.state_dict(), resumed.model.state_dict())
    # the three config assertions of _resume_checkpoint
    from orienmask_amd.trainer import Trainer
    for key in ("model", "optimizer", "lr_scheduler"):
        cfg = _config(tmp_path, "first", epochs=4)
        cfg[key] = dict(cfg[key], marker=1)
        model, optimizer, scheduler = _parts(_config(tmp_path, "first", epochs=4))
        with pytest.raises(AssertionError, match="differs from the checkpoint's"):
            Trainer(model, StubLoss(), optimizer, scheduler, cfg, _loader(), None, None, torch.device("cpu"),
                    types.SimpleNamespace(resume=os.path.join(first.checkpoint_dir, "epoch2.pth"), weights=None), sync_free=False)


def test_best_symlink_is_replaced(built, tmp_path):
    from orienmask_amd.trainer import Trainer

    class WithVal(Trainer):
        def _val_epoch(self, epoch):
            return {"val_loss": {1: 3.0, 2: 2.0, 3: 2.5}[epoch]}

    t = _trainer(_config(tmp_path, "best", epochs=3, monitor_mode="min", save_freq=5), cls=WithVal, val_loader=[])
    t.train()
    d = t.checkpoint_dir
    link = os.path.join(d, "best_model.pth")
    assert os.path.islink(link) and os.readlink(link) == "best_epoch2.pth"
    assert sorted(f for f in os.listdir(d) if f.endswith(".pth")) == ["best_epoch2.pth", "best_model.pth"]
    assert t.monitor_best == 2.0
    ck = torch.load(link, weights_only=False)
    assert set(ck) == CHECKPOINT_KEYS and ck["epoch"] == 2 and ck["monitor_best"] == 2.0


def test_max_iter_writes_the_batch_checkpoint_and_stops(built, tmp_path):
    cfg = _config(tmp_path, "maxiter", epochs=3, lr_scheduler=dict(type="PolyLR", max_iter=7, power=0.9))
    t = _trainer(cfg)
    t.train()
    path = os.path.join(t.checkpoint_dir, "batch_7.pth")
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"state_dict", "config"}
    assert t.reached_max_iter and t.loss.calls == 7
    assert not os.path.exists(os.path.join(t.checkpoint_dir, "epoch2.pth"))


def test_nan_loss_raises_naming_epoch_and_batch(built, tmp_path):
    t = _trainer(_config(tmp_path, "nan", epochs=3), loss=StubLoss(nan_at=N_BATCHES + 3))
    with pytest.raises(FloatingPointError, match="epoch 2 batch 3"):
        t.train()
    assert "epoch 2 batch 3" in open(os.path.join(t.checkpoint_dir, "train.log")).read()


def test_set_weights_and_sync_free_needs_enqueue(built, tmp_path):
    from orienmask_amd.trainer import Trainer
    donor = _trainer(_config(tmp_path, "donor", epochs=1))
    donor.train()
    path = os.path.join(donor.checkpoint_dir, "epoch1.pth")
    t = _trainer(_config(tmp_path, "weights"), weights=path)
    assert _equal_state(t.model.state_dict(), donor.model.state_dict()) and t.start_epoch == 1
    model, optimizer, scheduler = _parts(_config(tmp_path, "x"))
    with pytest.raises(ValueError, match="enqueue"):
        Trainer(model, StubLoss(), optimizer, scheduler, _config(tmp_path, "refused"), _loader(), None, None, torch.device("cpu"),
                types.SimpleNamespace(resume=None, weights=None), sync_free=True)


def test_text_table_is_right_aligned_with_three_decimals():
    from orienmask_amd.trainer import text_table
    out = text_table(["TRAIN", "S32", "ALL"], [["loss_xy", 1.23456, 10.0], ["loss_sum", 0.5, ""]]).splitlines()
    assert out[1] == "|    TRAIN |   S32 |    ALL |" and out[3] == "|  loss_xy | 1.235 | 10.000 |" and out[4] == "| loss_sum | 0.500 |        |"
    assert out[0] == out[2] == out[5] == "+----------+-------+--------+"


# ---- the sync-free loop on a CPU counter block (DeviceEvalCounter's torch comparator): reads, means and the late stop
class EnqueueLoss:
    """A loss with the real key lists and no __call__: ``enqueue`` feeds seeded result vectors, batch b of an epoch vector b."""

    def __init__(self, bad_at=None, bad_flag=0):
        import loss_counter_cases as cases
        from orienmask_amd.loss import OrienMaskYOLOMultiScaleLoss
        real = OrienMaskYOLOMultiScaleLoss(**cases.loss_kwargs())
        for name in ("loss_id", "metric_id", "num_scales", "scales_weight", "num_classes", "scales_prefix", "loss_suffix",
                     "metric_suffix"):
            setattr(self, name, getattr(real, name))
        self.results = cases.seeded_results(9, steps=N_BATCHES)
        self.calls, self.bad_at, self.bad_flag = 0, bad_at, bad_flag

    def enqueue(self, predict, label, counter, step, training=True):
        r = self.results[self.calls % N_BATCHES].copy()
        self.calls += 1
        if self.calls == self.bad_at and self.bad_flag:
            r[-1:].view("int32")[0] = self.bad_flag           # om_loss's flag word
        elif self.calls == self.bad_at:
            r[0] = float("nan")
        return predict.sum() * 0 + counter.accumulate(torch.from_numpy(r), step, with_metrics=training is not True)


def _sync_free_trainer(config, loss):
    from orienmask_amd.trainer import Trainer

    class Recording(Trainer):
        results = None

        def _log_result(self, result):
            self.results = (self.results or []) + [dict(result)]
            super()._log_result(result)

    model, optimizer, scheduler = _parts(config)
    return Recording(model, loss, optimizer, scheduler, config, _loader(), None, None, torch.device("cpu"),
                     types.SimpleNamespace(resume=None, weights=None))


def test_sync_free_loop_is_the_default_with_enqueue_and_logs_the_means(built, tmp_path):
    loss = EnqueueLoss()
    t = _sync_free_trainer(_config(tmp_path, "free", epochs=2, log_freq=2), loss)
    assert t.sync_free is True
    t.train()
    assert loss.calls == 2 * N_BATCHES and len(t.results) == 2
    for result in t.results:
        assert list(result) == ["train_loss"] + ["train_" + k for k in loss.loss_id]
        # a raw key's epoch mean: the float64 sum of the five result vectors' floats in step order, over 5 items
        total = 0.0
        for r in loss.results:
            total += float(r[0])
        assert result["train_S32_loss_xy"] == total / N_BATCHES
        assert result["train_loss"] == result["train_cross_scale_loss_sum"] > 0


def test_sync_free_stop_comes_at_the_read_and_names_the_latched_batch(built, tmp_path):
    """accumulate 2 and log_freq 2: the counter is read every 4 batches.  The NaN of epoch 2 batch 2 (step 7) stops the run at
    the read of step 8, one batch late -- the documented difference from the reference -- and names epoch 2 batch 2."""
    loss = EnqueueLoss(bad_at=N_BATCHES + 2)
    t = _sync_free_trainer(_config(tmp_path, "late", epochs=3, log_freq=2), loss)
    with pytest.raises(FloatingPointError, match="epoch 2 batch 2") as e:
        t.train()
    assert loss.calls == 8 and "step 7" in str(e.value.__cause__)
    assert "epoch 2 batch 2" in open(os.path.join(t.checkpoint_dir, "train.log")).read()


def test_sync_free_target_error_keeps_its_own_text(built, tmp_path):
    """A latched OM_LOSS_FLAG_BAD_CLASS (4) stops the run as the ValueError the host path raises, with its text, plus the batch."""
    t = _sync_free_trainer(_config(tmp_path, "badcls", epochs=2, log_freq=1), EnqueueLoss(bad_at=3, bad_flag=4))
    with pytest.raises(ValueError, match=r"gt_cls value lies outside \[0, 3\).*step 3.*epoch 1 batch 3") as e:
        t.train()
    assert "nan or inf" not in str(e.value) and t.loss.calls == 4          # read at step 4 (accumulate 2, log_freq 1)
