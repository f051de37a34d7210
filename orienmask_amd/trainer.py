"""The reference's training loop (trainer/base.py, trainer/trainer.py) around this package's modules.

  BaseTrainer   the epoch loop, the monitor, ``_save_checkpoint`` (``epoch{N}.pth``, ``best_epoch{N}.pth`` behind the
                ``best_model.pth`` symlink, ``temp.pth``; the reference's dict keys), ``_resume_checkpoint`` with its three config
                assertions, ``_set_weights``; constructor arguments and config keys (``accumulate``, ``epochs``, ``val_freq``,
                ``save_freq``, ``monitor``, ``monitor_mode``, ``log_freq``, ``log_dir``, ``name``, ``n_gpu``) as the reference's
  Trainer       ``_train_epoch`` (step, schedule and ``zero_grad`` every ``accumulate`` batches and at the last batch; the
                ``max_iter`` exit that saves ``batch_<step>.pth``), ``_val_epoch`` (``tester.validate``) and ``_log_result``

Two loops.  ``sync_free=False`` is the reference's, in behaviour: ``loss(predict, label, training=True)`` with any loss callable, a
host EvalCounter, and ``isfinite(loss).item()`` / ``loss.item()`` on every batch -- two stalls of the host per step.  With
``sync_free=True`` (the default when the loss has ``enqueue``) the step holds no device-to-host copy: ``loss.enqueue`` leaves the
values in a ``DeviceEvalCounter`` (om_loss_accumulate, csrc/loss_counter.hip) and the host reads that block every ``writer_freq``
steps and at the end of the epoch.  The ONE deliberate difference in behaviour: the non-finite stop happens at that read, so up to
``log_freq * accumulate`` batches late; the block latches the first bad step, so the error still names the epoch and batch where
it happened (the optimizer has stepped on the bad gradients by then; the run is lost either way, as in the reference -- unless the
optimizer is orienmask_amd.optim.SGD with ``max_grad_norm`` and ``nonfinite="skip"``: its step decides on the device to leave
parameters and momentum buffers untouched when the gradient norm is not finite, so the weights at the stop are the last finite ones,
and the error says so).  With ``max_grad_norm`` set, rank 0 also writes ``train/grad_norm``, ``train/grad_norm_max``,
``train/clipped_steps`` and ``train/skipped_steps`` from ``optimizer.grad_norm_stats()`` at each of those reads; without it the
scalars are unchanged.

Weight EMA.  When the optimizer averages the weights (orienmask_amd.optim.SGD with ``ema_decay``), ``_val_epoch`` runs inside
``optimizer.ema_applied()``: validation, the monitored value and ``best_*`` refer to the AVERAGED weights (the BatchNorm running
statistics are the live ones: they are moving averages already), and the parameters are their own again after it.  Every checkpoint,
``batch_<step>.pth`` included, then has one more key, ``ema = {"state_dict": optimizer.ema_state_dict(model), "updates": n}``, beside
the reference's, which are unchanged, so the reference still resumes from the file; resuming restores shadows and count, and an
averaging run resumed from a file without the key starts its average again from the loaded weights and logs that.  Rank 0 writes
``train/ema_updates`` at the counter's read.  Without ``ema_decay`` files and scalars are what they were.

Other departures from the reference:
  * no ``exit()``: a non-finite loss raises FloatingPointError; reaching ``lr_scheduler.max_iter`` saves ``batch_<step>.pth`` and
    ends ``train()`` (``self.reached_max_iter``);
  * the ranks' counters are merged by an all-gather added in rank order (``DeviceEvalCounter.gather``), their COCO results through
    ``dist.gather_detections``, instead of ``_temp_counter_<rank>.pth`` / ``_temp_coco_eval_<rank>.json`` files; with
    ``sync_free=False`` and several ranks each rank logs its own counter;
  * ``tensorboardX``, ``prettytable`` and ``tqdm`` are optional: scalars go to whichever SummaryWriter imports, else as JSON lines
    to ``scalars.jsonl`` in the checkpoint directory; the tables are plain text; without tqdm there is no progress bar;
  * ``COCOMetrics`` is built only when the config has ``val_gt_file`` and there is a validation loader.
"""
import contextlib
import datetime
import json
import logging
import math
import os
import time

import torch

from .dist import world_info
from .loss import EvalCounter


class _JsonlWriter:
    """``add_scalar`` of a SummaryWriter, as one JSON object per line of <dir>/scalars.jsonl."""

    def __init__(self, logdir):
        self.path = os.path.join(logdir, "scalars.jsonl")

    def add_scalar(self, tag, value, step):
        with open(self.path, "a") as handle:
            handle.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")


def summary_writer(logdir):
    """The first SummaryWriter that imports (tensorboardX, then torch's), else the JSON-lines writer.  Only a failed import
    falls through: an error of an installed writer's constructor (an unwritable `logdir`, say) surfaces."""
    for module in ("tensorboardX", "torch.utils.tensorboard"):
        try:
            writer = __import__(module, fromlist=["SummaryWriter"]).SummaryWriter
        except ImportError:         # ModuleNotFoundError included: not installed, or installed without its own dependencies
            continue
        return writer(logdir)
    return _JsonlWriter(logdir)


def _progress(iterable, total, enabled, **kwargs):
    if enabled:
        try:
            from tqdm import tqdm
            return tqdm(iterable, total=total, **kwargs)
        except ImportError:
            pass
    return iterable


def text_table(field_names, rows):
    """A right-aligned plain-text table; floats with three decimals (the reference's PrettyTable settings)."""
    cells = [[str(c) for c in field_names]] + [["%.3f" % c if isinstance(c, float) else str(c) for c in row] for row in rows]
    widths = [max(len(r[i]) for r in cells) for i in range(len(field_names))]
    rule = "+" + "+".join("-" * (w + 2) for w in widths) + "+"
    lines = [rule]
    for k, row in enumerate(cells):
        lines.append("|" + "|".join(" " + c.rjust(w) + " " for c, w in zip(row, widths)) + "|")
        if k == 0:
            lines.append(rule)
    lines.append(rule)
    return "\n".join(lines)


MONITOR_MODES = ("min", "max", "off")
RESUME_SECTIONS = ("model", "optimizer", "lr_scheduler")       # config entries a checkpoint must share with the run resuming it
BEST_LINK = "best_model.pth"


class BaseTrainer:
    """The epoch loop, the monitor and the checkpoints; a subclass supplies ``_train_epoch(epoch) -> {key: value}``.

    Contract shared with the reference (trainer/base.py), so that either side reads the other's files: a checkpoint is a dict
    with exactly ``epoch``, ``state_dict``, ``optimizer``, ``lr_scheduler``, ``monitor_best`` and ``config``; it is written as
    ``epoch{N}.pth`` every ``save_freq`` epochs, as ``best_epoch{N}.pth`` when the monitored ``val_<monitor>`` improved (the
    relative symlink ``best_model.pth`` then moves to it and the file it pointed to is deleted), and as ``temp.pth`` after an
    epoch without validation.  A run directory ``<log_dir>/<name>_<month day>_<time>`` holds them beside ``config.json`` and
    ``train.log``; resuming continues in the checkpoint's own directory."""

    def __init__(self, model, loss, optimizer, lr_scheduler, config, train_loader, val_loader, device, args):
        self.model, self.loss, self.optimizer, self.lr_scheduler = model, loss, optimizer, lr_scheduler
        self.train_loader, self.val_loader = train_loader, val_loader
        self.config, self.device = config, device
        self.device_rank, self.world_size = world_info()
        self.is_distributed = config["n_gpu"] > 1            # the model is then wrapped (DistributedDataParallel)

        resume, weights = getattr(args, "resume", None), getattr(args, "weights", None)
        self.checkpoint_dir = os.path.dirname(resume) if resume is not None else self._new_run_directory()
        self.logger = self._open_log()

        for key in ("accumulate", "epochs", "val_freq", "save_freq"):
            setattr(self, key, config[key])
        self.writer_freq = config["log_freq"] * self.accumulate          # in batches
        if config["monitor_mode"] not in MONITOR_MODES:
            raise AssertionError("monitor_mode must be one of %s, got %r" % (MONITOR_MODES, config["monitor_mode"]))
        self.monitor, self.monitor_mode = "val_" + config["monitor"], config["monitor_mode"]
        self.monitor_best = math.inf if self.monitor_mode == "min" else -math.inf
        self.start_epoch, self.reached_max_iter = 1, False
        self.tensorboard = summary_writer(self.checkpoint_dir)

        if resume is not None:
            self._resume_checkpoint(resume)
        if weights is not None:
            self._set_weights(weights)

    # ---- the run directory and its log
    def _new_run_directory(self):
        stamp = datetime.datetime.now().strftime("%m%d_%H%M%S")
        path = os.path.join(self.config["log_dir"], "%s_%s" % (self.config["name"], stamp))
        if self.device_rank == 0:
            os.makedirs(path)                                # an existing directory is another run's: fail
            print("Set checkpoint directory: %s" % path)
            with open(os.path.join(path, "config.json"), "w") as handle:
                json.dump(self.config, handle, indent=4)
        if self.world_size > 1:
            torch.distributed.barrier()                      # the other ranks open train.log in it next
        return path

    def _open_log(self):
        """A logger of this run's own, to train.log and the console; ranks other than 0 log errors only.  (logging.basicConfig
        would configure the root logger, once per process.)"""
        logger = logging.getLogger("%s.%s" % (type(self).__name__, self.checkpoint_dir))
        logger.propagate = False
        logger.setLevel(logging.INFO if self.device_rank == 0 else logging.ERROR)
        for old in list(logger.handlers):                    # a run resumed in this process: do not log twice
            logger.removeHandler(old)
            old.close()
        for handler in (logging.FileHandler(os.path.join(self.checkpoint_dir, "train.log")), logging.StreamHandler()):
            handler.setFormatter(logging.Formatter("%(asctime)s %(message)s"))
            logger.addHandler(handler)
        return logger

    def _bare_model(self):
        return self.model.module if self.is_distributed else self.model

    # ---- the epoch loop
    def train(self):
        for epoch in range(self.start_epoch, self.epochs + 1):
            self.logger.info("==== epoch %d of %d ====", epoch, self.epochs)
            began = time.monotonic()
            result = self._train_epoch(epoch)
            self.logger.info("epoch %d done in %s", epoch, datetime.timedelta(seconds=round(time.monotonic() - began)))
            if self.reached_max_iter:
                break
            if self.device_rank != 0:
                continue
            self._log_result(result)
            if epoch % self.val_freq == 0:
                self._save_checkpoint(epoch, save_best=self._improved(result))
            else:
                self._save_checkpoint(epoch, temp=True)

    def _improved(self, result):
        """Whether the monitored value beats the best so far (and then becomes it); never with monitor_mode 'off'."""
        if self.monitor_mode == "off":
            return False
        if self.monitor not in result:
            raise AssertionError("the monitored item %r is not in the epoch's result" % self.monitor)
        value = result[self.monitor]
        better = value < self.monitor_best if self.monitor_mode == "min" else value > self.monitor_best
        if better:
            self.logger.info("%s improved: %f -> %f", self.monitor, self.monitor_best, value)
            self.monitor_best = value
        else:
            self.logger.info("%s did not improve on %f", self.monitor, self.monitor_best)
        return better

    def _train_epoch(self, epoch):
        raise NotImplementedError

    def _log_result(self, result):
        for key, value in result.items():
            self.logger.info("%s: %s", key, value)

    # ---- checkpoints
    def _averaging(self):
        """The optimizer keeps an EMA of the weights in its step (orienmask_amd.optim.SGD with ema_decay)."""
        return getattr(self.optimizer, "ema_decay", None) is not None and hasattr(self.optimizer, "ema_applied")

    def _ema_entry(self, model):
        """{"ema": ...} of a checkpoint whose state_dict is `model`'s; nothing without averaging: the file is then today's."""
        if not self._averaging():
            return {}
        return dict(ema=dict(state_dict=self.optimizer.ema_state_dict(model), updates=self.optimizer.ema_updates()))

    def _checkpoint_state(self, epoch):
        return dict(epoch=epoch, state_dict=self._bare_model().state_dict(), optimizer=self.optimizer.state_dict(),
                    lr_scheduler=self.lr_scheduler.state_dict(), monitor_best=self.monitor_best, config=self.config,
                    **self._ema_entry(self._bare_model()))

    def _save_checkpoint(self, epoch, save_best=False, temp=False):
        names = []
        if epoch % self.save_freq == 0:
            names.append("epoch%d.pth" % epoch)
        if save_best:
            names.append("best_epoch%d.pth" % epoch)
        if temp:
            names.append("temp.pth")
        if not names:
            return
        state = self._checkpoint_state(epoch)
        for name in names:
            torch.save(state, os.path.join(self.checkpoint_dir, name))
            self.logger.info("wrote checkpoint %s", os.path.join(self.checkpoint_dir, name))
        if save_best:
            self._move_best_link("best_epoch%d.pth" % epoch)

    def _move_best_link(self, name):
        """Point best_model.pth (a relative symlink) at `name` and delete the checkpoint it pointed to before."""
        link = os.path.join(self.checkpoint_dir, BEST_LINK)
        if os.path.islink(link):
            previous = os.readlink(link)
            os.remove(link)
            if previous != name:
                os.remove(os.path.join(self.checkpoint_dir, previous))
        os.symlink(name, link)

    def _resume_checkpoint(self, path):
        """Continue after the checkpoint's epoch.  Its run must have had this run's model, optimizer and lr_scheduler config."""
        checkpoint = torch.load(path, map_location=self.device, weights_only=False)
        for section in RESUME_SECTIONS:
            if checkpoint["config"][section] != self.config[section]:
                raise AssertionError("config[%r] differs from the checkpoint's: %r here, %r in %s"
                                     % (section, self.config[section], checkpoint["config"][section], path))
        self._bare_model().load_state_dict(checkpoint["state_dict"], strict=True)
        self.optimizer.load_state_dict(checkpoint["optimizer"])
        self.lr_scheduler.load_state_dict(checkpoint["lr_scheduler"])
        if self._averaging():
            if "ema" in checkpoint:
                self.optimizer.load_ema_state_dict(self._bare_model(), checkpoint["ema"]["state_dict"], checkpoint["ema"]["updates"])
                self.logger.info("restored the averaged weights after %d updates", checkpoint["ema"]["updates"])
            else:
                self.optimizer.ema_reset()
                self.logger.info("%s holds no averaged weights: the average starts again from the loaded weights", path)
        self.monitor_best = checkpoint["monitor_best"]
        self.start_epoch = checkpoint["epoch"] + 1
        self.logger.info("resumed from %s: epoch %d is next", path, self.start_epoch)

    def _set_weights(self, path):
        """Start from the weights of a checkpoint or a bare state_dict; keys that do not match are reported, not refused."""
        loaded = torch.load(path, map_location=self.device, weights_only=False)
        report = self._bare_model().load_state_dict(loaded.get("state_dict", loaded), strict=False)
        self.logger.info("weights from %s: %s", path, report)


class Trainer(BaseTrainer):
    """The training and validation epochs (the reference's trainer/trainer.py in behaviour).  `sync_free`: None (default) = True
    when the loss has ``enqueue``; see the module docstring.  `coco_metrics`: a cocoeval.COCOMetrics to use instead of the one
    built from config['val_gt_file']."""

    def __init__(self, model, loss, optimizer, lr_scheduler, config, train_loader, val_loader, postprocess, device, args,
                 sync_free=None, coco_metrics=None):
        super().__init__(model, loss, optimizer, lr_scheduler, config, train_loader, val_loader, device, args)
        self.postprocess = postprocess
        self.sync_free = hasattr(loss, "enqueue") if sync_free is None else bool(sync_free)
        if self.sync_free and not hasattr(loss, "enqueue"):
            raise ValueError("sync_free=True needs a loss with enqueue(predict, target, counter, step, training); %r has none"
                             % type(loss).__name__)
        if coco_metrics is None and val_loader is not None and config.get("val_gt_file"):
            from .cocoeval import COCOMetrics
            dataset = val_loader.dataset
            coco_metrics = COCOMetrics(gt_file=config["val_gt_file"], cat2label=dataset.CAT2LABEL, with_mask=dataset.with_mask,
                                       save_dir=self.checkpoint_dir, device=device)
        self.coco_metrics = coco_metrics
        self._counter = None

    # ---- one training epoch
    def _train_epoch(self, epoch):
        """Batches are numbered from 1 within the epoch and, as `step`, from 1 over the run.  The optimizer, the schedule and
        zero_grad run after every `accumulate`-th batch and after the last; the counter is read and its means written every
        `writer_freq` steps; at step lr_scheduler.max_iter (where the schedule has one) the weights go to batch_<step>.pth and
        training ends."""
        self.model.train()
        sampler = getattr(self.train_loader, "sampler", None)
        if self.world_size > 1 and hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        counter = self._train_counter()
        n_batches = len(self.train_loader)
        keys = ["loss"] + list(self.loss.loss_id)
        max_iter = getattr(self.lr_scheduler, "max_iter", None)
        bar = _progress(enumerate(self.train_loader, 1), n_batches, self.device_rank == 0, postfix=dict(lr="-", loss="-"))

        for batch, sample in bar:
            step = (epoch - 1) * n_batches + batch
            image = sample[0].to(self.device)
            target = [t.to(self.device) for t in sample[1]]
            if self.sync_free:
                self.loss.enqueue(self.model(image), target, counter, step, training=True).backward()
            else:
                value, loss_log, _ = self.loss(self.model(image), target, training=True)
                value.backward()
            if batch % self.accumulate == 0 or batch == n_batches:
                self.optimizer.step()
                self.lr_scheduler.step()
                self.optimizer.zero_grad()
            if not self.sync_free:
                # the reference's per-batch bookkeeping: two reads of the device scalar
                if not torch.isfinite(value).item():
                    self._stop(epoch, batch, loss_log)
                counter.update("loss", value.item())
                for key, v in loss_log.items():
                    counter.update(key, v)
            if step % self.writer_freq == 0:
                means = self._read(counter, "averages", keys, n_batches)
                if self.device_rank == 0:
                    self._write_train_scalars(means, step // self.accumulate, bar)
                counter.reset()
            if step == max_iter:
                if self.sync_free:
                    self._checked(counter.check, n_batches)
                self._save_at_max_iter(step)
                return {}

        means = self._read(counter, "averages_epoch", keys, n_batches)
        counter.reset_epoch()
        train_log = {}
        if self.device_rank == 0:
            train_log["train_loss"] = means["loss"]
            train_log.update(("train_" + key, means[key]) for key in self.loss.loss_id)
        if self.val_loader is not None and epoch % self.val_freq == 0:
            train_log.update(self._val_epoch(epoch))
        return train_log

    def _train_counter(self):
        if not self.sync_free:
            return EvalCounter()
        if self._counter is None:
            from .loss import DeviceEvalCounter
            self._counter = DeviceEvalCounter(self.loss, self.device)
        return self._counter

    def _read(self, counter, what, keys, n_batches):
        """{key: mean} of the stage (`what` = 'averages') or of the epoch ('averages_epoch').  In the sync-free loop this is the
        read of the device block, after the ranks' blocks were merged; the host counter answers key by key, for its own rank."""
        if not self.sync_free:
            one = counter.average if what == "averages" else counter.average_epoch
            return {key: one(key) for key in keys}
        if self.world_size > 1:
            counter.gather()
        return self._checked(lambda: getattr(counter, what)(keys), n_batches)

    def _write_train_scalars(self, means, at, bar):
        """lr/group<i> (as configured, before the division by accumulate), train/loss and train/<loss key> at optimizer step `at`."""
        groups = self.optimizer.param_groups
        for i, group in enumerate(groups):
            self.tensorboard.add_scalar("lr/group%d" % i, group["lr"] * self.accumulate, at)
        for key, value in means.items():
            self.tensorboard.add_scalar("train/%s" % key, value, at)
        if self._clipping():
            # one small read of the optimizer's device block, at the counter's read: the norms of the steps since the last one
            stats = self.optimizer.grad_norm_stats()
            skipped = stats["nonfinite_steps"] if self.optimizer.nonfinite == "skip" else 0
            for tag, value in (("grad_norm", stats["mean_norm"]), ("grad_norm_max", stats["max_norm"]),
                               ("clipped_steps", stats["clipped_steps"]), ("skipped_steps", skipped)):
                self.tensorboard.add_scalar("train/%s" % tag, value, at)
        if self._averaging():
            self.tensorboard.add_scalar("train/ema_updates", self.optimizer.ema_updates(), at)
        if hasattr(bar, "set_postfix"):
            bar.set_postfix(lr="%.2e" % (groups[0]["lr"] * self.accumulate), loss="%.4f" % means["loss"])

    def _clipping(self):
        """The optimizer clips the gradient norm in its step (orienmask_amd.optim.SGD with max_grad_norm)."""
        return getattr(self.optimizer, "max_grad_norm", None) is not None and hasattr(self.optimizer, "grad_norm_stats")

    def _save_at_max_iter(self, step):
        if self.device_rank == 0:
            path = os.path.join(self.checkpoint_dir, "batch_%d.pth" % step)
            torch.save(dict(state_dict=self.model.state_dict(), config=self.config, **self._ema_entry(self.model)), path)
            self.logger.info("max_iter reached: wrote %s", path)
        if self.world_size > 1:
            torch.distributed.barrier()
        self.reached_max_iter = True

    def _checked(self, read, n_batches):
        """A read of the device counter; its latched error becomes the loop's stop, with the epoch and batch of the latched step."""
        try:
            return read()
        except (FloatingPointError, ValueError) as e:
            step = self._counter.first_bad_step
            if step is None:
                raise
            self._stop((step - 1) // n_batches + 1, (step - 1) % n_batches + 1, {}, cause=e)

    def _stop(self, epoch, batch, loss_log, cause=None):
        """End the run: FloatingPointError for a non-finite loss or pred_wh; for the latched target errors (too many GTs, a bad
        class) a ValueError that carries the cause's own text.  Either names the epoch and batch; loss_log goes to the log."""
        where = "training stops at epoch %d batch %d" % (epoch, batch)
        if isinstance(cause, ValueError):
            error = ValueError("%s; %s" % (cause, where))
        else:
            kept = ""
            if self._clipping() and self.optimizer.nonfinite == "skip":
                first = self.optimizer.grad_norm_stats(reset=False)["first_nonfinite_step"]
                kept = ("; the optimizer skipped every step with a non-finite gradient norm (first at its step %d), so the "
                        "parameters were left at their last finite state" % first)
            error = FloatingPointError("non-finite loss%s; %s%s" % (" (%s)" % cause if cause is not None else "", where, kept))
        self.logger.error(str(error))
        if self.device_rank == 0:
            for key, value in loss_log.items():
                self.logger.error("%s: %s", key, value)
        raise error from cause

    # ---- validation
    def _val_epoch(self, epoch):
        from .tester import validate
        self.logger.info("validation after epoch %d", epoch)
        self.model.eval()
        counter = None
        if self.sync_free:
            from .loss import DeviceEvalCounter
            counter = DeviceEvalCounter(self.loss, self.device)
        # an averaging optimizer's weights are validated: the shadows are swapped in for the pass and out again after it
        with self.optimizer.ema_applied() if self._averaging() else contextlib.nullcontext():
            val_log = validate(self.model, self.loss, self.postprocess, self.val_loader, self.coco_metrics, counter=counter)
        if self.device_rank != 0:
            return {}
        for key, value in val_log.items():
            self.tensorboard.add_scalar("val/%s" % key[len("val_"):], value, epoch)
        return val_log

    # ---- the epoch's tables
    def _rows(self, result, prefix, suffixes):
        scales = list(self.loss.scales_prefix)
        return [[sid] + [result["%s_%s_%s" % (prefix, scale, sid)] for scale in scales + ["cross_scale"]] for sid in suffixes]

    def _log_result(self, result):
        scales = list(self.loss.scales_prefix)
        self.logger.info("\n" + text_table(["TRAIN"] + scales + ["ALL"], self._rows(result, "train", self.loss.loss_suffix)))
        if "val_{0}_{1}".format(scales[0], self.loss.loss_suffix[0]) not in result:
            return
        names = ["VAL"] + scales + ["ALL"]
        rows = self._rows(result, "val", self.loss.loss_suffix)
        if "val_{0}_{1}".format(scales[0], self.loss.metric_suffix[0]) in result:
            rows += self._rows(result, "val", self.loss.metric_suffix)
        cm = self.coco_metrics
        if cm is not None and "val_bbox_" + cm.metric_keys[0] in result:
            # the loss / metric rows and the COCO statistics side by side, as the reference's one table
            rows += [[""] * len(names) for _ in range(max(len(cm.metric_keys) - len(rows), 0))]
            extra = [""] * max(len(rows) - len(cm.metric_keys), 0)
            columns = [("", list(cm.metric_keys) + extra), ("BBOX", [result["val_bbox_" + k] for k in cm.metric_keys] + extra)]
            if cm.with_mask:
                columns.append(("SEGM", [result["val_segm_" + k] for k in cm.metric_keys] + extra))
            for name, column in columns:
                names = names + [name]
                rows = [row + [cell] for row, cell in zip(rows, column)]
        self.logger.info("\n" + text_table(names, rows))
        if cm is not None and len(cm.bbox_eval_stats):
            self.logger.info("BBOX " + " ".join("%.3f" % k for k in cm.bbox_eval_stats))
            if cm.with_mask:
                self.logger.info("SEGM " + " ".join("%.3f" % k for k in cm.segm_eval_stats))
