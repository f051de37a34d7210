"""Train an OrienMask model on the MI355X: the reference's train.py against orienmask_amd.

    python tools/train.py --config CONFIG [--resume CHECKPOINT | --weights WEIGHTS] [--synthetic N] [--frozen-stages K] [--amp bf16]
                          [--conv-forward {torch,hip}] [--conv-grad {torch,hip}] [--max-grad-norm X] [--nonfinite-grads {propagate,skip}]
                          [--ema-decay X] [--no-ema-warmup]

CONFIG is a JSON file -- the ``config.json`` a trainer writes into its checkpoint directory is one -- or, where a ``config``
package with the reference's ``get_config`` is importable, a config name.  ``--synthetic N`` trains on N seeded synthetic images
(tester.SyntheticLossLoader) of the loss's image size instead of config['train_loader'], so the tool runs without a dataset; no
validation then.  ``--frozen-stages K`` (0...6) overrides the model's ``frozen_stages``: backbone.conv1 ... conv{K} are frozen
(orienmask_amd.train), the usual way to fine-tune a pretrained backbone.  ``--amp bf16`` sets the model's ``amp``: bf16 activations
under torch.autocast, float32 parameters, statistics, loss and optimizer (resuming a checkpoint that was trained with another ``amp``
fails the trainer's model-config check, as any other change of the model does).  ``--conv-forward hip`` sets the model's
``conv_forward``: with ``--amp bf16`` every forward convolution is this package's bf16 kernel (csrc/conv_fwd_bf16.hip), frozen
blocks one fused kernel each; without amp it needs the config's ``conv_backend`` to be 'hip'.  ``--conv-grad hip`` sets the model's
``conv_grad``: with ``--amp bf16 --conv-forward hip`` the gradients of those convolutions are this package's bf16 kernels too
(csrc/conv_grad_bf16.hip), and a step repeats bit for bit.  ``--max-grad-norm X`` sets the optimizer's ``max_grad_norm`` (global L2
gradient-norm clipping inside the HIP SGD step, orienmask_amd.optim.SGD) and ``--nonfinite-grads skip`` its ``nonfinite``: a step
whose gradient norm is not finite leaves parameters and momentum buffers untouched, so a diverged run stops with its last finite
weights.  ``--ema-decay X`` sets the optimizer's ``ema_decay``: an exponential moving average of the weights kept inside the same
step kernel, which validation, the monitored value and the checkpoint's ``ema`` entry then use (``--no-ema-warmup`` sets
``ema_warmup`` to False: the decay is X from the first update on).  With several processes (torchrun), each uses the GPU of its LOCAL_RANK.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_config(name):
    if os.path.isfile(name):
        with open(name) as handle:
            return json.load(handle)
    try:
        from config import get_config
    except ImportError:
        raise SystemExit("--config %r is not a file, and no `config` package with get_config is importable" % name)
    return get_config(name)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--config", required=True, help="a config JSON file (or a config name, see above)")
    ap.add_argument("-r", "--resume", default=None, help="checkpoint to resume from")
    ap.add_argument("-w", "--weights", default=None, help="weights to start from (strict=False)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="train on N synthetic images")
    ap.add_argument("--frozen-stages", type=int, default=None, metavar="K",
                    help="freeze backbone.conv1 ... conv{K} (0...6), overriding the config's model.frozen_stages")
    ap.add_argument("--amp", choices=["bf16"], default=None,
                    help="mixed precision: bf16 activations (the model's amp), overriding the config's model.amp")
    ap.add_argument("--conv-forward", choices=["torch", "hip"], default=None,
                    help="whose forward convolution (the model's conv_forward), overriding the config's model.conv_forward")
    ap.add_argument("--conv-grad", choices=["torch", "hip"], default=None,
                    help="whose bf16 convolution gradients under --amp bf16 --conv-forward hip (the model's conv_grad), overriding "
                         "the config's model.conv_grad")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global L2 gradient norm to X inside the optimizer's HIP step (max_grad_norm of SGD, HipAdam, HipAdamW), overriding "
                         "the config's optimizer.max_grad_norm")
    ap.add_argument("--nonfinite-grads", choices=["propagate", "skip"], default=None,
                    help="with --max-grad-norm: what a step does whose gradient norm is not finite (the optimizer's nonfinite), "
                         "overriding the config's optimizer.nonfinite")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="X",
                    help="average the weights inside the optimizer's HIP step with decay X (ema_decay of SGD, HipAdam, HipAdamW), overriding the "
                         "config's optimizer.ema_decay")
    ap.add_argument("--no-ema-warmup", action="store_true",
                    help="with an averaging optimizer: no warm-up of the decay (the optimizer's ema_warmup=False), overriding the "
                         "config's optimizer.ema_warmup")
    args = ap.parse_args(argv)
    assert not (args.resume and args.weights), "--resume and --weights exclude each other"
    return args


def apply_overrides(config, args):
    """The config with the command line's model options in config['model'] and its optimizer options in config['optimizer']; the
    caller's dicts are not mutated."""
    if args.frozen_stages is not None:
        config = dict(config, model=dict(config["model"], frozen_stages=args.frozen_stages))
    if args.amp is not None:
        config = dict(config, model=dict(config["model"], amp=args.amp))
    if args.conv_forward is not None:
        config = dict(config, model=dict(config["model"], conv_forward=args.conv_forward))
    if args.conv_grad is not None:
        config = dict(config, model=dict(config["model"], conv_grad=args.conv_grad))
    if args.max_grad_norm is not None:
        config = dict(config, optimizer=dict(config["optimizer"], max_grad_norm=args.max_grad_norm))
    if args.nonfinite_grads is not None:
        config = dict(config, optimizer=dict(config["optimizer"], nonfinite=args.nonfinite_grads))
    if args.ema_decay is not None:
        config = dict(config, optimizer=dict(config["optimizer"], ema_decay=args.ema_decay))
    if args.no_ema_warmup:
        config = dict(config, optimizer=dict(config["optimizer"], ema_warmup=False))
    return config


def main(argv=None):
    args = parse_args(argv)

    import torch
    from orienmask_amd import builder
    config = apply_overrides(load_config(args.config), args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("training needs an MI355X")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        torch.distributed.init_process_group("nccl")
    train_loader = None
    if args.synthetic:
        from orienmask_amd.tester import SyntheticLossLoader
        loss_cfg = config["loss"]
        size = loss_cfg["image_size"]
        size = (size, size) if isinstance(size, int) else tuple(size)
        batch = config.get("train_loader", {}).get("batch_size", 8)
        train_loader = SyntheticLossLoader(args.synthetic, batch, size=size, seed=config.get("seed", 0),
                                           num_classes=loss_cfg["num_classes"], device=device)
        config = dict(config, val_loader=None)
    trainer = builder.build_trainer(config, args, device, train_loader=train_loader)
    trainer.train()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
