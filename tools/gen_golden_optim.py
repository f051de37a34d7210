"""Generate the optimizer fixtures under tests/golden/ (tests/test_optim_cpu.py, tests/test_optim.py):

  optim_sgd_<set>.npz      what torch.optim.SGD on CPU float32 tensors (the optimizer the reference builds, trainer/builder.py:118-130)
                           produced from tests/optim_np.py's seeded inputs, per step: p0, grads [steps, n], param [steps, n],
                           buf [steps, n] (absent without momentum), and the hyper-parameters.  One file per set of
                           optim_np.HYPER_SETS plus optim_sgd_specials.npz (zeros, denormals, +-Inf, NaN; momentum_decay's set).
                           A host whose torch rounds otherwise shows up as a disagreement between the live torch run and these.
  optim_lr_schedules.npz   the learning rates the REFERENCE's own optim/lr_scheduler.py produces: StepWarmUpLR with all three
                           warm-up types across the warm-up boundary and both milestones, and PolyLR (optim_np's cases).
  optim_param_groups.npz   (name, lr, weight_decay) of the REFERENCE's optim/param_groups.py on optim_np.groups_module().

Runs only where the reference exists (/root/reference, as tools/gen_golden.py).

    python tools/gen_golden_optim.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optim_np as N  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20


def import_reference_optim():
    sys.path.insert(0, "/root/reference")
    import optim as ref_optim
    return ref_optim


def sgd_fixture(path, p0, grads, hyper):
    runs = N.torch_cpu_run(p0, grads, hyper, foreach=False)
    again = N.torch_cpu_run(p0, grads, hyper, foreach=True)
    for (p, b), (p2, b2) in zip(runs, again):
        assert N.same_bits(p, p2) and (b is None or N.same_bits(b, b2)), "torch's two CPU paths disagree on this host"
    arrays = dict(p0=np.asarray(p0, np.float32), grads=np.stack(grads), param=np.stack([p for p, _ in runs]),
                  hyper=np.frombuffer(json.dumps(hyper, sort_keys=True).encode(), dtype=np.uint8))
    if runs[0][1] is not None:
        arrays["buf"] = np.stack([b for _, b in runs])
    np.savez_compressed(path, **arrays)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(1)
    for i, (name, hyper) in enumerate(N.HYPER_SETS.items()):
        p0, grads = N.seeded_inputs(SEED + i)
        sgd_fixture(os.path.join(OUT, "optim_sgd_%s.npz" % name), p0, grads, hyper)
    p0, grads = N.special_inputs()
    sgd_fixture(os.path.join(OUT, "optim_sgd_specials.npz"), p0, grads, N.HYPER_SETS["momentum_decay"])

    ref = import_reference_optim()
    seqs = {}
    for name, case in N.STEP_WARMUP_CASES.items():
        seqs["step_" + name] = N.lr_sequence(lambda opt, c=case: ref.StepWarmUpLR(optimizer=opt, **c), N.STEP_WARMUP_ITERS)
    seqs["poly"] = N.lr_sequence(lambda opt: ref.PolyLR(opt, **N.POLY_CASE), N.POLY_ITERS)
    path = os.path.join(OUT, "optim_lr_schedules.npz")
    np.savez_compressed(path, **seqs)
    print(os.path.basename(path), os.path.getsize(path), "bytes")

    model = N.groups_module()
    listing = N.groups_listing(model, ref.param_groups(model, **N.GROUPS_KWARGS))
    path = os.path.join(OUT, "optim_param_groups.npz")
    np.savez_compressed(path, names=np.array([n for n, _, _ in listing]), lr=np.array([l for _, l, _ in listing], np.float64),
                        weight_decay=np.array([w for _, _, w in listing], np.float64))
    print(os.path.basename(path), os.path.getsize(path), "bytes")
    for row in listing:
        print("  %-14s lr %-8g weight_decay %g" % row)


if __name__ == "__main__":
    main()
