"""Generate tests/golden/cocoeval_display.npz by running the REAL reference's COCOMetrics._get_per_cats_stats
(eval/coco_eval.py:207-217) and Tester.display_coco_eval (trainer/tester.py:64-96).

pycocotools is not available, so it is stubbed, and the evaluation object the reference reads is a stand-in carrying a
seeded `precision` array [T, 11, K=80, A, M] with -1 entries (whole categories undefined as well as scattered ones).
The reference modules are loaded from their files without executing the packages' __init__ (which would pull in the
native NMS extensions); utils.timer needs prettytable, stubbed too.  Never writes bytecode into the reference tree.

    python tools/gen_golden_cocoeval.py [reference root]       # writes tests/golden/cocoeval_display.npz
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

sys.dont_write_bytecode = True

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "cocoeval_display.npz")

import numpy as np  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference(root):
    for name in ("pycocotools", "pycocotools.mask", "pycocotools.coco", "pycocotools.cocoeval", "prettytable"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["pycocotools.cocoeval"].COCOeval = object
    sys.modules["prettytable"].PrettyTable = object
    for pkg in ("eval", "utils", "trainer"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(root, pkg)]
        sys.modules[pkg] = m
    coco_eval = _load("eval.coco_eval", os.path.join(root, "eval", "coco_eval.py"))
    _load("utils.timer", os.path.join(root, "utils", "timer.py"))
    sys.modules["utils"].timer = sys.modules["utils.timer"]
    tester = _load("trainer.tester", os.path.join(root, "trainer", "tester.py"))
    return coco_eval, tester


def seeded_precision(seed):
    rng = np.random.default_rng(seed)
    # [T, 11 recall samples, 80, A, M] on a coarse value grid: _get_per_cats_stats only needs the category axis at full size,
    # and the fixture stays ~0.2 MB
    p = rng.integers(0, 97, (10, 11, 80, 4, 3)) / 96.0
    p[rng.random(p.shape) < 0.15] = -1
    p[:, :, [7, 33, 61], :, :] = -1          # categories without any GT: nan in the per-category table
    return p


def main(root):
    coco_eval, tester = import_reference(root)
    sys.path.insert(0, REPO)
    from orienmask_amd.visualizer import CAT2LABEL, CLASSES
    metrics = coco_eval.COCOMetrics.__new__(coco_eval.COCOMetrics)
    import torch
    metrics.cat2label = torch.tensor(list(CAT2LABEL["COCO"]))
    metrics.with_mask = True
    out = {}
    for kind, seed in (("bbox", 1), ("segm", 2)):
        prec = seeded_precision(seed)
        per = metrics._get_per_cats_stats(types.SimpleNamespace(eval={"precision": prec}))
        stats = np.random.default_rng(10 + seed).random(12)
        stats[[3, 9]] = -1
        setattr(metrics, kind + "_eval_stats", stats)
        setattr(metrics, kind + "_eval_per_cats_stats", per)
        out[kind + "_precision"] = prec
        out[kind + "_per_cats"] = np.array(per, dtype=np.float64)
        out[kind + "_stats"] = stats
    t = tester.Tester.__new__(tester.Tester)
    t.coco_metrics = metrics
    t.test_loader = types.SimpleNamespace(dataset=types.SimpleNamespace(CLASSES=list(CLASSES["COCO"])))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        t.display_coco_eval(eval_type="bbox")
        t.display_coco_eval(eval_type="segm")
    out["text"] = np.array(buf.getvalue())
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
