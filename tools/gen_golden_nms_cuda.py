"""Record tests/golden/nms_cuda_ref.npz: the case sets of tests/nms_cases.py and the keep lists of the reference's own CUDA NMS
(eval/src/nms_cuda.cpp + nms_kernel.cu, built for gfx950 by oracle/build_ref_cuda.py into oracle/_ref/) in both builds.

Runs on an MI355X with oracle/_ref/ built.  Per case: name, family, threshold, classes, the "exact" keep list (every operation
rounded once) and the "fused" one (hipcc's default contraction); dets are stored up to nms_cases.STORED_MAX_N boxes, larger sets
are rebuilt from their seed (nms_cases.blocks_family) and pinned by a float64 checksum.  Prints, per family, the number of
cases and boxes, where the fused build differs, and how the reference module ordered the score ties.

    python tools/gen_golden_nms_cuda.py [out.npz]           # default tests/golden/nms_cuda_ref.npz
"""
import os
import sys
from collections import Counter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nms_cases as N  # noqa: E402
from oracle import orienmask_ref as R  # noqa: E402


def main(out):
    assert torch.cuda.is_available(), "needs the GPU the reference module runs on"
    cases = N.cases()
    rec = {"names": np.array([c["name"] for c in cases]), "families": np.array([c["family"] for c in cases])}
    boxes, diff_cases, diff_boxes = Counter(), Counter(), Counter()
    for c in cases:
        d = torch.from_numpy(c["dets"])
        exact = R.nms_cuda_reference(d, float(c["thr"]), "exact").numpy()
        fused = R.nms_cuda_reference(d, float(c["thr"]), "fused").numpy()
        again = R.nms_cuda_reference(d, float(c["thr"]), "exact").numpy()
        key = c["name"]
        if not np.array_equal(exact, again):                # torch's GPU sort may order score ties differently per run
            print("UNSTABLE: two runs of the exact module differ on %s" % key)
            rec[key + "_unstable"] = np.array(1, np.int8)
        n = c["dets"].shape[0]
        if n <= N.STORED_MAX_N:
            rec[key + "_dets"] = c["dets"]
        rec[key + "_checksum"] = np.array([c["dets"].astype(np.float64).sum()])
        rec[key + "_cats"] = c["cats"].astype(np.int8)
        rec[key + "_thr"] = np.array(c["thr"], np.float32)
        rec[key + "_keep"] = exact.astype(np.int16 if n < 32768 else np.int32)
        rec[key + "_keep_fused"] = fused.astype(np.int16 if n < 32768 else np.int32)
        boxes[c["family"]] += n
        if not np.array_equal(exact, fused):
            diff_cases[c["family"]] += 1
            diff_boxes[c["family"]] += len(set(exact.tolist()) ^ set(fused.tolist()))
        if c["family"] == "ties":
            # the visiting order the reference's own sort call (nms_kernel.cu:76) gives these scores on the GPU
            rec[key + "_order"] = torch.sort(d[:, 4].cuda(), 0, descending=True)[1].cpu().numpy().astype(np.int16)
            print("ties %s: reference keep list %s the stable (ascending index) order's, %s between runs" %
                  (c["name"], "==" if exact.tolist() == c["keep"].tolist() else "!=",
                   "same" if np.array_equal(exact, again) else "DIFFERENT"))
        elif exact.tolist() != c["keep"].tolist():
            print("MISMATCH case emulation vs exact module: %s" % c["name"])
        rs = R.nms_cuda(d, float(c["thr"])).tolist()
        if rs != exact.tolist():
            print("MISMATCH restatement vs exact module: %s" % c["name"])
    for fam in N.FAMILIES:
        k = [c for c in cases if c["family"] == fam]
        print("%-12s %3d cases %6d boxes; fused != exact in %d cases, %d boxes" %
              (fam, len(k), boxes[fam], diff_cases[fam], diff_boxes[fam]))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "nms_cuda_ref.npz"))
