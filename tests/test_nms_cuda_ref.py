"""GPU: the CUDA NMS backend pinned against the reference's own eval/src/nms_kernel.cu.

oracle/build_ref_cuda.py builds the reference's nms_cuda.cpp + nms_kernel.cu for gfx950 into oracle/_ref/ twice:
nms_cuda_ref_exact (-ffp-contract=off, every operation rounded once, as the source states) and nms_cuda_ref_fused (hipcc's
default contraction).  R.nms_cuda_reference runs either on cuda:0.  The case sets are tests/nms_cases.py.  Every family is
checked against the exact module through om_nms_ex (eval.nms, backend "cuda"), batched_nms, the C restatement
(oracle/nms_cuda_ref.c) and the fused postprocess; the tie family separately.  The teeth: the fused module differs from the exact
one on the contraction family, and three mutants of the restatement each disagree with the exact module somewhere.
"""
import os

import numpy as np
import pytest
import torch

import nms_cases as N
from conftest import GOLDEN, golden_files, post_cfg
from oracle import orienmask_ref as R
from orienmask_amd import synth

pytestmark = pytest.mark.gpu

ORDERED = tuple(f for f in N.FAMILIES if f != "ties")       # families whose scores are distinct
_KEEP = {}


@pytest.fixture(scope="module")
def dev(built):
    from orienmask_amd import lib as omlib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _ref(c, variant="exact"):
    key = (c["name"], variant)
    if key not in _KEEP:
        _KEEP[key] = R.nms_cuda_reference(torch.from_numpy(c["dets"]), float(c["thr"]), variant).numpy()
    return _KEEP[key]


@pytest.fixture
def exact_backend(monkeypatch):
    """R.batched_nms / R.PostProcessOracle with the reference's own CUDA NMS (exact build) in place of the C restatement."""
    monkeypatch.setattr(R, "nms_cuda", lambda dets, thr: R.nms_cuda_reference(dets, thr, "exact"))


@pytest.mark.parametrize("family", ORDERED)
def test_case_sets_are_what_the_reference_module_computes(dev, family):
    """The case sets' float32 restatement of devIoU (nms_cases.nms_exact) gives the exact module's keep list, in its order."""
    for c in N.cases((family,)):
        assert _ref(c).tolist() == c["keep"].tolist(), c["name"]


@pytest.mark.parametrize("family", ORDERED)
def test_om_nms_ex_matches_reference_module(dev, family):
    """eval.nms(backend="cuda") and om_nms_ex(semantics=1) return exactly the reference module's keep list, same order."""
    from orienmask_amd.eval import _nms_keep, nms
    for c in N.cases((family,)):
        want = _ref(c).tolist()
        d = torch.from_numpy(c["dets"]).to(dev)
        cats = torch.from_numpy(c["cats"]).to(dev)
        kd, kc, keep = nms(d, cats, float(c["thr"]), backend="cuda")
        assert keep.cpu().tolist() == want, c["name"]
        assert np.array_equal(kd.cpu().numpy(), c["dets"][want], equal_nan=True), c["name"]
        assert _nms_keep(d, float(c["thr"]), "cuda").cpu().tolist() == want, c["name"]


@pytest.mark.parametrize("family", ORDERED)
def test_restatement_matches_reference_module(dev, family):
    """oracle/nms_cuda_ref.c (R.nms_cuda) equals the reference module."""
    for c in N.cases((family,)):
        assert R.nms_cuda(torch.from_numpy(c["dets"]), float(c["thr"])).tolist() == _ref(c).tolist(), c["name"]


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("family", ORDERED)
def test_batched_nms_matches_reference_module(dev, exact_backend, family, normalized):
    """batched_nms(backend="cuda") equals the reference's batched_nms (function.py:77-103) on its own CUDA NMS, 1-3 classes."""
    from orienmask_amd.eval import batched_nms
    for c in N.cases((family,)):
        d, cats = torch.from_numpy(c["dets"]), torch.from_numpy(c["cats"])
        _, _, want = R.batched_nms(d, cats, float(c["thr"]), normalized, backend="cuda")
        kd, kc, got = batched_nms(d.to(dev), cats.to(dev), float(c["thr"]), normalized, backend="cuda")
        assert got.cpu().tolist() == want.tolist(), (c["name"], normalized)
        assert torch.equal(kc.cpu(), cats[want]), (c["name"], normalized)


def test_ties_follow_the_reference_module(dev):
    """Score ties.  The reference visits boxes in the order of torch's GPU sort (nms_kernel.cu:76, stable=False), which leaves
    ties unspecified; om_nms_ex and the C restatement visit ties in ascending index order.  Observed on the MI355X: from
    64 boxes up torch's sort is stable and the reference module's keep list is the stable order's, so om_nms_ex must give
    exactly that list; at 8 boxes (torch sorts up to 32 elements with an unstable bitonic network) the module is repeatable but
    visits ties in another order.  In every case the module's list is greedy NMS over the order torch's sort returns for the
    same scores, i.e. the tie order is the only difference."""
    from orienmask_amd.eval import _nms_keep
    for c in N.cases(("ties",)):
        d = torch.from_numpy(c["dets"])
        thr = float(c["thr"])
        first = R.nms_cuda_reference(d, thr).tolist()
        second = R.nms_cuda_reference(d, thr).tolist()
        stable = c["keep"].tolist()
        print("%s: reference keep list %s between runs, %s the stable order's" %
              (c["name"], "same" if first == second else "DIFFERENT", "==" if first == stable else "!="))
        torch_order = torch.sort(d[:, 4].to(dev), 0, descending=True)[1].cpu().numpy()
        if first == second:
            assert first == N.nms_exact(c["dets"], c["thr"], order=torch_order).tolist(), c["name"]
        if c["dets"].shape[0] > 32:
            assert first == second == stable, c["name"]
        assert _nms_keep(d.to(dev), thr, "cuda").cpu().tolist() == stable, c["name"]
        assert R.nms_cuda(d, thr).tolist() == stable, c["name"]


def test_fused_module_differs_on_contraction_family(dev):
    """The contraction family sits on single roundings: hipcc's default contraction (the fused build) changes the keep list
    on at least one of its cases, and on every one it gives what nms_cases.iou_fused predicts."""
    differ = 0
    for c in N.cases(("contraction",)):
        fused = _ref(c, "fused")
        differ += int(fused.tolist() != _ref(c).tolist())
        assert fused.tolist() == N.nms_exact(c["dets"], c["thr"], iou=N.iou_fused).tolist(), c["name"]
    assert differ >= 1
    print("fused != exact on %d of %d contraction cases" % (differ, len(N.cases(("contraction",)))))


@pytest.mark.parametrize("mutant", ["ge", "corner_area", "ascending"])
def test_mutants_of_the_restatement_are_caught(dev, mutant):
    """Each of three wrong readings of nms_kernel.cu disagrees with the exact module somewhere on the case sets: >= for >,
    corner areas (x2 - x1) * (y2 - y1) for w * h, the keep list in ascending index order."""
    kw = {"ge": dict(ge=True), "corner_area": dict(iou=N.iou_corner_area), "ascending": dict(ascending=True)}[mutant]
    caught = [c["name"] for c in N.cases(ORDERED) if c["dets"].shape[0] <= 1024
              and N.nms_exact(c["dets"], c["thr"], **kw).tolist() != _ref(c).tolist()]
    assert caught, mutant
    if mutant == "ge":
        assert any(n.startswith("thr") for n in caught)


# ---- the fused postprocess with nms_backend="cuda" against the reference's postprocess on its own CUDA NMS
_SOURCES = [("fixture", f) for f in golden_files("post_")] + \
    [("regime", r) for r in (("mixed", 201), ("sparse_many", 202), ("clustered", 203), ("ties_iou", 204))]


def _heads(kind, src):
    if kind == "fixture":
        g = np.load(os.path.join(GOLDEN, src))
        size = tuple(int(v) for v in g["size"])
        return size, synth.synth_heads(int(g["seed"]), int(g["batch"]), post_cfg(size)["grid_size"], regime=str(g["regime"]))
    regime, seed = src
    size = (544, 544) if regime == "ties_iou" else (160, 192)
    return size, synth.synth_heads(seed, 2, post_cfg(size)["grid_size"], regime=regime)


@pytest.mark.parametrize("kind,src", _SOURCES, ids=[s if k == "fixture" else s[0] for k, s in _SOURCES])
def test_postprocess_keep_matches_reference_module(dev, exact_backend, kind, src):
    """OrienMaskYOLOPostProcess(nms_backend="cuda"): post.last_keep equals the keep indices of the reference's postprocess
    (R.PostProcessOracle, postprocess.py:146-154) on the reference's own CUDA NMS, for nms_pre 400 / 700 / 1024 and both
    batched_nms normalisations."""
    import functools
    from orienmask_amd.eval import OrienMaskYOLOPostProcess, batched_nms
    size, heads = _heads(kind, src)
    pc = post_cfg(size)
    dheads = tuple((b.to(dev), o.to(dev)) for b, o in heads)
    for nms_pre in (400, 700, 1024):
        oracle = R.PostProcessOracle(pc["grid_size"], pc["image_size"], pc["anchors"], pc["anchor_mask"], 80,
                                     conf_thresh=pc["conf_thresh"], nms_pre=nms_pre, nms_backend="cuda")
        cand = [oracle.candidates(heads, b) for b in range(heads[0][0].shape[0])]
        for normalized in (True, False):
            cfg = dict(pc, nms_pre=nms_pre)
            post = OrienMaskYOLOPostProcess(device=dev, **dict(cfg, nms_func=functools.partial(
                batched_nms, threshold=0.5, normalized=normalized, backend="cuda")))
            assert post.nms_backend == "cuda"
            post(dheads)
            for b, (coord, score, cls, _, _) in enumerate(cand):
                dets = torch.cat([coord, score.unsqueeze(-1)], 1)
                kd, _, keep = R.batched_nms(dets, cls, 0.5, normalized, backend="cuda")
                if keep.numel() > oracle.nms_post:                                  # postprocess.py:150-154
                    keep = keep[kd[:, -1].topk(oracle.nms_post)[1]]
                assert post.last_keep[b].cpu().long().tolist() == keep.tolist(), (src, nms_pre, normalized, b)
