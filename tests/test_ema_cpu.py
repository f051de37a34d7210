"""CPU tests of the weight EMA of orienmask_amd.optim.SGD: the numpy yardstick (tests/ema_np.py) against a float64 average and against
known decays, the mutants the GPU comparison (tests/test_ema.py, the same case table) has to catch, and the host logic: refusals,
state_dict, build_optimizer, tools/train.py's and tools/eval_val2017.py's flags, the trainer's checkpoints and resume."""
import contextlib
import importlib.util
import inspect
import os
import types

import numpy as np
import pytest
import torch

from conftest import REPO
import ema_cases as K
import ema_np as E
import optim_np as N
import test_trainer_cpu as TC
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O

F32 = np.float32


# ---- 1: the yardstick against a float64 average ---------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.9998, 0.5])
def test_yardstick_tracks_a_float64_average(decay):
    """The float64 average E of the SAME float32 parameter sequence with the SAME float32 omd: E' = E + (p' - E) * omd.  The two
    differ by the yardstick's two roundings per step.  With M the largest magnitude among parameters and shadows: |p' - e| <= 2 M,
    so rounding the difference errs by at most ulp(2 M) / 2 = ulp(M), which the fma scales by omd; the fma's own rounding errs by at
    most ulp(M) / 2; the error carried over from the step before is scaled by 1 - omd <= 1.  For omd <= 1/2 (both decays here,
    warm-up off) a step so adds at most omd * ulp(M) + ulp(M) / 2 <= ulp(M): after `steps` steps |e - E| <= steps * ulp(M).  The
    float64 average's own error is 2^-29 of that."""
    steps = 50
    p0, grads = N.seeded_inputs(21, n=1003, steps=steps)
    out = E.run([p0], [[g] for g in grads], dict(lr=1e-3, momentum=0.9, weight_decay=5e-4), decay, warmup=False)
    omd = E.omd_at(0, decay, warmup=False)
    assert float(omd) <= 0.5
    wide = p0.astype(np.float64)
    biggest = float(np.abs(p0).max())
    for k, (ps, _, shadows, count, skipped) in enumerate(out):
        assert count == k + 1 and not skipped
        wide = wide + (ps[0].astype(np.float64) - wide) * np.float64(omd)
        biggest = max(biggest, float(np.abs(ps[0]).max()), float(np.abs(shadows[0]).max()))
        bound = (k + 1) * float(np.spacing(F32(biggest)))
        err = float(np.abs(shadows[0].astype(np.float64) - wide).max())
        assert err <= bound, (k, err, bound)
    print("decay", decay, "steps", steps, "max error", err, "bound", bound)
    assert np.abs(shadows[0] - p0).max() > 0 and np.abs(shadows[0] - ps[0]).max() > 0        # it moved, and it lags


# ---- 2: known decays ------------------------------------------------------------------------------------------------------------
def test_decay_at_known_answers():
    assert E.decay_at(0, 0.9998) == 0.1 and E.decay_at(1, 0.9998) == 2.0 / 11.0
    for k in range(8):
        assert E.decay_at(k, 0.5) == (1.0 + k) / (10.0 + k) < 0.5, k
    assert E.decay_at(8, 0.5) == 0.5 == (1.0 + 8) / (10.0 + 8)              # the cap takes over exactly here
    for k in (9, 10, 1000, 10 ** 9):
        assert E.decay_at(k, 0.5) == 0.5 < (1.0 + k) / (10.0 + k)
    assert E.decay_at(44990, 0.9998) == 0.9998 and E.decay_at(44989, 0.9998) < 0.9998   # (1 + k) / (10 + k) = 0.9998 at k = 44990
    for k in (0, 3, 10 ** 6):
        assert E.decay_at(k, 0.9998, warmup=False) == 0.9998 and E.decay_at(k, 0.1, warmup=False) == 0.1
    # omd is rounded once, from the float64 difference
    assert E.omd_at(0, 0.9998) == F32(0.9) and E.omd_at(0, 0.9998, warmup=False) == F32(1.0 - 0.9998)
    assert E.omd_at(0, 0.9998, warmup=False) != E.omd_at(0, 0.9998, warmup=False, f32_decay=True)
    # the optimizer's host side computes the same numbers
    for decay in (0.9998, 0.5, 0.1):
        for warmup in (True, False):
            for k in list(range(30)) + [44989, 44990, 44991, 10 ** 7]:
                assert O.ema_decay_at(k, decay, warmup) == float(E.decay_at(k, decay, warmup))
                assert F32(1.0 - O.ema_decay_at(k, decay, warmup)) == E.omd_at(k, decay, warmup)


def test_ema_update_is_one_difference_and_one_fma():
    e = np.array([1.0, -2.0, 0.0, 3.0e38, np.inf, np.nan], F32)
    p = np.array([1.5, -2.0, -0.0, -3.0e38, 1.0, 1.0], F32)
    got = E.ema_update(e, p, F32(0.25))
    assert got[0] == F32(1.125) and got[1] == F32(-2.0) and got[2] == 0
    assert got[3] == -np.inf                               # the difference overflows to -Inf, and the fma keeps it
    assert np.isnan(got[4]) and np.isnan(got[5])           # fma(-Inf, omd, Inf) and NaN propagate
    x = np.array([0.1], F32)
    assert N.same_bits(E.ema_update(x, x, F32(0.3)), x)    # p' == e: nothing moves, whatever omd


# ---- 3: the GPU test's cases tell the yardstick from each mutant -------------------------------------------------------------------
def _same(a, b):
    for (pa, ba, ea, ka, sa), (pb, bb, eb, kb, sb) in zip(a, b):
        if ka != kb or sa != sb:
            return False
        for x, y in zip(pa + ea, pb + eb):
            if not N.same_bits(x, y):
                return False
    return len(a) == len(b)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_case_catches_the_mutants_it_names(name):
    case = K.CASES[name]
    want = K.reference(name)
    assert _same(want, K.run_case(case))                    # the yardstick repeats
    for mutant in case["catches"]:
        assert mutant in E.MUTANTS
        assert not _same(want, K.run_case(case, **{mutant: True})), (name, mutant)
    # no mutant changes a parameter or a momentum buffer, and the yardstick's are the step's own (the average does not disturb it)
    cur, bufs = [p.copy() for p in case["params"]], [None] * len(case["params"])
    for grads, (ps, bs, _, _, skipped) in zip(case["grads"], want):
        if case["max_norm"] is None:
            cur, bufs = N.sgd_step_many(cur, grads, bufs, case["hypers"])
        else:
            import clip_np as C
            cur, bufs, _, _, was = C.clipped_step(cur, grads, bufs, case["hypers"], case["max_norm"], case["nonfinite"])
            assert was == skipped
        assert all(N.same_bits(a, b) for a, b in zip(cur, ps))
        assert all((a is None) == (b is None) and (a is None or N.same_bits(a, b)) for a, b in zip(bufs, bs))


def test_every_mutant_is_named_by_a_case_and_the_table_is_what_the_issue_lists():
    named = {m for case in K.CASES.values() for m in case["catches"]}
    assert named == set(E.MUTANTS)
    assert K.COUNTS == [1, 3, 4, 1003, 4096, 4097, 2 * 4096 + 5] and O.OM_SGD_CHUNK == 4096
    assert {"hyper_" + h for h in N.HYPER_SETS} <= set(K.CASES) and "special" in K.CASES
    skip = K.reference("skip")
    assert [s for *_, s in skip] == [False, True, False, True, False] and [k for *_, k, _ in skip] == [1, 1, 2, 2, 3]
    for before, after in ((0, 1), (2, 3)):                  # across a skipped step nothing moves
        for x, y in zip(skip[before][0] + skip[before][1] + skip[before][2], skip[after][0] + skip[after][1] + skip[after][2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    none = K.reference("grad_none")
    assert N.same_bits(none[0][2][1], none[2][2][1]) and not N.same_bits(none[2][2][1], none[3][2][1])      # the shadow waits
    assert [k for *_, k, _ in none] == [1, 2, 3, 4]         # the count is global
    cross = K.reference("warmup_cross")
    assert len(cross) == 11
    coefs = [float(C) for C in (E.omd_at(k, 0.5) for k in range(11))]
    assert coefs[0] == float(F32(0.9)) and all(c > 0.5 for c in coefs[:8]) and coefs[8:] == [0.5, 0.5, 0.5]
    clip = K.CASES["clip_below_one"]
    import clip_np as C
    assert all(C.coefficient(C.norm_of(g)[0], clip["max_norm"]) < 0.01 for g in clip["grads"])


# ---- 4: options -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_signature(monkeypatch):
    cpu = torch.nn.Parameter(torch.zeros(4))
    for bad in (0, 0.0, 1, 1.0, -0.5, 1.5, float("nan"), float("inf"), "0.9", True, False, [0.9]):
        with pytest.raises(ValueError, match="ema_decay"):
            O.SGD([cpu], lr=1e-3, ema_decay=bad)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        O.SGD([cpu], lr=1e-3, ema_decay=torch.tensor(0.9))
    with pytest.raises(ValueError, match="ema_warmup"):
        O.SGD([cpu], lr=1e-3, ema_decay=0.9, ema_warmup="yes")
    kinds = inspect.signature(O.SGD.__init__).parameters
    assert kinds["ema_decay"].kind is kinds["ema_warmup"].kind is inspect.Parameter.KEYWORD_ONLY
    assert kinds["ema_decay"].default is None and kinds["ema_warmup"].default is True
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU or eager fallback"):
        O.SGD([cpu], lr=1e-3, ema_decay=0.9)                                 # valid options: the device check is what refuses
    monkeypatch.setattr(O, "_check_param", lambda p: None)                   # past the device check, on a host without a GPU
    opt = O.SGD([cpu], lr=1e-3, momentum=0.9, ema_decay=0.9998, ema_warmup=False)
    assert opt.ema_decay == 0.9998 and opt.ema_warmup is False and opt.ema_updates() == 0
    assert "ema_decay" not in opt.defaults and "ema_warmup" not in opt.defaults
    assert all("ema_decay" not in g and "ema_warmup" not in g for g in opt.param_groups)
    plain = O.SGD([cpu], lr=1e-3, momentum=0.9)
    assert plain.ema_decay is None
    for o in (opt, plain):
        o.state[cpu]["momentum_buffer"] = torch.ones(4)
    a, b = plain.state_dict(), opt.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"] and a["param_groups"] == b["param_groups"]
    assert all(sorted(v) == ["momentum_buffer"] for v in b["state"].values())
    torch.optim.SGD([cpu], lr=1.0).load_state_dict(b)                        # torch's own keys, nothing more
    # a value assigned later is refused at step(), before anything is launched
    monkeypatch.setattr(omlib, "load", lambda: None)
    opt.ema_decay = 1.0
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()
    opt.ema_decay = torch.tensor(0.5)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        opt.step()
    # parameters on more than one device: one count, one swap
    two = O.SGD([cpu, torch.nn.Parameter(torch.zeros(4, device="meta"))], lr=1e-3, ema_decay=0.9)
    with pytest.raises(omlib.OrienMaskHipError, match="one device"):
        two._build_plans()
    for method in ("ema_swap", "ema_shadow", "ema_state_dict"):
        with pytest.raises(omlib.OrienMaskHipError, match="not enabled"):
            getattr(plain, method)(*{"ema_shadow": [cpu], "ema_state_dict": [torch.nn.Linear(1, 1)]}.get(method, []))
    with pytest.raises(ValueError, match="updates"):
        opt.load_ema_state_dict(torch.nn.Linear(1, 1), {}, -1)


def test_constants_and_signatures_match_the_header():
    import re
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define (OM_EMA_[A-Z_]+) (\d+)", header)}
    assert defines == dict(OM_EMA_UPDATES_OFF=0, OM_EMA_OMD_OFF=1, OM_EMA_STATE_DOUBLES=2)
    assert all(getattr(O, name) == value for name, value in defines.items())
    assert O.OM_CLIP_STATE_DOUBLES == 9 and O.TENSOR_ROW.itemsize == 64      # neither grew
    sig = omlib.SIGNATURES
    assert len(sig["om_sgd_ema_step"][1]) == 8 and len(sig["om_sgd_clip_ema_step"][1]) == 16 and len(sig["om_ema_swap"][1]) == 7
    assert len(sig["om_sgd_step"][1]) == 6 and len(sig["om_sgd_clip_step"][1]) == 12


def test_launchers_validate(built):
    L = omlib.load()
    assert L.om_sgd_ema_step(None, None, 1, None, 1, None, 0.5, None) != 0 and b"om_sgd_ema_step" in L.om_last_error()
    for bad in (0.0, -0.1, 1.5, float("nan")):              # the pointers are never followed: 64 is just not null
        assert L.om_sgd_ema_step(None, 64, 1, 64, 1, 64, bad, None) != 0 and b"omd" in L.om_last_error(), bad
    assert L.om_sgd_ema_step(None, 64, 0, 64, 1, 64, 0.5, None) != 0 and b"tensors" in L.om_last_error()
    ok = (None, 64, 1, 64, 1, 64, 64, 64, 1.0, 0, 1, 64, 64, 0.9, 1, None)
    for at, bad, word in ((11, None, b"null"), (12, None, b"null"), (12, 68, b"misaligned"), (13, 0.0, b"decay"), (13, 1.0, b"decay"),
                          (8, 0.0, b"max_norm"), (10, 0, b"step"), (2, 0, b"tensors")):
        args = list(ok)
        args[at] = bad
        assert L.om_sgd_clip_ema_step(*args) != 0 and word in L.om_last_error(), (at, bad, L.om_last_error())
    assert L.om_ema_swap(None, 64, 1, 64, 1, None, None) != 0 and b"om_ema_swap" in L.om_last_error()
    assert L.om_ema_swap(None, None, 1, 64, 1, 64, None) != 0 and b"null table" in L.om_last_error()


# ---- 5: builder and tools -------------------------------------------------------------------------------------------------------
def test_build_optimizer_passes_the_two_keys(monkeypatch):
    monkeypatch.setattr(O, "_check_param", lambda p: None)
    model = N.groups_module()
    config = dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4, ema_decay=0.9998, ema_warmup=False,
                  param_groups=dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4))
    before = repr(config)
    opt = builder.build_optimizer(config, 2, model)
    assert type(opt) is O.SGD and opt.ema_decay == 0.9998 and opt.ema_warmup is False and repr(config) == before
    assert opt.param_groups[0]["lr"] == 5e-4 and "ema_decay" not in opt.param_groups[0]
    plain = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, model)
    assert plain.ema_decay is None and plain.ema_warmup is True
    with pytest.raises(ValueError, match="ema_decay"):
        builder.build_optimizer(dict(type="SGD", lr=1e-3, ema_decay=1.0), 1, model)


def _tool(name):
    spec = importlib.util.spec_from_file_location("om_tool_ema_" + name, os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_train_tool_parses_the_two_flags():
    tool = _tool("train")
    config = dict(model=dict(type="OrienMaskYOLOFPNPlus"), optimizer=dict(type="SGD", lr=1e-3, ema_decay=0.99))
    args = tool.parse_args(["--config", "c.json", "--ema-decay", "0.9998", "--no-ema-warmup"])
    assert args.ema_decay == 0.9998 and args.no_ema_warmup is True
    out = tool.apply_overrides(config, args)
    assert out["optimizer"] == dict(type="SGD", lr=1e-3, ema_decay=0.9998, ema_warmup=False)
    assert config["optimizer"] == dict(type="SGD", lr=1e-3, ema_decay=0.99)             # the caller's dict is not mutated
    none = tool.parse_args(["--config", "c.json"])
    assert none.ema_decay is None and none.no_ema_warmup is False and tool.apply_overrides(config, none) is config
    only = tool.apply_overrides(config, tool.parse_args(["--config", "c.json", "--ema-decay", "0.5"]))
    assert only["optimizer"] == dict(type="SGD", lr=1e-3, ema_decay=0.5)


def test_eval_tool_takes_the_averaged_weights_or_refuses():
    tool = _tool("eval_val2017")
    ckpt = dict(state_dict={"w": 1}, config={}, ema=dict(state_dict={"w": 2}, updates=3))
    assert tool.ema_checkpoint(ckpt, False) is ckpt
    got = tool.ema_checkpoint(ckpt, True)
    assert got["state_dict"] == {"w": 2} and got["config"] == {} and ckpt["state_dict"] == {"w": 1}
    for bare in (dict(state_dict={"w": 1}, config={}), {"w": 1}):
        with pytest.raises(SystemExit, match="no averaged weights"):
            tool.ema_checkpoint(bare, True, "x.pth")


# ---- 6: the trainer's checkpoints ---------------------------------------------------------------------------------------------------
class AveragingSGD(torch.optim.SGD):
    """The stand-in of this GPU-less path: torch.optim.SGD (as tests/test_trainer_cpu.py uses) with the averaging INTERFACE of
    orienmask_amd.optim.SGD on the host.  The trainer is what these tests are about; the arithmetic is tests/test_ema.py's."""

    def __init__(self, params, ema_decay=None, ema_warmup=True, **kw):
        super().__init__(params, **kw)
        self.ema_decay, self.ema_warmup, self.k = ema_decay, ema_warmup, 0
        self.shadows = None
        self.swaps = 0

    def _held(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _ensure(self):
        if self.shadows is None:
            self.shadows = [p.detach().clone() for p in self._held()]

    def step(self, closure=None):
        self._ensure()
        super().step(closure)
        omd = float(F32(1.0 - O.ema_decay_at(self.k, self.ema_decay, self.ema_warmup)))
        with torch.no_grad():
            for e, p in zip(self.shadows, self._held()):
                e.add_(p - e, alpha=omd)
        self.k += 1

    def ema_updates(self):
        return self.k

    def ema_swap(self):
        self._ensure()
        self.swaps += 1
        with torch.no_grad():
            for e, p in zip(self.shadows, self._held()):
                keep = p.detach().clone()
                p.copy_(e)
                e.copy_(keep)

    @contextlib.contextmanager
    def ema_applied(self):
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()

    def ema_state_dict(self, model):
        self._ensure()
        shadow = {id(p): e for p, e in zip(self._held(), self.shadows)}
        out = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in shadow:
                out[name] = shadow[id(p)].clone()
        return out

    def load_ema_state_dict(self, model, state_dict, updates):
        self._ensure()
        shadow = {id(p): e for p, e in zip(self._held(), self.shadows)}
        with torch.no_grad():
            for name, p in model.named_parameters(remove_duplicate=False):
                if id(p) in shadow:
                    shadow[id(p)].copy_(state_dict[name])
        self.k = updates

    def ema_reset(self):
        self.shadows, self.k = None, 0


def _ema_trainer(config, resume=None, val_loader=None, cls=None):
    from orienmask_amd.trainer import Trainer
    torch.manual_seed(3)                                    # the model of tests/test_trainer_cpu.py's _parts
    model = torch.nn.Sequential(torch.nn.Linear(6, config["model"]["hidden"]), torch.nn.Linear(config["model"]["hidden"], 2))
    oc = dict(config["optimizer"])
    oc.pop("type")
    oc["lr"] = oc["lr"] / config["accumulate"]
    optimizer = AveragingSGD(model.parameters(), **oc)
    sc = dict(config["lr_scheduler"])
    scheduler = getattr(O, sc.pop("type"))(optimizer=optimizer, **sc)
    return (cls or Trainer)(model, TC.StubLoss(), optimizer, scheduler, config, TC._loader(), val_loader, None, torch.device("cpu"),
                            types.SimpleNamespace(resume=resume, weights=None), sync_free=False)


EMA_OPT = dict(type="SGD", lr=0.05, momentum=0.9, weight_decay=1e-4, ema_decay=0.9, ema_warmup=True)


def test_checkpoint_gains_the_ema_key_only_with_averaging(built, tmp_path):
    t = _ema_trainer(TC._config(tmp_path, "ema", epochs=2, save_freq=2, optimizer=EMA_OPT))
    t.train()
    ck = torch.load(os.path.join(t.checkpoint_dir, "epoch2.pth"), weights_only=False)
    assert set(ck) == TC.CHECKPOINT_KEYS | {"ema"} and set(ck["ema"]) == {"state_dict", "updates"}
    assert ck["ema"]["updates"] == t.optimizer.k == 6                       # 3 optimizer steps per epoch (accumulate 2, 5 batches)
    assert set(ck["ema"]["state_dict"]) == set(ck["state_dict"])
    assert all(torch.equal(ck["ema"]["state_dict"][k], e) for k, e in zip(ck["state_dict"], t.optimizer.shadows))
    assert any(not torch.equal(ck["ema"]["state_dict"][k], ck["state_dict"][k]) for k in ck["state_dict"])
    # the six reference keys are what a run without averaging writes, and that file has no seventh
    plain = TC._trainer(TC._config(tmp_path, "plain", epochs=2, save_freq=2))
    plain.train()
    pk = torch.load(os.path.join(plain.checkpoint_dir, "epoch2.pth"), weights_only=False)
    assert set(pk) == TC.CHECKPOINT_KEYS
    assert TC._equal_state(pk["state_dict"], ck["state_dict"]) and TC._equal_state(pk["optimizer"], ck["optimizer"])
    # batch_<step>.pth too
    m = _ema_trainer(TC._config(tmp_path, "maxiter", epochs=3, optimizer=EMA_OPT, lr_scheduler=dict(type="PolyLR", max_iter=7, power=0.9)))
    m.train()
    bk = torch.load(os.path.join(m.checkpoint_dir, "batch_7.pth"), weights_only=False)
    assert set(bk) == {"state_dict", "config", "ema"} and bk["ema"]["updates"] == m.optimizer.k


def test_validation_sees_the_averaged_weights_and_puts_the_parameters_back(built, tmp_path, monkeypatch):
    from orienmask_amd import tester
    seen = []

    def validate(model, loss, postprocess, loader, coco_metrics, counter=None):
        seen.append({k: v.clone() for k, v in model.state_dict().items()})
        return {"val_loss": 1.0}
    monkeypatch.setattr(tester, "validate", validate)
    t = _ema_trainer(TC._config(tmp_path, "val", epochs=1, optimizer=EMA_OPT), val_loader=[])
    t._log_result = lambda result: None
    t.train()
    assert len(seen) == 1 and t.optimizer.swaps == 2
    want = t.optimizer.ema_state_dict(t.model)
    live = t.model.state_dict()
    assert all(torch.equal(seen[0][k], want[k]) for k in want) and any(not torch.equal(seen[0][k], live[k]) for k in live)
    ck = torch.load(os.path.join(t.checkpoint_dir, "epoch1.pth"), weights_only=False)
    assert all(torch.equal(ck["state_dict"][k], live[k]) for k in live)          # the parameters are their own again
    # without averaging nothing is swapped
    plain = TC._trainer(TC._config(tmp_path, "plainval", epochs=1), val_loader=[])
    plain._log_result = lambda result: None
    plain.train()
    assert len(seen) == 2 and all(torch.equal(seen[1][k], v) for k, v in plain.model.state_dict().items())


def test_resume_restores_shadows_and_count_or_starts_again(built, tmp_path):
    whole = _ema_trainer(TC._config(tmp_path, "whole", epochs=4, optimizer=EMA_OPT))
    whole.train()
    first = _ema_trainer(TC._config(tmp_path, "first", epochs=2, optimizer=EMA_OPT))
    first.train()
    path = os.path.join(first.checkpoint_dir, "epoch2.pth")
    resumed = _ema_trainer(TC._config(tmp_path, "first", epochs=4, optimizer=EMA_OPT), resume=path)
    assert resumed.optimizer.k == 6 and all(torch.equal(a, b) for a, b in zip(resumed.optimizer.shadows, first.optimizer.shadows))
    resumed.train()
    assert resumed.optimizer.k == whole.optimizer.k == 12
    assert all(torch.equal(a, b) for a, b in zip(resumed.optimizer.shadows, whole.optimizer.shadows))
    assert TC._equal_state(whole.model.state_dict(), resumed.model.state_dict())
    # a checkpoint of the same config without the key: the average starts again from the loaded weights, and the log says so
    ck = torch.load(path, weights_only=False)
    del ck["ema"]
    bare = os.path.join(first.checkpoint_dir, "no_ema.pth")
    torch.save(ck, bare)
    again = _ema_trainer(TC._config(tmp_path, "first", epochs=4, optimizer=EMA_OPT), resume=bare)
    assert again.optimizer.k == 0 and again.optimizer.shadows is None and again.start_epoch == 3
    assert "starts again from the loaded weights" in open(os.path.join(first.checkpoint_dir, "train.log")).read()
    again.optimizer._ensure()
    assert all(torch.equal(e, ck["state_dict"][k]) for k, e in zip(ck["state_dict"], again.optimizer.shadows))
    # a run without averaging resumes from an averaging run's file only through the config check, as for any optimizer option
    with pytest.raises(AssertionError, match="differs from the checkpoint's"):
        TC._trainer(TC._config(tmp_path, "first", epochs=4), resume=path)
