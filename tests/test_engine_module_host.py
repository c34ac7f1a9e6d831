"""The base the five engine-backed modules share (models/modules/flat_params.py: FlatParams; swin_common.py: SwinFamily), without a GPU:
every refusal keeps the type and the words recorded before the modules were put on the base (tests/golden/engine_module_refusals.json,
written by tests/golden/make_engine_module_refusals.py), the engine state after construction and across copies and pickles,
Restormer's math mode, and that the plumbing exists once."""
import copy
import importlib
import inspect
import json
import os
import pickle
import pkgutil

import pytest
import torch

import make_engine_module_refusals as mr

G = os.path.join(os.path.dirname(__file__), "golden")
with open(os.path.join(G, "engine_module_refusals.json")) as f:
    TABLE = json.load(f)
STATE = ("_engine", "_engine_dev", "_flat", "_plist", "_math")
CLASSES = list(mr.OK)


def _expect(entry, call):
    if entry["type"] is None:
        call()
        return
    with pytest.raises(Exception) as e:
        call()
    assert (type(e.value).__name__, str(e.value)) == (entry["type"], entry["message"])


def _id(e):
    return f"{e['cls']}-{e['call']}-{TABLE.index(e)}"


def test_the_table_covers_what_the_script_lists():
    """every case of the script has its record (the script's lists are where a new refusal is added), and nothing in it is empty"""
    want = [{k: json.loads(json.dumps(v)) for k, v in e.items()} for e in mr.entries()]
    got = [{k: v for k, v in e.items() if k not in ("type", "message")} for e in TABLE]
    assert got == want
    for cls in CLASSES:
        mine = [e for e in TABLE if e["cls"] == cls]
        assert {e["call"] for e in mine} >= {"ctor", "get_engine_cpu", "forward"}
        assert all(e["type"] in ("ValueError", "XsdError") and e["message"] for e in mine if e["call"] != "set_math")


@pytest.mark.parametrize("entry", TABLE, ids=_id)
def test_refusal_keeps_its_type_and_words(entry):
    _expect(entry, lambda: mr.run(entry))
    if entry["call"] == "load_model_math":      # the words infer.load_model had of its own are Restormer.set_math's now
        _expect(entry, lambda: mr.build(entry["cls"], entry["kwargs"]).set_math(entry["arg"]))


@pytest.mark.parametrize("cls", CLASSES)
def test_state_after_construction_and_across_copies(cls):
    m = mr.build(cls, mr.OK[cls])
    assert all(getattr(m, a) is None for a in STATE), {a: getattr(m, a) for a in STATE}
    mode = "fp32" if cls == "Restormer" else "bf16x6"
    assert m.set_math(mode) is m and m.get_math() == mode and m._math == mode
    m._engine, m._engine_dev, m._flat, m._plist = object(), "cuda:0", torch.zeros(1), []     # as after a forward
    keys = list(m.state_dict())
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._math == mode and c.get_math() == mode
        assert all(getattr(c, a) is None for a in STATE[:-1]), {a: getattr(c, a) for a in STATE}
        assert list(c.state_dict()) == keys
        for (k, a), b in zip(m.state_dict().items(), c.state_dict().values()):
            assert torch.equal(a, b), k


def test_restormer_math_mode():
    from xmm_superres_denoise.models import Restormer
    m = Restormer(**mr.OK["Restormer"])
    assert m.get_math() == "fp32" and m.set_math("fp32").get_math() == "fp32"
    text = "restormer: math mode 'bf16x6' is not supported: the Restormer engine computes in 'fp32' only"
    with pytest.raises(ValueError) as e:
        m.set_math("bf16x6")
    assert str(e.value) == text and m.get_math() == "fp32"


def test_load_model_refuses_restormer_modes_with_a_real_checkpoint(tmp_path):
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.infer import load_model
    from xmm_superres_denoise.models import Model
    model = Model(model_cfg("restormer"), (16, 16), (16, 16))
    model.configure_model()
    ck = os.path.join(tmp_path, "restormer.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in model.model.state_dict().items()}}, ck)
    with pytest.raises(ValueError) as e:
        load_model(ck, "restormer", lr_res=16, device="cpu", math="bf16x6")
    assert str(e.value) == "restormer: math mode 'bf16x6' is not supported: the Restormer engine computes in 'fp32' only"
    loaded = load_model(ck, "restormer", lr_res=16, device="cpu", math="fp32")      # the one mode it takes; nothing runs on the CPU
    assert loaded.model.get_math() == "fp32"
    for (k, a), b in zip(model.model.state_dict().items(), loaded.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_the_plumbing_exists_once():
    import xmm_superres_denoise
    import xmm_superres_denoise.models as M
    from xmm_superres_denoise.models.modules.flat_params import FlatParams
    for cls in CLASSES:
        c = getattr(M, cls)
        assert issubclass(c, FlatParams)
        for name in ("_get_engine", "__getstate__", "set_math", "get_math", "_check_input", "flatten_parameters", "_param_version"):
            assert getattr(c, name) is getattr(FlatParams, name), (cls, name)
        for name in ("_pack_if_changed", "_packed_key"):      # no cached pack decision: every forward packs
            assert not hasattr(c, name) and not hasattr(mr.build(cls, mr.OK[cls]), name), (cls, name)
        assert "_make_engine" in vars(c) or any("_make_engine" in vars(b) for b in c.__mro__[1:] if b is not FlatParams), cls
    forward_only = set()
    for info in pkgutil.walk_packages(xmm_superres_denoise.__path__, "xmm_superres_denoise."):
        mod = importlib.import_module(info.name)
        for c in vars(mod).values():
            if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == mod.__name__ \
                    and "training is not on the MI355X engine" in inspect.getsource(c):
                forward_only.add(c)
    assert len(forward_only) == 1, forward_only
