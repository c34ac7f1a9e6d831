"""The bf16x6 math mode of the SwinFIR and HAT engines without a GPU: the signature defaults (math=None changes nothing), the CLI's
--math reaching train.test, the refusals that need no device, and set_math kept by a module that has no engine yet."""
import copy
import inspect
import pickle
import sys

import pytest

import gen_hat as gh
import gen_swinfir as gs


def test_signature_defaults():
    from xmm_superres_denoise import engine, infer, train
    assert inspect.signature(infer.load_model).parameters["math"].default is None
    assert inspect.signature(train.test).parameters["math"].default is None
    for fn in (engine.sw_gemm, engine.sw_conv3x3):
        p = inspect.signature(fn).parameters
        assert p["math"].default == "fp32" and p["bias"].default is None
    assert inspect.signature(engine.sw_gemm).parameters["act"].default is None
    assert list(inspect.signature(engine.sw_gemm).parameters)[:5] == ["a", "w", "bias", "act", "math"]
    assert list(inspect.signature(engine.sw_conv3x3).parameters)[:4] == ["x", "w", "bias", "math"]
    for cls in (engine.SwinFIREngine, engine.HATEngine):
        assert cls.MATH == {"fp32": 0, "bf16x6": 3}          # the mode numbers of xsd_set_math
        assert callable(cls.set_math) and callable(cls.get_math)
    assert engine.RestormerEngine.MATH == {"fp32": 0}


@pytest.mark.parametrize("model,math", [("hat", "bf16x6"), ("swinfir", "bf16x6"), ("hat", None), ("restormer", "fp32"), ("esr_gen", "f16x3")])
def test_cli_math_reaches_test(monkeypatch, model, math):
    from xmm_superres_denoise import train
    seen = {}
    monkeypatch.setattr(train, "test", lambda *a, **k: seen.update(k, args=a))
    argv = ["train.py", "test", "--model", model, "--checkpoint", "c.ckpt", "--dataset-dir", "d"] + (["--math", math] if math else [])
    monkeypatch.setattr(sys, "argv", argv)
    train.main()
    assert seen["args"] == ("c.ckpt", "d") and seen["name"] == model and seen["math"] == math


def test_cli_refuses_restormer_in_another_mode(monkeypatch, capsys):
    from xmm_superres_denoise import train
    monkeypatch.setattr(train, "test", lambda *a, **k: pytest.fail("test must not run"))
    monkeypatch.setattr(sys, "argv", ["train.py", "test", "--model", "restormer", "--checkpoint", "c.ckpt", "--dataset-dir", "d", "--math", "bf16x6"])
    with pytest.raises(SystemExit):
        train.main()
    assert "restormer: math mode 'bf16x6' is not supported" in capsys.readouterr().err


def test_refusals_that_need_no_gpu():
    from xmm_superres_denoise.engine import HATEngine, RestormerEngine, SwinFIREngine, XsdError
    from xmm_superres_denoise.infer import load_model
    with pytest.raises(ValueError, match="restormer: math mode 'bf16x6' is not supported"):
        load_model("no_such.ckpt", "restormer", math="bf16x6")       # said before anything is built or read
    r = object.__new__(RestormerEngine)                              # the refusal does not depend on the engine's state
    with pytest.raises(XsdError, match="Restormer: math mode 'bf16x6' is not supported"):
        r.set_math("bf16x6")
    r.set_math("fp32")
    assert r.get_math() == "fp32"
    for cls, name in ((HATEngine, "HAT"), (SwinFIREngine, "SwinFIR")):
        e = object.__new__(cls)                                      # both are refused before the library is asked
        with pytest.raises(XsdError, match=f"{name}: math mode 'f16x3' is not supported.*per-tensor scale"):
            e.set_math("f16x3")
        with pytest.raises(XsdError, match=f"{name}: unknown math mode 'tf32'.*bf16x6.*fp32"):
            e.set_math("tf32")


@pytest.mark.parametrize("net", ["hat", "swinfir"])
def test_set_math_is_kept_by_a_module_without_an_engine(net):
    import xmm_superres_denoise.models as models
    gen, cls = {"hat": (gh, "HAT"), "swinfir": (gs, "SwinFIR")}[net]
    case = next(iter(gen.CASES.values()))
    m = getattr(models, cls)(**gen.full_cfg(**case["cfg"]))
    assert m.get_math() == "fp32" and m._math is None
    assert m.set_math("bf16x6") is m
    assert m._engine is None and m.get_math() == "bf16x6"
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert other._engine is None and other.get_math() == "bf16x6"
    with pytest.raises(ValueError, match="per-tensor scale"):
        m.set_math("f16x3")
    with pytest.raises(ValueError, match="math mode 'tf32' is not supported"):
        m.set_math("tf32")
    assert m.get_math() == "bf16x6"
    assert m.set_math("fp32").get_math() == "fp32"
    # the reference's constructor signature has no math argument
    assert "math" not in inspect.signature(type(m).__init__).parameters
