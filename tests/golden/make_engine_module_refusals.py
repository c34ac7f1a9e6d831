"""Writes tests/golden/engine_module_refusals.json: what the five engine-backed modules (GeneratorRRDB_DN / _SR, Restormer, SwinFIR,
HAT, SwinIR) answer to a call that breaks ONE rule -- exception type and full message -- for every `raise` of their constructors that
one wrong argument reaches, set_math with an unknown mode and with 'f16x3', _get_engine on the CPU device and forward on CPU tensors of
the wrong dtype, rank, channel count or size.  No GPU and no library needed.

The committed JSON was recorded at the commit BEFORE the modules got their shared base (models/modules/flat_params.py), so
tests/test_engine_module_host.py holds the shared code to the words each module had of its own.  Restormer had no set_math then:
its entries were recorded through infer.load_model(..., "restormer", math=mode), whose wording Restormer.set_math took over.

    python tests/golden/make_engine_module_refusals.py        # rewrites the JSON from the code as it is now
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "xmm-superres-denoise_amd"))
OUT = os.path.join(HERE, "engine_module_refusals.json")

SWIN = dict(img_size=64, in_chans=1, embed_dim=8, depths=[1], num_heads=[1], window_size=4, upsampler="pixelshuffle")
OK = {
    "GeneratorRRDB_DN": dict(in_channels=1, out_channels=1, num_filters=4, num_res_blocks=1),
    "GeneratorRRDB_SR": dict(in_channels=1, out_channels=1, num_filters=4, num_res_blocks=1),
    "Restormer": dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 1, 1, 1]),
    "SwinFIR": SWIN,
    "HAT": dict(SWIN, compress_ratio=2, squeeze_factor=4),
    "SwinIR": SWIN,
}
# one wrong argument each ("@nn.X" stands for torch.nn.X); a dict with several keys sets up the one rule the LAST key breaks
SWIN_WRONG = [dict(ape=True), dict(upsampler="bogus"), dict(resi_connection="HSFB"), dict(norm_layer="@nn.BatchNorm2d"), dict(upscale=5),
              dict(in_chans=0), dict(in_chans=65), dict(embed_dim=1), dict(depths=[1] * 17), dict(depths=[65]), dict(num_heads=[]),
              dict(num_heads=[3]), dict(num_heads=[0]), dict(embed_dim=64), dict(mlp_ratio=0), dict(mlp_ratio=0.01), dict(img_range=0),
              dict(qk_scale=-1.0), dict(window_size=17), dict(window_size=0)]
WRONG = {
    "GeneratorRRDB_DN": [dict(in_channels=0), dict(out_channels=2000), dict(num_filters=0), dict(in_channels=2), dict(num_res_blocks=0),
                         dict(num_res_blocks=65)],
    "GeneratorRRDB_SR": [dict(in_channels=0), dict(num_filters=2000), dict(num_res_blocks=0), dict(num_upsample=3), dict(num_upsample=0)],
    "Restormer": [dict(dual_pixel_task=True), dict(out_channels=2), dict(inp_channels=0, out_channels=0), dict(dim=7), dict(dim=0),
                  dict(dim=2048), dict(num_blocks=[1, 1, 1]), dict(heads=[1, 1, 1]), dict(num_blocks=[65, 1, 1, 1]),
                  dict(num_refinement_blocks=65), dict(heads=[3, 1, 1, 1]), dict(heads=[1, 0, 1, 1]), dict(dim=256),
                  dict(ffn_expansion_factor=0), dict(ffn_expansion_factor=0.01)],
    "SwinFIR": SWIN_WRONG + [dict(upscale=1), dict(upsampler=""), dict(resi_connection="3conv")],
    "HAT": SWIN_WRONG + [dict(upscale=1), dict(upsampler=""), dict(resi_connection="SFB"), dict(window_size=1), dict(overlap_ratio=-0.5),
                         dict(overlap_ratio=0.3), dict(overlap_ratio=7.5), dict(compress_ratio=0), dict(compress_ratio=9),
                         dict(squeeze_factor=0), dict(squeeze_factor=30), dict(img_size=2)],
    "SwinIR": SWIN_WRONG + [dict(upsampler="nearest+conv", upscale=3), dict(resi_connection="3conv", embed_dim=2)],
}
# forward on CPU tensors: (dtype, shape).  The last of each list passes the module's own checks and ends at the CPU-device refusal.
INPUTS = {
    "GeneratorRRDB_DN": [("float64", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 1, 8, 8])],
    "GeneratorRRDB_SR": [("float16", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 1, 8, 8])],
    "Restormer": [("float64", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 2, 8, 8]), ("float32", [1, 1, 12, 16]),
                  ("float32", [1, 1, 8, 8])],
    "SwinFIR": [("float64", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 2, 8, 8]), ("float32", [1, 1, 8, 6]),
                ("float32", [1, 1, 8, 17 * 4]), ("float32", [1, 1, 8, 8])],
    "HAT": [("float64", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 2, 8, 8]), ("float32", [1, 1, 6, 8]), ("float32", [1, 1, 8, 8])],
    "SwinIR": [("bfloat16", [1, 1, 8, 8]), ("float32", [1, 8, 8]), ("float32", [1, 2, 8, 8]), ("float32", [1, 1, 2, 8]),
               ("float32", [1, 1, 8, 8])],
}
MODES = ("nope", "f16x3")


def build(cls: str, kwargs: dict):
    import xmm_superres_denoise.models as M
    from torch import nn
    kw = {k: getattr(nn, v[4:]) if isinstance(v, str) and v.startswith("@nn.") else v for k, v in kwargs.items()}
    return getattr(M, cls)(**kw)


def run(entry: dict):
    """the call an entry describes; raises what the module raises"""
    import torch
    call, arg = entry["call"], entry.get("arg")
    if call == "load_model_math":        # never opens the checkpoint: the mode is refused first
        from xmm_superres_denoise.infer import load_model
        return load_model("no_such.ckpt", "restormer", math=arg)
    m = build(entry["cls"], entry["kwargs"])
    if call == "set_math":
        return m.set_math(arg)
    if call == "get_engine_cpu":
        return m._get_engine(torch.device("cpu"))
    if call == "forward":
        return m(torch.zeros(arg[1], dtype=getattr(torch, arg[0])))
    return m


def outcome(entry: dict):
    try:
        run(entry)
    except Exception as e:      # noqa: BLE001 -- the record IS the exception
        return type(e).__name__, str(e)
    return None, None


def entries():
    for cls, ok in OK.items():
        for wrong in WRONG[cls]:
            yield dict(cls=cls, call="ctor", kwargs=dict(ok, **wrong))
        for mode in MODES:
            if cls == "Restormer":
                yield dict(cls=cls, call="load_model_math", kwargs=ok, arg=mode)
            else:
                yield dict(cls=cls, call="set_math", kwargs=ok, arg=mode)
        yield dict(cls=cls, call="get_engine_cpu", kwargs=ok)
        for dtype, shape in INPUTS[cls]:
            yield dict(cls=cls, call="forward", kwargs=ok, arg=[dtype, shape])


if __name__ == "__main__":
    table = []
    for e in entries():
        e["type"], e["message"] = outcome(e)
        table.append(e)
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(f"{len(table)} entries, {sum(e['type'] is None for e in table)} without an exception -> {OUT}")
