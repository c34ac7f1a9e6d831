"""SwinFIR on the MI355X engine with several RSTB layers of each residual connection, against the float64 restatement on the device
(tests/golden/swinfir_torch.py): with "1conv" the forward swaps its two token buffers after every layer, so the layers after the first
run on swapped buffers; an explicit qk_scale; and the constructor's refusal of a negative qk_scale."""
import numpy as np
import pytest
import torch

import gen_swinfir as gs
import swinfir_torch as st

BASE = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, window_size=4, upsampler="pixelshuffle")


def _errs(y, ref):
    e = (y.double() - ref).abs()
    return float(e.pow(2).mean().sqrt()), float(e.max() / ref.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", [
    ("1conv_3_layers", dict(BASE, depths=[2, 1, 2], num_heads=[2, 2, 4], resi_connection="1conv")),
    ("1conv_4_layers_no_shift", dict(BASE, img_size=8, window_size=8, depths=[1, 1, 1, 1], num_heads=[2, 4, 2, 4],
                                     resi_connection="1conv")),
    ("sfb_3_layers_qk_scale", dict(BASE, depths=[2, 2, 1], num_heads=[2, 2, 2], qk_scale=0.3)),
])
def test_several_layers_match_float64_restatement(name, cfg):
    _run(name, cfg, (2, 1, 16, 24))


@pytest.mark.gpu
def test_sfb_at_14_x_22_runs_the_radix_7_and_11_passes():
    """the FourierUnit at H = 2 x 7 and W = 2 x 11 inside the network: window 2, SFB, two layers"""
    _run("sfb_14x22_window_2", dict(BASE, img_size=14, window_size=2, depths=[2, 1], num_heads=[2, 2]), (2, 1, 14, 22))


def _run(name, cfg, shape):
    from xmm_superres_denoise.models import SwinFIR
    state = gs.make_state(cfg, 41)
    m = SwinFIR(**gs.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    m = m.cuda()
    x = torch.from_numpy(gs.make_input(shape, 42)).cuda()
    with torch.no_grad():
        y = m(x)
        y64 = st.swinfir_forward({k: torch.from_numpy(v).cuda().double() if v.dtype == np.float32 else torch.from_numpy(v).cuda()
                                  for k, v in state.items()}, x.double(), **cfg)
        y32 = st.swinfir_forward({k: torch.from_numpy(v).cuda() for k, v in state.items()}, x, **cfg)
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{name}: engine rms {rms:.3e} max-rel {mx:.3e} | torch fp32 rms {rms32:.3e} max-rel {mx32:.3e}")
    assert y.shape == y64.shape
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (name, rms, rms32, mx, mx32)


def test_negative_qk_scale_is_refused_by_name():
    from xmm_superres_denoise.models import SwinFIR
    with pytest.raises(ValueError, match="qk_scale -0.5"):
        SwinFIR(**dict(BASE, depths=[1], num_heads=[2], qk_scale=-0.5))
    SwinFIR(**dict(BASE, depths=[1], num_heads=[2], qk_scale=0.0))        # `qk_scale or head_dim ** -0.5`: 0 is the default
