"""The Restormer fixtures past 64 channels per head (numpy only): the cases of make_golden_restormer_wide.py and of the tests, on the
helpers of gen_restormer.py.  decoder_level1 and the refinement run 2 dim channels on heads[0] heads (restormer.py:341-358), so the
published network (dim 48, heads[0] = 1) has 96 channels per head there and dim 64 the 128 the engine takes at most."""
from __future__ import annotations

from collections import OrderedDict

from gen_restormer import DEFAULTS, full_cfg, make_input, make_state, param_shapes  # noqa: F401

# the fixtures: constructor arguments, batch, image size, seed
CASES = OrderedDict([
    # Restormer() as published: dim 48, 3 -> 3 channels, depths 4 / 6 / 6 / 8 + 4, heads 1 / 2 / 4 / 8
    ("e_defaults_dim48", dict(cfg=dict(), shape=(1, 3, 16, 24), seed=105)),
    # 128 channels per head at decoder_level1 and the refinement
    ("f_dim64_cap", dict(cfg=dict(inp_channels=1, out_channels=1, dim=64, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),
                         shape=(1, 1, 16, 16), seed=106)),
])
