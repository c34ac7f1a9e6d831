from ._lib import XsdError, build, load  # noqa: F401
from .engine import Engine, ExtMetricsEngine, HATEngine, RestormerEngine, STRETCH, SwinFIREngine, fft_size_supported, hat_channel_mean, hat_ocab_attention, sw_conv3x3, sw_gemm, compose_batch, compose_input, image_upsample, mask_pad_normalize, normalize  # noqa: F401
