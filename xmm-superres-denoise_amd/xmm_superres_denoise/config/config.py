"""The slice of the reference's pydantic config that defines the constructor-API contract of the hot path
(reference config/config.py:36-42,164-203).  Python 3.10 here: enum.StrEnum restated as (str, Enum)."""
from enum import Enum
from pathlib import Path
from typing import List, Literal, Optional, Tuple, Union

from pydantic import BaseModel, Field, NonNegativeFloat, NonNegativeInt, PositiveInt, model_validator


class BaseModels(str, Enum):
    ESR_GEN = "esr_gen"
    RRDB_DENOISE = "rrdb_denoise"
    SWINFIR = "swinfir"
    DRCT = "drct"
    HAT = "hat"
    RESTORMER = "restormer"

    def __str__(self):
        return self.value


class OptimizerCfg(BaseModel):
    learning_rate: NonNegativeFloat
    betas: Tuple[NonNegativeFloat, NonNegativeFloat]


class RrdbCfg(BaseModel):
    base_model: Literal["esr_gen", "rrdb_denoise"]
    in_channels: PositiveInt
    out_channels: PositiveInt
    filters: PositiveInt
    residual_blocks: PositiveInt


class RestormerCfg(BaseModel):
    """reference config/config.py:187-191"""
    base_model: Literal["restormer"]
    in_channels: PositiveInt
    out_channels: PositiveInt
    dim: PositiveInt


class TransformerCfg(BaseModel):
    """reference config/config.py:177-186"""
    base_model: Literal["swinfir", "drct", "hat"]
    patch_size: PositiveInt
    img_size: PositiveInt
    window_size: PositiveInt
    embed_dim: PositiveInt
    upsampler: Literal["pixelshuffle", "pixelshuffledirect", "nearest+conv", ""]
    in_channels: PositiveInt
    num_heads: List[PositiveInt]
    depths: List[PositiveInt]


class ModelCfg(BaseModel):
    name: BaseModels
    memory_efficient: bool
    batch_size: PositiveInt
    # reference: RrdbCfg | TransformerCfg | RestormerCfg (of the TransformerCfg models, SwinFIR and HAT run forward on the engine; DRCT
    # is refused by Model.configure_model, and so is HAT without its forward_only_hat keyword)
    model: Union[RrdbCfg, TransformerCfg, RestormerCfg] = Field(..., discriminator="base_model")
    optimizer: OptimizerCfg


# res/configs/models.toml of the reference: the two shipped RRDB models, SwinFIR, DRCT, HAT and the Restormer denoiser
MODELS_TOML = {
    "esr_gen": dict(base_model="esr_gen", in_channels=1, out_channels=1, filters=32, residual_blocks=4,
                    learning_rate=0.0001, betas=(0.9, 0.999)),
    "rrdb_denoise": dict(base_model="rrdb_denoise", in_channels=1, out_channels=1, filters=32, residual_blocks=4,
                         learning_rate=0.0001, betas=(0.9, 0.999)),
    "swinfir": dict(base_model="swinfir", img_size=416, window_size=16, patch_size=32, embed_dim=180, upsampler="pixelshuffle",
                    in_channels=1, num_heads=[6, 6, 6, 6, 6, 6], depths=[6, 6, 6, 6, 6, 6], learning_rate=0.0002, betas=(0.9, 0.999)),
    # :32-56 -- DRCT is configurable but refused by Model.configure_model (its body is dead code in the reference); HAT is built forward
    # only: infer.load_model and train.test construct it, a bare configure_model refuses it
    "drct": dict(base_model="drct", img_size=416, window_size=16, patch_size=32, embed_dim=180, upsampler="pixelshuffle",
                 in_channels=1, num_heads=[6, 6, 6, 6, 6, 6], depths=[6, 6, 6, 6, 6, 6], learning_rate=0.0002, betas=(0.9, 0.999)),
    "hat": dict(base_model="hat", img_size=416, window_size=16, patch_size=16, embed_dim=180, upsampler="pixelshuffle",
                in_channels=1, num_heads=[6, 6, 6, 6, 6, 6], depths=[6, 6, 6, 6, 6, 6], learning_rate=0.0002, betas=(0.9, 0.999)),
    "restormer": dict(base_model="restormer", in_channels=1, out_channels=1, dim=24, learning_rate=0.0001, betas=(0.9, 0.999)),
}


def model_cfg(name: str, batch_size: int = 1, memory_efficient: bool = False, **overrides) -> ModelCfg:
    """What train.py:35-44 of the reference does: merge the run config's model section with models.toml[name]
    and split the optimizer fields out."""
    d = dict(MODELS_TOML[name])
    d.update(overrides)
    opt = OptimizerCfg(learning_rate=d.pop("learning_rate"), betas=tuple(d.pop("betas")))
    kind = {"restormer": RestormerCfg, "swinfir": TransformerCfg, "drct": TransformerCfg, "hat": TransformerCfg}
    cfg = kind.get(d["base_model"], RrdbCfg)(**d)
    return ModelCfg(name=BaseModels(name), memory_efficient=memory_efficient, batch_size=batch_size, model=cfg, optimizer=opt)


class ConfigError(Exception):
    """reference config/config.py:19-21"""

    def __init__(self, message: str = ""):
        super().__init__(message)


class LossCfg(BaseModel):
    """reference config/config.py:222-237: relative percentages of the loss terms, 0 < sum <= 1"""
    l1: float = Field(ge=0, le=1)
    poisson: float = Field(ge=0, le=1)
    psnr: float = Field(ge=0, le=1)
    ssim: float = Field(ge=0, le=1)
    ms_ssim: float = Field(ge=0, le=1)

    @model_validator(mode="after")
    def check_sum(self):
        p_sum = self.l1 + self.poisson + self.psnr + self.ssim + self.ms_ssim
        if 0 < p_sum <= 1:
            return self
        raise ConfigError(f"Sum of relative percentages has to be between 0 and 1, got {p_sum}!")


# ---- dataset section (reference config/config.py:24-33,77-161) ----------------------------------------------------------
class DatasetType(str, Enum):
    SIM = "sim"
    REAL = "real"
    BORING = "boring"

    def __str__(self):
        return self.value


class ImageType(str, Enum):
    IMG = "img"
    AGN = "agn"
    BKG = "bkg"

    def __str__(self):
        return self.value


class HrDatasetCfg(BaseModel):
    det_mask: Optional[Path] = None
    agn: bool = True
    exp: NonNegativeInt = 100
    clamp_max: NonNegativeFloat = 0.0005584
    res: PositiveInt = 832


class LrDatasetCfg(BaseModel):
    bkg: Union[bool, NonNegativeInt] = 1
    det_mask: Optional[Path] = None
    exps: List[PositiveInt] = [20]
    clamp_max: NonNegativeFloat = 0.0022336
    res: PositiveInt = 416


class DatasetCfg(BaseModel):
    """reference config/config.py:102-161 (defaults: res/baseline_config.toml [dataset]).  The file-existence validators of the
    detector masks run where the masks are read (data/dataset.py)."""
    agn: Union[bool, NonNegativeInt] = 1
    batch_size: PositiveInt = 1
    check_files: bool = False
    debug: bool = False
    comb_hr: bool = False
    crop_mode: Literal["center", "random", "boresight"] = "center"
    directory: Path
    mode: Literal["img", "agn"] = "img"
    name: str = "sim_dataset"
    scaling: Literal["linear", "sqrt", "asinh", "log"] = "sqrt"
    type: DatasetType = DatasetType.SIM
    lr: LrDatasetCfg = LrDatasetCfg()
    hr: Optional[HrDatasetCfg] = HrDatasetCfg()

    @property
    def res_mult(self) -> int:
        if self.type is DatasetType.REAL:
            return 1
        return self.hr.res // self.lr.res

    @property
    def img_dir(self) -> Path:
        return self._mode_dir(ImageType.IMG)

    @property
    def agn_dir(self) -> Path:
        return self._mode_dir(ImageType.AGN)

    @property
    def bkg_dir(self) -> Path:
        return self._mode_dir(ImageType.BKG)

    def _mode_dir(self, mode: ImageType) -> Path:
        # <directory>/<name>/{img,agn,bkg} for simulations; real data has images only, at <directory>/<name>
        if self.type is DatasetType.SIM:
            return Path(self.directory) / self.name / mode.value
        if mode is ImageType.IMG and self.type is DatasetType.REAL:
            return Path(self.directory) / self.name
        raise ConfigError(f"Something went wrong while setting {mode.value.upper()} directory for type '{self.type}': "
                          f"\tPath to {mode.value.upper()} dir has not been set!")
