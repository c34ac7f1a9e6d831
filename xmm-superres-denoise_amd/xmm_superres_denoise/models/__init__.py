from .model import Model  # noqa: F401
from .modules.generator_rrdb import GeneratorRRDB_DN, GeneratorRRDB_SR  # noqa: F401
from .modules.hat import HAT  # noqa: F401
from .modules.restormer import Restormer  # noqa: F401
from .modules.swinfir import SwinFIR  # noqa: F401
from .modules.swinir import SwinIR  # noqa: F401
from .modules.swinir_train import TrainableSwinIR  # noqa: F401
from .modules.swinfir_train import TrainableSwinFIR  # noqa: F401
from .modules.hat_train import TrainableHAT  # noqa: F401
