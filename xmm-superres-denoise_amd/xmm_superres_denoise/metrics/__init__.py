from .xmm_metric_collection import (EXT_NAMES, ExtEpochState, FsimEpochState, XMMExtMetricCollection, XMMFsimCollection, XMMMetricCollection,
                                    get_ext_metrics, get_fsim_metrics, get_in_ext_metrics, get_in_fsim_metrics, get_in_metrics,
                                    get_metrics)  # noqa: F401
