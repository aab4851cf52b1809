from .dlwp import DLWPModel
from .fourcastnet import FourcastnetModel
from .fourcastnet_v2 import FourcastnetV2Model
from .fuxi import FuxiModel
from .graphcast import GraphcastModel
from .pangu import PanguModel

# The reference registers pangu, fourcastnet, fourcastnet_v2, dlwp, graphcast, fuxi, fengwu
# (/root/reference/skyrim/core/models/__init__.py:9-17).  This build ships the hot paths of
# six of them (FourCastNet v1: DESIGN.md 13, DLWP: DESIGN.md 14, FuXi: DESIGN.md 15) -- every model
# of the reference's CLI list, plus fuxi, which that list omits (common.AVAILABLE_MODELS keeps the reference's list); fengwu (an ONNX
# graph only in the reference) is absent rather than stubbed.
MODELS = {
    "pangu": PanguModel,
    "fourcastnet": FourcastnetModel,
    "fourcastnet_v2": FourcastnetV2Model,
    "graphcast": GraphcastModel,
    "dlwp": DLWPModel,
    "fuxi": FuxiModel,
}
