from .dlwp import DLWPModel
from .fengwu import FengwuModel
from .fourcastnet import FourcastnetModel
from .fourcastnet_v2 import FourcastnetV2Model
from .fuxi import FuxiModel
from .graphcast import GraphcastModel
from .pangu import PanguModel

# The reference registers pangu, fourcastnet, fourcastnet_v2, dlwp, graphcast, fuxi, fengwu
# (/root/reference/skyrim/core/models/__init__.py:9-17).  This build ships the hot paths of
# all seven (FourCastNet v1: DESIGN.md 13, DLWP: DESIGN.md 14, FuXi: DESIGN.md 15, FengWu: DESIGN.md
# 16) -- every model of the reference's CLI list, plus fuxi and fengwu, which that list omits (common.AVAILABLE_MODELS keeps the
# reference's list).
MODELS = {
    "pangu": PanguModel,
    "fourcastnet": FourcastnetModel,
    "fourcastnet_v2": FourcastnetV2Model,
    "graphcast": GraphcastModel,
    "dlwp": DLWPModel,
    "fuxi": FuxiModel,
    "fengwu": FengwuModel,
}
