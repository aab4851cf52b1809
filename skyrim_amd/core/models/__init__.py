from .dlwp import DLWPModel
from .fourcastnet import FourcastnetModel
from .fourcastnet_v2 import FourcastnetV2Model
from .graphcast import GraphcastModel
from .pangu import PanguModel

# The reference registers pangu, fourcastnet, fourcastnet_v2, dlwp, graphcast, fuxi, fengwu
# (/root/reference/skyrim/core/models/__init__.py:9-17).  This build ships the hot paths of
# five of them (FourCastNet v1: DESIGN.md 13, DLWP: DESIGN.md 14) -- every model of the reference's
# CLI list; fuxi and fengwu (ONNX graphs only in the reference) are absent rather than stubbed.
MODELS = {
    "pangu": PanguModel,
    "fourcastnet": FourcastnetModel,
    "fourcastnet_v2": FourcastnetV2Model,
    "graphcast": GraphcastModel,
    "dlwp": DLWPModel,
}
