"""Drop-in for v2/downstream/model_TVTSv2_ViT_B_16_mc.py (SSv2 multiple choice): same class name, constructor and forward contract."""
from ._common import MCBase, sim_matrix  # noqa: F401


class TVTSv2_B_16(MCBase):
    ARCH_NAME = "B_16"
