"""Drop-in for v2/downstream/model_TVTSv2_ViT_H_14_mc.py (SSv2 multiple choice): same class name, constructor and forward contract."""
from ._common import MCBase, sim_matrix  # noqa: F401


class TVTSv2_H_14(MCBase):
    ARCH_NAME = "H_14"
