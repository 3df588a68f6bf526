"""`from core import Fusionloss_grad2` (reference core/__init__.py re-exports loss.*, test_original.py:10)."""
from paif_amd.core.loss import (Fusionloss, Fusionloss2, Fusionloss3, Fusionloss4, Fusionloss6, Fusionloss_add,  # noqa: F401
                                Fusionloss_grad2, Fusionloss_grad3, NormalLoss, OhemCELoss, Sobelxy, SoftmaxFocalLoss,
                                Total_fusion_loss3)
from paif_amd.core.mix_transformer import *  # noqa: F401,F403
from paif_amd.core.segformer_head import SegFormerHead  # noqa: F401
from paif_amd.core.model_fusion_auto import WeTr  # noqa: F401
