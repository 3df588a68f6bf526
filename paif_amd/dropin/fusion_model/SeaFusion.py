"""`from fusion_model.SeaFusion import SeaFusion` (reference fusion_model/SeaFusion.py): the MI355X-native baseline."""
from paif_amd.fusion_model.seafusion import (Conv1, ConvBnLeakyRelu2d, ConvBnTanh2d, ConvLeakyRelu2d, DenseBlock, RGBD, SeaFusion,  # noqa: F401
                                             Sobelxy)
