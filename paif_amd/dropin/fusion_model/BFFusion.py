"""`from fusion_model.BFFusion import BFFR` (reference fusion_model/BFFusion.py): the MI355X-native BFFusion baseline, with the member
classes and the unused names the reference module carries."""
from paif_amd.fusion_model.bffusion import (BFFR, ConvLayer, ConvLayerLast, ConvLeakyRelu2d, DenseBlock, DenseBlock_light,  # noqa: F401
                                            FusionBlock_res, SelfAttention, Sobelxy, UpsampleReshape_eval, conv1x1, f_ConvLayer,
                                            qkv_transform)
