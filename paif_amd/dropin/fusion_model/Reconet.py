"""`from fusion_model.Reconet import ReCoNet` (reference test_original.py:19): the MI355X-native baseline."""
from paif_amd.fusion_model.reconet import ConvGroup, DGroup, ReCoNet  # noqa: F401
