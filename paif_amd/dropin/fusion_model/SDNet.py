"""`from fusion_model.SDNet import SDNet` (reference fusion_model/SDNet.py): the MI355X-native baseline."""
from paif_amd.fusion_model.sdnet import SDNet  # noqa: F401
