"""The segmentation criteria by the reference's `from core import OhemCELoss` spelling; everything else is imported by module.
This makes every `paif_amd.core.*` import load `.loss`, and with it `paif_amd.ops`: `ops` must never import from `paif_amd.core`."""
from .loss import NormalLoss, OhemCELoss, SoftmaxFocalLoss  # noqa: F401
