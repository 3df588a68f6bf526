"""`from fusion_model.DID import DID` (the reference keeps an empty module of this name; its class DID lives in fusion_model/AUIF.py): the
MI355X-native DIDFuse baseline.  A reference flow that constructs DID changes `from fusion_model.AUIF import DID` to this import."""
from paif_amd.fusion_model.didfuse import (AE_Decoder, AE_Encoder, Cov1, Cov2, Cov3, Cov4, Cov5, Cov6, Cov7, DID)  # noqa: F401
