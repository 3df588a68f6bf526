"""Competitor fusion networks of the paper's tables (reference fusion_model/*).  test_original.py:18-19 imports DID and ReCoNet:
ReCoNet is built (paif_amd/fusion_model/reconet.py, re-exported by Reconet.py), and so are SDNet (paif_amd/fusion_model/sdnet.py,
re-exported by SDNet.py), U2Fusion (paif_amd/fusion_model/u2fusion.py, re-exported by U2Fusion.py) and SeAFusion
(paif_amd/fusion_model/seafusion.py, re-exported by SeaFusion.py).  DIDFuse (class DID) is built too
(paif_amd/fusion_model/didfuse.py), re-exported by DID.py -- the reference has an empty module of that name: `from fusion_model.DID import
DID` gives the native classes.  `fusion_model.AUIF.DID`, the name the entry script imports and never constructs, still resolves to a class
that raises "out of scope" when constructed; a flow that constructs DID changes that one import line.  BFFusion (class BFFR) is built
(paif_amd/fusion_model/bffusion.py, re-exported by BFFusion.py): with it every competitor class of the reference has a native counterpart."""
