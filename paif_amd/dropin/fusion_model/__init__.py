"""Competitor fusion networks of the paper's tables (reference fusion_model/*).  test_original.py:18-19 imports DID and ReCoNet:
ReCoNet is built (paif_amd/fusion_model/reconet.py, re-exported by Reconet.py), and so are SDNet (paif_amd/fusion_model/sdnet.py,
re-exported by SDNet.py), U2Fusion (paif_amd/fusion_model/u2fusion.py, re-exported by U2Fusion.py) and SeAFusion
(paif_amd/fusion_model/seafusion.py, re-exported by SeaFusion.py); DID is out of scope -- the name resolves here and raises when constructed."""
