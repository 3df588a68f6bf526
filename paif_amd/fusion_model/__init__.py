"""Competitor fusion networks that run through the same composite model / attack flow as the searched network
(reference fusion_model/*).  Built: ReCoNet (reconet.py), SDNet (sdnet.py), U2Fusion (u2fusion.py), SeAFusion (seafusion.py), DIDFuse
(didfuse.py), BFFusion (bffusion.py); and the reference's own hand-designed Fusion_Network with its DRDB blocks (drdb.py).
Fusion_Network2 (skff.py), the variant with two SKFF gates and two guidance maps, is a module of its own outside that flow."""
