"""CPU: the oracle against the reference's own outputs on ragged sizes that are not in the other goldens
(tests/golden/gs_model_forward_ragged.npz, written by oracle/make_golden_standalone.py from the live reference import)."""
import os
import sys

import pytest
import torch

from oracle import paif_oracle as O
from paif_amd import synthetic as S
from tests.helpers import model_sd, t, maxabs

SHIMS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "shims")


@pytest.mark.parametrize("B,H,W", [(1, 40, 56), (3, 32, 72)])
def test_model_forward_live(B, H, W, golden):
    g = golden("gs_model_forward_ragged")
    f_ref, s_ref = g["fused_%dx%dx%d" % (B, H, W)], g["seg_%dx%dx%d" % (B, H, W)]
    sd = model_sd("mit_b0")          # = the reference model's formula state_dict (checked when the golden was written)
    ir, vis, _ = S.make_batch(B, H, W, start=5)
    with torch.no_grad():
        f, s = O.model_forward(t(ir), t(vis), sd, "mit_b0")
    assert f.shape == f_ref.shape and s.shape == s_ref.shape
    assert maxabs(f, f_ref) <= 1e-5
    assert maxabs(s, s_ref) <= 1e-4


def test_guided_filter_too_small_asserts_like_reference():
    # the reference's GuidedFilter is the third-party package the oracle's shim restates (oracle/shims/guided_filter_pytorch)
    sys.path.insert(0, SHIMS)
    try:
        from guided_filter_pytorch.guided_filter import GuidedFilter
    finally:
        sys.path.remove(SHIMS)

    with pytest.raises(AssertionError):
        GuidedFilter(4, 1e-3)(torch.zeros(1, 1, 9, 20), torch.zeros(1, 4, 9, 20))
