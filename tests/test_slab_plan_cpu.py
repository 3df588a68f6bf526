"""The operand-pack plan of the slab conv (csrc/conv_slab.h: plan_for) through the host-only paif_bffusion_ops_floats(M, K, taps).

The rule written above plan_for, restated here without its arithmetic: a block is 16 output channels; up to four blocks go in ONE
group; beyond that the blocks are cut into groups of MB = 4 or MB = 3, whichever pads fewer blocks, and a tie takes 4.  The pack then
holds groups * chunks * taps * MB * 256 floats (chunks of 16 input channels).  No GPU is needed."""
import pytest

from paif_amd import _lib


def _ceil(a, b):
    return -(-a // b)


def _plan(M):
    """-> (MB, groups) by the rule in words."""
    blocks = _ceil(M, 16)
    if blocks <= 4:
        return blocks, 1
    padded = {mb: _ceil(blocks, mb) * mb - blocks for mb in (4, 3)}
    mb = 4 if padded[4] <= padded[3] else 3
    return mb, _ceil(blocks, mb)


def _floats(M, K, taps):
    mb, groups = _plan(M)
    return groups * _ceil(K, 16) * taps * mb * 256


@pytest.mark.parametrize("taps", [1, 9])
def test_ops_floats_follows_the_plan_rule(taps):
    L = _lib.load()
    bad = [(M, K) for M in range(1, 331) for K in range(1, 331) if L.paif_bffusion_ops_floats(M, K, taps) != _floats(M, K, taps)]
    assert not bad, (taps, len(bad), bad[:5])


def test_ops_floats_refuses_bad_arguments():
    L = _lib.load()
    for M, K, taps in [(0, 16, 9), (16, 0, 9), (-1, 16, 1), (16, -16, 1), (16, 16, 0), (16, 16, 3), (16, 16, 8), (16, 16, 10), (16, 16, -9)]:
        assert L.paif_bffusion_ops_floats(M, K, taps) == 0, (M, K, taps)


@pytest.mark.parametrize("M,MB,groups", [(224, 3, 5), (288, 3, 6), (192, 4, 3), (44, 3, 1)])
def test_plans_the_sources_rely_on(M, MB, groups):
    """224: DRDB's tail transposes (14 blocks: 4 pads two, 3 pads one); 288: 18 blocks, 3 pads none; 192: twelve blocks, a tie, 4 wins;
    44: U2Fusion's growth, three blocks in one group."""
    assert _plan(M) == (MB, groups)
    L = _lib.load()
    for taps in (1, 9):
        for K in (16, 44, 64):
            assert L.paif_bffusion_ops_floats(M, K, taps) == groups * _ceil(K, 16) * taps * MB * 256
    assert L.paif_bffusion_ops_floats(M, 16, 1) == groups * MB * 256
