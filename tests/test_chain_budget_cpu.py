"""include/ia.h ia_chain_choice without a GPU: what a level takes of the chained-wave budget
(ia_chain_budget): two-wave workgroups (option "gather_wave") with twice its waves reserved, the
one-wave launches with the single reservation, or separate launches with nothing reserved.

Widths: cfg3's finest level (1024^2: steps of at most 342 queries, padded to 352, + 1 entering
row = 353 one-wave workgroups) and a 16-job batch of 512^2 levels (2,736 per launch).  Budget: a
whole MI355X at the merge + gather kernels' one wave per SIMD, 2 x 1,024 resident waves less 1/16
= 1,920."""
import pytest

import ia_amd  # noqa: F401
from ia_amd import _native

CFG3_FINEST = 353
BATCH16_512 = 2736


@pytest.fixture(scope='module')
def budget():
    b = _native.chain_budget(256, 264, 4, 64)
    assert b == 1920
    return b


def test_budget_of_two_wave_workgroups_is_the_same_resident_waves():
    # two workgroups of two waves per CU hold the four slots four one-wave workgroups hold
    assert _native.chain_budget(256, 264, 2, 128) == _native.chain_budget(256, 264, 4, 64)


def test_doubled_reservation_fits(budget):
    assert _native.chain_choice(CFG3_FINEST, 0, budget) == 2
    # ... up to the last wave: 2 x 353 = 706 of what is left
    assert _native.chain_choice(CFG3_FINEST, budget - 2 * CFG3_FINEST, budget) == 2
    # four pipelined levels of 1024^2 .. 128^2 would all take the doubled reservation
    used = 0
    for waves in (353, 193, 97, 65):
        assert _native.chain_choice(waves, used, budget) == 2
        used += 2 * waves
    assert used <= budget


def test_only_the_single_reservation_fits(budget):
    assert _native.chain_choice(CFG3_FINEST, budget - 2 * CFG3_FINEST + 1, budget) == 1
    assert _native.chain_choice(CFG3_FINEST, budget - CFG3_FINEST, budget) == 1
    # a level that does not qualify for the two-wave form never doubles
    assert _native.chain_choice(CFG3_FINEST, 0, budget, two_wave=0) == 1
    # a level wider than half the budget: 2 x 1,000 > 1,920 >= 1,000
    assert _native.chain_choice(1000, 0, budget) == 1


def test_neither_fits(budget):
    assert _native.chain_choice(CFG3_FINEST, budget - CFG3_FINEST + 1, budget) == 0
    assert _native.chain_choice(CFG3_FINEST, budget, budget) == 0
    assert _native.chain_choice(BATCH16_512, 0, budget) == 0
    assert _native.chain_choice(BATCH16_512, 0, budget, two_wave=0) == 0


def test_budget_zero_never_chains():
    for waves in (1, CFG3_FINEST, BATCH16_512):
        for two in (0, 1):
            assert _native.chain_choice(waves, 0, 0, two) == 0
    assert _native.chain_choice(0, 0, 1920) == 0      # an empty level reserves nothing
    assert _native.chain_choice(CFG3_FINEST, -1, 1920) == 0
