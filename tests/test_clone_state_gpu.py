"""A stream's carried state through smst_clone (unattached and as a pool member) and through the debug hooks, on the GPU
(tests/clone_cases.py)."""
import pytest

import clone_cases as cc


@pytest.mark.gpu
def test_split_clone_with_block_in_flight_and_two_table_rows(hip):
    cc.case_split_clone(hip, pooled=False)


@pytest.mark.gpu
def test_split_clone_of_a_pool_member(hip):
    cc.case_split_clone(hip, pooled=True)


@pytest.mark.gpu
@pytest.mark.parametrize("half_state", [False, True])
def test_debug_round_trip(hip, half_state):
    cc.case_debug_round_trip(hip, half_state)


@pytest.mark.gpu
def test_debug_hooks_check_their_ranges(hip):
    cc.case_debug_ranges(hip)
