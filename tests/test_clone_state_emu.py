"""A stream's carried state through smst_clone (unattached and as a pool member) and through the debug hooks, on the CPU stand-in
(tests/clone_cases.py)."""
import pytest

import clone_cases as cc


def test_split_clone_with_block_in_flight_and_two_table_rows(emu):
    cc.case_split_clone(emu, pooled=False)


def test_split_clone_of_a_pool_member(emu):
    cc.case_split_clone(emu, pooled=True)


@pytest.mark.parametrize("half_state", [False, True])
def test_debug_round_trip(emu, half_state):
    cc.case_debug_round_trip(emu, half_state)


def test_debug_hooks_check_their_ranges(emu):
    cc.case_debug_ranges(emu)
